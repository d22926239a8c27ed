// LoRA weight gradients: skinny "TN" reductions over the token dimension.
//   G[n, r] += scale * sum_m X[m, n] * T[m, r]        (X,T fp16; G fp32 with arbitrary strides)
// dUp[N,r]  = dY^T . t   (X = dY, T = t = x.down^T)        dDown[r,K] = u^T . x  (X = x, T = u = dY.up)
// HBM-bound (reads X once); VALU FMAs, coalesced over n, T rows broadcast.  Two-pass with a fixed
// reduction order so repeated runs are bit-identical.  Batched problems of ranks 17..64 run on the matrix cores instead
// (lora_wgrad_partial_mfma_multi below).
#include "common.h"

template <int RP>
__global__ __launch_bounds__(256) void lora_wgrad_partial(const f16* __restrict__ X, int64_t ldx, const f16* __restrict__ T, int64_t ldt,
                                                          float* __restrict__ partial, int M, int N, int rows_per_split) {
    __shared__ float red[3][64][RP + 1];
    const int nl = threadIdx.x & 63, mg = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + nl;
    const int m0 = blockIdx.y * rows_per_split;
    const int m1 = min(m0 + rows_per_split, M);
    float acc[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) acc[r] = 0.f;
    if (n < N) {
        for (int m = m0 + mg; m < m1; m += 4) {
            const float x = (float)X[(int64_t)m * ldx + n];
            const f16* tr = T + (int64_t)m * ldt;
#pragma unroll
            for (int r8 = 0; r8 < RP; r8 += 8) {
                const f16x8 tv = *(const f16x8*)(tr + r8);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r8 + j] += x * (float)tv[j];
            }
        }
    }
    if (mg > 0) {
#pragma unroll
        for (int r = 0; r < RP; ++r) red[mg - 1][nl][r] = acc[r];
    }
    __syncthreads();
    if (mg == 0 && n < N) {
#pragma unroll
        for (int r = 0; r < RP; ++r) {
            const float v = acc[r] + red[0][nl][r] + red[1][nl][r] + red[2][nl][r];
            partial[((int64_t)blockIdx.y * N + n) * RP + r] = v;
        }
    }
}

// Vectorised variant for small ranks: a thread owns CV consecutive columns (16-byte loads of X for CV = 8) and one row phase; a block
// covers CGB column groups x RT = 256 / CGB row phases (CGB = 40: 320 columns, the U-Net's channel granule).  The RT partial sums are
// combined through LDS in a fixed order.  Reads X at full line width instead of 2 bytes per lane.
template <int RP, int CV, int CGB>
__device__ __forceinline__ void lora_wgrad_partial_vec_body(const f16* __restrict__ X, int64_t ldx, const f16* __restrict__ T, int64_t ldt,
                                                            float* __restrict__ partial, int M, int N, int rows_per_split, int bx, int by,
                                                            float* red) {
    constexpr int RT = 256 / CGB;
    const int cgl = threadIdx.x % CGB, rt = threadIdx.x / CGB;
    const int n0 = (bx * CGB + cgl) * CV;
    const int m0 = by * rows_per_split;
    const int m1 = min(m0 + rows_per_split, M);
    float acc[CV][RP];
#pragma unroll
    for (int c = 0; c < CV; ++c)
#pragma unroll
        for (int r = 0; r < RP; ++r) acc[c][r] = 0.f;
    const bool active = rt < RT && n0 < N;      // N % CV == 0 is required by the launcher
    if (active) {
        constexpr int U = 4;                       // rows in flight per thread: the loop is latency-bound without this
        for (int m = m0 + rt; m < m1; m += U * RT) {
            f16 xv[U][CV];
            f16x8 tv[U][RP / 8];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int mm = m + u * RT;
                const bool ok = mm < m1;
                const int64_t mc = ok ? mm : m;   // clamp: the duplicate row is multiplied by zero below
                if (CV == 8) *(f16x8*)xv[u] = *(const f16x8*)(X + mc * ldx + n0);
                else if (CV == 4) *(f16x4*)xv[u] = *(const f16x4*)(X + mc * ldx + n0);
                else
#pragma unroll
                    for (int c = 0; c < CV; ++c) xv[u][c] = X[mc * ldx + n0 + c];
#pragma unroll
                for (int r8 = 0; r8 < RP / 8; ++r8) tv[u][r8] = *(const f16x8*)(T + mc * ldt + r8 * 8);
                if (!ok)
#pragma unroll
                    for (int c = 0; c < CV; ++c) xv[u][c] = (f16)0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float tf[RP];
#pragma unroll
                for (int r = 0; r < RP; ++r) tf[r] = (float)tv[u][r >> 3][r & 7];
#pragma unroll
                for (int c = 0; c < CV; ++c) {
                    const float x = (float)xv[u][c];
#pragma unroll
                    for (int r = 0; r < RP; ++r) acc[c][r] += x * tf[r];
                }
            }
        }
    }
    if (rt > 0 && rt < RT) {
        float* dst = red + ((rt - 1) * CGB + cgl) * (CV * RP + 1);
#pragma unroll
        for (int c = 0; c < CV; ++c)
#pragma unroll
            for (int r = 0; r < RP; ++r) dst[c * RP + r] = acc[c][r];
    }
    __syncthreads();
    if (rt == 0 && n0 < N) {
#pragma unroll
        for (int c = 0; c < CV; ++c)
#pragma unroll
            for (int r = 0; r < RP; ++r) {
                float v = acc[c][r];
#pragma unroll
                for (int k = 0; k < RT - 1; ++k) v += red[(k * CGB + cgl) * (CV * RP + 1) + c * RP + r];
                partial[((int64_t)by * N + n0 + c) * RP + r] = v;
            }
    }
}

template <int RP, int CV, int CGB>
__global__ __launch_bounds__(256) void lora_wgrad_partial_vec(const f16* __restrict__ X, int64_t ldx, const f16* __restrict__ T, int64_t ldt,
                                                              float* __restrict__ partial, int M, int N, int rows_per_split) {
    __shared__ float red[(256 / CGB - 1) * CGB * (CV * RP + 1)];
    lora_wgrad_partial_vec_body<RP, CV, CGB>(X, ldx, T, ldt, partial, M, N, rows_per_split, blockIdx.x, blockIdx.y, red);
}

// ---- batched form: up to FD_WGRAD_MAX independent problems (the 16 LoRA weight gradients of one transformer block's backward) in ONE partial
// launch and ONE final launch.  7808 + 7808 launches of ~10 + 7 us per training step were 3.7 % of it; the problems are far too small to fill the
// chip one at a time.  Same arithmetic and the same fixed reduction order per problem as the single-problem kernels.
struct WgradBatch {
    const f16* X[FD_WGRAD_MAX];
    const f16* T[FD_WGRAD_MAX];
    float* G[FD_WGRAD_MAX];
    int64_t ldx[FD_WGRAD_MAX], ldt[FD_WGRAD_MAX], sn[FD_WGRAD_MAX], sr[FD_WGRAD_MAX], poff[FD_WGRAD_MAX];
    int M[FD_WGRAD_MAX], N[FD_WGRAD_MAX], R[FD_WGRAD_MAX], rows[FD_WGRAD_MAX], ncb[FD_WGRAD_MAX], nsplit[FD_WGRAD_MAX];
    float scale[FD_WGRAD_MAX];
    int bstart[FD_WGRAD_MAX + 1];      // first block of each problem in the partial launch
    int ostart[FD_WGRAD_MAX + 1];      // first output element (n, r) of each problem in the final launch
    int n;
};

template <int RP, int CV, int CGB>
__global__ __launch_bounds__(256) void lora_wgrad_partial_multi(WgradBatch b, float* __restrict__ scratch) {
    FD_WG_TRACE(18);
    __shared__ float red[(256 / CGB - 1) * CGB * (CV * RP + 1)];
    int p = 0;
#pragma unroll 1
    while (p + 1 < b.n && (int)blockIdx.x >= b.bstart[p + 1]) ++p;
    const int local = blockIdx.x - b.bstart[p];
    const int bx = local % b.ncb[p], by = local / b.ncb[p];
    lora_wgrad_partial_vec_body<RP, CV, CGB>(b.X[p], b.ldx[p], b.T[p], b.ldt[p], scratch + b.poff[p], b.M[p], b.N[p], b.rows[p], bx, by, red);
}

// ---- padded ranks 32 and 64 on the matrix cores.  G^T[r, n] = sum_m T[m, r] X[m, n] is a product whose contraction index is the ROW index of both
// operands, so both are staged row-major, as they lie in HBM, and their 16x16x32 fragments are read column-wise with ds_read_b64_tr_b16: a 16-lane
// group g fetches the blocks [4 rows 4g ..][16 columns] and [4 rows 16 + 4g ..][16 columns] of a 32-row stage, lane i supplies the address of row
// i / 4, columns 4 (i % 4) .. + 3 and receives column i.  A and B take the same k order, so its permutation against the plain operand map cancels.
// A block of 4 waves owns WG_NC = 320 columns x RP ranks of one row range: wave w the columns 80 w .. + 79 as 5 x RP / 16 accumulator tiles, so X is
// read from HBM once and T once per 320 columns.  Row strides of 672 B (X) and 160 / 96 B (T) are odd multiples of 32 B: the 8 rows x 32 B that
// a 32-lane half reads together fall on 8 distinct 32-byte slots of the 256-byte bank row.  Rows past the range are zero in LDS; columns past N
// are zero too and their results are dropped.  No branch around a transposed read depends on the lane (EXEC is all ones there).
typedef short fd_s16x4 __attribute__((__vector_size__(8)));
constexpr int WG_KT = 32, WG_NC = 320, WG_XS = WG_NC + 16;

__device__ __forceinline__ f16x8 wgrad_read_tr(const f16* tile, int stride, int c0, int lane) {
    const f16* p = tile + (4 * (lane >> 4) + ((lane & 15) >> 2)) * stride + c0 + 4 * (lane & 3);
    const fd_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fd_s16x4*)p);
    const fd_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fd_s16x4*)(p + 16 * stride));
    const f16x4 a = __builtin_bit_cast(f16x4, lo), b = __builtin_bit_cast(f16x4, hi);
    return (f16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <int RP>
__global__ __launch_bounds__(256) void lora_wgrad_partial_mfma_multi(WgradBatch b, float* __restrict__ scratch) {
    FD_WG_TRACE(21);
    constexpr int TS = RP + 16, NRT = RP / 16, TCH = RP / 8, XCH = WG_NC / 8, XPT = WG_KT * XCH / 256;
    static_assert(WG_KT * XCH % 256 == 0 && WG_KT * TCH <= 256, "staging shares of 256 threads");
    __shared__ __attribute__((aligned(16))) f16 Xs[WG_KT * WG_XS];
    __shared__ __attribute__((aligned(16))) f16 Ts[WG_KT * TS];
    int p = 0;
#pragma unroll 1
    while (p + 1 < b.n && (int)blockIdx.x >= b.bstart[p + 1]) ++p;
    const int local = blockIdx.x - b.bstart[p];
    const int bx = local % b.ncb[p], by = local / b.ncb[p];
    const f16* __restrict__ X = b.X[p];
    const f16* __restrict__ T = b.T[p];
    const int64_t ldx = b.ldx[p], ldt = b.ldt[p];
    const int N = b.N[p], n0 = bx * WG_NC;
    const int m0 = by * b.rows[p], m1 = min(m0 + b.rows[p], b.M[p]);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    f32x4 acc[5][NRT];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < NRT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // one stage = 32 rows: 1280 16-byte pieces of X (5 per thread) and 32 * RP / 8 of T (at most one per thread), held in registers across the
    // MFMAs of the stage before
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 xr[XPT], tr = zero8;
    auto load = [&](int mk) {
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int c = tid + 256 * i, m = mk + c / XCH, col = n0 + (c % XCH) * 8;
            xr[i] = (m < m1 && col < N) ? *(const f16x8*)(X + (int64_t)m * ldx + col) : zero8;      // N % 8 == 0: a piece is inside or outside
        }
        if (tid < WG_KT * TCH) {
            const int m = mk + tid / TCH;
            tr = m < m1 ? *(const f16x8*)(T + (int64_t)m * ldt + (tid % TCH) * 8) : zero8;
        }
    };
    load(m0);
    for (int mk = m0; mk < m1; mk += WG_KT) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int c = tid + 256 * i;
            *(f16x8*)(Xs + (c / XCH) * WG_XS + (c % XCH) * 8) = xr[i];
        }
        if (tid < WG_KT * TCH) *(f16x8*)(Ts + (tid / TCH) * TS + (tid % TCH) * 8) = tr;
        __syncthreads();
        if (mk + WG_KT < m1) load(mk + WG_KT);
        f16x8 tf[NRT];
#pragma unroll
        for (int j = 0; j < NRT; ++j) tf[j] = wgrad_read_tr(Ts, TS, j * 16, lane);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const f16x8 xf = wgrad_read_tr(Xs, WG_XS, wave * 80 + i * 16, lane);
#pragma unroll
            for (int j = 0; j < NRT; ++j) acc[i][j] = FD_MFMA_16x16x32(tf[j], xf, acc[i][j]);
        }
    }
    // C/D map: column (lane & 15) = n, rows 4 (lane >> 4) .. + 3 = four consecutive ranks
    float* partial = scratch + b.poff[p];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int n = n0 + wave * 80 + i * 16 + (lane & 15);
        if (n < N) {
#pragma unroll
            for (int j = 0; j < NRT; ++j) *(f32x4*)(partial + ((int64_t)by * N + n) * RP + j * 16 + 4 * (lane >> 4)) = acc[i][j];
        }
    }
}

// Final pass of the MFMA arm: one THREAD per (n, padded r), consecutive threads on consecutive floats of a partial row, the splits added in ascending
// order.  (lora_wgrad_final_multi spends a wave per output element: fine for 320 x 4 outputs, 400 us for the 16 x 1280 x 50 of a rank-50 block.)
// Here ``ostart`` counts N x RP elements per problem.
template <int RP>
__global__ __launch_bounds__(256) void lora_wgrad_final_mfma_multi(WgradBatch b, const float* __restrict__ scratch) {
    FD_WG_TRACE(22);
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= b.ostart[b.n]) return;
    int p = 0;
#pragma unroll 1
    while (p + 1 < b.n && o >= b.ostart[p + 1]) ++p;
    const int lo = o - b.ostart[p];
    const int n = lo / RP, r = lo % RP;
    if (r >= b.R[p]) return;
    const int64_t step = (int64_t)b.N[p] * RP;
    const float* src = scratch + b.poff[p] + lo;
    float s = 0.f;
    const int ns = b.nsplit[p];
    int k = 0;
    for (; k + 4 <= ns; k += 4) {
        const float v0 = src[k * step], v1 = src[(k + 1) * step], v2 = src[(k + 2) * step], v3 = src[(k + 3) * step];
        s = (((s + v0) + v1) + v2) + v3;
    }
    for (; k < ns; ++k) s += src[k * step];
    b.G[p][n * b.sn[p] + r * b.sr[p]] += b.scale[p] * s;
}

__global__ __launch_bounds__(256) void lora_wgrad_final_multi(WgradBatch b, const float* __restrict__ scratch, int RP) {
    FD_WG_TRACE(19);
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= b.ostart[b.n]) return;
    int p = 0;
#pragma unroll 1
    while (p + 1 < b.n && o >= b.ostart[p + 1]) ++p;
    const int lo = o - b.ostart[p];
    const int lane = threadIdx.x & 63;
    const int R = b.R[p], N = b.N[p];
    const int n = lo / R, r = lo % R;
    const float* partial = scratch + b.poff[p];
    float s = 0.f;
    for (int k = lane; k < b.nsplit[p]; k += 64) s += partial[((int64_t)k * N + n) * RP + r];
    s = wave_sum(s);
    if (lane == 0) b.G[p][n * b.sn[p] + r * b.sr[p]] += b.scale[p] * s;
}

// one wave per output element (n, r): lanes stride over the splits in a fixed order, then a fixed-shape wave reduction
__global__ __launch_bounds__(256) void lora_wgrad_final(const float* partial, float* G, int64_t sn, int64_t sr, int N, int R, int RP, int nsplit,
                                                        float scale) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= N * R) return;
    const int lane = threadIdx.x & 63;
    const int n = o / R, r = o % R;
    float s = 0.f;
    for (int k = lane; k < nsplit; k += 64) s += partial[((int64_t)k * N + n) * RP + r];
    s = wave_sum(s);
    if (lane == 0) G[n * sn + r * sr] += scale * s;
}

extern "C" int fd_lora_wgrad(const void* X, int64_t ldx, const void* T, int64_t ldt, float* G, int64_t g_stride_n, int64_t g_stride_r, int M,
                             int N, int R, float scale, float* scratch, int64_t scratch_elems, void* stream) {
    FD_REQUIRE(M > 0 && N > 0 && R > 0 && R <= 64, "fd_lora_wgrad: rank must be in 1..64 (got %d)", R);
    const int RP = R <= 8 ? 8 : (R <= 16 ? 16 : (R <= 32 ? 32 : 64));
    FD_REQUIRE(ldt >= RP && (ldt & 7) == 0, "fd_lora_wgrad: T must be padded to %d columns (ldt=%ld)", RP, (long)ldt);
    // small ranks: vectorised kernel, 320 columns per block; otherwise 64 columns per block
    const bool vec = (RP == 8 && (N & 7) == 0 && (ldx & 7) == 0) || (RP == 16 && (N & 3) == 0 && (ldx & 3) == 0);
    const int cols_per_block = vec ? (RP == 8 ? 320 : 160) : 64;
    const int ncb = (N + cols_per_block - 1) / cols_per_block;
    int nsplit = (768 + ncb - 1) / ncb;
    if (nsplit > (M + 63) / 64) nsplit = (M + 63) / 64;
    while (nsplit > 1 && (int64_t)nsplit * N * RP > scratch_elems) nsplit >>= 1;
    FD_REQUIRE((int64_t)nsplit * N * RP <= scratch_elems, "fd_lora_wgrad: scratch too small");
    int rows = (M + nsplit - 1) / nsplit;
    rows = vec ? (rows + 5) / 6 * 6 : (rows + 3) & ~3;
    nsplit = (M + rows - 1) / rows;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(ncb, nsplit);
    switch (vec ? -RP : RP) {
        case -8: hipLaunchKernelGGL((lora_wgrad_partial_vec<8, 8, 40>), grid, dim3(256), 0, s, (const f16*)X, ldx, (const f16*)T, ldt, scratch, M, N, rows); break;
        case -16: hipLaunchKernelGGL((lora_wgrad_partial_vec<16, 4, 40>), grid, dim3(256), 0, s, (const f16*)X, ldx, (const f16*)T, ldt, scratch, M, N, rows); break;
        case 8: hipLaunchKernelGGL(lora_wgrad_partial<8>, grid, dim3(256), 0, s, (const f16*)X, ldx, (const f16*)T, ldt, scratch, M, N, rows); break;
        case 16: hipLaunchKernelGGL(lora_wgrad_partial<16>, grid, dim3(256), 0, s, (const f16*)X, ldx, (const f16*)T, ldt, scratch, M, N, rows); break;
        case 32: hipLaunchKernelGGL(lora_wgrad_partial<32>, grid, dim3(256), 0, s, (const f16*)X, ldx, (const f16*)T, ldt, scratch, M, N, rows); break;
        default: hipLaunchKernelGGL(lora_wgrad_partial<64>, grid, dim3(256), 0, s, (const f16*)X, ldx, (const f16*)T, ldt, scratch, M, N, rows); break;
    }
    hipLaunchKernelGGL(lora_wgrad_final, dim3((N * R + 3) / 4), dim3(256), 0, s, scratch, G, g_stride_n, g_stride_r, N, R, RP, nsplit, scale);
    return fd_check_launch("fd_lora_wgrad");
}

// The RP = 32 / 64 arm of fd_lora_wgrad_multi (the descriptors' sizes, ranks and counts are already checked).  Splits: about 2 blocks per CU (what the RP = 64 kernel's 172 registers admit) over the
// whole batch, shared out by work, at least 256 rows each (a split writes and the final pass re-reads N x RP floats: at 256 rows that is as many
// bytes as the split's X rows, beyond it mostly overhead); halved together until the partials fit the scratch that was passed.
static int lora_wgrad_multi_mfma(const fd_wgrad_desc* descs, int n, int RP, float* scratch, int64_t scratch_elems, hipStream_t s) {
    double work = 0;
    for (int i = 0; i < n; ++i) {
        const fd_wgrad_desc& d = descs[i];
        FD_REQUIRE((d.N & 7) == 0, "fd_lora_wgrad_multi: N must be a multiple of 8 for ranks above 16 (problem %d: N=%d)", i, d.N);
        FD_REQUIRE((d.ldx & 7) == 0 && d.ldx >= d.N, "fd_lora_wgrad_multi: ldx must be a multiple of 8 and >= N for ranks above 16 (problem %d: ldx=%ld)", i, (long)d.ldx);
        FD_REQUIRE(d.ldt >= RP && (d.ldt & 7) == 0, "fd_lora_wgrad_multi: ldt must be a multiple of 8 and >= %d (problem %d: ldt=%ld)", RP, i, (long)d.ldt);
        FD_REQUIRE(d.X && ((uintptr_t)d.X & 15) == 0, "fd_lora_wgrad_multi: X must be 16-byte aligned for ranks above 16 (problem %d)", i);
        FD_REQUIRE(d.T && ((uintptr_t)d.T & 15) == 0, "fd_lora_wgrad_multi: T must be 16-byte aligned for ranks above 16 (problem %d)", i);
        FD_REQUIRE(d.G, "fd_lora_wgrad_multi: G is null (problem %d)", i);
        FD_REQUIRE(d.N <= (1 << 20), "fd_lora_wgrad_multi: N must be at most 2^20 for ranks above 16 (problem %d: N=%d)", i, d.N);
        work += (double)d.M * d.N;
    }
    WgradBatch b;
    b.n = n;
    int blocks = 0, outs = 0;
    int64_t poff = 0;
    for (int div = 1;; div <<= 1) {
        blocks = 0; outs = 0; poff = 0;
        bool split = false;
        for (int i = 0; i < n; ++i) {
            const fd_wgrad_desc& d = descs[i];
            const int ncb = (d.N + WG_NC - 1) / WG_NC;
            int nsplit = (int)(512.0 * ((double)d.M * d.N / work) / ncb + 0.5);
            if (nsplit > (d.M + 255) / 256) nsplit = (d.M + 255) / 256;
            nsplit /= div;
            if (nsplit < 1) nsplit = 1;
            int rows = (d.M + nsplit - 1) / nsplit;
            rows = (rows + WG_KT - 1) / WG_KT * WG_KT;
            nsplit = (d.M + rows - 1) / rows;
            split |= nsplit > 1;
            b.X[i] = (const f16*)d.X; b.T[i] = (const f16*)d.T; b.G[i] = d.G;
            b.ldx[i] = d.ldx; b.ldt[i] = d.ldt; b.sn[i] = d.g_stride_n; b.sr[i] = d.g_stride_r; b.poff[i] = poff;
            b.M[i] = d.M; b.N[i] = d.N; b.R[i] = d.R; b.rows[i] = rows; b.ncb[i] = ncb; b.nsplit[i] = nsplit; b.scale[i] = d.scale;
            b.bstart[i] = blocks; b.ostart[i] = outs;
            blocks += ncb * nsplit;
            outs += d.N * RP;                      // the final pass of this arm walks whole partial rows
            poff += (int64_t)nsplit * d.N * RP;
        }
        if (poff <= scratch_elems || !split) break;
    }
    b.bstart[n] = blocks; b.ostart[n] = outs;
    FD_REQUIRE(scratch && poff <= scratch_elems, "fd_lora_wgrad_multi: scratch too small (%ld > %ld floats)", (long)poff, (long)scratch_elems);
    if (RP == 32) hipLaunchKernelGGL(lora_wgrad_partial_mfma_multi<32>, dim3(blocks), dim3(256), 0, s, b, scratch);
    else hipLaunchKernelGGL(lora_wgrad_partial_mfma_multi<64>, dim3(blocks), dim3(256), 0, s, b, scratch);
    if (RP == 32) hipLaunchKernelGGL(lora_wgrad_final_mfma_multi<32>, dim3((outs + 255) / 256), dim3(256), 0, s, b, (const float*)scratch);
    else hipLaunchKernelGGL(lora_wgrad_final_mfma_multi<64>, dim3((outs + 255) / 256), dim3(256), 0, s, b, (const float*)scratch);
    return fd_check_launch("fd_lora_wgrad_multi");
}

// Batched weight gradients: ``descs`` is a HOST array of n <= FD_WGRAD_MAX problems that share the padded rank RP (8, 16, 32 or 64).  RP 8 and 16
// run the vectorised kernel and need its alignment (N %% CV == 0, ldx %% CV == 0 with CV = 8 / 4); RP 32 and 64 run the MFMA kernel and need
// N %% 8 == 0, ldx %% 8 == 0 and 16-byte aligned X and T; anything else is rejected (callers fall back to fd_lora_wgrad).
extern "C" int fd_lora_wgrad_multi(const fd_wgrad_desc* descs, int n, float* scratch, int64_t scratch_elems, void* stream) {
    FD_REQUIRE(n >= 1 && n <= FD_WGRAD_MAX, "fd_lora_wgrad_multi: 1..%d problems (got %d)", FD_WGRAD_MAX, n);
    FD_REQUIRE_DESC(descs, fd_wgrad_desc, "fd_lora_wgrad_multi");       // element 0 first: its size is the array stride of the others
    for (int i = 1; i < n; ++i) FD_REQUIRE_DESC(descs + i, fd_wgrad_desc, "fd_lora_wgrad_multi");
    WgradBatch b;
    b.n = n;
    int RP = 0;
    double work = 0;
    for (int i = 0; i < n; ++i) {
        const fd_wgrad_desc& d = descs[i];
        FD_REQUIRE(d.M > 0 && d.N > 0 && d.R > 0 && d.R <= 64, "fd_lora_wgrad_multi: rank must be in 1..64 (problem %d: R=%d)", i, d.R);
        const int rp = d.R <= 8 ? 8 : (d.R <= 16 ? 16 : (d.R <= 32 ? 32 : 64));
        FD_REQUIRE(RP == 0 || rp == RP, "fd_lora_wgrad_multi: mixed padded ranks");
        RP = rp;
    }
    if (RP >= 32) return lora_wgrad_multi_mfma(descs, n, RP, scratch, scratch_elems, (hipStream_t)stream);
    for (int i = 0; i < n; ++i) {
        const fd_wgrad_desc& d = descs[i];
        const int cv = RP == 8 ? 8 : 4;
        FD_REQUIRE((d.N % cv) == 0 && (d.ldx % cv) == 0 && d.ldt >= RP && (d.ldt & 7) == 0, "fd_lora_wgrad_multi: alignment (N, ldx %% %d; ldt)", cv);
        work += (double)d.M * d.N;
    }
    const int cols_per_block = RP == 8 ? 320 : 160;
    int64_t poff = 0;
    int blocks = 0, outs = 0;
    for (int i = 0; i < n; ++i) {
        const fd_wgrad_desc& d = descs[i];
        const int ncb = (d.N + cols_per_block - 1) / cols_per_block;
        // ~1536 blocks over the whole batch, shared out by work; at least 64 rows per split
        int nsplit = (int)(1536.0 * ((double)d.M * d.N / work) / ncb + 0.5);
        if (nsplit < 1) nsplit = 1;
        if (nsplit > (d.M + 63) / 64) nsplit = (d.M + 63) / 64;
        int rows = (d.M + nsplit - 1) / nsplit;
        rows = (rows + 5) / 6 * 6;
        nsplit = (d.M + rows - 1) / rows;
        b.X[i] = (const f16*)d.X; b.T[i] = (const f16*)d.T; b.G[i] = d.G;
        b.ldx[i] = d.ldx; b.ldt[i] = d.ldt; b.sn[i] = d.g_stride_n; b.sr[i] = d.g_stride_r; b.poff[i] = poff;
        b.M[i] = d.M; b.N[i] = d.N; b.R[i] = d.R; b.rows[i] = rows; b.ncb[i] = ncb; b.nsplit[i] = nsplit; b.scale[i] = d.scale;
        b.bstart[i] = blocks; b.ostart[i] = outs;
        blocks += ncb * nsplit;
        outs += d.N * d.R;
        poff += (int64_t)nsplit * d.N * RP;
    }
    b.bstart[n] = blocks; b.ostart[n] = outs;
    FD_REQUIRE(poff <= scratch_elems, "fd_lora_wgrad_multi: scratch too small (%ld > %ld floats)", (long)poff, (long)scratch_elems);
    hipStream_t s = (hipStream_t)stream;
    if (RP == 8) hipLaunchKernelGGL((lora_wgrad_partial_multi<8, 8, 40>), dim3(blocks), dim3(256), 0, s, b, scratch);
    else hipLaunchKernelGGL((lora_wgrad_partial_multi<16, 4, 40>), dim3(blocks), dim3(256), 0, s, b, scratch);
    hipLaunchKernelGGL(lora_wgrad_final_multi, dim3((outs + 3) / 4), dim3(256), 0, s, b, (const float*)scratch, RP);
    return fd_check_launch("fd_lora_wgrad_multi");
}


// ------------------------------------------------------------------ 16-bit operand copies of LoRA pairs after an optimiser step
// 128 pairs x (zeros, two slice copies, two transposes) were ~1000 tiny torch launches per step (10 ms of host-bound time); here 16 pairs per launch.
#define FD_REFRESH_MAX 16
struct RefreshBatch { fd_lora_refresh_desc d[FD_REFRESH_MAX]; int n; };

__global__ void lora_refresh_kernel(RefreshBatch b) {
    const fd_lora_refresh_desc& p = b.d[blockIdx.y];
    const int nd = p.rp * p.K, nu = p.N * p.rp;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nd + nu; i += gridDim.x * blockDim.x) {
        if (i < nd) {
            const int j = i / p.K, k = i - j * p.K;
            const f16 v = (f16)(j < p.r ? p.down[(int64_t)j * p.K + k] : 0.f);
            ((f16*)p.d16)[(int64_t)j * p.ld_d16 + k] = v;
            ((f16*)p.dT16)[(int64_t)k * p.ld_dT16 + j] = v;
        } else {
            const int e = i - nd;
            const int n = e / p.rp, j = e - n * p.rp;
            const f16 v = (f16)(j < p.r ? p.up[(int64_t)n * p.r + j] * p.scale : 0.f);
            ((f16*)p.u16)[(int64_t)n * p.ld_u16 + j] = v;
            ((f16*)p.uT16)[(int64_t)j * p.ld_uT16 + n] = v;
        }
    }
}

extern "C" int fd_lora_refresh_multi(const fd_lora_refresh_desc* descs, int n, void* stream) {
    FD_REQUIRE(descs && n > 0, "fd_lora_refresh_multi: no pairs");
    for (int i = 0; i < n; ++i) FD_REQUIRE_DESC(descs + i, fd_lora_refresh_desc, "fd_lora_refresh_multi");
    for (int i0 = 0; i0 < n; i0 += FD_REFRESH_MAX) {
        RefreshBatch b;
        b.n = n - i0 < FD_REFRESH_MAX ? n - i0 : FD_REFRESH_MAX;
        int64_t most = 0;
        for (int i = 0; i < b.n; ++i) {
            b.d[i] = descs[i0 + i];
            const fd_lora_refresh_desc& p = b.d[i];
            FD_REQUIRE(p.down && p.up && p.d16 && p.dT16 && p.u16 && p.uT16 && p.r > 0 && p.rp >= p.r && p.K > 0 && p.N > 0, "fd_lora_refresh_multi: bad pair %d", i0 + i);
            const int64_t e = (int64_t)p.rp * (p.K + p.N);
            most = e > most ? e : most;
        }
        int bx = (int)((most + 255) / 256);
        if (bx > 64) bx = 64;
        hipLaunchKernelGGL(lora_refresh_kernel, dim3(bx, b.n), dim3(256), 0, (hipStream_t)stream, b);
    }
    return fd_check_launch("fd_lora_refresh_multi");
}


// ------------------------------------------------------------------ folding LoRA pairs into their base weights (fd_lora_merge_multi; header for the contract)
// out[n, k] = base[n, k] + scale * sum_j up[n, j] * down[j, k], all fp32, j ascending in one fma chain per element: plain VALU, no atomics, no MFMA, so
// the bits depend on the inputs alone.  One workgroup of 256 threads per 32 x 64 tile of out: the tile's 32 rows of up (contiguous in memory) and its
// 64 columns of down are staged in LDS once (25 KB), lane c of wave g then owns column c of the rows 8g .. 8g + 7 -- the down value is one LDS read per j
// shared by eight fmas; the up tile is kept TRANSPOSED ([j][row], row stride 36 floats: 16-byte aligned rows, and the 32 consecutive j of a coalesced
// staging read land on 16 banks instead of one), so the eight up values of a j are two 16-byte wave-wide broadcast reads (one 4-byte read each made the
// loop LDS-issue-bound: 9 LDS reads per 8 fmas).  base is read once and out written once, a 256-byte row segment per wave and row; every GLOBAL access is
// a 4-byte one, because down and up are views into a flat bank of which only that alignment is known.
#define FD_MERGE_MAX 16
#define FD_MERGE_TN 32
#define FD_MERGE_TK 64
#define FD_MERGE_RMAX 64
#define FD_MERGE_UP_LD 36
struct MergeBatch { fd_lora_merge_desc d[FD_MERGE_MAX]; int tstart[FD_MERGE_MAX + 1]; int n; };

__global__ __launch_bounds__(256) void lora_merge_kernel(MergeBatch b) {
    __shared__ __attribute__((aligned(16))) float s_up[FD_MERGE_RMAX * FD_MERGE_UP_LD];
    __shared__ float s_dn[FD_MERGE_RMAX * FD_MERGE_TK];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.tstart[i + 1]) ++i;
    const fd_lora_merge_desc& p = b.d[i];
    const int t = (int)blockIdx.x - b.tstart[i];
    const int tk = (p.K + FD_MERGE_TK - 1) / FD_MERGE_TK;
    const int n0 = (t / tk) * FD_MERGE_TN, k0 = (t % tk) * FD_MERGE_TK;
    const int r = p.r;
    const int rows = p.N - n0 < FD_MERGE_TN ? p.N - n0 : FD_MERGE_TN;
    const float* up = p.up + (int64_t)n0 * r;
    for (int e = threadIdx.x; e < FD_MERGE_TN * r; e += 256) {
        const int row = e / r, j = e - row * r;
        s_up[j * FD_MERGE_UP_LD + row] = e < rows * r ? up[e] : 0.f;
    }
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int k = k0 + c;
    for (int j = g; j < r; j += 4) s_dn[j * FD_MERGE_TK + c] = k < p.K ? p.down[(int64_t)j * p.K + k] : 0.f;
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    for (int j = 0; j < r; ++j) {
        const float d = s_dn[j * FD_MERGE_TK + c];
        const float4 u0 = *(const float4*)(s_up + j * FD_MERGE_UP_LD + g * 8), u1 = *(const float4*)(s_up + j * FD_MERGE_UP_LD + g * 8 + 4);
        acc[0] = fmaf(u0.x, d, acc[0]); acc[1] = fmaf(u0.y, d, acc[1]); acc[2] = fmaf(u0.z, d, acc[2]); acc[3] = fmaf(u0.w, d, acc[3]);
        acc[4] = fmaf(u1.x, d, acc[4]); acc[5] = fmaf(u1.y, d, acc[5]); acc[6] = fmaf(u1.z, d, acc[6]); acc[7] = fmaf(u1.w, d, acc[7]);
    }
    if (k >= p.K) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = n0 + g * 8 + q;
        if (n < p.N) {
            const int64_t at = (int64_t)n * p.K + k;
            p.out[at] = fmaf(p.scale, acc[q], p.base[at]);      // the same thread reads base[at] and writes out[at]: out == base is safe
        }
    }
}

static inline bool merge_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    return na > 0 && nb > 0 && (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na);
}

extern "C" int fd_lora_merge_multi(const fd_lora_merge_desc* descs, int n, void* stream) {
    FD_REQUIRE(descs && n > 0, "fd_lora_merge_multi: no pairs");
    for (int i = 0; i < n; ++i) FD_REQUIRE_DESC(descs + i, fd_lora_merge_desc, "fd_lora_merge_multi");
    // everything is refused here, before the first launch
    for (int i = 0; i < n; ++i) {
        const fd_lora_merge_desc& p = descs[i];
        FD_REQUIRE(p.down && p.up && p.base && p.out, "fd_lora_merge_multi: null down, up, base or out (pair %d)", i);
        FD_REQUIRE((((uintptr_t)p.down | (uintptr_t)p.up | (uintptr_t)p.base | (uintptr_t)p.out) & 3) == 0, "fd_lora_merge_multi: a pointer of pair %d is not aligned to 4 bytes", i);
        FD_REQUIRE(p.r >= 1 && p.r <= FD_MERGE_RMAX, "fd_lora_merge_multi: rank must be in 1..64 (pair %d: r = %d)", i, p.r);
        FD_REQUIRE(p.N >= 0 && p.K >= 0 && p.N <= 0x7fffff00 && p.K <= 0x7fffff00, "fd_lora_merge_multi: negative or oversized extent (pair %d: N = %d, K = %d)", i, p.N, p.K);
    }
    for (int i = 0; i < n; ++i) {
        const fd_lora_merge_desc& p = descs[i];
        const int64_t no = (int64_t)p.N * p.K;
        for (int j = 0; j < n; ++j) {
            const fd_lora_merge_desc& q = descs[j];
            const int64_t nq = (int64_t)q.N * q.K;
            const bool in_place = i == j && p.out == p.base;
            FD_REQUIRE(in_place || !merge_overlap(p.out, no, q.base, nq), "fd_lora_merge_multi: out of pair %d overlaps base of pair %d (only out == base of one pair is allowed)", i, j);
            FD_REQUIRE(i == j || !merge_overlap(p.out, no, q.out, nq), "fd_lora_merge_multi: out of pair %d overlaps out of pair %d", i, j);
            FD_REQUIRE(!merge_overlap(p.out, no, q.down, (int64_t)q.r * q.K) && !merge_overlap(p.out, no, q.up, (int64_t)q.N * q.r),
                       "fd_lora_merge_multi: out of pair %d overlaps down or up of pair %d", i, j);
        }
    }
    for (int i0 = 0; i0 < n; i0 += FD_MERGE_MAX) {
        int64_t tiles = 0;
        for (int i = i0; i < n && i < i0 + FD_MERGE_MAX; ++i)
            tiles += (int64_t)((descs[i].N + FD_MERGE_TN - 1) / FD_MERGE_TN) * ((descs[i].K + FD_MERGE_TK - 1) / FD_MERGE_TK);
        FD_REQUIRE(tiles <= 0x7fffffff, "fd_lora_merge_multi: pairs %d.. hold %lld tiles of 32 x 64 (one launch takes 2^31 - 1)", i0, (long long)tiles);
    }
    for (int i0 = 0; i0 < n; i0 += FD_MERGE_MAX) {
        MergeBatch b;
        b.n = n - i0 < FD_MERGE_MAX ? n - i0 : FD_MERGE_MAX;
        int tiles = 0;
        for (int i = 0; i < FD_MERGE_MAX; ++i) {
            b.d[i] = descs[i0 + (i < b.n ? i : 0)];
            b.tstart[i] = tiles;
            if (i < b.n) tiles += ((b.d[i].N + FD_MERGE_TN - 1) / FD_MERGE_TN) * ((b.d[i].K + FD_MERGE_TK - 1) / FD_MERGE_TK);
        }
        b.tstart[FD_MERGE_MAX] = tiles;
        if (tiles > 0) hipLaunchKernelGGL(lora_merge_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, b);
    }
    return fd_check_launch("fd_lora_merge_multi");
}

FD_WGT_SETTER(lora)
