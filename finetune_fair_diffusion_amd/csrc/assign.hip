// Device solver for the Monte-Carlo optimal-transport targets of the multi-attribute experiments (exp-3-debias-gender-race/
// 1-main-debias.py:1488-1536, exp-4 :1517-1569): for each of S draws of balanced cell counts the reference calls
// ``ot.emd(ones(N), counts, M)`` -- N unit-mass faces onto K cells with integer capacities that sum to N.  With unit sources and integer
// sinks the LP has an integral optimum, i.e. it is a linear assignment problem on the capacity-replicated cost matrix (column j stands
// for one seat of cell cell[j]).
//
// One 64-lane wave solves one draw with the shortest-augmenting-path (Hungarian, Jonker-Volgenant potentials) algorithm in fp64: rows
// are inserted one at a time; every step of the path search is a lane-parallel relaxation of the column slack ``minv`` and a wave-wide
// argmin.  All per-column state lives in LDS (N <= 1024 seats), the cost matrix (N x K doubles) is read through the cache.  The S
// draws are independent workgroups; a face's seat is added into the summed plan with a float atomic (integer-valued sums <= S: exact
// and order-independent).  Latency-bound by design (S = 100 waves on 256 CUs, ~N^2 dependent steps each): it exists to take the solve
// off the host, not to fill the chip.
//
// exp-6 (``fd_ot_expected_targets``) runs the same solver once per kept composition of N faces into the four race classes, without a plan
// (seats only), and reduces the seats to the weighted expected plan, its argmax and 1 - max on the device.
#include "common.h"

namespace {

struct ArgMin {
    double v;
    int j;
};

__device__ __forceinline__ ArgMin wave_argmin(ArgMin a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(a.v, o, 64);
        const int oj = __shfl_xor(a.j, o, 64);
        if (ov < a.v || (ov == a.v && oj < a.j)) {
            a.v = ov;
            a.j = oj;
        }
    }
    return a;
}

__global__ __launch_bounds__(64) void ot_assign_kernel(const double* __restrict__ cost, const int* __restrict__ counts, float* plan,
                                                       int* seats /* [S,N] cell of face i in draw s, or null */, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sh_raw[];
    const int n1 = N + 1;
    double* u = (double*)sh_raw;          // row potentials, 1-based
    double* v = u + n1;                   // seat potentials, 1-based (0 = the virtual start column)
    double* minv = v + n1;
    int* p = (int*)(minv + n1);           // p[j] = row seated at j (0 = free)
    int* way = p + n1;
    int* cell = way + n1;                 // cell of seat j
    int* used = cell + n1;
    const int lane = threadIdx.x;
    const int* cnt = counts + (size_t)blockIdx.x * K;
    const double INF = 1e300;

    for (int j = lane; j <= N; j += 64) {
        u[j] = 0.0;
        v[j] = 0.0;
        p[j] = 0;
        way[j] = 0;
        int c = 0, acc = 0;
        if (j >= 1) {
            for (int k = 0; k < K; ++k) {     // seat j (1-based) belongs to the first cell whose cumulative capacity reaches j
                acc += cnt[k];
                if (j <= acc) {
                    c = k;
                    break;
                }
            }
        }
        cell[j] = c;
    }
    __syncthreads();

    for (int i = 1; i <= N; ++i) {
        for (int j = lane; j <= N; j += 64) {
            minv[j] = INF;
            used[j] = 0;
        }
        if (lane == 0) p[0] = i;
        __syncthreads();
        int j0 = 0;
        while (true) {
            if (lane == 0) used[j0] = 1;
            __syncthreads();
            const int i0 = p[j0];
            const double ui = u[i0];
            const double* crow = cost + (size_t)(i0 - 1) * K;
            ArgMin best = {INF, 0x7fffffff};
            for (int j = lane + 1; j <= N; j += 64) {
                if (used[j]) continue;
                const double cur = crow[cell[j]] - ui - v[j];
                double mv = minv[j];
                if (cur < mv) {
                    mv = cur;
                    minv[j] = cur;
                    way[j] = j0;
                }
                if (mv < best.v) {      // strict: the first minimal seat of this lane; lanes are merged towards the smaller index
                    best.v = mv;
                    best.j = j;
                }
            }
            best = wave_argmin(best);
            const double delta = best.v;
            const int j1 = best.j;
            __syncthreads();
            for (int j = lane; j <= N; j += 64) {
                if (used[j]) {
                    u[p[j]] += delta;       // seated rows are distinct: no two lanes touch one u
                    v[j] -= delta;
                } else {
                    minv[j] -= delta;
                }
            }
            __syncthreads();
            j0 = j1;
            if (p[j0] == 0) break;
        }
        if (lane == 0) {                    // flip the alternating path back to the virtual column
            int jj = j0;
            while (jj) {
                const int jp = way[jj];
                p[jj] = p[jp];
                jj = jp;
            }
        }
        __syncthreads();
    }
    for (int j = lane + 1; j <= N; j += 64) {
        const int row = p[j] - 1;
        if (plan) atomicAdd(plan + (size_t)row * K + cell[j], 1.0f);
        if (seats) seats[(size_t)blockIdx.x * N + row] = cell[j];
    }
}

// IEEE round-to-nearest x / y.  The library builds with -ffast-math, under which ``x / y`` becomes a reciprocal-and-refine sequence that can
// differ from the host in the last bit; this is the sequence the compiler emits for an exact fp64 division (scale, reciprocal, two Newton
// steps, remainder, fmas, fixup), written with the intrinsics so that no fast-math rewrite applies.
__device__ __forceinline__ double div_rn(double x, double y) {
    bool unused;
    const double ds = __builtin_amdgcn_div_scale(x, y, false, &unused);      // scaled denominator
    const double r0 = __builtin_amdgcn_rcp(ds);
    const double e0 = __builtin_fma(-ds, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-ds, r1, 1.0);
    bool scaled;
    const double ns = __builtin_amdgcn_div_scale(x, y, true, &scaled);       // scaled numerator
    const double r2 = __builtin_fma(r1, e1, r1);
    const double q = ns * r2;
    const double rem = __builtin_fma(-ds, q, ns);
    return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(rem, r2, q, scaled), y, x);
}

// exp-6's expected transport plan (exp-6-debias-race/1-main-debias.py:1414-1483): ``target_probs += T_s * w_s`` over the kept compositions s in
// table order, row L1 normalisation, first argmax, 1 - max.  One thread per face with its K <= 16 fp64 cell sums in registers; the seats of
// composition s are read as one coalesced row of [S, N].  T_s is 0/1, so ``if (seat == k) acc[k] += w_s`` is the host's ``T * w`` sum bit for
// bit; the row sum is sequential over the cells like numpy's 4-wide ``norm(ord=1)``.  No atomics: the result does not depend on scheduling.
__global__ __launch_bounds__(1024) void ot_weighted_targets_kernel(const int* __restrict__ seats, const double* __restrict__ weights, int* targets,
                                                                   double* uncertainty, int N, int K, int S) {
#pragma clang fp reassociate(off) contract(off)     // the library builds with -ffast-math: keep the host's operation order
    const int i = threadIdx.x;
    if (i >= N) return;
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    for (int s = 0; s < S; ++s) {
        const int seat = seats[(size_t)s * N + i];
        const double w = weights[s];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (seat == k) acc[k] += w;
    }
    double l1 = acc[0];
#pragma unroll
    for (int k = 1; k < 16; ++k)
        if (k < K) l1 += acc[k];
    int best = 0;
    double pmax = div_rn(acc[0], l1);
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        if (k < K) {
            const double pk = div_rn(acc[k], l1);
            if (pk > pmax) {      // strict: the first maximal cell, like argmax
                pmax = pk;
                best = k;
            }
        }
    }
    targets[i] = best;
    uncertainty[i] = 1.0 - pmax;
}

}  // namespace

extern "C" int fd_ot_assign_sum(const double* cost, const int32_t* counts, float* plan, int32_t* seats, int N, int K, int S, void* stream) {
    FD_REQUIRE(N >= 1 && N <= 1024 && K >= 1 && K <= 4096 && S >= 1, "fd_ot_assign_sum: N=%d (1..1024) K=%d S=%d", N, K, S);
    const size_t lds = (size_t)(N + 1) * (3 * sizeof(double) + 4 * sizeof(int));
    hipLaunchKernelGGL(ot_assign_kernel, dim3(S), dim3(64), lds, (hipStream_t)stream, cost, (const int*)counts, plan, (int*)seats, N, K);
    return fd_check_launch("fd_ot_assign_sum");
}

extern "C" int fd_ot_expected_targets(const double* cost, const int32_t* counts, const double* weights, int32_t* seats, int32_t* targets,
                                      double* uncertainty, int N, int K, int S, void* stream) {
    FD_REQUIRE(N >= 1 && N <= 1024 && K >= 1 && K <= 16 && S >= 1, "fd_ot_expected_targets: N=%d (1..1024) K=%d (1..16) S=%d (>= 1)", N, K, S);
    FD_REQUIRE(cost && counts && weights && seats && targets && uncertainty, "fd_ot_expected_targets: null buffer");
    const size_t lds = (size_t)(N + 1) * (3 * sizeof(double) + 4 * sizeof(int));
    hipLaunchKernelGGL(ot_assign_kernel, dim3(S), dim3(64), lds, (hipStream_t)stream, cost, (const int*)counts, (float*)nullptr, (int*)seats, N, K);
    const int rc = fd_check_launch("fd_ot_expected_targets (assignment)");
    if (rc) return rc;
    hipLaunchKernelGGL(ot_weighted_targets_kernel, dim3(1), dim3((N + 63) / 64 * 64), 0, (hipStream_t)stream, (const int*)seats, weights, (int*)targets,
                       uncertainty, N, K, S);
    return fd_check_launch("fd_ot_expected_targets (reduction)");
}
