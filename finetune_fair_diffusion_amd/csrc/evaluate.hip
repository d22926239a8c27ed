// Device tail of the in-training validation (evaluation.py; exp-1-debias-gender/1-main-debias.py evaluate_process :1449-1571, plot_in_grid :151-217):
// the probability table of one validation prompt is reduced to integer counts, and the annotated image grid is painted as uint8, so that
// only 32 integers and the finished grid cross to the host.  Neither kernel is on the training step's critical path.
#include "common.h"
#include "../../include/fairdiff_hip.h"

// ---------------------------------------------------------------- fd_eval_tally
// One block: the counts are integers accumulated with LDS atomics, so the result is exact and independent of the order.  Thresholds are the
// fp32 values of the literals 0.2 / 0.5 / 0.8 (what torch compares a float32 tensor with; pinned by tests/golden/reference_eval_metrics.json).
struct EvalAttrs {
    int c0[FD_EVAL_MAX_ATTR];
    int k[FD_EVAL_MAX_ATTR];
};

__global__ __launch_bounds__(256) void eval_tally_kernel(const float* __restrict__ probs, int N, int ld, EvalAttrs at, int n_attr, int32_t* __restrict__ counts) {
    __shared__ int acc[FD_EVAL_COUNTS];
    if (threadIdx.x < FD_EVAL_COUNTS) acc[threadIdx.x] = 0;
    __syncthreads();
    for (int row = threadIdx.x; row < N; row += blockDim.x) {
        const float* p = probs + (int64_t)row * ld;
        int pred[FD_EVAL_MAX_ATTR];
        bool valid[FD_EVAL_MAX_ATTR];
        for (int a = 0; a < n_attr; ++a) {
            const int k = at.k[a];
            bool ok = true;
            int best = 0;
            float mx = p[at.c0[a]];
            for (int j = 0; j < k; ++j) {
                const float v = p[at.c0[a] + j];
                ok = ok && (v != -1.f);
                if (v > mx) {      // strict: the first maximum wins
                    mx = v;
                    best = j;
                }
            }
            valid[a] = ok;
            pred[a] = best;
            if (!ok) continue;
            atomicAdd(&acc[FD_EVAL_ATTR_STRIDE * a], 1);
            atomicAdd(&acc[FD_EVAL_ATTR_STRIDE * a + 1 + best], 1);
            if (mx < 0.8f) atomicAdd(&acc[FD_EVAL_ATTR_STRIDE * a + 5], 1);
        }
        if (at.k[0] == 2 && valid[0]) {
            const float p1 = p[at.c0[0] + 1];
            if (p1 >= 0.5f && p1 <= 1.f) atomicAdd(&acc[FD_EVAL_OFF_P1_HI], 1);
            if (p1 >= 0.f && p1 <= 0.5f) atomicAdd(&acc[FD_EVAL_OFF_P1_LO], 1);
            if (p1 >= 0.2f && p1 <= 0.8f) atomicAdd(&acc[FD_EVAL_OFF_P1_MID], 1);
            if (n_attr >= 2 && valid[1]) {
                atomicAdd(&acc[FD_EVAL_OFF_JOINT + 4 * pred[0] + pred[1]], 1);
                atomicAdd(&acc[FD_EVAL_OFF_JOINT_VALID], 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < FD_EVAL_COUNTS) counts[threadIdx.x] = acc[threadIdx.x];      // every entry is written: no zeroing by the caller
}

extern "C" int fd_eval_tally(const float* probs, int N, int ld, const int32_t* attr_c0, const int32_t* attr_k, int n_attr, int32_t* counts, void* stream) {
    FD_REQUIRE(probs && attr_c0 && attr_k && counts, "fd_eval_tally: null pointer");
    FD_REQUIRE(N >= 0 && N <= (1 << 20), "fd_eval_tally: N = %d, supported 0..2^20", N);
    FD_REQUIRE(n_attr >= 1 && n_attr <= FD_EVAL_MAX_ATTR, "fd_eval_tally: n_attr = %d, supported 1..%d", n_attr, FD_EVAL_MAX_ATTR);
    EvalAttrs at = {};
    for (int a = 0; a < n_attr; ++a) {      // attr_c0 / attr_k are HOST arrays
        FD_REQUIRE(attr_k[a] >= 1 && attr_k[a] <= FD_EVAL_MAX_K, "fd_eval_tally: attribute %d has k = %d, supported 1..%d", a, attr_k[a], FD_EVAL_MAX_K);
        FD_REQUIRE(attr_c0[a] >= 0 && attr_c0[a] + attr_k[a] <= ld, "fd_eval_tally: attribute %d covers columns %d..%d of a table with ld = %d", a, attr_c0[a],
                   attr_c0[a] + attr_k[a] - 1, ld);
        at.c0[a] = attr_c0[a];
        at.k[a] = attr_k[a];
    }
    hipLaunchKernelGGL(eval_tally_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, probs, N, ld, at, n_attr, counts);
    return fd_check_launch("fd_eval_tally");
}

// ---------------------------------------------------------------- fd_eval_grid_u8
#define EG_STRIP 50
#define EG_FRAME 10
#define EG_BOX 4

// one output byte of the grid; ``idx`` = flat byte index into [rows*(H+20), cols*(W+70), 3]
__device__ __forceinline__ uint32_t eval_grid_byte(int64_t idx, const f16* __restrict__ img, const int32_t* __restrict__ order, const int32_t* __restrict__ boxes,
                                                   const int32_t* __restrict__ preds, const float* __restrict__ maxprob, const uint8_t* __restrict__ palette,
                                                   int N, int H, int W, int cols) {
    const int tw = W + EG_STRIP + 2 * EG_FRAME, th = H + 2 * EG_FRAME;
    const int c = (int)(idx % 3);
    const int64_t pxl = idx / 3;
    const int GW = cols * tw;
    const int X = (int)(pxl % GW), Y = (int)(pxl / GW);
    const int tc = X / tw, tx = X - tc * tw, tr = Y / th, ty = Y - tr * th;
    const int t = tr * cols + tc;
    if (t >= N) return 255u;                                                                     // tiles past N are white
    if (tx < EG_FRAME || tx >= tw - EG_FRAME || ty < EG_FRAME || ty >= th - EG_FRAME) return 0u;  // black frame
    const int ix = tx - EG_FRAME, iy = ty - EG_FRAME;
    const int i = order[t];
    if (i < 0 || i >= N) return 255u;                                                            // a malformed order entry reads nothing
    const float p = maxprob[i];
    // the white bar covers columns 0..50 of the strip-expanded image (the image's first column included) and rows 0..int((1-p)*512), computed in
    // double from the fp32 value as the reference does with ``.item()``
    if (p < 1.f && ix <= EG_STRIP && iy <= (int)((1.0 - (double)p) * 512.0)) return 255u;
    const int cls = min(max(preds[i], -1), FD_EVAL_PALETTE - 2);
    const uint32_t col = palette[(cls + 1) * 3 + c];
    if (ix < EG_STRIP) return col;
    const int x = ix - EG_STRIP, y = iy;
    const int x0 = boxes[4 * i], y0 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], y1 = boxes[4 * i + 3];
    // PIL's rectangle outline of width 4 (evaluation.grid_host states the rule)
    const bool hor = ((y >= y0 && y < y0 + EG_BOX) || (y <= y1 && y > y1 - EG_BOX)) && x >= x0 && x <= x1;
    const int ya = y0 + EG_BOX, yb = y1 - EG_BOX + 1;
    const int lo = ya <= yb ? ya : yb + 1, hi = ya <= yb ? yb - 1 : ya;
    const bool ver = ((x >= x0 && x < x0 + EG_BOX) || (x <= x1 && x > x1 - EG_BOX)) && y >= lo && y <= hi;
    if (hor || ver) return col;
    float v;
    {
        // generate.to_uint8_hwc: (x * 0.5 + 0.5) in fp32, then * 255, then truncation -- the sum and the product must each round once (no
        // x * 127.5 + 127.5).  The compiler may still fuse x * 0.5 + 0.5 into one fma: x * 0.5 is exact for a 16-bit input, so the result is the same
#pragma clang fp reassociate(off) contract(off)
        const float u = (float)img[(((int64_t)i * 3 + c) * H + y) * W + x] * 0.5f + 0.5f;
        v = u * 255.f;
    }
    v = fminf(fmaxf(v, 0.f), 255.f);      // images are in [-1,1] by contract; a value outside must not make the conversion undefined
    return (uint32_t)(int)v;
}

__global__ __launch_bounds__(256) void eval_grid_kernel(const f16* __restrict__ img, const int32_t* __restrict__ order, const int32_t* __restrict__ boxes,
                                                        const int32_t* __restrict__ preds, const float* __restrict__ maxprob, const uint8_t* __restrict__ palette,
                                                        uint8_t* __restrict__ grid, int N, int H, int W, int cols, int64_t total) {
    // each thread produces 4 consecutive bytes and writes them with one 32-bit store (the buffer start is 4-byte aligned, checked by the entry point);
    // the last 1..3 bytes of a grid whose size is not a multiple of 4 are written one by one
    const int64_t nquad = (total + 3) / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q * 4;
        if (b + 4 <= total) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= eval_grid_byte(b + j, img, order, boxes, preds, maxprob, palette, N, H, W, cols) << (8 * j);
            *reinterpret_cast<uint32_t*>(grid + b) = w;
        } else {
            for (int64_t k = b; k < total; ++k) grid[k] = (uint8_t)eval_grid_byte(k, img, order, boxes, preds, maxprob, palette, N, H, W, cols);
        }
    }
}

extern "C" int fd_eval_grid_u8(const void* images, const int32_t* order, const int32_t* boxes, const int32_t* preds, const float* maxprob, const uint8_t* palette,
                               uint8_t* grid, int N, int H, int W, int rows, int cols, void* stream) {
    FD_REQUIRE(images && order && boxes && preds && maxprob && palette && grid, "fd_eval_grid_u8: null pointer");
    FD_REQUIRE(N >= 1 && N <= 4096 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "fd_eval_grid_u8: N = %d, H = %d, W = %d, supported 1..4096 each", N, H, W);
    FD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols >= N && (int64_t)rows * cols < (int64_t)N + cols,
               "fd_eval_grid_u8: a %d x %d grid does not hold %d tiles with a partly filled last row at most", rows, cols, N);
    FD_REQUIRE(((uintptr_t)grid & 3) == 0, "fd_eval_grid_u8: the grid buffer must be 4-byte aligned");
    const int64_t total = (int64_t)rows * (H + 2 * EG_FRAME) * cols * (W + EG_STRIP + 2 * EG_FRAME) * 3;
    FD_REQUIRE(total < ((int64_t)1 << 40), "fd_eval_grid_u8: a grid of %lld bytes is not supported", (long long)total);
    const int64_t nquad = (total + 3) / 4;
    const int64_t blocks = (nquad + 255) / 256;
    hipLaunchKernelGGL(eval_grid_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (const f16*)images, order, boxes, preds,
                       maxprob, palette, grid, N, H, W, cols, total);
    return fd_check_launch("fd_eval_grid_u8");
}
