// Device tail of the in-training validation (evaluation.py; exp-1-debias-gender/1-main-debias.py evaluate_process :1449-1571, plot_in_grid :151-217):
// the probability table of one validation prompt is reduced to integer counts, and the annotated image grid is painted as uint8, so that
// only 32 integers and the finished grid cross to the host.  Neither kernel is on the training step's critical path.
// The offline evaluator (evaluate_images.py; eval-generated-images.py) adds the two kernels that start from JPEG-decoded uint8 HWC images: the face-chip
// crop (crop_face :296-319 on ``u/255*2-1``) and the two- / three-strip grid (plot_in_grid_gender_race :65-168, plot_in_grid_gender_race_age :171-263).
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

// PIL's rectangle outline of width 4 with both ends drawn (evaluation.grid_host states the rule): is image pixel (x, y) on it?
__device__ __forceinline__ bool eval_box_outline(int x, int y, int x0, int y0, int x1, int y1) {
    const bool hor = ((y >= y0 && y < y0 + EG_BOX) || (y <= y1 && y > y1 - EG_BOX)) && x >= x0 && x <= x1;
    const int ya = y0 + EG_BOX, yb = y1 - EG_BOX + 1;
    const int lo = ya <= yb ? ya : yb + 1, hi = ya <= yb ? yb - 1 : ya;
    const bool ver = ((x >= x0 && x < x0 + EG_BOX) || (x <= x1 && x > x1 - EG_BOX)) && y >= lo && y <= hi;
    return hor || ver;
}

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
    if (eval_box_outline(x, y, x0, y0, x1, y1)) return col;
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

// ---------------------------------------------------------------- uint8 images of the offline evaluator
// ``img.float()/255*2-1`` (eval-generated-images.py:637) as torch computes it in fp32: a true division, then a product and a difference, each rounded
// once.  The translation unit is built with -ffast-math, under which an fp32 ``u / 255.f`` is lowered to u * (1/255) whatever ``#pragma clang fp``
// says (the approximate-function flag has no pragma), and that product differs from the quotient in the last bit for part of the 256 values.  The
// quotient is therefore formed in fp64 and rounded to fp32: 1/255 = 0.(00000001) in binary, so u/255 repeats the byte u with period 8 and lies at
// least 2^-9 ulp(fp32) from every fp32 rounding boundary -- any fp64 evaluation (a division, or a reciprocal product off by a few fp64 ulp) rounds to
// the correctly rounded fp32 quotient, for all 256 values (tests/test_evalimages_cpu.py checks the statement exhaustively).
__device__ __forceinline__ float eval_u8_unit(uint32_t u) {
#pragma clang fp reassociate(off) contract(off) reciprocal(off)
    const float d = (float)((double)u / 255.0);
    const float t = d * 2.f;
    return t - 1.f;
}

// ---------------------------------------------------------------- fd_crop_resize_u8_fwd
// img [B,H,W,3] uint8 -> chips [B,3,S,S] working dtype NCHW.  One thread per output pixel, all three channels: the three bytes of a tap are adjacent
// in HWC; threads run along the output row, so each channel plane is written in full rows.
__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ boxes, float fill, f16* __restrict__ chips,
                                                             int H, int W, int S, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % S);
        const int64_t p = i / S;
        const int oy = (int)(p % S);
        const int b = (int)(p / S);
        const int x0 = boxes[b * 4], y0 = boxes[b * 4 + 1], x1 = boxes[b * 4 + 2], y1 = boxes[b * 4 + 3];
        float v[3] = {fill, fill, fill};
        if (x1 > x0 && y1 > y0) {      // an empty box (the no-face box -1,-1,-1,-1) is a chip of ``fill``
            int ya, yb, xa, xb;
            float ly, lx;
            bilinear_src(oy, y1 - y0, S, ya, yb, ly);
            bilinear_src(ox, x1 - x0, S, xa, xb, lx);
            const uint8_t* ip = img + (int64_t)b * H * W * 3;
            float tap[4][3];
            const int py[4] = {ya, ya, yb, yb}, px[4] = {xa, xb, xa, xb};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int yy = y0 + py[k], xx = x0 + px[k];
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const uint8_t* t = ip + ((int64_t)yy * W + xx) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) tap[k][c] = in ? eval_u8_unit(t[c]) : fill;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = bilinear_blend(ly, lx, tap[0][c], tap[1][c], tap[2][c], tap[3][c]);
        }
        f16* o = chips + ((int64_t)b * 3 * S + oy) * S + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(int64_t)c * S * S] = (f16)v[c];
    }
}

extern "C" int fd_crop_resize_u8_fwd(const uint8_t* img, const int32_t* boxes, float fill, void* chips, int B, int H, int W, int S, void* stream) {
    FD_REQUIRE(img && boxes && chips, "fd_crop_resize_u8_fwd: null pointer");
    FD_REQUIRE(B >= 1 && S >= 1 && S <= 4096 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096,
               "fd_crop_resize_u8_fwd: B = %d (supported >= 1), S = %d, H = %d, W = %d (supported 1..4096 each)", B, S, H, W);
    const int64_t n = (int64_t)B * S * S;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, img, boxes, fill, (f16*)chips,
                       H, W, S, n);
    return fd_check_launch("fd_crop_resize_u8_fwd");
}

// ---------------------------------------------------------------- fd_eval_grid_attrs_u8
// one output byte of the grid; ``idx`` = flat byte index into [rows*(H+20), cols*(W+50*n_attr+20), 3].  The rules (which strip, which bar) are the
// caller's: the kernel paints preds / bar_rows / palette as given.
__device__ __forceinline__ uint32_t eval_grid_attrs_byte(int64_t idx, const uint8_t* __restrict__ img, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ boxes, const int32_t* __restrict__ preds, const int32_t* __restrict__ bar_rows,
                                                         const uint8_t* __restrict__ palette, int N, int H, int W, int n_attr, int cols) {
    const int tw = W + EG_STRIP * n_attr + 2 * EG_FRAME, th = H + 2 * EG_FRAME;
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
    // strips from the outside in: an outer strip is drawn later in the reference, so its bar -- 51 columns wide, one column into whatever lies to its
    // right -- wins over the next strip's colour (or, for the last strip, over the image's first column)
    for (int s = 0; s < n_attr; ++s) {
        const int bar = bar_rows[(int64_t)s * N + i];
        if (bar >= 0 && ix >= EG_STRIP * s && ix <= EG_STRIP * s + EG_STRIP && iy <= bar) return 255u;
        if (ix < EG_STRIP * s + EG_STRIP) {
            const int cls = min(max(preds[(int64_t)s * N + i], -1), FD_EVAL_PALETTE - 2);
            return palette[(s * FD_EVAL_PALETTE + cls + 1) * 3 + c];
        }
    }
    const int x = ix - EG_STRIP * n_attr, y = iy;
    if (eval_box_outline(x, y, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3])) return 0u;      // the outline is black here
    float v;
    {
        // ``ToPILImage()(img*0.5+0.5)`` on img = u/255*2-1: four fp32 roundings (quotient, difference, sum, product; the factors 2 and 0.5 are exact),
        // then truncation -- 63 of the 256 byte values come out one lower than they went in
#pragma clang fp reassociate(off) contract(off)
        const float h = eval_u8_unit(img[(((int64_t)i * H + y) * W + x) * 3 + c]) * 0.5f;
        const float w = h + 0.5f;
        v = w * 255.f;
    }
    return (uint32_t)(int)v;      // in [0, 255] for every byte value
}

__global__ __launch_bounds__(256) void eval_grid_attrs_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ order, const int32_t* __restrict__ boxes,
                                                              const int32_t* __restrict__ preds, const int32_t* __restrict__ bar_rows,
                                                              const uint8_t* __restrict__ palette, uint8_t* __restrict__ grid, int N, int H, int W, int n_attr, int cols,
                                                              int64_t total) {
    // 4 consecutive bytes per thread and one 32-bit store, the last 1..3 bytes one by one: as eval_grid_kernel
    const int64_t nquad = (total + 3) / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q * 4;
        if (b + 4 <= total) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= eval_grid_attrs_byte(b + j, img, order, boxes, preds, bar_rows, palette, N, H, W, n_attr, cols) << (8 * j);
            *reinterpret_cast<uint32_t*>(grid + b) = w;
        } else {
            for (int64_t k = b; k < total; ++k) grid[k] = (uint8_t)eval_grid_attrs_byte(k, img, order, boxes, preds, bar_rows, palette, N, H, W, n_attr, cols);
        }
    }
}

extern "C" int fd_eval_grid_attrs_u8(const uint8_t* images, const int32_t* order, const int32_t* boxes, const int32_t* preds, const int32_t* bar_rows,
                                     const uint8_t* palette, uint8_t* grid, int N, int H, int W, int n_attr, int rows, int cols, void* stream) {
    FD_REQUIRE(images && order && boxes && preds && bar_rows && palette && grid, "fd_eval_grid_attrs_u8: null pointer");
    FD_REQUIRE(N >= 1 && N <= 4096 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "fd_eval_grid_attrs_u8: N = %d, H = %d, W = %d, supported 1..4096 each", N, H, W);
    FD_REQUIRE(n_attr >= 1 && n_attr <= FD_EVAL_MAX_ATTR, "fd_eval_grid_attrs_u8: n_attr = %d, supported 1..%d", n_attr, FD_EVAL_MAX_ATTR);
    FD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols >= N && (int64_t)rows * cols < (int64_t)N + cols,
               "fd_eval_grid_attrs_u8: a %d x %d grid does not hold %d tiles with a partly filled last row at most", rows, cols, N);
    FD_REQUIRE(((uintptr_t)grid & 3) == 0, "fd_eval_grid_attrs_u8: the grid buffer must be 4-byte aligned");
    const int64_t total = (int64_t)rows * (H + 2 * EG_FRAME) * cols * (W + EG_STRIP * n_attr + 2 * EG_FRAME) * 3;
    FD_REQUIRE(total < ((int64_t)1 << 40), "fd_eval_grid_attrs_u8: a grid of %lld bytes is not supported", (long long)total);
    const int64_t nquad = (total + 3) / 4;
    const int64_t blocks = (nquad + 255) / 256;
    hipLaunchKernelGGL(eval_grid_attrs_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, images, order, boxes, preds, bar_rows,
                       palette, grid, N, H, W, n_attr, cols, total);
    return fd_check_launch("fd_eval_grid_attrs_u8");
}
