// Device tail of the in-training validation (evaluation.py; exp-1-debias-gender/1-main-debias.py evaluate_process :1449-1571, plot_in_grid :151-217):
// the probability table of one validation prompt is reduced to integer counts, and the annotated image grid is painted as uint8, so that
// only 32 integers and the finished grid cross to the host.  Neither kernel is on the training step's critical path.
// The offline evaluator (evaluate_images.py; eval-generated-images.py) adds the kernels that start from JPEG-decoded uint8 HWC images: the face-chip
// crop (crop_face :296-319 on ``u/255*2-1``), the aligned face chip (image_pipeline :321-341) and the two- / three-strip grid (plot_in_grid_gender_race :65-168, plot_in_grid_gender_race_age :171-263).
// The training monitor (step.py; exp-3 1-main-debias.py :1989-2002, :2063-2075, exp-4 :2088, :2176) paints the same two- / three-strip grid from the
// working-dtype NCHW images the step holds.  The three painters share one tile geometry, outline, strip / bar rule, pixel rule and thread mapping
// (the helpers below); they differ in the pixel fetch, and the one-strip painter in the colour of its outline and the form its bar arrives in.
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

// ---------------------------------------------------------------- the grid painters: shared device helpers
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

// Tile geometry of a grid [rows*(H+20), cols*(W+50*n_strip+20), 3] at flat byte index ``idx``.  Returns the byte of what lies outside a tile's inner
// area -- 255 for a tile past N (white) or one whose order entry is malformed (it reads nothing), 0 for the 10-pixel black frame -- or -1 with
// ``p`` = the channel, the image shown and the position inside the strip-expanded image.
struct EvalTilePos {
    int c, i, ix, iy;
};
__device__ __forceinline__ int eval_tile_locate(int64_t idx, const int32_t* __restrict__ order, int N, int H, int W, int n_strip, int cols, EvalTilePos& p) {
    const int tw = W + EG_STRIP * n_strip + 2 * EG_FRAME, th = H + 2 * EG_FRAME;
    p.c = (int)(idx % 3);
    const int64_t pxl = idx / 3;
    const int GW = cols * tw;
    const int X = (int)(pxl % GW), Y = (int)(pxl / GW);
    const int tc = X / tw, tx = X - tc * tw, tr = Y / th, ty = Y - tr * th;
    const int t = tr * cols + tc;
    if (t >= N) return 255;
    if (tx < EG_FRAME || tx >= tw - EG_FRAME || ty < EG_FRAME || ty >= th - EG_FRAME) return 0;
    p.ix = tx - EG_FRAME;
    p.iy = ty - EG_FRAME;
    p.i = order[t];
    if (p.i < 0 || p.i >= N) return 255;
    return -1;
}

// Strip s (counted from the outside in) at position (ix, iy) of the strip-expanded image; ``bar`` = last row of its white bar, -1 = no bar.  The bar is
// 51 columns wide -- one column into whatever lies to its right: the next strip's colour or, for the last strip, the image's first column -- and an
// outer strip is drawn later in the reference, so the caller asks the strips in the order s = 0, 1, ... and the first answer other than EG_RIGHT wins.
enum { EG_RIGHT = 0, EG_BAR = 1, EG_COLOUR = 2 };
__device__ __forceinline__ int eval_strip(int ix, int iy, int s, int bar) {
    if (bar >= 0 && ix >= EG_STRIP * s && ix <= EG_STRIP * s + EG_STRIP && iy <= bar) return EG_BAR;
    return ix < EG_STRIP * s + EG_STRIP ? EG_COLOUR : EG_RIGHT;
}

__device__ __forceinline__ uint32_t eval_palette(const uint8_t* __restrict__ palette, int s, int pred, int c) {
    const int cls = min(max(pred, -1), FD_EVAL_PALETTE - 2);
    return palette[(s * FD_EVAL_PALETTE + cls + 1) * 3 + c];
}

// ``ToPILImage()(x*0.5+0.5)`` (generate.to_uint8_hwc): the sum and the product in fp32, each rounded once (no x * 127.5 + 127.5; x * 0.5 is exact),
// then truncation.  Images are in [-1,1] by contract; a value outside must not make the conversion undefined.
__device__ __forceinline__ uint32_t eval_pixel_byte(float x) {
    float v;
    {
#pragma clang fp reassociate(off) contract(off)
        const float h = x * 0.5f;
        const float u = h + 0.5f;
        v = u * 255.f;
    }
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (uint32_t)(int)v;
}

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


// The pixel fetch, the one thing the painters do not share: channel c of pixel (x, y) of image i as the fp32 value the reference's tensor holds there.
// Working dtype NCHW: the stored value.  uint8 HWC: ``u/255*2-1``, so that the painted byte carries four fp32 roundings (quotient, difference, sum,
// product) and 63 of the 256 byte values come out one lower than they went in.
__device__ __forceinline__ float eval_fetch(const f16* __restrict__ img, int i, int c, int y, int x, int H, int W) {
    return (float)img[(((int64_t)i * 3 + c) * H + y) * W + x];
}
__device__ __forceinline__ float eval_fetch(const uint8_t* __restrict__ img, int i, int c, int y, int x, int H, int W) {
    return eval_u8_unit(img[(((int64_t)i * H + y) * W + x) * 3 + c]);
}

// Thread mapping of the painters: each thread produces 4 consecutive bytes and writes them with one 32-bit store (the buffer start is 4-byte aligned,
// checked by the entry points); the last 1..3 bytes of a grid whose size is not a multiple of 4 are written one by one.
template <typename ByteFn>
__device__ __forceinline__ void eval_grid_store(uint8_t* __restrict__ grid, int64_t total, ByteFn byte) {
    const int64_t nquad = (total + 3) / 4;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = q * 4;
        if (b + 4 <= total) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= byte(b + j) << (8 * j);
            *reinterpret_cast<uint32_t*>(grid + b) = w;
        } else {
            for (int64_t k = b; k < total; ++k) grid[k] = (uint8_t)byte(k);
        }
    }
}

// ---------------------------------------------------------------- fd_eval_grid_u8
// one output byte of the grid; ``idx`` = flat byte index into [rows*(H+20), cols*(W+70), 3]
__device__ __forceinline__ uint32_t eval_grid_byte(int64_t idx, const f16* __restrict__ img, const int32_t* __restrict__ order, const int32_t* __restrict__ boxes,
                                                   const int32_t* __restrict__ preds, const float* __restrict__ maxprob, const uint8_t* __restrict__ palette,
                                                   int N, int H, int W, int cols) {
    EvalTilePos p;
    const int outside = eval_tile_locate(idx, order, N, H, W, 1, cols, p);
    if (outside >= 0) return (uint32_t)outside;
    const int i = p.i;
    // the white bar ends at row int((1-p)*512), computed in double from the fp32 value as the reference does with ``.item()``
    const float pr = maxprob[i];
    const int hit = eval_strip(p.ix, p.iy, 0, pr < 1.f ? (int)((1.0 - (double)pr) * 512.0) : -1);
    if (hit == EG_BAR) return 255u;
    const uint32_t col = eval_palette(palette, 0, preds[i], p.c);
    if (hit == EG_COLOUR) return col;
    const int x = p.ix - EG_STRIP, y = p.iy;
    if (eval_box_outline(x, y, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3])) return col;      // the outline has the class colour here
    return eval_pixel_byte(eval_fetch(img, i, p.c, y, x, H, W));
}

__global__ __launch_bounds__(256) void eval_grid_kernel(const f16* __restrict__ img, const int32_t* __restrict__ order, const int32_t* __restrict__ boxes,
                                                        const int32_t* __restrict__ preds, const float* __restrict__ maxprob, const uint8_t* __restrict__ palette,
                                                        uint8_t* __restrict__ grid, int N, int H, int W, int cols, int64_t total) {
    eval_grid_store(grid, total, [=](int64_t k) { return eval_grid_byte(k, img, order, boxes, preds, maxprob, palette, N, H, W, cols); });
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
    hipLaunchKernelGGL(eval_grid_kernel, fd_grid_1d((total + 3) / 4, 65536), dim3(256), 0, (hipStream_t)stream, (const f16*)images, order, boxes, preds, maxprob, palette,
                       grid, N, H, W, cols, total);
    return fd_check_launch("fd_eval_grid_u8");
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
    hipLaunchKernelGGL(crop_resize_u8_kernel, fd_grid_1d(n, 65536), dim3(256), 0, (hipStream_t)stream, img, boxes, fill, (f16*)chips,
                       H, W, S, n);
    return fd_check_launch("fd_crop_resize_u8_fwd");
}

// ---------------------------------------------------------------- fd_warp_affine_u8_fwd
// img [B,H,W,3] uint8 -> aligned chips [n,3,S,S] working dtype NCHW (and their horizontal mirrors): warp_affine_fwd_kernel (smallconv.hip) -- the same
// map A[k] from output pixel (x, y, 1) to the sampling position and the same bilinear expression -- with the taps read from the bytes as ``u/255*2-1``.
// Thread mapping of crop_resize_u8_kernel: one thread per output pixel, all three channels.  src_index is device memory nobody has validated: an entry
// outside [0,B) makes its chip a chip of ``fill`` and reads no image byte.  A sampling position that does not fit an int (a malformed A) saturates in
// the conversion and its taps fail the bounds test: they read ``fill``.
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ src_index, const float* __restrict__ A,
                                                             float fill, f16* __restrict__ chips, f16* __restrict__ mirror, int B, int H, int W, int S, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % S);
        const int64_t p = i / S;
        const int oy = (int)(p % S);
        const int64_t k = p / S;
        const int b = src_index[k];
        float v[3] = {fill, fill, fill};
        if (b >= 0 && b < B) {
            const float* a = A + k * 6;
            const float xs = a[0] * ox + a[1] * oy + a[2], ys = a[3] * ox + a[4] * oy + a[5];
            const float xf = floorf(xs), yf = floorf(ys);
            const int x0 = (int)xf, y0 = (int)yf;
            const float lx = xs - xf, ly = ys - yf;
            const uint8_t* ip = img + (int64_t)b * H * W * 3;
            float tap[4][3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t yy = (int64_t)y0 + (q >> 1), xx = (int64_t)x0 + (q & 1);
                const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const uint8_t* t = ip + (in ? (yy * W + xx) * 3 : 0);
#pragma unroll
                for (int c = 0; c < 3; ++c) tap[q][c] = in ? eval_u8_unit(t[c]) : fill;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = bilinear_blend(ly, lx, tap[0][c], tap[1][c], tap[2][c], tap[3][c]);
        }
        const int64_t row = (k * 3 * S + oy) * S;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f16 h = (f16)v[c];
            chips[row + (int64_t)c * S * S + ox] = h;
            if (mirror) mirror[row + (int64_t)c * S * S + (S - 1 - ox)] = h;
        }
    }
}

extern "C" int fd_warp_affine_u8_fwd(const uint8_t* img, const int32_t* src_index, const float* A, float fill, void* chips, void* chips_mirror, int n_chips, int B,
                                     int H, int W, int S, void* stream) {
    FD_REQUIRE(img && src_index && A && chips, "fd_warp_affine_u8_fwd: null pointer");
    FD_REQUIRE(n_chips >= 1 && B >= 1 && S >= 1 && S <= 4096 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096,
               "fd_warp_affine_u8_fwd: n_chips = %d, B = %d (supported >= 1 each), S = %d, H = %d, W = %d (supported 1..4096 each)", n_chips, B, S, H, W);
    const int64_t n = (int64_t)n_chips * S * S;
    hipLaunchKernelGGL(warp_affine_u8_kernel, fd_grid_1d(n, 65536), dim3(256), 0, (hipStream_t)stream, img, src_index, A, fill,
                       (f16*)chips, (f16*)chips_mirror, B, H, W, S, n);
    return fd_check_launch("fd_warp_affine_u8_fwd");
}

// ---------------------------------------------------------------- fd_eval_grid_attrs_u8, fd_eval_grid_attrs
// one output byte of the grid; ``idx`` = flat byte index into [rows*(H+20), cols*(W+50*n_attr+20), 3].  The rules (which strip, which bar) are the
// caller's: the kernel paints preds / bar_rows / palette as given.  T = uint8_t: HWC bytes of the offline evaluator; T = f16: the training step's NCHW images.
template <typename T>
__device__ __forceinline__ uint32_t eval_grid_attrs_byte(int64_t idx, const T* __restrict__ img, const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ boxes, const int32_t* __restrict__ preds, const int32_t* __restrict__ bar_rows,
                                                         const uint8_t* __restrict__ palette, int N, int H, int W, int n_attr, int cols) {
    EvalTilePos p;
    const int outside = eval_tile_locate(idx, order, N, H, W, n_attr, cols, p);
    if (outside >= 0) return (uint32_t)outside;
    const int i = p.i;
    for (int s = 0; s < n_attr; ++s) {
        const int hit = eval_strip(p.ix, p.iy, s, bar_rows[(int64_t)s * N + i]);
        if (hit == EG_BAR) return 255u;
        if (hit == EG_COLOUR) return eval_palette(palette, s, preds[(int64_t)s * N + i], p.c);
    }
    const int x = p.ix - EG_STRIP * n_attr, y = p.iy;
    if (eval_box_outline(x, y, boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3])) return 0u;      // the outline is black here
    return eval_pixel_byte(eval_fetch(img, i, p.c, y, x, H, W));
}

template <typename T>
__global__ __launch_bounds__(256) void eval_grid_attrs_kernel(const T* __restrict__ img, const int32_t* __restrict__ order, const int32_t* __restrict__ boxes,
                                                              const int32_t* __restrict__ preds, const int32_t* __restrict__ bar_rows,
                                                              const uint8_t* __restrict__ palette, uint8_t* __restrict__ grid, int N, int H, int W, int n_attr, int cols,
                                                              int64_t total) {
    eval_grid_store(grid, total, [=](int64_t k) { return eval_grid_attrs_byte(k, img, order, boxes, preds, bar_rows, palette, N, H, W, n_attr, cols); });
}

// the two entry points: one argument list, one set of refusals
template <typename T>
static int eval_grid_attrs_launch(const char* who, const T* images, const int32_t* order, const int32_t* boxes, const int32_t* preds, const int32_t* bar_rows,
                                  const uint8_t* palette, uint8_t* grid, int N, int H, int W, int n_attr, int rows, int cols, void* stream) {
    FD_REQUIRE(images && order && boxes && preds && bar_rows && palette && grid, "%s: null pointer", who);
    FD_REQUIRE(N >= 1 && N <= 4096 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "%s: N = %d, H = %d, W = %d, supported 1..4096 each", who, N, H, W);
    FD_REQUIRE(n_attr >= 1 && n_attr <= FD_EVAL_MAX_ATTR, "%s: n_attr = %d, supported 1..%d", who, n_attr, FD_EVAL_MAX_ATTR);
    FD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols >= N && (int64_t)rows * cols < (int64_t)N + cols,
               "%s: a %d x %d grid does not hold %d tiles with a partly filled last row at most", who, rows, cols, N);
    FD_REQUIRE(((uintptr_t)grid & 3) == 0, "%s: the grid buffer must be 4-byte aligned", who);
    const int64_t total = (int64_t)rows * (H + 2 * EG_FRAME) * cols * (W + EG_STRIP * n_attr + 2 * EG_FRAME) * 3;
    FD_REQUIRE(total < ((int64_t)1 << 40), "%s: a grid of %lld bytes is not supported", who, (long long)total);
    hipLaunchKernelGGL(eval_grid_attrs_kernel<T>, fd_grid_1d((total + 3) / 4, 65536), dim3(256), 0, (hipStream_t)stream, images, order, boxes, preds, bar_rows, palette, grid,
                       N, H, W, n_attr, cols, total);
    return fd_check_launch(who);
}

extern "C" int fd_eval_grid_attrs_u8(const uint8_t* images, const int32_t* order, const int32_t* boxes, const int32_t* preds, const int32_t* bar_rows,
                                     const uint8_t* palette, uint8_t* grid, int N, int H, int W, int n_attr, int rows, int cols, void* stream) {
    return eval_grid_attrs_launch("fd_eval_grid_attrs_u8", images, order, boxes, preds, bar_rows, palette, grid, N, H, W, n_attr, rows, cols, stream);
}

extern "C" int fd_eval_grid_attrs(const void* images, const int32_t* order, const int32_t* boxes, const int32_t* preds, const int32_t* bar_rows,
                                  const uint8_t* palette, uint8_t* grid, int N, int H, int W, int n_attr, int rows, int cols, void* stream) {
    return eval_grid_attrs_launch("fd_eval_grid_attrs", (const f16*)images, order, boxes, preds, bar_rows, palette, grid, N, H, W, n_attr, rows, cols, stream);
}

// ---------------------------------------------------------------- fd_eval_grid_labels_u8
// The reference's index text (``img_pil_draw.text((400, 400), f"{idx.item()}", font=fnt)``, plot_in_grid :199-200 and its two- / three-strip
// siblings) as an in-place pass over a grid one of the three painters has written: tile t gets the 8-bit coverage mask of the string str(order[t]),
// rasterised on the host (evaluation.IndexLabels), blended as white ink by PIL's rule and clipped to the tile's inner area.  The descriptor table is
// device memory nobody has validated: every entry is checked against ``n_labels`` / ``mask_bytes`` before a mask byte is read, and a tile whose entry
// fails gets nothing.  blockIdx.y = tile, blockIdx.x strides over the visible mask rows, threads run along a mask row: mask reads are contiguous and
// the grid accesses are contiguous 3-byte pixels; each thread reads and writes only its own pixel.
#define EG_LABEL_ROW_BLOCKS 128

// PIL's ``MULDIV255``-style blend of ink 255 under coverage m (ImagingDraw's ``BLEND`` for 8-bit channels)
__device__ __forceinline__ uint32_t eval_label_blend(uint32_t a, uint32_t m) {
    const uint32_t t = a * (255u - m) + 255u * m + 128u;
    return ((t >> 8) + t) >> 8;
}

__global__ __launch_bounds__(256) void eval_grid_labels_kernel(uint8_t* __restrict__ grid, const int32_t* __restrict__ order, const uint8_t* __restrict__ masks,
                                                               int64_t mask_bytes, const int32_t* __restrict__ desc, int n_labels, int N, int H, int W, int n_strip,
                                                               int cols, int x, int y) {
    const int t = blockIdx.y;
    if (t >= N) return;
    const int i = order[t];
    if (i < 0 || i >= N || i >= n_labels) return;      // a malformed order entry is a white tile (eval_tile_locate); no mask for this index
    const int32_t* d = desc + (int64_t)i * 5;
    const int64_t w = d[0], h = d[1], boff = d[4];
    if (w <= 0 || h <= 0 || boff < 0 || w * h > mask_bytes || boff > mask_bytes - w * h) return;
    const int64_t IW = W + EG_STRIP * n_strip;
    const int64_t X0 = (int64_t)x + d[2], Y0 = (int64_t)y + d[3];      // the mask's top-left inside the strip-expanded image
    const int64_t c_lo = X0 < 0 ? -X0 : 0, c_hi = IW - X0 < w ? IW - X0 : w;
    const int64_t r_lo = Y0 < 0 ? -Y0 : 0, r_hi = H - Y0 < h ? H - Y0 : h;
    if (c_lo >= c_hi || r_lo >= r_hi) return;
    const int tw = W + EG_STRIP * n_strip + 2 * EG_FRAME, th = H + 2 * EG_FRAME;
    const int64_t GW = (int64_t)cols * tw;
    const int tr = t / cols, tc = t - tr * cols;
    for (int64_t r = r_lo + blockIdx.x; r < r_hi; r += gridDim.x) {
        const uint8_t* mrow = masks + boff + r * w;
        uint8_t* grow = grid + (((int64_t)tr * th + EG_FRAME + Y0 + r) * GW + (int64_t)tc * tw + EG_FRAME + X0) * 3;
        for (int64_t c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
            const uint32_t m = mrow[c];
            if (m == 0) continue;      // the blend is the identity there
            uint8_t* px = grow + c * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) px[k] = (uint8_t)eval_label_blend(px[k], m);
        }
    }
}

extern "C" int fd_eval_grid_labels_u8(uint8_t* grid, const int32_t* order, const uint8_t* masks, int64_t mask_bytes, const int32_t* desc, int n_labels, int N, int H,
                                      int W, int n_strip, int rows, int cols, int x, int y, void* stream) {
    FD_REQUIRE(grid && order && masks && desc, "fd_eval_grid_labels_u8: null pointer");
    FD_REQUIRE(N >= 1 && N <= 4096 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "fd_eval_grid_labels_u8: N = %d, H = %d, W = %d, supported 1..4096 each", N, H, W);
    FD_REQUIRE(n_strip >= 1 && n_strip <= FD_EVAL_MAX_ATTR, "fd_eval_grid_labels_u8: n_strip = %d, supported 1..%d", n_strip, FD_EVAL_MAX_ATTR);
    FD_REQUIRE(rows >= 1 && cols >= 1 && (int64_t)rows * cols >= N && (int64_t)rows * cols < (int64_t)N + cols,
               "fd_eval_grid_labels_u8: a %d x %d grid does not hold %d tiles with a partly filled last row at most", rows, cols, N);
    FD_REQUIRE(n_labels >= 1, "fd_eval_grid_labels_u8: n_labels = %d, at least 1", n_labels);
    FD_REQUIRE(mask_bytes >= 0, "fd_eval_grid_labels_u8: mask_bytes = %lld, must not be negative", (long long)mask_bytes);
    const unsigned bx = (unsigned)(H < EG_LABEL_ROW_BLOCKS ? H : EG_LABEL_ROW_BLOCKS);
    hipLaunchKernelGGL(eval_grid_labels_kernel, dim3(bx, (unsigned)N), dim3(256), 0, (hipStream_t)stream, grid, order, masks, mask_bytes, desc, n_labels, N, H, W,
                       n_strip, cols, x, y);
    return fd_check_launch("fd_eval_grid_labels_u8");
}
