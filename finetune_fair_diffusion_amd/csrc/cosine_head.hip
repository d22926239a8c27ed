// Cosine-similarity logits of the zero-shot CLIP classifier head (classifier.ZeroShotClipClassifier) and their gradient with respect to the raw image
// embedding.  fp32 in, fp32 out: the same code in both libraries.
//
//   inv_norm[n]  = 1 / max(|e_n|, 1e-12)                                   (the clamp of vit.feature_loss_and_grad)
//   logits[n, k] = scale * inv_norm[n] * <e_n, t_hat_k>
//   d_e[n]       = scale * inv_norm[n] * (sum_k d_logits[n, k] t_hat_k - (sum_k d_logits[n, k] c[n, k]) e_n inv_norm[n]),     c = logits / scale
//                  (0 for a row at the clamp, inv_norm[n] >= 5e11)
//
// Rows are independent.  Forward: one wave per row; every lane walks the row with stride 64 in ascending order and the K + 1 partial sums meet in the
// xor-shuffle tree of wave_sum, so the summation order is a function of (E, K) alone.  Backward: the only sum is the K-term one, which every thread
// takes in ascending k; the rest is element-wise.  No atomics, no LDS, scalar 4-byte accesses only (nothing but 4-byte alignment is assumed).
#include "common.h"

#define FD_COSINE_MAX_K 16
#define FD_COSINE_MAX_E 4096

__global__ __launch_bounds__(FD_WAVE) void cosine_logits_fwd_kernel(const float* __restrict__ e, int64_t lde, const float* __restrict__ t_hat, float scale,
                                                                    float* __restrict__ logits, float* __restrict__ inv_norm, int E, int K) {
    const int64_t row = blockIdx.x;
    const float* er = e + row * lde;
    const int lane = threadIdx.x;
    float ss = 0.f;
    float dot[FD_COSINE_MAX_K];
#pragma unroll
    for (int k = 0; k < FD_COSINE_MAX_K; ++k) dot[k] = 0.f;
    for (int c = lane; c < E; c += FD_WAVE) {
        const float v = er[c];
        ss += v * v;
#pragma unroll
        for (int k = 0; k < FD_COSINE_MAX_K; ++k)
            if (k < K) dot[k] += v * t_hat[(int64_t)k * E + c];
    }
    ss = wave_sum(ss);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int k = 0; k < FD_COSINE_MAX_K; ++k) {
        if (k < K) {                                         // K is uniform: every lane takes part in the shuffles
            const float d = wave_sum(dot[k]);
            if (lane == 0) logits[row * K + k] = scale * inv * d;
        }
    }
    if (lane == 0) inv_norm[row] = inv;
}

__global__ __launch_bounds__(256) void cosine_logits_bwd_kernel(const float* __restrict__ e, int64_t lde, const float* __restrict__ t_hat,
                                                                const float* __restrict__ logits, const float* __restrict__ inv_norm,
                                                                const float* __restrict__ d_logits, float scale, float* __restrict__ d_e, int E, int K) {
    const int64_t row = blockIdx.x;
    const float* er = e + row * lde;
    const float inv = inv_norm[row];
    // a row at the clamp (|e| <= 1e-12: in practice the all-zero row) has no direction: its logits are 0 and its gradient is defined as 0, not scale * 1e12 * t_hat
    const float g = inv >= 5e11f ? 0.f : scale * inv;
    float dl[FD_COSINE_MAX_K];
    float s = 0.f;                                           // sum_k d_logits c, ascending k, the same in every thread
#pragma unroll
    for (int k = 0; k < FD_COSINE_MAX_K; ++k) {
        dl[k] = 0.f;
        if (k < K) {
            dl[k] = d_logits[row * K + k];
            s += dl[k] * (scale != 0.f ? logits[row * K + k] / scale : 0.f);
        }
    }
    for (int c = threadIdx.x; c < E; c += 256) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < FD_COSINE_MAX_K; ++k)
            if (k < K) a += dl[k] * t_hat[(int64_t)k * E + c];
        d_e[row * E + c] = g * (a - s * (er[c] * inv));
    }
}

static int cosine_check(const char* who, bool buffers, int64_t lde, int N, int E, int K) {
    FD_REQUIRE(buffers, "%s: null buffer", who);
    FD_REQUIRE(N >= 1, "%s: N = %d, at least one row is needed", who, N);
    FD_REQUIRE(E >= 1 && E <= FD_COSINE_MAX_E, "%s: E = %d is outside 1..%d", who, E, FD_COSINE_MAX_E);
    FD_REQUIRE(K >= 1 && K <= FD_COSINE_MAX_K, "%s: K = %d is outside 1..%d", who, K, FD_COSINE_MAX_K);
    FD_REQUIRE(lde >= E, "%s: row stride lde = %lld is smaller than E = %d", who, (long long)lde, E);
    return FD_OK;
}

extern "C" int fd_cosine_logits_fwd(const float* e, int64_t lde, const float* t_hat, float scale, float* logits, float* inv_norm, int N, int E, int K,
                                    void* stream) {
    const int rc = cosine_check("fd_cosine_logits_fwd", e && t_hat && logits && inv_norm, lde, N, E, K);
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(cosine_logits_fwd_kernel, dim3((unsigned)N), dim3(FD_WAVE), 0, (hipStream_t)stream, e, lde, t_hat, scale, logits, inv_norm, E, K);
    return fd_check_launch("fd_cosine_logits_fwd");
}

extern "C" int fd_cosine_logits_bwd(const float* e, int64_t lde, const float* t_hat, const float* logits, const float* inv_norm, const float* d_logits,
                                    float scale, float* d_e, int N, int E, int K, void* stream) {
    const int rc = cosine_check("fd_cosine_logits_bwd", e && t_hat && logits && inv_norm && d_logits && d_e, lde, N, E, K);
    if (rc != FD_OK) return rc;
    hipLaunchKernelGGL(cosine_logits_bwd_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, e, lde, t_hat, logits, inv_norm, d_logits, scale, d_e, E,
                       K);
    return fd_check_launch("fd_cosine_logits_bwd");
}
