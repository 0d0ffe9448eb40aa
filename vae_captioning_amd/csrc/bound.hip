// Posterior at inference: the draws of q(z | caption, image) with their importance log-weights, the closed-form KL and the
// reduction to the ELBO / importance-weighted bound (generate.py: CaptionGenerator.bound; definitions in DESIGN.md "Bounds").
// Sequence rows are caption-major, draw-minor: row r = c*K + k.
//
//   vc_posterior_latent_f32  z[r, s, l] = mean[r / K, l] + std[r / K, l] * eps[r, s, l] (the expression of sample_kernel), eps injected
//                            or drawn here with the Philox / Box-Muller code of vc_philox_normal_f32 on the flat element index (same
//                            seed, offset, step: same bits), and logw[r] = log p(z | I) - log q(z | x, I) in float64, accumulated from
//                            the registers that hold z and eps: one pass over the row
//   vc_gauss_kl_rows_f64     KL(q || p) of a caption in closed form
//   vc_bound_reduce_f64      score_reduce_kernel's per-draw sums, then elbo / iwae / rec / kl_mc / ess of each caption
// No atomics: a float64 sum is per-lane partials in a fixed stride order, then a fixed shuffle tree (and, in the 256-lane kernel, the four
// waves' sums in wave order).  What a row gets depends on the row only.
#include <math.h>
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int BOUND_MAX_K = 256;

// One workgroup per row; thread t owns the in-row element quads t, t + 256, ... (a partition by the position INSIDE the row: the same
// whatever the row's index is).  Philox numbers are keyed by the flat element index row*SL + j, so a row whose first element is not a
// multiple of 4 starts inside a Philox quad: an in-row quad then takes its four numbers from two neighbouring Philox quads.
__global__ __launch_bounds__(256) void posterior_latent_kernel(long SL, int L, int K, const float* __restrict__ mean,
                                                               const float* __restrict__ std_, const float* __restrict__ pm,
                                                               const int32_t* __restrict__ img, float prior_std,
                                                               const float* __restrict__ eps, uint64_t seed, uint64_t offset,
                                                               const int32_t* __restrict__ step, float* __restrict__ z,
                                                               double* __restrict__ logw) {
    __shared__ double sh[4];
    const long r = blockIdx.x;
    const long c = r / K;
    const float* mu = mean + c * L;
    const float* sg = std_ + c * L;
    const float* pmr = pm ? pm + (long)(img ? img[c] : 0) * L : nullptr;
    const long base = r * SL;
    const uint32_t k1 = (uint32_t)(seed >> 32) + (step ? (uint32_t)step[0] : 0u);
    const double sp = (double)prior_std, log_sp = log(sp);
    double acc = 0.0;
    for (long j0 = (long)threadIdx.x * 4; j0 < SL; j0 += 1024) {
        float f[4];
        if (eps) {
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = j0 + j < SL ? eps[base + j0 + j] : 0.f;
        } else {   // = philox_kernel mode 1 on the elements base + j0 .. base + j0 + 3
            const long i0 = base + j0, q = i0 >> 2;
            const int sub = (int)(i0 & 3);
            uint32_t rr[4];
            float a[4], b[4] = {0.f, 0.f, 0.f, 0.f};
            philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, k1, rr);
            box_muller4(rr, a);
            if (sub) {
                const long q2 = q + 1;
                philox4x32_10((uint32_t)q2, (uint32_t)((uint64_t)q2 >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, k1, rr);
                box_muller4(rr, b);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = sub + j;   // 0..6 over the two quads
                f[j] = m == 0 ? a[0] : m == 1 ? a[1] : m == 2 ? a[2] : m == 3 ? a[3] : m == 4 ? b[0] : m == 5 ? b[1] : b[2];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long jj = j0 + j;
            if (jj < SL) {
                const int l = (int)(jj % L);
                const float s = sg[l];
                const float zz = mu[l] + s * f[j];   // (the expression of sample_kernel)
                z[base + jj] = zz;
                const double d = ((double)zz - (pmr ? (double)pmr[l] : 0.0)) / sp, e = (double)f[j];
                // log p - log q of the element, the 2 pi terms cancelled; q's term from eps itself (no cancellation for a sharp q)
                acc += (0.5 * e * e - 0.5 * d * d) + (log((double)s) - log_sp);
            }
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) logw[r] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One wave per caption; lane t owns the dimensions t, t + 64, ...  Every dimension's term is >= 0: the sum has no cancellation.
__global__ __launch_bounds__(64) void gauss_kl_rows_kernel(int S, int L, const float* __restrict__ mean, const float* __restrict__ std_,
                                                           const float* __restrict__ pm, const int32_t* __restrict__ img, float prior_std,
                                                           double* __restrict__ kl) {
    const long c = blockIdx.x;
    const float* pmr = pm ? pm + (long)(img ? img[c] : 0) * L : nullptr;
    const double sp = (double)prior_std, log_sp = log(sp), inv = 1.0 / (2.0 * sp * sp);
    double acc = 0.0;
    for (int l = threadIdx.x; l < L; l += 64) {
        const double s = (double)std_[c * L + l], d = (double)mean[c * L + l] - (pmr ? (double)pmr[l] : 0.0);
        acc += (log_sp - log(s)) + (s * s + d * d) * inv - 0.5;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) kl[c] = (double)S * acc;
}

// One wave per caption; lane l owns the draws l, l + 64, ... (K <= 256): score_reduce_kernel's scheme and its logprob sums.
__global__ __launch_bounds__(64) void bound_reduce_kernel(const float* __restrict__ lp, int T, int C, int K, const int32_t* __restrict__ len,
                                                          const double* __restrict__ logw, double* __restrict__ logprob,
                                                          double* __restrict__ out) {
    const int c = blockIdx.x, lane = threadIdx.x;
    int n = len[c];
    n = n < 0 ? 0 : (n > T ? T : n);
    const long N = (long)C * K;
    double a[BOUND_MAX_K / 64];
    double mx = -INFINITY, s_a = 0.0, s_rec = 0.0, s_w = 0.0;
#pragma unroll
    for (int j = 0; j < BOUND_MAX_K / 64; ++j) {
        const int k = lane + j * 64;
        double v = 0.0;
        if (k < K) {
            double s = 0.0;
            for (int t = 0; t < n; ++t) s += (double)lp[t * N + (long)c * K + k];   // ascending t, float64 sum
            logprob[(long)c * K + k] = s;
            const double w = logw[(long)c * K + k];
            v = s + w;
            mx = fmax(mx, v);
            s_a += v;
            s_rec += s;
            s_w += w;
        }
        a[j] = v;
    }
    mx = wave_max(mx);
    double e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int j = 0; j < BOUND_MAX_K / 64; ++j)
        if (lane + j * 64 < K) {
            const double v = exp(a[j] - mx);
            e1 += v;
            e2 += v * v;
        }
    s_a = wave_sum(s_a);
    s_rec = wave_sum(s_rec);
    s_w = wave_sum(s_w);
    e1 = wave_sum(e1);
    e2 = wave_sum(e2);
    if (lane == 0) {
        double* o = out + (long)c * 5;
        o[0] = s_a / (double)K;                      // elbo
        o[1] = mx + log(e1) - log((double)K);        // iwae
        o[2] = s_rec / (double)K;                    // rec
        o[3] = -s_w / (double)K;                     // kl_mc
        o[4] = e1 * e1 / e2;                         // ess
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_posterior_latent_f32(void* stream, long rows, int K, int S, int L, const float* mean, const float* std_, const float* pm,
                                       const int32_t* img, float prior_std, const float* eps, uint64_t seed, uint64_t offset,
                                       const int32_t* step, float* z, double* logw) {
    VC_CHECK_ARG(K >= 1 && K <= BOUND_MAX_K, "K must be 1..256");
    VC_CHECK_ARG(rows >= 0 && S >= 1 && L >= 1, "bad shape");
    VC_CHECK_ARG(rows % K == 0, "rows must be captions * K");
    VC_CHECK_ARG(rows < (1L << 31), "too many rows");
    VC_CHECK_ARG(z && logw, "null output");
    VC_CHECK_ARG(mean && std_, "null operand");
    VC_CHECK_ARG(!pm == !img, "pm and img come together");
    VC_CHECK_ARG(prior_std > 0.f && prior_std < INFINITY, "prior_std must be finite and > 0");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(posterior_latent_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (long)S * L, L, K, mean, std_, pm, img,
                       prior_std, eps, seed, offset, step, z, logw);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_gauss_kl_rows_f64(void* stream, long C, int S, int L, const float* mean, const float* std_, const float* pm,
                                    const int32_t* img, float prior_std, double* kl) {
    VC_CHECK_ARG(C >= 0 && C < (1L << 31) && S >= 1 && L >= 1, "bad shape");
    VC_CHECK_ARG(kl, "null output");
    VC_CHECK_ARG(mean && std_, "null operand");
    VC_CHECK_ARG(!pm == !img, "pm and img come together");
    VC_CHECK_ARG(prior_std > 0.f && prior_std < INFINITY, "prior_std must be finite and > 0");
    if (C == 0) return 0;
    hipLaunchKernelGGL(gauss_kl_rows_kernel, dim3((unsigned)C), dim3(64), 0, (hipStream_t)stream, S, L, mean, std_, pm, img, prior_std, kl);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_bound_reduce_f64(void* stream, const float* lp, int T, int C, int K, const int32_t* len, const double* logw,
                                   double* logprob, double* out) {
    VC_CHECK_ARG(K >= 1 && K <= BOUND_MAX_K, "K must be 1..256");
    VC_CHECK_ARG(T >= 0 && C >= 0, "bad shape");
    VC_CHECK_ARG(logprob && out, "null output");
    VC_CHECK_ARG(len && logw && (lp || T == 0), "null operand");
    if (C == 0) return 0;
    hipLaunchKernelGGL(bound_reduce_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, lp, T, C, K, len, logw, logprob, out);
    VC_LAUNCH_CHECK();
    return 0;
}
