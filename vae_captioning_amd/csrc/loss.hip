// Loss-side kernels: masked sparse softmax cross-entropy (forward + gradient in one pass
// over the logits), reparameterised Gaussian sample, KL terms for the Normal / GMM / AG
// priors and their gradients, and the 90-component head mixing of the GMM / AG encoders.
//
// Reference: main.py:118-177 (KL, masked CE, lower bound), vae_model/encoder.py:59-109
// (heads, zs.Normal sample), vae_model/decoder.py:109-110 (the z buffer is consumed as a
// raw [N, S*L] reshape of [S, N, L] -- quirk Q1 -- i.e. the SAME memory, no kernel).
#include <type_traits>

#include "row_ops.h"
#include "vaecap.h"
#include "xent_row.h"

namespace vc {

static inline int grid_for(long work_items, int per_block = 256, int cap = 2048) {
    long b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// ---------------------------------------------------------------------------------------
// tf.nn.sparse_softmax_cross_entropy_with_logits + mask + div (main.py:152-158, Q8).
// One workgroup per row; the row (V <= 12288, row pitch % 4 == 0) lives in registers, so the
// logits are read ONCE from HBM and overwritten in place by d(loss)/d(logits):
//   ce = logsumexp(x) - x[label]; mask = (label != 0); row_loss = ce * mask
//   dlogits = (softmax(x) - onehot(label)) * mask * gscale / den[0]
// HBM traffic = 4 B read + 4 B written per logit (the algorithmic minimum for an unfused
// softmax-CE with gradient).
// ---------------------------------------------------------------------------------------
template <bool WRITE_GRAD>
__global__ __launch_bounds__(256) void xent_reg_kernel(float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                       int V, long ld, const float* __restrict__ den, float gscale,
                                                       float* __restrict__ row_loss) {
    __shared__ float sh[4];
    const long row = blockIdx.x;
    float4* p = reinterpret_cast<float4*>(logits + row * ld);
    const int V4 = (V + 3) >> 2;  // V % 4 != 0 (the reference's observed 11313): the row's last quad reaches into the ld padding
    const int label = labels[row];
    float4 x[XENT_MAXQ];
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < XENT_MAXQ; ++q) {
        const int i = threadIdx.x + q * 256;
        if (i < V4) {
            x[q] = p[i];
            if (i * 4 + 3 >= V) {  // columns >= V do not exist: -inf drops them from the max and the sum (exp -> 0, gradient 0)
                if (i * 4 + 1 >= V) x[q].y = -INFINITY;
                if (i * 4 + 2 >= V) x[q].z = -INFINITY;
                x[q].w = -INFINITY;
            }
            mx = fmaxf(mx, fmaxf(fmaxf(x[q].x, x[q].y), fmaxf(x[q].z, x[q].w)));
        }
    }
    mx = block_max<256>(mx, sh);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < XENT_MAXQ; ++q) {
        const int i = threadIdx.x + q * 256;
        if (i < V4) {
            x[q].x = __expf(x[q].x - mx); x[q].y = __expf(x[q].y - mx);
            x[q].z = __expf(x[q].z - mx); x[q].w = __expf(x[q].w - mx);
            s += (x[q].x + x[q].y) + (x[q].z + x[q].w);
        }
    }
    s = block_sum<256>(s, sh);
    const bool live = label != 0;
    if (threadIdx.x == 0) {
        float l = 0.f;
        if (live && label > 0 && label < V) l = __logf(s) + mx - logits[row * ld + label];
        row_loss[row] = l;
    }
    if (WRITE_GRAD) {
        __syncthreads();  // thread 0 has read logits[label] before anyone overwrites it
        const float k = live ? gscale / den[0] : 0.f;
        const float inv = k / s;
#pragma unroll
        for (int q = 0; q < XENT_MAXQ; ++q) {
            const int i = threadIdx.x + q * 256;
            if (i < V4) {
                float4 d = make_float4(x[q].x * inv, x[q].y * inv, x[q].z * inv, x[q].w * inv);
                const int c = i * 4;
                if (label >= c && label < c + 4) {
                    if (label == c) d.x -= k; else if (label == c + 1) d.y -= k; else if (label == c + 2) d.z -= k; else d.w -= k;
                }
                p[i] = d;
            }
        }
    }
}

// Generic V: three passes over the row (passes 2 and 3 hit L2).
template <bool WRITE_GRAD>
__global__ __launch_bounds__(256) void xent_mem_kernel(float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                       int V, long ld, const float* __restrict__ den, float gscale,
                                                       float* __restrict__ row_loss) {
    __shared__ float sh[4];
    const long row = blockIdx.x;
    float* p = logits + row * ld;
    const int label = labels[row];
    float mx = -INFINITY;
    for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, p[c]);
    mx = block_max<256>(mx, sh);
    float s = 0.f;
    for (int c = threadIdx.x; c < V; c += 256) s += __expf(p[c] - mx);
    s = block_sum<256>(s, sh);
    const bool live = label != 0;
    if (threadIdx.x == 0) {
        float l = 0.f;
        if (live && label > 0 && label < V) l = __logf(s) + mx - p[label];
        row_loss[row] = l;
    }
    if (WRITE_GRAD) {
        __syncthreads();
        const float k = live ? gscale / den[0] : 0.f;
        const float inv = k / s;
        for (int c = threadIdx.x; c < V; c += 256) {
            float d = __expf(p[c] - mx) * inv;
            if (c == label) d -= k;
            p[c] = d;
        }
    }
}

// softmax probabilities per row (gen mode: tf.nn.softmax, vae_model/decoder.py:140,142)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, int V, long ld,
                                                           float* __restrict__ y, long ldy) {
    __shared__ float sh[4];
    const float* p = x + (long)blockIdx.x * ld;
    float* q = y + (long)blockIdx.x * ldy;
    float mx = -INFINITY;
    for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, p[c]);
    mx = block_max<256>(mx, sh);
    float s = 0.f;
    for (int c = threadIdx.x; c < V; c += 256) s += __expf(p[c] - mx);
    s = block_sum<256>(s, sh);
    const float inv = 1.f / s;
    for (int c = threadIdx.x; c < V; c += 256) q[c] = __expf(p[c] - mx) * inv;
}

// The same with the row held in registers (V <= 12288, 16-byte aligned pitches): one read of the logits instead of three, 16-byte
// accesses (34 -> ~12 us for 640 rows x 10 000 columns)
__global__ __launch_bounds__(256) void softmax_rows_reg_kernel(const float* __restrict__ x, int V, long ld,
                                                               float* __restrict__ y, long ldy) {
    __shared__ float sh[4];
    const float4* p = reinterpret_cast<const float4*>(x + (long)blockIdx.x * ld);
    float4* q = reinterpret_cast<float4*>(y + (long)blockIdx.x * ldy);
    const int Q = V >> 2;
    float4 r[12];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < Q) {
            r[i] = p[c];
            mx = fmaxf(fmaxf(mx, fmaxf(r[i].x, r[i].y)), fmaxf(r[i].z, r[i].w));
        }
    }
    mx = block_max<256>(mx, sh);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < Q) {
            r[i].x = __expf(r[i].x - mx); r[i].y = __expf(r[i].y - mx); r[i].z = __expf(r[i].z - mx); r[i].w = __expf(r[i].w - mx);
            s += (r[i].x + r[i].y) + (r[i].z + r[i].w);
        }
    }
    s = block_sum<256>(s, sh);
    const float inv = 1.f / s;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < Q) q[c] = make_float4(r[i].x * inv, r[i].y * inv, r[i].z * inv, r[i].w * inv);
    }
}

// Categorical sample per row from logits / temperature (tf.multinomial, vae_model/decoder.py:137-138) by
// inverse CDF with an INJECTED uniform u[row] in [0,1): index = first i with cumsum(softmax)[i] > u.
// (TF draws with its own Gumbel/Philox stream, which cannot be matched; the distribution is the same.)  The draw is row_ops.h's; the
// scaled maximum in front of it is taken with strided (coalesced) loads, the row being read in place.
__global__ __launch_bounds__(256) void multinomial_rows_kernel(const float* __restrict__ logits, int V, long ld, float inv_temp,
                                                               const float* __restrict__ u, int32_t* __restrict__ out) {
    __shared__ float sh[4];
    __shared__ float part[256];
    const float* p = logits + (long)blockIdx.x * ld;
    float mx = -INFINITY;
    for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, p[c] * inv_temp);
    mx = block_max<256>(mx, sh);
    int c0, c1;
    const int per = row_chunk(V, c0, c1);
    row_cdf_part(p, c0, c1, inv_temp, mx, part);
    if (threadIdx.x == 0) out[blockIdx.x] = row_cdf_pick(p, V, per, inv_temp, mx, part, u + blockIdx.x);
}

// ---------------------------------------------------------------------------------------
// z[s,n,l] = mean[n,l] + std[n,l] * eps[s,n,l]   (zs.Normal, n_samples=S; encoder.py:108-109)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ mean, const float* __restrict__ std_,
                                                     const float* __restrict__ eps, long NL, long total,
                                                     float* __restrict__ z) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long j = i % NL;
        z[i] = mean[j] + std_[j] * eps[i];
    }
}

// Data-parallel form of the sample (quirk Q1 under sharding, see dp.py): the z_rnn input rows of this
// rank are the flat range q in [q0, q0+nq) of the GLOBAL [S, Ng, L] sample tensor, q = s*Ng + n.
//   z[(q-q0), l] = mean_g[q % Ng, l] + std_g[q % Ng, l] * eps[(q-q0), l]
// With Ng = N, q0 = 0, nq = S*N it is exactly sample_kernel.
__global__ __launch_bounds__(256) void sample_mixed_kernel(const float* __restrict__ mean_g, const float* __restrict__ std_g,
                                                           const float* __restrict__ eps, int Ng, int L, long q0, long total,
                                                           float* __restrict__ z) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long q = q0 + i / L;
        const long j = (q % Ng) * L + i % L;
        z[i] = mean_g[j] + std_g[j] * eps[i];
    }
}
// ... and of its gradient: per global row n, the sums over this rank's q == n (mod Ng):
//   dmean_part[n,l] = sum dz[(q-q0), l],   dstd_part[n,l] = sum dz[(q-q0), l] * eps[(q-q0), l]
// (rows that do not occur get zeros); the partials are then reduce-scattered over the ranks.
__global__ __launch_bounds__(256) void latent_sums_mixed_kernel(const float* __restrict__ dz, const float* __restrict__ eps,
                                                                int Ng, int L, long q0, long nq, float* __restrict__ dmean,
                                                                float* __restrict__ dstd) {
    const long NL = (long)Ng * L;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < NL; j += (long)gridDim.x * 256) {
        const long n = j / L;
        const int l = (int)(j % L);
        long q = q0 + ((n - q0 % Ng) % Ng + Ng) % Ng;  // first q >= q0 with q % Ng == n
        float dm = 0.f, ds = 0.f;
        for (; q < q0 + nq; q += Ng) {
            const float g = dz[(q - q0) * L + l];
            dm += g;
            ds += g * eps[(q - q0) * L + l];
        }
        dmean[j] = dm;
        dstd[j] = ds;
    }
}

// ---------------------------------------------------------------------------------------
// KL per row.  mode 0 (Normal / GMM, main.py:120-124,131-135):
//     -0.5 * sum_l (1 + log(std^2 + 1e-5) - mean^2 - std^2)
// mode 1 (AG, main.py:140-145):
//     -0.5 * sum_l [0.5 + log(std+1e-5) - log(0.1+1e-5) - ((mean-mu_p)^2 + std^2)/(2*0.1^2+1e-7)]
// One wave per row.
// ---------------------------------------------------------------------------------------
#define VC_AG_SIGMA 0.1f
__global__ __launch_bounds__(256) void kl_rows_kernel(const float* __restrict__ mean, const float* __restrict__ std_,
                                                      const float* __restrict__ mu_p, int N, int L, int mode,
                                                      float* __restrict__ row_kl) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int l = lane; l < L; l += 64) {
        const float m = mean[(long)row * L + l], sd = std_[(long)row * L + l];
        if (mode == 0) {
            s += 1.f + logf(sd * sd + 1e-5f) - m * m - sd * sd;
        } else {
            const float d = m - mu_p[(long)row * L + l];
            s += 0.5f + logf(sd + 1e-5f) - logf(VC_AG_SIGMA + 1e-5f) - (d * d + sd * sd) / (2.f * VC_AG_SIGMA * VC_AG_SIGMA + 1e-7f);
        }
    }
    s = wave_sum(s);
    if (lane == 0) row_kl[row] = -0.5f * s;
}

// ---------------------------------------------------------------------------------------
// GMM / AG heads.  heads [N, 2*K*L]: columns [k*L + l] = component means tm[n,k,l],
// columns [K*L + k*L + l] = log-stds tl[n,k,l]  (vae_model/encoder.py:71-107).
//   AG : mean = sum_k c[n,k]*tm[n,k,:],  std = sum_k c[n,k]*exp(tl[n,k,:])   (:105-107)
//   GMM: mean = tm[n, idx[n], :],        std = exp(tl[n, idx[n], :])         (:87-88)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void heads_mix_fwd_kernel(const float* __restrict__ heads, const float* __restrict__ c,
                                                            const int32_t* __restrict__ idx, int N, int K, int L,
                                                            float* __restrict__ mean, float* __restrict__ std_) {
    const long NL = (long)N * L;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < NL; j += (long)gridDim.x * 256) {
        const long n = j / L;
        const int l = (int)(j % L);
        const float* h = heads + n * 2 * K * L;
        float m = 0.f, s = 0.f;
        if (idx) {
            const int k = idx[n];
            m = h[k * L + l];
            s = __expf(h[K * L + k * L + l]);
        } else {
            for (int k = 0; k < K; ++k) {
                const float ck = c[n * K + k];
                if (ck != 0.f) {
                    m += ck * h[k * L + l];
                    s += ck * __expf(h[K * L + k * L + l]);
                }
            }
        }
        mean[j] = m;
        std_[j] = s;
    }
}

__global__ __launch_bounds__(256) void heads_mix_bwd_kernel(const float* __restrict__ heads, const float* __restrict__ c,
                                                            const int32_t* __restrict__ idx, const float* __restrict__ dmean,
                                                            const float* __restrict__ dstd, int N, int K, int L,
                                                            float* __restrict__ dheads) {
    const long total = (long)N * K * L;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long n = i / ((long)K * L);
        const int kl = (int)(i % ((long)K * L));
        const int k = kl / L, l = kl % L;
        const float w = idx ? (idx[n] == k ? 1.f : 0.f) : c[n * K + k];
        const long o = n * 2 * K * L;
        float gm = 0.f, gs = 0.f;
        if (w != 0.f) {
            gm = w * dmean[n * L + l];
            gs = w * dstd[n * L + l] * __expf(heads[o + (long)K * L + kl]);
        }
        dheads[o + kl] = gm;
        dheads[o + (long)K * L + kl] = gs;
    }
}

// Scalars of one step (main.py:156-177): out[0] rec_loss = ce_num/ce_den (+ reg), out[1] mean KL,
// out[2] lower_bound = rec + ann*kld/10 (mean over rows for the AG vector loss, what main.py:247-251
// prints), out[3] annealing coefficient.  All inputs are device scalars.
__global__ void loss_finalize_kernel(const float* ce_num, const float* ce_den, const float* reg, float reg_scale,
                                     const float* kl_sum, float inv_n, const float* ann, float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float rec = ce_num[0] / ce_den[0];
    if (reg) rec += reg[0] * reg_scale;
    const float a = ann ? ann[0] : 1.f;
    const float kld = kl_sum ? kl_sum[0] * inv_n : 0.f;
    out[0] = rec;
    out[1] = kld;
    out[2] = kl_sum ? rec + a * kld / 10.f : rec;
    out[3] = a;
}

// =======================================================================================
// Training objective options (DESIGN.md "Training objective options"): label smoothing, free bits, KL weight.  Every kernel
// below is a NEW one beside the plain form above -- with an option off the engine launches the plain entry, unchanged.
// =======================================================================================

// Label-smoothed masked cross-entropy: target (1 - eps) * onehot + eps / V over the V real columns.
//   row_loss = mask * (lse(x) - (1 - eps) * x[label] - (eps / V) * sum_{v < V} x[v])
//   dlogits[v] = mask * (gscale / den) * (softmax[v] - (1 - eps) * [v == label] - eps / V)   (v < V)
// The columns of the row-pitch padding (V <= v < ld) do not exist: they are kept out of sum x (the plain kernel's -inf marker
// would poison it) and their gradient is written as exactly 0 (dense_bwd_w contracts over the padded pitch).
// Same traffic as the plain kernel: each logit read once and written once; sum x rides in the max's block reduction.
// (The plain entry keeps kernels of its own: compiled with the smoothing taken out, this body's x * inv - m * k does not round the
// label's column as the plain kernel's branch does, and a cfg2 training step's gradients then differ in their last bits.)
template <bool REG, bool WRITE_GRAD>
__global__ __launch_bounds__(256) void xent_smooth_kernel(float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          int V, long ld, const float* __restrict__ den, float gscale,
                                                          float eps, float* __restrict__ row_loss) {
    __shared__ float sh[8];
    const long row = blockIdx.x;
    float* r = logits + row * ld;
    const int label = labels[row];
    XentRow<REG> x(r, V);
    float sx, mx = x.thread_max(&sx);
    block_max_sum(mx, sx, sh);
    const float s = block_sum<256>(x.exp_sum(mx), sh);
    const bool live = label != 0, word = label > 0 && label < V;
    const float ev = eps / (float)V;
    if (threadIdx.x == 0) {
        float l = 0.f;
        if (word) l = __logf(s) + mx - (1.f - eps) * r[label] - ev * sx;
        row_loss[row] = l;
    }
    if (WRITE_GRAD) {
        __syncthreads();  // thread 0 has read logits[label] before anyone overwrites it
        const float k = live ? gscale / den[0] : 0.f;
        const float inv = k / s, ke = k * ev, kl = k * (1.f - eps);
        x.store([=](float e) { return e * inv - ke; }, word ? label : -1, kl);
        x.zero_pitch(ld);
    }
}

// Per-dimension KL kl[n,l]: the summand of kl_rows_kernel with its -0.5.  Free bits compare this f32 value with the floor in
// the forward AND in the backward kernel, so both evaluate it through this one function with contraction off: the two kernels
// then agree on every element whatever the code around the call looks like.
__device__ __forceinline__ float kl_elem(int mode, float m, float sd, float mup) {
#pragma clang fp contract(off)
    if (mode == 0) return -0.5f * (1.f + logf(sd * sd + 1e-5f) - m * m - sd * sd);
    const float d = m - mup;
    return -0.5f * (0.5f + logf(sd + 1e-5f) - logf(VC_AG_SIGMA + 1e-5f) - (d * d + sd * sd) / (2.f * VC_AG_SIGMA * VC_AG_SIGMA + 1e-7f));
}

// Free bits (Kingma et al. 2016), per dimension and row: row_kl[n] = sum_l max(fb, kl[n,l]); beside it the unclamped sum and the
// number of dimensions held at the floor (those with kl <= fb).  One wave per row, four rows per workgroup, like kl_rows_kernel.
__global__ __launch_bounds__(256) void kl_rows_fb_kernel(const float* __restrict__ mean, const float* __restrict__ std_,
                                                         const float* __restrict__ mu_p, int N, int L, int mode, float fb,
                                                         float* __restrict__ row_kl, float* __restrict__ row_kl_raw,
                                                         int32_t* __restrict__ row_floored) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f, raw = 0.f;
    int nf = 0;
    for (int l = lane; l < L; l += 64) {
        const long j = (long)row * L + l;
        const float kl = kl_elem(mode, mean[j], std_[j], mode ? mu_p[j] : 0.f);
        raw += kl;
        if (kl > fb) {
            s += kl;
        } else {
            s += fb;
            ++nf;
        }
    }
    s = wave_sum(s);
    raw = wave_sum(raw);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if (lane == 0) {
        row_kl[row] = s;
        row_kl_raw[row] = raw;
        row_floored[row] = nf;
    }
}

// ---------------------------------------------------------------------------------------
// Gradient w.r.t. (mean, std) of   [sum over the S samples through z]  +  kl_w * KL:
//   dmean = sum_s dz[s] + dKL/dmean ;  dstd = sum_s dz[s]*eps[s] + dKL/dstd
// kl_w = ann[0] * kl_scale (device annealing coefficient x host constant: 1/10, and 1/N for
// the batch-mean Normal KL).  out_logstd: return d/d(logstd) = dstd * std (Normal heads).
// FB (free bits): a dimension held at the floor (kl <= fb, kl_rows_fb_kernel's comparison) gets no KL gradient -- its dmean / dstd
// are the sums over the samples alone.
// ---------------------------------------------------------------------------------------
template <bool FB>
__global__ __launch_bounds__(256) void latent_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ eps,
                                                         const float* __restrict__ mean, const float* __restrict__ std_,
                                                         const float* __restrict__ mu_p, const float* __restrict__ ann,
                                                         float kl_scale, float fb, int S, long NL, int mode, int out_logstd,
                                                         float* __restrict__ dmean, float* __restrict__ dstd) {
    const float w = (ann ? ann[0] : 1.f) * kl_scale;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < NL; j += (long)gridDim.x * 256) {
        // S == 0: dmean / dstd already hold the sums over the samples (vc_latent_sums_mixed_f32)
        float dm = S ? 0.f : dmean[j], ds = S ? 0.f : dstd[j];
        int s = 0;
        for (; s + 8 <= S; s += 8) {   // sixteen loads in flight, the sums in the same order as the plain loop (a thread per element is all
            float g[8], e[8];          // the parallelism N * L = 48 000 gives: with one load pair at a time the launch took 65 us at cfg4)
#pragma unroll
            for (int k = 0; k < 8; ++k) { g[k] = dz[(long)(s + k) * NL + j]; e[k] = eps[(long)(s + k) * NL + j]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { dm += g[k]; ds += g[k] * e[k]; }
        }
        for (; s < S; ++s) {
            const float g = dz[(long)s * NL + j];
            dm += g;
            ds += g * eps[(long)s * NL + j];
        }
        const float m = mean[j], sd = std_[j];
        const float mup = mode ? mu_p[j] : 0.f;
        if (!FB || kl_elem(mode, m, sd, mup) > fb) {
            if (mode == 0) {
                dm += w * m;
                ds -= w * (sd / (sd * sd + 1e-5f) - sd);
            } else {
                const float den = 2.f * VC_AG_SIGMA * VC_AG_SIGMA + 1e-7f;
                dm += w * (m - mup) / den;
                ds -= 0.5f * w * (1.f / (sd + 1e-5f) - 2.f * sd / den);
            }
        }
        dmean[j] = dm;
        dstd[j] = out_logstd ? ds * sd : ds;
    }
}

// Batch means of what kl_rows_fb_kernel leaves per row: out[0] = mean unclamped KL per row, out[1] = share of the N * L
// dimensions held at the floor.  One workgroup (N rows: a few thousand at most), fixed summation order.
__global__ __launch_bounds__(256) void objective_stats_kernel(const float* __restrict__ row_kl_raw, const int32_t* __restrict__ row_floored,
                                                              int N, int L, float* __restrict__ out) {
    __shared__ float sh[4];
    float a = 0.f, b = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        a += row_kl_raw[n];
        b += (float)row_floored[n];
    }
    a = block_sum<256>(a, sh);
    b = block_sum<256>(b, sh);
    if (threadIdx.x == 0) {
        out[0] = a / (float)N;
        out[1] = b / ((float)N * (float)L);
    }
}

// loss_finalize_kernel with the KL coefficient as an argument: out[2] = rec + ann * kl_coef * kld (kl_coef = beta / 10).
__global__ void loss_finalize_kl_kernel(const float* ce_num, const float* ce_den, const float* reg, float reg_scale,
                                        const float* kl_sum, float inv_n, const float* ann, float kl_coef, float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float rec = ce_num[0] / ce_den[0];
    if (reg) rec += reg[0] * reg_scale;
    const float a = ann ? ann[0] : 1.f;
    const float kld = kl_sum ? kl_sum[0] * inv_n : 0.f;
    out[0] = rec;
    out[1] = kld;
    out[2] = kl_sum ? rec + a * kl_coef * kld : rec;
    out[3] = a;
}

// =======================================================================================
// Self-critical training (DESIGN.md "Self-critical training"): the policy-gradient loss of SAMPLED captions.  Rows are time-major
// [T, N]; row r belongs to caption n = r % N, whose advantage adv[n] weights the log-probability of every token it took:
//   J = scale * sum over live rows ( -adv[n] * log p(label) - beta * H ),   H = lse - sum_v p_v x_v  (the row's entropy)
//   row_lp = live * (x[label] - lse),  row_ent = live * H
//   dlogits[v] = live * scale * ( adv[n] * (p_v - [v == label]) + beta * p_v * ((x_v - lse) + H) )   (v < V), exactly 0 for V <= v < ld
// live = 0 < label < V.  The row is held as d_v = x_v - max (ENT) or exp(d_v) (plain): with H = log s - (sum_v e^d_v d_v) / s and
// x_v - lse = d_v - log s nothing is ever the logarithm of a probability, so an underflowed p_v adds exactly 0.  ENT = false
// (beta == 0) compiles the entropy arithmetic away: the kernel is then xent_smooth_kernel's at eps = 0 with a per-row scale.
// The second launch bound is the waves per SIMD the register form runs at (4 with the entropy terms, 6 without, 8 without a gradient):
// left to itself the scheduler spends 11 to 16 more registers on the ENT = false forms and loses a wave.
// =======================================================================================
template <bool REG, bool WRITE_GRAD, bool ENT>
__global__ __launch_bounds__(256, ENT ? 4 : (WRITE_GRAD ? 6 : 8))
void xent_policy_kernel(float* __restrict__ logits, const int32_t* __restrict__ labels, int V, long ld,
                        const float* __restrict__ adv, int N, float scale, float beta, float* __restrict__ row_lp,
                        float* __restrict__ row_ent) {
    __shared__ float sh[4];
    const long row = blockIdx.x;
    float* r = logits + row * ld;
    const int label = labels[row];
    XentRow<REG, ENT> x(r, V);
    const float mx = block_max<256>(x.thread_max(), sh);
    float sd = 0.f;   // sum e^d * d
    const float s = block_sum<256>(x.exp_sum(mx, ENT ? &sd : nullptr), sh);
    if (ENT) sd = block_sum<256>(sd, sh);
    const bool live = label > 0 && label < V;
    const float logs = __logf(s);
    const float H = ENT ? logs - sd / s : 0.f;
    if (threadIdx.x == 0) {
        row_lp[row] = live ? (r[label] - mx) - logs : 0.f;
        if (ENT) row_ent[row] = live ? H : 0.f;
    }
    if (WRITE_GRAD) {
        __syncthreads();  // thread 0 has read logits[label] before anyone overwrites it
        const float ka = live ? scale * adv[row % N] : 0.f, kb = live ? scale * beta : 0.f;
        const float inv = 1.f / s, hb = H - logs;
        if (ENT) {   // p_v * (ka + kb * ((d_v - log s) + H)); p_v == 0 -> exactly 0 (a masked lane's d is -inf)
            x.store([=](float d) { const float pv = __expf(d) * inv; return pv > 0.f ? pv * (ka + kb * (d + hb)) : 0.f; }, live ? label : -1, ka);
        } else if (REG) {
            const float k = ka * inv;
            x.store([=](float e) { return e * k; }, live ? label : -1, ka);
        } else {   // (the memory form has always rounded e * inv first: p_v * ka, not e_v * (ka / s))
            x.store([=](float e) { return e * inv * ka; }, live ? label : -1, ka);
        }
        x.zero_pitch(ld);
    }
}

// =======================================================================================
// Unlikelihood training (DESIGN.md "Unlikelihood training"; Welleck et al. 2020, token level): the smoothed cross-entropy of
// xent_smooth_kernel plus alpha * sum_{c in C} -log(1 - p_c) over the row's candidate set C, the distinct words of the same caption's
// up to `window` earlier labels (rows are time-major, r = t * N + n) that are words (0 < c < V) and not the row's own label y.
//   om_c = 1 - p_c; a candidate with om_c <= 1e-5 is CLAMPED: it adds -log(1e-5) to row_ul and nothing to the gradient (torch.clamp);
//   r_c = p_c / om_c otherwise, R = sum_c r_c.  live = 0 < y < V, k = live * gscale / den:
//   row_loss = the smoothed kernel's (cross-entropy alone); row_ul = live * sum_c -log(max(om_c, 1e-5)); row_cand = live * |C|;
//   row_mass = live * sum_c p_c;  d[v] = k * (p_v * (1 - alpha * R) - (1 - eps) [v == y] - eps / V + alpha * r_v [v in C, unclamped]).
// How the hazards of doing this in place are handled, in both forms of the row:
//   * thread i < min(window, t) owns the label i + 1 steps back.  It reads that label, and -- before anything else is waited for -- the
//     logit x_c of it; thread 0 reads x_y likewise.  All of these loads stand in front of the block reductions, whose barriers every
//     thread passes before the first store to the row: no x_c or x_y can see a gradient.
//   * duplicates: the raw candidates go to LDS, and behind the barriers of the first reduction a thread drops its word when a thread
//     with a smaller index holds the same one.  No compaction, no host-built table; t = 0 (and a PAD row) has no owner threads at all.
//   * the row is scaled and stored as the smoothed kernel does it (p_v * (1 - alpha * R) in place of p_v; label column patched branch-free
//     by the thread that stores it), padding columns and quads written as exact zeros by the threads that stored them.  The candidate
//     columns are NOT patched inside those vector stores: behind one more workgroup barrier (the vector stores of other threads must be
//     ordered before it) the owner thread stores its column's complete value, one float.  A candidate is never the label (excluded)
//     and two owners never hold the same word (dedupe), so a candidate sharing its float4 with the label, with another candidate or
//     with the pitch padding of the last quad (V % 4 != 0) is simply another 4-byte store to an address nobody else writes after the
//     barrier; the padding stays the zeros its owner wrote (c < V).
// Traffic: the smoothed kernel's 4 B read + 4 B written per logit, plus at most 128 label reads, 128 scattered 4-byte reads and 128
// scattered 4-byte writes per row.
// =======================================================================================
constexpr int UL_MAXW = 128;
#define VC_UL_CLAMP 1e-5f

// number of owner threads of row `row`: min(window, t), none for a row that is not live
__device__ __forceinline__ int ul_owners(long row, int N, int window, bool live) {
    const long t = row / N;
    return live ? (int)(t < (long)window ? t : (long)window) : 0;
}
// thread i < owners: the label i + 1 steps back in the same caption, -1 unless it is a word other than y; left in cand[i] for ul_first
__device__ __forceinline__ int ul_load(const int32_t* __restrict__ labels, long row, int N, int V, int owners, int y, int* cand /* UL_MAXW */) {
    int c = -1;
    if ((int)threadIdx.x < owners) {
        c = labels[row - (long)(threadIdx.x + 1) * N];
        if (c <= 0 || c >= V || c == y) c = -1;
        cand[threadIdx.x] = c;
    }
    return c;
}
// (behind a barrier) keep the word only in the owner with the smallest index
__device__ __forceinline__ int ul_first(int c, const int* cand) {
    if (c >= 0)
        for (int j = 0; j < (int)threadIdx.x; ++j)
            if (cand[j] == c) { c = -1; break; }
    return c;
}
// one candidate's terms from e_c = exp(x_c - max) and s = sum exp: -log(max(om, clamp)), p_c, r_c (0 when clamped)
__device__ __forceinline__ void ul_terms(float ec, float s, float& ul, float& pc, float& rc) {
    pc = ec / s;
    const float om = 1.f - pc;
    const bool clamped = om <= VC_UL_CLAMP;
    ul = clamped ? -logf(VC_UL_CLAMP) : -log1pf(-pc);
    rc = clamped ? 0.f : pc / om;
}

template <bool REG, bool WRITE_GRAD>
__global__ __launch_bounds__(256) void xent_ul_kernel(float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                      int V, long ld, const float* __restrict__ den, float gscale,
                                                      float eps, int N, float alpha, int window, float* __restrict__ row_loss,
                                                      float* __restrict__ row_ul, int32_t* __restrict__ row_cand,
                                                      float* __restrict__ row_mass) {
    __shared__ float sh[16];
    __shared__ int cand[UL_MAXW];
    const long row = blockIdx.x;
    float* r = logits + row * ld;
    const int label = labels[row];
    const bool live = label > 0 && label < V;
    XentRow<REG> x(r, V);
    int c = ul_load(labels, row, N, V, ul_owners(row, N, window, live), label, cand);
    const float xc = c >= 0 ? r[c] : 0.f;                            // (a duplicate reads its word's logit too: dropped below)
    const float xy = (threadIdx.x == 0 && live) ? r[label] : 0.f;
    float sx, mx = x.thread_max(&sx);
    block_max_sum(mx, sx, sh);   // (its barriers stand between ul_load's cand[] writes and ul_first's reads)
    c = ul_first(c, cand);
    const float s = block_sum<256>(x.exp_sum(mx), sh);
    float ec = 0.f, ul = 0.f, mass = 0.f, rc = 0.f, R, cnt = 0.f;
    if (c >= 0) {
        ec = __expf(xc - mx);
        ul_terms(ec, s, ul, mass, rc);
        cnt = 1.f;
    }
    R = rc;
    block_sum4(ul, mass, R, cnt, sh);   // every x_c and x_y has been read in front of these barriers: the stores below come behind them
    const float ev = eps / (float)V;
    if (threadIdx.x == 0) {
        row_loss[row] = live ? __logf(s) + mx - (1.f - eps) * xy - ev * sx : 0.f;
        row_ul[row] = ul;
        row_cand[row] = (int32_t)cnt;
        row_mass[row] = mass;
    }
    if (WRITE_GRAD) {
        const float k = live ? gscale / den[0] : 0.f;
        const float inv = k * (1.f - alpha * R) / s, ke = k * ev, kl = k * (1.f - eps);
        x.store([=](float e) { return e * inv - ke; }, live ? label : -1, kl);
        x.zero_pitch(ld);
        __syncthreads();   // the candidate columns were vector-stored by other threads: their owners write them behind this barrier
        if (c >= 0) r[c] = (ec * inv - ke) + k * alpha * rc;
    }
}

// =======================================================================================
// Bag-of-words auxiliary loss (DESIGN.md "Bag-of-words loss"; Zhao, Zhao & Eskenazi 2017): the multi-label member of the family.  One
// row of logits per CAPTION n; its targets are the bag of the caption's words, read from the step's time-major labels
// (labels[t * ldl + n], 0 <= t < T <= 256), PAD and ids outside (0, V) left out.  m = the bag's size with multiplicity, c_w = the count
// of word w, p = softmax over the V real columns, k = gscale / den:
//   row_loss = m * lse(x) - sum_w c_w x_w;  row_mass = sum over the DISTINCT bag words of p_w;  row_words = their number;
//   d[v] = k * (m * p_v - c_v) for v < V, exactly 0 in the pitch padding; a row with m = 0 comes back all-zero.
// In place, with the means of xent_ul_kernel:
//   * thread i < T owns position i.  It reads its word and that word's logit x_w in front of the first block reduction, whose barriers
//     every thread passes before the first store to the row: no x_w can see a gradient.  The words go to LDS.
//   * behind those barriers an owner KEEPS its word only if no lower-indexed owner holds it (bow_keep); the keeper counts the word's
//     multiplicity over the owners behind it.  Two keepers never hold the same word.
//   * the vector stores write k * m * p_v everywhere; behind one more workgroup barrier each keeper stores its column's complete value
//     k * (m * p_w - c_w) as one float.  A bag word that shares its float4 with another bag word, or with the last quad's padding
//     (V % 4 != 0), is still a single writer behind that barrier; the padding stays the zeros the vector store wrote (w < V).
// Traffic: 4 B read + 4 B written per logit, plus at most T label reads, T scattered 4-byte reads and T scattered 4-byte writes a row.
// =======================================================================================
constexpr int BOW_MAXT = 256;

// thread i: the word at position i of caption `row`, -1 unless 0 < word < V (and for i >= T); left in bag[i] for bow_keep
__device__ __forceinline__ int bow_load(const int32_t* __restrict__ labels, long row, int T, long ldl, int V, int* bag /* BOW_MAXT */) {
    int w = -1;
    if ((int)threadIdx.x < T) {
        w = labels[(long)threadIdx.x * ldl + row];
        if (w <= 0 || w >= V) w = -1;
    }
    bag[threadIdx.x] = w;
    return w;
}
// (behind a barrier) the multiplicity c_w of the thread's word if it is the word's first owner, 0 otherwise (and for w < 0)
__device__ __forceinline__ int bow_keep(int w, int T, const int* bag) {
    if (w < 0) return 0;
    for (int j = 0; j < (int)threadIdx.x; ++j)
        if (bag[j] == w) return 0;
    int cnt = 1;
    for (int j = threadIdx.x + 1; j < T; ++j) cnt += bag[j] == w ? 1 : 0;
    return cnt;
}

template <bool REG, bool WRITE_GRAD>
__global__ __launch_bounds__(256) void bow_xent_kernel(float* __restrict__ logits, int V, long ld, const int32_t* __restrict__ labels,
                                                       int T, long ldl, const float* __restrict__ den, float gscale,
                                                       float* __restrict__ row_loss, float* __restrict__ row_mass,
                                                       int32_t* __restrict__ row_words) {
    __shared__ float sh[16];
    __shared__ int bag[BOW_MAXT];
    const long row = blockIdx.x;
    float* r = logits + row * ld;
    XentRow<REG> x(r, V);
    const int w = bow_load(labels, row, T, ldl, V, bag);
    const float xw = w >= 0 ? r[w] : 0.f;                            // (a duplicate reads its word's logit too: dropped below)
    const float mx = block_max<256>(x.thread_max(), sh);   // (its barriers stand between bow_load's bag[] writes and bow_keep's reads)
    const int cw = bow_keep(w, T, bag);
    const float s = block_sum<256>(x.exp_sum(mx), sh);
    const float ec = cw > 0 ? __expf(xw - mx) : 0.f;
    float m = w >= 0 ? 1.f : 0.f, cx = (float)cw * (xw - mx), mass = ec / s, words = cw > 0 ? 1.f : 0.f;
    block_sum4(m, cx, mass, words, sh);   // every x_w has been read in front of these barriers: the stores below come behind them
    if (threadIdx.x == 0) {
        row_loss[row] = m > 0.f ? m * __logf(s) - cx : 0.f;
        row_mass[row] = mass;
        row_words[row] = (int32_t)words;
    }
    if (WRITE_GRAD) {
        const float k = m > 0.f ? gscale / den[0] : 0.f;
        const float inv = k * m / s;
        x.store([=](float e) { return e * inv; }, -1, 0.f);
        x.zero_pitch(ld, /*last_quad=*/false);   // (the last quad's masked lanes were stored as 0 * inv)
        __syncthreads();   // the bag columns were vector-stored by other threads: their keepers write them behind this barrier
        if (cw > 0) r[w] = ec * inv - k * (float)cw;
    }
}

// What vc_bow_xent_f32 leaves per row, as the three reported numbers of this call's rows, sums in fixed order: out3 = {sum row_loss /
// sum m, sum row_words / #non-empty, sum row_mass / #non-empty}, m counted from the labels (zeros when every bag is empty).  One workgroup.
__global__ __launch_bounds__(256) void bow_stats_kernel(const int32_t* __restrict__ labels, int T, long ldl, int V, const float* __restrict__ row_loss,
                                                        const float* __restrict__ row_mass, const int32_t* __restrict__ row_words,
                                                        long rows, float* __restrict__ out) {
    __shared__ float sh[16];
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f, m = 0.f;
    for (long i = threadIdx.x; i < rows; i += 256) {
        a += row_loss[i];
        b += (float)row_words[i];
        c += row_mass[i];
        d += row_words[i] > 0 ? 1.f : 0.f;
        for (int t = 0; t < T; ++t) {
            const int w = labels[(long)t * ldl + i];
            m += (w > 0 && w < V) ? 1.f : 0.f;
        }
    }
    block_sum4(a, b, c, d, sh);
    m = block_sum<256>(m, sh);
    if (threadIdx.x == 0) {
        const float inv = d > 0.f ? 1.f / d : 0.f;
        out[0] = m > 0.f ? a / m : 0.f;
        out[1] = b * inv;
        out[2] = c * inv;
    }
}

}  // namespace vc

using namespace vc;

// The dispatch of the in-place cross-entropy family: the register form of the row where it fits, the gradient compiled in or out.
// `launch` is a generic lambda that receives REG and WRITE_GRAD as std::bool_constant values and launches that instantiation.
template <class F>
static inline void xent_dispatch(const float* logits, int V, long ld, int write_grad, F launch) {
    if (xent_row_in_registers(logits, V, ld)) {
        if (write_grad) launch(std::true_type(), std::true_type()); else launch(std::true_type(), std::false_type());
    } else {
        if (write_grad) launch(std::false_type(), std::true_type()); else launch(std::false_type(), std::false_type());
    }
}

extern "C" int vc_loss_finalize_f32(void* stream, const float* ce_num, const float* ce_den, const float* reg_sumsq,
                                    float reg_scale, const float* kl_sum, float inv_n, const float* ann, float* out4) {
    VC_CHECK_ARG(ce_num && ce_den && out4, "null pointer");
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ce_num, ce_den, reg_sumsq, reg_scale, kl_sum, inv_n, ann, out4);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_softmax_xent_f32(void* stream, float* logits, const int32_t* labels, long rows, int V, long ld,
                                   const float* den, float gscale, float* row_loss, int write_grad) {
    VC_CHECK_ARG(logits && labels && row_loss && rows >= 0 && V > 0 && ld >= V, "bad argument");
    VC_CHECK_ARG(!write_grad || den, "den required for the gradient");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    xent_dispatch(logits, V, ld, write_grad, [&](auto R, auto W) {
        auto* kernel = decltype(R)::value ? xent_reg_kernel<decltype(W)::value> : xent_mem_kernel<decltype(W)::value>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(256), 0, st, logits, labels, V, ld, den, gscale, row_loss);
    });
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_softmax_rows_f32(void* stream, const float* x, long rows, int V, long ld, float* y, long ldy) {
    VC_CHECK_ARG(x && y && rows >= 0 && V > 0 && ld >= V && ldy >= V, "bad argument");
    if (rows == 0) return 0;
    if ((V & 3) == 0 && V <= 12288 && (ld & 3) == 0 && (ldy & 3) == 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0)
        hipLaunchKernelGGL(softmax_rows_reg_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, V, ld, y, ldy);
    else
        hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, V, ld, y, ldy);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_multinomial_rows_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature,
                                       const float* u, int32_t* out) {
    VC_CHECK_ARG(logits && u && out && rows >= 0 && V > 0 && ld >= V && temperature > 0.f, "bad argument");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(multinomial_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, V, ld, 1.0f / temperature, u, out);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_latent_sample_f32(void* stream, int S, int N, int L, const float* mean, const float* std_,
                                    const float* eps, float* z) {
    VC_CHECK_ARG(mean && std_ && eps && z && S > 0 && N > 0 && L > 0, "bad argument");
    const long NL = (long)N * L, total = NL * S;
    hipLaunchKernelGGL(sample_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, mean, std_, eps, NL, total, z);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_latent_sample_mixed_f32(void* stream, int Ng, int L, long q0, long nq, const float* mean_g,
                                          const float* std_g, const float* eps, float* z) {
    VC_CHECK_ARG(mean_g && std_g && eps && z && Ng > 0 && L > 0 && q0 >= 0 && nq > 0, "bad argument");
    const long total = nq * L;
    hipLaunchKernelGGL(sample_mixed_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, mean_g, std_g, eps, Ng, L, q0, total, z);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_latent_sums_mixed_f32(void* stream, int Ng, int L, long q0, long nq, const float* dz, const float* eps,
                                        float* dmean_part, float* dstd_part) {
    VC_CHECK_ARG(dz && eps && dmean_part && dstd_part && Ng > 0 && L > 0 && q0 >= 0 && nq > 0, "bad argument");
    hipLaunchKernelGGL(latent_sums_mixed_kernel, dim3(grid_for((long)Ng * L)), dim3(256), 0, (hipStream_t)stream, dz, eps, Ng, L, q0, nq, dmean_part, dstd_part);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_kl_rows_f32(void* stream, int N, int L, int mode, const float* mean, const float* std_,
                              const float* mu_p, float* row_kl) {
    VC_CHECK_ARG(mean && std_ && row_kl && N > 0 && L > 0 && (mode == 0 || (mode == 1 && mu_p)), "bad argument");
    hipLaunchKernelGGL(kl_rows_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, mean, std_, mu_p, N, L, mode, row_kl);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_latent_bwd_f32(void* stream, int S, int N, int L, int mode, int out_logstd, const float* dz,
                                 const float* eps, const float* mean, const float* std_, const float* mu_p,
                                 const float* ann, float kl_scale, float* dmean, float* dstd) {
    VC_CHECK_ARG(mean && std_ && dmean && dstd && S >= 0 && (S == 0 || (dz && eps)) && N > 0 && L > 0, "bad argument");
    VC_CHECK_ARG(mode == 0 || (mode == 1 && mu_p), "mu_p required for the AG prior");
    const long NL = (long)N * L;
    hipLaunchKernelGGL(latent_bwd_kernel<false>, dim3(grid_for(NL)), dim3(256), 0, (hipStream_t)stream, dz, eps, mean, std_, mu_p, ann,
                       kl_scale, 0.f, S, NL, mode, out_logstd, dmean, dstd);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_heads_mix_fwd_f32(void* stream, int N, int K, int L, const float* heads, const float* c_i,
                                    const int32_t* idx, float* mean, float* std_) {
    VC_CHECK_ARG(heads && mean && std_ && (c_i || idx) && N > 0 && K > 0 && L > 0, "bad argument");
    hipLaunchKernelGGL(heads_mix_fwd_kernel, dim3(grid_for((long)N * L)), dim3(256), 0, (hipStream_t)stream, heads, c_i, idx, N, K, L, mean, std_);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_heads_mix_bwd_f32(void* stream, int N, int K, int L, const float* heads, const float* c_i,
                                    const int32_t* idx, const float* dmean, const float* dstd, float* dheads) {
    VC_CHECK_ARG(heads && dmean && dstd && dheads && (c_i || idx) && N > 0 && K > 0 && L > 0, "bad argument");
    hipLaunchKernelGGL(heads_mix_bwd_kernel, dim3(grid_for((long)N * K * L)), dim3(256), 0, (hipStream_t)stream, heads, c_i, idx, dmean, dstd, N, K, L, dheads);
    VC_LAUNCH_CHECK();
    return 0;
}

// ---- training objective options (each beside its plain entry above)
extern "C" int vc_softmax_xent_smooth_f32(void* stream, float* logits, const int32_t* labels, long rows, int V, long ld,
                                          const float* den, float gscale, float eps, float* row_loss, int write_grad) {
    VC_CHECK_ARG(logits && labels && row_loss && rows >= 0 && V > 0 && ld >= V, "bad argument");
    VC_CHECK_ARG(!write_grad || den, "den required for the gradient");
    VC_CHECK_ARG(eps >= 0.f && eps < 1.f, "eps must be in [0, 1)");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    xent_dispatch(logits, V, ld, write_grad, [&](auto R, auto W) {
        hipLaunchKernelGGL((xent_smooth_kernel<decltype(R)::value, decltype(W)::value>), dim3((unsigned)rows), dim3(256), 0, st,
                           logits, labels, V, ld, den, gscale, eps, row_loss);
    });
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_kl_rows_fb_f32(void* stream, int N, int L, int mode, const float* mean, const float* std_, const float* mu_p,
                                 float free_bits, float* row_kl, float* row_kl_raw, int32_t* row_floored) {
    VC_CHECK_ARG(mean && std_ && row_kl && row_kl_raw && row_floored && N > 0 && L > 0 && (mode == 0 || (mode == 1 && mu_p)), "bad argument");
    hipLaunchKernelGGL(kl_rows_fb_kernel, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, mean, std_, mu_p, N, L, mode, free_bits,
                       row_kl, row_kl_raw, row_floored);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_latent_bwd_fb_f32(void* stream, int S, int N, int L, int mode, int out_logstd, const float* dz, const float* eps,
                                    const float* mean, const float* std_, const float* mu_p, const float* ann, float kl_scale,
                                    float free_bits, float* dmean, float* dstd) {
    VC_CHECK_ARG(mean && std_ && dmean && dstd && S >= 0 && (S == 0 || (dz && eps)) && N > 0 && L > 0, "bad argument");
    VC_CHECK_ARG(mode == 0 || (mode == 1 && mu_p), "mu_p required for the AG prior");
    const long NL = (long)N * L;
    hipLaunchKernelGGL(latent_bwd_kernel<true>, dim3(grid_for(NL)), dim3(256), 0, (hipStream_t)stream, dz, eps, mean, std_, mu_p, ann,
                       kl_scale, free_bits, S, NL, mode, out_logstd, dmean, dstd);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_objective_stats_f32(void* stream, int N, int L, const float* row_kl_raw, const int32_t* row_floored, float* out2) {
    VC_CHECK_ARG(row_kl_raw && row_floored && out2 && N > 0 && L > 0, "bad argument");
    hipLaunchKernelGGL(objective_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_kl_raw, row_floored, N, L, out2);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_loss_finalize_kl_f32(void* stream, const float* ce_num, const float* ce_den, const float* reg_sumsq, float reg_scale,
                                       const float* kl_sum, float inv_n, const float* ann, float kl_coef, float* out4) {
    VC_CHECK_ARG(ce_num && ce_den && out4, "null pointer");
    hipLaunchKernelGGL(loss_finalize_kl_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ce_num, ce_den, reg_sumsq, reg_scale, kl_sum, inv_n,
                       ann, kl_coef, out4);
    VC_LAUNCH_CHECK();
    return 0;
}

// ---- self-critical training: the policy-gradient loss (beta == 0 runs the kernels without
// the entropy arithmetic, row_ent may then be NULL)
extern "C" int vc_softmax_xent_policy_f32(void* stream, float* logits, const int32_t* labels, long rows, int V, long ld,
                                          const float* adv, int N, float scale, float beta, float* row_lp, float* row_ent, int write_grad) {
    VC_CHECK_ARG(logits && labels && adv && row_lp && rows >= 0 && V > 0 && ld >= V, "bad argument");
    VC_CHECK_ARG(N > 0 && rows % N == 0, "rows must be a multiple of N (time-major [T, N] rows)");
    VC_CHECK_ARG(beta >= 0.f && beta < INFINITY && scale == scale && fabsf(scale) < INFINITY, "beta must be finite and >= 0, scale finite");
    VC_CHECK_ARG(beta == 0.f || row_ent, "row_ent required with beta > 0");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    xent_dispatch(logits, V, ld, write_grad, [&](auto R, auto W) {
        constexpr bool REG = decltype(R)::value, WG = decltype(W)::value;
        auto* kernel = beta > 0.f ? xent_policy_kernel<REG, WG, true> : xent_policy_kernel<REG, WG, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(256), 0, st, logits, labels, V, ld, adv, N, scale, beta, row_lp, row_ent);
    });
    VC_LAUNCH_CHECK();
    return 0;
}

// ---- unlikelihood training: the smoothed cross-entropy with the repetition penalty in the same pass
extern "C" int vc_softmax_xent_ul_f32(void* stream, float* logits, const int32_t* labels, long rows, int N, int V, long ld,
                                      const float* den, float gscale, float eps, float alpha, int window, float* row_loss,
                                      float* row_ul, int32_t* row_cand, float* row_mass, int write_grad) {
    VC_CHECK_ARG(logits && labels && row_loss && rows >= 0 && V > 0 && ld >= V, "bad argument");
    VC_CHECK_ARG(!write_grad || den, "den required for the gradient");
    VC_CHECK_ARG(eps >= 0.f && eps < 1.f, "eps must be in [0, 1)");
    VC_CHECK_ARG(row_ul && row_cand && row_mass, "row_ul, row_cand and row_mass required");
    VC_CHECK_ARG(window >= 1 && window <= UL_MAXW, "window must be in 1..128");
    VC_CHECK_ARG(alpha > 0.f && alpha < INFINITY, "alpha must be finite and > 0");
    VC_CHECK_ARG(N > 0 && rows % N == 0, "rows must be a multiple of N (time-major [T, N] rows)");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    xent_dispatch(logits, V, ld, write_grad, [&](auto R, auto W) {
        hipLaunchKernelGGL((xent_ul_kernel<decltype(R)::value, decltype(W)::value>), dim3((unsigned)rows), dim3(256), 0, st,
                           logits, labels, V, ld, den, gscale, eps, N, alpha, window, row_loss, row_ul, row_cand, row_mass);
    });
    VC_LAUNCH_CHECK();
    return 0;
}

// What vc_softmax_xent_ul_f32 leaves per row, as three means over the live rows (0 < label < V) of the call, sums in fixed order:
// out3 = {sum row_ul, sum row_cand, sum row_mass} / #live (zeros when no row is live).  One workgroup.
namespace vc {
__global__ __launch_bounds__(256) void ul_stats_kernel(const int32_t* __restrict__ labels, int V, const float* __restrict__ row_ul,
                                                       const int32_t* __restrict__ row_cand, const float* __restrict__ row_mass,
                                                       long rows, float* __restrict__ out) {
    __shared__ float sh[16];
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
    for (long i = threadIdx.x; i < rows; i += 256) {
        a += row_ul[i];
        b += (float)row_cand[i];
        c += row_mass[i];
        d += (labels[i] > 0 && labels[i] < V) ? 1.f : 0.f;
    }
    block_sum4(a, b, c, d, sh);
    if (threadIdx.x == 0) {
        const float inv = d > 0.f ? 1.f / d : 0.f;
        out[0] = a * inv;
        out[1] = b * inv;
        out[2] = c * inv;
    }
}
}  // namespace vc

extern "C" int vc_ul_stats_f32(void* stream, long rows, int V, const int32_t* labels, const float* row_ul, const int32_t* row_cand,
                               const float* row_mass, float* out3) {
    VC_CHECK_ARG(labels && row_ul && row_cand && row_mass && out3 && rows > 0 && V > 0, "bad argument");
    hipLaunchKernelGGL(ul_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, labels, V, row_ul, row_cand, row_mass, rows, out3);
    VC_LAUNCH_CHECK();
    return 0;
}

// ---- bag-of-words auxiliary loss: one row of logits per caption against the bag of its words
extern "C" int vc_bow_xent_f32(void* stream, float* logits, long rows, int V, long ld, const int32_t* labels, int T, long ldl,
                               const float* den, float gscale, float* row_loss, float* row_mass, int32_t* row_words, int write_grad) {
    VC_CHECK_ARG(logits && labels && row_loss && row_mass && row_words, "null pointer");
    VC_CHECK_ARG(rows >= 0 && V > 0 && ld >= V, "bad argument");
    VC_CHECK_ARG(T >= 1 && T <= BOW_MAXT, "T must be in 1..256 (one caption position per thread)");
    VC_CHECK_ARG(ldl >= rows, "ldl must be >= rows (labels are time-major [T, ldl])");
    VC_CHECK_ARG(!write_grad || den, "den required for the gradient");
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    xent_dispatch(logits, V, ld, write_grad, [&](auto R, auto W) {
        hipLaunchKernelGGL((bow_xent_kernel<decltype(R)::value, decltype(W)::value>), dim3((unsigned)rows), dim3(256), 0, st,
                           logits, V, ld, labels, T, ldl, den, gscale, row_loss, row_mass, row_words);
    });
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_bow_stats_f32(void* stream, long rows, int V, const int32_t* labels, int T, long ldl, const float* row_loss,
                                const float* row_mass, const int32_t* row_words, float* out3) {
    VC_CHECK_ARG(labels && row_loss && row_mass && row_words && out3 && rows > 0 && V > 0 && T >= 1 && ldl >= rows, "bad argument");
    hipLaunchKernelGGL(bow_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, labels, T, ldl, V, row_loss, row_mass, row_words, rows, out3);
    VC_LAUNCH_CHECK();
    return 0;
}
