// Optimiser-side kernels (ops/optimizers.py): global-norm clip, Adam / SGD / Momentum
// over flat parameter buffers, device-resident step scalars (so a captured hipGraph can be
// replayed without host-side argument changes), and the Philox4x32-10 generator that
// replaces TF's random_normal / dropout streams.
//
// HBM-bound: Adam touches 4 reads + 3 writes x 4 B = 28 B per parameter; with the parameter average folded in (EMA) one more
// stream is read and written: 36 B.  A stand-alone averaging pass behind the update moves 12 B of its own (40 B for the pair).
#include "common.h"
#include <stdlib.h>
#include "vaecap.h"

namespace vc {

static inline int grid_for(long work_items, int per_block = 256, int cap = 2048) {
    long b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

constexpr int SUMSQ_BLOCKS = 512;

// Workgroups of an Adam launch (grid-stride, all resident at once; 256 / 512 / 1024 measured no better: HISTORY.md section R)
static inline int adam_grid(long n) { return grid_for(n / 4 + 1, 256, 2048); }

// partial[b] = sum over a fixed grid-stride slice of x^2: deterministic for a fixed n.
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long n, float* __restrict__ partial) {
    __shared__ float sh[4];
    float s = 0.f;
    const long n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = x4[i];
        s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += x[i] * x[i];
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// tf.clip_by_global_norm (ops/optimizers.py:15-16; TF-sem.): norm = sqrt(sum), scale =
// clip * min(1/norm, 1/clip).  out[0] = norm, out[1] = scale.
__global__ __launch_bounds__(256) void clip_finalize_kernel(const float* __restrict__ partial, int np,
                                                            float clip, float* __restrict__ out) {
    __shared__ float sh[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) s += partial[i];
    s = block_sum<256>(s, sh);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(s);
        out[0] = norm;
        out[1] = norm > 0.f ? clip * fminf(1.f / norm, 1.f / clip) : 1.f;
    }
}

// Device-resident step bookkeeping.  step[0] = global_step BEFORE this step (the value the
// reference feeds to `anneal`, main.py:237-238).  Writes
//   s[0] Adam lr_t (non-CNN)   = lr * sqrt(1-b2^t)/(1-b1^t), t = step+1   (TF-sem.)
//   s[1] annealing coefficient = (tanh((step - 1000*ann_param)/1000)+1)/2 or 1 (main.py:163-170)
//   s[2] staircase-decayed lr  = lr * 0.5^floor(step/decay_steps)        (ops/optimizers.py:24-31)
//   s[3] Adam lr_t (CNN), s[4] staircase-decayed CNN lr
// then increments step.
__global__ void step_update_kernel(int32_t* step, float* s, float lr, float cnn_lr, float beta1, float beta2,
                                   float ann_param, int ann_on, int decay_steps) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int gs = step[0];
    const float t = (float)(gs + 1);
    const float corr = sqrtf(1.f - powf(beta2, t)) / (1.f - powf(beta1, t));
    s[0] = lr * corr;
    s[1] = ann_on ? (tanhf(((float)gs - 1000.f * ann_param) / 1000.f) + 1.f) * 0.5f : 1.f;
    const float dec = powf(0.5f, (float)(decay_steps > 0 ? gs / decay_steps : 0));
    s[2] = lr * dec;
    s[3] = cnn_lr * corr;
    s[4] = cnn_lr * dec;
    step[0] = gs + 1;
}

// Cyclical KL annealing (Fu et al. 2019), launched BEHIND step_update_kernel (which has already incremented step): overwrites s[1] only,
//   ann = min(1, (gs mod P) / (R * P))  while gs < M * P or M == 0,  1 afterwards      (gs = the step counter before this step)
// computed from the device counter like the tanh schedule, so a captured step keeps advancing it.
__global__ void cyclical_ann_kernel(const int32_t* step, float* s, int period, float ramp, int cycles) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int gs = step[0] - 1;
    float a = 1.f;
    if (cycles == 0 || (long)gs < (long)cycles * period) a = fminf(1.f, (float)(gs % period) / (ramp * (float)period));
    s[1] = a;
}

// Exponential moving average of the parameters (tf.train.ExponentialMovingAverage with num_updates): the weight of the new value is
//   w = max(1 - decay, 9 / (10 + t))      [= 1 - min(decay, (1 + t) / (10 + t))],  t = step[0] = updates including this one
// (step_update_kernel has already incremented the counter when an optimiser runs), or 1 - decay with a null step.  The host passes
// omd = 1 - decay computed in double: 1.f - 0.9999f is off by 1.7e-4 relative.  Read from the device counter, so a captured step replays.
__device__ __forceinline__ float ema_weight(float omd, const int32_t* __restrict__ step) {
    return step ? fmaxf(omd, 9.f / (10.f + (float)step[0])) : omd;
}
// e += w * (p_new - e) with an explicit fma: every kernel that applies it (adam_kernel<., true>, ema_kernel) produces the same bits
__device__ __forceinline__ float ema_apply(float w, float p_new, float e) { return fmaf(w, p_new - e, e); }
__device__ __forceinline__ void ema_apply4(float w, const float4& p, float4& e) {
    e.x = ema_apply(w, p.x, e.x); e.y = ema_apply(w, p.y, e.y);
    e.z = ema_apply(w, p.z, e.z); e.w = ema_apply(w, p.w, e.w);
}

// tf.train.AdamOptimizer.apply_gradients (ops/optimizers.py:37-40,72-75; TF-sem.):
//   g' = g*scale (+ l2*p);  m = b1*m + (1-b1)*g';  v = b2*v + (1-b2)*g'^2;  p -= lr_t*m/(sqrt(v)+eps)
// SUMSQ: also leaves sum(p_new^2) of the block in sumsq_partial[blockIdx.x] -- the regulariser's loss term of the NEXT step
// (main.py:69-74 sums w^2 over the cnn/* variables) without another 0.5 GB pass over the parameters.
// EMA: also folds the new parameters into their moving average `ema` (ema_apply above): one more float4 stream, read and written, in
// each of the three loops; p, m, v and the sums are those of the EMA = false instantiation to the bit (the same `upd` on the same data).
template <bool SUMSQ, bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, const float* __restrict__ lr_t,
                                                   const float* __restrict__ scale, float beta1, float beta2, float eps,
                                                   float l2, float* __restrict__ sumsq_partial, float* __restrict__ ema, float omd,
                                                   const int32_t* __restrict__ step) {
    __shared__ float sh[4];
    float s2 = 0.f;
    const float lr = lr_t[0];
    const float w = EMA ? ema_weight(omd, step) : 0.f;
    float4* e4 = reinterpret_cast<float4*>(ema);
    const float sc = scale ? scale[0] : 1.f;
    const long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        gg = gg * sc + l2 * pp;
        mm = beta1 * mm + (1.f - beta1) * gg;
        vv = beta2 * vv + (1.f - beta2) * gg * gg;
        pp -= lr * mm / (sqrtf(vv) + eps);
        if (SUMSQ) s2 += pp * pp;
    };
    // two independent 16-byte groups per thread and iteration: eight loads in flight before the first use (HBM-bound: 28 B / parameter)
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {
        const long j = i + stride;
        float4 pa = p4[i], ma = m4[i], va = v4[i];
        const float4 ga = g4[i];
        float4 pb = p4[j], mb = m4[j], vb = v4[j];
        const float4 gb = g4[j];
        float4 ea, eb;
        if (EMA) { ea = e4[i]; eb = e4[j]; }
        upd(pa.x, ga.x, ma.x, va.x); upd(pa.y, ga.y, ma.y, va.y);
        upd(pa.z, ga.z, ma.z, va.z); upd(pa.w, ga.w, ma.w, va.w);
        upd(pb.x, gb.x, mb.x, vb.x); upd(pb.y, gb.y, mb.y, vb.y);
        upd(pb.z, gb.z, mb.z, vb.z); upd(pb.w, gb.w, mb.w, vb.w);
        p4[i] = pa; m4[i] = ma; v4[i] = va;
        p4[j] = pb; m4[j] = mb; v4[j] = vb;
        if (EMA) {
            ema_apply4(w, pa, ea); ema_apply4(w, pb, eb);
            e4[i] = ea; e4[j] = eb;
        }
    }
    if (i < n4) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        float4 ee;
        if (EMA) ee = e4[i];
        upd(pp.x, gg.x, mm.x, vv.x); upd(pp.y, gg.y, mm.y, vv.y);
        upd(pp.z, gg.z, mm.z, vv.z); upd(pp.w, gg.w, mm.w, vv.w);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (EMA) {
            ema_apply4(w, pp, ee);
            e4[i] = ee;
        }
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        upd(p[i], g[i], m[i], v[i]);
        if (EMA) ema[i] = ema_apply(w, p[i], ema[i]);
    }
    if (SUMSQ) {
        s2 = block_sum<256>(s2, sh);
        if (threadIdx.x == 0) sumsq_partial[blockIdx.x] = s2;
    }
}

// The average as a pass of its own (SGD / Momentum, whose update kernels are not fused with it; the A/B partner of adam_kernel<., true>):
// 2 reads + 1 write x 4 B = 12 B per parameter.
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float omd,
                                                  const int32_t* __restrict__ step) {
    const float w = ema_weight(omd, step);
    const long n4 = n >> 2;
    float4* e4 = reinterpret_cast<float4*>(ema);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 pp = p4[i];
        float4 ee = e4[i];
        ema_apply4(w, pp, ee);
        e4[i] = ee;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) ema[i] = ema_apply(w, p[i], ema[i]);
}

// GradientDescentOptimizer: p -= lr * (g*scale + l2*p)
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, long n,
                                                  const float* __restrict__ lr, const float* __restrict__ scale, float l2) {
    const float a = lr[0], sc = scale ? scale[0] : 1.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] -= a * (g[i] * sc + l2 * p[i]);
}

// MomentumOptimizer (TF-sem.): a = mom*a + g'; p -= lr*a.  row_mask (per row of width E):
// the sparse variant only touches rows present in the batch's indices.
__global__ __launch_bounds__(256) void momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ a,
                                                       long n, const float* __restrict__ lr, const float* __restrict__ scale,
                                                       float mom, float l2, const float* __restrict__ row_mask, int E) {
    const float al = lr[0], sc = scale ? scale[0] : 1.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        if (row_mask && row_mask[i / E] == 0.f) continue;
        const float gg = g[i] * sc + l2 * p[i];
        const float aa = mom * a[i] + gg;
        a[i] = aa;
        p[i] -= al * aa;
    }
}

// mode 0: raw uint32; 1: N(0,1) via Box-Muller; 2: Bernoulli(keep) as 0/1 floats; 3: uniform [0,1)
// `step` (nullable, device): added to the high KEY word so that a captured graph draws a fresh
// stream every replay without any host-side argument change.  (Counter words stay (element quad,
// offset): callers put a stream id into offset >> 32, so step must not share a word with it --
// stream k at step s+1 would repeat stream k+1 at step s.)
__global__ __launch_bounds__(256) void philox_kernel(void* __restrict__ out, long n, uint64_t seed, uint64_t offset, int mode,
                                                     float keep, const int32_t* __restrict__ step) {
    const long nq = (n + 3) >> 2;
    const uint32_t k1 = (uint32_t)(seed >> 32) + (step ? (uint32_t)step[0] : 0u);
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        uint32_t r[4];
        philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, k1, r);
        float f[4];
        if (mode == 1) {
            box_muller4(r, f);
        } else if (mode == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = ((float)r[j] * 2.3283064365386963e-10f < keep) ? 1.f : 0.f;
        } else if (mode == 3) {
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = (float)(r[j] >> 8) * 5.9604644775390625e-08f;  // 24 bits -> [0, 1)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = q * 4 + j;
            if (i < n) {
                if (mode == 0) reinterpret_cast<uint32_t*>(out)[i] = r[j];
                else reinterpret_cast<float*>(out)[i] = f[j];
            }
        }
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_sumsq_blocks(void) { return SUMSQ_BLOCKS; }

extern "C" int vc_sumsq_partial_f32(void* stream, const float* x, long n, float* partial) {
    VC_CHECK_ARG(x && partial && n >= 0 && (((uintptr_t)x & 15) == 0), "bad argument (x must be 16-byte aligned)");
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, x, n, partial);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_clip_finalize_f32(void* stream, const float* partial, int n_partial, float clip, float* out_norm_scale) {
    VC_CHECK_ARG(partial && out_norm_scale && n_partial > 0 && clip > 0.f, "bad argument");
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n_partial, clip, out_norm_scale);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_step_update(void* stream, int32_t* step, float* scalars, float lr, float cnn_lr, float beta1, float beta2,
                              float ann_param, int ann_on, int decay_steps) {
    VC_CHECK_ARG(step && scalars, "null pointer");
    hipLaunchKernelGGL(step_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, scalars, lr, cnn_lr, beta1, beta2, ann_param, ann_on, decay_steps);
    VC_LAUNCH_CHECK();
    return 0;
}

// vc_step_update with the cyclical KL schedule in scalars[1]: step_update_kernel itself (tanh schedule off) writes every other scalar
// and increments the counter, then cyclical_ann_kernel overwrites scalars[1] -- s[0], s[2..4] are vc_step_update's to the bit.
extern "C" int vc_step_update_cyclical(void* stream, int32_t* step, float* scalars, float lr, float cnn_lr, float beta1, float beta2,
                                       int decay_steps, int cycle_steps, float cycle_ramp, int cycles) {
    VC_CHECK_ARG(step && scalars, "null pointer");
    VC_CHECK_ARG(cycle_steps > 0 && cycle_ramp > 0.f && cycle_ramp <= 1.f && cycles >= 0, "cycle_steps > 0, cycle_ramp in (0, 1], cycles >= 0");
    hipLaunchKernelGGL(step_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, scalars, lr, cnn_lr, beta1, beta2, 0.f, 0, decay_steps);
    hipLaunchKernelGGL(cyclical_ann_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, scalars, cycle_steps, cycle_ramp, cycles);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_adam_f32(void* stream, float* p, const float* g, float* m, float* v, long n, const float* lr_t,
                           const float* scale, float beta1, float beta2, float eps, float l2) {
    VC_CHECK_ARG(p && g && m && v && lr_t && n >= 0, "bad argument");
    VC_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "buffers must be 16-byte aligned");
    if (n == 0) return 0;
    hipLaunchKernelGGL((adam_kernel<false, false>), dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr_t, scale, beta1, beta2, eps, l2, nullptr, nullptr, 0.f, nullptr);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_adam_blocks(long n) { return adam_grid(n); }

extern "C" int vc_adam_sumsq_f32(void* stream, float* p, const float* g, float* m, float* v, long n, const float* lr_t,
                                 const float* scale, float beta1, float beta2, float eps, float l2, float* sumsq_partial) {
    VC_CHECK_ARG(p && g && m && v && lr_t && sumsq_partial && n > 0, "bad argument");
    VC_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "buffers must be 16-byte aligned");
    hipLaunchKernelGGL((adam_kernel<true, false>), dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr_t, scale, beta1, beta2, eps, l2, sumsq_partial, nullptr, 0.f, nullptr);
    VC_LAUNCH_CHECK();
    return 0;
}

// [a, a + n) and [b, b + n) share an element
static inline bool ranges_overlap(const float* a, const float* b, long n) {
    return (uintptr_t)a < (uintptr_t)(b + n) && (uintptr_t)b < (uintptr_t)(a + n);
}

extern "C" int vc_adam_ema_f32(void* stream, float* p, const float* g, float* m, float* v, float* ema, long n, const float* lr_t,
                               const float* scale, float beta1, float beta2, float eps, float l2, float omd, const int32_t* step) {
    VC_CHECK_ARG(p && g && m && v && ema && lr_t && n >= 0, "bad argument (null pointer or n < 0)");
    VC_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0, "buffers must be 16-byte aligned");
    VC_CHECK_ARG(omd > 0.f && omd <= 1.f, "omd = 1 - decay must be in (0, 1]");
    VC_CHECK_ARG(!ranges_overlap(ema, p, n) && !ranges_overlap(ema, m, n) && !ranges_overlap(ema, v, n), "ema must not alias p, m or v");
    if (n == 0) return 0;
    hipLaunchKernelGGL((adam_kernel<false, true>), dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr_t, scale, beta1, beta2, eps, l2, nullptr, ema, omd, step);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_adam_sumsq_ema_f32(void* stream, float* p, const float* g, float* m, float* v, float* ema, long n, const float* lr_t,
                                     const float* scale, float beta1, float beta2, float eps, float l2, float omd, const int32_t* step,
                                     float* sumsq_partial) {
    VC_CHECK_ARG(p && g && m && v && ema && lr_t && sumsq_partial && n > 0, "bad argument (null pointer or n <= 0)");
    VC_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0, "buffers must be 16-byte aligned");
    VC_CHECK_ARG(omd > 0.f && omd <= 1.f, "omd = 1 - decay must be in (0, 1]");
    VC_CHECK_ARG(!ranges_overlap(ema, p, n) && !ranges_overlap(ema, m, n) && !ranges_overlap(ema, v, n), "ema must not alias p, m or v");
    hipLaunchKernelGGL((adam_kernel<true, true>), dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr_t, scale, beta1, beta2, eps, l2, sumsq_partial, ema, omd, step);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_ema_update_f32(void* stream, float* ema, const float* p, long n, float omd, const int32_t* step) {
    VC_CHECK_ARG(ema && p && n >= 0, "bad argument (null pointer or n < 0)");
    VC_CHECK_ARG((((uintptr_t)ema | (uintptr_t)p) & 15) == 0, "buffers must be 16-byte aligned");
    VC_CHECK_ARG(omd > 0.f && omd <= 1.f, "omd = 1 - decay must be in (0, 1]");
    VC_CHECK_ARG(!ranges_overlap(ema, p, n), "ema must not alias p");
    if (n == 0) return 0;
    hipLaunchKernelGGL(ema_kernel, dim3(adam_grid(n)), dim3(256), 0, (hipStream_t)stream, ema, p, n, omd, step);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_sgd_f32(void* stream, float* p, const float* g, long n, const float* lr, const float* scale, float l2) {
    VC_CHECK_ARG(p && g && lr && n >= 0, "bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, n, lr, scale, l2);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_momentum_f32(void* stream, float* p, const float* g, float* accum, long n, const float* lr,
                               const float* scale, float momentum, float l2, const float* row_mask, int E) {
    VC_CHECK_ARG(p && g && accum && lr && n >= 0 && (!row_mask || E > 0), "bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(momentum_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, accum, n, lr, scale, momentum, l2, row_mask, E > 0 ? E : 1);
    VC_LAUNCH_CHECK();
    return 0;
}

static int philox_launch(void* stream, void* out, long n, uint64_t seed, uint64_t offset, int mode, float keep,
                         const int32_t* step) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(philox_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, seed, offset, mode, keep, step);
    return launch_status("vc_philox");
}

extern "C" int vc_philox_u32(void* stream, uint32_t* out, long n, uint64_t seed, uint64_t offset, const int32_t* step) {
    VC_CHECK_ARG(out && n >= 0, "bad argument");
    return philox_launch(stream, out, n, seed, offset, 0, 0.f, step);
}
extern "C" int vc_philox_normal_f32(void* stream, float* out, long n, uint64_t seed, uint64_t offset, const int32_t* step) {
    VC_CHECK_ARG(out && n >= 0, "bad argument");
    return philox_launch(stream, out, n, seed, offset, 1, 0.f, step);
}
extern "C" int vc_philox_uniform_f32(void* stream, float* out, long n, uint64_t seed, uint64_t offset, const int32_t* step) {
    VC_CHECK_ARG(out && n >= 0, "bad argument");
    return philox_launch(stream, out, n, seed, offset, 3, 0.f, step);
}
extern "C" int vc_philox_bernoulli_f32(void* stream, float* out, long n, float keep, uint64_t seed, uint64_t offset,
                                       const int32_t* step) {
    VC_CHECK_ARG(out && n >= 0 && keep > 0.f && keep <= 1.f, "bad argument");
    return philox_launch(stream, out, n, seed, offset, 2, keep, step);
}
