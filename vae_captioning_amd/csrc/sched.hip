// Scheduled sampling, parallel (two-pass) form: the mix between the two decoder passes of a training step (DESIGN.md "Scheduled
// sampling").  Pass 1 -- the teacher-forced forward -- has left logits for every position; each decoder input word behind <BOS>
// is replaced, with probability `rate`, by a word drawn from the model's own prediction for that position.
//
//   vc_sched_mix_f32   one workgroup per position (t, n) of the time-major [T, N] token array.  The eligibility (1 <= t < lens[n]) and
//                      coin (coin[t, n] < rate) tests come first: a position that fails one copies its gold token and touches no logits
//                      memory.  A selected position reads logits row (t-1) * N + n ONCE from memory (16-byte loads when the row's
//                      address allows them) into LDS and draws the word there: the inverse-CDF draw, or the first maximum when u is
//                      NULL, both row_ops.h's (the tokens of vc_multinomial_rows_f32 / vc_decode_pick_f32 and of
//                      vc_argmax_rows_f32).  Rows too wide for the LDS (V > SCHED_LDS_MAX,
//                      beyond every vocabulary the engine runs the mode with) are read in place, several times.
//                      The rate comes from the device step counter (constant / linear / inverse-sigmoid schedule): a captured step
//                      needs no host value.  A one-workgroup kernel behind it counts the eligible and the replaced positions with the
//                      same tests and reports the rate (plain integer adds by one thread: no atomics).
#include "row_ops.h"
#include "vaecap.h"

namespace vc {

constexpr int SCHED_LDS_MAX = 36864;   // floats of a logits row staged in LDS: 144 KiB of the CU's 160 KiB (2 KiB are static)

// The sampling rate of this optimiser step: s = step[0] - 1 (vc_step_update has already incremented the counter).  One copy of the code
// for both kernels (noinline): the counting kernel compares every coin with the very float the mixing kernel compared it with.
__device__ __noinline__ float sched_rate_dev(const int32_t* __restrict__ step, int schedule, float rate_max, int ramp) {
    const float s = (float)max(step[0] - 1, 0);
    const float k = (float)ramp;
    if (schedule == 1) return rate_max * fminf(1.f, s / k);
    // 1 - k / (k + exp(s / k)) == 1 / (1 + k exp(-s / k)): this form neither cancels at s = 0 nor overflows far behind the ramp
    if (schedule == 2) return rate_max / (1.f + k * expf(-s / k));
    return rate_max;
}

template <bool STAGE>
__global__ __launch_bounds__(256) void sched_mix_kernel(const float* __restrict__ logits, long ld, int V, int N,
                                                        const int32_t* __restrict__ cap, const int32_t* __restrict__ lens,
                                                        const float* __restrict__ coin, const float* __restrict__ u, float inv_temp,
                                                        const int32_t* __restrict__ step, int schedule, float rate_max, int ramp,
                                                        int32_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float srow[];
    __shared__ float sh[4];
    __shared__ float part[256];
    __shared__ int si[256];
    const long pos = blockIdx.x;   // t * N + n
    const int t = (int)(pos / N), n = (int)(pos - (long)t * N);
    const int tid = threadIdx.x;
    bool sel = false;
    if (t >= 1 && t < lens[n]) sel = coin[pos] < sched_rate_dev(step, schedule, rate_max, ramp);
    if (!sel) {   // (the whole workgroup: nothing below is reached, no logits memory is touched)
        if (tid == 0) out[pos] = cap[pos];
        return;
    }
    const float* p = logits + (pos - N) * ld;   // the prediction for input position (t, n): pass 1's output at (t - 1, n)
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const int V4 = vec ? (V >> 2) : 0;          // whole quads inside [0, V); the rest (every column of an unaligned row) by 4-byte loads
    if (u == nullptr) {
        // ---- the first maximum.  A thread meets its columns in ascending order, so `>` keeps the first of its maxima; the tree then
        // prefers the lower index among equal values (row_ops.h: block_first_max)
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int q = tid; q < V4; q += 256) {
            const float4 v = reinterpret_cast<const float4*>(p)[q];
            if (v.x > bv) { bv = v.x; bi = 4 * q; }
            if (v.y > bv) { bv = v.y; bi = 4 * q + 1; }
            if (v.z > bv) { bv = v.z; bi = 4 * q + 2; }
            if (v.w > bv) { bv = v.w; bi = 4 * q + 3; }
        }
        for (int c = 4 * V4 + tid; c < V; c += 256) {
            const float v = p[c];
            if (v > bv) { bv = v; bi = c; }
        }
        block_first_max(bv, bi, part, si);
        if (tid == 0) out[pos] = min(si[0], V - 1);   // (a row without any value above -inf: a token inside the vocabulary all the same)
        return;
    }
    // ---- the inverse-CDF draw.  The maximum of the scaled row is taken while the row is staged (a maximum does not depend on the
    // order); everything that is summed is row_ops.h's.
    float mx = -INFINITY;
    if (STAGE) {
        for (int q = tid; q < V4; q += 256) {
            const float4 v = reinterpret_cast<const float4*>(p)[q];
            reinterpret_cast<float4*>(srow)[q] = v;
            mx = fmaxf(mx, fmaxf(fmaxf(v.x * inv_temp, v.y * inv_temp), fmaxf(v.z * inv_temp, v.w * inv_temp)));
        }
        for (int c = 4 * V4 + tid; c < V; c += 256) {
            const float v = p[c];
            srow[c] = v;
            mx = fmaxf(mx, v * inv_temp);
        }
        __syncthreads();
        p = srow;
    } else {
        for (int c = tid; c < V; c += 256) mx = fmaxf(mx, p[c] * inv_temp);
    }
    mx = block_max<256>(mx, sh);
    int c0, c1;
    const int per = row_chunk(V, c0, c1);
    row_cdf_part(p, c0, c1, inv_temp, mx, part);
    if (tid == 0) out[pos] = row_cdf_pick(p, V, per, inv_temp, mx, part, u + pos);   // (STAGE: the walk inside the chosen chunk reads LDS)
}

// stats[0] += eligible positions, stats[1] += replaced positions, rate_out[0] = the rate: one workgroup, the mixing kernel's tests
__global__ __launch_bounds__(256) void sched_stats_kernel(const int32_t* __restrict__ lens, const float* __restrict__ coin,
                                                          const int32_t* __restrict__ step, int schedule, float rate_max, int ramp,
                                                          int N, long TN, int32_t* __restrict__ stats, float* __restrict__ rate_out) {
    __shared__ int se[4], sr[4];
    const float rate = sched_rate_dev(step, schedule, rate_max, ramp);
    int e = 0, r = 0;
    for (long i = N + threadIdx.x; i < TN; i += 256) {   // (t >= 1)
        const int t = (int)(i / N), n = (int)(i - (long)t * N);
        if (t < lens[n]) {
            ++e;
            if (coin[i] < rate) ++r;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        e += __shfl_xor(e, o, 64);
        r += __shfl_xor(r, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        se[threadIdx.x >> 6] = e;
        sr[threadIdx.x >> 6] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (stats) {
            stats[0] += (se[0] + se[1]) + (se[2] + se[3]);
            stats[1] += (sr[0] + sr[1]) + (sr[2] + sr[3]);
        }
        if (rate_out) rate_out[0] = rate;
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_sched_mix_f32(void* stream, const float* logits, long ld, int V, int T, int N, const int32_t* cap_dec_t,
                                const int32_t* lens, const float* coin, const float* u, float temperature, const int32_t* step,
                                int schedule, float rate_max, int ramp_steps, int32_t* dec_mix_t, int32_t* stats, float* rate_out) {
    VC_CHECK_ARG(logits && cap_dec_t && lens && coin && step && dec_mix_t, "null pointer");
    VC_CHECK_ARG(V >= 1 && ld >= V && T >= 1 && N >= 1 && (long)T * N < (1L << 31), "V >= 1, ld >= V, T >= 1, N >= 1 and T * N < 2^31 required");
    VC_CHECK_ARG(u == nullptr || temperature > 0.f, "temperature must be > 0 for the sampled pick");
    VC_CHECK_ARG(rate_max >= 0.f && rate_max <= 1.f, "rate_max must be in [0, 1]");
    VC_CHECK_ARG(schedule >= 0 && schedule <= 2, "unknown schedule (0 constant, 1 linear, 2 inverse sigmoid)");
    VC_CHECK_ARG(schedule == 0 || ramp_steps > 0, "ramp_steps must be > 0 for the linear and the inverse-sigmoid schedule");
    hipStream_t st = (hipStream_t)stream;
    const long TN = (long)T * N;
    const float inv_temp = u ? 1.0f / temperature : 1.0f;
    const bool stage = u != nullptr && V <= SCHED_LDS_MAX;
    if (stage) {
        const size_t lds = (size_t)V * sizeof(float);
        if (lds > 48 * 1024) {   // beyond the default dynamic LDS of a launch: raise the kernel's limit to the largest row it stages, once
            static bool raised = false;
            if (!raised) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sched_mix_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                         (int)(SCHED_LDS_MAX * sizeof(float)));
                if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute (%ld bytes of dynamic LDS) failed", __func__, (long)(SCHED_LDS_MAX * sizeof(float)));
                raised = true;
            }
        }
        hipLaunchKernelGGL(sched_mix_kernel<true>, dim3((unsigned)TN), dim3(256), lds, st, logits, ld, V, N, cap_dec_t, lens, coin, u, inv_temp, step,
                           schedule, rate_max, ramp_steps, dec_mix_t);
    } else {
        hipLaunchKernelGGL(sched_mix_kernel<false>, dim3((unsigned)TN), dim3(256), 0, st, logits, ld, V, N, cap_dec_t, lens, coin, u, inv_temp, step,
                           schedule, rate_max, ramp_steps, dec_mix_t);
    }
    VC_LAUNCH_CHECK();
    if (stats || rate_out) {
        hipLaunchKernelGGL(sched_stats_kernel, dim3(1), dim3(256), 0, st, lens, coin, step, schedule, rate_max, ramp_steps, N, TN, stats, rate_out);
        VC_LAUNCH_CHECK();
    }
    return 0;
}
