// One row of logits as the in-place softmax cross-entropy kernels of loss.hip walk it: one workgroup of 256 threads per row, the
// gradient written over the logits.  XentRow<true> holds the row in registers and reads the logits ONCE (V <= XENT_MAXQ * 1024, a
// 16-byte aligned row whose pitch covers whole float4 quads: xent_row_in_registers); XentRow<false> serves any V, pitch or alignment
// with three passes over the row (passes 2 and 3 hit L2).  Both offer the same steps, in the order a kernel takes them:
//   thread_max   per-thread maximum over the V real columns, with the per-thread sum x beside it if asked for
//   exp_sum      per-thread sum exp(x - mx); the row is from then on held as e = exp(x - mx), or as d = x - mx with KEEP_D
//   store        the gradient f(held value) of every real column, minus `sub` at the label's column
//   zero_pitch   the columns of the row pitch past V
// Summation orders are part of the interface (the kernels' results are pinned bit for bit): the register form adds a quad as
// (x + y) + (z + w) and a thread's quads in ascending order, the memory form adds a thread's columns in ascending order.  The block
// reductions between the steps are the kernel's (common.h).
// What a kernel reads of the row on the side (x[label], a candidate's logit) it reads in front of its first block reduction, whose
// barriers every thread passes before the first store: no such read can see a gradient.
#pragma once
#include "common.h"

namespace vc {

constexpr int XENT_MAXQ = 12;  // float4 per thread

// rows of whole float4 quads -- V % 4 == 0, or a row pitch padded to a multiple of 4 (ld >= roundup(V, 4)) -- that fit the registers
static inline bool xent_row_in_registers(const float* logits, int V, long ld) {
    return (ld % 4 == 0) && (ld >= (long)((V + 3) / 4) * 4) && (V <= XENT_MAXQ * 256 * 4) && (((uintptr_t)logits & 15) == 0);
}

template <bool REG, bool KEEP_D = false>
struct XentRow;

template <bool KEEP_D>
struct XentRow<true, KEEP_D> {
    float* r;
    float4* p;
    int V, V4;   // V % 4 != 0 (the reference's observed 11313): the row's last quad reaches into the ld padding
    float4 x[XENT_MAXQ];

    // Straight-line loads: a thread past the row's last quad re-reads that quad (a valid address; its lanes are masked in thread_max),
    // so all twelve 16-byte loads are in flight at once -- with the load inside `if (i < V4)` and the padding handled by branches each
    // load waited for the one before it and was split into a 12-byte and a 4-byte one (24 serialised round trips per thread).
    __device__ __forceinline__ XentRow(float* row, int V_) : r(row), p(reinterpret_cast<float4*>(row)), V(V_), V4((V_ + 3) >> 2) {
#pragma unroll
        for (int q = 0; q < XENT_MAXQ; ++q) x[q] = p[min((int)threadIdx.x + q * 256, V4 - 1)];
    }

    // columns >= V (the pitch padding, and every lane of a thread past the row) do not exist: 0 in sum x, -inf for max and exp
    __device__ __forceinline__ float thread_max(float* sx = nullptr) {
        float mx = -INFINITY, t = 0.f;
#pragma unroll
        for (int q = 0; q < XENT_MAXQ; ++q) {
            const int c = ((int)threadIdx.x + q * 256) * 4;
            const bool v0 = c < V, v1 = c + 1 < V, v2 = c + 2 < V, v3 = c + 3 < V;
            if (sx) t += ((v0 ? x[q].x : 0.f) + (v1 ? x[q].y : 0.f)) + ((v2 ? x[q].z : 0.f) + (v3 ? x[q].w : 0.f));
            x[q].x = v0 ? x[q].x : -INFINITY; x[q].y = v1 ? x[q].y : -INFINITY;
            x[q].z = v2 ? x[q].z : -INFINITY; x[q].w = v3 ? x[q].w : -INFINITY;
            mx = fmaxf(mx, fmaxf(fmaxf(x[q].x, x[q].y), fmaxf(x[q].z, x[q].w)));
        }
        if (sx) *sx = t;
        return mx;
    }

    // (exp(-inf) = 0: the masked lanes add nothing.)  KEEP_D: *sd = sum e * d beside it; a term whose e is 0 (masked: d = -inf;
    // underflowed: d finite) is exactly 0, never 0 * -inf
    __device__ __forceinline__ float exp_sum(float mx, float* sd = nullptr) {
        float s = 0.f, t = 0.f;
#pragma unroll
        for (int q = 0; q < XENT_MAXQ; ++q) {
            const float d0 = x[q].x - mx, d1 = x[q].y - mx, d2 = x[q].z - mx, d3 = x[q].w - mx;
            const float e0 = __expf(d0), e1 = __expf(d1), e2 = __expf(d2), e3 = __expf(d3);
            s += (e0 + e1) + (e2 + e3);
            if (KEEP_D) {
                t += ((e0 > 0.f ? e0 * d0 : 0.f) + (e1 > 0.f ? e1 * d1 : 0.f)) + ((e2 > 0.f ? e2 * d2 : 0.f) + (e3 > 0.f ? e3 * d3 : 0.f));
                x[q] = make_float4(d0, d1, d2, d3);
            } else {
                x[q] = make_float4(e0, e1, e2, e3);
            }
        }
        if (KEEP_D) *sd = t;
        return s;
    }

    // A map-and-store with a branch-free patch of the label's column (label < 0: no column is patched).  lq: which of this thread's
    // quads holds the label, -1 in every other thread.
    template <class F>
    __device__ __forceinline__ void store(F f, int label, float sub) {
        const bool own = label >= 0 && (int)threadIdx.x == ((label >> 2) & 255);
        const int lq = own ? (label >> 10) : -1, lc = label & 3;
        const float a0 = lc == 0 ? sub : 0.f, a1 = lc == 1 ? sub : 0.f, a2 = lc == 2 ? sub : 0.f, a3 = lc == 3 ? sub : 0.f;
#pragma unroll
        for (int q = 0; q < XENT_MAXQ; ++q) {
            const int i = threadIdx.x + q * 256;
            if (i < V4) {
                const float m = q == lq ? 1.f : 0.f;
                p[i] = make_float4(f(x[q].x) - m * a0, f(x[q].y) - m * a1, f(x[q].z) - m * a2, f(x[q].w) - m * a3);
            }
        }
    }

    // The padding must come back as exact zeros: dense_bwd_w contracts over the padded pitch.  The last quad's padding columns hold
    // f(exp(-inf)), whatever that is: the thread that stored that quad overwrites them (last_quad = false: the caller's f maps 0 to 0).
    // Then the quads of the pitch past the last real column.
    __device__ __forceinline__ void zero_pitch(long ld, bool last_quad = true) {
        if (last_quad && (int)threadIdx.x == ((V4 - 1) & 255))
            for (int c = V; c < V4 * 4; ++c) r[c] = 0.f;
        const int L4 = (int)(ld >> 2);
        for (int i = V4 + threadIdx.x; i < L4; i += 256) p[i] = f4zero();
    }
};

template <bool KEEP_D>
struct XentRow<false, KEEP_D> {
    float* p;
    int V;
    float mx;   // the row's maximum, kept by exp_sum for store's pass

    __device__ __forceinline__ XentRow(float* row, int V_) : p(row), V(V_) {}

    __device__ __forceinline__ float thread_max(float* sx = nullptr) {
        float m = -INFINITY, t = 0.f;
        for (int c = threadIdx.x; c < V; c += 256) {
            const float v = p[c];
            m = fmaxf(m, v);
            if (sx) t += v;
        }
        if (sx) *sx = t;
        return m;
    }

    __device__ __forceinline__ float exp_sum(float mx_, float* sd = nullptr) {
        mx = mx_;
        float s = 0.f, t = 0.f;
        for (int c = threadIdx.x; c < V; c += 256) {
            const float d = p[c] - mx, e = __expf(d);
            s += e;
            if (KEEP_D) t += e > 0.f ? e * d : 0.f;
        }
        if (KEEP_D) *sd = t;
        return s;
    }

    template <class F>
    __device__ __forceinline__ void store(F f, int label, float sub) {
        for (int c = threadIdx.x; c < V; c += 256) {
            const float d = p[c] - mx;
            float g = f(KEEP_D ? d : __expf(d));
            if (c == label) g -= sub;
            p[c] = g;
        }
    }

    __device__ __forceinline__ void zero_pitch(long ld, bool = true) {
        for (long c = V + threadIdx.x; c < ld; c += 256) p[c] = 0.f;
    }
};

}  // namespace vc
