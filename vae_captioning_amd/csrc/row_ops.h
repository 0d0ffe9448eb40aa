// Device pieces shared by the kernels that run one workgroup of 256 threads per row of logits.  Every function here is the ONE
// definition of something several entries must compute bit for bit alike; a kernel that needs the piece calls it, none keeps a copy.
//
// The contract (tests/test_gpu_row_contract.py asserts it across entries):
//   * temperature-1 log-softmax of a word, lsm_term(x, M, log S) with (M, S) from row_max_sum over row_chunk's partition: the same
//     float32 bits in vc_decode_pick_f32 / vc_decode_pick_trunc_f32 (the logprob increment), vc_sbs_expand_f32 (cand_lsm and the term
//     inside cand_key), vc_mixture_topk_f32 (stat = (M, log S)) and vc_mixture_advance_f32 (the logw increment);
//   * first maximum, block_first_max over per-thread (value, first index) pairs: the same token from vc_argmax_rows_f32,
//     vc_topk_rows_f32 (every pass), vc_decode_pick_f32 (u = NULL) and vc_sched_mix_f32 (u = NULL);
//   * inverse-CDF draw, row_cdf_part + row_cdf_pick on the scaled row: the same token from vc_multinomial_rows_f32,
//     vc_decode_pick_f32 and vc_sched_mix_f32 for the same uniform;
//   * pair order, better / wave_best: (value descending, index ascending), a strict total order over pairs with distinct indices, for
//     every "best k of a row" selection (top-k, stochastic beam search, marginal decoding, the ranking of diverse captions).
// Summation and reduction ORDERS are part of this interface, not an implementation detail: the partition into 256 contiguous chunks,
// a thread's ascending walk over its chunk, block_max / block_sum's wave butterfly followed by the waves in wave order, thread 0's
// ascending walk over the 256 chunk sums.  A maximum does not depend on the order it is taken in, so a kernel may take the row's
// maximum in another pass of its own (decode_pick_trunc_kernel, multinomial_rows_kernel and sched_mix_kernel do); a sum does.
#pragma once
#include "common.h"

namespace vc {

constexpr int ROW_LDS_MAX = 12288;   // logits rows up to this width are staged in LDS (48 KiB): the row is read from memory once

// ---- staged row: the row is copied to LDS with coalesced loads and every later pass reads it there (STAGE), or is read in place
template <bool STAGE>
__device__ __forceinline__ const float* stage_row(const float* p, int V, float* srow) {
    if (STAGE) {
        for (int c = threadIdx.x; c < V; c += 256) srow[c] = p[c];
        __syncthreads();
        p = srow;
    }
    return p;
}

// ---- row stats.  Contiguous chunk [c0, c1) per thread: the scan order is the index order.  Returns the chunk width.
__device__ __forceinline__ int row_chunk(int V, int& c0, int& c1) {
    const int per = (V + 255) / 256;
    c0 = threadIdx.x * per;
    c1 = min(V, c0 + per);
    return per;
}

// S = sum over the row of exp(x - mx1): chunk sums in index order, then block_sum
__device__ __forceinline__ float row_exp_sum(const float* p, int c0, int c1, float mx1, float* sh /* 4 */) {
    float s1 = 0.f;
    for (int c = c0; c < c1; ++c) s1 += __expf(p[c] - mx1);
    return block_sum<256>(s1, sh);
}

// (M, S) of the temperature-1 log-softmax, and the thread's first maximum (bv, bi) of its chunk for block_first_max
__device__ __forceinline__ void row_max_sum(const float* p, int c0, int c1, float* sh /* 4 */, float& mx1, float& s1, float& bv, int& bi) {
    float v1 = -INFINITY;
    int i1 = 0x7fffffff;
    for (int c = c0; c < c1; ++c) {
        const float v = p[c];
        if (v > v1) { v1 = v; i1 = c; }
    }
    mx1 = block_max<256>(v1, sh);
    s1 = row_exp_sum(p, c0, c1, mx1, sh);
    bv = v1;
    bi = i1;
}
__device__ __forceinline__ void row_max_sum(const float* p, int c0, int c1, float* sh /* 4 */, float& mx1, float& s1) {
    float bv;
    int bi;
    row_max_sum(p, c0, c1, sh, mx1, s1, bv, bi);
}

// log softmax at temperature 1 of a word with logit x: ls = logf(S)
__device__ __forceinline__ float lsm_term(float x, float mx1, float ls) { return (x - mx1) - ls; }

// ---- first maximum: 256-wide LDS tree on (value descending, index ascending); the winner is in sv[0], si[0] for every thread.
// A thread that met its columns in ascending order and kept the first of its maxima (`>`) hands in (bv, bi): np.argmax's tie rule.
__device__ __forceinline__ void block_first_max(float bv, int bi, float* sv /* 256 */, int* si /* 256 */) {
    const int t = threadIdx.x;
    sv[t] = bv;
    si[t] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const float v2 = sv[t + o];
            const int i2 = si[t + o];
            if (v2 > sv[t] || (v2 == sv[t] && i2 < si[t])) {
                sv[t] = v2;
                si[t] = i2;
            }
        }
        __syncthreads();
    }
}

// ---- inverse-CDF draw on the row scaled by inv_temp, mx = its maximum: index = first i with cumsum(exp(x * inv_temp - mx))[i] > u * total.
// row_cdf_part: the thread's chunk sum into part[]; row_cdf_pick: thread 0's walk over the chunks, then inside the chosen one.
// u points at the row's uniform and is read behind the sum of the chunk sums: handed in as a value, its load stands in front of that
// loop and every wait on the loop's LDS reads then waits for all of them (measured: vc_sched_mix_f32's draw 3 % slower).
__device__ __forceinline__ void row_cdf_part(const float* p, int c0, int c1, float inv_temp, float mx, float* part /* 256 */) {
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += __expf(p[c] * inv_temp - mx);
    part[threadIdx.x] = s;
    __syncthreads();
}
__device__ __forceinline__ int row_cdf_pick(const float* p, int V, int per, float inv_temp, float mx, const float* part, const float* u) {
    float tot = 0.f;
    for (int i = 0; i < 256; ++i) tot += part[i];
    const float target = u[0] * tot;
    float run = 0.f;
    int k = 0;
    for (; k < 255; ++k) {
        if (run + part[k] > target) break;
        run += part[k];
    }
    int idx = min(V - 1, k * per);
    for (int c = k * per; c < min(V, (k + 1) * per); ++c) {
        run += __expf(p[c] * inv_temp - mx);
        idx = c;
        if (run > target) break;
    }
    return idx;
}

// ---- pair order.  (value descending, index ascending): a strict total order over pairs with distinct indices
template <typename T>
__device__ __forceinline__ bool better(T va, int ia, T vb, int ib) { return va > vb || (va == vb && ia < ib); }

// the best pair of the wave, in every lane
template <typename T>
__device__ __forceinline__ void wave_best(T& bv, int& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}

}  // namespace vc
