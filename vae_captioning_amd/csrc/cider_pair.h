// The ONE definition of the one-reference CIDEr-D pair score: consensus.hip (vc_consensus_score: a candidate against the pool of its
// neighbours' captions) and cider_gram.hip (vc_cider_gram: every caption of an image against every other one) call it, neither keeps
// a copy, so the two entries give the same float32 bits for the same (hypothesis, reference) pair.
//
//   CIDEr-D(c, r) = 10 exp(-(L(c) - L(r))^2 / 72) / 4 sum_n sum_g min(c_g, r_g) r_g / (|c_n| |r_n|)     (an order with a zero norm adds 0)
//
// The ORDER of the arithmetic is part of the interface: the reference's keys are walked in their sorted order, fminf(wc, wr) * wr is
// added to its order's f32 sum as it is met, the four orders are added n = 1..4, and the length penalty multiplies last.
#pragma once
#include "common.h"

namespace vc {

constexpr int CP_SLOTS = 256;   // n-gram slots of a staged hypothesis: 4 * 64 (64 + 63 + 62 + 61 used at most)

// What a thread keeps of the CPB hypotheses its workgroup has staged in LDS: sorted keys / weights at s_ck[c] / s_cw[c] [0, cn[c]),
// words cl[c], norms cnorm[c][0..3].  A missing hypothesis has cn = 0, cl = 0 and zero norms: its score is 0.
template <int CPB>
struct CiderHyps {
    int cn[CPB], cl[CPB];
    float cnorm[CPB][4];
};

// Stage hypothesis rows c0 .. c0 + nc - 1 (nc <= CPB) of an ngram_vectors table with the workgroup's 256 threads; the caller
// synchronises before the first cider_pair_scores.
template <int CPB>
__device__ __forceinline__ void cider_stage_hyps(int c0, int nc, const int32_t* __restrict__ c_off, const int32_t* __restrict__ c_nnz,
                                                 const uint64_t* __restrict__ c_keys, const float* __restrict__ c_w,
                                                 const float* __restrict__ c_norm, const int32_t* __restrict__ c_len,
                                                 uint64_t (*s_ck)[CP_SLOTS], float (*s_cw)[CP_SLOTS], CiderHyps<CPB>& h) {
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < CPB; ++c) {
        h.cn[c] = 0;
        h.cl[c] = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) h.cnorm[c][q] = 0.f;
        if (c < nc) {
            const int ci = c0 + c;
            h.cn[c] = min(c_nnz[ci], CP_SLOTS);
            h.cl[c] = c_len[ci];
#pragma unroll
            for (int q = 0; q < 4; ++q) h.cnorm[c][q] = c_norm[(long)ci * 4 + q];
            for (int i = t; i < h.cn[c]; i += 256) {
                s_ck[c][i] = c_keys[(long)c_off[ci] + i];
                s_cw[c][i] = c_w[(long)c_off[ci] + i];
            }
        }
    }
}

// One thread: reference row r of an ngram_vectors table against the CPB staged hypotheses -> sc[c] = CIDEr-D(hypothesis c, reference r).
template <int CPB>
__device__ __forceinline__ void cider_pair_scores(int r, const int32_t* __restrict__ r_off, const int32_t* __restrict__ r_nnz,
                                                  const uint64_t* __restrict__ r_keys, const float* __restrict__ r_w,
                                                  const float* __restrict__ r_norm, const int32_t* __restrict__ r_len,
                                                  const uint64_t (*s_ck)[CP_SLOTS], const float (*s_cw)[CP_SLOTS], const CiderHyps<CPB>& h,
                                                  float (&sc)[CPB]) {
    const long ro = r_off[r];
    const int rn = r_nnz[r];
    float sim[CPB][4];
#pragma unroll
    for (int c = 0; c < CPB; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) sim[c][q] = 0.f;
    for (int e0 = 0; e0 < rn; e0 += 8) {   // eight keys in flight per load round (the loop is latency-bound otherwise)
        uint64_t kk[8];
        float ww[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool ok = e0 + u < rn;
            kk[u] = ok ? r_keys[ro + e0 + u] : 0ull;
            ww[u] = ok ? r_w[ro + e0 + u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (e0 + u >= rn) break;
            const uint64_t key = kk[u];
            const float wr = ww[u];
            const int n = key_order(key) - 1;
            int pos[CPB];   // per hypothesis the last slot with a key < key: fixed 8 steps, the CPB searches interleave
#pragma unroll
            for (int c = 0; c < CPB; ++c) pos[c] = -1;
#pragma unroll
            for (int st = CP_SLOTS / 2; st > 0; st >>= 1)
#pragma unroll
                for (int c = 0; c < CPB; ++c)
                    if (pos[c] + st < h.cn[c] && s_ck[c][pos[c] + st] < key) pos[c] += st;
#pragma unroll
            for (int c = 0; c < CPB; ++c) {
                const int lo = pos[c] + 1;
                if (lo < h.cn[c] && s_ck[c][lo] == key) {
                    const float v = fminf(s_cw[c][lo], wr) * wr;
#pragma unroll
                    for (int q = 0; q < 4; ++q) sim[c][q] += q == n ? v : 0.f;
                }
            }
        }
    }
    const int rl = r_len[r];
    float rnorm[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rnorm[q] = r_norm[(long)r * 4 + q];
#pragma unroll
    for (int c = 0; c < CPB; ++c) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) s += (h.cnorm[c][q] > 0.f && rnorm[q] > 0.f) ? sim[c][q] / (h.cnorm[c][q] * rnorm[q]) : 0.f;
        const float d = (float)(h.cl[c] - rl);
        sc[c] = 10.0f * expf(-(d * d) / 72.0f) * (0.25f * s);
    }
}

}  // namespace vc
