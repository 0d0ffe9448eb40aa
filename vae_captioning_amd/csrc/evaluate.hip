// Caption-set evaluation (evaluate.py: CaptionEvaluator): BLEU-style clipped n-gram counts of hypothesis captions against a contiguous
// range of reference rows, on the n-gram vectors vc_ngram_vectors writes (consensus.hip) with an EMPTY df table, so that every weight
// is the n-gram's count as an exact float.
//
//   vc_ngram_overlap   per hypothesis row (one wave): its sorted distinct keys and counts staged in LDS with a running maximum per key;
//                      the lanes stride over the keys of reference rows [lo, hi) \ {skip}, look each up by a fixed-step binary search
//                      and raise the maximum with an integer atomicMax in LDS; then total / clipped match / distinct / unseen per
//                      order and the closest reference length.  Integer sums and maxima only: the result of a row depends on nothing
//                      but the row and its range.
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int OV_SLOTS = 256;   // key slots of a caption (consensus.hip: NG_SLOTS; 64 + 63 + 62 + 61 used at most)
constexpr int OV_WAVES = 4;     // hypotheses per workgroup, one wave each

// Wave w of workgroup g owns hypothesis row g * OV_WAVES + w.  The waves share nothing but the two barriers (which stand outside every
// loop whose trip count differs between waves).  LDS: 4 * 256 * (8 + 4 + 4) = 16 KiB.
__global__ __launch_bounds__(64 * OV_WAVES) void ngram_overlap_kernel(long C, const int32_t* __restrict__ c_off, const int32_t* __restrict__ c_nnz,
                                                                      const uint64_t* __restrict__ c_keys, const float* __restrict__ c_w,
                                                                      const int32_t* __restrict__ c_len, int n_ref,
                                                                      const int32_t* __restrict__ r_off, const int32_t* __restrict__ r_nnz,
                                                                      const uint64_t* __restrict__ r_keys, const float* __restrict__ r_w,
                                                                      const int32_t* __restrict__ r_len, const int32_t* __restrict__ lo,
                                                                      const int32_t* __restrict__ hi, const int32_t* __restrict__ skip,
                                                                      int32_t* __restrict__ total, int32_t* __restrict__ match,
                                                                      int32_t* __restrict__ distinct, int32_t* __restrict__ unseen,
                                                                      int32_t* __restrict__ ref_len) {
    __shared__ uint64_t s_key[OV_WAVES][OV_SLOTS];
    __shared__ int s_cnt[OV_WAVES][OV_SLOTS];
    __shared__ int s_max[OV_WAVES][OV_SLOTS];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * OV_WAVES + wv;
    const bool live = c < C;
    int cn = 0, r0 = 0, r1 = 0, sk = -1, lc = 0;
    if (live) {
        cn = min(max(c_nnz[c], 0), OV_SLOTS);
        lc = c_len[c];
        r0 = min(max(lo[c], 0), n_ref);             // the range clamped into [0, n_ref]; lo > hi: empty
        r1 = min(max(hi[c], r0), n_ref);
        sk = skip[c];
        const long base = c_off[c];
        for (int i = lane; i < cn; i += 64) {
            s_key[wv][i] = c_keys[base + i];
            s_cnt[wv][i] = (int)(c_w[base + i] + 0.5f);
            s_max[wv][i] = 0;
        }
    }
    __syncthreads();
    // closest reference length: the minimum of (|L_r - L_c|, L_r) packed into one int (L <= 64)
    int best = 0x7fffffff;
    for (int r = r0 + lane; r < r1; r += 64) {
        if (r == sk) continue;
        const int lr = r_len[r];
        best = min(best, (abs(lr - lc) << 8) | (lr & 0xff));
    }
    for (int r = r0; r < r1; ++r) {
        if (r == sk) continue;
        const long ro = r_off[r];
        const int rn = min(max(r_nnz[r], 0), OV_SLOTS);
        for (int e0 = 0; e0 < rn; e0 += 128) {   // two keys in flight per lane
            uint64_t kk[2];
            float ww[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = e0 + u * 64 + lane;
                kk[u] = e < rn ? r_keys[ro + e] : 0ull;
                ww[u] = e < rn ? r_w[ro + e] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (e0 + u * 64 + lane >= rn) continue;
                const uint64_t key = kk[u];
                int pos = -1;   // the last slot with a key < key: fixed 8 steps
#pragma unroll
                for (int st = OV_SLOTS / 2; st > 0; st >>= 1)
                    if (pos + st < cn && s_key[wv][pos + st] < key) pos += st;
                const int p = pos + 1;
                if (p < cn && s_key[wv][p] == key) atomicMax(&s_max[wv][p], (int)(ww[u] + 0.5f));
            }
        }
    }
    __syncthreads();
    int acc[16];   // total, match, distinct, unseen of the four orders
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0;
    for (int i = lane; i < cn; i += 64) {
        const int n = key_order(s_key[wv][i]) - 1;
        const int cg = s_cnt[wv][i], mg = s_max[wv][i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool on = q == n;
            acc[q] += on ? cg : 0;
            acc[4 + q] += on ? min(cg, mg) : 0;
            acc[8 + q] += on ? 1 : 0;
            acc[12 + q] += on && mg == 0 ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] += __shfl_xor(acc[q], o, 64);
        best = min(best, __shfl_xor(best, o, 64));
    }
    if (live && lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            total[c * 4 + q] = acc[q];
            match[c * 4 + q] = acc[4 + q];
            distinct[c * 4 + q] = acc[8 + q];
            unseen[c * 4 + q] = acc[12 + q];
        }
        ref_len[c] = best == 0x7fffffff ? 0 : (best & 0xff);
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_ngram_overlap(void* stream, long C, const int32_t* c_off, const int32_t* c_nnz, const uint64_t* c_keys, const float* c_w,
                                const int32_t* c_len, long n_ref, const int32_t* r_off, const int32_t* r_nnz, const uint64_t* r_keys,
                                const float* r_w, const int32_t* r_len, const int32_t* lo, const int32_t* hi, const int32_t* skip,
                                int32_t* total, int32_t* match, int32_t* distinct, int32_t* unseen, int32_t* ref_len) {
    VC_CHECK_ARG(c_off && c_nnz && c_keys && c_w && c_len && r_off && r_nnz && r_keys && r_w && r_len && lo && hi && skip && total &&
                 match && distinct && unseen && ref_len, "null pointer");
    VC_CHECK_ARG(C >= 0 && n_ref >= 0 && n_ref < (1L << 31), "C >= 0 and 0 <= n_ref < 2^31");
    VC_CHECK_ARG((C + OV_WAVES - 1) / OV_WAVES < (1L << 31), "too many hypothesis rows for one launch");
    if (C == 0) return 0;
    hipLaunchKernelGGL(ngram_overlap_kernel, dim3((unsigned)((C + OV_WAVES - 1) / OV_WAVES)), dim3(64 * OV_WAVES), 0, (hipStream_t)stream, C,
                       c_off, c_nnz, c_keys, c_w, c_len, (int)n_ref, r_off, r_nnz, r_keys, r_w, r_len, lo, hi, skip, total, match, distinct,
                       unseen, ref_len);
    VC_LAUNCH_CHECK();
    return 0;
}
