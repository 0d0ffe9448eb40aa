// ROUGE-L counts (evaluate.py: lcs_overlap, CaptionEvaluator; scst.py: RougeReward): the longest common subsequence (LCS) of a
// hypothesis caption with every row of a contiguous range of reference rows, on the word rows consensus.word_rows makes.
//
//   vc_lcs_overlap   per hypothesis row (one wave): lane i holds hypothesis word i.  A reference row is loaded coalesced (lane j: word
//                    j; the next row's load is issued before the current row is worked on); its words are broadcast one by one
//                    (v_readlane: the index is wave-uniform) and compared by all lanes at once, so the match mask M of a reference word
//                    against the whole hypothesis is one v_cmp into a scalar register pair.  The LCS row state is ONE wave-uniform
//                    64-bit integer V (bit i clear: the LCS grows at hypothesis word i), advanced per reference word by the
//                    bit-parallel recurrence of Crochemore et al. (2001) / Hyyro (2004):
//                        U = V & M;   V = (V + U) | (V - U)      (modulo 2^64: the carry out of bit 63 is dropped on purpose)
//                    and LCS = L_c - popcount(V & low_mask(L_c)).  Integers only; no LDS, no atomics, no barrier: a row's result
//                    depends on nothing but the row and its range.
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int LCS_WAVES = 4;    // hypotheses per workgroup, one wave each (as vc_ngram_overlap)
constexpr int LCS_WORDS = 64;   // words per caption: one per lane, one per bit of V

__device__ __forceinline__ int lcs_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ uint64_t lcs_low_mask(int n) {   // bits 0 .. n-1, 0 <= n <= 64 (a shift by 64 is not a shift)
    return n >= 64 ? ~0ull : (1ull << n) - 1ull;
}

__global__ __launch_bounds__(64 * LCS_WAVES) void lcs_overlap_kernel(long C, const int32_t* __restrict__ c_tok, long c_ld,
                                                                     const int32_t* __restrict__ c_len, int n_ref,
                                                                     const int32_t* __restrict__ r_tok, long r_ld,
                                                                     const int32_t* __restrict__ r_len, const int32_t* __restrict__ lo,
                                                                     const int32_t* __restrict__ hi, const int32_t* __restrict__ skip,
                                                                     int32_t* __restrict__ lcs_max, int32_t* __restrict__ rec_lcs,
                                                                     int32_t* __restrict__ rec_len) {
    const int wv = lcs_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * LCS_WAVES + wv;
    if (c >= C) return;   // wave-uniform; the waves of a workgroup share nothing
    const int c_cap = (int)min((long)LCS_WORDS, c_ld), r_cap = (int)min((long)LCS_WORDS, r_ld);
    const int lc = lcs_uniform(min(max(c_len[c], 0), c_cap));
    const int r0 = lcs_uniform(min(max(lo[c], 0), n_ref));   // the range clamped into [0, n_ref]; lo > hi: empty
    const int r1 = lcs_uniform(min(max(hi[c], r0), n_ref));
    const int sk = lcs_uniform(skip[c]);
    const int32_t mine = lane < lc ? c_tok[c * c_ld + lane] : 0;   // (words at and past len are never read)
    const uint64_t valid = lcs_low_mask(lc);                        // padding lanes stay out of every match mask
    int best_max = 0, best_lcs = 0, best_len = 0;                   // best_len == 0: no row has qualified yet
    int nl = 0;
    int32_t nw = 0;
    if (r0 < r1) {
        nl = min(max(r_len[r0], 0), r_cap);
        nw = lane < nl ? r_tok[(long)r0 * r_ld + lane] : 0;
    }
    for (int r = r0; r < r1; ++r) {
        const int lr = lcs_uniform(nl);
        const int32_t words = nw;
        if (r + 1 < r1) {   // the next row's load is in flight while this row's chain runs
            nl = min(max(r_len[r + 1], 0), r_cap);
            nw = lane < nl ? r_tok[(long)(r + 1) * r_ld + lane] : 0;
        }
        if (r == sk || lr == 0) continue;   // only rows with at least one word take part
        uint64_t V = ~0ull;
        for (int j = 0; j < lr; ++j) {
            const int32_t w = __builtin_amdgcn_readlane(words, j);
            const uint64_t M = __ballot(mine == w) & valid;
            const uint64_t U = V & M;
            V = (V + U) | (V - U);
        }
        const int l = lc - __popcll(V & valid);
        best_max = max(best_max, l);
        // the larger l / lr by cross-multiplication (products <= 64 * 64); a tie in the ratio goes to the smaller lr
        const int a = l * best_len, b = best_lcs * lr;
        if (best_len == 0 || a > b || (a == b && lr < best_len)) {
            best_lcs = l;
            best_len = lr;
        }
    }
    if (lane == 0) {
        lcs_max[c] = best_max;
        rec_lcs[c] = best_lcs;
        rec_len[c] = best_len;
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_lcs_overlap(void* stream, long C, const int32_t* c_tok, long c_ld, const int32_t* c_len, long n_ref, const int32_t* r_tok,
                              long r_ld, const int32_t* r_len, const int32_t* lo, const int32_t* hi, const int32_t* skip, int32_t* lcs_max,
                              int32_t* rec_lcs, int32_t* rec_len) {
    VC_CHECK_ARG(C >= 0 && n_ref >= 0 && n_ref < (1L << 31), "C >= 0 and 0 <= n_ref < 2^31");
    VC_CHECK_ARG(c_ld >= 1 && r_ld >= 1, "c_ld >= 1 and r_ld >= 1");
    VC_CHECK_ARG((C + LCS_WAVES - 1) / LCS_WAVES < (1L << 31), "too many hypothesis rows for one launch");
    if (C == 0) return 0;
    VC_CHECK_ARG(c_tok && c_len && r_tok && r_len && lo && hi && skip && lcs_max && rec_lcs && rec_len, "null pointer");
    hipLaunchKernelGGL(lcs_overlap_kernel, dim3((unsigned)((C + LCS_WAVES - 1) / LCS_WAVES)), dim3(64 * LCS_WAVES), 0, (hipStream_t)stream, C,
                       c_tok, c_ld, c_len, (int)n_ref, r_tok, r_ld, r_len, lo, hi, skip, lcs_max, rec_lcs, rec_len);
    VC_LAUNCH_CHECK();
    return 0;
}
