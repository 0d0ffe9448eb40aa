// DPP selection (mbr.py: CiderGram.select; definition in include/vaecap.h and DESIGN.md "DPP selection"): n captions of an image chosen
// jointly for quality and for difference from each other -- the fast greedy MAP of a determinantal point process (Chen, Zhang & Zhou,
// NeurIPS 2018) over L = diag(q) S diag(q), S the symmetrised, clipped in-set CIDEr-D matrix that vc_cider_gram has just written.
//
//   vc_dpp_select_f64   one workgroup per image, lane i = caption i.  A lane keeps its d_i, q_i and taken flag in registers; the c_t
//                       vectors of the steps done live in LDS ([step][caption] doubles).  Per step: an index-carrying argmax of d over
//                       the live lanes (xor shuffle tree per wave, the four wave results through LDS in wave order; equal values go to
//                       the lower index), then lane i reads G[j][i] and G[i][j] once, subtracts the k earlier products in ascending
//                       step order and writes c_k[i].  One barrier per step: the argmax slots alternate between two banks, and the
//                       barrier that publishes a step's maxima also publishes the c row of the step before it.
// All arithmetic is float64 without contraction: every lane's d follows the header's sequence of operations term by term.  No atomics;
// an image's outputs depend on its own rows, q and n only.
#include <math.h>
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int DPP_THREADS = 256;   // = the most captions per image: one lane each
constexpr int DPP_MAX_N = 32;

struct DppBest {
    double d;   // -1: no live lane (a live d is > 0)
    int i;
};

// the better of two candidates: the larger d, equal values to the lower index
__device__ __forceinline__ DppBest dpp_better(DppBest a, DppBest b) {
    return (b.d > a.d || (b.d == a.d && b.i < a.i)) ? b : a;
}

template <int NMAX>
__global__ __launch_bounds__(DPP_THREADS) void dpp_select_kernel(const int32_t* __restrict__ cand_img, int max_cands,
                                                                 const float* __restrict__ gram, long ld, const double* __restrict__ q,
                                                                 int n, int32_t* __restrict__ sel, double* __restrict__ gain,
                                                                 int32_t* __restrict__ n_dpp) {
#pragma clang fp contract(off)
    __shared__ double s_c[NMAX * DPP_THREADS];   // c_t[i] at [t * 256 + i]
    __shared__ double s_q[DPP_THREADS];
    __shared__ double s_bd[2][4];                // the waves' maxima, two banks
    __shared__ int s_bi[2][4];
    __shared__ int s_cnt[4];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i0 = cand_img[b];
    const int m = min(max(cand_img[b + 1] - i0, 0), max_cands);   // (<= 256: one lane per caption; a longer list is cut as vc_cider_gram cuts it)
    const int want = min(n, m);
    int32_t* sel_b = sel + (long)b * n;
    double* gain_b = gain + (long)b * n;
    const bool mine = t < m;
    const double qi = mine ? q[i0 + t] : 0.0;
    const double q2 = qi * qi;
    double d = q2;
    bool taken = !mine;
    s_q[t] = qi;
    int k = 0;
    for (; k < want; ++k) {
        DppBest best;
        best.d = (!taken && d > DPP_EPS * q2) ? d : -1.0;
        best.i = t;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            DppBest other;
            other.d = __shfl_xor(best.d, o, 64);
            other.i = __shfl_xor(best.i, o, 64);
            best = dpp_better(best, other);
        }
        const int bank = k & 1;
        if (lane == 0) {
            s_bd[bank][w] = best.d;
            s_bi[bank][w] = best.i;
        }
        __syncthreads();   // the maxima of this step, c of the step before (and, at k == 0, s_q)
        best.d = s_bd[bank][0];
        best.i = s_bi[bank][0];
#pragma unroll
        for (int v = 1; v < 4; ++v) {
            DppBest other;
            other.d = s_bd[bank][v];
            other.i = s_bi[bank][v];
            best = dpp_better(best, other);
        }
        if (best.d < 0.0) break;   // no caption is live (uniform: every lane read the same slots)
        const int j = best.i;
        const double dj = best.d;
        if (t == 0) {
            sel_b[k] = j;
            gain_b[k] = dj;
        }
        if (t == j) taken = true;
        if (!taken) {
            const double s = ((double)gram[(long)(i0 + j) * ld + t] + (double)gram[(long)(i0 + t) * ld + j]) / 20.0;
            const double sim = fmin(1.0, fmax(0.0, s));
            double acc = s_q[j] * sim * qi;
            for (int u = 0; u < k; ++u) acc -= s_c[u * DPP_THREADS + j] * s_c[u * DPP_THREADS + t];
            const double e = acc / sqrt(dj);
            s_c[k * DPP_THREADS + t] = e;
            d -= e * e;
        }
    }
    // the slots the loop left: the untaken captions in ascending index with gain 0, then -1 / 0 up to n
    const int chosen = k;
    const bool left = mine && !taken;
    const unsigned long long mask = __ballot(left);
    if (lane == 0) s_cnt[w] = __popcll(mask);
    __syncthreads();
    int rank = __popcll(mask & ((1ull << lane) - 1ull));
    for (int v = 0; v < w; ++v) rank += s_cnt[v];
    if (left && chosen + rank < want) {
        sel_b[chosen + rank] = t;
        gain_b[chosen + rank] = 0.0;
    }
    if (t >= want && t < n) {
        sel_b[t] = -1;
        gain_b[t] = 0.0;
    }
    if (t == 0) n_dpp[b] = chosen;
}

}  // namespace vc

using namespace vc;

extern "C" int vc_dpp_select_f64(void* stream, int B, const int32_t* cand_img, int max_cands, const float* gram, long ld, const double* q,
                                 int n, int32_t* sel, double* gain, int32_t* n_dpp) {
    VC_CHECK_ARG(B >= 0, "B must be >= 0");
    VC_CHECK_ARG(max_cands >= 1 && max_cands <= DPP_THREADS, "max_cands must be 1..256");
    VC_CHECK_ARG(n >= 1 && n <= DPP_MAX_N, "n must be 1..32");
    VC_CHECK_ARG(ld >= max_cands, "ld must be >= max_cands");
    if (B == 0) return 0;
    VC_CHECK_ARG(cand_img && gram && q, "null operand");
    VC_CHECK_ARG(sel && gain && n_dpp, "null output");
    // the c vectors of n steps: 16 KiB of LDS up to n = 8 (the default selects 5), 64 KiB up to 32; the arithmetic is the same
    if (n <= 8)
        hipLaunchKernelGGL((dpp_select_kernel<8>), dim3((unsigned)B), dim3(DPP_THREADS), 0, (hipStream_t)stream, cand_img, max_cands, gram, ld, q,
                           n, sel, gain, n_dpp);
    else
        hipLaunchKernelGGL((dpp_select_kernel<DPP_MAX_N>), dim3((unsigned)B), dim3(DPP_THREADS), 0, (hipStream_t)stream, cand_img, max_cands,
                           gram, ld, q, n, sel, gain, n_dpp);
    VC_LAUNCH_CHECK();
    return 0;
}
