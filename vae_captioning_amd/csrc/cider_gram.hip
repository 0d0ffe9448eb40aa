// In-set CIDEr-D (mbr.py: CiderGram): the CIDEr-D of every caption of an image against every caption of the SAME image, and each
// caption's weighted mean over the set -- its expected CIDEr-D under the image's own samples (minimum-Bayes-risk selection) and the
// matrix whose eigenvalues give Self-CIDEr.
//
//   vc_cider_gram   per (image, 4 hypothesis rows): the four hypotheses' keys / weights staged in LDS (12 KiB), thread t scores column t
//                   (reference = caption t of the image) with cider_pair.h's pair function -- vc_consensus_score's bits for the same
//                   pair -- stores the four row entries (coalesced across the threads) and the rows' float64 weighted means.  No pool
//                   list, no sort.
#include "common.h"
#include "cider_pair.h"
#include "vaecap.h"

namespace vc {

constexpr int CG_CPB = 4;          // hypothesis rows per workgroup
constexpr int CG_MAX_CANDS = 256;  // captions per image: one column per thread

// A row's bits depend on the image's captions (and, for mbr, its weights) only: a column is one thread's pair score, and the float64
// sums have a fixed order -- one term per lane, an xor shuffle tree per wave, the four wave sums in wave order.
__global__ __launch_bounds__(256) void cider_gram_kernel(const int32_t* __restrict__ cand_img, int max_cands, int groups,
                                                         const int32_t* __restrict__ off, const int32_t* __restrict__ nnz,
                                                         const uint64_t* __restrict__ keys,
                                                         const float* __restrict__ w, const float* __restrict__ norm,
                                                         const int32_t* __restrict__ words, const double* __restrict__ weight,
                                                         float* __restrict__ gram, long ld, double* __restrict__ mbr) {
    __shared__ uint64_t s_ck[CG_CPB][CP_SLOTS];
    __shared__ float s_cw[CG_CPB][CP_SLOTS];
    __shared__ double s_red[CG_CPB + 1][4];
    const int b = blockIdx.x / groups;
    const int g = blockIdx.x - b * groups;
    const int t = threadIdx.x;
    const int i0 = cand_img[b];
    const int nb = min(cand_img[b + 1] - i0, max_cands);   // (<= 256 = one column per thread; a longer list is cut, never written past ld)
    const int c0 = i0 + g * CG_CPB;
    const int nc = min(CG_CPB, i0 + nb - c0);
    if (nc <= 0) return;   // (uniform over the workgroup, before any barrier)
    CiderHyps<CG_CPB> hyp;
    cider_stage_hyps<CG_CPB>(c0, nc, off, nnz, keys, w, norm, words, s_ck, s_cw, hyp);
    __syncthreads();
    const bool live = t < nb;
    float sc[CG_CPB];
#pragma unroll
    for (int c = 0; c < CG_CPB; ++c) sc[c] = 0.f;
    if (live) {
        cider_pair_scores<CG_CPB>(i0 + t, off, nnz, keys, w, norm, words, s_ck, s_cw, hyp, sc);
        if (gram) {
#pragma unroll
            for (int c = 0; c < CG_CPB; ++c)
                if (c < nc) gram[(long)(c0 + c) * ld + t] = sc[c];
        }
    }
    if (!mbr) return;      // (uniform)
    const double wt = live ? (weight ? weight[i0 + t] : 1.0) : 0.0;
    double acc[CG_CPB + 1];
#pragma unroll
    for (int c = 0; c < CG_CPB; ++c) acc[c] = wt * (double)sc[c];
    acc[CG_CPB] = wt;
#pragma unroll
    for (int c = 0; c <= CG_CPB; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
        if ((t & 63) == 0) s_red[c][t >> 6] = acc[c];
    }
    __syncthreads();
    if (t < nc) {
        const double num = s_red[t][0] + s_red[t][1] + s_red[t][2] + s_red[t][3];
        const double den = s_red[CG_CPB][0] + s_red[CG_CPB][1] + s_red[CG_CPB][2] + s_red[CG_CPB][3];
        mbr[c0 + t] = den != 0.0 ? num / den : 0.0;
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_cider_gram(void* stream, int B, const int32_t* cand_img, int max_cands, const int32_t* off, const int32_t* nnz,
                             const uint64_t* keys, const float* w, const float* norm, const int32_t* words, const double* weight,
                             float* gram, long ld, double* mbr) {
    VC_CHECK_ARG(cand_img && off && nnz && keys && w && norm && words, "null pointer");
    VC_CHECK_ARG(gram || mbr, "at least one of gram and mbr");
    VC_CHECK_ARG(B >= 0 && max_cands >= 0 && max_cands <= CG_MAX_CANDS, "B >= 0, <= 256 captions per image");
    VC_CHECK_ARG(ld >= max_cands, "ld must be >= max_cands");
    if (B == 0 || max_cands == 0) return 0;
    const int groups = (max_cands + CG_CPB - 1) / CG_CPB;
    VC_CHECK_ARG((long)B * groups < (1L << 31), "too many images x row groups for one launch");
    hipLaunchKernelGGL(cider_gram_kernel, dim3((unsigned)(B * groups)), dim3(256), 0, (hipStream_t)stream, cand_img, max_cands, groups, off,
                       nnz, keys, w, norm, words, weight, gram, ld, mbr);
    VC_LAUNCH_CHECK();
    return 0;
}
