// Marginal decoding on device: the next-word distribution of a hypothesis under the K-draw mixture p(y | I) ~ 1/K sum_k p(y | z_k, I)
// (generate.py: CaptionGenerator.marginal_greedy / marginal_beam_search; DESIGN.md "Marginal decoding").  A hypothesis group g owns
// the K consecutive rows r = g*K + k of the logits (diverse()'s image-major, draw-minor rows).
//
//   vc_mixture_topk_f32     q_g(v) = sum_k w_r exp(x_rv - M_r) / S_r with w = softmax_k(logw): the kc best words of every group.
//                           Three launches, the vocabulary split across workgroups:
//                             1. mixture_stat_kernel     one workgroup per row: (M_r, log S_r) by row_ops.h's row_max_sum
//                             2. mixture_partial_kernel  one workgroup per (group, 1024-column chunk): the group's weights (K <= 256
//                                                        float64 terms, tree sums in LDS), the chunk's q in registers (four columns
//                                                        per thread, k ascending), the best kc of each wave by shuffles, the four
//                                                        waves' lists ranked by wave 0 -> the chunk's best kc in the workspace
//                             3. mixture_merge_kernel    one wave per group: the best kc of its chunks' lists
//                           Every sum has a fixed order and no launch hands data to another workgroup of the same launch: no atomics,
//                           and a group's outputs depend on its K rows only.  Words are selected by comparing (value, column) pairs
//                           whose columns come from the thread's position: no value read from memory becomes an address.
//   vc_mixture_advance_f32  the chosen word's log-softmax under every draw added to the draws' prefix log-likelihoods (f32 term, f64
//                           sum), the rows' parents and tokens for the next round, and greedy decoding's per-group bookkeeping.
#include <limits.h>

#include "row_ops.h"
#include "vaecap.h"

namespace vc {

constexpr int MIX_CHUNK = 1024;      // columns per workgroup of the partial top-kc: four per thread
constexpr int MIX_MAX_K = 256;       // draws per group: one thread per draw
constexpr int MIX_MAX_KC = 16;       // words per group (vc_beam_update's BEAM_MAX)
constexpr int MIX_MERGE_LDS = 1024;  // chunk lists of up to this many entries are merged from LDS

// One workgroup per row: stat[r] = (M_r, log S_r), the terms of the temperature-1 log-softmax (row_ops.h).
template <bool STAGE>
__global__ __launch_bounds__(256) void mixture_stat_kernel(const float* __restrict__ logits, int V, long ld, float* __restrict__ stat) {
    extern __shared__ float srow[];
    __shared__ float sh[4];
    const long r = blockIdx.x;
    const int t = threadIdx.x;
    const float* p = stage_row<STAGE>(logits + r * ld, V, srow);
    int c0, c1;
    row_chunk(V, c0, c1);
    float mx1, s1;
    row_max_sum(p, c0, c1, sh, mx1, s1);
    if (t == 0) {
        stat[2 * r] = mx1;
        stat[2 * r + 1] = logf(s1);
    }
}

// One workgroup per (chunk of MIX_CHUNK columns, group).  part_v / part_i [G, nchunks, kc]: the chunk's best kc (value, column) pairs,
// best first; a chunk with fewer than kc columns pads with (-2, INT_MAX), below every word (a word's value is >= 0, or -1 when the
// group's rows give no number).
__global__ __launch_bounds__(256) void mixture_partial_kernel(const float* __restrict__ logits, int K, int V, long ld,
                                                              const double* __restrict__ logw, const float* __restrict__ stat, int kc,
                                                              int vec, float* __restrict__ part_v, int32_t* __restrict__ part_i) {
    __shared__ double s_red[256];
    __shared__ float s_coef[MIX_MAX_K], s_m[MIX_MAX_K];
    __shared__ float s_cv[4 * MIX_MAX_KC];
    __shared__ int s_ci[4 * MIX_MAX_KC];
    const int chunk = blockIdx.x, nchunks = gridDim.x, t = threadIdx.x;
    const long g = blockIdx.y, r0 = g * K;
    // ---- the draws' weights: w_k = exp(logw_k - max) / sum (float64; both reductions are the same LDS tree in every launch)
    const double lw = t < K ? logw[r0 + t] : -INFINITY;
    s_red[t] = lw;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) s_red[t] = fmax(s_red[t], s_red[t + o]);
        __syncthreads();
    }
    const double mx = s_red[0];
    __syncthreads();
    const double e = t < K ? exp(lw - mx) : 0.0;
    s_red[t] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) s_red[t] += s_red[t + o];
        __syncthreads();
    }
    if (t < K) {   // w_k / S_k as ONE f32 factor (S from its float64 exponential: log S is what the row statistics keep)
        s_m[t] = stat[2 * (r0 + t)];
        s_coef[t] = (float)((e / s_red[0]) * exp(-(double)stat[2 * (r0 + t) + 1]));
    }
    __syncthreads();
    // ---- q of this thread's four columns, k ascending
    const int c0 = chunk * MIX_CHUNK + t * 4;
    const float* base = logits + r0 * ld;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec && c0 + 3 < V) {   // (16-byte loads of columns < V only: the padding of a row is never read)
        for (int k = 0; k < K; ++k) {
            const float4 x = *reinterpret_cast<const float4*>(base + (long)k * ld + c0);
            const float m = s_m[k], cf = s_coef[k];
            q[0] += cf * __expf(x.x - m);
            q[1] += cf * __expf(x.y - m);
            q[2] += cf * __expf(x.z - m);
            q[3] += cf * __expf(x.w - m);
        }
    } else {
        for (int k = 0; k < K; ++k) {
            const float m = s_m[k], cf = s_coef[k];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c0 + j < V) q[j] += cf * __expf(base[(long)k * ld + c0 + j] - m);
        }
    }
    float v[4];
    int idx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool valid = c0 + j < V;
        v[j] = valid ? (q[j] >= 0.f ? q[j] : -1.f) : -2.f;   // (a NaN compares false: it becomes -1, below every probability)
        idx[j] = valid ? c0 + j : INT_MAX;
    }
    // ---- the wave's best kc: kc rounds of "best pair not taken yet" (registers and shuffles only); lane p keeps the p-th
    const int lane = t & 63, w = t >> 6;
    unsigned taken = 0;
    float mv = -2.f;
    int mi = INT_MAX;
    for (int p = 0; p < kc; ++p) {
        float bv = -3.f;
        int bi = INT_MAX;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!((taken >> j) & 1u) && better(v[j], idx[j], bv, bi)) { bv = v[j]; bi = idx[j]; }
        wave_best(bv, bi);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (idx[j] == bi && v[j] == bv) taken |= 1u << j;
        if (lane == p) { mv = bv; mi = bi; }
    }
    if (lane < MIX_MAX_KC) {
        s_cv[w * MIX_MAX_KC + lane] = mv;
        s_ci[w * MIX_MAX_KC + lane] = mi;
    }
    __syncthreads();
    // ---- the four lists ranked by wave 0: one pair per lane, rank = the pairs that precede it (equal padding pairs: by lane)
    if (w == 0) {
        const float cv = s_cv[lane];
        const int ci = s_ci[lane];
        int rank = 0;
        for (int j = 0; j < 64; ++j) {
            const float ov = __shfl(cv, j, 64);
            const int oi = __shfl(ci, j, 64);
            if (better(ov, oi, cv, ci) || (ov == cv && oi == ci && j < lane)) ++rank;
        }
        if (rank < kc) {
            const long o = (g * nchunks + chunk) * kc + rank;
            part_v[o] = cv;
            part_i[o] = ci;
        }
    }
}

// One wave per group: the best kc of its n = nchunks * kc listed pairs, by kc rounds of "best pair after the previous winner" (the
// order is total over the words, so nothing has to be marked).
__global__ __launch_bounds__(64) void mixture_merge_kernel(const float* __restrict__ part_v, const int32_t* __restrict__ part_i, int n, int kc,
                                                           int V, float* __restrict__ top_p, int32_t* __restrict__ top_i) {
    __shared__ float sv[MIX_MERGE_LDS];
    __shared__ int si[MIX_MERGE_LDS];
    const long g = blockIdx.x;
    const int lane = threadIdx.x;
    const float* pv = part_v + g * n;
    const int32_t* pi = part_i + g * n;
    if (n <= MIX_MERGE_LDS) {
        for (int j = lane; j < n; j += 64) { sv[j] = pv[j]; si[j] = pi[j]; }
        __syncthreads();
        pv = sv;
        pi = si;
    }
    float lv = INFINITY;
    int li = -1;
    for (int p = 0; p < kc; ++p) {
        float bv = -3.f;
        int bi = INT_MAX;
        for (int j = lane; j < n; j += 64) {
            const float v = pv[j];
            const int i = pi[j];
            if (better(lv, li, v, i) && better(v, i, bv, bi)) { bv = v; bi = i; }
        }
        wave_best(bv, bi);
        if (lane == 0) {
            top_p[g * kc + p] = bv;
            top_i[g * kc + p] = min(max(bi, 0), V - 1);
        }
        lv = bv;
        li = bi;
    }
}

// One workgroup per new group, thread k = draw k.
__global__ __launch_bounds__(256) void mixture_advance_kernel(const float* __restrict__ logits, int V, long ld, const float* __restrict__ stat,
                                                              int Gn, int K, const int32_t* __restrict__ parent, const int32_t* __restrict__ tok,
                                                              const double* __restrict__ logw_in, double* __restrict__ logw_out,
                                                              int32_t* __restrict__ parent_rows, int32_t* __restrict__ tok_rows, int eos,
                                                              int32_t* __restrict__ done, int32_t* __restrict__ seq, int Lmax,
                                                              int32_t* __restrict__ len) {
    const long g = blockIdx.x;
    const int k = threadIdx.x;
    const int w = tok[g];
    const long pg = parent ? min(max(parent[g], 0), Gn - 1) : g;
    bool was_done = false, live = true;
    int n = 0;
    if (done) {
        was_done = done[g] != 0;
        n = len[g];
        live = !was_done && n >= 0 && n < Lmax;
    }
    __syncthreads();   // every thread has read the group's flags before thread 0 changes them
    if (k < K) {
        const long src = pg * K + k, dst = g * K + k;
        double lw = logw_in[src];
        if (live) {
            const float lsm = lsm_term(logits[src * ld + min(max(w, 0), V - 1)], stat[2 * src], stat[2 * src + 1]);
            lw += (double)lsm;
        }
        logw_out[dst] = lw;
        if (parent_rows) parent_rows[dst] = (int32_t)src;
        tok_rows[dst] = w;
    }
    if (done && k == 0 && !was_done) {
        if (live) {
            seq[g * Lmax + n] = w;
            len[g] = n + 1;
        }
        done[g] = w == eos ? 1 : 0;
    }
}

}  // namespace vc

using namespace vc;

extern "C" size_t vc_mixture_topk_workspace_bytes(long G, int V, int kc) {
    if (G <= 0 || V <= 0 || kc <= 0) return 0;
    return (size_t)G * (size_t)cdiv(V, MIX_CHUNK) * (size_t)kc * (sizeof(float) + sizeof(int32_t));
}

extern "C" int vc_mixture_topk_f32(void* stream, const float* logits, long G, int K, int V, long ld, const double* logw, int kc, float* top_p,
                                   int32_t* top_i, float* stat, void* ws, size_t ws_bytes) {
    VC_CHECK_ARG(logits && logw && top_p && top_i && stat && ws, "null pointer");
    VC_CHECK_ARG(G > 0 && G <= 65535 && V > 0 && ld >= V, "bad shape (1 <= G <= 65535, ld >= V)");
    VC_CHECK_ARG(K >= 1 && K <= MIX_MAX_K, "K must be 1..256");
    VC_CHECK_ARG(kc >= 1 && kc <= MIX_MAX_KC && kc <= V, "kc must be 1..16 and <= V");
    if (ws_bytes < vc_mixture_topk_workspace_bytes(G, V, kc))
        return fail(VC_EWORKSPACE, "%s: workspace too small (%ld bytes, vc_mixture_topk_workspace_bytes = %ld)", __func__, (long)ws_bytes,
                    (long)vc_mixture_topk_workspace_bytes(G, V, kc));
    const hipStream_t st = (hipStream_t)stream;
    const long rows = G * K;
    const int nchunks = cdiv(V, MIX_CHUNK);
    float* part_v = (float*)ws;
    int32_t* part_i = (int32_t*)(part_v + G * nchunks * kc);
    if (V <= ROW_LDS_MAX)
        hipLaunchKernelGGL(mixture_stat_kernel<true>, dim3((unsigned)rows), dim3(256), (size_t)V * sizeof(float), st, logits, V, ld, stat);
    else
        hipLaunchKernelGGL(mixture_stat_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, logits, V, ld, stat);
    VC_LAUNCH_CHECK();
    const int vec = (ld % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(mixture_partial_kernel, dim3(nchunks, (unsigned)G), dim3(256), 0, st, logits, K, V, ld, logw, stat, kc, vec, part_v, part_i);
    VC_LAUNCH_CHECK();
    hipLaunchKernelGGL(mixture_merge_kernel, dim3((unsigned)G), dim3(64), 0, st, part_v, part_i, nchunks * kc, kc, V, top_p, top_i);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_mixture_advance_f32(void* stream, const float* logits, int V, long ld, const float* stat, long Gn, int K,
                                      const int32_t* parent, const int32_t* tok, const double* logw_in, double* logw_out,
                                      int32_t* parent_rows, int32_t* tok_rows, int eos, int32_t* done, int32_t* seq, int Lmax, int32_t* len) {
    VC_CHECK_ARG(logits && stat && tok && logw_in && logw_out && tok_rows, "null pointer");
    VC_CHECK_ARG(logw_in != logw_out, "logw_in and logw_out must be different buffers (a group reads its parent's rows)");
    VC_CHECK_ARG(Gn > 0 && Gn <= INT_MAX / MIX_MAX_K && V > 0 && ld >= V, "bad shape");
    VC_CHECK_ARG(K >= 1 && K <= MIX_MAX_K, "K must be 1..256");
    VC_CHECK_ARG((done && seq && len && Lmax > 0 && !parent) || (!done && !seq && !len),
                 "greedy form: done, seq, len with Lmax > 0 and no parent; beam form: none of the three");
    hipLaunchKernelGGL(mixture_advance_kernel, dim3((unsigned)Gn), dim3(256), 0, (hipStream_t)stream, logits, V, ld, stat, (int)Gn, K, parent, tok,
                       logw_in, logw_out, parent_rows, tok_rows, eos, done, seq, Lmax, len);
    VC_LAUNCH_CHECK();
    return 0;
}
