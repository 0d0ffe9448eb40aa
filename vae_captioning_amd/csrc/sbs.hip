// Stochastic beam search on device (Kool, van Hoof, Welling, ICML 2019: Gumbel top-k): n distinct captions per image, an exact sample
// WITHOUT replacement from the model (generate.py: CaptionGenerator.stochastic_beam_search; DESIGN.md "Stochastic beam search").
// Beam rows are image-major: row r = b*n + i is entry i of image b.
//
//   vc_sbs_init        the starting state of every image, the image states expanded to the beam rows.
//   vc_sbs_expand_f32  one workgroup per live, unfinished row: the f32 log-softmax of the row over the full vocabulary
//                      (row_ops.h: the same bits as vc_decode_pick_f32's), a float64 Gumbel per word (injected,
//                      or from Philox) and the kc best words by key = (double)lsm + g.  The row is staged in LDS (one read from
//                      memory); every thread holds the keys of its columns in registers (twelve Philox quads = 48 columns per
//                      tile of 12 288); every wave picks its best kc by kc rounds of "best pair after the previous winner"
//                      (registers and shuffles only), wave 0 merges the four lists with the tiles before.  No atomics, every sum in a
//                      fixed order, (key, column) pairs whose columns come from the thread's position.
//   vc_sbs_update      one wave per image: the conditioned perturbed score G' of every candidate (the kc children of every live
//                      entry, every finished entry itself) in parallel, then the best n + 1 of them by n + 1 rounds of "best triple
//                      after the previous winner" under the total order (G' descending, parent ascending, word ascending) -- no heap,
//                      no sequential walk --, the new entries in rank order, the (n+1)-th into kappa, and the sentence copies.
#include <float.h>
#include <limits.h>

#include "beam_heap.h"
#include "row_ops.h"

namespace vc {

constexpr int SBS_MAX_N = 32;         // entries per image: one lane each, n + 1 winners <= 64
constexpr int SBS_MAX_KC = 33;        // candidates per row: n + 1 (the (n+1)-th largest perturbed score is exact only then)
constexpr int SBS_QPT = 12;           // Philox quads per thread and tile: 48 float64 keys in registers
constexpr int SBS_TILE_Q = 256 * SBS_QPT;
constexpr int SBS_LISTS = 5;          // the four waves' lists + the best kc of the tiles before
constexpr int SBS_SLOTS = (SBS_MAX_N * SBS_MAX_KC + 63) / 64;   // candidates per lane of vc_sbs_update

__device__ __forceinline__ double sbs_sane(double k) { return k == k ? k : -INFINITY; }   // a NaN ranks below every number

template <bool STAGE>
__global__ __launch_bounds__(256) void sbs_expand_kernel(const float* __restrict__ logits, long rows, int n, int V, long ld,
                                                         const int32_t* __restrict__ count, const int32_t* __restrict__ done, int kc,
                                                         const double* __restrict__ gumbel, int g_rounds, const int32_t* __restrict__ round,
                                                         uint64_t seed, uint64_t offset, const int32_t* __restrict__ step,
                                                         double* __restrict__ cand_key, float* __restrict__ cand_lsm,
                                                         int32_t* __restrict__ cand_idx) {
    extern __shared__ float srow[];
    __shared__ float sh[4];
    __shared__ double s_k[SBS_LISTS * SBS_MAX_KC];
    __shared__ int s_i[SBS_LISTS * SBS_MAX_KC];
    const long r = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if ((int)(r % n) >= count[r / n] || done[r] != 0) return;   // (the same for every thread of the workgroup)
    const float* p = stage_row<STAGE>(logits + r * ld, V, srow);
    // ---- M and S (row_ops.h)
    int c0, c1;
    row_chunk(V, c0, c1);
    float mx1, s1;
    row_max_sum(p, c0, c1, sh, mx1, s1);
    const float ls = logf(s1);
    // ---- the noise: element r*V + v of the call's stream; a thread takes whole Philox quads of the flat index
    const int rd = round ? round[0] : 0;
    const uint32_t k1 = (uint32_t)(seed >> 32) + (uint32_t)rd + (step ? (uint32_t)step[0] : 0u);
    const long base = r * (long)V;
    const int off = (int)(base & 3);
    const long q0 = base >> 2;
    const int nq = (off + V + 3) >> 2;
    const double* gp = gumbel ? gumbel + ((long)min(max(rd, 0), g_rounds - 1) * rows + r) * (long)V : nullptr;
    if (t < SBS_MAX_KC) {   // the list of the tiles before: empty
        s_k[4 * SBS_MAX_KC + t] = -INFINITY;
        s_i[4 * SBS_MAX_KC + t] = INT_MAX;
    }
    double mk = -INFINITY;   // (wave 0) lane p: the p-th best pair so far
    int mi = INT_MAX;
    for (int tq0 = 0; tq0 < nq; tq0 += SBS_TILE_Q) {
        double key[SBS_QPT * 4];
#pragma unroll
        for (int j = 0; j < SBS_QPT; ++j) {
            const int lq = tq0 + j * 256 + t;
            uint32_t rr[4] = {0u, 0u, 0u, 0u};
            if (!gumbel && lq < nq) {
                const long q = q0 + lq;
                philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, k1, rr);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = 4 * lq + e - off;
                double k = -INFINITY;
                if (lq < nq && v >= 0 && v < V) {
                    double g;
                    if (gumbel) {
                        g = gp[v];
                    } else {
                        const double u = ((double)rr[e] + 0.5) * 2.3283064365386963e-10;   // (0, 1): never 0 or 1
                        g = -log(-log(u));
                    }
                    const float lsm = lsm_term(p[v], mx1, ls);
                    k = sbs_sane((double)lsm + g);
                }
                key[j * 4 + e] = k;
            }
        }
        // ---- the wave's best kc of the tile: lane p keeps the p-th
        double pk = INFINITY, wk = -INFINITY;
        int pi = -1, wi = INT_MAX;
        for (int pp = 0; pp < kc; ++pp) {
            double bk = -INFINITY;
            int bi = INT_MAX;
#pragma unroll
            for (int j = 0; j < SBS_QPT; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int v = 4 * (tq0 + j * 256 + t) + e - off;
                    const int idx = (v >= 0 && v < V) ? v : INT_MAX;
                    const double k = key[j * 4 + e];
                    if (better(pk, pi, k, idx) && better(k, idx, bk, bi)) { bk = k; bi = idx; }
                }
            }
            wave_best(bk, bi);
            if (lane == pp) { wk = bk; wi = bi; }
            pk = bk;
            pi = bi;
            if (bi == INT_MAX) break;   // nothing is left (the same in every lane)
        }
        __syncthreads();   // (the lists of the tile before have been read)
        if (lane < SBS_MAX_KC) {
            s_k[w * SBS_MAX_KC + lane] = wk;
            s_i[w * SBS_MAX_KC + lane] = wi;
        }
        __syncthreads();
        // ---- wave 0: the best kc of the five lists (three pairs per lane)
        if (w == 0) {
            double ek[3];
            int ei[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int s = lane + 64 * j;
                const bool have = s < SBS_LISTS * SBS_MAX_KC;
                ek[j] = have ? s_k[s] : -INFINITY;
                ei[j] = have ? s_i[s] : INT_MAX;
            }
            pk = INFINITY;
            pi = -1;
            mk = -INFINITY;
            mi = INT_MAX;
            for (int pp = 0; pp < kc; ++pp) {
                double bk = -INFINITY;
                int bi = INT_MAX;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (better(pk, pi, ek[j], ei[j]) && better(ek[j], ei[j], bk, bi)) { bk = ek[j]; bi = ei[j]; }
                wave_best(bk, bi);
                if (lane == pp) { mk = bk; mi = bi; }
                pk = bk;
                pi = bi;
            }
        }
        __syncthreads();   // (wave 0 has read the five lists)
        if (w == 0 && lane < SBS_MAX_KC) {
            s_k[4 * SBS_MAX_KC + lane] = mk;
            s_i[4 * SBS_MAX_KC + lane] = mi;
        }
    }
    if (w == 0 && lane < kc) {
        const int idx = min(max(mi, 0), V - 1);   // (kc <= V: every listed pair is a word)
        const long o = r * kc + lane;
        cand_key[o] = mk;
        cand_lsm[o] = lsm_term(p[idx], mx1, ls);
        cand_idx[o] = idx;
    }
}

struct SbsState {
    int B, n, Lmax, bos, eos;
    int32_t *count, *p_len, *p_done, *sent_next, *parent, *tok, *round;
    const int32_t* sent_cur;
    double *p_phi, *p_G, *kappa;
};

__device__ __forceinline__ double sbs_log1mexp(double x) { return x > -0.6931471805599453 ? log(-expm1(x)) : log1p(-exp(x)); }

// (G' descending, parent ascending, word ascending) with tie = parent << 32 | word: a strict total order over the candidates
__device__ __forceinline__ bool sbs_before(double ga, long long ta, double gb, long long tb) { return ga > gb || (ga == gb && ta < tb); }

__global__ __launch_bounds__(64) void sbs_update_kernel(SbsState a, int kc, const double* __restrict__ cand_key,
                                                        const float* __restrict__ cand_lsm, const int32_t* __restrict__ cand_idx) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, L = a.Lmax;
    const long r0 = (long)b * n;
    const int cnt = min(max(__builtin_amdgcn_readfirstlane(a.count[b]), 0), n);
    // ---- entry `lane` of the image, read before anything is written (the state is updated in place)
    double e_phi = 0.0, e_G = 0.0;
    int e_len = 1, e_done = 1;
    if (lane < cnt) {
        e_phi = a.p_phi[r0 + lane];
        e_G = a.p_G[r0 + lane];
        e_len = min(max(a.p_len[r0 + lane], 0), L);
        e_done = (a.p_done[r0 + lane] != 0 || e_len >= L) ? 1 : 0;
    }
    const double kap = a.kappa[b];
    __syncthreads();
    int ncand = lane < cnt ? (e_done ? 1 : kc) : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ncand += __shfl_xor(ncand, o, 64);
    // ---- the candidates: slot q = i*kc + c is child c of entry i (a finished entry: c = 0 only, itself)
    const int total = cnt * kc;
    double cg[SBS_SLOTS];
    long long ct[SBS_SLOTS];
#pragma unroll
    for (int s = 0; s < SBS_SLOTS; ++s) {
        cg[s] = -INFINITY;
        ct[s] = LLONG_MAX;
        if (s * 64 < total) {   // (the same in every lane)
            const int q = s * 64 + lane;
            const bool have = q < total;
            const int i = have ? q / kc : 0, c = have ? q - i * kc : 0;
            const double phi_i = __shfl(e_phi, i, 64), G_i = __shfl(e_G, i, 64);
            const int fin = __shfl(e_done, i, 64);
            if (have && fin) {
                if (c == 0) {
                    cg[s] = sbs_sane(G_i);
                    ct[s] = ((long long)i << 32) | (unsigned)a.eos;
                }
            } else if (have) {
                const long o = (r0 + i) * kc;
                const double Gt = phi_i + cand_key[o + c], Z = phi_i + cand_key[o];
                const double x = Gt - Z;
                double g = G_i;   // the arg-max child keeps its parent's G exactly
                if (c > 0 && x != 0.0) {
                    const double tt = G_i - Gt + sbs_log1mexp(x);
                    g = G_i - fmax(0.0, tt) - log1p(exp(-fabs(tt)));
                }
                cg[s] = sbs_sane(g);
                ct[s] = ((long long)i << 32) | (unsigned)min(max(cand_idx[o + c], 0), INT_MAX);
            }
        }
    }
    // ---- the best n + 1 in order: lane j keeps the j-th (its G', parent and word, and its slot)
    const int m = min(n, ncand), picks = min(n + 1, ncand);
    double pg = INFINITY, wg = 0.0;
    long long ptie = -1, wt = 0;
    int wq = 0;
    for (int pp = 0; pp < picks; ++pp) {
        double bg = -INFINITY;
        long long bt = LLONG_MAX;
        int bq = 0;
#pragma unroll
        for (int s = 0; s < SBS_SLOTS; ++s)
            if (s * 64 < total && sbs_before(pg, ptie, cg[s], ct[s]) && sbs_before(cg[s], ct[s], bg, bt)) { bg = cg[s]; bt = ct[s]; bq = s * 64 + lane; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double og = __shfl_xor(bg, o, 64);
            const long long ot = __shfl_xor(bt, o, 64);
            const int oq = __shfl_xor(bq, o, 64);
            if (sbs_before(og, ot, bg, bt)) { bg = og; bt = ot; bq = oq; }
        }
        if (lane == pp) { wg = bg; wt = bt; wq = bq; }
        pg = bg;
        ptie = bt;
    }
    // ---- the new entries (rank order), the rows of the next round, kappa
    const bool won = lane < m;
    const int i_w = won ? min(max((int)(wt >> 32), 0), n - 1) : 0;
    const int word = (int)(wt & 0xffffffffLL);
    const double phi_i = __shfl(e_phi, i_w, 64);
    const int len_i = __shfl(e_len, i_w, 64), fin = __shfl(e_done, i_w, 64);
    int new_len = 1, tk = a.bos;
    if (lane < n) {
        const long o = r0 + lane;
        if (won) {
            const int c = min(max(wq - i_w * kc, 0), kc - 1);
            new_len = fin ? len_i : len_i + 1;
            tk = fin ? a.eos : word;
            a.p_phi[o] = fin ? phi_i : phi_i + (double)cand_lsm[(r0 + i_w) * kc + c];
            a.p_G[o] = wg;
            a.p_len[o] = new_len;
            a.p_done[o] = (fin || word == a.eos || new_len >= L) ? 1 : 0;
            a.parent[o] = (int32_t)(r0 + i_w);
            a.tok[o] = tk;
        } else {   // an empty slot: finished (no round expands it), continues its own row
            a.p_phi[o] = 0.0; a.p_G[o] = 0.0; a.p_len[o] = 1; a.p_done[o] = 1;
            a.parent[o] = (int32_t)o;
            a.tok[o] = a.bos;
        }
    }
    if (lane == n && ncand > n) a.kappa[b] = fmax(kap, wg);   // the best candidate NOT taken
    if (lane == 0) {
        a.count[b] = m;
        if (a.round && b == 0) a.round[0] += 1;
    }
    // ---- the sentences: the parent's words, plus the new one
    const int32_t* cur = a.sent_cur + r0 * L;
    int32_t* nxt = a.sent_next + r0 * L;
    for (int j = 0; j < m; ++j) {
        const int src = __shfl(i_w, j, 64), keep = __shfl(fin ? len_i : min(len_i, L - 1), j, 64), len = __shfl(new_len, j, 64);
        const int last = __shfl(tk, j, 64);
        for (int tt = lane; tt < len; tt += 64) nxt[j * L + tt] = tt < keep ? cur[src * L + tt] : last;
    }
}

__global__ __launch_bounds__(256) void sbs_init_kernel(SbsState a, int H, const float* __restrict__ c_in, const float* __restrict__ h_in,
                                                       float* __restrict__ c_out, float* __restrict__ h_out, int32_t* __restrict__ sent_cur) {
    const long M = (long)a.B * a.n, stride = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
    beam_rows_init(M, a.n, a.Lmax, H, a.bos, t0, stride, c_in, h_in, c_out, h_out, sent_cur, a.sent_next);
    for (long i = t0; i < M; i += stride) {
        a.p_phi[i] = 0.0; a.p_G[i] = 0.0; a.p_len[i] = 1;
        a.p_done[i] = i % a.n == 0 ? 0 : 1;
        a.parent[i] = (int32_t)i; a.tok[i] = a.bos;
    }
    for (long i = t0; i < a.B; i += stride) {
        a.count[i] = 1;
        a.kappa[i] = -INFINITY;
    }
    if (a.round && t0 == 0) a.round[0] = 0;
}

}  // namespace vc

using namespace vc;

extern "C" int vc_sbs_init(void* stream, int B, int n, int Lmax, int bos, int H, const float* c_in, const float* h_in, float* c_out,
                           float* h_out, int32_t* count, double* p_phi, double* p_G, int32_t* p_len, int32_t* p_done, int32_t* sent_cur,
                           int32_t* sent_next, double* kappa, int32_t* parent, int32_t* tok, int32_t* round) {
    VC_CHECK_ARG(B > 0 && n >= 1 && n <= SBS_MAX_N && Lmax > 1 && H > 0 && (long)B * n <= INT_MAX, "bad shape (1 <= n <= 32, Lmax > 1)");
    VC_CHECK_ARG(c_in && h_in && c_out && h_out && count && p_phi && p_G && p_len && p_done && sent_cur && sent_next && kappa && parent && tok,
                 "null pointer");
    SbsState a;
    a.B = B; a.n = n; a.Lmax = Lmax; a.bos = bos; a.eos = 0;
    a.count = count; a.p_len = p_len; a.p_done = p_done; a.sent_cur = sent_cur; a.sent_next = sent_next; a.parent = parent; a.tok = tok;
    a.round = round; a.p_phi = p_phi; a.p_G = p_G; a.kappa = kappa;
    const long work = (long)B * n * (H > Lmax ? H : Lmax);
    hipLaunchKernelGGL(sbs_init_kernel, dim3((unsigned)(cdiv(work, 256L) < 1024 ? cdiv(work, 256L) : 1024)), dim3(256), 0, (hipStream_t)stream, a,
                       H, c_in, h_in, c_out, h_out, sent_cur);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_sbs_expand_f32(void* stream, const float* logits, long rows, int n, int V, long ld, const int32_t* count,
                                 const int32_t* done, int kc, const double* gumbel, int g_rounds, const int32_t* round, uint64_t seed,
                                 uint64_t offset, const int32_t* step, double* cand_key, float* cand_lsm, int32_t* cand_idx) {
    VC_CHECK_ARG(logits && count && done && cand_key && cand_lsm && cand_idx, "null pointer");
    VC_CHECK_ARG(rows > 0 && rows <= INT_MAX && n >= 1 && n <= SBS_MAX_N && rows % n == 0, "bad shape (rows = images * n, 1 <= n <= 32)");
    VC_CHECK_ARG(V > 0 && ld >= V, "bad shape (ld >= V)");
    VC_CHECK_ARG(kc >= 1 && kc <= SBS_MAX_KC && kc <= V, "kc must be 1..33 and <= V");
    VC_CHECK_ARG(!gumbel || g_rounds >= 1, "g_rounds must be >= 1 with injected noise");
    if (V <= ROW_LDS_MAX)
        hipLaunchKernelGGL(sbs_expand_kernel<true>, dim3((unsigned)rows), dim3(256), (size_t)V * sizeof(float), (hipStream_t)stream, logits, rows, n, V,
                           ld, count, done, kc, gumbel, g_rounds, round, seed, offset, step, cand_key, cand_lsm, cand_idx);
    else
        hipLaunchKernelGGL(sbs_expand_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, rows, n, V, ld, count, done,
                           kc, gumbel, g_rounds, round, seed, offset, step, cand_key, cand_lsm, cand_idx);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_sbs_update(void* stream, int B, int n, int kc, int Lmax, int bos, int eos, const double* cand_key, const float* cand_lsm,
                             const int32_t* cand_idx, int32_t* count, double* p_phi, double* p_G, int32_t* p_len, int32_t* p_done,
                             const int32_t* sent_cur, int32_t* sent_next, double* kappa, int32_t* parent, int32_t* tok, int32_t* round) {
    VC_CHECK_ARG(B > 0 && n >= 1 && n <= SBS_MAX_N && Lmax > 1 && (long)B * n <= INT_MAX, "bad shape (1 <= n <= 32, Lmax > 1)");
    VC_CHECK_ARG(kc >= 1 && kc <= SBS_MAX_KC, "kc must be 1..33");
    VC_CHECK_ARG(cand_key && cand_lsm && cand_idx && count && p_phi && p_G && p_len && p_done && sent_cur && sent_next && kappa && parent && tok,
                 "null pointer");
    VC_CHECK_ARG(sent_cur != sent_next, "sent_cur and sent_next must be different buffers (an entry reads its parent's words)");
    SbsState a;
    a.B = B; a.n = n; a.Lmax = Lmax; a.bos = bos; a.eos = eos;
    a.count = count; a.p_len = p_len; a.p_done = p_done; a.sent_cur = sent_cur; a.sent_next = sent_next; a.parent = parent; a.tok = tok;
    a.round = round; a.p_phi = p_phi; a.p_G = p_G; a.kappa = kappa;
    hipLaunchKernelGGL(sbs_update_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a, kc, cand_key, cand_lsm, cand_idx);
    VC_LAUNCH_CHECK();
    return 0;
}
