// Consensus re-ranking of diverse captions (consensus.py: ConsensusIndex; Devlin et al. 2015): the k nearest index images of a query
// by cosine of fc2 features, their human captions pooled, and every candidate caption scored by its mean CIDEr-D agreement with its m
// best-matching pool captions.  The cosine products go through vc_gemm_f32 (normalised queries x normalised index, tb = 1).
//
//   vc_l2_normalize_rows_f32   y = x / |x| per row (zero rows stay zero); one workgroup per row
//   vc_topk_rows_wide_f32      per-row top-k (k <= 256) of wide rows in vc_topk_rows_f32's order, one read of each row: the best k of
//                              each 4096-column chunk selected in LDS by a 64-bit (value, index) key, the lists merged 4096 keys per
//                              workgroup
//   vc_ngram_vectors           per caption (one wave): its words, sorted distinct 1..4-gram keys, count * idf weights, the four norms
//   vc_consensus_score         per (image, 4 candidates): the pool of the neighbours' captions, CIDEr-D of every (candidate, pool
//                              caption) pair in f32 (cider_pair.h: the one definition of the pair score, shared with
//                              cider_gram.hip), each candidate's m' best sorted in LDS, their float64 mean
#include "common.h"
#include "cider_pair.h"
#include "vaecap.h"

namespace vc {

constexpr int TOPKW_CHUNK = 4096;     // keys per workgroup (32 KiB of LDS)
constexpr int TOPKW_MAX_K = 256;
constexpr int NG_MAX_WORDS = 64;      // words per caption
constexpr int NG_SLOTS = CP_SLOTS;    // 4 * 64 n-gram slots (64 + 63 + 62 + 61 used at most)
constexpr int CS_CPB = 4;             // candidates per scoring workgroup
constexpr int CS_MAX_POOL = 2048;
constexpr int CS_MAX_K = 256;

__device__ __forceinline__ int next_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// (value descending, index ascending) as ONE unsigned descending order: the float's bits made monotone (+0 and -0 equal, as their
// comparison is) above the complemented index.  A real key is never 0 (the monotone bits of -inf are 0x007fffff): 0 pads a list.
__device__ __forceinline__ uint64_t topk_key(float v, int c) {
    uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint64_t)(0xffffffffu - (uint32_t)c);
}

// bitonic sort of s[0, N) (N a power of two) with NT threads; DESC = largest first
template <int NT, bool DESC, typename T>
__device__ __forceinline__ void bitonic_sort(T* s, int N) {
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (N >> 1); i += NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = ((lo & size) == 0) == DESC;   // this pair's half is ordered largest first
                const T a = s[lo], b = s[hi];
                if (up ? (a < b) : (b < a)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// The K2 (a power of two, <= N) largest of s[0, N) sorted largest first into s[0, K2): K2-blocks sorted in alternating directions,
// then halving rounds -- block p <- max(block 2p [descending], block 2p+1 [ascending]) element-wise, a bitonic sequence holding the K2
// largest of both, merged in its own direction -- until one block is left.  (A full sort of 4096 keys costs 78 stages of 2048
// compare-exchanges; this one 28 + ~8 shrinking stages per round for K2 = 128.)
template <int NT>
__device__ __forceinline__ void bitonic_topk_desc(uint64_t* s, int N, int K2) {
    for (int size = 2; size <= K2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (N >> 1); i += NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = s[lo], b = s[hi];
                if (desc ? (a < b) : (b < a)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
    constexpr int PER = TOPKW_CHUNK / 2 / NT;
    for (int nb = N / K2; nb > 1; nb >>= 1) {
        const int half = (nb >> 1) * K2;
        uint64_t v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + j * NT;
            if (i < half) {
                const int p = i / K2, e = i - p * K2;
                const uint64_t a = s[2 * p * K2 + e], b = s[(2 * p + 1) * K2 + e];
                v[j] = a > b ? a : b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + j * NT;
            if (i < half) s[i] = v[j];
        }
        __syncthreads();
        for (int stride = K2 >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (half >> 1); i += NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & K2) == 0;
                const uint64_t a = s[lo], b = s[hi];
                if (desc ? (a < b) : (b < a)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* x, int cols, long ld, float* y, long ldy) {
    __shared__ float sh[4];
    const float* p = x + (long)blockIdx.x * ld;
    float* q = y + (long)blockIdx.x * ldy;
    float ss = 0.f;
    for (int c = threadIdx.x; c < cols; c += 256) ss += p[c] * p[c];
    ss = block_sum<256>(ss, sh);
    const float sc = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
    for (int c = threadIdx.x; c < cols; c += 256) q[c] = p[c] * sc;
}

// One launch of the wide top-k.  FROM_X: workgroup (row, g) sorts columns [g*seg, g*seg + seg) of x; else it sorts lists
// [g*seg, g*seg + seg) of the row's in_lists k-key lists.  Its k best keys go to out_keys[row, g] or, when out_lists == 1, decoded to
// out_val / out_idx (the value re-read from x: bit for bit the input's).
template <bool FROM_X>
__global__ __launch_bounds__(256) void topk_wide_kernel(const float* __restrict__ x, long ld, int cols, const int32_t* __restrict__ exclude,
                                                        const uint64_t* __restrict__ in_keys, int in_lists, int k, int seg, int out_lists,
                                                        uint64_t* __restrict__ out_keys, float* __restrict__ out_val,
                                                        int32_t* __restrict__ out_idx) {
    __shared__ uint64_t s[TOPKW_CHUNK];
    const long row = blockIdx.x / out_lists;
    const int g = (int)(blockIdx.x - row * out_lists);
    int n;
    if (FROM_X) {
        const int c0 = g * seg;
        n = min(seg, cols - c0);
        const int ex = exclude ? exclude[row] : -1;
        const float* p = x + row * ld;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int c = c0 + i;
            s[i] = c == ex ? 0ull : topk_key(p[c], c);
        }
    } else {
        const int l0 = g * seg;
        n = min(seg, in_lists - l0) * k;
        const uint64_t* src = in_keys + ((long)row * in_lists + l0) * k;
        for (int i = threadIdx.x; i < n; i += 256) s[i] = src[i];
    }
    const int K2 = next_pow2(k), N = max(next_pow2(n), K2);
    for (int i = n + threadIdx.x; i < N; i += 256) s[i] = 0ull;
    __syncthreads();
    bitonic_topk_desc<256>(s, N, K2);
    for (int j = threadIdx.x; j < k; j += 256) {
        const uint64_t key = s[j];
        if (out_lists == 1 && out_val) {
            const int c = key ? (int)(0xffffffffu - (uint32_t)key) : -1;
            out_idx[row * k + j] = c;
            out_val[row * k + j] = c >= 0 ? x[row * ld + c] : -INFINITY;
        } else {
            out_keys[((long)row * out_lists + g) * k + j] = key;
        }
    }
}

// words of a token row: ids with <BOS>, <EOS> and PAD removed, in order (at most NG_MAX_WORDS kept)
__device__ __forceinline__ uint64_t ngram_key(const int* w, int i, int n) {
    uint64_t key = 0;
    for (int j = 0; j < n; ++j) key = (key << 16) | (uint64_t)(w[i + j] & 0xffff);
    return key;
}

// One wave (workgroup of 64) per caption.
__global__ __launch_bounds__(64) void ngram_vectors_kernel(const int32_t* __restrict__ tok, long ld, const int32_t* __restrict__ len, int bos,
                                                           int eos, const uint64_t* __restrict__ df_keys, const float* __restrict__ idf,
                                                           long n_df, float idf_unseen, const int32_t* __restrict__ off,
                                                           uint64_t* __restrict__ keys, float* __restrict__ w, int32_t* __restrict__ nnz,
                                                           float* __restrict__ norm, int32_t* __restrict__ words) {
    __shared__ int sw[NG_MAX_WORDS];
    __shared__ uint64_t sk[NG_SLOTS];
    __shared__ int scnt[64];
    const long r = blockIdx.x;
    const int lane = threadIdx.x;
    const int nt = (int)min(max((long)len[r], 0L), ld);
    const int32_t* row = tok + r * ld;
    int nw = 0;
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + lane;
        const int v = t < nt ? row[t] : 0;
        const bool word = t < nt && v != 0 && v != bos && v != eos;
        const unsigned long long m = __ballot(word);
        const int pos = nw + __popcll(m & ((1ull << lane) - 1ull));
        if (word && pos < NG_MAX_WORDS) sw[pos] = v;
        nw += __popcll(m);
    }
    nw = min(nw, NG_MAX_WORDS);
    __syncthreads();
#pragma unroll
    for (int n = 1; n <= 4; ++n) sk[(n - 1) * 64 + lane] = lane + n <= nw ? ngram_key(sw, lane, n) : ~0ull;
    __syncthreads();
    bitonic_sort<64, false>(sk, NG_SLOTS);
    // thread t owns slots 4t .. 4t+3: the first slot of each run of equal keys is a distinct n-gram, its run length the count
    int first[4], cnt[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s = 4 * lane + j;
        const uint64_t key = sk[s];
        first[j] = key != ~0ull && (s == 0 || sk[s - 1] != key);
        cnt[j] = 0;
        if (first[j]) {
            int e = s;
            while (e < NG_SLOTS && sk[e] == key) ++e;
            cnt[j] = e - s;
            ++mine;
        }
    }
    scnt[lane] = mine;
    __syncthreads();
    int pos = 0, total = 0;
    for (int i = 0; i < 64; ++i) {
        const int c = scnt[i];
        pos += i < lane ? c : 0;
        total += c;
    }
    const long base = off[r], cap = off[r + 1] - base;
    double ss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!first[j]) continue;
        const uint64_t key = sk[4 * lane + j];
        long lo = 0, hi = n_df;   // first df key >= key
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (df_keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        const float f = lo < n_df && df_keys[lo] == key ? idf[lo] : idf_unseen;
        const float wt = (float)cnt[j] * f;
        if (pos < cap) {
            keys[base + pos] = key;
            w[base + pos] = wt;
        }
        ++pos;
        const int n = key_order(key);
#pragma unroll
        for (int q = 0; q < 4; ++q) ss[q] += q == n - 1 ? (double)wt * (double)wt : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss[q] += __shfl_xor(ss[q], o, 64);
    }
    if (lane == 0) {
        nnz[r] = (int)min((long)total, cap);
        words[r] = nw;
#pragma unroll
        for (int q = 0; q < 4; ++q) norm[r * 4 + q] = (float)sqrt(ss[q]);
    }
}

// Workgroup (b, group of CS_CPB candidates of image b).  The pool (every caption of the k neighbours, neighbour order) and each
// candidate's sorted keys / weights are staged in LDS; thread j scores pool captions j, j + 256, ... against the group's candidates
// (cider_pair_scores: each reference key looked up by binary search in the candidate's keys), then each candidate's pool scores are
// sorted and the m' largest summed in float64.  LDS: 8 + 4 * 3 + 4 * 8 KiB + small = ~53 KiB (two workgroups per CU fit in 160 KiB).
__global__ __launch_bounds__(256) void consensus_score_kernel(int k, const int32_t* __restrict__ nbr, const int32_t* __restrict__ img_cap,
                                                              const int32_t* __restrict__ r_off, const int32_t* __restrict__ r_nnz,
                                                              const uint64_t* __restrict__ r_keys, const float* __restrict__ r_w,
                                                              const float* __restrict__ r_norm, const int32_t* __restrict__ r_len,
                                                              const int32_t* __restrict__ cand_img, int groups, const int32_t* __restrict__ c_off,
                                                              const int32_t* __restrict__ c_nnz, const uint64_t* __restrict__ c_keys,
                                                              const float* __restrict__ c_w, const float* __restrict__ c_norm,
                                                              const int32_t* __restrict__ c_len, int m, double* __restrict__ score) {
    __shared__ int s_pool[CS_MAX_POOL];
    __shared__ int s_cnt[CS_MAX_K];
    __shared__ uint64_t s_ck[CS_CPB][NG_SLOTS];
    __shared__ float s_cw[CS_CPB][NG_SLOTS];
    __shared__ float s_sc[CS_CPB][CS_MAX_POOL];
    __shared__ double s_red[4];
    const int b = blockIdx.x / groups;
    const int g = blockIdx.x - b * groups;
    const int t = threadIdx.x;
    const int c0 = cand_img[b] + g * CS_CPB;
    const int nc = min(CS_CPB, cand_img[b + 1] - c0);
    if (nc <= 0) return;
    // the pool: exclusive scan of the neighbours' caption counts (k <= 256: one per thread)
    const int* nb = nbr + (long)b * k;
    int cnt = 0, id = -1;
    if (t < k) {
        id = nb[t];
        cnt = id >= 0 ? img_cap[id + 1] - img_cap[id] : 0;
    }
    s_cnt[t] = cnt;
    __syncthreads();
    int p0 = 0, np = 0;
    for (int i = 0; i < k; ++i) {
        const int c = s_cnt[i];
        p0 += i < t ? c : 0;
        np += c;
    }
    np = min(np, CS_MAX_POOL);
    for (int i = 0; i < cnt && p0 + i < CS_MAX_POOL; ++i) s_pool[p0 + i] = img_cap[id] + i;
    CiderHyps<CS_CPB> hyp;
    cider_stage_hyps<CS_CPB>(c0, nc, c_off, c_nnz, c_keys, c_w, c_norm, c_len, s_ck, s_cw, hyp);
    __syncthreads();
    for (int j = t; j < np; j += 256) {
        float sc[CS_CPB];   // CIDEr-D of the group's candidates against pool caption j (cider_pair.h: the one definition)
        cider_pair_scores<CS_CPB>(s_pool[j], r_off, r_nnz, r_keys, r_w, r_norm, r_len, s_ck, s_cw, hyp, sc);
#pragma unroll
        for (int c = 0; c < CS_CPB; ++c) s_sc[c][j] = sc[c];
    }
    const int N = next_pow2(np);
    for (int i = np + t; i < N; i += 256)
#pragma unroll
        for (int c = 0; c < CS_CPB; ++c) s_sc[c][i] = -INFINITY;
    __syncthreads();
    // the CS_CPB score lists sorted as one bitonic network over CS_CPB * N slots (each list sorted on its own: pairs never cross lists)
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < CS_CPB * (N >> 1); i += 256) {
                const int c = i / (N >> 1), ii = i - c * (N >> 1);
                const int lo = 2 * ii - (ii & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const float a = s_sc[c][lo], v = s_sc[c][hi];
                if (desc ? (a < v) : (v < a)) { s_sc[c][lo] = v; s_sc[c][hi] = a; }
            }
            __syncthreads();
        }
    }
    const int mm = min(m, np);
    for (int c = 0; c < nc; ++c) {
        double acc = 0.0;
        for (int i = t; i < mm; i += 256) acc += (double)s_sc[c][i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if ((t & 63) == 0) s_red[t >> 6] = acc;
        __syncthreads();
        if (t == 0) score[c0 + c] = mm > 0 ? (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (double)mm : 0.0;
        __syncthreads();
    }
}

static inline long topkw_lists(int cols) { return (cols + TOPKW_CHUNK - 1) / TOPKW_CHUNK; }

}  // namespace vc

using namespace vc;

extern "C" int vc_l2_normalize_rows_f32(void* stream, const float* x, long rows, int cols, long ld, float* y, long ldy) {
    VC_CHECK_ARG(x && y && rows >= 0 && cols > 0 && ld >= cols && ldy >= cols, "bad argument");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, cols, ld, y, ldy);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vc_topk_rows_wide_workspace_bytes(long rows, int cols, int k) {
    if (rows <= 0 || cols <= 0 || k <= 0 || k > TOPKW_MAX_K) return 0;
    const long l1 = topkw_lists(cols);
    if (l1 <= 1) return 0;
    const long g = TOPKW_CHUNK / k, l2 = (l1 + g - 1) / g;
    return (size_t)rows * (size_t)(l1 + (l2 > 1 ? l2 : 0)) * (size_t)k * sizeof(uint64_t);
}

extern "C" int vc_topk_rows_wide_f32(void* stream, const float* x, long rows, int cols, long ld, int k, const int32_t* exclude,
                                     float* out_val, int32_t* out_idx, void* ws, size_t ws_bytes) {
    VC_CHECK_ARG(x && out_val && out_idx && rows >= 0 && cols > 0 && ld >= cols && k > 0 && k <= cols, "bad argument");
    VC_CHECK_ARG(k <= TOPKW_MAX_K, "k must be <= 256");
    if (rows == 0) return 0;
    const size_t need = vc_topk_rows_wide_workspace_bytes(rows, cols, k);
    VC_CHECK_ARG(need == 0 || (ws && ws_bytes >= need), "workspace too small (need vc_topk_rows_wide_workspace_bytes)");
    const long l1 = topkw_lists(cols);
    VC_CHECK_ARG(rows * l1 < (1L << 31), "too many rows x column chunks for one launch");
    hipStream_t st = (hipStream_t)stream;
    uint64_t* buf[2] = {(uint64_t*)ws, (uint64_t*)ws + (l1 > 1 ? rows * l1 * k : 0)};
    hipLaunchKernelGGL(topk_wide_kernel<true>, dim3((unsigned)(rows * l1)), dim3(256), 0, st, x, ld, cols, exclude, nullptr, 0, k,
                       TOPKW_CHUNK, (int)l1, l1 > 1 ? buf[0] : nullptr, l1 > 1 ? nullptr : out_val, out_idx);
    VC_LAUNCH_CHECK();
    const int g = TOPKW_CHUNK / k;
    long lists = l1;
    int cur = 0;
    while (lists > 1) {   // merge g lists per workgroup until one is left: 4096 columns -> 1, 4096 * g -> 2 launches, ...
        const long next = (lists + g - 1) / g;
        hipLaunchKernelGGL(topk_wide_kernel<false>, dim3((unsigned)(rows * next)), dim3(256), 0, st, x, ld, cols, nullptr, buf[cur],
                           (int)lists, k, g, (int)next, next > 1 ? buf[cur ^ 1] : nullptr, next > 1 ? nullptr : out_val, out_idx);
        VC_LAUNCH_CHECK();
        lists = next;
        cur ^= 1;
    }
    return 0;
}

extern "C" int vc_ngram_vectors(void* stream, const int32_t* tok, long n, long ld, const int32_t* len, int bos, int eos,
                                const uint64_t* df_keys, const float* idf, long n_df, float idf_unseen, const int32_t* off,
                                uint64_t* keys, float* w, int32_t* nnz, float* norm, int32_t* words) {
    VC_CHECK_ARG(tok && len && off && keys && w && nnz && norm && words && n >= 0 && ld > 0, "bad argument");
    VC_CHECK_ARG(n_df == 0 || (df_keys && idf && n_df > 0), "df table");
    if (n == 0) return 0;
    hipLaunchKernelGGL(ngram_vectors_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, tok, ld, len, bos, eos, df_keys, idf,
                       n_df, idf_unseen, off, keys, w, nnz, norm, words);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_consensus_score(void* stream, int B, int k, const int32_t* nbr, const int32_t* img_cap, const int32_t* r_off,
                                  const int32_t* r_nnz, const uint64_t* r_keys, const float* r_w, const float* r_norm, const int32_t* r_len,
                                  const int32_t* cand_img, int max_cands, const int32_t* c_off, const int32_t* c_nnz, const uint64_t* c_keys,
                                  const float* c_w, const float* c_norm, const int32_t* c_len, int m, double* score) {
    VC_CHECK_ARG(nbr && img_cap && r_off && r_nnz && r_keys && r_w && r_norm && r_len && cand_img && c_off && c_nnz && c_keys && c_w &&
                 c_norm && c_len && score, "null pointer");
    VC_CHECK_ARG(B >= 0 && k >= 1 && k <= CS_MAX_K && m >= 1 && max_cands >= 0 && max_cands <= 256, "k must be 1..256, m >= 1, <= 256 candidates");
    if (B == 0 || max_cands == 0) return 0;
    const int groups = (max_cands + CS_CPB - 1) / CS_CPB;
    hipLaunchKernelGGL(consensus_score_kernel, dim3((unsigned)(B * groups)), dim3(256), 0, (hipStream_t)stream, k, nbr, img_cap, r_off,
                       r_nnz, r_keys, r_w, r_norm, r_len, cand_img, groups, c_off, c_nnz, c_keys, c_w, c_norm, c_len, m, score);
    VC_LAUNCH_CHECK();
    return 0;
}
