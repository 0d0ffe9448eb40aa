// Diverse captioning on device: K latent draws per image, each decoded to a candidate caption, the candidates of an image
// merged by token sequence and ranked (generate.py: CaptionGenerator.diverse).  Candidate rows are image-major: row r = b*K + k.
//
//   vc_diverse_latent_f32    z[r, s, l] = pm[r / K, l] + std * eps[r, s, l]: no [rows*S, L] mean / std tensors; eps injected or drawn
//                            here with the Philox / Box-Muller code of vc_philox_normal_f32 (same seed, offset, step: same bits)
//   vc_decode_pick_f32       one decoder round's token per row from ONE read of the logits: argmax (first maximum) or the
//                            inverse-CDF draw, plus the token's log-softmax at temperature 1 accumulated into the row's candidate
//                            (sequence, length, float64 log-likelihood, <EOS> flag); the pieces and the entries they agree with bit
//                            for bit: row_ops.h
//   vc_decode_pick_trunc_f32 the same round with the distribution truncated before the draw: the top_k best words and / or the smallest
//                            set of best words holding a share top_p of the probability, found by a radix select (no sort of V words)
//   vc_decode_pick_typical_f32 the same round with cuts that follow the row's entropy or peak: locally typical sampling (the words whose
//                            surprisal is closest to the entropy, by the same radix select over another key), min-p and eta floors
//   vc_decode_round_end_i32  pending = rows without <EOS>, round += 1 (the device round counter keys the next round's uniforms)
//   vc_diverse_rank          one workgroup per image: scores, 64-bit hashes confirmed by full compares, duplicates merged, ranked
#include "row_ops.h"
#include "vaecap.h"

namespace vc {

constexpr int RANK_MAX_K = 256;

__global__ __launch_bounds__(256) void diverse_latent_kernel(long n, long SL, int L, int K, const float* __restrict__ pm, float std_,
                                                             const float* __restrict__ eps, uint64_t seed, uint64_t offset,
                                                             const int32_t* __restrict__ step, float* __restrict__ z) {
    const long nq = (n + 3) >> 2;
    const uint32_t k1 = (uint32_t)(seed >> 32) + (step ? (uint32_t)step[0] : 0u);
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        float f[4];
        if (eps) {
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = q * 4 + j < n ? eps[q * 4 + j] : 0.f;
        } else {   // = philox_kernel mode 1 on element quad q
            uint32_t r[4];
            philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, k1, r);
            box_muller4(r, f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = q * 4 + j;
            if (i < n) {
                const float m = pm ? pm[(i / SL / K) * L + i % L] : 0.f;
                z[i] = m + std_ * f[j];   // (the expression of sample_kernel)
            }
        }
    }
}

// One workgroup per row.  STAGE: the row is copied to LDS with coalesced loads and every later pass reads it there.
template <bool STAGE>
__global__ __launch_bounds__(256) void decode_pick_kernel(const float* __restrict__ logits, long rows, int V, long ld, float inv_temp,
                                                          const float* __restrict__ u, int u_rounds, const int32_t* __restrict__ round,
                                                          int eos, int32_t* __restrict__ tok, int32_t* __restrict__ done,
                                                          int32_t* __restrict__ seq, int Lmax, int32_t* __restrict__ len,
                                                          double* __restrict__ logprob) {
    extern __shared__ float srow[];
    __shared__ float sh[4];
    __shared__ float part[256];
    __shared__ int si[256];
    __shared__ int s_tok;
    const long r = blockIdx.x;
    const int t = threadIdx.x;
    const float* p = stage_row<STAGE>(logits + r * ld, V, srow);
    int c0, c1;
    const int per = row_chunk(V, c0, c1);
    float mx1, s1, bv;
    int bi;
    row_max_sum(p, c0, c1, sh, mx1, s1, bv, bi);
    if (u == nullptr) {   // argmax: the first maximum (chunks are in index order)
        block_first_max(bv, bi, part, si);
        if (t == 0) s_tok = si[0];
    } else {              // the inverse-CDF draw (the scaled maximum over the chunks: the row may sit in LDS)
        float mx = -INFINITY;
        for (int c = c0; c < c1; ++c) mx = fmaxf(mx, p[c] * inv_temp);
        mx = block_max<256>(mx, sh);
        row_cdf_part(p, c0, c1, inv_temp, mx, part);
        if (t == 0) {
            const int rd = round ? min(max(round[0], 0), u_rounds - 1) : 0;
            s_tok = row_cdf_pick(p, V, per, inv_temp, mx, part, u + ((long)rd * rows + r));
        }
    }
    if (t == 0) {
        const int w = s_tok;
        tok[r] = w;
        const int n = len[r];
        if (!done[r] && n >= 0 && n < Lmax) {
            const float lp = lsm_term(p[min(max(w, 0), V - 1)], mx1, logf(s1));
            seq[r * Lmax + n] = w;
            len[r] = n + 1;
            logprob[r] += (double)lp;
            if (w == eos) done[r] = 1;
        }
    }
}

// ---- truncated pick (top-k / nucleus).  Order: descending y = fl32(x * inv_temp), equal y by lower index.  Everything the selection
// decides on is an integer: the order-preserving 32-bit image of y (the key) and the word's mass exp(y - max y) rounded to a multiple of
// 2^-32 (sums of integers are exact: no result depends on the order in which LDS atomics or partial sums arrive).
__device__ __forceinline__ uint32_t pick_key(float x, float inv_temp) {
    uint32_t b = __float_as_uint(__fmul_rn(x, inv_temp));
    if ((b << 1) == 0u) b = 0u;   // -0 == +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ unsigned long long key_mass(uint32_t k, float my) {
    return __float2ull_rn(__expf(key_value(k) - my) * 4294967296.0f);   // <= 2^32 per word: 2^31 words stay below 2^63
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int o) {
    const uint32_t lo = __shfl_up((uint32_t)v, o, 64), hi = __shfl_up((uint32_t)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
// inclusive prefix sum over the 256 threads (thread order); total in every thread
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long* ws /* 4 */, unsigned long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long n = shfl_up_u64(v, o);
        if (lane >= o) v += n;
    }
    __syncthreads();
    if (lane == 63) ws[w] = v;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < w) base += ws[i];
        tot += ws[i];
    }
    total = tot;
    return v + base;
}

constexpr int PICK_HIST_COPIES = 4;   // a bin's copies sit side by side (other LDS banks): lanes t, t + 4, ... share one, not all 64
struct PickSel {
    unsigned long long hist[256 * PICK_HIST_COPIES];
    unsigned long long ws[4];
    unsigned long long above;
    int bin, found;
};

// The key of word c that radix_select orders by, and the mass of a word with that key.  LogitKey: the truncation's order, descending y.
struct LogitKey {
    const float* p;
    float inv_temp, my;
    __device__ __forceinline__ uint32_t key(int c) const { return pick_key(p[c], inv_temp); }
    __device__ __forceinline__ unsigned long long mass(int, uint32_t k) const { return key_mass(k, my); }
};

// MSB-first radix select, 8 bits per pass, over the words with key > lo: the key T at which the running quantity (MASS: the words' masses,
// else their number), summed from the best word down, first reaches thr; above = the quantity of the keys > T.  false: the eligible
// words together stay below thr.  Each pass: a 256-bin histogram of the words that share the prefix found so far, scanned from the top.
template <bool MASS, class KeyF>
__device__ bool radix_select(const KeyF& key, int V, long long lo, double thr, PickSel& S, uint32_t& T, unsigned long long& above) {
    const int t = threadIdx.x;
    uint32_t prefix = 0;
    unsigned long long ab = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
#pragma unroll
        for (int i = 0; i < PICK_HIST_COPIES; ++i) S.hist[t + 256 * i] = 0;
        if (t == 0) { S.found = 0; S.bin = 0; S.above = ab; }
        __syncthreads();
        for (int c = t; c < V; c += 256) {
            const uint32_t k = key.key(c);
            const bool in = pass == 0 || (k >> (shift + 8)) == prefix;
            if ((long long)k > lo && in) atomicAdd(&S.hist[((k >> shift) & 255u) * PICK_HIST_COPIES + (t & (PICK_HIST_COPIES - 1))], MASS ? key.mass(c, k) : 1ull);
        }
        __syncthreads();
        unsigned long long v = 0;   // thread t holds the t-th bin from the top
#pragma unroll
        for (int i = 0; i < PICK_HIST_COPIES; ++i) v += S.hist[(255 - t) * PICK_HIST_COPIES + i];
        unsigned long long tot;
        const unsigned long long incl = block_scan_u64(v, S.ws, tot);
        if ((double)(ab + incl) >= thr && !((double)(ab + incl - v) >= thr)) { S.bin = 255 - t; S.above = ab + incl - v; S.found = 1; }
        __syncthreads();
        const bool found = S.found != 0;
        prefix = (prefix << 8) | (uint32_t)S.bin;
        ab = S.above;
        __syncthreads();
        if (!found && pass == 0) return false;
    }
    T = prefix;
    above = ab;
    return true;
}

// how many of the equal words of mass m at the cut are needed for above + j * m >= thr (1 <= j <= cap)
__device__ __forceinline__ long tie_count(double thr, unsigned long long above, unsigned long long m, long cap) {
    long j = m ? (long)ceil((thr - (double)above) / (double)m) : 1;
    j = max(1l, min(j, cap));
    while (j > 1 && (double)(above + (unsigned long long)(j - 1) * m) >= thr) --j;
    while (j < cap && (double)(above + (unsigned long long)j * m) < thr) ++j;
    return j;
}

// One workgroup per row, the row staged in LDS (STAGE) or re-read.  top_k in (0, V) and / or top_p < 1 (the entry dispatches the rest).
template <bool STAGE>
__global__ __launch_bounds__(256) void decode_pick_trunc_kernel(const float* __restrict__ logits, long rows, int V, long ld, float inv_temp,
                                                                int top_k, float top_p, const float* __restrict__ u, int u_rounds,
                                                                const int32_t* __restrict__ round, int eos, int32_t* __restrict__ tok,
                                                                int32_t* __restrict__ done, int32_t* __restrict__ seq, int Lmax,
                                                                int32_t* __restrict__ len, double* __restrict__ logprob,
                                                                int32_t* __restrict__ kept) {
    extern __shared__ float srow[];
    __shared__ PickSel S;
    __shared__ float sh[4];
    __shared__ int s_tok, s_last;
    const long r = blockIdx.x;
    const int t = threadIdx.x;
    const float* p = stage_row<STAGE>(logits + r * ld, V, srow);
    if (t == 0) { s_tok = -1; s_last = 0; }
    int c0, c1;
    row_chunk(V, c0, c1);
    float bv = -INFINITY;
    for (int c = t; c < V; c += 256) bv = fmaxf(bv, p[c]);   // (strided: the same maximum as row_max_sum's)
    const float mx1 = block_max<256>(bv, sh);
    const float s1 = row_exp_sum(p, c0, c1, mx1, sh);
    const float my = key_value(pick_key(mx1, inv_temp));   // max y (the scaling is monotone)

    // ---- the cut: words with key > T are kept, and the first j (index order) of the words with key == T
    uint32_t T = 0;
    long j = 1, jcap = V;
    long long lo = -1;
    unsigned long long ab;
    const bool by_k = top_k > 0 && top_k < V;
    if (by_k) {
        radix_select<false>(LogitKey{p, inv_temp, my}, V, -1, (double)top_k, S, T, ab);
        j = jcap = (long)top_k - (long)ab;
        lo = (long long)T;
    }
    if (top_p < 1.0f) {
        unsigned long long z = 0, zk;
        for (int c = t; c < V; c += 256) {
            const uint32_t k = pick_key(p[c], inv_temp);
            if ((long long)k > lo) z += key_mass(k, my);
        }
        block_scan_u64(z, S.ws, zk);   // mass of the keys > lo
        __syncthreads();
        const unsigned long long above_k = zk, mk = by_k ? key_mass(T, my) : 0ull;
        zk += (unsigned long long)j * mk * (by_k ? 1ull : 0ull);
        const double thr = (double)top_p * (double)zk;
        uint32_t Tp;
        if (radix_select<true>(LogitKey{p, inv_temp, my}, V, lo, thr, S, Tp, ab)) {
            T = Tp;
            jcap = V;
            j = tie_count(thr, ab, key_mass(T, my), V);
        } else {   // the cut falls among the top-k set's last equal words
            j = tie_count(thr, above_k, mk, jcap);
        }
    }
    // ---- kept words per chunk: their number, the rank of the chunk's first word of key T among the equal words, their mass
    const unsigned long long mT = key_mass(T, my);
    unsigned long long cnt = 0, mass_gt = 0;   // cnt: (words with key > T) << 32 | words with key == T
    for (int c = c0; c < c1; ++c) {
        const uint32_t k = pick_key(p[c], inv_temp);
        if (k > T) { cnt += 1ull << 32; mass_gt += key_mass(k, my); }
        else if (k == T) cnt += 1ull;
    }
    unsigned long long cnt_all, z_kept;
    const unsigned long long cnt_incl = block_scan_u64(cnt, S.ws, cnt_all);
    __syncthreads();
    const long n_eq = (long)(cnt_all & 0xffffffffull), n_gt = (long)(cnt_all >> 32);
    j = max(1l, min(min(j, jcap), n_eq));
    const long eq0 = (long)((cnt_incl - cnt) & 0xffffffffull);   // equal words before this chunk
    const long my_eq = max(0l, min((long)(cnt & 0xffffffffull), j - eq0));   // equal words of this chunk that are kept
    const unsigned long long part = mass_gt + (unsigned long long)my_eq * mT;
    const unsigned long long run_incl = block_scan_u64(part, S.ws, z_kept);
    const int rd = round ? min(max(round[0], 0), u_rounds - 1) : 0;
    const double target = (double)u[(long)rd * rows + r] * (double)z_kept;
    if ((double)run_incl > target && !((double)(run_incl - part) > target)) {   // inverse CDF over the kept words in index order
        unsigned long long run = run_incl - part;
        long e = eq0;
        int idx = -1;
        for (int c = c0; c < c1; ++c) {
            const uint32_t k = pick_key(p[c], inv_temp);
            if (k > T || (k == T && e++ < j)) {
                run += key_mass(k, my);
                idx = c;
                if ((double)run > target) break;
            }
        }
        s_tok = idx;
    }
    __syncthreads();
    if (s_tok < 0) {   // no running mass exceeds the target (u >= 1): the last kept word
        long e = eq0;
        int last = -1;
        for (int c = c0; c < c1; ++c) {
            const uint32_t k = pick_key(p[c], inv_temp);
            if (k > T || (k == T && e++ < j)) last = c;
        }
        if (last >= 0) atomicMax(&s_last, last);
        __syncthreads();
    }
    if (t == 0) {
        const int w = min(max(s_tok >= 0 ? s_tok : s_last, 0), V - 1);
        tok[r] = w;
        if (kept) kept[r] = (int32_t)(n_gt + j);
        const int n = len[r];
        if (!done[r] && n >= 0 && n < Lmax) {
            const float lp = lsm_term(p[w], mx1, logf(s1));   // over the full vocabulary
            seq[r * Lmax + n] = w;
            len[r] = n + 1;
            logprob[r] += (double)lp;
            if (w == eos) done[r] = 1;
        }
    }
}

// ---- typical / min-p / eta pick.  Cuts that follow the row's entropy H or its peak, all taken on the FULL distribution p = softmax(y):
//   typical_p tau: order by d = |-log p - H| ascending, equal d by lower index; the shortest prefix whose mass is >= tau
//   min_p, eta:    p >= max(min_p * p_max, min(eta, sqrt(eta) * exp(-H)))
// and the kept set is their intersection (empty: the first maximum of y).  With g = max y - y >= 0, the integer masses m (key_mass) and
// their exact sums Z = sum m, E = sum round(m * g):  A = E / Z,  -log p - H = g - A (log Z cancels),  H = log(Z 2^-32) + A,  and a floor
// f on p is the threshold g <= -log f - log(Z 2^-32) (min_p alone: g <= -log min_p, so min_p = 1 keeps exactly the maxima of y).
// A word of zero mass (a banned word's -FLT_MAX scaled to -inf has g = +inf) adds nothing to E and is never kept.  A and the threshold
// are formed in float64 from the integer sums and rounded once to f32; d = |g - A| is one f32 subtraction (monotone in g, equal for
// equal y), far inside the margin the reference leaves around a cut.
// The select needs a word's mass only where its key falls into the prefix found so far, so the mass (an exponential and a 64-bit
// conversion) is formed on demand.  A word of zero mass needs no key of its own: it adds 0 to every histogram bin and to every running
// mass, so no cut can fall on it, and the kept test asks for m != 0.
struct TypWord {
    uint32_t yk;   // pick_key of the word
    uint32_t dk;   // order-preserving image of -d: ~bits(d), d = |g - A| >= 0 in f32 (the radix select runs from the largest key down)
    float g;
};
struct TypKey {
    const float* p;
    float inv_temp, my, A;
    __device__ __forceinline__ TypWord word(int c) const {
        TypWord w;
        w.yk = pick_key(p[c], inv_temp);
        w.g = my - key_value(w.yk);
        w.dk = ~__float_as_uint(fabsf(w.g - A));   // (g = +inf: d = +inf, the smallest key)
        return w;
    }
    __device__ __forceinline__ uint32_t key(int c) const { return word(c).dk; }
    __device__ __forceinline__ unsigned long long mass(int c, uint32_t) const { return key_mass(pick_key(p[c], inv_temp), my); }
};

// One workgroup per row, the row staged in LDS (STAGE) or re-read.  At least one cut is on (the entry dispatches the rest).
template <bool STAGE>
__global__ __launch_bounds__(256) void decode_pick_typical_kernel(const float* __restrict__ logits, long rows, int V, long ld, float inv_temp,
                                                                  float typical_p, float min_p, float eta, const float* __restrict__ u,
                                                                  int u_rounds, const int32_t* __restrict__ round, int eos,
                                                                  int32_t* __restrict__ tok, int32_t* __restrict__ done,
                                                                  int32_t* __restrict__ seq, int Lmax, int32_t* __restrict__ len,
                                                                  double* __restrict__ logprob, int32_t* __restrict__ kept,
                                                                  float* __restrict__ entropy) {
    extern __shared__ float srow[];
    __shared__ PickSel S;
    __shared__ float sh[4];
    __shared__ int s_tok, s_last, s_first, s_j;
    const long r = blockIdx.x;
    const int t = threadIdx.x;
    const float* p = stage_row<STAGE>(logits + r * ld, V, srow);
    if (t == 0) { s_tok = -1; s_last = 0; s_first = 0x7fffffff; s_j = 0; }
    int c0, c1;
    row_chunk(V, c0, c1);
    float bv = -INFINITY;
    for (int c = t; c < V; c += 256) bv = fmaxf(bv, p[c]);
    const float mx1 = block_max<256>(bv, sh);
    const float s1 = row_exp_sum(p, c0, c1, mx1, sh);
    const uint32_t kmy = pick_key(mx1, inv_temp);
    const float my = key_value(kmy);

    // ---- the row's statistics: Z, E (exact integer sums) and the first maximum of y
    unsigned long long z = 0, e = 0, Z, E;
    int first = 0x7fffffff;
    for (int c = t; c < V; c += 256) {
        const uint32_t k = pick_key(p[c], inv_temp);
        if (k == kmy) first = min(first, c);
        const unsigned long long m = key_mass(k, my);
        if (m) {   // (zero mass: g may be +inf, and 0 * inf would poison the sum)
            z += m;
            // round(m * g) as the mantissa of m * g + 2^52: m <= 2^32 and g < 24 where m > 0, so the product stays below 2^37
            e += (unsigned long long)__double_as_longlong((double)m * (double)(my - key_value(k)) + 4503599627370496.0) & 0xfffffffffffffull;
        }
    }
    if (first != 0x7fffffff) atomicMin(&s_first, first);
    block_scan_u64(z, S.ws, Z);
    block_scan_u64(e, S.ws, E);
    const double Zd = (double)Z, A = (double)E / Zd, lz = log(Zd * (1.0 / 4294967296.0)), H = lz + A;
    double gm = INFINITY;   // the floors as one threshold on g
    if (min_p > 0.f) gm = -log((double)min_p);
    if (eta > 0.f) gm = fmin(gm, -log(fmin((double)eta, sqrt((double)eta) * exp(-H))) - lz);
    const float gmax = (float)gm;   // (min_p = 1: -0, and g <= -0 holds for g = 0 alone)

    // ---- the typical cut: words with dk > Td, and the first j (index order) of the words with dk == Td
    const bool typ = typical_p < 1.0f;
    const TypKey key{p, inv_temp, my, (float)A};
    uint32_t Td = 0;
    long j = 0, eq0 = 0;
    if (typ) {
        const double thr = (double)typical_p * Zd;
        unsigned long long ab;
        if (!radix_select<true>(key, V, -1, thr, S, Td, ab)) { Td = 0xffffffffu; ab = 0; }   // (a row without a finite maximum: nothing is kept)
        unsigned long long eqm = 0, eqc = 0, tot;
        for (int c = c0; c < c1; ++c) {
            const TypWord w = key.word(c);
            if (w.dk == Td) { eqm += key_mass(w.yk, my); ++eqc; }
        }
        const unsigned long long incl = ab + block_scan_u64(eqm, S.ws, tot);
        eq0 = (long)(block_scan_u64(eqc, S.ws, tot) - eqc);   // equal words before this chunk
        if ((double)incl >= thr && !((double)(incl - eqm) >= thr)) {   // the chunk in which the running mass reaches tau * Z
            unsigned long long run = incl - eqm;
            long n = eq0;
            for (int c = c0; c < c1; ++c) {
                const TypWord w = key.word(c);
                if (w.dk != Td) continue;
                run += key_mass(w.yk, my);
                ++n;
                if ((double)run >= thr) break;
            }
            s_j = (int)n;
        }
        __syncthreads();
        j = s_j;
    }
    // eq: the number of words with dk == Td met so far, in index order
    auto is_kept = [&](const TypWord& w, long& eq, unsigned long long& m) {
        const bool in = !typ || w.dk > Td || (w.dk == Td && eq++ < j);
        if (!(in && w.g <= gmax)) return false;
        m = key_mass(w.yk, my);
        return m != 0;
    };
    // ---- kept words per chunk: their number and mass; the draw
    unsigned long long part = 0, cnt = 0, z_kept, n_kept, m;
    long eq = eq0;
    for (int c = c0; c < c1; ++c)
        if (is_kept(key.word(c), eq, m)) { part += m; ++cnt; }
    const unsigned long long run_incl = block_scan_u64(part, S.ws, z_kept);
    block_scan_u64(cnt, S.ws, n_kept);
    const int rd = round ? min(max(round[0], 0), u_rounds - 1) : 0;
    const double target = (double)u[(long)rd * rows + r] * (double)z_kept;
    if (n_kept && (double)run_incl > target && !((double)(run_incl - part) > target)) {   // inverse CDF over the kept words in index order
        unsigned long long run = run_incl - part;
        int idx = -1;
        eq = eq0;
        for (int c = c0; c < c1; ++c) {
            if (is_kept(key.word(c), eq, m)) {
                run += m;
                idx = c;
                if ((double)run > target) break;
            }
        }
        s_tok = idx;
    }
    __syncthreads();
    if (n_kept && s_tok < 0) {   // no running mass exceeds the target (u >= 1): the last kept word
        int last = -1;
        eq = eq0;
        for (int c = c0; c < c1; ++c)
            if (is_kept(key.word(c), eq, m)) last = c;
        if (last >= 0) atomicMax(&s_last, last);
        __syncthreads();
    }
    if (t == 0) {
        const int w = min(max(!n_kept ? s_first : s_tok >= 0 ? s_tok : s_last, 0), V - 1);   // an empty intersection: the first maximum of y
        tok[r] = w;
        if (kept) kept[r] = n_kept ? (int32_t)n_kept : 1;
        if (entropy) entropy[r] = (float)H;
        const int n = len[r];
        if (!done[r] && n >= 0 && n < Lmax) {
            const float lp = lsm_term(p[w], mx1, logf(s1));   // over the full vocabulary
            seq[r * Lmax + n] = w;
            len[r] = n + 1;
            logprob[r] += (double)lp;
            if (w == eos) done[r] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void fill_kept_kernel(int32_t* __restrict__ kept, long rows, int v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) kept[i] = v;
}

__global__ __launch_bounds__(256) void round_end_kernel(const int32_t* __restrict__ done, long rows, float* __restrict__ pending,
                                                        int32_t* __restrict__ round) {
    __shared__ float sh[4];
    float open = 0.f;
    for (long i = threadIdx.x; i < rows; i += 256) open += done[i] ? 0.f : 1.f;
    open = block_sum<256>(open, sh);
    if (threadIdx.x == 0) {
        pending[0] = open;
        if (round) round[0] += 1;
    }
}

// One workgroup per image, thread k = draw k.  O(K^2) LDS work per image with K <= 256: each draw finds the draws with its sequence
// (hash + length filter, full compare to confirm), is its group's representative iff no other member scores better (ties: lower draw),
// and the representatives' ranks are counts of the representatives that precede them.
__global__ __launch_bounds__(256) void diverse_rank_kernel(int K, int Lmax, const int32_t* __restrict__ seq, const int32_t* __restrict__ len,
                                                           const int32_t* __restrict__ ended, const double* __restrict__ logprob,
                                                           double len_norm_f, int32_t* __restrict__ n_distinct, int32_t* __restrict__ rep,
                                                           int32_t* __restrict__ count, double* __restrict__ score) {
    __shared__ unsigned long long s_hash[RANK_MAX_K];
    __shared__ double s_score[RANK_MAX_K];
    __shared__ int s_len[RANK_MAX_K], s_end[RANK_MAX_K], s_lead[RANK_MAX_K];
    __shared__ float sh[4];
    const int k = threadIdx.x;
    const long base = (long)blockIdx.x * K;
    const int32_t* rowk = seq + (base + k) * Lmax;
    int n = 0, e = 0;
    double sc = 0.0;
    if (k < K) {
        n = min(max(len[base + k], 0), Lmax);
        e = ended[base + k] != 0;
        sc = logprob[base + k] / pow(1.0 + (double)n, len_norm_f);
        unsigned long long h = 1469598103934665603ull ^ (unsigned long long)n;   // FNV-1a over the tokens
        for (int i = 0; i < n; ++i) h = (h ^ (uint32_t)rowk[i]) * 1099511628211ull;
        s_hash[k] = h;
        s_score[k] = sc;
        s_len[k] = n;
        s_end[k] = e;
    }
    __syncthreads();
    int lead = 0, cnt = 0;
    if (k < K) {
        lead = 1;
        const unsigned long long h = s_hash[k];
        for (int j = 0; j < K; ++j) {
            if (s_hash[j] != h || s_len[j] != n) continue;
            bool same = true;
            if (j != k) {
                const int32_t* rowj = seq + (base + j) * Lmax;
                for (int i = 0; i < n && same; ++i) same = rowj[i] == rowk[i];
            }
            if (!same) continue;
            ++cnt;
            if (j != k && better(s_score[j], j, sc, k)) lead = 0;
        }
    }
    s_lead[k] = lead;
    __syncthreads();
    const int nd = (int)block_sum<256>(lead ? 1.f : 0.f, sh);
    if (lead) {
        int pos = 0;
        for (int j = 0; j < K; ++j)
            if (s_lead[j] && j != k && (s_end[j] > e || (s_end[j] == e && better(s_score[j], j, sc, k)))) ++pos;
        rep[base + pos] = k;
        count[base + pos] = cnt;
        score[base + pos] = sc;
    }
    __syncthreads();
    if (k < K && k >= nd) {
        rep[base + k] = -1;
        count[base + k] = 0;
        score[base + k] = 0.0;
    }
    if (k == 0) n_distinct[blockIdx.x] = nd;
}

}  // namespace vc

using namespace vc;

extern "C" int vc_diverse_latent_f32(void* stream, long rows, int K, int S, int L, const float* pm, float std_, const float* eps,
                                     uint64_t seed, uint64_t offset, const int32_t* step, float* z) {
    VC_CHECK_ARG(z && rows > 0 && K > 0 && S > 0 && L > 0, "bad argument");
    VC_CHECK_ARG(rows % K == 0, "rows must be images * K");
    const long SL = (long)S * L, n = rows * SL;
    const long nq = (n + 3) >> 2;
    const int grid = (int)(nq / 256 + 1 < 4096 ? nq / 256 + 1 : 4096);
    hipLaunchKernelGGL(diverse_latent_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, SL, L, K, pm, std_, eps, seed, offset, step, z);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_decode_pick_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature, const float* u,
                                  int u_rounds, const int32_t* round, int eos, int32_t* tok, int32_t* done, int32_t* seq, int Lmax,
                                  int32_t* len, double* logprob) {
    VC_CHECK_ARG(logits && tok && done && seq && len && logprob, "null pointer");
    VC_CHECK_ARG(rows > 0 && V > 0 && ld >= V && Lmax > 0, "bad shape");
    VC_CHECK_ARG(!u || (temperature > 0.f && u_rounds > 0), "sampling needs temperature > 0 and u_rounds > 0");
    const float inv_temp = u ? 1.0f / temperature : 1.0f;
    if (V <= ROW_LDS_MAX)
        hipLaunchKernelGGL(decode_pick_kernel<true>, dim3((unsigned)rows), dim3(256), (size_t)V * sizeof(float), (hipStream_t)stream, logits,
                           rows, V, ld, inv_temp, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob);
    else
        hipLaunchKernelGGL(decode_pick_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, rows, V, ld,
                           inv_temp, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_decode_pick_trunc_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature, int top_k,
                                        float top_p, const float* u, int u_rounds, const int32_t* round, int eos, int32_t* tok,
                                        int32_t* done, int32_t* seq, int Lmax, int32_t* len, double* logprob, int32_t* kept) {
    VC_CHECK_ARG(logits && tok && done && seq && len && logprob, "null pointer");
    VC_CHECK_ARG(rows > 0 && V > 0 && ld >= V && Lmax > 0, "bad shape");
    VC_CHECK_ARG(u && u_rounds > 0, "truncated sampling needs uniforms (u, u_rounds > 0): without a draw it is the argmax");
    VC_CHECK_ARG(temperature > 0.f && temperature < INFINITY, "temperature must be finite and > 0");
    VC_CHECK_ARG(top_k >= 0, "top_k must be >= 0 (0 = off)");
    VC_CHECK_ARG(top_p > 0.f && top_p <= 1.0f, "top_p must be in (0, 1] (1 = off)");
    const hipStream_t st = (hipStream_t)stream;
    if ((top_k == 0 || top_k >= V) && top_p == 1.0f) {   // nothing to cut: the plain draw, bit for bit
        const int rc = vc_decode_pick_f32(stream, logits, rows, V, ld, temperature, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob);
        if (rc) return rc;
        if (kept) hipLaunchKernelGGL(fill_kept_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, kept, rows, V);
        VC_LAUNCH_CHECK();
        return 0;
    }
    const float inv_temp = 1.0f / temperature;
    if (V <= ROW_LDS_MAX)
        hipLaunchKernelGGL(decode_pick_trunc_kernel<true>, dim3((unsigned)rows), dim3(256), (size_t)V * sizeof(float), st, logits, rows, V, ld,
                           inv_temp, top_k, top_p, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob, kept);
    else
        hipLaunchKernelGGL(decode_pick_trunc_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, logits, rows, V, ld, inv_temp, top_k,
                           top_p, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob, kept);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_decode_pick_typical_f32(void* stream, const float* logits, long rows, int V, long ld, float temperature, float typical_p,
                                          float min_p, float eta, const float* u, int u_rounds, const int32_t* round, int eos, int32_t* tok,
                                          int32_t* done, int32_t* seq, int Lmax, int32_t* len, double* logprob, int32_t* kept,
                                          float* entropy) {
    VC_CHECK_ARG(logits && tok && done && seq && len && logprob, "null pointer");
    VC_CHECK_ARG(rows > 0 && V > 0 && ld >= V && Lmax > 0, "bad shape");
    VC_CHECK_ARG(u && u_rounds > 0, "typical / min-p / eta sampling needs uniforms (u, u_rounds > 0): without a draw it is the argmax");
    VC_CHECK_ARG(temperature > 0.f && temperature < INFINITY, "temperature must be finite and > 0");
    VC_CHECK_ARG(typical_p > 0.f && typical_p <= 1.0f, "typical_p must be in (0, 1] (1 = off)");
    VC_CHECK_ARG(min_p >= 0.f && min_p <= 1.0f, "min_p must be in [0, 1] (0 = off)");
    VC_CHECK_ARG(eta >= 0.f && eta < 1.0f, "eta must be in [0, 1) (0 = off)");
    const hipStream_t st = (hipStream_t)stream;
    if (typical_p == 1.0f && min_p == 0.f && eta == 0.f) {   // nothing to cut: the plain draw, bit for bit (entropy is left untouched)
        const int rc = vc_decode_pick_f32(stream, logits, rows, V, ld, temperature, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob);
        if (rc) return rc;
        if (kept) hipLaunchKernelGGL(fill_kept_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, kept, rows, V);
        VC_LAUNCH_CHECK();
        return 0;
    }
    const float inv_temp = 1.0f / temperature;
    if (V <= ROW_LDS_MAX)
        hipLaunchKernelGGL(decode_pick_typical_kernel<true>, dim3((unsigned)rows), dim3(256), (size_t)V * sizeof(float), st, logits, rows, V, ld,
                           inv_temp, typical_p, min_p, eta, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob, kept, entropy);
    else
        hipLaunchKernelGGL(decode_pick_typical_kernel<false>, dim3((unsigned)rows), dim3(256), 0, st, logits, rows, V, ld, inv_temp, typical_p,
                           min_p, eta, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob, kept, entropy);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_decode_round_end_i32(void* stream, const int32_t* done, long rows, float* pending, int32_t* round) {
    VC_CHECK_ARG(done && pending && rows > 0, "bad argument");
    hipLaunchKernelGGL(round_end_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, done, rows, pending, round);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_diverse_rank(void* stream, long rows, int B, int K, int Lmax, const int32_t* seq, const int32_t* len, const int32_t* ended,
                               const double* logprob, double len_norm_f, int32_t* n_distinct, int32_t* rep, int32_t* count, double* score) {
    VC_CHECK_ARG(seq && len && ended && logprob && n_distinct && rep && count && score, "null pointer");
    VC_CHECK_ARG(B > 0 && K > 0 && K <= RANK_MAX_K && Lmax > 0, "K must be 1..256");
    VC_CHECK_ARG(rows == (long)B * K, "rows must be B * K");
    hipLaunchKernelGGL(diverse_rank_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, K, Lmax, seq, len, ended, logprob, len_norm_f,
                       n_distinct, rep, count, score);
    VC_LAUNCH_CHECK();
    return 0;
}
