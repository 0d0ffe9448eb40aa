// Diverse captioning on device: K latent draws per image, each decoded to a candidate caption, the candidates of an image
// merged by token sequence and ranked (generate.py: CaptionGenerator.diverse).  Candidate rows are image-major: row r = b*K + k.
//
//   vc_diverse_latent_f32    z[r, s, l] = pm[r / K, l] + std * eps[r, s, l]: no [rows*S, L] mean / std tensors; eps injected or drawn
//                            here with the Philox / Box-Muller code of vc_philox_normal_f32 (same seed, offset, step: same bits)
//   vc_decode_pick_f32       one decoder round's token per row from ONE read of the logits: argmax (first maximum, as
//                            argmax_rows_kernel) or the inverse-CDF draw with multinomial_rows_kernel's 256-chunk partition (same
//                            expressions, same order: same token), plus the token's log-softmax at temperature 1 accumulated into the
//                            row's candidate (sequence, length, float64 log-likelihood, <EOS> flag)
//   vc_decode_round_end_i32  pending = rows without <EOS>, round += 1 (the device round counter keys the next round's uniforms)
//   vc_diverse_rank          one workgroup per image: scores, 64-bit hashes confirmed by full compares, duplicates merged, ranked
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int PICK_LDS_MAX = 12288;   // logits rows up to this width are staged in LDS (48 KiB): the row is read from memory once
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
    const float* p = logits + r * ld;
    if (STAGE) {
        for (int c = t; c < V; c += 256) srow[c] = p[c];
        __syncthreads();
        p = srow;
    }
    // contiguous chunk per thread (multinomial_rows_kernel's partition: the scan order is the index order)
    const int per = (V + 255) / 256;
    const int c0 = t * per, c1 = min(V, c0 + per);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = c0; c < c1; ++c) {
        const float v = p[c];
        if (v > bv) { bv = v; bi = c; }
    }
    const float mx1 = block_max<256>(bv, sh);
    float s1 = 0.f;
    for (int c = c0; c < c1; ++c) s1 += __expf(p[c] - mx1);
    s1 = block_sum<256>(s1, sh);
    if (u == nullptr) {   // argmax: the first maximum (chunks are in index order, so (value, lower index) picks argmax_rows_kernel's)
        part[t] = bv;
        si[t] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) {
                const float v2 = part[t + o];
                const int i2 = si[t + o];
                if (v2 > part[t] || (v2 == part[t] && i2 < si[t])) {
                    part[t] = v2;
                    si[t] = i2;
                }
            }
            __syncthreads();
        }
        if (t == 0) s_tok = si[0];
    } else {              // multinomial_rows_kernel, expression for expression
        float mx = -INFINITY;
        for (int c = c0; c < c1; ++c) mx = fmaxf(mx, p[c] * inv_temp);
        mx = block_max<256>(mx, sh);
        float s = 0.f;
        for (int c = c0; c < c1; ++c) s += __expf(p[c] * inv_temp - mx);
        part[t] = s;
        __syncthreads();
        if (t == 0) {
            const int rd = round ? min(max(round[0], 0), u_rounds - 1) : 0;
            float tot = 0.f;
            for (int i = 0; i < 256; ++i) tot += part[i];
            const float target = u[(long)rd * rows + r] * tot;
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
            s_tok = idx;
        }
    }
    if (t == 0) {
        const int w = s_tok;
        tok[r] = w;
        const int n = len[r];
        if (!done[r] && n >= 0 && n < Lmax) {
            const float lp = (p[min(max(w, 0), V - 1)] - mx1) - logf(s1);   // log softmax at temperature 1
            seq[r * Lmax + n] = w;
            len[r] = n + 1;
            logprob[r] += (double)lp;
            if (w == eos) done[r] = 1;
        }
    }
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

__device__ __forceinline__ bool rank_better(double sa, int a, double sb, int b) { return sa > sb || (sa == sb && a < b); }

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
            if (j != k && rank_better(s_score[j], j, sc, k)) lead = 0;
        }
    }
    s_lead[k] = lead;
    __syncthreads();
    const int nd = (int)block_sum<256>(lead ? 1.f : 0.f, sh);
    if (lead) {
        int pos = 0;
        for (int j = 0; j < K; ++j)
            if (s_lead[j] && j != k && (s_end[j] > e || (s_end[j] == e && rank_better(s_score[j], j, sc, k)))) ++pos;
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
    if (V <= PICK_LDS_MAX)
        hipLaunchKernelGGL(decode_pick_kernel<true>, dim3((unsigned)rows), dim3(256), (size_t)V * sizeof(float), (hipStream_t)stream, logits,
                           rows, V, ld, inv_temp, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob);
    else
        hipLaunchKernelGGL(decode_pick_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, rows, V, ld,
                           inv_temp, u, u_rounds, round, eos, tok, done, seq, Lmax, len, logprob);
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
