// Contrastive search (Su et al., NeurIPS 2022), the per-row pick of one round (include/vaecap.h: vc_contrastive_pick_f32).
//
// A row has k candidate words with their probabilities and, from one decoder step over rows * k rows, the k LSTM outputs h_i that
// feeding each candidate gives.  The pick is the candidate with the largest
//     s_i = (1 - alpha) * p_i - alpha * max_j <h_i, g_j> / ||h_i||
// over the unit vectors g_j of the row's history (the states its caption has produced so far); equal s goes to the lower rank.
//
// One workgroup of four waves per row.  Wave w owns the candidates w, w + 4, w + 8, w + 12 and keeps them in registers (lane l the
// float4s l, l + 64, ... of each); every history vector is then streamed ONCE per wave, float4 per lane, and multiplied into all of the
// wave's candidates -- not once per candidate, which would read k * n * H floats per row.  A dot product is a lane's partial sum in index
// order followed by the xor tree of wave_sum: its bits depend on H alone, never on the number of rows, on the row's place in the launch
// or on k.  The scores meet in LDS, every thread takes the same pick from them, and the whole workgroup writes the row's outputs with
// vector stores; nothing is shared between rows and there are no atomics.
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int CS_MAX_K = 16;      // candidates per row
constexpr int CS_WAVES = 4;       // waves per row
constexpr int CS_PER_WAVE = CS_MAX_K / CS_WAVES;

struct ContrastiveArgs {
    int k, H, Lmax, eos, emit;
    float alpha;
    const float* h2;          // [rows * k, H] look-ahead states
    const int32_t* cand_tok;  // [rows, k]
    const float* cand_p;      // [rows, k]
    float* hist;              // [rows, Lmax + 1, H] unit vectors
    int32_t* len;             // [rows]
    int32_t* done;            // [rows]
    int32_t* seq;             // [rows, Lmax]
    double* logprob;          // [rows]
    float* h_sel;             // [rows, H]
    int32_t* parent;          // [rows * k]
    int32_t* pick;            // [rows] or NULL
    float* score;             // [rows, k] or NULL
};

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// NQ: float4s of a vector per lane (H <= 256 * NQ), the candidates live in registers; NQ == 0: any H, the candidates are re-read from
// memory (their rows stay in the L1 / L2 of the one workgroup that reads them) -- same sums in the same order.
template <int NQ>
__global__ __launch_bounds__(64 * CS_WAVES) void contrastive_pick_kernel(ContrastiveArgs a) {
    __shared__ float sh_s[CS_MAX_K], sh_norm[CS_MAX_K];
    const long row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k, H4 = a.H >> 2;
    const int len0 = a.len[row];
    // (uniform over the workgroup: a finished row writes nothing at all, and a row that already holds Lmax words has no slot left)
    if (a.done[row] != 0 || len0 < 0 || len0 + (a.emit ? 1 : 0) > a.Lmax) return;
    const int n_hist = len0 + (a.emit ? 1 : 0);   // g_0 .. g_len; the <BOS> round (emit == 0, len == 0) has none yet
    const float4* h2 = reinterpret_cast<const float4*>(a.h2) + row * k * H4;
    const float4* hist = reinterpret_cast<const float4*>(a.hist) + row * (long)(a.Lmax + 1) * H4;
    constexpr int RQ = NQ > 0 ? NQ : 1;
    const int nq = NQ > 0 ? NQ : (H4 + 63) / 64;

    // ---- the wave's candidates: into registers, with their squared norms
    float4 cand[CS_PER_WAVE][RQ];
    float nrm[CS_PER_WAVE], best[CS_PER_WAVE];
#pragma unroll
    for (int c = 0; c < CS_PER_WAVE; ++c) {
        const int i = wave + CS_WAVES * c;
        float acc = 0.f;
        if (NQ > 0) {
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
                const int o = lane + 64 * q;
                cand[c][q] = (i < k && o < H4) ? h2[(long)i * H4 + o] : f4zero();
                acc = dot4(cand[c][q], cand[c][q], acc);
            }
        } else {
            cand[c][0] = f4zero();
            if (i < k) {
                for (int q = 0; q < nq; ++q) {
                    const int o = lane + 64 * q;
                    const float4 v = o < H4 ? h2[(long)i * H4 + o] : f4zero();
                    acc = dot4(v, v, acc);
                }
            }
        }
        nrm[c] = sqrtf(wave_sum(acc));
        best[c] = -INFINITY;
    }

    // ---- every history vector once per wave, against all of the wave's candidates
    for (int j = 0; j < n_hist; ++j) {
        const float4* g = hist + (long)j * H4;
        float acc[CS_PER_WAVE];
#pragma unroll
        for (int c = 0; c < CS_PER_WAVE; ++c) acc[c] = 0.f;
        if (NQ > 0) {
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
                const int o = lane + 64 * q;
                const float4 gv = o < H4 ? g[o] : f4zero();
#pragma unroll
                for (int c = 0; c < CS_PER_WAVE; ++c) acc[c] = dot4(cand[c][q], gv, acc[c]);
            }
        } else {
            for (int q = 0; q < nq; ++q) {
                const int o = lane + 64 * q;
                const float4 gv = o < H4 ? g[o] : f4zero();
#pragma unroll
                for (int c = 0; c < CS_PER_WAVE; ++c) {
                    const int i = wave + CS_WAVES * c;
                    if (i < k) acc[c] = dot4(o < H4 ? h2[(long)i * H4 + o] : f4zero(), gv, acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CS_PER_WAVE; ++c) best[c] = fmaxf(best[c], wave_sum(acc[c]));
    }

    // ---- scores into LDS
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CS_PER_WAVE; ++c) {
            const int i = wave + CS_WAVES * c;
            if (i < k) {
                const float sim = (n_hist > 0 && nrm[c] > 0.f) ? best[c] / nrm[c] : 0.f;
                const float s = (1.0f - a.alpha) * a.cand_p[row * k + i] - a.alpha * sim;
                sh_s[i] = s;
                sh_norm[i] = nrm[c];
                if (a.score) a.score[row * k + i] = s;
            }
        }
    }
    __syncthreads();
    int pk = 0;
    float s_best = sh_s[0];
    for (int i = 1; i < k; ++i) {
        const float s = sh_s[i];
        if (s > s_best) { s_best = s; pk = i; }   // strictly greater: equal scores stay with the lower rank
    }
    const float norm = sh_norm[pk];

    // ---- the row's outputs: the picked state (as it is, for the logits product) and its unit vector (the history's next entry)
    const float4* hp = h2 + (long)pk * H4;
    float4* sel = reinterpret_cast<float4*>(a.h_sel) + row * H4;
    float4* app = reinterpret_cast<float4*>(a.hist) + (row * (long)(a.Lmax + 1) + n_hist) * H4;
    for (int o = tid; o < H4; o += 64 * CS_WAVES) {
        const float4 v = hp[o];
        sel[o] = v;
        app[o] = norm > 0.f ? make_float4(v.x / norm, v.y / norm, v.z / norm, v.w / norm) : v;
    }
    if (tid < k) a.parent[row * k + tid] = (int)(row * k) + pk;
    if (tid == 0) {
        if (a.pick) a.pick[row] = pk;
        if (a.emit) {
            const int w = a.cand_tok[row * k + pk];
            a.seq[row * a.Lmax + len0] = w;
            a.len[row] = len0 + 1;
            a.logprob[row] += (double)logf(a.cand_p[row * k + pk]);   // f32 log of the f32 probability, f64 sum (as vc_beam_update)
            a.done[row] = w == a.eos ? 1 : 0;
        }
    }
}

}  // namespace vc

extern "C" int vc_contrastive_pick_f32(void* stream, long rows, int k, int H, int Lmax, const float* h2, const int32_t* cand_tok,
                                       const float* cand_p, float* hist, int32_t* len, int32_t* done, int32_t* seq, double* logprob,
                                       float alpha, int eos, int emit, float* h_sel, int32_t* parent, int32_t* pick, float* score) {
    using namespace vc;
    VC_CHECK_ARG(rows >= 0 && rows <= 0x7fffffffL / CS_MAX_K, "rows out of range");
    VC_CHECK_ARG(k >= 1 && k <= CS_MAX_K, "k must be 1..16");
    VC_CHECK_ARG(H > 0 && H % 4 == 0, "H must be a positive multiple of 4");
    VC_CHECK_ARG(Lmax >= 1, "Lmax must be >= 1");
    VC_CHECK_ARG(alpha >= 0.0f && alpha <= 1.0f, "alpha must be finite and in [0, 1]");   // (a NaN fails both comparisons)
    VC_CHECK_ARG(h2 && cand_tok && cand_p && hist && len && done && seq && logprob && h_sel && parent, "null pointer");
    VC_CHECK_ARG((((uintptr_t)h2 | (uintptr_t)hist | (uintptr_t)h_sel) & 15) == 0, "h2, hist and h_sel must be 16-byte aligned");
    if (rows == 0) return 0;
    const ContrastiveArgs a{k, H, Lmax, eos, emit ? 1 : 0, alpha, h2, cand_tok, cand_p, hist, len, done, seq, logprob, h_sel, parent, pick, score};
    const dim3 grid((unsigned)rows), block(64 * CS_WAVES);
    const hipStream_t st = (hipStream_t)stream;
    if (H <= 256) hipLaunchKernelGGL(contrastive_pick_kernel<1>, grid, block, 0, st, a);
    else if (H <= 512) hipLaunchKernelGGL(contrastive_pick_kernel<2>, grid, block, 0, st, a);
    else if (H <= 1024) hipLaunchKernelGGL(contrastive_pick_kernel<4>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(contrastive_pick_kernel<0>, grid, block, 0, st, a);
    VC_LAUNCH_CHECK();
    return 0;
}
