// Decoding controls on device (generate.py: the `controls` keyword of the decoders; controls.py: DecodeControls): a row's logits are
// processed IN PLACE from the words the row has emitted so far, before the round's pick / softmax / top-k reads them.
//
//   vc_decode_controls_f32   per row, in this order: repetition penalty (every distinct history word once), no-repeat n-gram bans,
//                            the banned table, <EOS> banned below the minimum length.  Banned = -FLT_MAX, a finite value: every consumer
//                            gives the word probability exactly 0 and the top-k kernels, which mark taken slots with -inf, still return
//                            valid, distinct indices.
//
// One wave64 per row, CTRL_ROWS rows per workgroup; the row's history and the banned table are staged in LDS, positions are strided over
// the lanes.  A row touches at most W + n_banned + 1 logits: the kernel is launch latency, not bandwidth.  Every touched address has ONE
// owner lane, which resolves "penalised and banned" before its single store (no atomics, no reliance on store order):
//   a word of the history   -> the lane of its FIRST occurrence (penalty, and every kind of ban: an n-gram ban is always a history word)
//   a word of the table     -> the lane of its table entry, unless the word is in the history
//   <EOS> below min_len     -> lane 0, unless the word is in the history or the table
#include <float.h>
#include <math.h>

#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int CTRL_ROWS = 4;          // waves (rows) per workgroup
constexpr int CTRL_MAX_LEN = 2048;    // history positions staged per row (CTRL_ROWS * 8 KiB of LDS)
constexpr int CTRL_MAX_BANNED = 256;
constexpr int CTRL_MAX_NGRAM = 8;

__device__ __forceinline__ bool in_sorted(const int32_t* tab, int n, int w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo < n && tab[lo] == w;
}

__global__ __launch_bounds__(64 * CTRL_ROWS) void decode_controls_kernel(float* __restrict__ logits, long rows, int V, long ld,
                                                                          const int32_t* __restrict__ hist, long hist_ld, int Lmax, int skip,
                                                                          const int32_t* __restrict__ len, const int32_t* __restrict__ done,
                                                                          int ngram, int min_len, int eos, float penalty, float inv_penalty,
                                                                          const int32_t* __restrict__ banned, int n_banned) {
    extern __shared__ int32_t s_hist[];   // [CTRL_ROWS][Lmax]
    __shared__ int32_t s_ban[CTRL_MAX_BANNED];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * CTRL_ROWS + wv;
    const bool active = r < rows && !(done && done[r] != 0);
    int W = 0;
    if (active) W = min(max(len[r], skip), Lmax) - skip;   // 0 <= W <= Lmax - skip: stale or wild lengths read nothing out of bounds
    int32_t* h = s_hist + (long)wv * Lmax;
    for (int i = lane; i < W; i += 64) h[i] = hist[r * hist_ld + skip + i];
    for (int j = threadIdx.x; j < n_banned; j += 64 * CTRL_ROWS) s_ban[j] = banned[j];
    __syncthreads();
    if (!active) return;
    float* x = logits + r * ld;
    const bool ban_eos = W < min_len;
    const bool ng = ngram > 0 && W >= ngram;
    const int sfx = W - ngram + 1;   // the suffix h[sfx .. W) of ngram - 1 words

    // ---- words of the history, each at its first occurrence
    for (int i = lane; i < W; i += 64) {
        const int w = h[i];
        if (w < 0 || w >= V) continue;
        bool first = true;
        for (int j = 0; j < i && first; ++j) first = h[j] != w;
        if (!first) continue;
        bool ban = (ban_eos && w == eos) || in_sorted(s_ban, n_banned, w);
        if (ng && !ban) {
            for (int p = max(i, ngram - 1); p < W && !ban; ++p) {
                if (h[p] != w) continue;
                bool same = true;
                for (int q = 0; q < ngram - 1 && same; ++q) same = h[p - ngram + 1 + q] == h[sfx + q];
                ban = same;
            }
        }
        if (ban) {
            x[w] = -FLT_MAX;
        } else if (penalty != 1.0f) {
            const float v = x[w];
            x[w] = v > 0.f ? v * inv_penalty : v * penalty;
        }
    }
    // ---- words of the table that the history does not hold
    for (int j = lane; j < n_banned; j += 64) {
        const int w = s_ban[j];
        if (w < 0 || w >= V) continue;
        bool seen = false;
        for (int i = 0; i < W && !seen; ++i) seen = h[i] == w;
        if (!seen) x[w] = -FLT_MAX;
    }
    // ---- <EOS> below the minimum length, when neither of the above owns it
    if (lane == 0 && ban_eos && !in_sorted(s_ban, n_banned, eos)) {
        bool seen = false;
        for (int i = 0; i < W && !seen; ++i) seen = h[i] == eos;
        if (!seen) x[eos] = -FLT_MAX;
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_decode_controls_f32(void* stream, float* logits, long rows, int V, long ld, const int32_t* hist, long hist_ld, int Lmax,
                                      int skip, const int32_t* len, const int32_t* done, int ngram, int min_len, int eos, float penalty,
                                      const int32_t* banned, int n_banned) {
    VC_CHECK_ARG(rows >= 0 && V > 0 && ld >= V, "bad shape (rows >= 0, V > 0, ld >= V)");
    VC_CHECK_ARG(Lmax > 0 && Lmax <= CTRL_MAX_LEN && hist_ld >= Lmax && skip >= 0 && skip <= Lmax, "bad history layout (0 < Lmax <= 2048, hist_ld >= Lmax, 0 <= skip <= Lmax)");
    VC_CHECK_ARG(ngram >= 0 && ngram <= CTRL_MAX_NGRAM, "ngram must be 0..8 (0 = off)");
    VC_CHECK_ARG(min_len >= 0, "min_len must be >= 0 (0 = off)");
    VC_CHECK_ARG(penalty >= 1.0f && penalty < INFINITY, "penalty must be finite and >= 1 (1 = off)");
    VC_CHECK_ARG(n_banned >= 0 && n_banned <= CTRL_MAX_BANNED && (n_banned == 0 || banned), "n_banned must be 0..256, with a table");
    VC_CHECK_ARG(eos >= 0 && eos < V, "eos outside [0, V)");
    if (rows == 0) return 0;
    VC_CHECK_ARG(logits && hist && len, "null pointer");
    const long grid = (rows + CTRL_ROWS - 1) / CTRL_ROWS;
    VC_CHECK_ARG(grid <= 0x7fffffffl, "too many rows for one launch");
    hipLaunchKernelGGL(decode_controls_kernel, dim3((unsigned)grid), dim3(64 * CTRL_ROWS), (size_t)CTRL_ROWS * Lmax * sizeof(int32_t),
                       (hipStream_t)stream, logits, rows, V, ld, hist, hist_ld, Lmax, skip, len, done, ngram, min_len, eos, penalty,
                       1.0f / penalty, banned, n_banned);
    VC_LAUNCH_CHECK();
    return 0;
}
