// Scoring given captions under the model (generate.py: CaptionGenerator.score).
//   vc_logits_logprob_f32  lp[r] = log softmax(hs[r] . W + bias)[labels[r]] with the [rows, V] logits never written: the logits product
//                          on the f32 MFMA tile engine (gemm_core.h, the tiles and main loop of gemm_kernel) with an epilogue that reduces
//                          each 128-column tile of a row to (max, sum exp(x - max)) and picks out the label's logit, then a per-row
//                          merge of the tiles' pairs in ascending tile order.
//   vc_score_reduce_f64    per caption and draw the float64 sum of its tokens' terms, and the marginal over the draws.
// Forward only: the training step keeps vc_gemm_f32 + vc_softmax_xent_f32, whose backward needs d(logits).
#include <math.h>
#include "gemm_core.h"
#include "vaecap.h"

namespace vc {

using CfgScore = TileCfg<2, 2, 2, 2>;   // gemm_kernel's 128 x 128 tile: four waves of 64 x 64

struct ScoreArgs {
    const float* hs;
    const float* W;
    const float* bias;
    const int32_t* labels;
    float2* part;   // [tiles_n][rows] (max, sum exp(x - max)) of a row's columns inside one tile
    float* lab;     // [rows] the label's logit (rows with a label in [0, V) only)
    long pitch, ldw;
    int rows, V, Vload, H;
    int tiles_n, ntiles;
};

// One workgroup per 128 x 128 tile of the logits, K = H unsplit: what a row gets depends on its own operands only (the tile plan is the
// same for every 128-row block whatever `rows` is), and every workspace element is written by exactly one workgroup.
template <bool VEC>
__global__ __launch_bounds__(CfgScore::NT) void logits_partial_kernel(ScoreArgs g) {
    using CFG = CfgScore;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float2 halves[CFG::BM][CFG::WN];   // a wave reduces its 64 columns of a row; the two column waves meet here
    const int id = xcd_remap(blockIdx.x, g.ntiles);
    const int tn_ = id % g.tiles_n;
    const int m0 = (id / g.tiles_n) * CFG::BM, n0 = tn_ * CFG::BN;
    f32x16 acc[CFG::TM][CFG::TN];
    acc_zero<CFG>(acc);
    LoadMK<VEC> la;
    la.p = g.hs; la.ld = g.pitch; la.R = g.rows; la.K = g.H;
    LoadKM<VEC> lb;
    lb.p = g.W; lb.ld = g.ldw; lb.R = g.Vload; lb.K = g.H;
    mfma_mainloop<CFG, MODE_MK, MODE_KM>(acc, la, lb, m0, n0, 0, g.H, smem);
    const float NINF = -INFINITY;
    // (every lane runs the whole body: the 16 lanes that share a row reduce it with lane shuffles)
    epilogue_rows<CFG>(acc, smem, [&](int r, int c, float4 v) {
        const int row = m0 + r, col = n0 + c;
        float x[4] = {v.x, v.y, v.z, v.w};
        float m = NINF;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (col + i < g.V) {   // columns >= V (the padding of the stored kernel) never enter the sum
                if (g.bias) x[i] += g.bias[col + i];
                m = fmaxf(m, x[i]);
            } else {
                x[i] = NINF;
            }
        }
        if (row < g.rows) {
            const int lbl = g.labels[row];
            const int d = lbl - col;
            if (d >= 0 && d < 4 && lbl < g.V) g.lab[row] = d == 0 ? x[0] : d == 1 ? x[1] : d == 2 ? x[2] : x[3];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.f;
        if (m > NINF) {
#pragma unroll
            for (int i = 0; i < 4; ++i) s += __expf(x[i] - m);   // (exp(-inf) = 0 for the masked columns)
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((c & 63) == 0) halves[r][c >> 6] = make_float2(m, s);
    });
    // (epilogue_rows ends on a barrier: the halves are visible)
    const int r = threadIdx.x;
    if (r < CFG::BM && m0 + r < g.rows) {
        const float2 a = halves[r][0], b = halves[r][1];   // a: columns n0 .. n0+63 hold at least one column < V
        const float m = fmaxf(a.x, b.x);
        float s = a.y * __expf(a.x - m);
        if (b.x > NINF) s += b.y * __expf(b.x - m);
        g.part[(long)tn_ * g.rows + m0 + r] = make_float2(m, s);
    }
}

// One thread per row: the tiles' pairs merged in ascending tile order (fixed order: deterministic, and independent of `rows`).
__global__ __launch_bounds__(256) void logprob_merge_kernel(const float2* __restrict__ part, const float* __restrict__ lab,
                                                           const int32_t* __restrict__ labels, int rows, int V, int tiles_n,
                                                           float* __restrict__ lp) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int lbl = labels[r];
    if (lbl < 0 || lbl >= V) {   // row not scored
        lp[r] = 0.f;
        return;
    }
    float m = part[r].x;
    for (int t = 1; t < tiles_n; ++t) m = fmaxf(m, part[(long)t * rows + r].x);
    float s = 0.f;
    for (int t = 0; t < tiles_n; ++t) {
        const float2 p = part[(long)t * rows + r];
        s += p.y * expf(p.x - m);
    }
    lp[r] = lab[r] - (m + logf(s));
}

constexpr int SCORE_MAX_K = 256;

// One wave per caption; lane l owns the draws l, l + 64, ... (K <= 256).
__global__ __launch_bounds__(64) void score_reduce_kernel(const float* __restrict__ lp, int T, int C, int K, const int32_t* __restrict__ len,
                                                          double* __restrict__ logprob, double* __restrict__ marginal) {
    const int c = blockIdx.x, lane = threadIdx.x;
    int n = len[c];
    n = n < 0 ? 0 : (n > T ? T : n);
    const long N = (long)C * K;
    double v[SCORE_MAX_K / 64];
    double mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SCORE_MAX_K / 64; ++j) {
        const int k = lane + j * 64;
        double s = 0.0;
        if (k < K) {
            for (int t = 0; t < n; ++t) s += (double)lp[t * N + (long)c * K + k];   // ascending t, float64 sum (bound_reduce_kernel repeats it)
            logprob[(long)c * K + k] = s;
            mx = fmax(mx, s);
        }
        v[j] = s;
    }
    mx = wave_max(mx);
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < SCORE_MAX_K / 64; ++j)
        if (lane + j * 64 < K) e += exp(v[j] - mx);
    e = wave_sum(e);
    if (lane == 0) marginal[c] = mx + log(e) - log((double)K);
}

}  // namespace vc

using namespace vc;

static int score_tiles_n(int V) { return cdiv(V, CfgScore::BN); }

extern "C" size_t vc_logits_logprob_workspace_bytes(long rows, int V, int H) {
    (void)H;
    if (rows <= 0 || V <= 0) return 0;
    return (size_t)rows * (2 * (size_t)score_tiles_n(V) + 1) * sizeof(float);
}

extern "C" int vc_logits_logprob_f32(void* stream, long rows, int V, int H, const float* hs, long pitch, const float* W, long ldw,
                                     const float* bias, const int32_t* labels, float* lp, float* ws, size_t ws_bytes) {
    VC_CHECK_ARG(rows >= 0 && V > 0 && H > 0, "bad shape");
    VC_CHECK_ARG(rows < (1L << 31) - CfgScore::BM, "too many rows");
    VC_CHECK_ARG(H % 32 == 0, "H must be a multiple of 32");
    VC_CHECK_ARG(hs && W && labels && lp, "null operand");
    VC_CHECK_ARG(pitch >= H && ldw >= V, "leading dimension too small");
    if (rows == 0) return 0;
    if (!ws || ws_bytes < vc_logits_logprob_workspace_bytes(rows, V, H) || ((uintptr_t)ws & 7))
        return fail(VC_EWORKSPACE, "%s: workspace too small or not 8-byte aligned (need vc_logits_logprob_workspace_bytes)", __func__);
    ScoreArgs g;
    g.hs = hs; g.W = W; g.bias = bias; g.labels = labels;
    g.tiles_n = score_tiles_n(V);
    g.part = reinterpret_cast<float2*>(ws);
    g.lab = ws + 2 * (size_t)g.tiles_n * rows;
    g.pitch = pitch; g.ldw = ldw;
    g.rows = (int)rows; g.V = V; g.H = H;
    const long ntiles = (long)cdiv(rows, CfgScore::BM) * g.tiles_n;
    VC_CHECK_ARG(ntiles < (1L << 31), "too many tiles");
    g.ntiles = (int)ntiles;
    auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    // 16-byte operand loads: a quad of columns that straddles V reads the stored kernel's padding (< ldw), which the epilogue masks
    const bool vec = al(hs) && al(W) && pitch % 4 == 0 && ldw % 4 == 0;
    g.Vload = vec ? (V + 3) / 4 * 4 : V;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(logits_partial_kernel<true>, dim3(g.ntiles), dim3(CfgScore::NT), CfgScore::SMEM_BYTES, st, g);
    else hipLaunchKernelGGL(logits_partial_kernel<false>, dim3(g.ntiles), dim3(CfgScore::NT), CfgScore::SMEM_BYTES, st, g);
    VC_LAUNCH_CHECK();
    hipLaunchKernelGGL(logprob_merge_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, g.part, g.lab, labels, g.rows, V, g.tiles_n, lp);
    VC_LAUNCH_CHECK();
    return 0;
}

extern "C" int vc_score_reduce_f64(void* stream, const float* lp, int T, int C, int K, const int32_t* len, double* logprob, double* marginal) {
    VC_CHECK_ARG(T >= 0 && C >= 0, "bad shape");
    VC_CHECK_ARG(K >= 1 && K <= SCORE_MAX_K, "K must be 1..256");
    VC_CHECK_ARG(len && logprob && marginal && (lp || T == 0), "null operand");
    if (C == 0) return 0;
    hipLaunchKernelGGL(score_reduce_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, lp, T, C, K, len, logprob, marginal);
    VC_LAUNCH_CHECK();
    return 0;
}
