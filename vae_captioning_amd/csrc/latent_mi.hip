// Mutual information I(x; z) under the aggregated posterior (latent_mi.py: mutual_information; definitions in DESIGN.md "Bounds",
// "Mutual information"): every draw of every caption scored under every caption's Gaussian posterior, then log-sum-exps over the table.
//
//   vc_gauss_mix_lse_f64   t[n, s, m] = sum_l [ -0.5 ((z[n,s,l] - mean[m,l]) / std_[m,l])^2 - log std_[m,l] ] - 0.5 L log(2 pi)
//                          lse_block[n, s] = log sum_m exp(t[n, s, m]),  lse_full[n] = log sum_m exp(sum_s t[n, s, m])
//                          all float64 on the f32 inputs.
//
// A workgroup of 8 waves owns cpw = 128 / S whole captions = cpw * S (caption, draw) rows, 16 rows per wave (S < 8: cpw = 64 / S, 8 rows
// per wave, so that a wave's pairs of the full code still fit in registers beside those of its rows), and streams the posterior
// table past them in chunks of 64 posteriors (one per lane) by tiles of 32 latent dimensions: the tile's mean and 1 / std_ (one IEEE
// division per table element and workgroup, not per term) go to LDS as float64, transposed so that lane m reads its own posterior, and
// the rows' z tile beside them (read as a broadcast).  A lane keeps sum_l ((z - mean) * (1 / std_))^2 of its 16 rows in registers.
// After a chunk's last tile t = -0.5 * that sum + c[m], c[m] = -sum_l log std_[m,l] - 0.5 L log(2 pi) (a wave sum per posterior,
// once per chunk), enters the lane's running (max, sum) pair of the row, rescaled online.  lse_full: the rows' t of the chunk cross
// the waves through LDS, wave w adds the S terms of captions w, w + 8, ... in ascending s and keeps their pairs (FK of them).
// No atomics.  Every float64 sum has a fixed order: a lane takes m = lane, lane + 64, ... in ascending order, the 64 lanes' pairs are
// merged by a max tree and a sum tree of xor shuffles.  What a caption gets depends on its own z rows and the table only: not on N,
// on its index or on the rows it shares a workgroup with (the geometry depends on S alone).
#include <math.h>
#include "common.h"
#include "vaecap.h"

namespace vc {

constexpr int GM_NW = 8;                 // waves per workgroup
constexpr int GM_ROWS = GM_NW * 16;      // most rows per workgroup (16 per wave) = the largest S
constexpr int GM_SMALL_S = 8;            // below it: 8 rows and 8 full-code pairs per wave; from it on: 16 rows and 2 pairs
constexpr int GM_MC = 64;                // posteriors per chunk: one per lane
constexpr int GM_MCP = GM_MC + 1;        // LDS pitch of a tile row in doubles: the transposed 8-byte stores of 16 lanes fall on 32 banks
constexpr int GM_LT = 32;                // latent dimensions per tile
constexpr double GM_LOG_2PI = 1.8378770664093454835606594728112;

// (max, sum) <- (max, sum) + exp(t): one exp either way; the first term (max = -inf) gives (t, 1)
__device__ __forceinline__ void lse_push(double& mx, double& sm, double t) {
    const double e = exp(-fabs(t - mx));
    sm = t > mx ? fma(sm, e, 1.0) : sm + e;
    mx = fmax(mx, t);
}

// the 64 lanes' pairs -> log sum exp; a lane that never saw a term holds (-inf, 0) and adds nothing
__device__ __forceinline__ double lse_merge(double mx, double sm) {
    const double top = wave_max(mx);
    const double v = mx == -INFINITY ? 0.0 : sm * exp(mx - top);
    return top + log(wave_sum(v));
}

template <int GM_R, int GM_FK>
__global__ __launch_bounds__(GM_NW * 64) void gauss_mix_lse_kernel(long N, long M, int S, int L, int cpw, const float* __restrict__ z,
                                                                   const float* __restrict__ mean, const float* __restrict__ std_,
                                                                   double* __restrict__ lse_block, double* __restrict__ lse_full) {
    __shared__ double mu_s[GM_LT * GM_MCP];     // [l in tile][m in chunk]
    __shared__ double inv_s[GM_LT * GM_MCP];
    __shared__ double z_s[GM_ROWS * GM_LT];     // [row][l in tile]
    __shared__ double t_s[GM_ROWS * 64];        // [row][m in chunk]: the chunk's t, for the sums over s
    __shared__ double c_s[GM_MC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rows_wg = cpw * S;                                  // rows a full workgroup owns (<= GM_ROWS)
    const long row0 = (long)blockIdx.x * rows_wg;                 // its first row of z [N * S, L]
    const long left = N * (long)S - row0;
    const int rows_here = left < rows_wg ? (int)left : rows_wg;   // (whole captions: N * S and row0 are multiples of S)
    const bool wave_live = w * GM_R < rows_here;

    double mx[GM_R], sm[GM_R], fmx[GM_FK], fsm[GM_FK];
#pragma unroll
    for (int r = 0; r < GM_R; ++r) {
        mx[r] = -INFINITY;
        sm[r] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < GM_FK; ++k) {
        fmx[k] = -INFINITY;
        fsm[k] = 0.0;
    }

    for (long m0 = 0; m0 < M; m0 += GM_MC) {
        const int mc = M - m0 < GM_MC ? (int)(M - m0) : GM_MC;
        // c[m] of the chunk: wave w takes the posteriors w, w + 8, ...; lanes stride l.  (c_s of the chunk before was last read ahead of
        // that chunk's closing barrier.)
        for (int mi = w; mi < mc; mi += GM_NW) {
            const float* sg = std_ + (m0 + mi) * L;
            double a = 0.0;
            for (int l = lane; l < L; l += 64) a += log((double)sg[l]);
            a = wave_sum(a);
            if (lane == 0) c_s[mi] = -a - 0.5 * (double)L * GM_LOG_2PI;
        }
        double acc[GM_R];
#pragma unroll
        for (int r = 0; r < GM_R; ++r) acc[r] = 0.0;
        for (int l0 = 0; l0 < L; l0 += GM_LT) {
            const int lt = L - l0 < GM_LT ? L - l0 : GM_LT;
            __syncthreads();   // the tile before has been read (and, at l0 == 0, the chunk before is done with t_s)
            for (int e = tid; e < GM_MC * GM_LT; e += GM_NW * 64) {
                const int j = e & (GM_LT - 1), mi = e / GM_LT;
                double mu = 0.0, iv = 0.0;
                if (mi < mc && j < lt) {   // never past a row's end, never past the table's
                    const long i = (m0 + mi) * L + l0 + j;
                    mu = (double)mean[i];
                    iv = 1.0 / (double)std_[i];
                }
                mu_s[j * GM_MCP + mi] = mu;
                inv_s[j * GM_MCP + mi] = iv;
            }
            for (int e = tid; e < GM_NW * GM_R * GM_LT; e += GM_NW * 64) {
                const int j = e & (GM_LT - 1), q = e / GM_LT;
                z_s[e] = q < rows_here && j < lt ? (double)z[(row0 + q) * L + l0 + j] : 0.0;
            }
            __syncthreads();
            if (wave_live) {
                const double* zr = z_s + w * GM_R * GM_LT;
#pragma unroll 2
                for (int j = 0; j < lt; ++j) {
                    const double mu = mu_s[j * GM_MCP + lane], iv = inv_s[j * GM_MCP + lane];
#pragma unroll
                    for (int r = 0; r < GM_R; ++r) {
                        const double u = (zr[r * GM_LT + j] - mu) * iv;
                        acc[r] = fma(u, u, acc[r]);
                    }
                }
            }
        }
        const bool live = lane < mc;
        const double cm = live ? c_s[lane] : 0.0;
#pragma unroll
        for (int r = 0; r < GM_R; ++r) {
            const double t = fma(-0.5, acc[r], cm);
            t_s[(w * GM_R + r) * 64 + lane] = t;
            if (live && wave_live) lse_push(mx[r], sm[r], t);
        }
        __syncthreads();
        // the S * L-dimensional code: wave w owns the captions w, w + 8, ... of the workgroup; ascending s
#pragma unroll
        for (int k = 0; k < GM_FK; ++k) {
            const int c = k * GM_NW + w;
            if (c * S < rows_here && live) {
                const double* tc = t_s + (long)c * S * 64 + lane;
                double tf = 0.0;
                for (int s = 0; s < S; ++s) tf += tc[s * 64];
                lse_push(fmx[k], fsm[k], tf);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < GM_R; ++r) {
        const int q = w * GM_R + r;
        if (q < rows_here) {   // (uniform over the wave)
            const double v = lse_merge(mx[r], sm[r]);
            if (lane == 0) lse_block[row0 + q] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < GM_FK; ++k) {
        const int c = k * GM_NW + w;
        if (c * S < rows_here) {
            const double v = lse_merge(fmx[k], fsm[k]);
            if (lane == 0) lse_full[(long)blockIdx.x * cpw + c] = v;
        }
    }
}

}  // namespace vc

using namespace vc;

extern "C" int vc_gauss_mix_lse_f64(void* stream, long N, long M, int S, int L, const float* z, const float* mean, const float* std_,
                                    double* lse_block, double* lse_full) {
    VC_CHECK_ARG(N >= 0, "N must be >= 0");
    if (N == 0) return 0;
    VC_CHECK_ARG(M >= 1 && S >= 1 && L >= 1, "M, S and L must be >= 1");
    VC_CHECK_ARG(S <= GM_ROWS, "S must be <= 128 (the rows a workgroup keeps in registers)");
    VC_CHECK_ARG(N < (1L << 31) && M < (1L << 31), "too many rows");
    VC_CHECK_ARG(z && mean && std_, "null operand");
    VC_CHECK_ARG(lse_block && lse_full, "null output");
    if (S < GM_SMALL_S) {
        const int cpw = GM_NW * 8 / S;    // <= 64 = 8 waves x 8 pairs
        hipLaunchKernelGGL((gauss_mix_lse_kernel<8, 8>), dim3((unsigned)((N + cpw - 1) / cpw)), dim3(GM_NW * 64), 0, (hipStream_t)stream, N, M, S,
                           L, cpw, z, mean, std_, lse_block, lse_full);
    } else {
        const int cpw = GM_NW * 16 / S;   // <= 16 = 8 waves x 2 pairs
        hipLaunchKernelGGL((gauss_mix_lse_kernel<16, 2>), dim3((unsigned)((N + cpw - 1) / cpw)), dim3(GM_NW * 64), 0, (hipStream_t)stream, N, M, S,
                           L, cpw, z, mean, std_, lse_block, lse_full);
    }
    VC_LAUNCH_CHECK();
    return 0;
}
