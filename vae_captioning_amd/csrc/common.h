// Shared host/device helpers for libvaecap (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace vc {

// ---- error plumbing: every C-ABI entry returns 0 or a hipError_t / VC_E* code
enum { VC_OK = 0, VC_EINVAL = 10001, VC_EWORKSPACE = 10002 };

char* last_error_buf();  // thread-local, defined in api.hip

inline int fail(int code, const char* fmt, const char* a = "", long b = 0, long c = 0) {
    snprintf(last_error_buf(), 512, fmt, a, b, c);
    return code;
}

#define VC_CHECK_ARG(cond, what)                                              \
    do {                                                                      \
        if (!(cond)) return vc::fail(vc::VC_EINVAL, "%s: invalid argument: " what, __func__); \
    } while (0)

inline int launch_status(const char* fn) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(last_error_buf(), 512, "%s: kernel launch failed: %s", fn, hipGetErrorString(e));
    return (int)e;
}

#define VC_LAUNCH_CHECK()                                                     \
    do {                                                                      \
        int s__ = vc::launch_status(__func__);                                \
        if (s__) return s__;                                                  \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

// wave64 sum
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// block-wide sum for blockDim.x == NT (multiple of 64); result valid in every thread.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* sh /* >= NT/64 floats */) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += sh[i];  // fixed order -> deterministic
    return t;
}
template <int NT>
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float t = sh[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) t = fmaxf(t, sh[i]);
    return t;
}

// max and sum of two per-thread values in ONE pass through LDS (block_max + block_sum with their barriers shared)
__device__ __forceinline__ void block_max_sum(float& mx, float& sm, float* sh /* 8 floats */) {
    mx = wave_max(mx);
    sm = wave_sum(sm);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh[w] = mx; sh[4 + w] = sm; }
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    sm = ((sh[4] + sh[5]) + sh[6]) + sh[7];   // fixed order -> deterministic
}

// sums of four per-thread values in ONE pass through LDS (block_sum four times with the barriers shared), fixed order
__device__ __forceinline__ void block_sum4(float& a, float& b, float& c, float& d, float* sh /* 16 floats */) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); d = wave_sum(d);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh[w] = a; sh[4 + w] = b; sh[8 + w] = c; sh[12 + w] = d; }
    __syncthreads();
    a = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    b = ((sh[4] + sh[5]) + sh[6]) + sh[7];
    c = ((sh[8] + sh[9]) + sh[10]) + sh[11];
    d = ((sh[12] + sh[13]) + sh[14]) + sh[15];
}

// ---- Philox4x32-10 (Salmon et al. 2011), counter = (quad index lo, hi, offset lo, hi) -----
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// the four N(0,1) floats of one Philox quad (Box-Muller); shared by vc_philox_normal_f32 and vc_diverse_latent_f32, whose draws agree
// bit for bit
__device__ __forceinline__ void box_muller4(const uint32_t (&r)[4], float (&f)[4]) {
    const float u1 = ((float)r[0] + 1.0f) * 2.3283064365386963e-10f;  // (0,1]
    const float u2 = (float)r[1] * 2.3283064365386963e-10f;
    const float u3 = ((float)r[2] + 1.0f) * 2.3283064365386963e-10f;
    const float u4 = (float)r[3] * 2.3283064365386963e-10f;
    const float ra = sqrtf(-2.f * __logf(u1)), rb = sqrtf(-2.f * __logf(u3));
    float s, c;
    __sincosf(6.283185307179586f * u2, &s, &c);
    f[0] = ra * c; f[1] = ra * s;
    __sincosf(6.283185307179586f * u4, &s, &c);
    f[2] = rb * c; f[3] = rb * s;
}

// n of a packed n-gram key (four 16-bit word ids, ids >= 1: the highest non-zero 16-bit group); consensus.hip and evaluate.hip
__device__ __forceinline__ int key_order(uint64_t key) {
    return key >= (1ull << 48) ? 4 : key >= (1ull << 32) ? 3 : key >= (1ull << 16) ? 2 : 1;
}

// gemm.hip: split-K partial products for consumers that reduce them in their own kernel (lstm.hip)
int gemm_partials_f32(hipStream_t st, int ta, int tb, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                      float* ws, size_t ws_bytes, int max_splits, int* splits_out);
size_t gemm_partials_bytes(int M, int N, int K, int max_splits);
int gemm_default_precision();   // the deprecated process-wide default of vc_gemm_set_precision (0 unless a caller set it)

}  // namespace vc
