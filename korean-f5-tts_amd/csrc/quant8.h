// Row quantisers of F5_PREC_F8 (include/f5_hip.h "The f8 arithmetic contract"): a row of K real elements -> K OCP e4m3fn codes and ONE
// power-of-two scale, stored as an e8m0 byte b (value 2^(b - 127)).
//   scale: the smallest power of two s with amax / s <= 448 (amax over the row's K real elements; amax == 0: b = 127)
//   code : e4m3(x / s), round to nearest even, saturating at +-448; x / s is exact, so the code is a pure function of x and b
// (the arithmetic of both: e4m3.h)
// Two forms share them: quant_rows_e4m3_kernel (any rows of f32 / 16-bit values: attention output, FF hidden, weights at
// f5_finalize, the kernel-level entries) and the e4m3 output form of the AdaLN LayerNorm (elementwise.h layernorm_body), which
// quantises the f32 value LN(x)(1 + scale) + shift with no 16-bit step between.
#pragma once
#include "elementwise.h"
#include "gemm8.h"

namespace f5 {

template <typename T> __device__ __forceinline__ float4 load4_f32(const T* p);
template <> __device__ __forceinline__ float4 load4_f32<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 load4_f32<f16_t>(const f16_t* p) {
    const f16x4 v = *reinterpret_cast<const f16x4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
template <> __device__ __forceinline__ float4 load4_f32<bf16_t>(const bf16_t* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// T [R, ld] (K real elements per row, K % 4 == 0) -> codes [R, ldc] (columns K .. Kc - 1 are written as zero codes: the K padding of
// a GEMM operand; Kc % 4 == 0, Kc <= ldc) + scales [R].  One wave per row, two passes over the row (the second one hits the cache).
// m_limit: the device row count of a packed batch -- rows at or past it (or R) are neither read nor written.
template <typename T>
__global__ __launch_bounds__(256) void quant_rows_e4m3_kernel(const T* __restrict__ x, long ld, int R, int K, unsigned char* __restrict__ codes,
                                                              long ldc, int Kc, unsigned char* __restrict__ scales,
                                                              const int* __restrict__ m_limit) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R || (m_limit && r >= *m_limit)) return;
    const T* xr = x + (size_t)r * ld;
    float amax = 0.f;
    for (int c = lane * 4; c < K; c += 256) {
        const float4 v = load4_f32<T>(xr + c);
        amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    const unsigned b = e8m0_for_amax(wave_max(amax));
    const float inv = e8m0_inverse(b);
    unsigned* cr = reinterpret_cast<unsigned*>(codes + (size_t)r * ldc);
    for (int c = lane * 4; c < Kc; c += 256) {
        unsigned word = 0u;
        if (c < K) {
            const float4 v = load4_f32<T>(xr + c);
            word = e4m3_pack4(v.x, v.y, v.z, v.w, inv);
        }
        cr[c >> 2] = word;
    }
    if (lane == 0) scales[r] = (unsigned char)b;
}
template <typename T>
inline void launch_quant_rows_e4m3(hipStream_t s, const T* x, long ld, int R, int K, unsigned char* codes, long ldc, int Kc, unsigned char* scales,
                                   const int* m_limit) {
    hipLaunchKernelGGL((quant_rows_e4m3_kernel<T>), dim3((R + 3) / 4), dim3(256), 0, s, x, ld, R, K, codes, ldc, Kc, scales, m_limit);
}
// ... into an operand whose rows are zero-padded up to their pitch
template <typename T> inline void launch_quant_rows_e4m3(hipStream_t s, const T* x, long ld, int R, int K, const Rows8& out, const int* m_limit) {
    launch_quant_rows_e4m3<T>(s, x, ld, R, K, out.codes, out.pitch, out.pitch, out.scales, m_limit);
}

// The e4m3 output form of the two AdaLN LayerNorm kernels: codes [R, ldo] + one scale byte per row (layernorm_body, TO = e4m3_t).
// Kernels of their own, so that the ones every other precision launches keep their arguments and their code.
static __global__ __launch_bounds__(256) void layernorm_q8_kernel(const float* __restrict__ x, int ldx, e4m3_t* __restrict__ out, int ldo, int R, int D,
                                                           float eps, const float* __restrict__ A, const float* __restrict__ Bv, int vec_stride,
                                                           int rows_per_batch, int modulate, Prefetch pf, const int* __restrict__ m_limit,
                                                           unsigned char* __restrict__ scales) {
    layernorm_body<e4m3_t, false>(x, ldx, out, ldo, R, D, eps, A, Bv, vec_stride, rows_per_batch, modulate, pf, m_limit, 0, 0, nullptr, scales);
}
static __global__ __launch_bounds__(256) void layernorm_rows_q8_kernel(const float* __restrict__ x, int ldx, e4m3_t* __restrict__ out, int ldo, int R,
                                                                int D, float eps, const float* __restrict__ A, const float* __restrict__ Bv,
                                                                int vec_stride, Prefetch pf, const int* __restrict__ m_limit,
                                                                const int2* __restrict__ rowmap, unsigned char* __restrict__ scales) {
    layernorm_body<e4m3_t, true>(x, ldx, out, ldo, R, D, eps, A, Bv, vec_stride, 0, 1, pf, m_limit, 0, 0, rowmap, scales);
}
// the e4m3 output form of launch_adaln_norm (elementwise.h): codes in rows of out.pitch + one scale byte per row
inline void launch_adaln_norm(hipStream_t s, const AdaLN& a, const Rows8& out) {
    const dim3 grid((a.R + 3) / 4), block(256);
    e4m3_t* codes = reinterpret_cast<e4m3_t*>(out.codes);
    if (a.rowmap)
        hipLaunchKernelGGL(layernorm_rows_q8_kernel, grid, block, 0, s, a.x, a.D, codes, out.pitch, a.R, a.D, a.eps, a.scale, a.shift, a.vec_stride, a.pf,
                           a.m_limit, a.rowmap, out.scales);
    else
        hipLaunchKernelGGL(layernorm_q8_kernel, grid, block, 0, s, a.x, a.D, codes, out.pitch, a.R, a.D, a.eps, a.scale, a.shift, a.vec_stride,
                           a.rows_per_batch, 1, a.pf, a.m_limit, out.scales);
}

}  // namespace f5
