// Shared by the kernel-level entry points (kapi.hip: f5k_*, kapi_diag.hip: f5x_*).
#pragma once
#include <cstring>

#include "attn2.h"
#include "convpos.h"
#include "elementwise.h"
#include "flow.h"
#include "gemm_dispatch.h"
#include "internal.h"
#include "quant8.h"

using namespace f5;
#define fail f5_fail
// precision dispatch of a function template call FN<T>(args...); F5_PREC_F16X3 runs the f32 instantiation (on split operands)
#define F5K_BY_PREC(prec, FN, ...) \
    ((prec) == F5_PREC_BF16 ? FN<bf16_t>(__VA_ARGS__) : (prec) == F5_PREC_F16 ? FN<f16_t>(__VA_ARGS__) : FN<float>(__VA_ARGS__))

// f32 rows -> f16 hi / lo planes in place (split_planar_kernel); the split forms exist for f32 rows only
template <typename T> static hipError_t split_planes(hipStream_t s, T* w, size_t elems) {
    if constexpr (std::is_same_v<T, float>)
        hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)(elems / 32))), dim3(256), 0, s, w, (long)(elems / 32));
    return hipGetLastError();
}

// The operands of a test GEMM: A [M, K], W [N, K] (f32, rows of lda / ldw) cast to T in zero-padded rows of Kp, then split as `ops` says.
template <typename T> struct GemmStage {
    Scratch<T> a, w;
    int stage(hipStream_t s, const float* A, int lda, const float* W, int ldw, int M, int N, int K, int Kp,
              GemmOperands ops = GemmOperands::Plain) {
        HIPCHK(a.alloc((size_t)M * Kp));
        HIPCHK(w.alloc((size_t)N * Kp));
        hipLaunchKernelGGL((cast_pad_kernel<T>), dim3(ew_blocks((long)M * Kp)), dim3(256), 0, s, A, lda, M, K, a.p, Kp, M);
        hipLaunchKernelGGL((cast_pad_kernel<T>), dim3(ew_blocks((long)N * Kp)), dim3(256), 0, s, W, ldw, N, K, w.p, Kp, N);
        KCHK();
        if (ops != GemmOperands::Plain) HIPCHK(split_planes(s, w.p, (size_t)N * Kp));
        if (ops == GemmOperands::AWSplit) HIPCHK(split_planes(s, a.p, (size_t)M * Kp));
        return F5_OK;
    }
};
