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
// precision dispatch of a function template call FN<T>(args...) at the precision's element type (prec_info, internal.h): F5_PREC_F16X3
// runs the f32 instantiation (on split operands) -- and so does whatever is not a plain precision, where an entry does not refuse it
static constexpr PrecElem kernel_elem(int prec) { return prec_info(prec).plain() ? prec_info(prec).elem : PE_F32; }
#define F5K_BY_PREC(prec, FN, ...) \
    (kernel_elem(prec) == PE_BF16 ? FN<bf16_t>(__VA_ARGS__) : kernel_elem(prec) == PE_F16 ? FN<f16_t>(__VA_ARGS__) : FN<float>(__VA_ARGS__))
// the 16-bit output type of operand type T: T itself, f16 for e4m3 operands (as in the engine)
template <typename T> struct Out16 { using type = T; };
template <> struct Out16<e4m3_t> { using type = f16_t; };
// an optional int on the device: v >= 0 uploaded, else null (the m_limit of a packed batch)
struct DevInt {
    Scratch<int> d;
    int set(int v) {
        if (v < 0) return F5_OK;
        HIPCHK(d.alloc(1));
        HIPCHK(hipMemcpy(d.p, &v, 4, hipMemcpyHostToDevice));
        return F5_OK;
    }
    const int* get() const { return d.p; }
};

// f32 rows -> f16 hi / lo planes in place (split_planar_kernel); the split forms exist for f32 rows only
template <typename T> static hipError_t split_planes(hipStream_t s, T* w, size_t elems) {
    if constexpr (std::is_same_v<T, float>)
        hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)(elems / 32))), dim3(256), 0, s, w, (long)(elems / 32));
    return hipGetLastError();
}

// The operands of a test GEMM: A [M, K], W [N, K] (f32, rows of lda / ldw) cast to T in zero-padded rows of Kp, then split as `ops` says.
// T = e4m3_t (F5_PREC_F8): quantised row by row per the contract (quant_rows_e4m3_kernel), with one scale byte per row in sa / sw.
template <typename T> struct GemmStage {
    Scratch<T> a, w;
    Scratch<unsigned char> sa, sw;   // (null for every other T)
    int Kp = 0;
    int stage(hipStream_t s, const float* A, int lda, const float* W, int ldw, int M, int N, int K, int Kp_,
              GemmOperands ops = GemmOperands::Plain) {
        Kp = Kp_;
        HIPCHK(a.alloc((size_t)M * Kp));
        HIPCHK(w.alloc((size_t)N * Kp));
        if constexpr (std::is_same_v<T, e4m3_t>) {
            HIPCHK(sa.alloc((size_t)M + 16));
            HIPCHK(sw.alloc((size_t)N + 16));
            launch_quant_rows_e4m3<float>(s, A, lda, M, K, Rows8{&a.p->v, sa.p, Kp}, nullptr);
            launch_quant_rows_e4m3<float>(s, W, ldw, N, K, Rows8{&w.p->v, sw.p, Kp}, nullptr);
            KCHK();
        } else {
            hipLaunchKernelGGL((cast_pad_kernel<T>), dim3(ew_blocks((long)M * Kp)), dim3(256), 0, s, A, lda, M, K, a.p, Kp, M);
            hipLaunchKernelGGL((cast_pad_kernel<T>), dim3(ew_blocks((long)N * Kp)), dim3(256), 0, s, W, ldw, N, K, w.p, Kp, N);
            KCHK();
            if (ops != GemmOperands::Plain) HIPCHK(split_planes(s, w.p, (size_t)N * Kp));
            if (ops == GemmOperands::AWSplit) HIPCHK(split_planes(s, a.p, (size_t)M * Kp));
        }
        return F5_OK;
    }
};
