// e4m3 operands for the "TN" GEMM (F5_PREC_F8, include/f5_hip.h):  C[m][n] = 2^(ba[m] + bw[n] - 254) * sum_k codeA[m][k] codeW[n][k]
// on the block-scaled MFMA of gfx950, v_mfma_scale_f32_16x16x128_f8f6f4 with both operands OCP e4m3 (cbsz = blgp = 0): twice the
// bf16 / f16 rate per clock at half the operand bytes.
//
// The kernel is the LDS-DMA ring of gemm2.h at T = e4m3_t: a 128-byte LDS row is exactly one K = 128 step, so the staging, the XOR
// swizzle, the counted waits, the device row count, the remainder launch (GemmConv::m_base) and every store path are the ring's own.
// What differs is in this file:
//   * the MFMA step (Mma8): lane l of a fragment holds row (l & 15) and the two 16-byte chunks g = l >> 4 and 4 + g of that row's 128
//     codes -- 32 bytes, one operand of the instruction.  Both operands are read with the SAME lane -> k map, and a sum over k does not
//     care which bijection it is (the f32 form of gemm.h relies on the same fact), so the instruction's own A / B lane -> k map need
//     not be known -- only that it is the same for both operands.  The C / D map is shape-determined: that of the 16x16x32 forms.
//   * the scales (EpiScale8): one e8m0 byte per A row and per W row (output channel).  The instruction's scale operands are fed the
//     constant byte 127 (2^0) and the two powers of two are multiplied onto the f32 accumulators before the epilogue sees them --
//     exact (a power-of-two factor only moves the exponent), and independent of the instruction's scale byte selection.  EpiScale8
//     wraps an existing epilogue through its fragment-order row / col / preload / store interface; it copies none.
#pragma once
#include "e4m3.h"
#include <utility>
#include "gemm.h"

namespace f5 {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// one K = 128 step of a 16x16 tile: (a0, a1) / (b0, b1) = chunks g and 4 + g of the lane's row of each operand
struct Mma8 {
    static __device__ __forceinline__ f32x4 run(const u32x4& a0, const u32x4& a1, const u32x4& b0, const u32x4& b1, f32x4 c) {
        const i32x8 a = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
        const i32x8 b = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
};

// An epilogue behind the two scale vectors: sa[m] of the A row, sw[n] of the W row (n % 4 == 0 groups are read as one 32-bit word:
// sw is 4-byte aligned).  Rows and columns arrive clamped to the problem (gemm2.h), so every scale read is inside its array; the row
// index is the epilogue's own (m_base added by the kernel), hence the A scales are indexed from the first row of the whole problem.
// No staged form (gemm.h kStaged): the fragment-order paths only.
template <typename E, typename = void> struct epi_wt_of { static int get(const E&) { return 0; } };   // the inner epilogue's write-through switch, if it has one
template <typename E> struct epi_wt_of<E, std::void_t<decltype(std::declval<const E&>().wt)>> { static int get(const E& e) { return e.wt; } };
template <typename Epi> struct EpiScale8 {
    Epi in;
    const unsigned char* sa;
    const unsigned char* sw;
    int wt;   // in.wt (the ring kernel reads it from the epilogue it is given)
    EpiScale8(const Epi& e, const unsigned char* a, const unsigned char* w) : in(e), sa(a), sw(w), wt(epi_wt_of<Epi>::get(e)) {}
    static constexpr bool kWT = Epi::kWT, kRegroup16 = Epi::kRegroup16, kTransposes = Epi::kTransposes;
    struct RowCtx { typename Epi::RowCtx r; float s; };
    struct ColCtx { typename Epi::ColCtx c; f32x4 s; };
    struct TRowCtx { typename Epi::TRowCtx r; f32x4 s; };
    struct TColCtx { typename Epi::TColCtx c; float s; };
    typedef typename Epi::Pre Pre;
    __device__ __forceinline__ bool tile_transposed(int n0) const { return in.tile_transposed(n0); }
    __device__ __forceinline__ RowCtx row(int m) const { return {in.row(m), e8m0_value(sa[m])}; }
    __device__ __forceinline__ ColCtx col(int n) const {
        const unsigned b = *reinterpret_cast<const unsigned*>(sw + n);
        return {in.col(n), f32x4{e8m0_value(b & 255u), e8m0_value((b >> 8) & 255u), e8m0_value((b >> 16) & 255u), e8m0_value(b >> 24)}};
    }
    __device__ __forceinline__ Pre preload(const RowCtx& r, const ColCtx& c) const { return in.preload(r.r, c.c); }
    static __device__ __forceinline__ f32x4 scaled(f32x4 v, float rs, f32x4 cs) {
        return f32x4{v[0] * rs * cs[0], v[1] * rs * cs[1], v[2] * rs * cs[2], v[3] * rs * cs[3]};
    }
    template <bool WT = false>
    __device__ __forceinline__ void store(const RowCtx& r, const ColCtx& c, f32x4 v, const Pre& p) const {
        if constexpr (WT) in.template store<true>(r.r, c.c, scaled(v, r.s, c.s), p);
        else in.store(r.r, c.c, scaled(v, r.s, c.s), p);
    }
    __device__ __forceinline__ u32x2 pack(const RowCtx& r, const ColCtx& c, f32x4 v, const Pre& p) const {
        return in.pack(r.r, c.c, scaled(v, r.s, c.s), p);
    }
    __device__ __forceinline__ bool pair_ok(int n0, int n1) const { return in.pair_ok(n0, n1); }
    __device__ __forceinline__ bool keep(const RowCtx& r) const { return in.keep(r.r); }
    __device__ __forceinline__ auto dst_base(const ColCtx& c) const { return in.dst_base(c.c); }
    __device__ __forceinline__ size_t dst_off(const RowCtx& r, const ColCtx& c) const { return in.dst_off(r.r, c.c); }
    // transposed orientation: v[r] = C[m + r][n]; rows past the last one (M - 1) take its scale and are not stored
    __device__ __forceinline__ TRowCtx trow(int m, int M) const {
        return {in.trow(m, M), f32x4{e8m0_value(sa[min(m, M - 1)]), e8m0_value(sa[min(m + 1, M - 1)]), e8m0_value(sa[min(m + 2, M - 1)]),
                                     e8m0_value(sa[min(m + 3, M - 1)])}};
    }
    __device__ __forceinline__ TColCtx tcol(int n) const { return {in.tcol(n), e8m0_value(sw[n])}; }
    template <bool WT = false> __device__ __forceinline__ void tstore(const TRowCtx& r, const TColCtx& c, f32x4 v) const {
        if constexpr (WT) in.template tstore<true>(r.r, c.c, scaled(v, c.s, r.s));
        else in.tstore(r.r, c.c, scaled(v, c.s, r.s));
    }
};

}  // namespace f5
