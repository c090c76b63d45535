// OCP e4m3fn codes and e8m0 power-of-two scales (F5_PREC_F8, include/f5_hip.h "The f8 arithmetic contract"): plain integer arithmetic on
// the f32 bit pattern -- no conversion instruction whose rounding or saturation mode would have to be trusted -- and __host__ __device__,
// so that a CPU program checks the same text the kernels run.
#pragma once
#include "f5_common.h"

namespace f5 {

struct e4m3_t { unsigned char v; };   // one OCP e4m3fn code (never fnuz)

// A GEMM operand of F5_PREC_F8 as a value: rows of e4m3 codes `pitch` bytes apart and one e8m0 scale byte per row (an activation's rows, a
// weight's output channels).  Empty where there is none.  (The row quantisers that fill one are in quant8.h.)
struct Rows8 {
    unsigned char* codes = nullptr;
    unsigned char* scales = nullptr;
    int pitch = 0;
    explicit operator bool() const { return codes != nullptr; }
    const e4m3_t* e4m3() const { return reinterpret_cast<const e4m3_t*>(codes); }
    Rows8 from_row(size_t r) const { return {codes + r * pitch, scales + r, pitch}; }   // the rows from r on
    Rows8 at_pitch(int p) const { return {codes, scales, p}; }                          // the same storage as rows of p codes
};

// 2^(b - 127) of an e8m0 scale byte b (1 .. 254: a normal f32)
__host__ __device__ __forceinline__ float e8m0_value(unsigned b) {
    const unsigned bits = b << 23;
    return __builtin_bit_cast(float, bits);
}

// e8m0 byte of the row scale for a row maximum amax >= 0 (finite).  amax = m 2^e, 1 <= m < 2: s = 2^(e - 8) if m <= 1.75 (448 =
// 1.75 * 2^8), else 2^(e - 7).  Clamped below at byte 1 (rows whose amax is under 2^-118: the codes are then all zero or tiny).
__host__ __device__ __forceinline__ unsigned e8m0_for_amax(float amax) {
    const unsigned bits = __builtin_bit_cast(unsigned, amax);
    if (bits == 0u) return 127u;
    const int b = (int)(bits >> 23) - 8 + ((bits & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    return (unsigned)(b < 1 ? 1 : b);
}
// 1 / s of scale byte b (1 .. 253), exact
__host__ __device__ __forceinline__ float e8m0_inverse(unsigned b) { return e8m0_value(254u - b); }

// OCP e4m3fn code of y (finite), round to nearest even, saturating at +-448.  Normal results: the f32 mantissa rounded to 3 bits in
// the bit pattern (a carry moves into the exponent by itself; 448 = 0x7E is the largest, so nothing below it rounds past it);
// below 2^-6 the subnormal grid of step 2^-9, where 8 steps are the smallest normal's code.
__host__ __device__ __forceinline__ unsigned e4m3_code(float y) {
    const unsigned yb = __builtin_bit_cast(unsigned, y);
    const unsigned sign = (yb >> 24) & 0x80u;
    unsigned ab = yb & 0x7FFFFFFFu;
    if (ab > 0x43E00000u) ab = 0x43E00000u;   // 448.0f
    unsigned code;
    if (ab < 0x3C800000u) {                   // |y| < 2^-6
        code = (unsigned)__builtin_rintf(__builtin_bit_cast(float, ab) * 512.0f);   // (round to nearest even)
    } else {
        code = ((ab + 0x7FFFFu + ((ab >> 20) & 1u)) >> 20) - (120u << 3);
    }
    return sign | code;
}
__host__ __device__ __forceinline__ unsigned e4m3_pack4(float a, float b, float c, float d, float inv) {
    return e4m3_code(a * inv) | (e4m3_code(b * inv) << 8) | (e4m3_code(c * inv) << 16) | (e4m3_code(d * inv) << 24);
}

}  // namespace f5
