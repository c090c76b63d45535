// Kernels of the MMDiT backbone's joint attention (engine_impl.h run_mmdit_forward) that the other backbones do not have.
//
// The joint sequence of a batch row is laid out TEXT FIRST: positions [0, nt) are the text stream c, positions [nt, nt + N) the audio
// stream x.  Softmax does not depend on key order, and with this order the valid keys of a batch row (every text key, the audio keys
// below the row's own length) are the prefix nt + len: the attention kernels mask a key prefix, so they run unchanged.  q / k / v^T of
// both streams land in the joint image straight from the two QKV GEMMs (gemm.h EpiQKV<TO, true>); what is left is below.
#pragma once
#include "elementwise.h"

namespace f5 {

// qk_norm = "rms_norm" on ONE stream of the joint image (modules.py:588-608): q and k rows [off, off + Ns) of every (batch row, head)
// of [Bp, H, L, 64], as the QKV epilogue left them without rotary and scale, get RMSNorm(64, eps) with the stream's own gains, then
// the rotary embedding at the stream's own position (from 0, all heads), then q its softmax scale -- in place.  16 lanes per row.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_joint_kernel(T* __restrict__ q, T* __restrict__ k, const float* __restrict__ gq,
                                                                const float* __restrict__ gk, const float* __restrict__ rope_cos,
                                                                const float* __restrict__ rope_sin, long rows, int Ns, int L, int off,
                                                                float q_scale, float eps) {
    const long gid = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long r = gid >> 4;                              // (b * H + h) * Ns + pos
    if (r >= rows) return;
    const int d = (int)(gid & 15) * 4;
    const int pos = (int)(r % Ns);
    const long dst = (r / Ns) * L + off + pos;            // row of the joint image
    const float2 cs = *reinterpret_cast<const float2*>(rope_cos + (size_t)pos * 32 + (d >> 1));
    const float2 sn = *reinterpret_cast<const float2*>(rope_sin + (size_t)pos * 32 + (d >> 1));
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        T* p = (which ? k : q) + dst * 64 + d;
        const float4 g = *reinterpret_cast<const float4*>((which ? gk : gq) + d);
        float a0 = to_f32(p[0]), a1 = to_f32(p[1]), a2 = to_f32(p[2]), a3 = to_f32(p[3]);
        float ss = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64); ss += __shfl_xor(ss, 8, 64);
        const float rs = rsqrtf(ss * (1.0f / 64.0f) + eps);
        a0 = a0 * rs * g.x; a1 = a1 * rs * g.y; a2 = a2 * rs * g.z; a3 = a3 * rs * g.w;
        const float r0 = a0 * cs.x - a1 * sn.x, r1 = a1 * cs.x + a0 * sn.x;
        const float r2 = a2 * cs.y - a3 * sn.y, r3 = a3 * cs.y + a2 * sn.y;
        const float sc = which ? 1.0f : q_scale;
        store4(p, r0 * sc, r1 * sc, r2 * sc, r3 * sc);
    }
}

// key lengths of the joint sequence: every text key and the audio keys of the row's own length
static __global__ void joint_lens_kernel(const int* __restrict__ lens, int* __restrict__ out, int n, int nt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = lens[i] + nt;
}

// n16 16-byte pieces of zero (V^T before the first attention launch of a forward reads its Lpad tail columns).  A kernel, not a
// memset: inside a captured sample() body a memset node was seen to leave NaN bit patterns behind on every other replay.
static __global__ void zero_fill16_kernel(uint4* __restrict__ p, long n16) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}

// The attention output [Bp, L = nt + N, row_bytes] split into the dense A operands of the two out-projections: text rows
// [Bp * nt, row_bytes] and audio rows [Bp * N, row_bytes].  Rows move whole, as 16-byte pieces (row_bytes % 16 == 0: inner is a
// multiple of 64 elements), so any in-row operand layout (plain T, or pre-split f32 planes) survives.  oc may be null (the last block
// drops the text half).
static __global__ void joint_split_kernel(const uint4* __restrict__ ao, uint4* __restrict__ oc, uint4* __restrict__ ox, int Bp, int nt,
                                          int N, int row16) {
    const int L = nt + N;
    const long total = (long)Bp * L * row16;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % row16);
        const long row = idx / row16;
        const int b = (int)(row / L), p = (int)(row - (long)b * L);
        if (p < nt) {
            if (oc) oc[((size_t)b * nt + p) * row16 + c] = ao[idx];
        } else {
            ox[((size_t)b * N + (p - nt)) * row16 + c] = ao[idx];
        }
    }
}

}  // namespace f5
