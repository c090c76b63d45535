// Kernels of the MMDiT backbone's joint attention (engine_impl.h run_mmdit_forward) that the other backbones do not have.
//
// The joint sequence of a batch row is laid out TEXT FIRST: positions [0, nt) are the text stream c, positions [nt, nt + N) the audio
// stream x.  Softmax does not depend on key order, and with this order the valid keys of a batch row (every text key, the audio keys
// below the row's own length) are the prefix nt + len: the attention kernels mask a key prefix, so they run unchanged.  q / k / v^T of
// both streams land in the joint image straight from the two QKV GEMMs (gemm.h EpiQKV<TO, true>), and with qk_norm
// qknorm_rope_kernel (elementwise.h) norms and rotates one stream of it at (layout length, offset); what is left is below.
#pragma once
#include "elementwise.h"

namespace f5 {

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
