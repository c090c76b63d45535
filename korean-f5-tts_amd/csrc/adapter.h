// Resident adapters (include/f5_hip.h, F5_OPT_ADAPTERS): the kernel that rewrites packed weights in place.
//
// One launch serves a whole switch: blockIdx.y picks a job -- a slot of one of two device-resident descriptor tables (the engine's
// base table: "restore the master", or the adapter's: "master + low-rank term" / "replacement tensor") -- and blockIdx.x a
// 32 x 128 tile of that tensor.  The job list travels BY VALUE in the kernel arguments, so a switch uploads nothing.
//
// Per tile: the fp32 master is read once (float4 per lane), the low-rank term is formed from the 32 rows of B and the 128 columns
// of A the tile needs (staged in LDS 32 ranks at a time), and the result is stored in the operand's final layout: f32 rows, bf16 /
// f16 rows through the paired converts (store4: cvt2_f16, never a fused multiply-convert), or the hi / lo planes of the split
// layout (store4_planar), K padding zeroed.  The 32 lanes of a tile row write 512 (f32, split) or 256 (16-bit) contiguous bytes:
// whole 128-byte lines (ldw is a multiple of 64 elements for every GEMM operand).
//
// The arithmetic is the ABI's contract: acc = acc + B[o][r] * A[r][i] in ascending r, product rounded before the add (the
// library is built with -ffp-contract=off), then W + acc * scale, then the conversion cast_pad_kernel / split_planar_kernel
// apply.  A restore (rank 0) stores the master itself, without the add (W + 0 would turn -0 into +0).
#pragma once
#include "f5_common.h"

namespace f5 {

enum { MK_NONE = 0, MK_F32 = 1, MK_BF16 = 2, MK_F16 = 3, MK_PLANAR = 4,
       MK_TAPS = 5 };   // MK_TAPS: [out, 1, taps] depthwise conv weight -> [taps][out] f32 (permute_last2_kernel's layout)

struct MergeDesc {
    const float* W;   // fp32 source [out, in]: the master, or an adapter's replacement tensor
    const float* A;   // [rank, in]   (rank > 0)
    const float* B;   // [out, rank]
    void* dst0;       // packed destination [out, ldw] (a row offset into a fused operand is already applied)
    void* dst1;       // second destination (F5_PREC_F16P keeps the input projection twice) or null
    int out, in, ldw, rank;
    float scale;
    int kind0, kind1, pad;
};
static_assert(sizeof(MergeDesc) == 72, "MergeDesc layout");

enum { MERGE_TR = 32, MERGE_TC = 128, MERGE_RC = 32, MERGE_MAXJ = 512, MERGE_TABLE_BIT = 0x8000 };
struct MergeJobs { unsigned short slot[MERGE_MAXJ]; };   // MERGE_TABLE_BIT set: the adapter's table

__host__ __device__ inline int merge_tiles(const MergeDesc& d) {
    if (d.kind0 == MK_TAPS) return (d.out * d.in + MERGE_TR * MERGE_TC - 1) / (MERGE_TR * MERGE_TC);
    return ((d.out + MERGE_TR - 1) / MERGE_TR) * ((d.ldw + MERGE_TC - 1) / MERGE_TC);
}

__device__ __forceinline__ void merge_store(void* dst, int kind, size_t row, int ldw, int col, float a, float b, float c, float d) {
    switch (kind) {
        case MK_F32: store4(reinterpret_cast<float*>(dst) + row * ldw + col, a, b, c, d); break;
        case MK_BF16: store4(reinterpret_cast<bf16_t*>(dst) + row * ldw + col, a, b, c, d); break;
        case MK_F16: store4(reinterpret_cast<f16_t*>(dst) + row * ldw + col, a, b, c, d); break;
        case MK_PLANAR: store4_planar(reinterpret_cast<float*>(dst) + row * ldw, col, a, b, c, d); break;
        default: break;
    }
}

static __global__ __launch_bounds__(256) void adapter_merge_kernel(const MergeDesc* __restrict__ base, const MergeDesc* __restrict__ adp,
                                                                   const MergeJobs jobs) {
    const unsigned sl = jobs.slot[blockIdx.y];
    const MergeDesc d = ((sl & MERGE_TABLE_BIT) ? adp : base)[sl & (MERGE_TABLE_BIT - 1)];
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (tile >= merge_tiles(d)) return;   // (uniform: the grid is as wide as the job with the most tiles)
    if (d.kind0 == MK_TAPS) {
        float* o = reinterpret_cast<float*>(d.dst0);
        const int total = d.out * d.in, end = min(total, (tile + 1) * MERGE_TR * MERGE_TC);
        for (int i = tile * MERGE_TR * MERGE_TC + tid; i < end; i += 256) o[i] = d.W[(size_t)(i % d.out) * d.in + i / d.out];
        return;
    }
    const int tiles_c = (d.ldw + MERGE_TC - 1) / MERGE_TC;
    const int r0 = (tile / tiles_c) * MERGE_TR, c0 = (tile % tiles_c) * MERGE_TC;
    const int cg = tid & 31, rg = tid >> 5;   // this lane: columns c0 + 4 cg .. + 3 of rows r0 + 4 rg .. + 3
    const int col = c0 + 4 * cg;
    const bool col_in = col < d.in;           // (in % 4 == 0: a group of four is inside the tensor or all padding)
    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] = 0.f;
    __shared__ float sB[MERGE_TR][MERGE_RC + 1];
    __shared__ __attribute__((aligned(16))) float sA[MERGE_RC][MERGE_TC];
    for (int k0 = 0; k0 < d.rank; k0 += MERGE_RC) {
        const int kc = min((int)MERGE_RC, d.rank - k0);
        for (int i = tid; i < MERGE_TR * MERGE_RC; i += 256) {
            const int row = i >> 5, r = i & 31;
            sB[row][r] = (r0 + row < d.out && r < kc) ? d.B[(size_t)(r0 + row) * d.rank + k0 + r] : 0.f;
        }
        for (int i = tid; i < MERGE_RC * (MERGE_TC / 4); i += 256) {
            const int r = i >> 5, c = c0 + 4 * (i & 31);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < kc && c < d.in) v = *reinterpret_cast<const float4*>(d.A + (size_t)(k0 + r) * d.in + c);
            *reinterpret_cast<float4*>(&sA[r][4 * (i & 31)]) = v;
        }
        __syncthreads();
        for (int r = 0; r < kc; ++r) {   // ascending r, multiply then add: the contract (no fma: -ffp-contract=off)
            const float4 a = *reinterpret_cast<const float4*>(&sA[r][4 * cg]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = sB[4 * rg + j][r];
                acc[j][0] = acc[j][0] + b * a.x;
                acc[j][1] = acc[j][1] + b * a.y;
                acc[j][2] = acc[j][2] + b * a.z;
                acc[j][3] = acc[j][3] + b * a.w;
            }
        }
        __syncthreads();
    }
    if (col >= d.ldw) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = r0 + 4 * rg + j;
        if (row >= d.out) continue;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);   // K padding
        if (col_in) {
            w = *reinterpret_cast<const float4*>(d.W + (size_t)row * d.in + col);
            if (d.rank > 0) {
                w.x = w.x + acc[j][0] * d.scale;
                w.y = w.y + acc[j][1] * d.scale;
                w.z = w.z + acc[j][2] * d.scale;
                w.w = w.w + acc[j][3] * d.scale;
            }
        }
        merge_store(d.dst0, d.kind0, (size_t)row, d.ldw, col, w.x, w.y, w.z, w.w);
        if (d.kind1 != MK_NONE) merge_store(d.dst1, d.kind1, (size_t)row, d.ldw, col, w.x, w.y, w.z, w.w);
    }
}

}  // namespace f5
