// The glue of CFM.forward (cfm.py:261-300) around one backbone evaluation: f5_flow_loss (engine_impl.h) and the test exports
// f5k_flow_mix / f5k_flow_loss_reduce (kapi.hip) launch these kernels through the helpers below.  Inference-mode only: no gradient.
//
// Arithmetic contract (the library is built with -ffp-contract=off: every product below is rounded before it is added)
//   flow_mix_kernel    phi[b, n, c]  = (1.0f - t[b]) * x0[b, n, c] + t[b] * x1[b, n, c]      f32, in torch's order of (1 - t) * x0 + t * x1
//                      cond[b, n, c] = +0.0 for span[b].x <= n < span[b].y, else the bits of x1[b, n, c]
//                      every frame n < N is written, the frames at or past an item's length like any other (cfm.py:279-283 does so)
//   flow_loss_kernel   for a span frame:  f = x1 - x0 (f32), d = pred - f (f32), d * d and every sum in f64
//                      row[b, n] = the frame's sum over mel: lane l (0 .. 63) folds the float4s c = l, l + 64, ... of the row in that order,
//                      inside a float4 x, y, z, w in that order, onto +0.0; then six butterfly rounds v[l] += v[l ^ o], o = 32, 16, .., 1
//                      frame_err[b, n] = (float)(row / (double)mel) inside the span, +0.0 outside it
//                      part[b, k] = the rows of the block's FLOW_BLOCK_FRAMES frames: wave w folds its frames n = 64 k + w, + 4, ... in
//                      that order onto +0.0 (a frame outside the span adds nothing), then (((+0.0 + wave 0) + wave 1) + wave 2) + wave 3
//                      a frame outside the span is not read: pred, x0 and x1 may hold anything there (NaN included)
//   flow_loss_finish_kernel  sq_sum[b] = lane l folds part[b, l], part[b, l + 64], ... onto +0.0, then the same six butterfly rounds;
//                      count[b] = span[b].y - span[b].x
// One fixed order, no atomics: two runs agree bit for bit, and sq_sum is a sum of non-negative f64 terms.
#pragma once
#include "elementwise.h"

namespace f5 {

// the six butterfly rounds of wave_sum, on a double: every lane ends with the same sum
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int FLOW_BLOCK_FRAMES = 64;   // frames of one flow_loss_kernel block: 4 waves x 16 frames, one wave per frame row

// mel % 4 == 0.  One float4 per lane, consecutive lanes on consecutive addresses; x0 and x1 are read once.  cond may be null.
static __global__ void flow_mix_kernel(const float* __restrict__ x0, const float* __restrict__ x1, const float* __restrict__ t,
                                       const int2* __restrict__ span, float* __restrict__ phi, float* __restrict__ cond, int B, int N,
                                       int mel) {
    const int c4n = mel / 4;
    const long per_row = (long)N * c4n, total = (long)B * per_row;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per_row);
        const int n = (int)((i - (long)b * per_row) / c4n);
        const float tb = t[b], om = 1.0f - tb;
        const int2 sp = span[b];
        const float4 a = reinterpret_cast<const float4*>(x0)[i], v = reinterpret_cast<const float4*>(x1)[i];
        store4(phi + i * 4, om * a.x + tb * v.x, om * a.y + tb * v.y, om * a.z + tb * v.z, om * a.w + tb * v.w);
        if (cond) {
            const bool in = n >= sp.x && n < sp.y;
            reinterpret_cast<float4*>(cond)[i] = in ? make_float4(0.f, 0.f, 0.f, 0.f) : v;
        }
    }
}
inline void launch_flow_mix(hipStream_t s, const float* x0, const float* x1, const float* t, const int2* span, float* phi, float* cond, int B,
                            int N, int mel) {
    hipLaunchKernelGGL(flow_mix_kernel, dim3(ew_blocks((long)B * N * mel / 4)), dim3(256), 0, s, x0, x1, t, span, phi, cond, B, N, mel);
}

// grid (ceil(N / FLOW_BLOCK_FRAMES), B), 256 threads.  part f64[B, gridDim.x]; frame_err f32[B, N] or null.
static __global__ void flow_loss_kernel(const float* __restrict__ pred, const float* __restrict__ x0, const float* __restrict__ x1,
                                        const int2* __restrict__ span, double* __restrict__ part, float* __restrict__ frame_err, int N,
                                        int mel) {
    __shared__ double wave_part[4];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c4n = mel / 4;
    const int2 sp = span[b];
    const int n_end = min((int)(blockIdx.x + 1) * FLOW_BLOCK_FRAMES, N);
    double acc = 0.0;   // (wave-uniform: wave_sum_f64 leaves the row's sum in every lane)
    for (int n = blockIdx.x * FLOW_BLOCK_FRAMES + wave; n < n_end; n += 4) {
        const size_t row = (size_t)b * N + n;
        if (n < sp.x || n >= sp.y) {
            if (frame_err && lane == 0) frame_err[row] = 0.0f;
            continue;
        }
        double v = 0.0;
        for (int c = lane; c < c4n; c += F5_WAVE) {
            const float4 p = reinterpret_cast<const float4*>(pred + row * mel)[c];
            const float4 a = reinterpret_cast<const float4*>(x0 + row * mel)[c];
            const float4 z = reinterpret_cast<const float4*>(x1 + row * mel)[c];
            const float dx = p.x - (z.x - a.x), dy = p.y - (z.y - a.y), dz = p.z - (z.z - a.z), dw = p.w - (z.w - a.w);
            v += (double)dx * (double)dx;
            v += (double)dy * (double)dy;
            v += (double)dz * (double)dz;
            v += (double)dw * (double)dw;
        }
        v = wave_sum_f64(v);
        if (frame_err && lane == 0) frame_err[row] = (float)(v / (double)mel);
        acc += v;
    }
    if (lane == 0) wave_part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int w = 0; w < 4; ++w) sum += wave_part[w];
        part[(size_t)b * gridDim.x + blockIdx.x] = sum;
    }
}
// grid B, one wave
static __global__ void flow_loss_finish_kernel(const double* __restrict__ part, const int2* __restrict__ span, int nparts,
                                               double* __restrict__ sq_sum, int* __restrict__ count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double v = 0.0;
    for (int k = lane; k < nparts; k += F5_WAVE) v += part[(size_t)b * nparts + k];
    v = wave_sum_f64(v);
    if (lane == 0) {
        const int2 sp = span[b];
        sq_sum[b] = v;
        count[b] = sp.y - sp.x;
    }
}
inline int flow_loss_parts(int N) { return (N + FLOW_BLOCK_FRAMES - 1) / FLOW_BLOCK_FRAMES; }
// part: scratch of B * flow_loss_parts(N) doubles, 8-byte aligned
inline void launch_flow_loss(hipStream_t s, const float* pred, const float* x0, const float* x1, const int2* span, double* part,
                             double* sq_sum, int* count, float* frame_err, int B, int N, int mel) {
    const int nparts = flow_loss_parts(N);
    hipLaunchKernelGGL(flow_loss_kernel, dim3(nparts, B), dim3(256), 0, s, pred, x0, x1, span, part, frame_err, N, mel);
    hipLaunchKernelGGL(flow_loss_finish_kernel, dim3(B), dim3(F5_WAVE), 0, s, part, span, nparts, sq_sum, count);
}

}  // namespace f5
