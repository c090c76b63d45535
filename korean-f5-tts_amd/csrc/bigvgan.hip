// BigVGAN v2 generator (mel -> waveform) on gfx950 -- the vocoder of BASELINE config 5 / SURVEY a20, which the reference
// loads from an un-vendored submodule (infer/utils_infer.py:138-152, called as `vocoder(mel)` at :705; forced to fp32,
// :332).  PARITY UNPINNED: neither BigVGAN's source nor its weights are in the container; this restates the published
// architecture of nvidia/bigvgan_v2_24khz_100band_256x (tests/test_bigvgan.py checks the kernels against a CPU
// restatement of the same published design).  All f32, time-major [L, C] activations (no [B, C, T] permutes), every contraction an exact-f32 MFMA GEMM:
//   conv_pre            Conv1d(mels, C0, 7)            = im2col (strided mel view) x W[C0, 7 mels]
//   ups[i]              ConvTranspose1d(C, C/2, k, u)  = GEMM x[L, C] x W'[(tap, co), C]^T -> Z[L, k C/2], then each output
//                                                        sample gathers its k / u taps from Z (+ bias)
//   AMPBlock1 convs     Conv1d(C, C, k, dilation d)    = dilated im2col x W[C, k C] with bias (+ residual) epilogues
//   Activation1d        2x kaiser-sinc upsample -> SnakeBeta -> 2x low-pass downsample, ONE kernel: an output sample needs the
//                       12 upsampled samples around it, each a 6-tap sum over the input rows t-5 .. t+5 held in registers
//   conv_post           Conv1d(C_last, 1, 7) + clamp / tanh, direct (168 MACs per sample)
#include <cmath>
#include <string>
#include <vector>

#include "elementwise.h"
#include "gemm_dispatch.h"
#include "internal.h"

using namespace f5;
#define fail f5_fail

// ------------------------------------------------------------------------------------------------ kernels
// A[t][tap * C + c] = x[t + (tap - (k-1)/2) * dil][c]  (zero outside [0, L); columns >= k C zero: K padding of the GEMM)
static __global__ void bv_im2col_kernel(const float* __restrict__ x, float* __restrict__ A, long L, int C, int k, int dil, int ld) {
    const int l4 = ld / 4;
    const long total = L * l4;
    const int half = (k - 1) / 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % l4) * 4;
        const long t = i / l4;
        float4 v = make_float4(0, 0, 0, 0);
        if (col < k * C) {
            const int tap = col / C, c = col - tap * C;
            const long tt = t + (long)(tap - half) * dil;
            if (tt >= 0 && tt < L) v = *reinterpret_cast<const float4*>(x + tt * C + c);
        }
        reinterpret_cast<float4*>(A)[i] = v;
    }
}

// sin for the snake activation: three-constant Cody-Waite reduction by pi/2 (fma: |x| up to ~1e6 keeps the absolute error
// at the f32 level) + degree-7 / degree-8 minimax polynomials on [-pi/4, pi/4].  Measured against float64 sin over
// |x| <= 200: max |error| 9.2e-8 (libm's f32 sinf: 6.9e-8).  The library sinf inlines a Payne-Hanek path at each of the
// activation kernel's call sites (17,000 instructions, 284 registers, one wave per SIMD); this is ~20 instructions.
__device__ __forceinline__ float bv_sin(float x) {
    const float k = rintf(x * 0.63661977236758134f);
    float r = fmaf(-k, 1.57079637050628662109375f, x);
    r = fmaf(-k, -4.371138828673792886547744274139404296875e-8f, r);
    r = fmaf(-k, -1.7151245100058818728e-15f, r);
    const int q = (int)k;
    const float r2 = r * r;
    const float ps = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f) * r2, r, r);
    const float pc = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f), r2 * r2,
                          fmaf(-0.5f, r2, 1.0f));
    const float res = (q & 1) ? pc : ps;
    return (q & 2) ? -res : res;
}

// precision "f16x3": the same reduction to [-pi, pi] by one multiple of 2 pi, then the hardware v_sin_f32 (argument in revolutions):
// 9 issue slots instead of ~20; max |error| 3.5e-7 over the reduced range (tools/probe/sin_probe.hip) against 9.2e-8.
__device__ __forceinline__ float bv_sin_hw(float x) {
    const float k = rintf(x * 0.15915494309189535f);
    float r = fmaf(-k, 6.283185482025146484375f, x);
    r = fmaf(-k, -1.7484555314695172e-7f, r);
    return __builtin_amdgcn_sinf(r * 0.15915494309189535f);
}
template <bool HW> __device__ __forceinline__ float bv_snake(float v, float a, float invb) {
    const float s = HW ? bv_sin_hw(v * a) : bv_sin(v * a);
    return v + invb * (s * s);
}

// Activation1d(SnakeBeta) (alias-free activation): y[t] = sum_m fd[m] a[clamp(2t + m - 5, 0, 2L-1)],
// a[u] = snake(2 sum_{j = (u+1) mod 2 + 2q} fu[j] x[clamp((u + 15 - j) / 2 - 5, 0, L-1)])
// One thread = BV_TT consecutive time steps x 4 channels, streamed: the 12 upsampled samples a[2t-5 .. 2t+6] that output t
// reads live in registers and slide by two per step; the two new ones (u = 2t+5, 2t+6) both read input rows t .. t+5, a
// six-row register window that slides by one.  Every upsampled sample (one sinf) is so evaluated once per thread instead of
// once per output that reads it: (10 + 2 BV_TT) / BV_TT evaluations per output instead of 12.
constexpr int BV_TT = 8;

struct BvSnake { float a0, a1, a2, a3, b0, b1, b2, b3; };

template <bool HW> __device__ __forceinline__ float4 bv_snake4(const float4 u, const BvSnake& p) {
    return make_float4(bv_snake<HW>(2.0f * u.x, p.a0, p.b0), bv_snake<HW>(2.0f * u.y, p.a1, p.b1), bv_snake<HW>(2.0f * u.z, p.a2, p.b2),
                       bv_snake<HW>(2.0f * u.w, p.a3, p.b3));
}

// a[clamp(u)] from global rows (tile start and sequence edges)
template <bool HW>
__device__ __forceinline__ float4 bv_up_generic(const float* __restrict__ x, long u, long L, int C, int c, const float* sfu,
                                                const BvSnake& p) {
    u = u < 0 ? 0 : (u > 2 * L - 1 ? 2 * L - 1 : u);
    float4 s = make_float4(0, 0, 0, 0);
    for (int j = (int)((u + 1) & 1); j < 12; j += 2) {
        long tt = (u + 15 - j) / 2 - 5;
        tt = tt < 0 ? 0 : (tt > L - 1 ? L - 1 : tt);
        const float f = sfu[j];
        const float4 v = *reinterpret_cast<const float4*>(x + tt * C + c);
        s.x += f * v.x; s.y += f * v.y; s.z += f * v.z; s.w += f * v.w;
    }
    return bv_snake4<HW>(s, p);
}

// One thread's tile: the BV_TT outputs t0 .. t0 + BV_TT - 1 (those below L) of channels c .. c + 3 of ONE sequence x, y: [L, C].
// Both kernels below run exactly this body; the ragged one only puts an index computation in front of it.
template <bool HW>
__device__ __forceinline__ void bv_act_tile(const float* __restrict__ x, float* __restrict__ y, long t0, long L, int C, int c,
                                            const float* __restrict__ log_alpha, const float* __restrict__ log_beta, const float* sfu,
                                            const float* sfd, int planar) {
    const float4 la = *reinterpret_cast<const float4*>(log_alpha + c), lb = *reinterpret_cast<const float4*>(log_beta + c);
    const BvSnake p{expf(la.x), expf(la.y), expf(la.z), expf(la.w), 1.0f / (expf(lb.x) + 1e-9f), 1.0f / (expf(lb.y) + 1e-9f),
                    1.0f / (expf(lb.z) + 1e-9f), 1.0f / (expf(lb.w) + 1e-9f)};
    auto row = [&](long tt) {
        tt = tt < 0 ? 0 : (tt > L - 1 ? L - 1 : tt);
        return *reinterpret_cast<const float4*>(x + tt * C + c);
    };
    float4 a[12], r[6];
#pragma unroll
    for (int m = 0; m < 10; ++m) a[m] = bv_up_generic<HW>(x, 2 * t0 + m - 5, L, C, c, sfu, p);
#pragma unroll
    for (int q = 0; q < 6; ++q) r[q] = row(t0 + q);
#pragma unroll 1
    for (int k = 0; k < BV_TT; ++k) {
        const long t = t0 + k;
        if (t < L) {
            const float4 nxt = row(t + 6);                     // (issued early: consumed at the end of the step)
            // u = 2t+5 (odd): taps j = 2q on rows t+5-q;  u = 2t+6 (even): taps j = 2q+1 on the same rows
            float4 s0 = make_float4(0, 0, 0, 0), s1 = make_float4(0, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const float f0 = sfu[2 * q], f1 = sfu[2 * q + 1];
                const float4 v = r[5 - q];
                s0.x += f0 * v.x; s0.y += f0 * v.y; s0.z += f0 * v.z; s0.w += f0 * v.w;
                s1.x += f1 * v.x; s1.y += f1 * v.y; s1.z += f1 * v.z; s1.w += f1 * v.w;
            }
            // past the end a[u] repeats a[2L-1] (replicate padding of the low-pass filter)
            a[10] = 2 * t + 5 <= 2 * L - 1 ? bv_snake4<HW>(s0, p) : a[9];
            a[11] = 2 * t + 6 <= 2 * L - 1 ? bv_snake4<HW>(s1, p) : a[10];
            float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                const float g = sfd[m];
                acc.x += g * a[m].x; acc.y += g * a[m].y; acc.z += g * a[m].z; acc.w += g * a[m].w;
            }
            store4_at(y + t * C, c, planar, acc.x, acc.y, acc.z, acc.w);
#pragma unroll
            for (int m = 0; m < 10; ++m) a[m] = a[m + 2];
#pragma unroll
            for (int q = 0; q < 5; ++q) r[q] = r[q + 1];
            r[5] = nxt;
        }
    }
}

template <bool HW>
static __global__ __launch_bounds__(256) void bv_act_kernel(const float* __restrict__ x, float* __restrict__ y, long L, int C,
                                                             const float* __restrict__ log_alpha, const float* __restrict__ log_beta,
                                                             const float* __restrict__ fu, const float* __restrict__ fd, int planar) {
    // planar: rows written pre-split for the split-operand convolution GEMM that reads them (f5_common.h store4_planar)
    __shared__ float sfu[12], sfd[12];
    if (threadIdx.x < 12) { sfu[threadIdx.x] = fu[threadIdx.x]; sfd[threadIdx.x] = fd[threadIdx.x]; }
    __syncthreads();
    const int c4n = C / 4;
    const long tiles = (L + BV_TT - 1) / BV_TT;
    const long total = tiles * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        bv_act_tile<HW>(x, y, (i / c4n) * BV_TT, L, C, (int)(i % c4n) * 4, log_alpha, log_beta, sfu, sfd, planar);
}

// ---- ragged batch (f5_bigvgan_forward_ragged): ONE packed time axis.  Item b owns the frames row_start[b] .. + frames[b] of it and
// is followed by dead ("gap") frames up to row_start[b + 1]; at a stage with U rows per frame every row index is the frame index
// times U.  The item of a row is found by binary search over the frame table (segment_of_row, elementwise.h).
struct BvSeg { const int* row_start; const int* frames; int B; };
// row (of a stage with U rows per frame) -> first row *r0 and row count *Lb of its item; false: a gap row behind that item
__device__ __forceinline__ bool bv_item_of_row(const BvSeg& sg, long row, int U, long* r0, long* Lb) {
    const int b = segment_of_row(sg.row_start, sg.B, (int)(row / U));
    *r0 = (long)sg.row_start[b] * U;
    *Lb = (long)sg.frames[b] * U;
    return row - *r0 < *Lb;
}

// The activation over the packed axis (L rows in all).  Every item starts at a multiple of BV_TT rows (f5_bigvgan_ragged_plan), so a
// tile that starts inside an item is the tile the B = 1 call runs at the same offset from the item's first row -- same clamps (the
// item's own first and last row), same register windows, same bits -- and a tile that starts in a gap holds no item row.  Gap rows
// of y are written as zeros (plain or planar): they are the zero padding the convolutions read around each item.
template <bool HW>
static __global__ __launch_bounds__(256) void bv_act_ragged_kernel(const float* __restrict__ x, float* __restrict__ y, long L, int C,
                                                                    const float* __restrict__ log_alpha, const float* __restrict__ log_beta,
                                                                    const float* __restrict__ fu, const float* __restrict__ fd, int planar,
                                                                    BvSeg sg, int U) {
    __shared__ float sfu[12], sfd[12];
    if (threadIdx.x < 12) { sfu[threadIdx.x] = fu[threadIdx.x]; sfd[threadIdx.x] = fd[threadIdx.x]; }
    __syncthreads();
    const int c4n = C / 4;
    const long tiles = (L + BV_TT - 1) / BV_TT;
    const long total = tiles * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        const long t0 = (i / c4n) * BV_TT;
        long r0, Lb;
        if (bv_item_of_row(sg, t0, U, &r0, &Lb))
            bv_act_tile<HW>(x + r0 * C, y + r0 * C, t0 - r0, Lb, C, c, log_alpha, log_beta, sfu, sfd, planar);
        const long z1 = t0 + BV_TT < L ? t0 + BV_TT : L;
        for (long t = t0 > r0 + Lb ? t0 : r0 + Lb; t < z1; ++t) store4_at(y + t * C, c, planar, 0.f, 0.f, 0.f, 0.f);
    }
}

// Conv1d(C, C, k, dilation) for the NARROW last stages (C < 64: 48 and 24 channels in the 24 kHz config, where a GEMM tile
// would be mostly padding and the im2col operand ~200 MB).  One workgroup = 4 waves = 64 MT time steps x all channels:
//   - the input rows [t0 - halo, t0 + TB + halo) are staged once in LDS (row stride C + 1 words: the 16 rows x 2 columns a
//     half-wave reads at once fall in distinct banks), zero outside [0, L): every tap re-reads them shifted, no im2col;
//   - v_mfma_f32_16x16x4_f32 with the WEIGHT as first operand: lane (lr = lane % 16, lk = lane / 16) feeds W[n = 16 nt + lr]
//     [K = 4 kk + lk] and x[t = m0 + lr + shift(tap)][ci = 4 cs + lk], and ends with out[t = m0 + lr][n = 16 nt + 4 lk .. + 3]
//     -- a float4 of channels per lane for the bias / residual / store;
//   - the weights are pre-packed [K / 4][NT][64 lanes] (bv_pack_narrow_kernel) so a fragment is one coalesced 256-byte
//     load, requested one k-step ahead of its use (all workgroups read the same <= 100 KB: L1/L2 hits).
typedef float bv_f32x4 __attribute__((ext_vector_type(4)));

static __global__ void bv_pack_narrow_kernel(const float* __restrict__ w /*[Co][ld] tap-major*/, float* __restrict__ wn, int Co, int ld,
                                             int K, int NT) {
    const long total = (long)(K / 4) * NT * 64;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63), lr = lane & 15, lk = lane >> 4;
        const long f = i >> 6;
        const int nt = (int)(f % NT), kk = (int)(f / NT);
        const int n = nt * 16 + lr;
        wn[i] = n < Co ? w[(long)n * ld + kk * 4 + lk] : 0.0f;
    }
}

template <int NT, int MT>
static __global__ __launch_bounds__(256) void bv_conv_narrow_kernel(const float* __restrict__ x, const float* __restrict__ wn,
                                                                     const float* __restrict__ bias, const float* res, float* out,
                                                                     long L, int C, int k, int dil) {
    extern __shared__ float bv_xs[];
    constexpr int TB = 4 * MT * 16;
    const int half = (k - 1) / 2, halo = half * dil, S = C + 1, rows = TB + 2 * halo, c4n = C / 4;
    const long t0 = (long)blockIdx.x * TB;
    // (four loads in flight per thread, from clamped addresses, before their stores: a load-if-in-range / store loop compiles to
    //  one serialised memory round trip per iteration -- convpos.h)
    for (int base = threadIdx.x; base < rows * c4n; base += 4 * 256) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(base + u * 256, rows * c4n - 1), row = i / c4n, col = (i - row * c4n) * 4;
            const long g = min(max(t0 - halo + row, 0L), L - 1);
            v[u] = *reinterpret_cast<const float4*>(x + g * C + col);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * 256, row = i / c4n, col = (i - row * c4n) * 4;
            const long g = t0 - halo + row;
            const bool in = g >= 0 && g < L;
            if (i < rows * c4n) {
                float* d = bv_xs + row * S + col;
                d[0] = in ? v[u].x : 0.f; d[1] = in ? v[u].y : 0.f; d[2] = in ? v[u].z : 0.f; d[3] = in ? v[u].w : 0.f;
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    bv_f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = bv_f32x4{0, 0, 0, 0};
    const float* wl = wn + lane;
    const float* xl = bv_xs + (wave * MT * 16 + lr + halo) * S + lk;
    const int total = k * c4n;
    float b[NT], bn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b[nt] = wl[nt * 64];
    int kk = 0;
    for (int tap = 0; tap < k; ++tap) {
        const float* xt = xl + (tap - half) * dil * S;
        for (int cs = 0; cs < c4n; ++cs, ++kk) {
            const int kn = min(kk + 1, total - 1);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bn[nt] = wl[(long)(kn * NT + nt) * 64];
            float a[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = xt[mt * 16 * S + cs * 4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nt], a[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = bn[nt];
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const long t = t0 + (wave * MT + mt) * 16 + lr;
        if (t >= L) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = nt * 16 + 4 * lk;
            if (n >= C) continue;
            const float4 bv = *reinterpret_cast<const float4*>(bias + n);
            float4 o = make_float4(acc[mt][nt][0] + bv.x, acc[mt][nt][1] + bv.y, acc[mt][nt][2] + bv.z, acc[mt][nt][3] + bv.w);
            if (res) {
                const float4 rv = *reinterpret_cast<const float4*>(res + t * C + n);
                o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w;
            }
            *reinterpret_cast<float4*>(out + t * C + n) = o;
        }
    }
}

constexpr int BV_NARROW_MT = 2;
static hipError_t launch_conv_narrow(hipStream_t s, const float* x, const float* wn, const float* bias, const float* res, float* out,
                                     long L, int C, int k, int dil) {
    constexpr int MT = BV_NARROW_MT, TB = 4 * MT * 16;
    const int NT = (C + 15) / 16;
    const size_t smem = (size_t)(TB + (k - 1) * dil) * (C + 1) * 4;
    const dim3 grid((unsigned)((L + TB - 1) / TB)), block(256);
    switch (NT) {
        case 1: hipLaunchKernelGGL((bv_conv_narrow_kernel<1, MT>), grid, block, smem, s, x, wn, bias, res, out, L, C, k, dil); break;
        case 2: hipLaunchKernelGGL((bv_conv_narrow_kernel<2, MT>), grid, block, smem, s, x, wn, bias, res, out, L, C, k, dil); break;
        case 3: hipLaunchKernelGGL((bv_conv_narrow_kernel<3, MT>), grid, block, smem, s, x, wn, bias, res, out, L, C, k, dil); break;
        case 4: hipLaunchKernelGGL((bv_conv_narrow_kernel<4, MT>), grid, block, smem, s, x, wn, bias, res, out, L, C, k, dil); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// the narrow kernel's LDS tile must fit the default 64 KB dynamic limit
static bool conv_narrow_ok(int C, int k, int dil) {
    return C % 4 == 0 && C < 64 && (size_t)(4 * BV_NARROW_MT * 16 + (k - 1) * dil) * (C + 1) * 4 <= 64 * 1024;
}

// ConvTranspose1d tail: y[n][co] = bias[co] + sum_q Z[(n + p - j) / u][j * Co + co], j = (n + p) % u + q u < k, 0 <= (n + p - j) / u < Li
__device__ __forceinline__ float4 bv_gather_row(const float* __restrict__ Z, const float* __restrict__ bias, long n, long Li, int Co,
                                                int k, int u, int p, int c) {
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
    for (int j = (int)((n + p) % u); j < k; j += u) {
        const long ii = (n + p - j) / u;
        if (n + p - j >= 0 && ii < Li) {
            const float4 v = *reinterpret_cast<const float4*>(Z + ii * (long)k * Co + (long)j * Co + c);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    return acc;
}
static __global__ void bv_upsample_gather_kernel(const float* __restrict__ Z, const float* __restrict__ bias, float* __restrict__ y,
                                                 long Li, int Co, int k, int u, int p) {
    const int c4n = Co / 4;
    const long Lo = Li * u;
    const long total = Lo * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<float4*>(y)[i] = bv_gather_row(Z, bias, i / c4n, Li, Co, k, u, p, (int)(i % c4n) * 4);
}
// The same over the packed axis (Li packed input rows, Uin of them per frame): an item's output rows take their taps from the Z
// rows of that item only; a gap row gets the bias (something finite: the arena is reused, and this buffer feeds the next GEMM).
static __global__ void bv_upsample_gather_ragged_kernel(const float* __restrict__ Z, const float* __restrict__ bias, float* __restrict__ y,
                                                        long Li, int Co, int k, int u, int p, BvSeg sg, int Uin) {
    const int c4n = Co / 4;
    const long total = Li * u * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        const long n = i / c4n;
        long r0, Lb;   // in output rows
        reinterpret_cast<float4*>(y)[i] = bv_item_of_row(sg, n, Uin * u, &r0, &Lb)
                                              ? bv_gather_row(Z + (r0 / u) * (long)k * Co, bias, n - r0, Lb / u, Co, k, u, p, c)
                                              : *reinterpret_cast<const float4*>(bias + c);
    }
}
// x = (r0 + r1 + ... ) / n over n buffers spaced `stride` floats apart  (xs / num_kernels)
static __global__ void bv_mean_kernel(const float* __restrict__ r, long stride, int n, float* __restrict__ x, long count4) {
    const float inv = 1.0f / (float)n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < count4; i += (long)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<const float4*>(r)[i];
        for (int j = 1; j < n; ++j) {
            const float4 b = reinterpret_cast<const float4*>(r + j * stride)[i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        reinterpret_cast<float4*>(x)[i] = make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
    }
}
// conv_post: wav[t] = clamp / tanh( bias + sum_{tap, c} w[tap * C + c] a[t + tap - 3][c] )
__device__ __forceinline__ float bv_post_sample(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                                long t, long L, int C, int use_tanh) {
    float s = bias ? bias[0] : 0.f;
    for (int tap = 0; tap < 7; ++tap) {
        const long tt = t + tap - 3;
        if (tt < 0 || tt >= L) continue;
        for (int c = 0; c < C; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(a + tt * C + c);
            const float4 ww = *reinterpret_cast<const float4*>(w + tap * C + c);
            s += v.x * ww.x; s += v.y * ww.y; s += v.z * ww.z; s += v.w * ww.w;
        }
    }
    return use_tanh ? tanhf(s) : fminf(fmaxf(s, -1.0f), 1.0f);
}
static __global__ void bv_post_kernel(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                      float* __restrict__ wav, long L, int C, int use_tanh) {
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < L; t += (long)gridDim.x * blockDim.x)
        wav[t] = bv_post_sample(a, w, bias, t, L, C, use_tanh);
}
// The same per item of the packed axis (blockIdx.y = item; U rows per frame): taps inside the item's own rows only, then x gain[b]
// as a separate multiply, then zeros up to wav_stride.  wav [B, wav_stride].
static __global__ void bv_post_ragged_kernel(const float* __restrict__ a, const float* __restrict__ w, const float* __restrict__ bias,
                                             float* __restrict__ wav, long wav_stride, int C, int use_tanh, BvSeg sg, int U,
                                             const float* __restrict__ gain) {
    const int b = blockIdx.y;
    const long L = (long)sg.frames[b] * U;
    const float* ab = a + (long)sg.row_start[b] * U * C;
    const float g = gain[b];
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < wav_stride; t += (long)gridDim.x * blockDim.x)
        wav[b * wav_stride + t] = t < L ? bv_post_sample(ab, w, bias, t, L, C, use_tanh) * g : 0.f;
}
// conv_pre operand of the packed axis: A[r][tap * C + c] = frame (mel_start[b] + t + tap - 3) of batch row b for packed frame
// r = row_start[b] + t, t < frames[b]; taps outside [0, frames[b]) are the conv's zero padding and gap rows are all zero -- frames
// outside an item's window and other items' frames are never read.  One block per packed frame (the lookup is uniform over it).
static __global__ __launch_bounds__(256) void bv_im2col7_ragged_kernel(const float* __restrict__ mel, long sb, long sc, long st,
                                                                       const int* __restrict__ mel_start, float* __restrict__ A, int C,
                                                                       int R, int ld, BvSeg sg) {
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const int b = segment_of_row(sg.row_start, sg.B, r);
        const int t = r - sg.row_start[b], Tb = sg.frames[b];
        const float* src = mel + b * sb + (long)mel_start[b] * st;
        for (int col = threadIdx.x; col < ld; col += blockDim.x) {
            float v = 0.f;
            if (col < 7 * C && t < Tb) {
                const int k = col / C, ci = col - k * C;
                const int tt = t + k - 3;
                if (tt >= 0 && tt < Tb) v = src[ci * sc + tt * st];
            }
            A[(size_t)r * ld + col] = v;
        }
    }
}
// ConvTranspose1d weight [Ci][Co][k] (torch) -> GEMM operand W'[(j * Co + co)][ci]
static __global__ void bv_pack_convT_kernel(const float* __restrict__ in, float* __restrict__ out, int Ci, int Co, int k, int ld) {
    const long total = (long)k * Co * ld;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % ld);
        const long r = i / ld;
        const int co = (int)(r % Co), j = (int)(r / Co);
        out[i] = ci < Ci ? in[((long)ci * Co + co) * k + j] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ handle
namespace {
struct BConv { float *w = nullptr, *b = nullptr, *wn = nullptr; int ld = 0; bool split = false; };   // split: w in the split_planar layout (F5_PREC_F16X3)   // wn: bv_pack_narrow_kernel layout (C < 64 only)          // [Co, ld] tap-major, ld = round_up(k C, 32)
struct BAct { float *alpha = nullptr, *beta = nullptr; };
struct BRes { std::vector<BConv> c1, c2; std::vector<BAct> act; int k = 0; };
struct BUp { float *w = nullptr, *b = nullptr; int ci = 0, co = 0, k = 0, u = 0, ld = 0; bool split = false; };
}  // namespace

struct f5_bigvgan {
    f5_bigvgan_config cfg{};
    WeightStore raw;
    DevPool pool;   // what finalize built
    bool finalized = false;
    BConv pre;
    int kpre = 0;
    std::vector<BUp> ups;
    std::vector<BRes> res;
    BAct post_act;
    float *post_w = nullptr, *post_b = nullptr, *fu = nullptr, *fd = nullptr;
    int c_last = 0, total_up = 1;
    Arena arena;
    Staging stage;   // pinned slots for the ragged call's per-item tables
};

extern "C" int f5_bigvgan_create(const f5_bigvgan_config* c, f5_bigvgan** out) {
    if (!c || !out) return fail(F5_EINVAL, "f5_bigvgan_create: null argument");
    if (c->num_upsamples <= 0 || c->num_upsamples > 8 || c->num_kernels <= 0 || c->num_kernels > 4 || c->num_dilations <= 0 ||
        c->num_dilations > 4 || c->num_mels % 4 || c->upsample_initial_channel % (4 << c->num_upsamples))
        return fail(F5_EINVAL, "f5_bigvgan_create: unsupported dimensions (channels must stay a multiple of 4 after every halving)");
    for (int i = 0; i < c->num_upsamples; ++i)
        if (c->upsample_rates[i] <= 0 || c->upsample_kernel_sizes[i] % c->upsample_rates[i] || (c->upsample_kernel_sizes[i] - c->upsample_rates[i]) % 2)
            return fail(F5_EINVAL, "f5_bigvgan_create: upsample kernel must be a multiple of its rate and k - u even");
    for (int j = 0; j < c->num_kernels; ++j)
        if (c->resblock_kernel_sizes[j] % 2 == 0) return fail(F5_EINVAL, "f5_bigvgan_create: resblock kernels must be odd");
    if (c->precision != F5_PREC_F32 && c->precision != F5_PREC_F16X3)
        return fail(F5_EINVAL, "f5_bigvgan_create: precision must be F5_PREC_F32 or F5_PREC_F16X3");
    f5_bigvgan* v = new f5_bigvgan();
    v->cfg = *c;
    v->kpre = round_up(7 * c->num_mels, 32);
    v->c_last = c->upsample_initial_channel >> c->num_upsamples;
    for (int i = 0; i < c->num_upsamples; ++i) v->total_up *= c->upsample_rates[i];
    *out = v;
    return F5_OK;
}
extern "C" int f5_bigvgan_destroy(f5_bigvgan* v) {
    if (v) {
        (void)hipDeviceSynchronize();
        delete v;
    }
    return F5_OK;
}
extern "C" int f5_bigvgan_load_weight(f5_bigvgan* v, const char* name, const void* dev, const int64_t* shape, int32_t ndim,
                                      f5_stream stream) {
    if (!v) return fail(F5_EINVAL, "f5_bigvgan_load_weight: bad arguments");
    CHK(v->raw.put("f5_bigvgan_load_weight", name, dev, shape, ndim, (hipStream_t)stream));
    v->finalized = false;
    return F5_OK;
}

static int weight_copy(f5_bigvgan* v, hipStream_t s, const std::string& n, std::vector<int64_t> shape, float** out) {
    return v->pool.copy_of(v->raw, n, shape, "bigvgan", s, out);
}
// Conv1d weight [Co, Ci, k] (+ bias) -> tap-major GEMM operand [Co, round_up(k Ci, 32)]
static int bconv(f5_bigvgan* v, hipStream_t s, const std::string& pfx, int Co, int Ci, int k, bool bias, BConv* c) {
    const Tensor* t = nullptr;
    CHK(v->raw.need(pfx + ".weight", {Co, Ci, k}, "bigvgan", &t));
    c->ld = round_up(k * Ci, 32);
    CHK(v->pool.alloc((size_t)Co * c->ld, &c->w));
    hipLaunchKernelGGL((conv_pack_kernel<float>), dim3(ew_blocks((long)Co * c->ld)), dim3(256), 0, s, t->p, c->w, (long)Co, Ci, k, c->ld);
    KCHK();
    c->b = nullptr;
    if (bias) CHK(weight_copy(v, s, pfx + ".bias", {Co}, &c->b));
    c->wn = nullptr;
    if (Co == Ci && Ci % 4 == 0 && Ci < 64 && bias) {
        const int NT = (Co + 15) / 16, K = k * Ci;
        CHK(v->pool.alloc((size_t)(K / 4) * NT * 64, &c->wn));
        hipLaunchKernelGGL(bv_pack_narrow_kernel, dim3(ew_blocks((long)(K / 4) * NT * 64)), dim3(256), 0, s, c->w, c->wn, Co, c->ld, K, NT);
        KCHK();
    }
    c->split = v->cfg.precision == F5_PREC_F16X3 && !c->wn;     // (the narrow stages keep f32 MFMA: 7 % of the generator's flops)
    if (c->split) {
        hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)Co * c->ld / 32)), dim3(256), 0, s, c->w, (long)Co * c->ld / 32);
        KCHK();
    }
    return F5_OK;
}

static const float* epi_res(const EpiStore<float>&) { return nullptr; }
static float* epi_out(const EpiStore<float>& e) { return e.out; }
static const float* epi_res(const EpiGateRes& e) { return e.res; }
static float* epi_out(const EpiGateRes& e) { return e.x; }

extern "C" int f5_bigvgan_finalize(f5_bigvgan* v, f5_stream stream) {
    if (!v) return fail(F5_EINVAL, "null bigvgan");
    hipStream_t s = (hipStream_t)stream;
    const f5_bigvgan_config& c = v->cfg;
    v->pool.clear();
    CHK(bconv(v, s, "conv_pre", c.upsample_initial_channel, c.num_mels, 7, true, &v->pre));
    v->ups.assign(c.num_upsamples, BUp{});
    v->res.assign((size_t)c.num_upsamples * c.num_kernels, BRes{});
    int ch = c.upsample_initial_channel;
    for (int i = 0; i < c.num_upsamples; ++i) {
        BUp& u = v->ups[i];
        u.ci = ch; u.co = ch / 2; u.k = c.upsample_kernel_sizes[i]; u.u = c.upsample_rates[i]; u.ld = round_up(ch, 32);
        const std::string p = "ups." + std::to_string(i) + ".0";
        const Tensor* t = nullptr;
        CHK(v->raw.need(p + ".weight", {u.ci, u.co, u.k}, "bigvgan", &t));
        CHK(v->pool.alloc((size_t)u.k * u.co * u.ld, &u.w));
        hipLaunchKernelGGL(bv_pack_convT_kernel, dim3(ew_blocks((long)u.k * u.co * u.ld)), dim3(256), 0, s, t->p, u.w, u.ci, u.co, u.k, u.ld);
        KCHK();
        u.split = c.precision == F5_PREC_F16X3 && u.ci % 32 == 0;      // (K = ci must be whole K-tiles for the LDS-DMA kernels)
        if (u.split) {
            hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)u.k * u.co * u.ld / 32)), dim3(256), 0, s, u.w, (long)u.k * u.co * u.ld / 32);
            KCHK();
        }
        CHK(weight_copy(v, s, p + ".bias", {u.co}, &u.b));
        ch /= 2;
        for (int j = 0; j < c.num_kernels; ++j) {
            BRes& r = v->res[(size_t)i * c.num_kernels + j];
            r.k = c.resblock_kernel_sizes[j];
            const std::string rp = "resblocks." + std::to_string(i * c.num_kernels + j);
            r.c1.assign(c.num_dilations, BConv{});
            r.c2.assign(c.num_dilations, BConv{});
            r.act.assign(2 * c.num_dilations, BAct{});
            for (int m = 0; m < c.num_dilations; ++m) {
                CHK(bconv(v, s, rp + ".convs1." + std::to_string(m), ch, ch, r.k, true, &r.c1[m]));
                CHK(bconv(v, s, rp + ".convs2." + std::to_string(m), ch, ch, r.k, true, &r.c2[m]));
            }
            for (int a = 0; a < 2 * c.num_dilations; ++a) {
                CHK(weight_copy(v, s, rp + ".activations." + std::to_string(a) + ".act.alpha", {ch}, &r.act[a].alpha));
                CHK(weight_copy(v, s, rp + ".activations." + std::to_string(a) + ".act.beta", {ch}, &r.act[a].beta));
            }
        }
    }
    CHK(weight_copy(v, s, "activation_post.act.alpha", {v->c_last}, &v->post_act.alpha));
    CHK(weight_copy(v, s, "activation_post.act.beta", {v->c_last}, &v->post_act.beta));
    {   // conv_post [1, C, 7] -> [7][C]
        const Tensor* t = nullptr;
        CHK(v->raw.need("conv_post.weight", {1, v->c_last, 7}, "bigvgan", &t));
        CHK(v->pool.alloc((size_t)7 * v->c_last, &v->post_w));
        hipLaunchKernelGGL((permute_last2_kernel<float>), dim3(ew_blocks(7L * v->c_last)), dim3(256), 0, s, t->p, v->post_w, 1L, v->c_last, 7);
        KCHK();
        v->post_b = nullptr;
        if (c.use_bias_at_final) CHK(weight_copy(v, s, "conv_post.bias", {1}, &v->post_b));
    }
    CHK(weight_copy(v, s, "aux.up_filter", {12}, &v->fu));
    CHK(weight_copy(v, s, "aux.down_filter", {12}, &v->fd));
    HIPCHK(hipStreamSynchronize(s));
    v->raw.clear();
    v->finalized = true;
    return F5_OK;
}

namespace {
// Workspace of one pass over T frames: one utterance of the rectangular call (utterances are decoded one after another: a stage's
// im2col operand is ~200 MB at 8 s), or the packed axis of a ragged batch.
struct BvWork {
    float *x, *r, *act, *t1, *col, *Z;
    int* tab;          // ragged only: BvTables
    size_t lc_max;     // floats per residual-block buffer
    int halo;          // zero rows around act for the implicit convolutions
    bool narrow_ok, implicit_ok;
};
// The ragged call's per-item tables, row_start[B + 1] | mel_start[B] | frames[B] | gain[B]: one layout for the pinned slot and BvWork::tab
struct BvTables {
    int *row_start, *mel_start, *frames;
    float* gain;
    BvTables(void* base, int B)
        : row_start(static_cast<int*>(base)), mel_start(row_start + B + 1), frames(mel_start + B), gain(reinterpret_cast<float*>(frames + B)) {}
    static size_t words(int B) { return (size_t)4 * B + 1; }
};
}  // namespace

static int bv_halo(const f5_bigvgan_config& c) {
    int halo = 0;
    for (int j = 0; j < c.num_kernels; ++j)
        for (int m = 0; m < c.num_dilations; ++m) halo = std::max(halo, (c.resblock_kernel_sizes[j] - 1) / 2 * c.resblock_dilations[m]);
    return halo;
}
// does this convolution go through the materialised operand (col)?
static bool bv_conv_uses_col(const BvWork& w, const BConv& cw, int ch, int k, int d) {
    return !(w.narrow_ok && cw.wn && conv_narrow_ok(ch, k, d)) && !(w.implicit_ok && ch % 32 == 0);
}

// carves the workspace out of the handle's arena (Arena::reserve: growth is the only synchronisation of a call).  exact_col: the
// im2col operand only for the stages that materialise it (the ragged call: sized over every stage it is ~270 KB per frame).
static int bv_workspace(f5_bigvgan* v, long T, bool exact_col, size_t ntab, BvWork* w) {
    const f5_bigvgan_config& c = v->cfg;
    w->halo = bv_halo(c);
    w->narrow_ok = !(getenv("F5_BIGVGAN_NARROW") && getenv("F5_BIGVGAN_NARROW")[0] == '0');         // diagnostic: 0 = GEMM path for C < 64
    w->implicit_ok = !(getenv("F5_BIGVGAN_IMPLICIT") && getenv("F5_BIGVGAN_IMPLICIT")[0] == '0');   // diagnostic: 0 = im2col everywhere
    size_t lc_max = (size_t)T * c.upsample_initial_channel, col_max = (size_t)T * v->kpre, z_max = 0;
    {
        long L = T;
        int ch = c.upsample_initial_channel;
        for (int i = 0; i < c.num_upsamples; ++i) {
            z_max = std::max(z_max, (size_t)L * c.upsample_kernel_sizes[i] * (ch / 2));
            L *= c.upsample_rates[i];
            ch /= 2;
            lc_max = std::max(lc_max, (size_t)L * ch);
            for (int j = 0; j < c.num_kernels; ++j) {
                const BRes& rb = v->res[(size_t)i * c.num_kernels + j];
                bool uses = !exact_col;
                for (int m = 0; m < c.num_dilations && !uses; ++m)
                    uses = bv_conv_uses_col(*w, rb.c1[m], ch, rb.k, c.resblock_dilations[m]) || bv_conv_uses_col(*w, rb.c2[m], ch, rb.k, 1);
                if (uses) col_max = std::max(col_max, (size_t)L * round_up(c.resblock_kernel_sizes[j] * ch, 32));
            }
        }
    }
    w->lc_max = lc_max;
    auto plan = [&](Arena& a) {
        a.reset();
        w->x = a.take<float>(lc_max);
        w->r = a.take<float>(lc_max * c.num_kernels);
        w->act = a.take<float>(lc_max + 2 * (size_t)w->halo * (c.upsample_initial_channel / 2));
        w->t1 = a.take<float>(lc_max);
        w->col = a.take<float>(col_max);
        w->Z = a.take<float>(z_max);
        w->tab = a.take<int>(ntab);
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(v->arena.reserve(plan(dry)));
    (void)plan(v->arena);
    return F5_OK;
}

// conv_pre GEMM .. activation_post over the T frames whose conv_pre operand is in w.col; leaves the last activation's output
// [T * total_up, c_last] in w.act.  sg == nullptr: one sequence.  sg: the packed axis of a ragged batch -- the GEMMs, the narrow
// convolution and the im2col run over it as over one long sequence (the zero gap rows of act are every item's padding), the
// activation and the transposed convolution's gather take their segment-aware forms.
static int bv_generator(f5_bigvgan* v, hipStream_t s, const BvWork& w, long T, const BvSeg* sg) {
    const f5_bigvgan_config& c = v->cfg;
    float *x = w.x, *r = w.r, *act = w.act, *t1 = w.t1, *col = w.col, *Z = w.Z;
    const size_t lc_max = w.lc_max;
    const int halo = w.halo;
    const bool narrow_ok = w.narrow_ok, implicit_ok = w.implicit_ok;
    long L = T;
    int ch = c.upsample_initial_channel, U = 1;     // U: rows per frame
    auto activation = [&](const float* in, float* out, const BAct& a, int planar) -> hipError_t {
        const dim3 grid(ew_blocks((L + BV_TT - 1) / BV_TT * (ch / 4))), block(256);
        const bool hw = c.precision == F5_PREC_F16X3;     // (precision f16x3 takes the hardware-sin activation)
        if (sg && hw) hipLaunchKernelGGL(bv_act_ragged_kernel<true>, grid, block, 0, s, in, out, L, ch, a.alpha, a.beta, v->fu, v->fd, planar, *sg, U);
        else if (sg) hipLaunchKernelGGL(bv_act_ragged_kernel<false>, grid, block, 0, s, in, out, L, ch, a.alpha, a.beta, v->fu, v->fd, planar, *sg, U);
        else if (hw) hipLaunchKernelGGL(bv_act_kernel<true>, grid, block, 0, s, in, out, L, ch, a.alpha, a.beta, v->fu, v->fd, planar);
        else hipLaunchKernelGGL(bv_act_kernel<false>, grid, block, 0, s, in, out, L, ch, a.alpha, a.beta, v->fu, v->fd, planar);
        return hipGetLastError();
    };
    HIPCHK(launch_gemm<float>(s, col, v->kpre, v->pre.w, v->pre.ld, (int)T, ch, v->kpre, EpiStore<float>{x, ch, v->pre.b, F5_ACT_NONE},
                              {v->pre.split ? GemmOperands::WSplit : GemmOperands::Plain}));
    for (int i = 0; i < c.num_upsamples; ++i) {
        const BUp& u = v->ups[i];
        // ConvTranspose1d: Z[L, k Co] = x[L, Ci] W'^T, then gather
        HIPCHK(launch_gemm<float>(s, x, u.ci, u.w, u.ld, (int)L, u.k * u.co, u.ci, EpiStore<float>{Z, u.k * u.co, nullptr, F5_ACT_NONE},
                                  {u.split ? GemmOperands::WSplit : GemmOperands::Plain}));
        if (sg)
            hipLaunchKernelGGL(bv_upsample_gather_ragged_kernel, dim3(ew_blocks(L * u.u * (u.co / 4))), dim3(256), 0, s, Z, u.b, x, L, u.co,
                               u.k, u.u, (u.k - u.u) / 2, *sg, U);
        else
            hipLaunchKernelGGL(bv_upsample_gather_kernel, dim3(ew_blocks(L * u.u * (u.co / 4))), dim3(256), 0, s, Z, u.b, x, L, u.co, u.k, u.u,
                               (u.k - u.u) / 2);
        KCHK();
        L *= u.u;
        U *= u.u;
        ch = u.co;
        const long cnt = L * ch;
        // Stages whose channel count is a multiple of the f32 K-tile (32) run their dilated convolutions as implicit GEMMs
        // (GemmConv, gemm2.h) straight off the activation buffer, which then carries `halo` zero rows on both sides; the narrow
        // last stages (48 / 24 channels in the 24 kHz config) keep the materialised operand.
        const bool implicit = implicit_ok && ch % 32 == 0;
        float* acti = act;                      // first activation row
        if (implicit) {
            acti = act + (size_t)halo * ch;
            HIPCHK(hipMemsetAsync(act, 0, (size_t)halo * ch * 4, s));
            HIPCHK(hipMemsetAsync(acti + cnt, 0, (size_t)halo * ch * 4, s));
        }
        auto conv = [&](const BConv& cw, int k, int d, const auto& epi) -> hipError_t {
            if (narrow_ok && cw.wn && conv_narrow_ok(ch, k, d))
                return launch_conv_narrow(s, acti, cw.wn, cw.b, epi_res(epi), epi_out(epi), L, ch, k, d);
            // (AWSplit: the activation kernel wrote these rows pre-split -- planar1 / planar2 below)
            if (implicit) return launch_gemm<float>(s, acti, ch, cw.w, cw.ld, (int)L, ch, cw.ld, epi,
                                                    {cw.split ? GemmOperands::AWSplit : GemmOperands::Plain, -1, nullptr, 0, GemmConv{ch / 32, d, (k - 1) / 2}});
            hipLaunchKernelGGL(bv_im2col_kernel, dim3(ew_blocks(L * (cw.ld / 4))), dim3(256), 0, s, acti, col, L, ch, k, d, cw.ld);
            return launch_gemm<float>(s, col, cw.ld, cw.w, cw.ld, (int)L, ch, cw.ld, epi, {cw.split ? GemmOperands::WSplit : GemmOperands::Plain});
        };
        for (int j = 0; j < c.num_kernels; ++j) {
            const BRes& rb = v->res[(size_t)i * c.num_kernels + j];
            float* rj = r + (size_t)j * lc_max;
            for (int m = 0; m < c.num_dilations; ++m) {
                const float* rin = m == 0 ? x : rj;     // the block's input: the first pair reads x itself (no copy into rj)
                const int d = c.resblock_dilations[m];
                const bool use_narrow1 = narrow_ok && rb.c1[m].wn && conv_narrow_ok(ch, rb.k, d);
                const bool use_narrow2 = narrow_ok && rb.c2[m].wn && conv_narrow_ok(ch, rb.k, 1);
                const int planar1 = implicit && !use_narrow1 && rb.c1[m].split, planar2 = implicit && !use_narrow2 && rb.c2[m].split;
                HIPCHK(activation(rin, acti, rb.act[2 * m], planar1));
                HIPCHK(conv(rb.c1[m], rb.k, d, EpiStore<float>{t1, ch, rb.c1[m].b, F5_ACT_NONE}));
                HIPCHK(activation(t1, acti, rb.act[2 * m + 1], planar2));
                // x_j = x_j + (conv2(.) + bias): residual epilogue (in place from the second pair on)
                HIPCHK(conv(rb.c2[m], rb.k, 1, EpiGateRes{rj, rin, ch, rb.c2[m].b, nullptr, 0, (int)L + 1, nullptr}));
            }
        }
        hipLaunchKernelGGL(bv_mean_kernel, dim3(ew_blocks(cnt / 4)), dim3(256), 0, s, r, (long)lc_max, c.num_kernels, x, cnt / 4);
        KCHK();
    }
    HIPCHK(activation(x, act, v->post_act, 0));
    return F5_OK;
}

// mel f32 addressed as mel[b * sb + c * sc + t * st] (element strides) -> wav f32[B, T * prod(rates)]
extern "C" int f5_bigvgan_forward(f5_bigvgan* v, const float* mel, int32_t B, int32_t T, int64_t sb, int64_t sc, int64_t st,
                                  float* wav, f5_stream stream) {
    if (!v || !mel || !wav) return fail(F5_EINVAL, "f5_bigvgan_forward: null argument");
    if (!v->finalized) return fail(F5_ESTATE, "f5_bigvgan_finalize has not been called");
    if (B <= 0 || T < 1) return fail(F5_EINVAL, "f5_bigvgan_forward: need B >= 1 and T >= 1 frames");
    hipStream_t s = (hipStream_t)stream;
    const f5_bigvgan_config& c = v->cfg;
    BvWork w;
    CHK(bv_workspace(v, T, false, 0, &w));
    const long Lout = (long)T * v->total_up;
    for (int b = 0; b < B; ++b) {
        hipLaunchKernelGGL(im2col7_kernel, dim3(ew_blocks((long)T * v->kpre)), dim3(256), 0, s, mel + (size_t)b * sb, 0L, (long)sc, (long)st,
                           w.col, 1, c.num_mels, T, v->kpre);
        KCHK();
        CHK(bv_generator(v, s, w, T, nullptr));
        hipLaunchKernelGGL(bv_post_kernel, dim3(ew_blocks(Lout)), dim3(256), 0, s, w.act, v->post_w, v->post_b, wav + (size_t)b * Lout, Lout,
                           v->c_last, c.use_tanh_at_final);
        KCHK();
    }
    return F5_OK;
}

// ------------------------------------------------------------------------------------------------ ragged batch
// The layout of the packed axis (pure host arithmetic).  Item b of frames[b] frames starts at frame row_start[b]; behind it come
// at least `gap` dead frames, gap * rates[0] >= the widest convolution's reach (bv_halo), so that at every stage an item's taps end
// in its own rows or in gap rows; every start is rounded up so that its first row at the first stage (and so at every later one) is
// a multiple of the activation kernel's BV_TT-row tile.  row_start[B] = the packed frame count (no gap behind the last item).
static int bv_gcd(int a, int b) { return b ? bv_gcd(b, a % b) : a; }
extern "C" int f5_bigvgan_ragged_plan(const f5_bigvgan_config* c, int32_t B, const int32_t* frames_host, int32_t* row_start_out,
                                      int32_t* gap_frames_out) {
    if (!c || !frames_host || !row_start_out || !gap_frames_out)
        return fail(F5_EINVAL, "f5_bigvgan_ragged_plan: null cfg / frames_host / row_start_out / gap_frames_out");
    if (B <= 0 || B > 65535) return fail(F5_EINVAL, "f5_bigvgan_ragged_plan: need 1 <= B <= 65535 items (B = %d)", B);
    if (c->num_upsamples <= 0 || c->num_upsamples > 8 || c->num_kernels <= 0 || c->num_kernels > 4 || c->num_dilations <= 0 ||
        c->num_dilations > 4)
        return fail(F5_EINVAL, "f5_bigvgan_ragged_plan: unsupported dimensions");
    long up = 1;
    for (int i = 0; i < c->num_upsamples; ++i) {
        if (c->upsample_rates[i] <= 0) return fail(F5_EINVAL, "f5_bigvgan_ragged_plan: upsample rate %d is %d", i, c->upsample_rates[i]);
        up *= c->upsample_rates[i];
    }
    const int u0 = c->upsample_rates[0];
    const int gap = (bv_halo(*c) + u0 - 1) / u0, align = BV_TT / bv_gcd(BV_TT, u0);
    long at = 0;
    for (int b = 0; b < B; ++b) {
        if (frames_host[b] < 1) return fail(F5_EINVAL, "f5_bigvgan_ragged_plan: item %d has %d frame(s); need at least 1", b, frames_host[b]);
        row_start_out[b] = (int32_t)at;
        const long end = at + frames_host[b];
        if (end * up > (1L << 24))
            return fail(F5_EINVAL, "f5_bigvgan_ragged_plan: more than 2^24 packed rows at the last stage at item %d (the GEMMs index rows as int)", b);
        at = (end + gap + align - 1) / align * align;
        if (b == B - 1) row_start_out[B] = (int32_t)end;
    }
    *gap_frames_out = gap;
    return F5_OK;
}

// Item b = frames [starts[b], ends[b]) of batch row b of mel (element strides as f5_bigvgan_forward) -> wav[b * wav_stride ..]:
// T_b * prod(rates) samples, bit-identical to f5_bigvgan_forward on that slice alone, x gain[b] as a separate f32 multiply, then
// +0.0 up to wav_stride.  One pass over the packed axis of f5_bigvgan_ragged_plan.
extern "C" int f5_bigvgan_forward_ragged(f5_bigvgan* v, const float* mel, int32_t B, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                                         const int32_t* starts_host, const int32_t* ends_host, const float* gain_host, float* wav,
                                         int64_t wav_stride, f5_stream stream) {
    if (!v || !mel || !ends_host || !wav) return fail(F5_EINVAL, "f5_bigvgan_forward_ragged: null argument");
    if (!v->finalized) return fail(F5_ESTATE, "f5_bigvgan_finalize has not been called");
    if (B <= 0 || B > 65535) return fail(F5_EINVAL, "f5_bigvgan_forward_ragged: need 1 <= B <= 65535 items (B = %d)", B);
    const f5_bigvgan_config& c = v->cfg;
    std::vector<int32_t> host((size_t)2 * B + 1);
    int32_t *frames = host.data(), *rs = frames + B, gap = 0;
    long lmax = 0;
    for (int b = 0; b < B; ++b) {
        const int st = starts_host ? starts_host[b] : 0;
        const long Tb = (long)ends_host[b] - st;
        if (st < 0) return fail(F5_EINVAL, "f5_bigvgan_forward_ragged: item %d starts at frame %d < 0", b, st);
        if (Tb < 1 || Tb > (1L << 24))
            return fail(F5_EINVAL, "f5_bigvgan_forward_ragged: item %d has %ld frame(s) (frames [%d, %d)); need 1 .. 2^24", b, std::max(0L, Tb), st,
                        ends_host[b]);
        frames[b] = (int32_t)Tb;
        lmax = std::max(lmax, Tb * v->total_up);
    }
    if (wav_stride < lmax)
        return fail(F5_EINVAL, "f5_bigvgan_forward_ragged: wav_stride %lld is less than the longest waveform (%ld samples)",
                    (long long)wav_stride, lmax);
    if (f5_bigvgan_ragged_plan(&c, B, frames, rs, &gap) != F5_OK) return F5_EINVAL;   // (its message names the item)
    const long P = rs[B];   // packed frames
    hipStream_t s = (hipStream_t)stream;
    BvWork w;
    CHK(bv_workspace(v, P, true, BvTables::words(B), &w));
    // the segment table, the window starts, the frame counts and the gains go down through one pinned slot; the device copy is
    // read by this call's kernels only, which are ahead of the next call's copy on the stream
    CHK(v->stage.upload(w.tab, BvTables::words(B) * 4, s, [&](char* hb) {
        const BvTables h(hb, B);
        for (int b = 0; b < B; ++b) {
            h.row_start[b] = rs[b];
            h.mel_start[b] = starts_host ? starts_host[b] : 0;
            h.frames[b] = frames[b];
            h.gain[b] = gain_host ? gain_host[b] : 1.0f;
        }
        h.row_start[B] = rs[B];
    }));
    const BvTables d(w.tab, B);
    const BvSeg sg{d.row_start, d.frames, B};
    hipLaunchKernelGGL(bv_im2col7_ragged_kernel, dim3((unsigned)std::min(P, 16384L)), dim3(256), 0, s, mel, (long)stride_b, (long)stride_c,
                       (long)stride_t, d.mel_start, w.col, c.num_mels, (int)P, v->kpre, sg);
    KCHK();
    CHK(bv_generator(v, s, w, P, &sg));
    hipLaunchKernelGGL(bv_post_ragged_kernel, dim3(ew_blocks(wav_stride), B), dim3(256), 0, s, w.act, v->post_w, v->post_b, wav,
                       (long)wav_stride, v->c_last, c.use_tanh_at_final, sg, v->total_up, d.gain);
    KCHK();
    return F5_OK;
}
