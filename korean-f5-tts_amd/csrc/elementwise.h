// Bandwidth-bound kernels of the F5-TTS path (norms, packing, Euler/CFG update, text-encoder and Vocos glue).
// All of them stream rows with 16-byte accesses, one wave (64 lanes) per row where a row reduction is needed
// (wave shuffles only, no LDS), and keep statistics in fp32.
#pragma once
#include "e4m3.h"
#include "f5_common.h"

namespace f5 {

// The launch_* helpers below, each next to its kernel, are the launches of sample()'s step glue: engine_impl.h and the kernel-level
// entry points (kapi.hip f5k_*) both call them, so a test drives the grid and the arguments the engine uses.  They only enqueue; the
// caller reads hipGetLastError().

// blocks of a grid-stride launch over `total` work items: at most `cap`, the loop covers the rest
inline int ew_blocks(long total, int per_block = 256, int cap = 4096) {
    long b = (total + per_block - 1) / per_block;
    if (b < 1) b = 1;
    return (int)(b > cap ? cap : b);
}

// ------------------------------------------------------------------------------------------- LayerNorm
// out[r, :] = LN(x[r, :]; eps) * A + B with either
//   modulate: A = 1 + scale[b(r), :], B = shift[b(r), :]   (AdaLayerNorm, modules.py:314-320,335-341,680-693)
//   affine  : A = weight, B = bias                         (nn.LayerNorm(dim), modules.py:259; Vocos norms)
// One wave per row; D <= 2048, D % 4 == 0.  Two-pass statistics in registers (mean, then centred variance).
//
// Prefetch: up to two byte ranges (the weights of the GEMMs that follow) are read and discarded, spread over the grid,
// requested AFTER the row so that they never delay it.  The 370 MB of block weights do not fit the 256 MB Infinity
// Cache, so every GEMM of a step otherwise starts with HBM-latency misses on its W tiles; this launch is latency-bound
// and has the memory system to itself.
struct Prefetch { const char* p0 = nullptr; size_t n0 = 0; const char* p1 = nullptr; size_t n1 = 0; };
// Write-through form of a norm kernel's row store (f5_common.h "store policy"): lane -> columns 4 lane + 256 i, y[i] = the four results of
// chunk i (the lane -> column map of the statistics is untouched).  16-bit rows: lanes 2p and 2p + 1 exchange halves of two whole chunks
// i, i + 1 -- the even lane then holds 8 contiguous values of chunk i, the odd lane 8 of chunk i + 1 -- and store 16 bytes each; a
// chunk without a whole partner keeps its 8-byte pieces.  f32 rows are 16 bytes per lane already (pre-split rows: two 8-byte pieces).
template <typename TO>
__device__ __forceinline__ void store_row_wt(TO* out, size_t row_off, const float4 (&y)[8], int D, int lane, int planar) {
    if constexpr (sizeof(TO) == 2) {
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            const u32x2 a = pack4<TO>(y[i].x, y[i].y, y[i].z, y[i].w), b = pack4<TO>(y[i + 1].x, y[i + 1].y, y[i + 1].z, y[i + 1].w);
            if ((i + 2) * 256 <= D) {   // (wave-uniform: every lane takes part in the exchange)
                const bool odd = lane & 1;
                const u32x2 send = odd ? a : b;
                const u32x2 recv = {(unsigned)__shfl_xor((int)send[0], 1, 64), (unsigned)__shfl_xor((int)send[1], 1, 64)};
                const u32x4 d = odd ? u32x4{recv[0], recv[1], b[0], b[1]} : u32x4{a[0], a[1], recv[0], recv[1]};
                store16_wt(out, (row_off + (i + (odd ? 1 : 0)) * 256 + (lane >> 1) * 8) * 2, d);
            } else {
                if (lane * 4 + i * 256 < D) store8_wt(out + row_off + lane * 4 + i * 256, a);
                if (lane * 4 + (i + 1) * 256 < D) store8_wt(out + row_off + lane * 4 + (i + 1) * 256, b);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (lane * 4 + i * 256 < D) store4_at_wt(out, row_off, lane * 4 + i * 256, planar, y[i].x, y[i].y, y[i].z, y[i].w);
    }
}
// The body of the two LayerNorm kernels below.  ROWS: row r's vectors are those of batch row rowmap[r].x (a packed batch whose batch rows
// have their own vectors), not of r / rows_per_batch.
template <typename TO, bool ROWS>
__device__ __forceinline__ void layernorm_body(const float* __restrict__ x, int ldx, TO* __restrict__ out, int ldo, int R, int D, float eps,
                                               const float* __restrict__ A, const float* __restrict__ Bv, int vec_stride,
                                               int rows_per_batch, int modulate, const Prefetch& pf, const int* __restrict__ m_limit,
                                               int planar, int wt, const int2* __restrict__ rowmap,
                                               unsigned char* __restrict__ scales = nullptr) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R || (m_limit && r >= *m_limit)) return;   // (m_limit: rows present in a packed batch, RowPack)
    const float* xr = x + (size_t)r * ldx;
    float4 v[8], ga[8], gb[8];
    // the modulation / affine vectors do not depend on the statistics: request them together with the row so that the
    // kernel is ONE memory round trip deep, not two
    size_t vb;
    if constexpr (ROWS) vb = (size_t)rowmap[r].x * vec_stride;   // (r < *m_limit: a row fill_rowmap_kernel has written)
    else vb = (size_t)(rows_per_batch > 0 ? r / rows_per_batch : 0) * vec_stride;
    const float a0 = modulate ? 0.f : 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
        ga[i] = (A && c < D) ? *reinterpret_cast<const float4*>(A + vb + c) : make_float4(a0, a0, a0, a0);
        gb[i] = (Bv && c < D) ? *reinterpret_cast<const float4*>(Bv + vb + c) : make_float4(0, 0, 0, 0);
    }
    u32x4 pfv[8] = {};
    if (pf.n0 | pf.n1) {
        const size_t gtid = (size_t)blockIdx.x * 256 + threadIdx.x, gsz = (size_t)gridDim.x * 256;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t off = (gtid + (size_t)(i & 3) * gsz) * 16;   // four 16-byte chunks per thread and range
            const char* base = i < 4 ? pf.p0 : pf.p1;
            const size_t n = i < 4 ? pf.n0 : pf.n1;
            if (off + 16 <= n) pfv[i] = *reinterpret_cast<const u32x4*>(base + off);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < D) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    if constexpr (sizeof(TO) == 1) {   // e4m3 codes + one power-of-two scale per row (quant8.h): the same f32 expressions, quantised
        float4 y[8];
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float4 a = ga[i];
            const float4 b = gb[i];
            if (modulate) { a.x += 1.f; a.y += 1.f; a.z += 1.f; a.w += 1.f; }
            y[i] = make_float4((v[i].x - mean) * rstd * a.x + b.x, (v[i].y - mean) * rstd * a.y + b.y, (v[i].z - mean) * rstd * a.z + b.z,
                               (v[i].w - mean) * rstd * a.w + b.w);
            if (lane * 4 + i * 256 < D) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(y[i].x), fabsf(y[i].y))), fmaxf(fabsf(y[i].z), fabsf(y[i].w)));
        }
        const unsigned sb = e8m0_for_amax(wave_max(amax));
        const float inv = e8m0_inverse(sb);
        unsigned* cr = reinterpret_cast<unsigned*>(out + (size_t)r * ldo);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (lane * 4 + i * 256 < D) cr[lane + i * 64] = e4m3_pack4(y[i].x, y[i].y, y[i].z, y[i].w, inv);
        if (lane == 0) scales[r] = (unsigned char)sb;
    } else if (wt) {   // write-through stores: the same expressions, stored by store_row_wt
        float4 y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float4 a = ga[i];
            const float4 b = gb[i];
            if (modulate) { a.x += 1.f; a.y += 1.f; a.z += 1.f; a.w += 1.f; }
            y[i] = make_float4((v[i].x - mean) * rstd * a.x + b.x, (v[i].y - mean) * rstd * a.y + b.y, (v[i].z - mean) * rstd * a.z + b.z,
                               (v[i].w - mean) * rstd * a.w + b.w);
        }
        store_row_wt(out, (size_t)r * ldo, y, D, lane, planar);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < D) {
                float4 a = ga[i];
                const float4 b = gb[i];
                if (modulate) { a.x += 1.f; a.y += 1.f; a.z += 1.f; a.w += 1.f; }
                store4_at(out + (size_t)r * ldo, c, planar, (v[i].x - mean) * rstd * a.x + b.x, (v[i].y - mean) * rstd * a.y + b.y,
                          (v[i].z - mean) * rstd * a.z + b.z, (v[i].w - mean) * rstd * a.w + b.w);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" ::"v"(pfv[i]));   // keep the prefetch loads; nothing uses their data
}
template <typename TO>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int ldx, TO* __restrict__ out,
                                                        int ldo, int R, int D, float eps, const float* __restrict__ A,
                                                        const float* __restrict__ Bv, int vec_stride,
                                                        int rows_per_batch, int modulate, Prefetch pf,
                                                        const int* __restrict__ m_limit = nullptr, int planar = 0, int wt = 0) {
    layernorm_body<TO, false>(x, ldx, out, ldo, R, D, eps, A, Bv, vec_stride, rows_per_batch, modulate, pf, m_limit, planar, wt, nullptr);
}
// ... of a per-item call on packed rows (every batch row has its own AdaLN vectors): a kernel of its own, so that the one every other
// forward launches keeps its arguments and its code
template <typename TO>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* __restrict__ x, int ldx, TO* __restrict__ out, int ldo, int R,
                                                             int D, float eps, const float* __restrict__ A, const float* __restrict__ Bv,
                                                             int vec_stride, Prefetch pf, const int* __restrict__ m_limit,
                                                             const int2* __restrict__ rowmap, int planar, int wt) {
    layernorm_body<TO, true>(x, ldx, out, ldo, R, D, eps, A, Bv, vec_stride, 0, 1, pf, m_limit, planar, wt, rowmap);
}
// One AdaLN LayerNorm launch, out = LN(x) (1 + scale) + shift over R dense rows of D: what every output form of it is given.  Batch row
// b's vectors are at scale / shift + b * vec_stride (0: shared); row r belongs to batch row r / rows_per_batch, or -- rowmap: a packed
// batch whose batch rows have their own vectors -- to rowmap[r].x.  pf: weights to prefetch; m_limit: the device row count of a packed batch.
struct AdaLN {
    const float *x, *scale, *shift;
    int R, D, vec_stride, rows_per_batch;
    float eps = 1e-6f;
    const int2* rowmap = nullptr;
    Prefetch pf{};
    const int* m_limit = nullptr;
};
// ... into rows of TO (planar: pre-split f32 rows; wt: write-through stores).  The e4m3 form is quant8.h's overload.
template <typename TO> inline void launch_adaln_norm(hipStream_t s, const AdaLN& a, TO* out, int planar, int wt) {
    const dim3 grid((a.R + 3) / 4), block(256);
    if (a.rowmap)
        hipLaunchKernelGGL((layernorm_rows_kernel<TO>), grid, block, 0, s, a.x, a.D, out, a.D, a.R, a.D, a.eps, a.scale, a.shift, a.vec_stride, a.pf,
                           a.m_limit, a.rowmap, planar, wt);
    else
        hipLaunchKernelGGL((layernorm_kernel<TO>), grid, block, 0, s, a.x, a.D, out, a.D, a.R, a.D, a.eps, a.scale, a.shift, a.vec_stride,
                           a.rows_per_batch, 1, a.pf, a.m_limit, planar, wt);
}

// x_transformers.RMSNorm as used by UNetT (unett.py:154,168,185): F.normalize(x, dim=-1) * sqrt(D) * g
template <typename TO>
__global__ __launch_bounds__(256) void xrmsnorm_kernel(const float* __restrict__ x, int ldx, TO* __restrict__ out, int ldo,
                                                       int R, int D, const float* __restrict__ gvec, int planar = 0, int wt = 0) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* xr = x + (size_t)r * ldx;
    float4 v[8];
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = c < D ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0, 0, 0, 0);
        q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float nrm = fmaxf(sqrtf(wave_sum(q)), 1e-12f);
    const float sc = sqrtf((float)D) / nrm;
    if (wt) {   // write-through stores: the same expressions, stored by store_row_wt
        float4 y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = lane * 4 + i * 256;
            const float4 gg = c < D ? *reinterpret_cast<const float4*>(gvec + c) : make_float4(0, 0, 0, 0);
            y[i] = make_float4(v[i].x * sc * gg.x, v[i].y * sc * gg.y, v[i].z * sc * gg.z, v[i].w * sc * gg.w);
        }
        store_row_wt(out, (size_t)r * ldo, y, D, lane, planar);
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < D) {
            const float4 gg = *reinterpret_cast<const float4*>(gvec + c);
            store4_at(out + (size_t)r * ldo, c, planar, v[i].x * sc * gg.x, v[i].y * sc * gg.y, v[i].z * sc * gg.z, v[i].w * sc * gg.w);
        }
    }
}
// wt: write-through stores asked for (applied where the output is small enough for their 32-bit offsets)
inline int wt_fits(int wt, size_t bytes) { return wt && bytes < F5_WT_MAX_BYTES ? 1 : 0; }
template <typename TO>
inline void launch_xrmsnorm(hipStream_t s, const float* x, TO* out, int rows, int D, const float* g, int planar, int wt = 0) {
    hipLaunchKernelGGL((xrmsnorm_kernel<TO>), dim3((rows + 3) / 4), dim3(256), 0, s, x, D, out, D, rows, D, g, planar,
                       wt_fits(wt, (size_t)rows * D * sizeof(TO)));
}

// --------------------------------------------------------------------------------- input-embedding operand
// A[b', n, :] = [ x[b, n, :mel] | cond[b, n, :mel] (0 for the uncond half / drop_audio_cond) | text[b', n, :Dt] ]
// (dit.py:135-138, cfg_infer packing dit.py:296-305).  b' in [0, Bp); rows b' >= B are the uncond half.
// rowmap (RowPack, may be null): output row r is (b', n) = rowmap[r] for r < *row_limit instead of r = b' N + n; rows
// whose position lies past the sample's own length (the <= 3 alignment rows of a packed utterance) are written as zero.
template <typename T>
__global__ void pack_input_kernel(const float* __restrict__ x, const float* __restrict__ cond,
                                  const float* __restrict__ text_c, const float* __restrict__ text_u,
                                  T* __restrict__ out, int ldo, int B, int Bp, int N, int mel, int Dt, int drop_cond_first,
                                  const int2* __restrict__ rowmap = nullptr, const int* __restrict__ row_limit = nullptr,
                                  const int* __restrict__ lens = nullptr) {
    const int K4 = (2 * mel + Dt) / 4;
    const long total = (rowmap ? (long)*row_limit : (long)Bp * N) * K4;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % K4) * 4;
        const long row = idx / K4;
        int n = (int)(row % N), bp = (int)(row / N);
        if (rowmap) { const int2 m = rowmap[row]; bp = m.x; n = m.y; }
        const bool un = bp >= B;
        const int b = un ? bp - B : bp;
        float4 v;
        if (rowmap && n >= lens[b]) v = make_float4(0, 0, 0, 0);
        else if (c < mel) v = *reinterpret_cast<const float4*>(x + ((size_t)b * N + n) * mel + c);
        else if (c < 2 * mel)
            v = (un || drop_cond_first) ? make_float4(0, 0, 0, 0)
                                        : *reinterpret_cast<const float4*>(cond + ((size_t)b * N + n) * mel + (c - mel));
        else
            v = *reinterpret_cast<const float4*>((un ? text_u : text_c) + ((size_t)b * N + n) * Dt + (c - 2 * mel));
        store4(out + (size_t)row * ldo + c, v.x, v.y, v.z, v.w);
    }
}
// (the grid is that of the padded batch, Bp * N rows, also when a rowmap packs them)
template <typename T>
inline void launch_pack_input(hipStream_t s, const float* x, const float* cond, const float* text_c, const float* text_u, T* out, int ldo, int B,
                              int Bp, int N, int mel, int Dt, int drop_cond_first, const int2* rowmap, const int* row_limit, const int* lens) {
    const int rows = Bp * N, kin = 2 * mel + Dt;
    hipLaunchKernelGGL((pack_input_kernel<T>), dim3(ew_blocks((long)rows * kin / 4)), dim3(256), 0, s, x, cond, text_c, text_u, out, ldo, B, Bp,
                       N, mel, Dt, drop_cond_first, rowmap, row_limit, lens);
}

// ------------------------------------------------------------------------------------------ UNetT glue
// x[b', 0, :] = t_emb[b' or shared]; x[b', 1 + n, :] = h[b', n, :]      (unett.py:244: cat([t[:, None], x], dim=1))
static __global__ void unett_assemble_kernel(const float* __restrict__ h, const float* __restrict__ temb, int temb_stride,
                                             float* __restrict__ x, int Bp, int N, int D) {
    const int d4 = D / 4;
    const long total = (long)Bp * (N + 1) * d4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4);
        const long row = i / d4;
        const int n = (int)(row % (N + 1)), b = (int)(row / (N + 1));
        const float4 v = n == 0 ? reinterpret_cast<const float4*>(temb + (size_t)b * temb_stride)[c]
                                : reinterpret_cast<const float4*>(h + ((size_t)b * N + (n - 1)) * D)[c];
        reinterpret_cast<float4*>(x)[i] = v;
    }
}
inline void launch_unett_assemble(hipStream_t s, const float* h, const float* temb, int temb_stride, float* x, int Bp, int N, int D) {
    const int rows = Bp * (N + 1);
    hipLaunchKernelGGL(unett_assemble_kernel, dim3(ew_blocks((long)rows * D / 4)), dim3(256), 0, s, h, temb, temb_stride, x, Bp, N, D);
}
// out[r, :] = [x[r, :] | skip[r, :]] converted to T   (unett.py:266: cat((x, skip), dim=-1))
// planar (T = float, F5_PREC_F16X3): the row is written pre-split (store4_planar) -- the A operand of an AWSplit GEMM (GemmOperands, ring or ping-pong)
template <typename T>
__global__ void cat2_kernel(const float* __restrict__ x, const float* __restrict__ skip, T* __restrict__ out, long rows, int D, int planar = 0) {
    const int d4 = D / 4;
    const long total = rows * 2 * d4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % (2 * d4));
        const long r = i / (2 * d4);
        const float4 v = c < d4 ? reinterpret_cast<const float4*>(x + r * D)[c]
                                : reinterpret_cast<const float4*>(skip + r * D)[c - d4];
        store4_at(out + r * 2 * D, c * 4, planar, v.x, v.y, v.z, v.w);
    }
}
template <typename T> inline void launch_cat2(hipStream_t s, const float* x, const float* skip, T* out, int rows, int D, int planar) {
    hipLaunchKernelGGL((cat2_kernel<T>), dim3(ew_blocks((long)rows * 2 * D / 4)), dim3(256), 0, s, x, skip, out, (long)rows, D, planar);
}
// pred[b', n, :] = pred_all[b', 1 + n, :]     (unett.py:278: norm_out(x)[:, 1:, :])
static __global__ void strip_first_token_kernel(const float* __restrict__ in, float* __restrict__ out, int Bp, int N, int C) {
    const int c4 = C / 4;
    const long total = (long)Bp * N * c4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4);
        const long row = i / c4;
        const int n = (int)(row % N), b = (int)(row / N);
        reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(in + ((size_t)b * (N + 1) + n + 1) * C)[c];
    }
}
inline void launch_strip_first_token(hipStream_t s, const float* in, float* out, int Bp, int N, int C) {
    const int rows_in = Bp * N;
    hipLaunchKernelGGL(strip_first_token_kernel, dim3(ew_blocks((long)rows_in * C / 4)), dim3(256), 0, s, in, out, Bp, N, C);
}

// ------------------------------------------------------------------------------------- CFG + Euler update
// y += dt * (p + (p - u) * cfg)   (cfm.py:190-191 + fixed-grid Euler, f5_tts_trtllm.py:360-369); also emits the new
// state into the trajectory slot.  pred holds [cond half ; uncond half] when cfg is on.
static __global__ void euler_cfg_kernel(float* __restrict__ y, const float* __restrict__ pred, long half_elems,
                                        const float* __restrict__ tgrid, int step, float cfg, int use_cfg,
                                        float* __restrict__ traj_slot) {
    const float dt = tgrid[step + 1] - tgrid[step];   // f32 subtraction, as torch does on the f32 grid (cfm.py:211-218)
    const long n4 = half_elems / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 yy = reinterpret_cast<float4*>(y)[i];
        const float4 p = reinterpret_cast<const float4*>(pred)[i];
        float4 v = p;
        if (use_cfg) {
            const float4 u = reinterpret_cast<const float4*>(pred + half_elems)[i];
            v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
            v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
        }
        yy.x += dt * v.x; yy.y += dt * v.y; yy.z += dt * v.z; yy.w += dt * v.w;
        reinterpret_cast<float4*>(y)[i] = yy;
        if (traj_slot) reinterpret_cast<float4*>(traj_slot)[i] = yy;
    }
}

// The same update when the backbone ran on PACKED rows (RowPack): pred[r, :] with r = row_start[b'] + n for n < lens[b];
// frames past a sample's own length keep their value (they influence nothing when attn_mask_enabled, and are not computed).
static __global__ void euler_cfg_packed_kernel(float* __restrict__ y, const float* __restrict__ pred, int B, int N, int mel,
                                               const int* __restrict__ row_start, const int* __restrict__ lens,
                                               const float* __restrict__ tgrid, int step, float cfg, int use_cfg,
                                               float* __restrict__ traj_slot) {
    const float dt = tgrid[step + 1] - tgrid[step];
    const int c4n = mel / 4;
    const long total = (long)B * N * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n);
        const long fr = i / c4n;
        const int n = (int)(fr % N), b = (int)(fr / N);
        float4 yy = reinterpret_cast<float4*>(y)[i];
        if (n < lens[b]) {
            const float4 p = reinterpret_cast<const float4*>(pred + ((size_t)row_start[b] + n) * mel)[c];
            float4 v = p;
            if (use_cfg) {
                const float4 u = reinterpret_cast<const float4*>(pred + ((size_t)row_start[B + b] + n) * mel)[c];
                v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
                v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
            }
            yy.x += dt * v.x; yy.y += dt * v.y; yy.z += dt * v.z; yy.w += dt * v.w;
            reinterpret_cast<float4*>(y)[i] = yy;
        }
        if (traj_slot) reinterpret_cast<float4*>(traj_slot)[i] = yy;
    }
}
// ------------------------------------------------------------------------------------- CFG + midpoint half step
// y_mid = y + (p + (p - u) * cfg) * (dt / 2)   (torchdiffeq Midpoint._step_func: f0 at (t[i], y), y_mid = y + f0 * half_dt).
// The full step is euler_cfg(_packed)_kernel on the prediction made at y_mid: y += dt * f(t[i] + dt / 2, y_mid).
static __global__ void midpoint_half_cfg_kernel(const float* __restrict__ y, const float* __restrict__ pred, long half_elems,
                                                const float* __restrict__ tgrid, int step, float cfg, int use_cfg,
                                                float* __restrict__ y_mid) {
    const float hdt = 0.5f * (tgrid[step + 1] - tgrid[step]);   // f32, in torchdiffeq's order
    const long n4 = half_elems / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 yy = reinterpret_cast<const float4*>(y)[i];
        const float4 p = reinterpret_cast<const float4*>(pred)[i];
        float4 v = p;
        if (use_cfg) {
            const float4 u = reinterpret_cast<const float4*>(pred + half_elems)[i];
            v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
            v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
        }
        yy.x += v.x * hdt; yy.y += v.y * hdt; yy.z += v.z * hdt; yy.w += v.w * hdt;
        reinterpret_cast<float4*>(y_mid)[i] = yy;
    }
}
// RowPack twin (pred on packed rows, as euler_cfg_packed_kernel reads it); frames past a sample's length get y_mid = y
static __global__ void midpoint_half_cfg_packed_kernel(const float* __restrict__ y, const float* __restrict__ pred, int B, int N,
                                                       int mel, const int* __restrict__ row_start, const int* __restrict__ lens,
                                                       const float* __restrict__ tgrid, int step, float cfg, int use_cfg,
                                                       float* __restrict__ y_mid) {
    const float hdt = 0.5f * (tgrid[step + 1] - tgrid[step]);
    const int c4n = mel / 4;
    const long total = (long)B * N * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n);
        const long fr = i / c4n;
        const int n = (int)(fr % N), b = (int)(fr / N);
        float4 yy = reinterpret_cast<const float4*>(y)[i];
        if (n < lens[b]) {
            const float4 p = reinterpret_cast<const float4*>(pred + ((size_t)row_start[b] + n) * mel)[c];
            float4 v = p;
            if (use_cfg) {
                const float4 u = reinterpret_cast<const float4*>(pred + ((size_t)row_start[B + b] + n) * mel)[c];
                v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
                v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
            }
            yy.x += v.x * hdt; yy.y += v.y * hdt; yy.z += v.z * hdt; yy.w += v.w * hdt;
        }
        reinterpret_cast<float4*>(y_mid)[i] = yy;
    }
}
// One ODE update of B utterances as sample_body launches it: the packed form when the backbone ran on packed rows (row_start non-null).
// y += dt * v into y and the trajectory slot (may be null) ...
inline void launch_euler_cfg(hipStream_t s, float* y, const float* pred, int B, int N, int mel, const int* row_start, const int* lens,
                             const float* tgrid, int step, float cfg, int use_cfg, float* traj_slot) {
    const long n = (long)B * N * mel;
    if (row_start)
        hipLaunchKernelGGL(euler_cfg_packed_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, s, y, pred, B, N, mel, row_start, lens, tgrid, step,
                           cfg, use_cfg, traj_slot);
    else
        hipLaunchKernelGGL(euler_cfg_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, s, y, pred, n, tgrid, step, cfg, use_cfg, traj_slot);
}
// ... and y_mid = y + v * dt / 2
inline void launch_midpoint_half_cfg(hipStream_t s, const float* y, const float* pred, int B, int N, int mel, const int* row_start,
                                     const int* lens, const float* tgrid, int step, float cfg, int use_cfg, float* y_mid) {
    const long n = (long)B * N * mel;
    if (row_start)
        hipLaunchKernelGGL(midpoint_half_cfg_packed_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, s, y, pred, B, N, mel, row_start, lens, tgrid,
                           step, cfg, use_cfg, y_mid);
    else
        hipLaunchKernelGGL(midpoint_half_cfg_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, s, y, pred, n, tgrid, step, cfg, use_cfg, y_mid);
}

// ------------------------------------------------------------------------------------- per-item sampler settings
// f5_sample_items: every utterance b of the (rectangular) batch has its own grid t_items[b * (steps_max + 1) + 0 .. steps[b]], its own
// guidance cfg_items[b] and its own step count.  The two updates above with b = frame / N; an utterance that has finished
// (step >= steps[b]) is not touched -- no multiplication by a zero dt -- and the trajectory slot receives its final state.
// An utterance with cfg_items[b] < 1e-5 takes v = p (cfm.py:167-178) although the batch ran both halves.
static __global__ void euler_cfg_items_kernel(float* __restrict__ y, const float* __restrict__ pred, int B, int N, int mel,
                                              const float* __restrict__ t_items, const float* __restrict__ cfg_items,
                                              const int* __restrict__ steps_items, int steps_max, int step, int use_cfg,
                                              float* __restrict__ traj_slot) {
    const int c4n = mel / 4;
    const long total = (long)B * N * c4n, half_elems = (long)B * N * mel;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / c4n / N);
        float4 yy = reinterpret_cast<float4*>(y)[i];
        if (step < steps_items[b]) {
            const float* tg = t_items + (size_t)b * (steps_max + 1);
            const float dt = tg[step + 1] - tg[step];
            const float cfg = cfg_items[b];
            const float4 p = reinterpret_cast<const float4*>(pred)[i];
            float4 v = p;
            if (use_cfg && !(cfg < 1e-5f)) {
                const float4 u = reinterpret_cast<const float4*>(pred + half_elems)[i];
                v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
                v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
            }
            yy.x += dt * v.x; yy.y += dt * v.y; yy.z += dt * v.z; yy.w += dt * v.w;
            reinterpret_cast<float4*>(y)[i] = yy;
        }
        if (traj_slot) reinterpret_cast<float4*>(traj_slot)[i] = yy;
    }
}
// ... and the midpoint half step; a finished utterance gets y_mid = y (nothing reads it)
static __global__ void midpoint_half_cfg_items_kernel(const float* __restrict__ y, const float* __restrict__ pred, int B, int N, int mel,
                                                      const float* __restrict__ t_items, const float* __restrict__ cfg_items,
                                                      const int* __restrict__ steps_items, int steps_max, int step, int use_cfg,
                                                      float* __restrict__ y_mid) {
    const int c4n = mel / 4;
    const long total = (long)B * N * c4n, half_elems = (long)B * N * mel;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / c4n / N);
        float4 yy = reinterpret_cast<const float4*>(y)[i];
        if (step < steps_items[b]) {
            const float* tg = t_items + (size_t)b * (steps_max + 1);
            const float hdt = 0.5f * (tg[step + 1] - tg[step]);
            const float cfg = cfg_items[b];
            const float4 p = reinterpret_cast<const float4*>(pred)[i];
            float4 v = p;
            if (use_cfg && !(cfg < 1e-5f)) {
                const float4 u = reinterpret_cast<const float4*>(pred + half_elems)[i];
                v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
                v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
            }
            yy.x += v.x * hdt; yy.y += v.y * hdt; yy.z += v.z * hdt; yy.w += v.w * hdt;
        }
        reinterpret_cast<float4*>(y_mid)[i] = yy;
    }
}
// The per-item updates when the backbone ran on PACKED rows (an isolated per-item call, f5_set_isolated_rows): the index shape of
// euler_cfg_packed_kernel -- pred[r, :] with r = row_start[b] + n, the unconditional half at row_start[B + b] + n, only n < lens[b] --
// and the per-item part of euler_cfg_items_kernel.  A finished item and the frames past an item's own length are not written; the
// trajectory slot receives y as it stands.
static __global__ void euler_cfg_items_packed_kernel(float* __restrict__ y, const float* __restrict__ pred, int B, int N, int mel,
                                                     const int* __restrict__ row_start, const int* __restrict__ lens,
                                                     const float* __restrict__ t_items, const float* __restrict__ cfg_items,
                                                     const int* __restrict__ steps_items, int steps_max, int step, int use_cfg,
                                                     float* __restrict__ traj_slot) {
    const int c4n = mel / 4;
    const long total = (long)B * N * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n);
        const long fr = i / c4n;
        const int n = (int)(fr % N), b = (int)(fr / N);
        float4 yy = reinterpret_cast<float4*>(y)[i];
        if (step < steps_items[b] && n < lens[b]) {
            const float* tg = t_items + (size_t)b * (steps_max + 1);
            const float dt = tg[step + 1] - tg[step];
            const float cfg = cfg_items[b];
            const float4 p = reinterpret_cast<const float4*>(pred + ((size_t)row_start[b] + n) * mel)[c];
            float4 v = p;
            if (use_cfg && !(cfg < 1e-5f)) {
                const float4 u = reinterpret_cast<const float4*>(pred + ((size_t)row_start[B + b] + n) * mel)[c];
                v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
                v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
            }
            yy.x += dt * v.x; yy.y += dt * v.y; yy.z += dt * v.z; yy.w += dt * v.w;
            reinterpret_cast<float4*>(y)[i] = yy;
        }
        if (traj_slot) reinterpret_cast<float4*>(traj_slot)[i] = yy;
    }
}
// ... and the midpoint half step; a finished item and the frames past an item's length get y_mid = y
static __global__ void midpoint_half_cfg_items_packed_kernel(const float* __restrict__ y, const float* __restrict__ pred, int B, int N,
                                                             int mel, const int* __restrict__ row_start, const int* __restrict__ lens,
                                                             const float* __restrict__ t_items, const float* __restrict__ cfg_items,
                                                             const int* __restrict__ steps_items, int steps_max, int step, int use_cfg,
                                                             float* __restrict__ y_mid) {
    const int c4n = mel / 4;
    const long total = (long)B * N * c4n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n);
        const long fr = i / c4n;
        const int n = (int)(fr % N), b = (int)(fr / N);
        float4 yy = reinterpret_cast<const float4*>(y)[i];
        if (step < steps_items[b] && n < lens[b]) {
            const float* tg = t_items + (size_t)b * (steps_max + 1);
            const float hdt = 0.5f * (tg[step + 1] - tg[step]);
            const float cfg = cfg_items[b];
            const float4 p = reinterpret_cast<const float4*>(pred + ((size_t)row_start[b] + n) * mel)[c];
            float4 v = p;
            if (use_cfg && !(cfg < 1e-5f)) {
                const float4 u = reinterpret_cast<const float4*>(pred + ((size_t)row_start[B + b] + n) * mel)[c];
                v.x = p.x + (p.x - u.x) * cfg; v.y = p.y + (p.y - u.y) * cfg;
                v.z = p.z + (p.z - u.z) * cfg; v.w = p.w + (p.w - u.w) * cfg;
            }
            yy.x += v.x * hdt; yy.y += v.y * hdt; yy.z += v.z * hdt; yy.w += v.w * hdt;
        }
        reinterpret_cast<float4*>(y_mid)[i] = yy;
    }
}
// One per-item ODE update of a chunk of B utterances as sample_body launches it: the packed form when the backbone ran on packed rows
// (row_start non-null; lens comes with it).  The tables start at the chunk's first utterance (t_items, cfg_items, steps_items already offset).
inline void launch_euler_cfg_items(hipStream_t s, float* y, const float* pred, int B, int N, int mel, const int* row_start, const int* lens,
                                   const float* t_items, const float* cfg_items, const int* steps_items, int steps_max, int step, int use_cfg,
                                   float* traj_slot) {
    const dim3 grid(ew_blocks((long)B * N * mel / 4));
    if (row_start)
        hipLaunchKernelGGL(euler_cfg_items_packed_kernel, grid, dim3(256), 0, s, y, pred, B, N, mel, row_start, lens, t_items, cfg_items,
                           steps_items, steps_max, step, use_cfg, traj_slot);
    else
        hipLaunchKernelGGL(euler_cfg_items_kernel, grid, dim3(256), 0, s, y, pred, B, N, mel, t_items, cfg_items, steps_items, steps_max, step,
                           use_cfg, traj_slot);
}
inline void launch_midpoint_half_cfg_items(hipStream_t s, const float* y, const float* pred, int B, int N, int mel, const int* row_start,
                                           const int* lens, const float* t_items, const float* cfg_items, const int* steps_items,
                                           int steps_max, int step, int use_cfg, float* y_mid) {
    const dim3 grid(ew_blocks((long)B * N * mel / 4));
    if (row_start)
        hipLaunchKernelGGL(midpoint_half_cfg_items_packed_kernel, grid, dim3(256), 0, s, y, pred, B, N, mel, row_start, lens, t_items,
                           cfg_items, steps_items, steps_max, step, use_cfg, y_mid);
    else
        hipLaunchKernelGGL(midpoint_half_cfg_items_kernel, grid, dim3(256), 0, s, y, pred, B, N, mel, t_items, cfg_items, steps_items,
                           steps_max, step, use_cfg, y_mid);
}
// dst[r, :] = src[idx[r % nidx], :] for r < rows: the time rows (AdaLN vectors, or the UNetT's time embedding) of one evaluation, one per
// batch row of a chunk -- nidx utterances, the conditional half and then (rows = 2 nidx) the unconditional half.  width % 4 == 0.
static __global__ void mod_gather_kernel(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ dst, int rows,
                                         int nidx, int width) {
    const int w4 = width / 4;
    const long total = (long)rows * w4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int r = (int)(i / w4), c = (int)(i % w4);
        reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src + (size_t)idx[r % nidx] * width)[c];
    }
}
inline void launch_mod_gather(hipStream_t s, const float* src, const int* idx, float* dst, int rows, int nidx, int width) {
    hipLaunchKernelGGL(mod_gather_kernel, dim3(ew_blocks((long)rows * width / 4)), dim3(256), 0, s, src, idx, dst, rows, nidx, width);
}

// f5_sample_span: the start state of a slice.  y[b, n, :] for b < B, n < N is prev[rows[b], n, :] where rows[b] >= 0 and n < prev_N, +0.0
// where rows[b] >= 0 and n >= prev_N (a frame the previous batch did not have), and y_new[b, n, :] where rows[b] == -1.  One float4
// per lane, consecutive lanes on consecutive addresses of y and, inside a row, of the source; mel % 4 == 0.  prev / y_new may be null
// when no row reads them.
// pitch >= N: the frames between two rows of y (a length bucket stages rows of N frames at the bucket's ceiling; the frames N .. pitch-1
// of a row are not written here).  prev and y_new keep their own pitches, prev_N and N.
static __global__ void span_stage_kernel(float* __restrict__ y, const float* __restrict__ prev, const float* __restrict__ y_new,
                                         const int* __restrict__ rows, int B, int N, int prev_N, int mel, int pitch) {
    const int c4n = mel / 4;
    const long per_row = (long)N * c4n, total = (long)B * per_row, keep = (long)(prev_N < N ? prev_N : N) * c4n;
    const long skip = (long)(pitch - N) * c4n;   // float4s between the end of a row and the start of the next
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per_row);
        const long j = i - (long)b * per_row;   // float4 index inside the row: n * c4n + c
        const int r = rows[b];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < 0) v = reinterpret_cast<const float4*>(y_new)[i];
        else if (j < keep) v = reinterpret_cast<const float4*>(prev)[(long)r * prev_N * c4n + j];
        reinterpret_cast<float4*>(y)[i + (long)b * skip] = v;
    }
}
inline void launch_span_stage(hipStream_t s, float* y, const float* prev, const float* y_new, const int* rows, int B, int N, int prev_N,
                              int mel, int pitch) {
    hipLaunchKernelGGL(span_stage_kernel, dim3(ew_blocks((long)B * N * mel / 4)), dim3(256), 0, s, y, prev, y_new, rows, B, N, prev_N, mel,
                       pitch);
}

// rowmap[row_start[b'] + n] = (b', n) for n < row_start[b' + 1] - row_start[b']   (one block per batch row)
static __global__ void fill_rowmap_kernel(const int* __restrict__ row_start, int2* __restrict__ rowmap) {
    const int bp = blockIdx.x, r0 = row_start[bp], cnt = row_start[bp + 1] - r0;
    for (int n = threadIdx.x; n < cnt; n += blockDim.x) rowmap[r0 + n] = make_int2(bp, n);
}
inline void launch_fill_rowmap(hipStream_t s, const int* row_start, int2* rowmap, int Bp) {
    hipLaunchKernelGGL(fill_rowmap_kernel, dim3(Bp), dim3(256), 0, s, row_start, rowmap);
}

// out = where(mask, a, b) row-wise: cfm.py:151-153 (step_cond) and :221-223 (final out)
static __global__ void select_rows_kernel(const float* a, const float* bsrc, const unsigned char* __restrict__ rowmask,
                                   float* out, long rows, int C) {  // out may alias bsrc (in-place select)
    const int c4 = C / 4;
    const long total = rows * c4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / c4;
        const float* src = rowmask[r] ? a : bsrc;
        float4 v = make_float4(0, 0, 0, 0);
        if (src) v = reinterpret_cast<const float4*>(src)[i];
        reinterpret_cast<float4*>(out)[i] = v;
    }
}
inline void launch_select_rows(hipStream_t s, const float* a, const float* b, const unsigned char* rowmask, float* out, long rows, int C) {
    hipLaunchKernelGGL(select_rows_kernel, dim3(ew_blocks(rows * C / 4)), dim3(256), 0, s, a, b, rowmask, out, rows, C);
}

// ------------------------------------------------------------------------------------ time-step features
// feat[s, j] = sin(arg), feat[s, 128 + j] = cos(arg), arg = (1000 * t[s]) * freq[j]   (modules.py:157-164)
static __global__ void time_sinus_kernel(const float* __restrict__ t, const float* __restrict__ freq, float* __restrict__ feat,
                                  int S, int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * half) return;
    const int s = i / half, j = i - s * half;
    const float arg = (1000.0f * t[s]) * freq[j];
    feat[(size_t)s * 2 * half + j] = sinf(arg);
    feat[(size_t)s * 2 * half + half + j] = cosf(arg);
}
inline void launch_time_sinus(hipStream_t s, const float* t, const float* freq, float* feat, int S) {
    hipLaunchKernelGGL(time_sinus_kernel, dim3((S * 128 + 255) / 256), dim3(256), 0, s, t, freq, feat, S, 128);
}

static __global__ void act_kernel(const float* __restrict__ in, float* __restrict__ out, long n, int act) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = apply_act(in[i], act);
}

// ------------------------------------------------------------------------------------------ text encoder
// h[b, n, :] = E[id] + pos[n]  with id = text[b, n] + 1 (0 = filler, also for n >= nt), drop_text -> id = 0
// (dit.py:87-101).  Rows n >= lens[b] are written as zero; with mask_padding filler rows are zeroed (dit.py:104-105).
static __global__ void text_embed_kernel(const long long* __restrict__ text, int nt, const float* __restrict__ E,
                                  const float* __restrict__ pos, float* __restrict__ out, int B, int N, int Dt,
                                  const int* __restrict__ lens, int drop_text, int mask_padding, int add_pos,
                                  int pos_clamp) {
    const int d4 = Dt / 4;
    const long total = (long)B * N * d4;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % d4) * 4;
        const long row = idx / d4;
        const int n = (int)(row % N), b = (int)(row / N);
        const int len = lens ? lens[b] : N;
        long long id = (n < nt) ? text[(size_t)b * nt + n] + 1 : 0;
        const bool filler = (id == 0);
        if (drop_text) id = 0;
        float4 v = make_float4(0, 0, 0, 0);
        if (n < len && !(mask_padding && filler)) {
            v = *reinterpret_cast<const float4*>(E + (size_t)id * Dt + c);
            if (add_pos) {
                const int pn = n < pos_clamp ? n : pos_clamp - 1;
                const float4 p = *reinterpret_cast<const float4*>(pos + (size_t)pn * Dt + c);
                v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
            }
        }
        reinterpret_cast<float4*>(out)[idx] = v;
    }
}

// zero the rows whose (shifted) token id is the filler (text_mask_padding=True, dit.py:106-108)
static __global__ void zero_filler_rows_kernel(const long long* __restrict__ text, int nt, float* __restrict__ h, int B, int N,
                                        int C) {
    const int c4 = C / 4;
    const long total = (long)B * N * c4;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long row = idx / c4;
        const int n = (int)(row % N), b = (int)(row / N);
        const long long id = (n < nt) ? text[(size_t)b * nt + n] + 1 : 0;
        if (id == 0) reinterpret_cast<float4*>(h)[idx] = make_float4(0, 0, 0, 0);
    }
}

// Depthwise Conv1d(k=7, pad=3) over the sequence + LayerNorm(C, affine, eps)   (ConvNeXt blocks: modules.py:256-270,
// Vocos ConvNeXtBlock), one wave per token: token n of a segment of `len` tokens whose rows start at xs ([len, C] fp32);
// wk: [7][C] (repacked).  Taps outside [0, len) read as zero.  Both kernels below run this body, so a token's value does
// not depend on how its segment was laid out.
static __device__ __forceinline__ void dwconv7_ln_token(const float* __restrict__ xs, float* __restrict__ orow,
                                                        const float* __restrict__ wk, const float* __restrict__ wb,
                                                        const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                        int n, int len, int C, float eps, int lane) {
    float4 v[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = make_float4(0, 0, 0, 0);
        if (c < C) {
            float4 a = *reinterpret_cast<const float4*>(wb + c);
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int nn = n + k - 3;
                if (nn >= 0 && nn < len) {
                    const float4 xv = *reinterpret_cast<const float4*>(xs + (size_t)nn * C + c);
                    const float4 w = *reinterpret_cast<const float4*>(wk + (size_t)k * C + c);
                    a.x += w.x * xv.x; a.y += w.y * xv.y; a.z += w.z * xv.z; a.w += w.w * xv.w;
                }
            }
            v[i] = a;
            s += (a.x + a.y) + (a.z + a.w);
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < C) {
            const float a = v[i].x - mean, bb = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + bb * bb) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < C) {
            const float4 w = *reinterpret_cast<const float4*>(lnw + c), bi = *reinterpret_cast<const float4*>(lnb + c);
            *reinterpret_cast<float4*>(orow + c) =
                make_float4((v[i].x - mean) * rstd * w.x + bi.x, (v[i].y - mean) * rstd * w.y + bi.y,
                            (v[i].z - mean) * rstd * w.z + bi.z, (v[i].w - mean) * rstd * w.w + bi.w);
        }
    }
}

// x, out: [B, N, C] fp32.  Tokens outside [0, lens[b]) read as zero (each sample is convolved at its own length, dit.py:247-258).
static __global__ __launch_bounds__(256) void dwconv7_ln_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                         const float* __restrict__ wk, const float* __restrict__ wb,
                                                         const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                         int B, int N, int C, const int* __restrict__ lens, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (row >= (long)B * N) return;
    const int n = (int)(row % N), b = (int)(row / N);
    dwconv7_ln_token(x + (size_t)b * N * C, out + (size_t)row * C, wk, wb, lnw, lnb, n, lens ? lens[b] : N, C, eps, lane);
}

// Segment table of a packed ragged batch: item b owns rows row_start[b] .. row_start[b + 1] - 1 (B + 1 entries, every
// segment non-empty).  The item of row r by binary search: r is uniform over a wave (or a block) in the kernels below, so
// the ~log2(B) probes are scalar loads of a table that stays in cache.
static __device__ __forceinline__ int segment_of_row(const int* __restrict__ row_start, int B, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_start[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// The same over packed rows x, out: [R, C]: each token is convolved inside its own segment, whose ends are the zero padding.
static __global__ __launch_bounds__(256) void dwconv7_ln_ragged_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                const float* __restrict__ wk, const float* __restrict__ wb,
                                                                const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                                const int* __restrict__ row_start, int B, int R, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (row >= R) return;
    const int b = segment_of_row(row_start, B, (int)row);
    const int r0 = row_start[b];
    dwconv7_ln_token(x + (size_t)r0 * C, out + (size_t)row * C, wk, wb, lnw, lnb, (int)row - r0, row_start[b + 1] - r0, C, eps, lane);
}

// GRN (modules.py:231-240): Gx[b, c] = ||h[b, :len, c]||_2 over the SEQUENCE; Nx = Gx / (mean_c Gx + 1e-6);
// h <- gamma * (h * Nx) + beta + h.   Deterministic two-stage reduction: P partial sums per (b, c), combined in order.
constexpr int GRN_P = 16;
static __global__ void grn_partial_kernel(const float* __restrict__ h, float* __restrict__ part, int N, int C,
                                   const int* __restrict__ lens) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y, b = blockIdx.z;
    if (c >= C) return;
    const int len = lens ? lens[b] : N;
    float s = 0.f;
    for (int n = p; n < len; n += GRN_P) {
        const float v = h[((size_t)b * N + n) * C + c];
        s += v * v;
    }
    part[((size_t)b * GRN_P + p) * C + c] = s;
}
static __global__ __launch_bounds__(256) void grn_apply_kernel(float* __restrict__ h, const float* __restrict__ part,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int N, int C, const int* __restrict__ lens, int rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* gx = reinterpret_cast<float*>(smem_raw);  // [C] then [4] wave partials
    const int b = blockIdx.y, tid = threadIdx.x;
    float loc = 0.f;
    for (int c = tid; c < C; c += 256) {
        float s = 0.f;
#pragma unroll
        for (int p = 0; p < GRN_P; ++p) s += part[((size_t)b * GRN_P + p) * C + c];
        const float gv = sqrtf(s);
        gx[c] = gv;
        loc += gv;
    }
    loc = wave_sum(loc);
    if ((tid & 63) == 0) gx[C + (tid >> 6)] = loc;
    __syncthreads();
    const float mean = (gx[C] + gx[C + 1] + gx[C + 2] + gx[C + 3]) / (float)C;
    const float inv = 1.0f / (mean + 1e-6f);
    const int len = lens ? lens[b] : N;
    const int n0 = blockIdx.x * rows_per_block;
    const int c4n = C / 4;
    for (int i = tid; i < rows_per_block * c4n; i += 256) {
        const int n = n0 + i / c4n, c = (i % c4n) * 4;
        if (n >= len) continue;
        float4* ptr = reinterpret_cast<float4*>(h + ((size_t)b * N + n) * C + c);
        float4 v = *ptr;
        const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
        v.x = ga.x * (v.x * (gx[c] * inv)) + be.x + v.x;
        v.y = ga.y * (v.y * (gx[c + 1] * inv)) + be.y + v.y;
        v.z = ga.z * (v.z * (gx[c + 2] * inv)) + be.z + v.z;
        v.w = ga.w * (v.w * (gx[c + 3] * inv)) + be.w + v.w;
        *ptr = v;
    }
}

// zero rows n >= lens[b] of [B, N, C]
static __global__ void zero_tail_rows_kernel(float* __restrict__ h, int B, int N, int C, const int* __restrict__ lens) {
    const int c4 = C / 4;
    const long total = (long)B * N * c4;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long row = idx / c4;
        const int n = (int)(row % N), b = (int)(row / N);
        if (n >= lens[b]) reinterpret_cast<float4*>(h)[idx] = make_float4(0, 0, 0, 0);
    }
}

// zipvoice-style late average upsampling of the text embedding (dit.py:54-84; text_embedding_average_upsampling=True): the VALID
// tokens of a sample (original id != filler, position < the sample's own length) are repeated to fill its audio length, the
// last `remainder` tokens once more than the others; rows past the length and samples without a valid token are zero.
// One workgroup per sample; `in` -> `out` (different buffers).
static __global__ __launch_bounds__(256) void text_avg_upsample_kernel(const long long* __restrict__ text, int nt, const float* __restrict__ in,
                                                                        float* __restrict__ out, int N, int Dt, const int* __restrict__ lens) {
    extern __shared__ int valid_idx[];                    // [N]: positions of the valid tokens, in order
    __shared__ int n_valid;
    const int b = blockIdx.x;
    const int alen = lens ? min(lens[b], N) : N;
    if (threadIdx.x == 0) {
        int c = 0;
        for (int n = 0; n < alen && n < nt; ++n)
            if (text[(size_t)b * nt + n] + 1 != 0) valid_idx[c++] = n;
        n_valid = c;
    }
    __syncthreads();
    const int tl = n_valid, d4 = Dt / 4;
    const int base = tl > 0 ? alen / tl : 0, rem = tl > 0 ? alen % tl : 0;
    const int split = (tl - rem) * base;                  // output rows fed by the tokens that repeat `base` times
    for (long idx = threadIdx.x; idx < (long)N * d4; idx += blockDim.x) {
        const int n = (int)(idx / d4), c = (int)(idx % d4);
        float4 v = make_float4(0, 0, 0, 0);
        if (n < alen && tl > 0) {
            const int j = n < split ? n / base : (tl - rem) + (n - split) / (base + 1);
            v = reinterpret_cast<const float4*>(in + ((size_t)b * N + valid_idx[j]) * Dt)[c];
        }
        reinterpret_cast<float4*>(out + ((size_t)b * N + n) * Dt)[c] = v;
    }
}

// qk_norm = "rms_norm" (modules.py:397-404,481-497; the MMDiT's joint attention modules.py:588-608): the Ns positions of one stream
// in q and k, as the QKV epilogue left them WITHOUT rotary and scale, get RMSNorm(64, eps) with the stream's own gains, then the
// rotary embedding at the stream's own position (from 0) on the first pe_heads heads, then q its softmax scale -- in place.
// q / k are [Bp, H, L, 64] and the stream sits at layout positions [off, off + Ns): L = Ns, off = 0 for a backbone with one stream,
// (nt + N, 0) and (nt + N, nt) for the text and audio streams of the MMDiT's joint image (mmdit.h).
// 16 lanes per (batch row, head, position): 4 consecutive dims per lane = two rotary pairs.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(T* __restrict__ q, T* __restrict__ k, const float* __restrict__ gq,
                                                          const float* __restrict__ gk, const float* __restrict__ rope_cos,
                                                          const float* __restrict__ rope_sin, long rows, int Ns, int L, int off, int H,
                                                          int pe_heads, float q_scale, float eps) {
    const long gid = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long r = gid >> 4;                              // (b * H + h) * Ns + pos
    if (r >= rows) return;
    const int d = (int)(gid & 15) * 4;
    const int pos = (int)(r % Ns), h = (int)((r / Ns) % H);
    const long dst = (r / Ns) * L + off + pos;            // row of the layout
    float2 cs = make_float2(1, 1), sn = make_float2(0, 0);
    const bool rot = h < pe_heads;
    if (rot) {
        cs = *reinterpret_cast<const float2*>(rope_cos + (size_t)pos * 32 + (d >> 1));
        sn = *reinterpret_cast<const float2*>(rope_sin + (size_t)pos * 32 + (d >> 1));
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        T* p = (which ? k : q) + dst * 64 + d;
        const float4 g = *reinterpret_cast<const float4*>((which ? gk : gq) + d);
        float a0 = to_f32(p[0]), a1 = to_f32(p[1]), a2 = to_f32(p[2]), a3 = to_f32(p[3]);
        float ss = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64); ss += __shfl_xor(ss, 8, 64);
        const float rs = rsqrtf(ss * (1.0f / 64.0f) + eps);
        a0 = a0 * rs * g.x; a1 = a1 * rs * g.y; a2 = a2 * rs * g.z; a3 = a3 * rs * g.w;
        if (rot) {
            const float r0 = a0 * cs.x - a1 * sn.x, r1 = a1 * cs.x + a0 * sn.x;
            const float r2 = a2 * cs.y - a3 * sn.y, r3 = a3 * cs.y + a2 * sn.y;
            a0 = r0; a1 = r1; a2 = r2; a3 = r3;
        }
        const float sc = which ? 1.0f : q_scale;
        store4(p, a0 * sc, a1 * sc, a2 * sc, a3 * sc);
    }
}
// the one launch of it (the engine's qkv_project and the kernel-level API): Bp * H * Ns rows of 16 lanes
template <typename T>
static hipError_t launch_qknorm_rope(hipStream_t s, T* q, T* k, const float* gq, const float* gk, const float* rope_cos, const float* rope_sin,
                                     int Bp, int H, int Ns, int L, int off, int pe_heads, float q_scale, float eps) {
    if (Bp <= 0 || H <= 0 || Ns <= 0 || off < 0 || off + Ns > L) return hipErrorInvalidValue;   // (the stream lies inside the layout)
    const long rows = (long)Bp * H * Ns;
    hipLaunchKernelGGL((qknorm_rope_kernel<T>), dim3((unsigned)((rows * 16 + 255) / 256)), dim3(256), 0, s, q, k, gq, gk, rope_cos, rope_sin, rows,
                       Ns, L, off, H, pe_heads, q_scale, eps);
    return hipGetLastError();
}

// --------------------------------------------------------------------------------------- weight repacking
// Conv1d weight [R = out channels][A = in channels per group][31 taps] (torch) -> implicit-GEMM operand
// out[r][tap * A + a], rows zero-padded to ld_out (a whole number of 128-byte K-tiles, convpos.h)
template <typename T>
__global__ void conv_pack_kernel(const float* __restrict__ in, T* __restrict__ out, long R, int A, int Bd, int ld_out) {
    const long total = R * ld_out;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % ld_out);
        const long r = i / ld_out;
        const int a = k % A, bd = k / A;
        out[i] = bd < Bd ? from_f32<T>(in[(r * A + a) * Bd + bd]) : from_f32<T>(0.f);
    }
}

// in [R][A][Bd] fp32 -> out [R][Bd][A] (T)
template <typename T>
__global__ void permute_last2_kernel(const float* __restrict__ in, T* __restrict__ out, long R, int A, int Bd) {
    const long total = R * A * Bd;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int a = (int)(i % A);
        const long t = i / A;
        const int bd = (int)(t % Bd);
        const long r = t / Bd;
        out[i] = from_f32<T>(in[(r * A + a) * Bd + bd]);
    }
}
// 2-D copy with conversion and zero padding: out[r][c] = c < cols ? in[r][c] : 0, r < rows_out (rows >= rows_in zero)
template <typename T>
__global__ void cast_pad_kernel(const float* __restrict__ in, int ld_in, int rows_in, int cols, T* __restrict__ out,
                                int ld_out, int rows_out) {
    const long total = (long)rows_out * ld_out;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ld_out);
        const long r = i / ld_out;
        out[i] = from_f32<T>((r < rows_in && c < cols) ? in[r * ld_in + c] : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------ Vocos
// A[b*T + t][k*C + ci] = mel[b][ci][t + k - 3]  (Conv1d(C, dim, k=7, pad=3) as a GEMM); columns >= 7*C zero (K padding).
// mel is read through element strides (sb, sc, st), so the [B, T, C] mel that sample() returns can be decoded through
// the reference's `vocoder.decode(mel.permute(0, 2, 1))` view without a transposing copy.
static __global__ void im2col7_kernel(const float* __restrict__ mel, long sb, long sc, long st, float* __restrict__ A, int B, int C,
                                      int T, int ld) {
    const long total = (long)B * T * ld;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % ld);
        const long r = i / ld;
        const int t = (int)(r % T), b = (int)(r / T);
        float v = 0.f;
        if (col < 7 * C) {
            const int k = col / C, ci = col - k * C;
            const int tt = t + k - 3;
            if (tt >= 0 && tt < T) v = mel[b * sb + ci * sc + tt * st];
        }
        A[i] = v;
    }
}
// ISTFT head (export_vocoder_to_onnx.py:51-59): h[r, 0:F] = log-magnitude, h[r, F:2F] = phase;
// S[r, f] = min(exp(m), 100) * cos(p), S[r, F + f] = ... * sin(p); columns >= 2F zeroed (K padding of the iDFT GEMM).
static __global__ void istft_spec_kernel(const float* __restrict__ h, int ldh, float* __restrict__ S, int lds, long R, int F) {
    const long total = R * lds;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % lds);
        const long r = i / lds;
        float v = 0.f;
        if (c < 2 * F) {
            const int f = c < F ? c : c - F;
            const float mag = fminf(expf(h[r * ldh + f]), 100.0f);
            const float p = h[r * ldh + F + f];
            v = c < F ? mag * cosf(p) : mag * sinf(p);
        }
        S[i] = v;
    }
}
// Ragged im2col7: packed row r = (item b, local frame t) of the segment table; item b is frames [mel_start[b], mel_start[b] +
// T_b) of batch row b, and taps outside [0, T_b) are the conv's zero padding -- frames before the window (the prompt), past
// it, and other items' rows are never read.  One block per packed row (the item lookup is uniform over the block).
static __global__ __launch_bounds__(256) void im2col7_ragged_kernel(const float* __restrict__ mel, long sb, long sc, long st,
                                                             const int* __restrict__ row_start, const int* __restrict__ mel_start,
                                                             float* __restrict__ A, int B, int C, int R, int ld) {
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const int b = segment_of_row(row_start, B, r);
        const int r0 = row_start[b], t = r - r0, Tb = row_start[b + 1] - r0;
        const float* src = mel + b * sb + (long)mel_start[b] * st;
        for (int col = threadIdx.x; col < ld; col += blockDim.x) {
            float v = 0.f;
            if (col < 7 * C) {
                const int k = col / C, ci = col - k * C;
                const int tt = t + k - 3;
                if (tt >= 0 && tt < Tb) v = src[ci * sc + tt * st];
            }
            A[(size_t)r * ld + col] = v;
        }
    }
}
// overlap-add of windowed frames + window-envelope normalisation + centre trim = torch.istft(center=True): sample i of one
// item of T frames [T, nfft] (already multiplied by the synthesis window)
static __device__ __forceinline__ float istft_ola_sample(const float* __restrict__ frames, const float* __restrict__ win, int T,
                                                         int nfft, int hop, int i) {
    const int pos = i + nfft / 2;
    int t1 = pos / hop;
    if (t1 > T - 1) t1 = T - 1;
    int t0 = (pos - nfft + hop) / hop;  // smallest t with t*hop + nfft > pos
    if (pos - nfft + 1 <= 0) t0 = 0;
    float acc = 0.f, env = 0.f;
    for (int t = t0; t <= t1; ++t) {
        const int j = pos - t * hop;
        if (j >= 0 && j < nfft) {
            acc += frames[(size_t)t * nfft + j];
            env += win[j] * win[j];
        }
    }
    return acc / env;
}
// frames [B*T, nfft], wav [B, (T-1)*hop]
static __global__ void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ win, float* __restrict__ wav,
                                 int B, int T, int nfft, int hop) {
    const int L = (T - 1) * hop;
    const long total = (long)B * L;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / L);
        wav[i] = istft_ola_sample(frames + (size_t)b * T * nfft, win, T, nfft, hop, (int)(i % L));
    }
}
// The same per item of a packed batch (blockIdx.y = item): frames [R, nfft]; frame range, envelope and centre trim at the
// item's own T_b; then x gain[b] as a separate multiply; then zeros up to wav_stride.  wav [B, wav_stride].
static __global__ void istft_ola_ragged_kernel(const float* __restrict__ frames, const float* __restrict__ win,
                                        const int* __restrict__ row_start, const float* __restrict__ gain,
                                        float* __restrict__ wav, long wav_stride, int nfft, int hop) {
    const int b = blockIdx.y;
    const int r0 = row_start[b], T = row_start[b + 1] - r0;
    const long L = (long)(T - 1) * hop;
    const float g = gain[b];
    const float* fr = frames + (size_t)r0 * nfft;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < wav_stride; i += (long)gridDim.x * blockDim.x)
        wav[b * wav_stride + i] = i < L ? istft_ola_sample(fr, win, T, nfft, hop, (int)i) * g : 0.f;
}

// In place: W f32 [rows, ld] (ld % 32 == 0) -> per 32-element block the 128 bytes the split-operand GEMM reads (gemm2.h GemmOperands::WSplit):
// 16-byte chunk g = f16 hi of k = 4g..4g+3, 16+4g..16+4g+3; chunk 4 + g = f16 lo (w - hi) of the same k.  One thread per block.
static __global__ void split_planar_kernel(float* __restrict__ w, long blocks) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < blocks; i += (long)gridDim.x * blockDim.x) {
        float4* p = reinterpret_cast<float4*>(w + i * 32);
        float v[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 t = p[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
        f16_t hi[32], lo[32];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const float x = v[(s < 4 ? 4 * g : 16 + 4 * g - 4) + s];
                const f16_t h = (f16_t)x;
                hi[g * 8 + s] = h;
                lo[g * 8 + s] = (f16_t)(x - (float)h);
            }
        f16x8* o = reinterpret_cast<f16x8*>(w + i * 32);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x8 a, b;
#pragma unroll
            for (int s = 0; s < 8; ++s) { a[s] = hi[g * 8 + s]; b[s] = lo[g * 8 + s]; }
            o[g] = a;
            o[4 + g] = b;
        }
    }
}

// Diagnostic (F5_X3_ABLATE): out = (float)(f16)in -- an f32 operand that is not stored split, as plain f16 would see it
static __global__ void round_f16_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (float)(f16_t)in[i];
}
// The rotary table in the order the QKV epilogue's accumulator lanes read it (EpiQKV, gemm.h): out[pos][g][j] = {cos, cos, sin, sin} of
// the pairs (j*8 + g*2, j*8 + g*2 + 1) from the [maxpos][32] tables (modules.py:398-424 / x_transformers RotaryEmbedding values).
static __global__ __launch_bounds__(256) void rope_frag_kernel(const float* __restrict__ cs, const float* __restrict__ sn, float* __restrict__ out,
                                                        long maxpos) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < maxpos * 16; i += (long)gridDim.x * blockDim.x) {   // one (pos, g, j)
        const long pos = i >> 4;
        const int g = (int)(i >> 2) & 3, j = (int)i & 3, pair = j * 8 + g * 2;
        const float2 c = *reinterpret_cast<const float2*>(cs + pos * 32 + pair), s2 = *reinterpret_cast<const float2*>(sn + pos * 32 + pair);
        *reinterpret_cast<float4*>(out + i * 4) = make_float4(c.x, c.y, s2.x, s2.y);
    }
}

// Diagnostic (F5_X3_ABLATE, tools/x3_ablate.py): zeroes the lo halves (chunks 4..7 of every 128-byte block) of a split-planar
// operand in place, which turns the three-product f16x3 contraction into the plain f16 one (a_hi w_hi) for that operand.
static __global__ void zero_lo_planar_kernel(float* __restrict__ w, long blocks) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < blocks * 4; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<float4*>(w + (i >> 2) * 32)[4 + (i & 3)] = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace f5
