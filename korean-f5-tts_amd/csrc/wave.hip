// Waveform post-processing on gfx950.  f5_wave_crossfade: the cross-fade concatenation of the chunks of one long text
// (infer/utils_infer.py:734-775), so that a batch of decoded chunks becomes one waveform without leaving the device.
//
// The reference folds the pieces from the left: final <- [final[:-n], final[-n:] * linspace(1, 0, n) + next[:n] * linspace(0, 1, n),
// next[n:]] in float64.  Every output sample is a function of the samples of the pieces that cover it alone, so the fold runs per
// output sample, over the covering pieces in ascending order, in double, and is rounded to f32 once at the end -- the bits of
// numpy's result cast to float32 (the file is built with -ffp-contract=off: multiply, multiply, add as written).
//
// f5_wave_join: the same fold with a fade request per piece, for the multi-voice script of infer/infer_cli.py:363-415 -- cross-fades
// inside a tagged stretch, plain concatenation between stretches -- over up to 65535 pieces that lie anywhere under one base pointer.
// Its table goes through the pinned slot and the workspace of the handle-less calls (CallState, internal.h); a tile finds its first
// piece by bisection over the pieces' ends, which never decrease, and walks up while a later piece can still start inside it.
#include "join.h"

using namespace f5;
#define fail f5_fail

namespace {
constexpr int kMaxPieces = 64;
constexpr int kThreads = 256;
constexpr int kPerThread = JOIN_PER_THREAD;         // consecutive samples per thread: one 16-byte store
constexpr int kTile = kThreads * kPerThread;        // samples per block and round

// the thread's four samples, rounded to f32 once: one 16-byte store where the address allows; nothing at or past total
__device__ __forceinline__ void store_samples(float* __restrict__ out, long long p0, long long total, int out_aligned,
                                              const double (&v)[kPerThread]) {
    if (p0 + kPerThread <= total && out_aligned) {
        *reinterpret_cast<float4*>(out + p0) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < kPerThread; ++e)
            if (p0 + e < total) out[p0 + e] = (float)v[e];
    }
}

// The host plan, passed by value as a kernel argument (1.5 KiB): nothing to copy, nothing to keep alive, capturable.
struct WavePlan {
    long long off[kMaxPieces];   // position of the piece's first sample in the output
    double step[kMaxPieces];     // 1 / (n - 1): numpy's linspace step (0 for n < 2)
    int n[kMaxPieces];           // samples of the piece's head that fade in over what is already there
    int len[kMaxPieces];
};

__global__ __launch_bounds__(kThreads) void wave_crossfade_kernel(const float* __restrict__ wav, long long wav_stride, int B,
                                                                   const WavePlan pl, float* __restrict__ out, long long total,
                                                                   long long ntiles, int out_aligned) {
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long t0 = tile * kTile, t1 = t0 + kTile;      // the block's span (block-uniform)
        const long long p0 = t0 + (long long)threadIdx.x * kPerThread;
        double v[kPerThread] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < B; ++i) {
            const long long off = pl.off[i];
            const int len = pl.len[i];
            if (off >= t1 || off + len <= t0) continue;           // uniform: the piece does not touch this tile
            fold_piece(wav + (long long)i * wav_stride, off, len, i > 0 ? pl.n[i] : 0, pl.step[i], p0, v);
        }
        store_samples(out, p0, total, out_aligned, v);
    }
}

__global__ __launch_bounds__(kThreads) void wave_join_kernel(const float* __restrict__ base, const JoinPiece* __restrict__ pieces, int B,
                                                              float* __restrict__ out, long long total, long long ntiles,
                                                              int out_aligned) {
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long t0 = tile * kTile, t1 = t0 + kTile;      // the block's span (block-uniform, like everything up to fold_piece)
        const long long p0 = t0 + (long long)threadIdx.x * kPerThread;
        double v[kPerThread] = {0.0, 0.0, 0.0, 0.0};
        fold_pieces(base, pieces, B, first_piece(pieces, B, t0), t1, p0, v);   // (t0 < total = end[B - 1])
        store_samples(out, p0, total, out_aligned, v);
    }
}
}  // namespace

extern "C" int f5_wave_crossfade(const float* wav, int32_t B, int64_t wav_stride, const int32_t* lens_host,
                                 int32_t cross_fade_samples, float* out, int64_t out_cap, int64_t* out_len_host, f5_stream stream) {
    if (B < 1 || B > kMaxPieces) return fail(F5_EINVAL, "f5_wave_crossfade: need 1 <= B <= %d pieces (B = %d)", kMaxPieces, B);
    if (!wav) return fail(F5_EINVAL, "f5_wave_crossfade: wav is null");
    if (!lens_host) return fail(F5_EINVAL, "f5_wave_crossfade: lens_host is null");
    if (!out) return fail(F5_EINVAL, "f5_wave_crossfade: out is null");
    WavePlan pl{};
    long long L = 0;
    int max_len = 0;
    for (int i = 0; i < B; ++i) {
        const int len = lens_host[i];
        if (len < 1) return fail(F5_EINVAL, "f5_wave_crossfade: lens_host[%d] = %d; every piece needs at least 1 sample", i, len);
        max_len = std::max(max_len, len);
        long long n = 0;
        if (i > 0 && cross_fade_samples > 0) n = std::min<long long>(std::min<long long>(cross_fade_samples, L), len);
        pl.off[i] = L - n;
        pl.n[i] = (int)n;
        pl.len[i] = len;
        pl.step[i] = n > 1 ? 1.0 / (double)(n - 1) : 0.0;
        L = pl.off[i] + len;
    }
    if (wav_stride < max_len)
        return fail(F5_EINVAL, "f5_wave_crossfade: wav_stride %lld is less than the longest piece (%d samples)", (long long)wav_stride,
                    max_len);
    if (out_cap < L)
        return fail(F5_EINVAL, "f5_wave_crossfade: out_cap %lld is less than the %lld samples of the result", (long long)out_cap, L);
    const long long ntiles = (L + kTile - 1) / kTile;
    const int grid = (int)std::min<long long>(ntiles, 2048);
    const int out_aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    wave_crossfade_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(wav, (long long)wav_stride, B, pl, out, L, ntiles, out_aligned);
    KCHK();
    if (out_len_host) *out_len_host = L;
    return F5_OK;
}

extern "C" int f5_wave_join(const float* base, int32_t B, const int64_t* start_host, const int32_t* lens_host, const int32_t* fade_host,
                            float* out, int64_t out_cap, int64_t* out_len_host, f5_stream stream) {
    const char* who = "f5_wave_join";
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 pieces (B = %d)", who, B);
    if (!base) return fail(F5_EINVAL, "%s: base is null", who);
    if (!start_host) return fail(F5_EINVAL, "%s: start_host is null", who);
    if (!lens_host) return fail(F5_EINVAL, "%s: lens_host is null", who);
    if (!fade_host) return fail(F5_EINVAL, "%s: fade_host is null", who);
    if (!out) return fail(F5_EINVAL, "%s: out is null", who);
    std::vector<JoinPiece> pieces((size_t)B);
    JoinRun run;
    for (int i = 0; i < B; ++i) {
        const int len = lens_host[i], fade = fade_host[i];
        if (len < 1) return fail(F5_EINVAL, "%s: lens_host[%d] = %d; every piece needs at least 1 sample", who, i, len);
        if (fade < 0) return fail(F5_EINVAL, "%s: fade_host[%d] = %d < 0", who, i, fade);
        if (start_host[i] < 0) return fail(F5_EINVAL, "%s: start_host[%d] = %lld < 0", who, i, (long long)start_host[i]);
        run.place(i == 0, start_host[i], len, fade, &pieces[i]);
    }
    const long long L = run.L;
    if (out_cap < L) return fail(F5_EINVAL, "%s: out_cap %lld is less than the %lld samples of the result", who, (long long)out_cap, L);
    run.close(pieces.data(), B);
    const size_t tab_bytes = (size_t)B * sizeof(JoinPiece);

    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) { __builtin_memcpy(host, pieces.data(), tab_bytes); }));
    const long long ntiles = (L + kTile - 1) / kTile;
    const int grid = (int)std::min<long long>(ntiles, 2048);
    const int out_aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    wave_join_kernel<<<grid, kThreads, 0, s>>>(base, reinterpret_cast<const JoinPiece*>(tab), B, out, L, ntiles, out_aligned);
    KCHK();
    if (out_len_host) *out_len_host = L;
    return st->leave(s);
}
