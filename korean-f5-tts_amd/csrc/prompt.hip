// Prompt preparation (utils_infer.py:523-533, eval/utils_eval.py:111-118): mono mix, RMS, the gain
// up to target_rms and torchaudio's polyphase windowed-sinc Resample for a ragged batch of prompts of any channel count, length
// and rate, in three launches with no host read.  The arithmetic contract is in include/f5_hip.h; in short
//   prompt_rms_partial_kernel   one block per 2048-sample tile of an item: the mono mix on the fly, its squares summed in f64 in a
//                               fixed order (thread t takes j = t, t + 256, ...; a fixed tree over the threads)
//   prompt_rms_finish_kernel    one thread per item: the tiles' sums in ascending order, rms = (float)sqrt(S / n)
//   prompt_resample_kernel      one block per run of output frames of an item: the levelled mono window staged in LDS (mono mix and
//                               gain applied as it loads, the zero padding by index logic), then per output sample the taps in
//                               ascending order, f32 multiply then f32 add; items already at the target rate pass through levelled
// The mono mix is computed twice (once per kernel) by the same instructions instead of being stored: an item's bits depend on
// the item alone either way, and the stage keeps no signal-sized workspace.
// The banks live transposed, [K, new]: consecutive output samples of a frame (consecutive phases) read consecutive words.
#include "elementwise.h"
#include "internal.h"
#include "mel_handle.h"
#include "resample.h"

using namespace f5;
#define fail f5_fail

namespace {
constexpr int RMS_TILE = 2048;      // samples per partial sum (part of the contract: it fixes the order of the f64 sum)
constexpr int OUT_TILE = RS_OUT_TILE;
constexpr int LDS_FLOATS = RS_LDS_FLOATS;   // a window that does not fit is read from global memory instead
constexpr long long MAX_UNITS = 1LL << 30;   // tiles / blocks of one call (grid sizes and the segment tables are int)

struct PromptItem {
    long long in_start, out_start, out_len;   // elements from base / out; samples written
    const float* bank;                        // [K, new], null for an item at the target rate
    int channels, n, orig, nw, width, K, F, direct;   // F frames per block; direct: the window does not fit the LDS
};
// The per-item tables of one call, items[B] | tile_start[B + 1] | blk_start[B + 1]: one layout for the pinned slot and the device
struct PromptTables {
    PromptItem* items;
    int *tile_start, *blk_start;
    PromptTables(char* base, int B)
        : items(reinterpret_cast<PromptItem*>(base)), tile_start(reinterpret_cast<int*>(base + (size_t)B * sizeof(PromptItem))),
          blk_start(tile_start + B + 1) {}
    static size_t bytes(int B) { return (size_t)B * sizeof(PromptItem) + ((size_t)2 * B + 2) * 4; }
};
}  // namespace

// step 1 of the contract: the channels in ascending order, then one division
static __device__ __forceinline__ float mono_sample(const float* __restrict__ x, int channels, int n, int j) {
    float s = x[j];
    if (channels == 1) return s;
    for (int c = 1; c < channels; ++c) s = s + x[(size_t)c * n + j];
    return s / (float)channels;
}
// steps 1 and 3 at position j of the zero-padded signal (the zeros are index logic: nothing outside [0, n) is read)
static __device__ __forceinline__ float levelled_sample(const float* __restrict__ x, int channels, int n, long long j, bool scale,
                                                        float target_rms, float rms) {
    if (j < 0 || j >= n) return 0.f;
    float m = mono_sample(x, channels, n, (int)j);
    if (scale) m = (m * target_rms) / rms;
    return m;
}

static __global__ __launch_bounds__(256) void prompt_rms_partial_kernel(const float* __restrict__ base, const PromptItem* __restrict__ items,
                                                                        const int* __restrict__ tile_start, int B,
                                                                        double* __restrict__ partial) {
    __shared__ double red[256];
    const int tile = blockIdx.x;
    const int b = segment_of_row(tile_start, B, tile);
    const PromptItem it = items[b];
    const float* x = base + it.in_start;
    const int j0 = (tile - tile_start[b]) * RMS_TILE;
    const int count = min(RMS_TILE, it.n - j0);
    double s = 0.0;
    for (int j = threadIdx.x; j < count; j += 256) {
        const double m = (double)mono_sample(x, it.channels, it.n, j0 + j);
        s = s + m * m;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[tile] = red[0];
}

static __global__ __launch_bounds__(64) void prompt_rms_finish_kernel(const PromptItem* __restrict__ items, const int* __restrict__ tile_start,
                                                                      int B, const double* __restrict__ partial, float* __restrict__ rms_out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double S = 0.0;
    for (int t = tile_start[b]; t < tile_start[b + 1]; ++t) S = S + partial[t];
    rms_out[b] = (float)sqrt(S / (double)items[b].n);
}

static __global__ __launch_bounds__(256) void prompt_resample_kernel(const float* __restrict__ base, const PromptItem* __restrict__ items,
                                                                     const int* __restrict__ blk_start, int B, const float* __restrict__ rms_in,
                                                                     float target_rms, float* __restrict__ out) {
    __shared__ float xs[LDS_FLOATS];
    const int blk = blockIdx.x;
    const int b = segment_of_row(blk_start, B, blk);
    const PromptItem it = items[b];
    const float* x = base + it.in_start;
    float* y = out + it.out_start;
    const float rms = rms_in[b];
    const bool scale = rms < target_rms;   // (false for a NaN rms, as the host's `if rms < target_rms`)
    const long long tile = blk - blk_start[b];

    if (it.orig == it.nw) {   // at the target rate: the levelled mono signal, bit for bit
        const long long o0 = tile * OUT_TILE + 4 * (long long)threadIdx.x;
        if (o0 >= it.out_len) return;
        float v[4];
        for (int q = 0; q < 4; ++q) v[q] = levelled_sample(x, it.channels, it.n, o0 + q < it.out_len ? o0 + q : -1, scale, target_rms, rms);
        if (o0 + 4 <= it.out_len && (reinterpret_cast<uintptr_t>(y + o0) & 15) == 0) {
            *reinterpret_cast<float4*>(y + o0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int q = 0; q < 4; ++q)
                if (o0 + q < it.out_len) y[o0 + q] = v[q];
        }
        return;
    }

    const long long frame0 = tile * it.F;
    const long long win0 = frame0 * it.orig - it.width;   // position in the unpadded signal of the window's first sample
    if (!it.direct) {
        const int win = (it.F - 1) * it.orig + it.K;      // <= LDS_FLOATS by the host's choice of F
        for (int e = threadIdx.x; e < win; e += 256) xs[e] = levelled_sample(x, it.channels, it.n, win0 + e, scale, target_rms, rms);
        __syncthreads();
    }
    const long long o_first = frame0 * it.nw;
    const long long nout = min((long long)it.F * it.nw, it.out_len - o_first);   // > 0: the host counts blocks from out_len
    for (long long l0 = 4 * (long long)threadIdx.x; l0 < nout; l0 += OUT_TILE) {
        int xi[4], bp[4];
        for (int q = 0; q < 4; ++q) {
            const long long l = l0 + q < nout ? l0 + q : l0;   // a lane past the end repeats a valid sample and stores nothing
            const int f = (int)(l / it.nw);
            xi[q] = f * it.orig;
            bp[q] = (int)(l - (long long)f * it.nw);
        }
        float acc[4];
        if (!it.direct)
            resample_taps(it.bank, it.nw, it.K, xi, bp, [&](int e) { return xs[e]; }, acc);
        else
            resample_taps(it.bank, it.nw, it.K, xi, bp,
                          [&](int e) { return levelled_sample(x, it.channels, it.n, win0 + e, scale, target_rms, rms); }, acc);
        float* dst = y + o_first + l0;
        if (l0 + 4 <= nout && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
            for (int q = 0; q < 4; ++q)
                if (l0 + q < nout) dst[q] = acc[q];
        }
    }
}

// shared by the plan and the prepare call: every per-item refusal, the packing, and (pairs != null) each item's rate pair
static int prepare_plan(const char* who, int B, const int32_t* n_host, const int32_t* sr_host, int target_sr, int64_t* len_out,
                        int64_t* start_out, int64_t* total_out, RatePair* pairs) {
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 items (B = %d)", who, B);
    if (target_sr < 1) return fail(F5_EINVAL, "%s: target_sr = %d < 1", who, target_sr);
    int64_t run = 0;
    for (int b = 0; b < B; ++b) {
        if (n_host[b] < 1) return fail(F5_EINVAL, "%s: item %d has n = %d samples (need n >= 1)", who, b, n_host[b]);
        if (sr_host[b] < 1) return fail(F5_EINVAL, "%s: item %d has sr = %d (need sr >= 1)", who, b, sr_host[b]);
        RatePair r;
        if (!rate_pair(sr_host[b], target_sr, &r))
            return fail(F5_EINVAL, "%s: item %d: the resample bank of %d Hz -> %d Hz has more than 2^20 elements (resample it on the host)",
                        who, b, sr_host[b], target_sr);
        if (pairs) pairs[b] = r;
        run = (run + 3) / 4 * 4;
        start_out[b] = run;
        len_out[b] = ((int64_t)r.nw * n_host[b] + r.orig - 1) / r.orig;
        run += len_out[b];
    }
    *total_out = run;
    return F5_OK;
}

extern "C" int f5_mel_prepare_plan(int32_t B, const int32_t* n_host, const int32_t* sr_host, int32_t target_sr, int64_t* len_out,
                                   int64_t* start_out, int64_t* total_out) {
    if (!n_host) return fail(F5_EINVAL, "f5_mel_prepare_plan: null n_host");
    if (!sr_host) return fail(F5_EINVAL, "f5_mel_prepare_plan: null sr_host");
    if (!len_out) return fail(F5_EINVAL, "f5_mel_prepare_plan: null len_out");
    if (!start_out) return fail(F5_EINVAL, "f5_mel_prepare_plan: null start_out");
    if (!total_out) return fail(F5_EINVAL, "f5_mel_prepare_plan: null total_out");
    return prepare_plan("f5_mel_prepare_plan", B, n_host, sr_host, target_sr, len_out, start_out, total_out, nullptr);
}

extern "C" int f5_mel_resample_bank(f5_mel* m, int32_t sr, int32_t target_sr, const float* bank_host, int64_t numel, f5_stream stream) {
    if (!m) return fail(F5_EINVAL, "f5_mel_resample_bank: null handle m");
    if (!bank_host) return fail(F5_EINVAL, "f5_mel_resample_bank: null bank_host");
    if (sr < 1 || target_sr < 1) return fail(F5_EINVAL, "f5_mel_resample_bank: need sr >= 1 and target_sr >= 1 (sr = %d, target_sr = %d)", sr, target_sr);
    RatePair r;
    if (!rate_pair(sr, target_sr, &r))
        return fail(F5_EINVAL, "f5_mel_resample_bank: the resample bank of %d Hz -> %d Hz has more than 2^20 elements", sr, target_sr);
    if (r.same()) return fail(F5_EINVAL, "f5_mel_resample_bank: sr == target_sr = %d needs no bank", sr);
    if (numel != (int64_t)r.nw * r.K)
        return fail(F5_EINVAL, "f5_mel_resample_bank: numel = %lld, the bank of %d Hz -> %d Hz is [%d, %d]", (long long)numel, sr, target_sr, r.nw,
                    r.K);
    const auto key = std::make_pair(r.orig, r.nw);
    if (m->bank_of.count(key)) return F5_OK;
    std::vector<float> t((size_t)numel);   // [new, K] -> [K, new]
    for (int p = 0; p < r.nw; ++p)
        for (int k = 0; k < r.K; ++k) t[(size_t)k * r.nw + p] = bank_host[(size_t)p * r.K + k];
    float* dev = nullptr;
    CHK(m->banks.alloc((size_t)numel, &dev));
    HIPCHK(hipMemcpy(dev, t.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
    m->bank_of[key] = dev;
    return F5_OK;
}

extern "C" int f5_mel_resample_bank_count(f5_mel* m, int32_t* uploads_out) {
    if (!m || !uploads_out) return fail(F5_EINVAL, "f5_mel_resample_bank_count: null handle m / uploads_out");
    *uploads_out = (int32_t)m->bank_of.size();
    return F5_OK;
}

extern "C" int f5_mel_prepare_ragged(f5_mel* m, const float* base, int32_t B, const int64_t* start_host, const int32_t* channels_host,
                                     const int32_t* n_host, const int32_t* sr_host, int32_t target_sr, float target_rms, float* out,
                                     int64_t out_capacity, float* rms_out, f5_stream stream) {
    const char* who = "f5_mel_prepare_ragged";
    if (!m) return fail(F5_EINVAL, "%s: null handle m", who);
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!channels_host) return fail(F5_EINVAL, "%s: null channels_host", who);
    if (!n_host) return fail(F5_EINVAL, "%s: null n_host", who);
    if (!sr_host) return fail(F5_EINVAL, "%s: null sr_host", who);
    if (!out) return fail(F5_EINVAL, "%s: null out", who);
    if (!rms_out) return fail(F5_EINVAL, "%s: null rms_out", who);
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 items (B = %d)", who, B);
    if (!(target_rms > 0.f)) return fail(F5_EINVAL, "%s: target_rms = %g (need target_rms > 0)", who, (double)target_rms);
    for (int b = 0; b < B; ++b) {
        if (start_host[b] < 0) return fail(F5_EINVAL, "%s: item %d starts at start = %lld < 0", who, b, (long long)start_host[b]);
        if (channels_host[b] < 1) return fail(F5_EINVAL, "%s: item %d has channels = %d (need channels >= 1)", who, b, channels_host[b]);
    }
    m->plan_out.resize((size_t)2 * B);
    int64_t* len = m->plan_out.data();
    int64_t* start = len + B;
    int64_t total = 0;
    std::vector<RatePair> pairs((size_t)B);
    CHK(prepare_plan(who, B, n_host, sr_host, target_sr, len, start, &total, pairs.data()));
    // the block counts of the two ragged launches
    std::vector<int> F((size_t)B), direct((size_t)B), tile_start((size_t)B + 1), blk_start((size_t)B + 1);
    long long tiles = 0, blks = 0;
    for (int b = 0; b < B; ++b) {
        const RatePair& r = pairs[b];
        tile_start[b] = (int)tiles;
        blk_start[b] = (int)blks;
        tiles += ((long long)n_host[b] + RMS_TILE - 1) / RMS_TILE;
        if (r.same()) {
            F[b] = 0;
            direct[b] = 0;
            blks += (len[b] + OUT_TILE - 1) / OUT_TILE;
        } else {
            direct[b] = r.K > LDS_FLOATS;
            const int f = direct[b] ? std::max(1, OUT_TILE / r.nw) : frames_per_block(r);
            F[b] = f;
            const long long frames = (len[b] + r.nw - 1) / r.nw;
            blks += (frames + f - 1) / f;
        }
        if (tiles > MAX_UNITS || blks > MAX_UNITS)
            return fail(F5_EINVAL, "%s: more than 2^30 tiles of work at item %d (split the batch)", who, b);
    }
    tile_start[B] = (int)tiles;
    blk_start[B] = (int)blks;
    if (out_capacity < total)
        return fail(F5_EINVAL, "%s: out_capacity = %lld is less than the plan's total of %lld elements", who, (long long)out_capacity,
                    (long long)total);
    std::vector<const float*> bank((size_t)B, nullptr);
    for (int b = 0; b < B; ++b) {
        if (pairs[b].same()) continue;
        auto it = m->bank_of.find(std::make_pair(pairs[b].orig, pairs[b].nw));
        if (it == m->bank_of.end())
            return fail(F5_ESTATE, "%s: item %d: no resample bank for %d Hz -> %d Hz yet (f5_mel_resample_bank)", who, b, sr_host[b], target_sr);
        bank[b] = it->second;
    }

    hipStream_t s = (hipStream_t)stream;
    double* partial = nullptr;
    char* tab = nullptr;
    auto plan = [&](Arena& a) {
        a.reset();
        partial = a.take<double>((size_t)tiles);
        tab = a.take<char>(PromptTables::bytes(B));
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(m->arena.reserve(plan(dry)));
    (void)plan(m->arena);
    // one pinned slot, one copy; the device tables are read by this call's kernels only
    CHK(m->stage.upload(tab, PromptTables::bytes(B), s, [&](char* host) {
        const PromptTables h(host, B);
        for (int b = 0; b < B; ++b) {
            const RatePair& r = pairs[b];
            h.items[b] = PromptItem{start_host[b], start[b], len[b], bank[b], channels_host[b], n_host[b], r.orig, r.nw, r.width, r.K, F[b], direct[b]};
            h.tile_start[b] = tile_start[b];
            h.blk_start[b] = blk_start[b];
        }
        h.tile_start[B] = tile_start[B];
        h.blk_start[B] = blk_start[B];
    }));
    const PromptTables d(tab, B);
    hipLaunchKernelGGL(prompt_rms_partial_kernel, dim3((unsigned)tiles), dim3(256), 0, s, base, d.items, d.tile_start, B, partial);
    KCHK();
    hipLaunchKernelGGL(prompt_rms_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, d.items, d.tile_start, B, partial, rms_out);
    KCHK();
    hipLaunchKernelGGL(prompt_resample_kernel, dim3((unsigned)blks), dim3(256), 0, s, base, d.items, d.blk_start, B, rms_out, target_rms, out);
    KCHK();
    return F5_OK;
}
