// Delivery of generated audio at a client's rate and sample format (what the reference's clients and evaluation scripts do to
// every generated file: eval/utils_eval.py:403-411 resamples to 16 kHz, a socket wants PCM16).  f5_wave_deliver: a ragged batch of
// 24 kHz f32 streams, each possibly unfinished, resampled by the tap loop of the prompt stage (resample.h) and stored as f32 or
// as the 16-bit view of generated audio (segments.h), for any output range whose taps are all there -- so that a stream delivered
// in pieces as it grows is, bit for bit, the stream delivered at once.  The arithmetic contract is in include/f5_hip.h; in short
//   wave_deliver_kernel   one block per run of output frames of an item: the window staged in LDS (the zero padding by index
//                         logic), then per output sample the taps in ascending order; a stream at the output rate passes through.
//                         A thread's four samples are aligned to the item's destination: one 16-byte (f32) or 8-byte (s16) store
//                         inside the range, element stores at its two edges.
#include "deliver.h"
#include "elementwise.h"
#include "mel_handle.h"

using namespace f5;
#define fail f5_fail

namespace {
struct DeliverTables {                        // items[B] | blk_start[B + 1]: one layout for the pinned slot and the device
    DeliverItem* items;
    int* blk_start;
    DeliverTables(char* base, int B) : items(reinterpret_cast<DeliverItem*>(base)), blk_start(reinterpret_cast<int*>(base + (size_t)B * sizeof(DeliverItem))) {}
    static size_t bytes(int B) { return (size_t)B * sizeof(DeliverItem) + ((size_t)B + 1) * 4; }
};
}  // namespace

static __global__ __launch_bounds__(256) void wave_deliver_kernel(const float* __restrict__ base, const DeliverItem* __restrict__ items,
                                                                  const int* __restrict__ blk_start, int B, int format, void* __restrict__ out) {
    __shared__ float xs[RS_LDS_FLOATS];
    const int blk = blockIdx.x;
    const int b = segment_of_row(blk_start, B, blk);
    const DeliverItem it = items[b];
    const float* x = base + it.in_start;
    const long long tile = blk - blk_start[b];
    const long long count = it.o1 - it.o0;          // > 0: the host gives an empty range no block

    if (it.orig == it.nw) {   // at the output rate: the sample itself
        const long long d = tile * RS_OUT_TILE + 4 * (long long)threadIdx.x;
        if (d >= count) return;
        float v[4];
        for (int q = 0; q < 4; ++q) v[q] = d + q < count ? x[it.o0 + d + q] : 0.f;   // o1 <= n
        store_quad(out, format, it.out_start, d, 0, count, v);
        return;
    }

    const DeliverWindow w = deliver_window(it, tile);
    for (int e = threadIdx.x; e < w.win; e += 256) {
        const long long j = w.win0 + e;
        xs[e] = (j >= 0 && j < it.n) ? x[j] : 0.f;
    }
    __syncthreads();
    deliver_from_window(it, w.frame0, xs, format, out);
}

extern "C" int f5_wave_deliver_plan(int32_t out_rate, int64_t n, int32_t final, int64_t* len_out, int64_t* ready_out) {
    const char* who = "f5_wave_deliver_plan";
    if (!len_out) return fail(F5_EINVAL, "%s: null len_out", who);
    if (!ready_out) return fail(F5_EINVAL, "%s: null ready_out", who);
    if (n < 0 || n > INT32_MAX) return fail(F5_EINVAL, "%s: n = %lld samples (need 0 <= n < 2^31)", who, (long long)n);
    RatePair r;
    CHK(deliver_rate(who, out_rate, &r));
    long long len = 0, ready = 0;
    deliver_lengths(r, n, final != 0, &len, &ready);
    *len_out = len;
    *ready_out = ready;
    return F5_OK;
}

extern "C" int f5_wave_deliver(f5_mel* m, const float* base, int32_t B, const int64_t* start_host, const int32_t* n_host,
                               const int32_t* final_host, const int64_t* o0_host, const int64_t* o1_host, int32_t out_rate,
                               int32_t format, void* out, int64_t out_capacity, int64_t* out_start_out, f5_stream stream) {
    const char* who = "f5_wave_deliver";
    if (!m) return fail(F5_EINVAL, "%s: null handle m", who);
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!n_host) return fail(F5_EINVAL, "%s: null n_host", who);
    if (!final_host) return fail(F5_EINVAL, "%s: null final_host", who);
    if (!o0_host) return fail(F5_EINVAL, "%s: null o0_host", who);
    if (!o1_host) return fail(F5_EINVAL, "%s: null o1_host", who);
    if (!out) return fail(F5_EINVAL, "%s: null out", who);
    if (!out_start_out) return fail(F5_EINVAL, "%s: null out_start_out", who);
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 items (B = %d)", who, B);
    if (format != F5_PCM_F32 && format != F5_PCM_S16) return fail(F5_EINVAL, "%s: unknown format %d (F5_PCM_F32 or F5_PCM_S16)", who, format);
    RatePair r;
    CHK(deliver_rate(who, out_rate, &r));
    const int F = r.same() ? 0 : frames_per_block(r);
    const int per16 = format == F5_PCM_F32 ? 4 : 8;   // elements per 16 bytes: where an item may start
    std::vector<int> blk_start((size_t)B + 1);
    std::vector<long long> at((size_t)B);
    long long blks = 0, run = 0;
    for (int b = 0; b < B; ++b) {
        if (start_host[b] < 0) return fail(F5_EINVAL, "%s: item %d starts at start = %lld < 0", who, b, (long long)start_host[b]);
        if (n_host[b] < 0) return fail(F5_EINVAL, "%s: item %d has n = %d samples (need n >= 0)", who, b, n_host[b]);
        long long len = 0, ready = 0;
        deliver_lengths(r, n_host[b], final_host[b] != 0, &len, &ready);
        const long long o0 = o0_host[b], o1 = o1_host[b];
        if (o0 < 0 || o1 < o0 || o1 > ready)
            return fail(F5_EINVAL, "%s: item %d: the range [%lld, %lld) is outside [0, ready = %lld] (%d samples, %s)", who, b, o0, o1, ready,
                        n_host[b], final_host[b] ? "final" : "not final");
        run = (run + per16 - 1) / per16 * per16;
        at[b] = run;
        run += o1 - o0;
        blk_start[b] = (int)blks;
        if (o1 > o0) blks += deliver_blocks(r, F, o0, o1);
        if (blks > DELIVER_MAX_UNITS) return fail(F5_EINVAL, "%s: more than 2^30 blocks of work at item %d (split the batch)", who, b);
    }
    blk_start[B] = (int)blks;
    if (out_capacity < run)
        return fail(F5_EINVAL, "%s: out_capacity = %lld is less than the plan's total of %lld elements", who, (long long)out_capacity, run);
    const float* bank = nullptr;
    if (!r.same()) {
        auto it = m->bank_of.find(std::make_pair(r.orig, r.nw));
        if (it == m->bank_of.end())
            return fail(F5_ESTATE, "%s: no resample bank for %d Hz -> %d Hz yet (f5_mel_resample_bank)", who, DELIVER_STREAM_RATE, out_rate);
        bank = it->second;
    }
    for (int b = 0; b < B; ++b) out_start_out[b] = at[b];
    if (blks == 0) return F5_OK;

    hipStream_t s = (hipStream_t)stream;
    char* tab = nullptr;
    auto plan = [&](Arena& a) {
        a.reset();
        tab = a.take<char>(DeliverTables::bytes(B));
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(m->arena.reserve(plan(dry)));
    (void)plan(m->arena);
    CHK(m->stage.upload(tab, DeliverTables::bytes(B), s, [&](char* host) {
        const DeliverTables h(host, B);
        for (int b = 0; b < B; ++b) {
            h.items[b] = DeliverItem{start_host[b], at[b], o0_host[b], o1_host[b], bank, n_host[b], r.orig, r.nw, r.width, r.K, F};
            h.blk_start[b] = blk_start[b];
        }
        h.blk_start[B] = blk_start[B];
    }));
    const DeliverTables d(tab, B);
    hipLaunchKernelGGL(wave_deliver_kernel, dim3((unsigned)blks), dim3(256), 0, s, base, d.items, d.blk_start, B, format, out);
    KCHK();
    return F5_OK;
}
