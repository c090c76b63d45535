// Join and delivery for many streams in one launch (what a server tick needs: every client's new audio, each at its own rate and
// sample format).  f5_wave_emit composes f5_wave_join (join.h) and f5_wave_deliver (deliver.h) per stream without ever writing the
// joined waveform: the arithmetic contract is in include/f5_hip.h; in short
//   wave_emit_kernel   one block per run of output frames of a stream, as in wave_deliver_kernel, but the block's window is folded
//                      from the stream's pieces: bisection to the first piece that reaches into the window, then per quad of
//                      window samples the fold in double over the covering pieces, rounded to f32 once into LDS.  From there on
//                      the block is deliver.hip's: the taps in ascending order, the quads aligned to the stream's destination.
//                      A stream at the output rate folds its four samples and stores them.
// Streams of different rates and formats share the launch: the geometry, the bank and the format travel in the stream's item.
#include "deliver.h"
#include "elementwise.h"
#include "join.h"
#include "mel_handle.h"

using namespace f5;
#define fail f5_fail

namespace {
struct EmitItem {
    DeliverItem d;                            // n = the settled samples; out_start in elements of the format; in_start unused
    int piece0, pieces, format, pad;          // the stream's pieces in the table
};
struct EmitTables {                           // pieces[P] | items[S] | blk_start[S + 1]: one layout for the pinned slot and the device
    JoinPiece* pieces;
    EmitItem* items;
    int* blk_start;
    EmitTables(char* base, int P, int S)
        : pieces(reinterpret_cast<JoinPiece*>(base)), items(reinterpret_cast<EmitItem*>(base + (size_t)P * sizeof(JoinPiece))),
          blk_start(reinterpret_cast<int*>(base + (size_t)P * sizeof(JoinPiece) + (size_t)S * sizeof(EmitItem))) {}
    static size_t bytes(int P, int S) { return (size_t)P * sizeof(JoinPiece) + (size_t)S * sizeof(EmitItem) + ((size_t)S + 1) * 4; }
};
static_assert(sizeof(JoinPiece) % 8 == 0 && sizeof(EmitItem) % 8 == 0, "the tables follow each other without padding");
}  // namespace

static __global__ __launch_bounds__(256) void wave_emit_kernel(const float* __restrict__ base, const JoinPiece* __restrict__ pieces,
                                                               const EmitItem* __restrict__ items, const int* __restrict__ blk_start, int S,
                                                               void* __restrict__ out) {
    __shared__ float xs[RS_LDS_FLOATS];
    const int blk = blockIdx.x;
    const int s = segment_of_row(blk_start, S, blk);
    const EmitItem item = items[s];
    const DeliverItem& it = item.d;
    const JoinPiece* pcs = pieces + item.piece0;
    const long long tile = blk - blk_start[s];
    const long long count = it.o1 - it.o0;          // > 0: the host gives an empty range no block

    if (it.orig == it.nw) {   // at the output rate: the joined sample itself
        const long long t0 = it.o0 + tile * RS_OUT_TILE;                      // the block's span (block-uniform); t0 < o1 <= n <= total
        const long long d = tile * RS_OUT_TILE + 4 * (long long)threadIdx.x;
        if (d >= count) return;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        fold_pieces(base, pcs, item.pieces, first_piece(pcs, item.pieces, t0), t0 + RS_OUT_TILE, it.o0 + d, v);
        const float f[4] = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        store_quad(out, item.format, it.out_start, d, 0, count, f);
        return;
    }

    const DeliverWindow w = deliver_window(it, tile);
    const long long w0 = max(w.win0, 0LL), w1 = min(w.win0 + w.win, (long long)it.n);   // the window inside the settled stream
    const int lo = w0 < w1 ? first_piece(pcs, item.pieces, w0) : 0;
    for (int e0 = 4 * threadIdx.x; e0 < w.win; e0 += RS_OUT_TILE) {
        const long long p0 = w.win0 + e0;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (p0 < w1 && p0 + 4 > w0) fold_pieces(base, pcs, item.pieces, lo, w1, p0, v);
        for (int q = 0; q < 4; ++q)
            if (e0 + q < w.win) xs[e0 + q] = (p0 + q >= 0 && p0 + q < it.n) ? (float)v[q] : 0.f;
    }
    __syncthreads();
    deliver_from_window(it, w.frame0, xs, item.format, out);
}

extern "C" int f5_wave_emit(f5_mel* m, const float* base, int32_t S, const int32_t* piece_count_host, const int64_t* start_host,
                            const int32_t* lens_host, const int32_t* fade_host, const int64_t* settled_host, const int32_t* final_host,
                            const int64_t* o0_host, const int64_t* o1_host, const int32_t* rate_host, const int32_t* format_host, void* out,
                            int64_t out_capacity_bytes, int64_t* out_start_bytes_out, f5_stream stream) {
    const char* who = "f5_wave_emit";
    if (!m) return fail(F5_EINVAL, "%s: null handle m", who);
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!piece_count_host) return fail(F5_EINVAL, "%s: null piece_count_host", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!lens_host) return fail(F5_EINVAL, "%s: null lens_host", who);
    if (!fade_host) return fail(F5_EINVAL, "%s: null fade_host", who);
    if (!settled_host) return fail(F5_EINVAL, "%s: null settled_host", who);
    if (!final_host) return fail(F5_EINVAL, "%s: null final_host", who);
    if (!o0_host) return fail(F5_EINVAL, "%s: null o0_host", who);
    if (!o1_host) return fail(F5_EINVAL, "%s: null o1_host", who);
    if (!rate_host) return fail(F5_EINVAL, "%s: null rate_host", who);
    if (!format_host) return fail(F5_EINVAL, "%s: null format_host", who);
    if (!out) return fail(F5_EINVAL, "%s: null out", who);
    if (!out_start_bytes_out) return fail(F5_EINVAL, "%s: null out_start_bytes_out", who);
    if (S < 1 || S > 65535) return fail(F5_EINVAL, "%s: need 1 <= S <= 65535 streams (S = %d)", who, S);
    long long P = 0;
    for (int s = 0; s < S; ++s) {
        if (piece_count_host[s] < 1) return fail(F5_EINVAL, "%s: stream %d has piece_count = %d (need at least 1 piece)", who, s, piece_count_host[s]);
        P += piece_count_host[s];
        if (P > 65535) return fail(F5_EINVAL, "%s: more than 65535 pieces in all at stream %d (split the call)", who, s);
    }

    std::vector<JoinPiece> pieces((size_t)P);
    std::vector<EmitItem> items((size_t)S);
    std::vector<int> blk_start((size_t)S + 1);
    std::vector<RatePair> rates((size_t)S);
    long long blks = 0, run = 0;                                  // blocks; bytes of out
    int at = 0;                                                   // the stream's first piece
    for (int s = 0; s < S; ++s) {
        const int count = piece_count_host[s];
        JoinRun join;
        for (int i = 0; i < count; ++i) {
            const int g = at + i, len = lens_host[g], fade = fade_host[g];
            if (len < 1)
                return fail(F5_EINVAL, "%s: stream %d piece %d: lens_host[%d] = %d; every piece needs at least 1 sample", who, s, i, g, len);
            if (fade < 0) return fail(F5_EINVAL, "%s: stream %d piece %d: fade_host[%d] = %d < 0", who, s, i, g, fade);
            if (start_host[g] < 0)
                return fail(F5_EINVAL, "%s: stream %d piece %d: start_host[%d] = %lld < 0", who, s, i, g, (long long)start_host[g]);
            join.place(i == 0, start_host[g], len, fade, &pieces[(size_t)g]);
        }
        join.close(&pieces[(size_t)at], count);
        const long long total = join.L, n = settled_host[s];
        if (n < 0 || n > total)
            return fail(F5_EINVAL, "%s: stream %d: settled = %lld is outside [0, total = %lld]", who, s, n, total);
        if (n > INT32_MAX) return fail(F5_EINVAL, "%s: stream %d: settled = %lld samples (need settled < 2^31)", who, s, n);
        const int format = format_host[s];
        if (format != F5_PCM_F32 && format != F5_PCM_S16)
            return fail(F5_EINVAL, "%s: stream %d: unknown format %d (F5_PCM_F32 or F5_PCM_S16)", who, s, format);
        char who_s[48];
        snprintf(who_s, sizeof(who_s), "%s: stream %d", who, s);
        RatePair& r = rates[(size_t)s];
        CHK(deliver_rate(who_s, rate_host[s], &r));
        const int F = r.same() ? 0 : frames_per_block(r);
        long long len = 0, ready = 0;
        deliver_lengths(r, n, final_host[s] != 0, &len, &ready);
        const long long o0 = o0_host[s], o1 = o1_host[s];
        if (o0 < 0 || o1 < o0 || o1 > ready)
            return fail(F5_EINVAL, "%s: stream %d: the range [%lld, %lld) is outside [0, ready = %lld] (%lld settled samples, %s)", who, s, o0, o1,
                        ready, n, final_host[s] ? "final" : "not final");
        const int elem = format == F5_PCM_F32 ? 4 : 2;
        run = (run + 15) / 16 * 16;
        items[(size_t)s] = EmitItem{DeliverItem{0, run / elem, o0, o1, nullptr, (int)n, r.orig, r.nw, r.width, r.K, F}, at, count, format, 0};
        run += (o1 - o0) * elem;
        blk_start[(size_t)s] = (int)blks;
        if (o1 > o0) blks += deliver_blocks(r, F, o0, o1);
        if (blks > DELIVER_MAX_UNITS) return fail(F5_EINVAL, "%s: more than 2^30 blocks of work at stream %d (split the call)", who, s);
        at += count;
    }
    blk_start[(size_t)S] = (int)blks;
    if (out_capacity_bytes < run)
        return fail(F5_EINVAL, "%s: out_capacity_bytes = %lld is less than the plan's total of %lld bytes", who, (long long)out_capacity_bytes, run);
    for (int s = 0; s < S; ++s) {
        const RatePair& r = rates[(size_t)s];
        if (r.same()) continue;
        auto it = m->bank_of.find(std::make_pair(r.orig, r.nw));
        if (it == m->bank_of.end())
            return fail(F5_ESTATE, "%s: stream %d: no resample bank for %d Hz -> %d Hz yet (f5_mel_resample_bank)", who, s, DELIVER_STREAM_RATE,
                        rate_host[s]);
        items[(size_t)s].d.bank = it->second;
    }
    for (int s = 0; s < S; ++s) out_start_bytes_out[s] = items[(size_t)s].d.out_start * (items[(size_t)s].format == F5_PCM_F32 ? 4 : 2);
    if (blks == 0) return F5_OK;

    hipStream_t hs = (hipStream_t)stream;
    const size_t tab_bytes = EmitTables::bytes((int)P, S);
    char* tab = nullptr;
    auto plan = [&](Arena& a) {
        a.reset();
        tab = a.take<char>(tab_bytes);
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(m->arena.reserve(plan(dry)));
    (void)plan(m->arena);
    CHK(m->stage.upload(tab, tab_bytes, hs, [&](char* host) {
        const EmitTables h(host, (int)P, S);
        __builtin_memcpy(h.pieces, pieces.data(), (size_t)P * sizeof(JoinPiece));
        __builtin_memcpy(h.items, items.data(), (size_t)S * sizeof(EmitItem));
        __builtin_memcpy(h.blk_start, blk_start.data(), ((size_t)S + 1) * 4);
    }));
    const EmitTables d(tab, (int)P, S);
    hipLaunchKernelGGL(wave_emit_kernel, dim3((unsigned)blks), dim3(256), 0, hs, base, d.pieces, d.items, d.blk_start, S, out);
    KCHK();
    return F5_OK;
}
