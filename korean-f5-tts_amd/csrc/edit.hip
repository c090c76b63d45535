// Speech editing on gfx950 (infer/speech_edit.py): the two data movements around CFM.sample(edit_mask=...).
//   f5_edit_assemble  the conditioning mel of a batch of recordings from their original mels: the script's torch.cat chain
//                     (speech_edit.py:157-195) as one launch -- every output frame is a bit copy of its source frame or +0.0;
//   f5_wave_splice    outside the edited spans, the original recording instead of the vocoder's resynthesis of it, with a short
//                     linear cross-fade at every inner boundary (no reference counterpart; the contract is in include/f5_hip.h).
// Both take the segment table of every item from the host, validate it there (segments.h), and hand it to the kernel as every
// ragged stage does: a table layout carved out of the workspace of the handle-less calls (CallState, internal.h), filled through one
// pinned slot and one copy: no synchronisation unless the workspace grows, nothing of the caller's to keep alive.
// Built with -ffp-contract=off: the fade is multiply, multiply, add as written, in double.
#include <cstdint>

#include "segments.h"

#define fail f5_fail

namespace {
constexpr int kMaxItems = 64;
constexpr int kMaxSegs = 33;                        // 16 parts: 17 KEEP and 16 EDIT segments per item
constexpr int kThreads = 256;
constexpr int kPerThread = 4;                       // consecutive f32 per thread: one 16-byte access
constexpr int kTile = kThreads * kPerThread;

struct SpliceSeg {                                  // a KEEP segment in samples, clipped (include/f5_hip.h)
    long long p0, p1, q0;                           // claims out[p0, p1); the source of p is a[q0 + (p - p0)]
    double step;                                    // 1 / (m - 1): linspace's step (0 for m < 2)
    int m;                                          // fade length
    int ends;                                       // bit 0: the head fades in, bit 1: the tail fades out
};

// the device tables of one call, one layout for slot and device; item b owns seg[first[b] .. first[b + 1])
struct AssembleTables {                             // first[B + 1] | seg[nseg]
    int* first;
    Seg* seg;
    AssembleTables(char* base, int B) : first(reinterpret_cast<int*>(base)), seg(reinterpret_cast<Seg*>(first + B + 1)) {}
    static size_t bytes(int B, int nseg) { return ((size_t)B + 1) * 4 + (size_t)std::max(nseg, 1) * sizeof(Seg); }
};
struct SpliceTables {                               // a_start[B] | seg[nseg] | first[B + 1] | len[B]: the 8-byte entries first
    long long* a_start;
    SpliceSeg* seg;
    int* first;
    int* len;                                       // L_b
    SpliceTables(char* base, int B, int nseg)
        : a_start(reinterpret_cast<long long*>(base)), seg(reinterpret_cast<SpliceSeg*>(a_start + B)),
          first(reinterpret_cast<int*>(seg + std::max(nseg, 1))), len(first + B + 1) {}
    static size_t bytes(int B, int nseg) { return (size_t)B * 8 + (size_t)std::max(nseg, 1) * sizeof(SpliceSeg) + (2 * (size_t)B + 1) * 4; }
};
static_assert(sizeof(SpliceSeg) % 8 == 0, "first follows the segments; the segments follow a_start and are 8-byte aligned");

// ---------------------------------------------------------------------------------------------------- assembly
// One thread per 16 bytes of the output (VEC) or per element; blockIdx.y is the item.  A frame that no segment covers, an EDIT
// frame and a frame behind D_b are the same thing here: +0.0.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void edit_assemble_kernel(const float* __restrict__ mel, long long mel_stride, int row,
                                                                 const int* __restrict__ first, const Seg* __restrict__ segs,
                                                                 float* __restrict__ cond, int D_max) {
    const int b = blockIdx.y;
    const int per_row = VEC ? row / 4 : row;        // work items per frame
    const long long n = (long long)D_max * per_row;
    const Seg* my = segs + first[b];
    const int count = first[b + 1] - first[b];
    const float* src_item = mel + (long long)b * mel_stride;
    float* dst_item = cond + (long long)b * D_max * row;
    int hint = -1;
    for (long long w = (long long)blockIdx.x * kThreads + threadIdx.x; w < n; w += (long long)gridDim.x * kThreads) {
        const int d = (int)(w / per_row), c = (int)(w % per_row);
        const int from = source_frame(my, count, d, &hint);
        if (VEC) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (from >= 0) v = *reinterpret_cast<const float4*>(src_item + (long long)from * row + 4 * c);
            *reinterpret_cast<float4*>(dst_item + (long long)d * row + 4 * c) = v;
        } else {
            dst_item[(long long)d * row + c] = from >= 0 ? src_item[(long long)from * row + c] : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- splice
__global__ __launch_bounds__(kThreads) void wave_splice_kernel(const float* __restrict__ gen, long long gen_stride,
                                                               const float* __restrict__ a_base,
                                                               const long long* __restrict__ a_start,
                                                               const SpliceSeg* __restrict__ segs, const int* __restrict__ first,
                                                               const int* __restrict__ len, float* __restrict__ out,
                                                               long long out_stride) {
    const int b = blockIdx.y;
    const long long L = len[b];
    const int s0 = first[b], s1 = first[b + 1];
    const float* g = gen + (long long)b * gen_stride;
    const float* a = a_base + a_start[b];
    float* orow = out + (long long)b * out_stride;
    const long long ntiles = (out_stride + kTile - 1) / kTile;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long pb = tile * kTile + (long long)threadIdx.x * kPerThread;
        if (pb >= out_stride) continue;
        float v[kPerThread];
#pragma unroll
        for (int e = 0; e < kPerThread; ++e) {
            const long long p = pb + e;
            v[e] = p < L ? g[p] : 0.0f;              // nothing at or past L of the generated row is read
        }
        for (int s = s0; s < s1; ++s) {
            const SpliceSeg k = segs[s];
            if (k.p1 <= pb || k.p0 >= pb + kPerThread) continue;
#pragma unroll
            for (int e = 0; e < kPerThread; ++e) {
                const long long p = pb + e;
                if (p < k.p0 || p >= k.p1) continue;
                const float av = a[k.q0 + (p - k.p0)];   // q < n_b: p1 is clipped to the original's length
                const long long jh = p - k.p0, jt = k.p1 - 1 - p;
                long long j = -1;
                if ((k.ends & 1) && jh < k.m) j = jh;
                else if ((k.ends & 2) && jt < k.m) j = jt;
                if (j < 0) {
                    v[e] = av;
                } else {
                    double fi, fo;
                    fade_weights(j, k.m, k.step, &fi, &fo);
                    v[e] = (float)((double)v[e] * fo + (double)av * fi);
                }
            }
        }
        float* o = orow + pb;
        if (pb + kPerThread <= out_stride && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < kPerThread; ++e)
                if (pb + e < out_stride) o[e] = v[e];
        }
    }
}
}  // namespace

extern "C" int f5_edit_assemble(const float* mel, int32_t B, int64_t mel_stride, int32_t row, const int32_t* frames_host,
                                const int32_t* seg_count_host, const int32_t* segs_host, const int32_t* dur_host, float* cond,
                                int32_t D_max, f5_stream stream) {
    const char* who = "f5_edit_assemble";
    if (B < 1 || B > kMaxItems) return fail(F5_EINVAL, "%s: need 1 <= B <= %d items (B = %d)", who, kMaxItems, B);
    if (!mel) return fail(F5_EINVAL, "%s: mel is null", who);
    if (!frames_host) return fail(F5_EINVAL, "%s: frames_host is null", who);
    if (!seg_count_host) return fail(F5_EINVAL, "%s: seg_count_host is null", who);
    if (!segs_host) return fail(F5_EINVAL, "%s: segs_host is null", who);
    if (!dur_host) return fail(F5_EINVAL, "%s: dur_host is null", who);
    if (!cond) return fail(F5_EINVAL, "%s: cond is null", who);
    if (row < 1 || D_max < 1) return fail(F5_EINVAL, "%s: row %d, D_max %d; need at least 1 of each", who, row, D_max);
    std::vector<int> first((size_t)B + 1);
    int total = 0;
    for (int b = 0; b < B; ++b) {
        const int T = frames_host[b], D = dur_host[b], count = seg_count_host[b];
        if (T < 0 || (long long)T * row > mel_stride)
            return fail(F5_EINVAL, "%s: item %d has %d frames of %d; its stride is %lld elements", who, b, T, row, (long long)mel_stride);
        if (D < 0 || D > D_max) return fail(F5_EINVAL, "%s: item %d has %d output frames; D_max is %d", who, b, D, D_max);
        if (count < 0 || count > kMaxSegs)
            return fail(F5_EINVAL, "%s: item %d has %d segments; at most %d", who, b, count, kMaxSegs);
        const int32_t* segs = segs_host + 3 * (size_t)total;
        CHK(check_segments(who, b, segs, count, -1, INT32_MAX));
        for (int s = 0; s < count; ++s) {
            const long long dst = segs[3 * s], src = segs[3 * s + 1], frames = segs[3 * s + 2];
            if (dst + frames > D)
                return fail(F5_EINVAL, "%s: item %d segment %d writes frames [%lld, %lld); the item has %d of D_max %d", who, b, s, dst,
                            dst + frames, D, D_max);
            if (src >= 0 && src + frames > T)
                return fail(F5_EINVAL, "%s: item %d segment %d reads frames [%lld, %lld) of %d", who, b, s, src, src + frames, T);
        }
        first[b] = total;
        total += count;
    }
    first[B] = total;
    const size_t tab_bytes = AssembleTables::bytes(B, total);

    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        const AssembleTables h(host, B);
        for (int b = 0; b <= B; ++b) h.first[b] = first[b];
        for (int k = 0; k < total; ++k) h.seg[k] = Seg{segs_host[3 * k], segs_host[3 * k + 1], segs_host[3 * k + 2]};
    }));
    const AssembleTables d(tab, B);
    const bool vec = row % 4 == 0 && mel_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(mel) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(cond) & 15) == 0;
    const long long n = (long long)D_max * (vec ? row / 4 : row);
    const dim3 grid((unsigned)std::min<long long>((n + kThreads - 1) / kThreads, 4096), (unsigned)B);
    if (vec)
        edit_assemble_kernel<true><<<grid, kThreads, 0, s>>>(mel, (long long)mel_stride, row, d.first, d.seg, cond, D_max);
    else
        edit_assemble_kernel<false><<<grid, kThreads, 0, s>>>(mel, (long long)mel_stride, row, d.first, d.seg, cond, D_max);
    KCHK();
    return st->leave(s);
}

extern "C" int f5_wave_splice(const float* gen, int32_t B, int64_t gen_stride, const int32_t* len_host, const float* a_base,
                              const int64_t* a_start_host, const int32_t* a_len_host, const int32_t* seg_count_host,
                              const int32_t* segs_host, int32_t hop, int32_t cross_fade_samples, float* out, int64_t out_stride,
                              f5_stream stream) {
    const char* who = "f5_wave_splice";
    if (B < 1 || B > kMaxItems) return fail(F5_EINVAL, "%s: need 1 <= B <= %d items (B = %d)", who, kMaxItems, B);
    if (!gen) return fail(F5_EINVAL, "%s: gen is null", who);
    if (!len_host) return fail(F5_EINVAL, "%s: len_host is null", who);
    if (!a_base) return fail(F5_EINVAL, "%s: a_base is null", who);
    if (!a_start_host) return fail(F5_EINVAL, "%s: a_start_host is null", who);
    if (!a_len_host) return fail(F5_EINVAL, "%s: a_len_host is null", who);
    if (!seg_count_host) return fail(F5_EINVAL, "%s: seg_count_host is null", who);
    if (!segs_host) return fail(F5_EINVAL, "%s: segs_host is null", who);
    if (!out) return fail(F5_EINVAL, "%s: out is null", who);
    if (hop < 1 || hop > 65536) return fail(F5_EINVAL, "%s: hop %d; need 1 <= hop <= 65536", who, hop);
    if (cross_fade_samples < 0) return fail(F5_EINVAL, "%s: cross_fade_samples %d is negative", who, cross_fade_samples);
    if (out_stride < 1) return fail(F5_EINVAL, "%s: out_stride %lld; need at least 1", who, (long long)out_stride);
    std::vector<int> first((size_t)B + 1);
    std::vector<SpliceSeg> kept;
    int given = 0;
    for (int b = 0; b < B; ++b) {
        const long long L = len_host[b], n = a_len_host[b];
        const int count = seg_count_host[b];
        if (L < 0 || L > gen_stride || L > out_stride)
            return fail(F5_EINVAL, "%s: item %d has %lld samples; the row strides are %lld (gen) and %lld (out)", who, b, L,
                        (long long)gen_stride, (long long)out_stride);
        if (n < 0 || a_start_host[b] < 0)
            return fail(F5_EINVAL, "%s: item %d's original has %lld samples at offset %lld", who, b, n, (long long)a_start_host[b]);
        if (count < 0 || count > kMaxSegs)
            return fail(F5_EINVAL, "%s: item %d has %d segments; at most %d", who, b, count, kMaxSegs);
        const int32_t* segs = segs_host + 3 * (size_t)given;
        CHK(check_segments(who, b, segs, count, 0, INT32_MAX));
        first[b] = (int)kept.size();
        for (int s = 0; s < count; ++s) {
            const long long dst = segs[3 * s], src = segs[3 * s + 1], frames = segs[3 * s + 2];
            SpliceSeg k{};
            k.p0 = dst * hop;
            k.q0 = src * hop;
            k.p1 = std::min(std::min((dst + frames) * hop, L), k.p0 + n - k.q0);
            if (k.p1 <= k.p0) continue;             // nothing left of it after clipping
            k.m = (int)std::min<long long>(cross_fade_samples, (k.p1 - k.p0) / 2);
            k.ends = (k.p0 > 0 ? 1 : 0) | (k.p1 < L ? 2 : 0);
            k.step = k.m > 1 ? 1.0 / (double)(k.m - 1) : 0.0;
            kept.push_back(k);
        }
        given += count;
    }
    const int total = (int)kept.size();
    first[B] = total;
    const size_t tab_bytes = SpliceTables::bytes(B, total);

    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        const SpliceTables h(host, B, total);
        for (int b = 0; b < B; ++b) h.a_start[b] = a_start_host[b], h.len[b] = len_host[b];
        for (int b = 0; b <= B; ++b) h.first[b] = first[b];
        for (int k = 0; k < total; ++k) h.seg[k] = kept[k];
    }));
    const SpliceTables d(tab, B, total);
    const long long ntiles = (out_stride + kTile - 1) / kTile;
    const dim3 grid((unsigned)std::min<long long>(ntiles, 2048), (unsigned)B);
    wave_splice_kernel<<<grid, kThreads, 0, s>>>(gen, (long long)gen_stride, a_base, d.a_start, d.seg, d.first, d.len, out,
                                                 (long long)out_stride);
    KCHK();
    return st->leave(s);
}
