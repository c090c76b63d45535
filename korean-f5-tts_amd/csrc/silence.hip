// Silence clipping on gfx950 (infer/utils_infer.py:348-361, 385-419, 784-793: pydub's detect_silence / split_on_silence /
// detect_leading_silence and the per-millisecond loop of remove_silence_edges, on the 16-bit view of f32 audio).  The arithmetic
// contract is in include/f5_hip.h; every decision is exact integer arithmetic, so a result does not depend on a reduction order.
//   silence_energy_kernel     one block per tile of 256 milliseconds of an item: 16 lanes share a millisecond, add the squares of
//                             its 16-bit samples over all channels in int64 and fold them with shuffles; the block also adds its
//                             256 energies into the tile's sum.  The only kernel that reads the audio: 16-byte loads where the
//                             rows are aligned, element loads otherwise or through a segment table, the same integers either way
//   silence_tile_scan_kernel  one block per item: the exclusive prefix of its tiles' sums, 256 at a time with a carry
//   silence_prefix_kernel     one block per tile: the exclusive prefix of its energies plus the tile's offset, in place
//   silence_flags_kernel      one thread per flag of every (item, query): E = P[end] - P[start] against cnt * (T + 1)^2
//   wave_gather_kernel        the clipped waveform: every output frame is q / 32768 of its source frame, or +0.0
// The scan is the plain three-phase one (tile sums, scan of tile sums, apply): no workgroup ever waits for another.  No atomics.
// The per-call tables (items, tile and flag offsets, the segment tables) go through one pinned slot and one copy into the
// workspace of the handle-less calls (CallState, internal.h), which grows with use; no host read and no synchronisation otherwise.
#include <cmath>
#include <cstdint>

#include "segments.h"

#define fail f5_fail

namespace {
constexpr int kThreads = 256;
constexpr int kTile = 256;                          // prefix slots of a tile: one per thread
constexpr int kGroup = 16;                          // lanes that share one millisecond
constexpr int kMaxQueries = 8;
constexpr int kOutTile = kThreads * 4;              // output frames of a gather block: one 16-byte store per thread
constexpr long long kMaxSlots = 1LL << 30;          // prefix slots / gather tiles of one call (grid sizes are int)
constexpr int kMaxMs = 1 << 24;

struct Query {
    int W, s, T, kind;
};
struct Queries {
    Query q[kMaxQueries];
};
struct Item {
    long long in_start;                             // elements from base
    long long slot_start;                           // analyse: first prefix slot; gather: first output element
    int C, F, R, L;                                 // gather: L = F_out
    int seg_first, seg_count;                       // seg_count < 0: identity
    int vec, pad;                                   // analyse: the rows are 16-byte aligned
};

__host__ __device__ __forceinline__ long long ms_pos(int R, long long ms) { return ((long long)R * ms) / 1000; }

// the last entry of start[0 .. n) that is <= r (start is ascending, start[0] <= r)
template <typename T> __device__ __forceinline__ int last_not_above(const T* __restrict__ start, int n, T r) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// inclusive scan over the block's 256 values (Hillis-Steele in LDS); every thread of the block calls it
__device__ __forceinline__ long long block_inclusive_scan(long long v, long long* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const long long a = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const long long r = sh[t];
    __syncthreads();
    return r;
}

template <bool MAPPED>
__global__ __launch_bounds__(kThreads) void silence_energy_kernel(const float* __restrict__ base, const Item* __restrict__ items,
                                                                  const int* __restrict__ tile_start, int B,
                                                                  const Seg* __restrict__ segs, float qscale,
                                                                  long long* __restrict__ slots, long long* __restrict__ tile_sum) {
    __shared__ long long red[kThreads / 64];
    const int tile = blockIdx.x;
    const int b = last_not_above(tile_start, B, tile);
    const Item it = items[b];
    const float* x = base + it.in_start;
    const int m0 = (tile - tile_start[b]) * kTile;
    const int g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const Seg* my = segs + it.seg_first;
    long long mine = 0;                             // the energy of slot m0 + threadIdx.x
    for (int i = 0; i < kGroup; ++i) {
        const int m = m0 + g * kGroup + i;
        long long e = 0;
        if (m < it.L) {                             // (slot L is the zero that closes the prefix)
            const int f0 = (int)ms_pos(it.R, m), f1 = (int)ms_pos(it.R, m + 1);
            if (MAPPED) {
                int hint = -1;
                for (int f = f0 + lane; f < f1; f += kGroup) {
                    const int src = source_frame(my, it.seg_count, f, &hint);
                    if (src < 0 || src >= it.F) continue;
                    for (int c = 0; c < it.C; ++c) {
                        const int q = quantise(x[(size_t)c * it.F + src], qscale);
                        e += (long long)(q * q);
                    }
                }
            } else if (it.vec) {                    // F % 4 == 0: a quad that starts inside a row lies inside it
                const int k1 = (f1 + 3) >> 2;
                for (int k = (f0 >> 2) + lane; k < k1; k += kGroup) {
                    const int fb = 4 * k;
                    if (fb >= it.F) break;
                    for (int c = 0; c < it.C; ++c) {
                        const float4 v = *reinterpret_cast<const float4*>(x + (size_t)c * it.F + fb);
                        const float w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (fb + j < f0 || fb + j >= f1) continue;
                            const int q = quantise(w[j], qscale);
                            e += (long long)(q * q);
                        }
                    }
                }
            } else {
                const int fe = min(f1, it.F);
                for (int f = f0 + lane; f < fe; f += kGroup) {
                    for (int c = 0; c < it.C; ++c) {
                        const int q = quantise(x[(size_t)c * it.F + f], qscale);
                        e += (long long)(q * q);
                    }
                }
            }
        }
        for (int off = kGroup / 2; off > 0; off >>= 1) e += __shfl_xor(e, off, kGroup);
        if (lane == i) mine = e;
    }
    const int slot = m0 + threadIdx.x;
    if (slot <= it.L) slots[it.slot_start + slot] = mine;
    long long sum = mine;
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[tile] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(kThreads) void silence_tile_scan_kernel(const int* __restrict__ tile_start, long long* __restrict__ tile_sum) {
    __shared__ long long sh[kThreads];
    const int t0 = tile_start[blockIdx.x], t1 = tile_start[blockIdx.x + 1];
    long long carry = 0;
    for (int c0 = t0; c0 < t1; c0 += kThreads) {    // (uniform over the block)
        const int idx = c0 + threadIdx.x;
        const long long v = idx < t1 ? tile_sum[idx] : 0;
        const long long incl = block_inclusive_scan(v, sh);
        if (idx < t1) tile_sum[idx] = carry + incl - v;
        carry += sh[kThreads - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void silence_prefix_kernel(const Item* __restrict__ items, const int* __restrict__ tile_start, int B,
                                                                 const long long* __restrict__ tile_sum, long long* __restrict__ slots) {
    __shared__ long long sh[kThreads];
    const int tile = blockIdx.x;
    const int b = last_not_above(tile_start, B, tile);
    const long long first = items[b].slot_start;
    const int L = items[b].L;
    const int slot = (tile - tile_start[b]) * kTile + threadIdx.x;
    const long long v = slot <= L ? slots[first + slot] : 0;
    const long long incl = block_inclusive_scan(v, sh);
    if (slot <= L) slots[first + slot] = tile_sum[tile] + incl - v;
}

__global__ __launch_bounds__(kThreads) void silence_flags_kernel(const Item* __restrict__ items, const long long* __restrict__ flag_first,
                                                                int pairs, int nq, Queries qs, const long long* __restrict__ prefix,
                                                                unsigned char* __restrict__ flags, long long total) {
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (long long)gridDim.x * kThreads) {
        const int k = last_not_above(flag_first, pairs, idx);
        const int b = k / nq;
        const Query q = qs.q[k - b * nq];
        const long long j = idx - flag_first[k];
        const int C = items[b].C, R = items[b].R, L = items[b].L;
        long long a = j * q.s;
        if (q.kind == 0 && a > L - q.W) a = L - q.W;   // the extra start behind the regular ones
        const long long e = min(a + (long long)q.W, (long long)L);
        const long long* P = prefix + items[b].slot_start;
        const long long E = P[e] - P[a];
        const long long cnt = (long long)C * (ms_pos(R, e) - ms_pos(R, a));
        const long long k1 = (long long)q.T + 1;
        flags[idx] = E < cnt * (k1 * k1) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void wave_gather_kernel(const float* __restrict__ base, const Item* __restrict__ items,
                                                              const int* __restrict__ tile_start, int B, const Seg* __restrict__ segs,
                                                              float qscale, float* __restrict__ out) {
    const int tile = blockIdx.x;
    const int b = last_not_above(tile_start, B, tile);
    const Item it = items[b];
    const int F_out = it.L;
    const int per_row = (F_out + kOutTile - 1) / kOutTile;
    const int tl = tile - tile_start[b];
    const int c = tl / per_row;
    const int o0 = (tl - c * per_row) * kOutTile + 4 * (int)threadIdx.x;
    if (o0 >= F_out) return;
    const float* x = base + it.in_start + (size_t)c * it.F;
    const Seg* my = segs + it.seg_first;
    float v[4];
    int hint = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = 0.0f;
        if (o0 + j >= F_out) continue;
        const int src = source_frame(my, it.seg_count, o0 + j, &hint);
        if (src >= 0 && src < it.F) v[j] = (float)quantise(x[src], qscale) / 32768.0f;
    }
    float* dst = out + it.slot_start + (size_t)c * F_out + o0;
    if (o0 + 4 <= F_out && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (o0 + j < F_out) dst[j] = v[j];
    }
}

// ---------------------------------------------------------------------------------------------------- host checks
int check_queries(const char* who, int nq, const int32_t* queries_host, Queries* out) {
    if (nq < 1 || nq > kMaxQueries) return fail(F5_EINVAL, "%s: need 1 <= nq <= %d queries (nq = %d)", who, kMaxQueries, nq);
    if (!queries_host) return fail(F5_EINVAL, "%s: null queries_host", who);
    for (int k = 0; k < nq; ++k) {
        const Query q{queries_host[4 * k], queries_host[4 * k + 1], queries_host[4 * k + 2], queries_host[4 * k + 3]};
        if (q.W < 1 || q.W > kMaxMs || q.s < 1 || q.s > kMaxMs)
            return fail(F5_EINVAL, "%s: query %d has W = %d, s = %d ms (need 1 <= W, s <= 2^24)", who, k, q.W, q.s);
        if (q.T < 0 || q.T > 32767) return fail(F5_EINVAL, "%s: query %d has threshold T = %d (need 0 <= T <= 32767)", who, k, q.T);
        if (q.kind != 0 && q.kind != 1) return fail(F5_EINVAL, "%s: query %d has kind = %d (0 or 1)", who, k, q.kind);
        if (out) out->q[k] = q;
    }
    return F5_OK;
}

long long flag_count(int L, const Query& q) {
    if (q.kind == 1) return ((long long)L + q.s - 1) / q.s;
    if (L < q.W) return 0;
    const long long last = (long long)L - q.W;
    return last / q.s + 1 + (last % q.s ? 1 : 0);
}

int plan_flags(const char* who, int B, const int32_t* len_ms_host, int nq, const int32_t* queries_host, int32_t* count_out,
               int64_t* start_out, int64_t* total_out, Queries* qs) {
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 items (B = %d)", who, B);
    if (!len_ms_host) return fail(F5_EINVAL, "%s: null len_ms_host", who);
    Queries local;
    CHK(check_queries(who, nq, queries_host, &local));
    if (qs) *qs = local;
    int64_t run = 0;
    for (int b = 0; b < B; ++b) {
        const int L = len_ms_host[b];
        if (L < 0 || L > kMaxMs) return fail(F5_EINVAL, "%s: item %d has L = %d ms (need 0 <= L <= 2^24)", who, b, L);
        for (int k = 0; k < nq; ++k) {
            const long long n = flag_count(L, local.q[k]);
            if (count_out) count_out[(size_t)b * nq + k] = (int32_t)n;
            if (start_out) start_out[(size_t)b * nq + k] = run;
            run += n;
        }
    }
    *total_out = run;
    return F5_OK;
}

// what analyse and gather ask of every item, and of its segment table where there is one (*given: segments consumed so far)
int check_item(const char* who, int b, int64_t start, int C, int F, const int32_t* seg_count_host, const int32_t* segs_host, int* given,
               long long dst_limit) {
    if (start < 0) return fail(F5_EINVAL, "%s: item %d starts at start = %lld < 0", who, b, (long long)start);
    if (C < 1) return fail(F5_EINVAL, "%s: item %d has channels = %d (need channels >= 1)", who, b, C);
    if (F < 1) return fail(F5_EINVAL, "%s: item %d has frames = %d (need frames >= 1)", who, b, F);
    if ((long long)C * F > INT32_MAX) return fail(F5_EINVAL, "%s: item %d has %d x %d samples (need channels * frames < 2^31)", who, b, C, F);
    if (!seg_count_host) return F5_OK;
    const int count = seg_count_host[b];
    if (count < 0) return fail(F5_EINVAL, "%s: item %d has %d segments", who, b, count);
    if ((long long)*given + count > (1 << 26)) return fail(F5_EINVAL, "%s: more than 2^26 segments at item %d", who, b);
    CHK(check_segments(who, b, segs_host + 3 * (size_t)*given, count, 0, dst_limit));
    *given += count;
    return F5_OK;
}

// the device tables of one call, items[B] | flag_first[pairs + 1] | tile_start[B + 1] | segs[nseg]: one layout for slot and device
struct Tables {
    Item* items;
    long long* flag_first;
    int* tile_start;
    Seg* segs;
    Tables(char* base, int B, int pairs)
        : items(reinterpret_cast<Item*>(base)), flag_first(reinterpret_cast<long long*>(base + (size_t)B * sizeof(Item))),
          tile_start(reinterpret_cast<int*>(flag_first + pairs + 1)), segs(reinterpret_cast<Seg*>(tile_start + B + 1)) {}
    static size_t bytes(int B, int pairs, int nseg) {
        return (size_t)B * sizeof(Item) + ((size_t)pairs + 1) * 8 + ((size_t)B + 1) * 4 + (size_t)std::max(nseg, 1) * sizeof(Seg);
    }
};
static_assert(sizeof(Item) % 8 == 0, "flag_first follows the items and is 8-byte aligned");
}  // namespace

extern "C" int f5_silence_plan(int32_t B, const int32_t* len_ms_host, int32_t nq, const int32_t* queries_host, int32_t* count_out,
                               int64_t* start_out, int64_t* total_out) {
    const char* who = "f5_silence_plan";
    if (!count_out) return fail(F5_EINVAL, "%s: null count_out", who);
    if (!start_out) return fail(F5_EINVAL, "%s: null start_out", who);
    if (!total_out) return fail(F5_EINVAL, "%s: null total_out", who);
    return plan_flags(who, B, len_ms_host, nq, queries_host, count_out, start_out, total_out, nullptr);
}

extern "C" int f5_silence_analyse(const float* base, int32_t B, const int64_t* start_host, const int32_t* channels_host,
                                  const int32_t* frames_host, const int32_t* rate_host, const int32_t* len_ms_host, float qscale,
                                  int32_t nq, const int32_t* queries_host, const int32_t* seg_count_host, const int32_t* segs_host,
                                  uint8_t* flags, int64_t flags_capacity, f5_stream stream) {
    const char* who = "f5_silence_analyse";
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!channels_host) return fail(F5_EINVAL, "%s: null channels_host", who);
    if (!frames_host) return fail(F5_EINVAL, "%s: null frames_host", who);
    if (!rate_host) return fail(F5_EINVAL, "%s: null rate_host", who);
    if (!flags) return fail(F5_EINVAL, "%s: null flags", who);
    if (seg_count_host && !segs_host) return fail(F5_EINVAL, "%s: null segs_host with a seg_count_host", who);
    if (!(qscale > 0.0f && qscale <= 32768.0f)) return fail(F5_EINVAL, "%s: qscale = %g (need 0 < qscale <= 32768)", who, (double)qscale);
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 items (B = %d)", who, B);
    CHK(check_queries(who, nq, queries_host, nullptr));
    Queries qs{};
    int64_t total_flags = 0;
    std::vector<int64_t> flag_first((size_t)B * nq + 1);
    CHK(plan_flags(who, B, len_ms_host, nq, queries_host, nullptr, flag_first.data(), &total_flags, &qs));
    const int pairs = B * nq;
    flag_first[pairs] = total_flags;
    if (flags_capacity < total_flags)
        return fail(F5_EINVAL, "%s: flags_capacity = %lld is less than the plan's total of %lld flags", who, (long long)flags_capacity,
                    (long long)total_flags);
    std::vector<Item> items((size_t)B);
    std::vector<int> tile_start((size_t)B + 1);
    long long slots = 0, tiles = 0;
    int given = 0;
    for (int b = 0; b < B; ++b) {
        const int first = given;
        CHK(check_item(who, b, start_host[b], channels_host[b], frames_host[b], seg_count_host, segs_host, &given, INT32_MAX));
        const int R = rate_host[b], L = len_ms_host[b];
        if (R < 11025 || R > 384000) return fail(F5_EINVAL, "%s: item %d has rate = %d Hz (need 11025 <= rate <= 384000)", who, b, R);
        if (ms_pos(R, L) > INT32_MAX) return fail(F5_EINVAL, "%s: item %d: L = %d ms at %d Hz is past what 32 bits hold", who, b, L, R);
        Item& it = items[b];
        it.in_start = start_host[b];
        it.slot_start = slots;
        it.C = channels_host[b], it.F = frames_host[b], it.R = R, it.L = L;
        it.seg_first = first, it.seg_count = seg_count_host ? seg_count_host[b] : -1;
        it.vec = it.F % 4 == 0 && (reinterpret_cast<uintptr_t>(base + it.in_start) & 15) == 0;
        it.pad = 0;
        tile_start[b] = (int)tiles;
        slots += (long long)L + 1;
        tiles += ((long long)L + 1 + kTile - 1) / kTile;
        if (slots > kMaxSlots) return fail(F5_EINVAL, "%s: more than 2^30 milliseconds in one call at item %d (split the batch)", who, b);
    }
    tile_start[B] = (int)tiles;
    const size_t tab_bytes = Tables::bytes(B, pairs, given);

    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    long long *slot_buf = nullptr, *tile_sum = nullptr;
    char* tab = nullptr;
    auto plan = [&](Arena& a) {
        a.reset();
        slot_buf = a.take<long long>((size_t)slots);
        tile_sum = a.take<long long>((size_t)tiles);
        tab = a.take<char>(tab_bytes);
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(st->arena.reserve(plan(dry)));
    (void)plan(st->arena);
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        const Tables h(host, B, pairs);
        for (int b = 0; b < B; ++b) h.items[b] = items[b];
        for (int k = 0; k <= pairs; ++k) h.flag_first[k] = flag_first[k];
        for (int b = 0; b <= B; ++b) h.tile_start[b] = tile_start[b];
        for (int k = 0; k < given; ++k) h.segs[k] = Seg{segs_host[3 * k], segs_host[3 * k + 1], segs_host[3 * k + 2]};
    }));
    const Tables d(tab, B, pairs);
    if (seg_count_host)
        silence_energy_kernel<true><<<dim3((unsigned)tiles), kThreads, 0, s>>>(base, d.items, d.tile_start, B, d.segs, qscale, slot_buf, tile_sum);
    else
        silence_energy_kernel<false><<<dim3((unsigned)tiles), kThreads, 0, s>>>(base, d.items, d.tile_start, B, d.segs, qscale, slot_buf, tile_sum);
    KCHK();
    silence_tile_scan_kernel<<<dim3((unsigned)B), kThreads, 0, s>>>(d.tile_start, tile_sum);
    KCHK();
    silence_prefix_kernel<<<dim3((unsigned)tiles), kThreads, 0, s>>>(d.items, d.tile_start, B, tile_sum, slot_buf);
    KCHK();
    if (total_flags > 0) {
        const unsigned grid = (unsigned)std::min<long long>((total_flags + kThreads - 1) / kThreads, 65536);
        silence_flags_kernel<<<dim3(grid), kThreads, 0, s>>>(d.items, d.flag_first, pairs, nq, qs, slot_buf, flags, (long long)total_flags);
        KCHK();
    }
    return st->leave(s);
}

extern "C" int f5_wave_gather(const float* base, int32_t B, const int64_t* start_host, const int32_t* channels_host,
                              const int32_t* frames_host, float qscale, const int32_t* seg_count_host, const int32_t* segs_host,
                              const int32_t* out_frames_host, const int64_t* out_start_host, float* out, int64_t out_capacity,
                              f5_stream stream) {
    const char* who = "f5_wave_gather";
    if (B < 1 || B > 65535) return fail(F5_EINVAL, "%s: need 1 <= B <= 65535 items (B = %d)", who, B);
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!channels_host) return fail(F5_EINVAL, "%s: null channels_host", who);
    if (!frames_host) return fail(F5_EINVAL, "%s: null frames_host", who);
    if (!seg_count_host) return fail(F5_EINVAL, "%s: null seg_count_host", who);
    if (!segs_host) return fail(F5_EINVAL, "%s: null segs_host", who);
    if (!out_frames_host) return fail(F5_EINVAL, "%s: null out_frames_host", who);
    if (!out_start_host) return fail(F5_EINVAL, "%s: null out_start_host", who);
    if (!out) return fail(F5_EINVAL, "%s: null out", who);
    if (!(qscale > 0.0f && qscale <= 32768.0f)) return fail(F5_EINVAL, "%s: qscale = %g (need 0 < qscale <= 32768)", who, (double)qscale);
    std::vector<Item> items((size_t)B);
    std::vector<int> tile_start((size_t)B + 1);
    long long tiles = 0;
    int given = 0;
    for (int b = 0; b < B; ++b) {
        const int first = given;
        const int F_out = out_frames_host[b];
        if (F_out < 0) return fail(F5_EINVAL, "%s: item %d has out_frames = %d < 0", who, b, F_out);
        CHK(check_item(who, b, start_host[b], channels_host[b], frames_host[b], seg_count_host, segs_host, &given, F_out));
        const long long n = (long long)channels_host[b] * F_out;
        if (out_start_host[b] < 0 || out_start_host[b] + n > out_capacity)
            return fail(F5_EINVAL, "%s: item %d writes elements [%lld, %lld) of out_capacity = %lld", who, b, (long long)out_start_host[b],
                        (long long)out_start_host[b] + n, (long long)out_capacity);
        Item& it = items[b];
        it.in_start = start_host[b];
        it.slot_start = out_start_host[b];
        it.C = channels_host[b], it.F = frames_host[b], it.R = 0, it.L = F_out;
        it.seg_first = first, it.seg_count = seg_count_host[b];
        it.vec = 0, it.pad = 0;
        tile_start[b] = (int)tiles;
        tiles += (long long)it.C * ((F_out + kOutTile - 1) / kOutTile);
        if (tiles > kMaxSlots) return fail(F5_EINVAL, "%s: more than 2^30 tiles of work at item %d (split the batch)", who, b);
    }
    tile_start[B] = (int)tiles;
    if (tiles == 0) return F5_OK;                   // every item is empty
    const size_t tab_bytes = Tables::bytes(B, 0, given);

    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        const Tables h(host, B, 0);
        for (int b = 0; b < B; ++b) h.items[b] = items[b];
        h.flag_first[0] = 0;
        for (int b = 0; b <= B; ++b) h.tile_start[b] = tile_start[b];
        for (int k = 0; k < given; ++k) h.segs[k] = Seg{segs_host[3 * k], segs_host[3 * k + 1], segs_host[3 * k + 2]};
    }));
    const Tables d(tab, B, 0);
    wave_gather_kernel<<<dim3((unsigned)tiles), kThreads, 0, s>>>(base, d.items, d.tile_start, B, d.segs, qscale, out);
    KCHK();
    return st->leave(s);
}
