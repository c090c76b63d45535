// DTW-aligned mel-cepstral distance of a ragged batch of mel pairs on gfx950 (the contract is in include/f5_hip.h): what the
// engine's own sample() output is scored with against a recording, on the device, without an n x m matrix anywhere.
//   mel_cepstra_kernel   one thread per (row, k) over the packed rows of both sides of every pair: c_k = sum_j (double)x_j * T[k][j]
//                        in f64, j ascending, no cross-lane reduction.  The DCT table comes from the host (no device cos) and goes
//                        through LDS in chunks of kCepChunk mel bins; the rows are read where they lie (offset + row stride).
//   mel_dtw_kernel       one workgroup of kDtwThreads per pair, the largest pairs first.  The shorter side is the column side:
//                        thread t owns the strip of W adjacent columns [t W, t W + W), W the smallest power of two with
//                        W * kDtwThreads >= columns (W <= kDtwMaxStrip), and walks the rows in a wavefront, row s - t at step s.
//                        D(i-1, j) of its strip stays in registers; D(i, j-1) and D(i-1, j-1) of its first column are the left
//                        neighbour's last column of the step before and of two steps before: a lane shift inside a wave, a
//                        two-slot LDS ring between waves, ONE barrier per step.  d(i, j) of a step is computed in the step before
//                        it, beside the recurrence and off its dependency chain (the f64 sqrt included).  The row side's cepstra
//                        stream through an LDS ring in blocks of kDtwRowBlock rows, written two blocks ahead under the same
//                        barrier; the column side's cepstra sit in LDS, strip-interleaved so that adjacent lanes are an odd
//                        number of doubles apart.  Whichever of the two does not fit the kDtwLdsBytes of a workgroup (n_cep = 64
//                        with 256 active threads; more than about 1,250 columns at n_cep = 13) is read through the caches instead:
//                        the same values, so nothing else changes.  For that the cepstra launch writes a column side as
//                        [c][k][t] (column t W + c), whole strips: adjacent lanes read adjacent doubles.  State: O(n + m) doubles.
// Every cell is one addition per candidate and a three-way minimum: no evaluation order can change a bit of D, so a pair's value is
// the same alone and in any batch, and value(a, b) == value(b, a) bit for bit.  No atomics.  The per-call tables (the DCT table,
// pairs, row segments, launch order) go through one pinned slot and one copy into the workspace of the handle-less calls
// (CallState, internal.h), which grows with use; no host read and no synchronisation otherwise.
//   f5_mel_align         the same two launches with the recurrence's pointer form (dtw_run<W, true>: ONE body, a compile-time switch)
//                        and a third, mel_backtrack_kernel.  The pointer form names every cell's predecessor -- 0: (i-1, j-1),
//                        1: (i-1, j), 2: (i, j-1) in terms of (a, b), the first of the smallest sums in that order whichever side is
//                        the column side -- in 2 bits.  A thread gathers the codes of its strip over 16 / W of its rows in one
//                        register and stores the 32-bit word when it is full: word [row / (16 / W)][t] of the pair's store, so a
//                        cell costs one compare chain and a shift, a row of the wave one partial store.  The backtrack is one wave
//                        per pair with one walking lane (at most n + m - 2 dependent steps, a word reread only when the walk leaves
//                        it): it writes the cells backwards from the end of the pair's n + m - 1 slots, then the wave moves them to
//                        the front, so that the path reads forward from (0, 0).
#include <cmath>
#include <cstdint>
#include <numeric>

#include "internal.h"

#define fail f5_fail

namespace {
constexpr int kDtwThreads = 256;                    // threads of a pair's workgroup = strips of the column side
constexpr int kDtwMaxStrip = 16;                    // columns of a strip at most: kDtwThreads * kDtwMaxStrip = 4096 frames
constexpr int kDtwRowBlock = 32;                    // rows of the streamed side per LDS refill
constexpr int kDtwLdsBytes = 159 * 1024;            // dynamic LDS a workgroup may ask for (160 KiB per CU)
constexpr int kWaves = kDtwThreads / 64;
constexpr int kCepThreads = 256;
constexpr int kCepChunk = 32;                       // mel bins of the DCT table in LDS at a time
constexpr int kMaxPairs = 65535, kMaxFrames = 4096, kMaxCep = 64, kMinMels = 2, kMaxMels = 256;
constexpr long long kMaxValues = 1LL << 28;         // cepstral values of one call (grid sizes are int; 2 GiB of workspace)
constexpr double kMcdScale = 0x1.15f2ced384f28p+2;  // 10 / ln 10 = 4.3429448190325175

struct Seg {                                        // one side of one pair: `frames` rows of n_mels f32, `stride` elements apart
    long long start, stride;
    long long dst_row;                              // where its cepstra start in the workspace, in rows of n_cep doubles
    int first_row, side;                            // its first row among the rows of the call; side 1: b_base
    int W, T;                                       // the column side of its pair: the pair's strip and thread count; else W = 0
};
struct Pair {
    long long rows_off, cols_off;                   // where the row (longer) and the column (shorter) side's cepstra start, in rows
    int n_rows, n_cols;
    int W, T;                                       // strip width and active threads: T = ceil(n_cols / W)
    int C, flags;                                   // ring capacity in rows: T + 2 kDtwRowBlock; bit 0: rows in LDS, bit 1: columns,
};                                                  // bit 2: a is the column side (n < m)
struct Trace {                                      // f5_mel_align: where a pair's back-pointer words and its path start
    long long bp_off, path_off;                     // in 32-bit words of the store; in (i, j) pairs of `path`
};
static_assert(sizeof(Seg) == 40 && sizeof(Pair) == 40 && sizeof(Trace) == 16, "table layout");
constexpr int kMaxTraceBytes = 1 << 26;             // back-pointers of one call: 2 bits a cell, a 4096 x 4096 pair is 4 MiB
constexpr int kWalkThreads = 64;

__host__ __device__ __forceinline__ int lds_stride(int n_cep) { return n_cep | 1; }   // doubles per LDS row: odd, so no bank is hit twice

// the last entry of segs[0 .. n) whose first_row is <= r (ascending, segs[0].first_row = 0)
__device__ __forceinline__ int seg_of_row(const Seg* __restrict__ segs, int n, int r) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_row <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kCepThreads) void mel_cepstra_kernel(const float* __restrict__ a_base, const float* __restrict__ b_base,
                                                                  const Seg* __restrict__ segs, int nseg,
                                                                  const double* __restrict__ table /* [n_mels][n_cep] */, int n_mels,
                                                                  int n_cep, long long total, double* __restrict__ cep) {
    __shared__ double tile[kCepChunk * kMaxCep];
    const long long idx = (long long)blockIdx.x * kCepThreads + threadIdx.x;
    const bool live = idx < total;
    const int row = live ? (int)(idx / n_cep) : 0, k = live ? (int)(idx % n_cep) : 0;
    const float* x = nullptr;
    size_t dst = 0;                                 // row side: [row][k]; column side: [c][k][t] for column t W + c
    if (live) {
        const Seg g = segs[seg_of_row(segs, nseg, row)];
        const int j = row - g.first_row;
        x = (g.side ? b_base : a_base) + g.start + (long long)j * g.stride;
        dst = (size_t)g.dst_row * n_cep + (g.W ? ((size_t)(j % g.W) * n_cep + k) * g.T + j / g.W : (size_t)j * n_cep + k);
    }
    double acc = 0.0;
    for (int j0 = 0; j0 < n_mels; j0 += kCepChunk) {    // (uniform over the block)
        const int cnt = min(kCepChunk, n_mels - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * n_cep; e += kCepThreads) tile[e] = table[(size_t)j0 * n_cep + e];
        __syncthreads();
        if (live)
            for (int jj = 0; jj < cnt; ++jj) acc += (double)x[j0 + jj] * tile[jj * n_cep + k];
    }
    if (live) cep[dst] = acc;
}

// rows [r0, r0 + kDtwRowBlock) of the row side into their ring slots; every thread of the block calls it
__device__ __forceinline__ void ring_fill(double* ring, const double* __restrict__ rows_g, int r0, int n, int C, int n_cep) {
    const int ld = lds_stride(n_cep);
    for (int e = threadIdx.x; e < kDtwRowBlock * n_cep; e += kDtwThreads) {
        const int r = r0 + e / n_cep, k = e % n_cep;
        if (r < n) ring[(r % C) * ld + k] = rows_g[(size_t)r * n_cep + k];
    }
}

// PTR: the pointer form -- beside D, every cell's predecessor code goes to `bp` (this pair's words)
template <int W, bool PTR>
__device__ __forceinline__ void dtw_run(const Pair pr, const double* __restrict__ cep, int n_cep, double* smem, double* result,
                                        uint32_t* __restrict__ bp) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = pr.n_rows, m = pr.n_cols, T = pr.T, C = pr.C, ld = lds_stride(n_cep);
    const bool rows_lds = pr.flags & 1, cols_lds = pr.flags & 2;
    constexpr int R = kDtwMaxStrip / W;             // rows of the strip in one 32-bit word of codes
    constexpr int kUnrollK = PTR && W == kDtwMaxStrip ? 2 : 4;   // the widest strip of the pointer form has no registers for four
    const double inf = __builtin_huge_val();
    double* xch = smem;                             // [2][kWaves]: a wave's last column, for the wave to its right
    double* ring = smem + 2 * kWaves;               // [C][ld]
    double* cols_l = ring + (rows_lds ? (size_t)C * ld : 0);   // [W][T][ld]
    const double* rows_g = cep + (size_t)pr.rows_off * n_cep;
    const double* cols_g = cep + (size_t)pr.cols_off * n_cep;

    if (t < 2 * kWaves) xch[t] = inf;
    if (cols_lds)
        for (int e = t; e < W * n_cep * T; e += kDtwThreads) {   // (whole strips: a column past the end holds stale values, unused)
            const int c = e / (n_cep * T), k = e / T % n_cep;
            cols_l[((size_t)c * T + e % T) * ld + k] = cols_g[e];
        }
    if (rows_lds) ring_fill(ring, rows_g, 0, n, C, n_cep);
    __syncthreads();

    const bool active = t < T;
    const int j0 = t * W;
    // coefficient k of column j0 + c is cptr[c][k * ks]: in LDS [c][t][k], in the workspace [c][k][t] -- adjacent lanes one double
    // apart, so a wave's load is one contiguous 512 bytes
    const double* cptr[W];
    const int ks = cols_lds ? 1 : T;
#pragma unroll
    for (int c = 0; c < W; ++c) cptr[c] = cols_lds ? cols_l + ((size_t)c * T + min(t, T - 1)) * ld : cols_g + (size_t)c * n_cep * T + min(t, T - 1);

    // d(i, j0 .. j0 + W) of row i, whose ring slot is `slot`
    auto frame_distances = [&](int i, int slot, double* d) {
        const double* ra = rows_lds ? ring + (size_t)slot * ld : rows_g + (size_t)i * n_cep;
        double acc[W];
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] = 0.0;
#pragma unroll kUnrollK                             // (several k's loads in flight: one wave per SIMD has nothing else to hide them)
        for (int k = 0; k < n_cep; ++k) {
            const double r = ra[k];
#pragma unroll
            for (int c = 0; c < W; ++c) {
                const double diff = r - cptr[c][(size_t)k * ks];
                acc[c] += diff * diff;
            }
        }
#pragma unroll
        for (int c = 0; c < W; ++c) d[c] = kMcdScale * sqrt(2.0 * acc[c]);
    };

    double prev[W], dcur[W], dnext[W];              // D(i - 1, j) of the strip; d of this step's row and of the next one's
#pragma unroll
    for (int c = 0; c < W; ++c) prev[c] = inf, dcur[c] = 0.0, dnext[c] = 0.0;
    double last = inf;                              // D of the strip's last column after the step before
    double diag = t == 0 ? 0.0 : inf;               // D(i - 1, j0 - 1); the virtual D(-1, -1) = 0 makes D(0, 0) = 2 d(0, 0)
    int slot = ((-t) % C + C) % C;                  // the ring slot of row s + 1 - t, kept by increments
    const bool a_cols = pr.flags & 4;
    uint32_t word = 0;
    if (t == 0) frame_distances(0, 0, dcur);
    slot = slot + 1 == C ? 0 : slot + 1;

    const int steps = n + T - 1;
    for (int s = 0; s < steps; ++s) {
        if (rows_lds && s % kDtwRowBlock == 0) ring_fill(ring, rows_g, s + kDtwRowBlock, n, C, n_cep);
        const int i = s - t;
        if (active && i + 1 >= 0 && i + 1 < n) frame_distances(i + 1, slot, dnext);
        slot = slot + 1 == C ? 0 : slot + 1;
        double recv = __shfl_up(last, 1, 64);       // D(i, j0 - 1): the left neighbour's row i was its step s - 1
        if (lane == 0) recv = wave == 0 ? inf : xch[((s + 1) & 1) * kWaves + wave - 1];
        if (active && i >= 0 && i < n) {
            double left = recv, dg = diag;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (j0 + c < m) {
                    const double up = prev[c], d = dcur[c];
                    const double cu = up + d, cd = dg + 2.0 * d, cl = left + d;
                    const double cur = fmin(fmin(cu, cd), cl);
                    if constexpr (PTR) {            // the first candidate equal to the minimum; `up` is a's step unless a is
                        const uint32_t code = cd == cur ? 0u : ((a_cols ? cl : cu) == cur ? 1u : 2u);   // the column side
                        word |= code << (2 * ((i % R) * W + c));
                    }
                    dg = up;
                    left = cur;
                    prev[c] = cur;
                }
            }
            last = left;
            if (i == n - 1 && t == T - 1) *result = left / (double)(n + m);
            if constexpr (PTR) {
                if (i % R == R - 1 || i == n - 1) {
                    bp[(size_t)(i / R) * T + t] = word;
                    word = 0;
                }
            }
        }
        diag = recv;
        if (lane == 63) xch[(s & 1) * kWaves + wave] = last;
#pragma unroll
        for (int c = 0; c < W; ++c) dcur[c] = dnext[c];
        __syncthreads();
    }
}

template <bool PTR>
__global__ __launch_bounds__(kDtwThreads) void mel_dtw_kernel(const Pair* __restrict__ pairs, const int* __restrict__ order,
                                                              const double* __restrict__ cep, int n_cep, double* __restrict__ out,
                                                              const Trace* __restrict__ trace, uint32_t* __restrict__ store) {
    extern __shared__ __attribute__((aligned(16))) char dtw_smem[];
    double* smem = reinterpret_cast<double*>(dtw_smem);
    const int p = order[blockIdx.x];
    const Pair pr = pairs[p];
    uint32_t* bp = nullptr;
    if constexpr (PTR) bp = store + trace[p].bp_off;
    switch (pr.W) {                                 // (uniform over the block)
        case 1: dtw_run<1, PTR>(pr, cep, n_cep, smem, out + p, bp); break;
        case 2: dtw_run<2, PTR>(pr, cep, n_cep, smem, out + p, bp); break;
        case 4: dtw_run<4, PTR>(pr, cep, n_cep, smem, out + p, bp); break;
        case 8: dtw_run<8, PTR>(pr, cep, n_cep, smem, out + p, bp); break;
        default: dtw_run<kDtwMaxStrip, PTR>(pr, cep, n_cep, smem, out + p, bp); break;
    }
}

// One wave per pair; lane 0 walks the codes from (n-1, m-1) to (0, 0).  On the grid's first row and column the only step there is
// is taken whatever the code says, so the walk stays inside the grid and ends after at most n + m - 2 steps on any store.
__global__ __launch_bounds__(kWalkThreads) void mel_backtrack_kernel(const Pair* __restrict__ pairs, const Trace* __restrict__ trace,
                                                                     const uint32_t* __restrict__ store, const double* __restrict__ dist,
                                                                     int* __restrict__ path_len, int2* __restrict__ path) {
    __shared__ int len_s;
    const int p = blockIdx.x, lane = threadIdx.x;
    const Pair pr = pairs[p];
    const bool a_cols = pr.flags & 4;
    const int n = a_cols ? pr.n_cols : pr.n_rows, m = a_cols ? pr.n_rows : pr.n_cols;   // of a and of b
    const int slots = n + m - 1, R = kDtwMaxStrip / pr.W;
    const uint32_t* bp = store + trace[p].bp_off;
    int2* out = path + trace[p].path_off;
    if (lane == 0) {
        int len = 0;
        const double v = dist[p];
        if (v - v == 0.0) {                         // finite
            int i = n - 1, j = m - 1;
            long long at = -1;
            uint32_t word = 0;
            for (;;) {
                out[slots - 1 - len] = make_int2(i, j);
                ++len;
                if (i == 0 && j == 0) break;
                const int r = a_cols ? j : i, c = a_cols ? i : j;
                const long long idx = (long long)(r / R) * pr.T + c / pr.W;
                if (idx != at) word = bp[idx], at = idx;
                uint32_t code = (word >> (2 * ((r % R) * pr.W + c % pr.W))) & 3u;
                if (i == 0) code = 2;
                else if (j == 0) code = 1;
                if (code != 2) --i;
                if (code != 1) --j;
            }
        }
        len_s = len;
        path_len[p] = len;
    }
    __syncthreads();
    const int len = len_s, shift = slots - len;
    if (shift == 0) return;
    for (int k0 = 0; k0 < len; k0 += kWalkThreads) {   // dst < src, ascending: a chunk is read whole before it is written
        int2 v = make_int2(0, 0);
        if (k0 + lane < len) v = out[shift + k0 + lane];
        __syncthreads();
        if (k0 + lane < len) out[k0 + lane] = v;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- host side
// a pair's strip: the smallest power of two W with W * kDtwThreads >= columns; its threads: ceil(columns / W)
void strip_of(int columns, int* W, int* T) {
    *W = 1;
    while (*W * kDtwThreads < columns) *W *= 2;
    *T = (columns + *W - 1) / *W;
}

// *rows_out: the rows of cepstra the call holds, the column side of every pair rounded up to whole strips
int check_counts(const char* who, int P, const int32_t* a_frames_host, const int32_t* b_frames_host, int n_cep, long long* rows_out) {
    if (P < 1 || P > kMaxPairs) return fail(F5_EINVAL, "%s: need 1 <= P <= %d pairs (P = %d)", who, kMaxPairs, P);
    if (!a_frames_host) return fail(F5_EINVAL, "%s: null a_frames_host", who);
    if (!b_frames_host) return fail(F5_EINVAL, "%s: null b_frames_host", who);
    if (n_cep < 1 || n_cep > kMaxCep) return fail(F5_EINVAL, "%s: n_cep = %d (need 1 <= n_cep <= min(%d, n_mels - 1))", who, n_cep, kMaxCep);
    long long rows = 0;
    for (int p = 0; p < P; ++p) {
        const int n = a_frames_host[p], m = b_frames_host[p];
        if (n < 1 || n > kMaxFrames) return fail(F5_EINVAL, "%s: pair %d has a_frames = %d (need 1 <= frames <= %d)", who, p, n, kMaxFrames);
        if (m < 1 || m > kMaxFrames) return fail(F5_EINVAL, "%s: pair %d has b_frames = %d (need 1 <= frames <= %d)", who, p, m, kMaxFrames);
        int W = 0, T = 0;
        strip_of(std::min(n, m), &W, &T);
        rows += (long long)std::max(n, m) + W * T;
        if (rows * n_cep > kMaxValues)
            return fail(F5_EINVAL, "%s: more than 2^28 cepstral values in one call at pair %d (split the batch)", who, p);
    }
    *rows_out = rows;
    return F5_OK;
}

// largest n * m first, ties by index: the long pairs open the launch instead of forming its tail
void launch_order(int P, const int32_t* a_frames_host, const int32_t* b_frames_host, int32_t* order) {
    std::iota(order, order + P, 0);
    std::stable_sort(order, order + P, [&](int32_t x, int32_t y) {
        return (long long)a_frames_host[x] * b_frames_host[x] > (long long)a_frames_host[y] * b_frames_host[y];
    });
}

// the tables of one call, table[n_mels * n_cep] | pairs[P] | segs[2 P] | trace[P] (f5_mel_align only) | order[P]: one layout for slot
// and device.  The workspace keeps room for the table of kMaxMels bins, so that the plan needs no n_mels.
struct Tables {
    double* table;
    Pair* pairs;
    Seg* segs;
    Trace* trace;
    int* order;
    Tables(char* base, int P, int n_mels, int n_cep, bool align)
        : table(reinterpret_cast<double*>(base)), pairs(reinterpret_cast<Pair*>(table + (size_t)n_mels * n_cep)),
          segs(reinterpret_cast<Seg*>(pairs + P)), trace(reinterpret_cast<Trace*>(segs + 2 * (size_t)P)),
          order(reinterpret_cast<int*>(trace + (align ? P : 0))) {}
    static size_t bytes(int P, int n_mels, int n_cep, bool align) {
        return (size_t)n_mels * n_cep * 8 + (size_t)P * (sizeof(Pair) + 2 * sizeof(Seg) + (align ? sizeof(Trace) : 0) + 4);
    }
};

struct Carve {
    double* cep;
    char* tab;
    uint32_t* store;
};
// trace_words < 0: f5_mel_distance, which holds no back-pointer store
size_t carve(Arena& a, long long rows, int P, int n_cep, long long trace_words, Carve* out) {
    a.reset();
    out->cep = a.take<double>((size_t)rows * n_cep);
    out->tab = a.take<char>(Tables::bytes(P, kMaxMels, n_cep, trace_words >= 0));
    out->store = trace_words >= 0 ? a.take<uint32_t>((size_t)trace_words) : nullptr;
    return align_up(a.off, 256) + 256;
}

// how a pair runs: the column side (a_cols: it is a), its strip, and what of its cepstra fits the workgroup's LDS; returns the LDS
// bytes it needs
int shape_pair(Pair* pr, int n_cep, bool a_cols) {
    strip_of(pr->n_cols, &pr->W, &pr->T);
    pr->C = pr->T + 2 * kDtwRowBlock;
    const long long ld = lds_stride(n_cep);
    long long need = 2 * kWaves * 8;
    pr->flags = a_cols ? 4 : 0;
    if (need + pr->C * ld * 8 <= kDtwLdsBytes) pr->flags |= 1, need += pr->C * ld * 8;
    if (need + (long long)pr->W * pr->T * ld * 8 <= kDtwLdsBytes) pr->flags |= 2, need += (long long)pr->W * pr->T * ld * 8;
    return (int)need;
}

// the 32-bit words of a pair's back-pointers: one per thread and 16 / W rows; *words_out their sum over the call
int check_trace(const char* who, int P, const int32_t* a_frames_host, const int32_t* b_frames_host, long long* words_out) {
    long long words = 0;
    for (int p = 0; p < P; ++p) {
        int W = 0, T = 0;
        strip_of(std::min(a_frames_host[p], b_frames_host[p]), &W, &T);
        const int R = kDtwMaxStrip / W;
        words += (long long)((std::max(a_frames_host[p], b_frames_host[p]) + R - 1) / R) * T;
        if (words * 4 > kMaxTraceBytes)
            return fail(F5_EINVAL, "%s: more than %d bytes of back-pointers in one call at pair %d (split the batch)", who, kMaxTraceBytes, p);
    }
    *words_out = words;
    return F5_OK;
}

// f5_mel_distance (path == nullptr) and f5_mel_align: one set of checks, tables and launches
int run(const char* who, const float* a_base, const float* b_base, int32_t P, const int64_t* a_start_host, const int32_t* a_frames_host,
        int64_t a_row_stride, const int64_t* b_start_host, const int32_t* b_frames_host, int64_t b_row_stride, int32_t n_mels,
        int32_t n_cep, double* out, int32_t* path_len, int32_t* path, hipStream_t s) {
    const bool align = path != nullptr;
    if (!a_base) return fail(F5_EINVAL, "%s: null a_base", who);
    if (!b_base) return fail(F5_EINVAL, "%s: null b_base", who);
    if (!a_start_host) return fail(F5_EINVAL, "%s: null a_start_host", who);
    if (!b_start_host) return fail(F5_EINVAL, "%s: null b_start_host", who);
    if (!out) return fail(F5_EINVAL, "%s: null out", who);
    if (n_mels < kMinMels || n_mels > kMaxMels)
        return fail(F5_EINVAL, "%s: n_mels = %d (need %d <= n_mels <= %d)", who, n_mels, kMinMels, kMaxMels);
    if (n_cep > n_mels - 1) return fail(F5_EINVAL, "%s: n_cep = %d (need 1 <= n_cep <= min(%d, n_mels - 1))", who, n_cep, kMaxCep);
    if (a_row_stride < n_mels) return fail(F5_EINVAL, "%s: a_row_stride = %lld is less than n_mels = %d", who, (long long)a_row_stride, n_mels);
    if (b_row_stride < n_mels) return fail(F5_EINVAL, "%s: b_row_stride = %lld is less than n_mels = %d", who, (long long)b_row_stride, n_mels);
    long long rows = 0, trace_words = -1;
    CHK(check_counts(who, P, a_frames_host, b_frames_host, n_cep, &rows));
    if (align) CHK(check_trace(who, P, a_frames_host, b_frames_host, &trace_words));
    for (int p = 0; p < P; ++p) {
        if (a_start_host[p] < 0) return fail(F5_EINVAL, "%s: pair %d has a_start = %lld < 0", who, p, (long long)a_start_host[p]);
        if (b_start_host[p] < 0) return fail(F5_EINVAL, "%s: pair %d has b_start = %lld < 0", who, p, (long long)b_start_host[p]);
    }
    std::vector<Pair> pairs((size_t)P);
    std::vector<Seg> segs(2 * (size_t)P);
    std::vector<Trace> trace(align ? (size_t)P : 0);
    std::vector<int32_t> order((size_t)P);
    launch_order(P, a_frames_host, b_frames_host, order.data());
    int first = 0, lds = 0;
    long long at = 0, frames = 0, words = 0, cells = 0;
    for (int p = 0; p < P; ++p) {
        const int n = a_frames_host[p], m = b_frames_host[p];
        Pair& pr = pairs[p];
        const bool a_rows = n >= m;                 // the shorter side is the column side; either choice gives the same bits
        pr.n_rows = a_rows ? n : m, pr.n_cols = a_rows ? m : n;
        lds = std::max(lds, shape_pair(&pr, n_cep, !a_rows));
        pr.rows_off = at, pr.cols_off = at + pr.n_rows;
        segs[2 * p] = Seg{a_start_host[p], a_row_stride, a_rows ? pr.rows_off : pr.cols_off, first, 0, a_rows ? 0 : pr.W, pr.T};
        segs[2 * p + 1] = Seg{b_start_host[p], b_row_stride, a_rows ? pr.cols_off : pr.rows_off, first + n, 1, a_rows ? pr.W : 0, pr.T};
        first += n + m;
        frames += n + m;
        at += pr.n_rows + (long long)pr.W * pr.T;
        if (align) {
            const int R = kDtwMaxStrip / pr.W;
            trace[p] = Trace{words, cells};
            words += (long long)((pr.n_rows + R - 1) / R) * pr.T;
            cells += n + m - 1;
        }
    }
    const long long total = frames * n_cep;         // one thread per (frame, k); `rows` of cepstra with the strips' padding
    const size_t tab_bytes = Tables::bytes(P, n_mels, n_cep, align);

    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    Arena dry;
    Carve c;
    CHK(st->arena.reserve(carve(dry, rows, P, n_cep, trace_words, &c)));
    (void)carve(st->arena, rows, P, n_cep, trace_words, &c);
    const void* dtw = align ? reinterpret_cast<const void*>(&mel_dtw_kernel<true>) : reinterpret_cast<const void*>(&mel_dtw_kernel<false>);
    HIPCHK(hipFuncSetAttribute(dtw, hipFuncAttributeMaxDynamicSharedMemorySize, kDtwLdsBytes));
    CHK(st->enter(s));
    CHK(st->stage.upload(c.tab, tab_bytes, s, [&](char* host) {
        const Tables h(host, P, n_mels, n_cep, align);
        const double norm = std::sqrt(2.0 / n_mels);
        for (int j = 0; j < n_mels; ++j)
            for (int k = 1; k <= n_cep; ++k) h.table[(size_t)j * n_cep + (k - 1)] = norm * std::cos(M_PI * k * (j + 0.5) / n_mels);
        for (int p = 0; p < P; ++p) h.pairs[p] = pairs[p], h.order[p] = order[p];
        for (int g = 0; g < 2 * P; ++g) h.segs[g] = segs[g];
        for (int p = 0; align && p < P; ++p) h.trace[p] = trace[p];
    }));
    const Tables d(c.tab, P, n_mels, n_cep, align);
    const unsigned grid = (unsigned)((total + kCepThreads - 1) / kCepThreads);
    mel_cepstra_kernel<<<dim3(grid), kCepThreads, 0, s>>>(a_base, b_base, d.segs, 2 * P, d.table, n_mels, n_cep, total, c.cep);
    KCHK();
    if (!align) {
        mel_dtw_kernel<false><<<dim3((unsigned)P), kDtwThreads, (size_t)lds, s>>>(d.pairs, d.order, c.cep, n_cep, out, nullptr, nullptr);
        KCHK();
        return st->leave(s);
    }
    mel_dtw_kernel<true><<<dim3((unsigned)P), kDtwThreads, (size_t)lds, s>>>(d.pairs, d.order, c.cep, n_cep, out, d.trace, c.store);
    KCHK();
    mel_backtrack_kernel<<<dim3((unsigned)P), kWalkThreads, 0, s>>>(d.pairs, d.trace, c.store, out, path_len, reinterpret_cast<int2*>(path));
    KCHK();
    return st->leave(s);
}

int plan(const char* who, bool align, int32_t P, const int32_t* a_frames_host, const int32_t* b_frames_host, int32_t n_cep,
         int32_t* order_out, int64_t* workspace_bytes_out) {
    if (!order_out) return fail(F5_EINVAL, "%s: null order_out", who);
    if (!workspace_bytes_out) return fail(F5_EINVAL, "%s: null workspace_bytes_out", who);
    long long rows = 0, trace_words = -1;
    CHK(check_counts(who, P, a_frames_host, b_frames_host, n_cep, &rows));
    if (align) CHK(check_trace(who, P, a_frames_host, b_frames_host, &trace_words));
    launch_order(P, a_frames_host, b_frames_host, order_out);
    Arena dry;
    Carve c;
    *workspace_bytes_out = (int64_t)carve(dry, rows, P, n_cep, trace_words, &c);
    return F5_OK;
}
}  // namespace

extern "C" int f5_mel_distance_plan(int32_t P, const int32_t* a_frames_host, const int32_t* b_frames_host, int32_t n_cep,
                                    int32_t* order_out, int64_t* workspace_bytes_out) {
    return plan("f5_mel_distance_plan", false, P, a_frames_host, b_frames_host, n_cep, order_out, workspace_bytes_out);
}

extern "C" int f5_mel_distance(const float* a_base, const float* b_base, int32_t P, const int64_t* a_start_host,
                               const int32_t* a_frames_host, int64_t a_row_stride, const int64_t* b_start_host,
                               const int32_t* b_frames_host, int64_t b_row_stride, int32_t n_mels, int32_t n_cep, double* out,
                               f5_stream stream) {
    return run("f5_mel_distance", a_base, b_base, P, a_start_host, a_frames_host, a_row_stride, b_start_host, b_frames_host, b_row_stride,
               n_mels, n_cep, out, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int f5_mel_align_plan(int32_t P, const int32_t* a_frames_host, const int32_t* b_frames_host, int32_t n_cep,
                                 int32_t* order_out, int64_t* workspace_bytes_out) {
    return plan("f5_mel_align_plan", true, P, a_frames_host, b_frames_host, n_cep, order_out, workspace_bytes_out);
}

extern "C" int f5_mel_align(const float* a_base, const float* b_base, int32_t P, const int64_t* a_start_host,
                            const int32_t* a_frames_host, int64_t a_row_stride, const int64_t* b_start_host,
                            const int32_t* b_frames_host, int64_t b_row_stride, int32_t n_mels, int32_t n_cep, double* dist,
                            int32_t* path_len, int32_t* path, f5_stream stream) {
    const char* who = "f5_mel_align";
    if (!path_len) return fail(F5_EINVAL, "%s: null path_len", who);
    if (!path) return fail(F5_EINVAL, "%s: null path", who);
    return run(who, a_base, b_base, P, a_start_host, a_frames_host, a_row_stride, b_start_host, b_frames_host, b_row_stride, n_mels,
               n_cep, dist, path_len, path, (hipStream_t)stream);
}

