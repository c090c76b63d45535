// Gaussian cepstral divergence on gfx950 (the contract is in include/f5_hip.h): the moments of ragged sets of mel frames and the
// second-order divergence between two such records -- whether what the engine generated sounds like its prompt, text-independent,
// with no model.
//   mom_cepstra_kernel   one thread per (row, k), k = 0 .. n_cep: dtw.hip's cepstrum restated (c_k = sum_j (double)x_j * T[k][j], f64,
//                        j ascending, the host's DCT table through LDS in chunks of kCepChunk bins); slot k = n_cep is the row's
//                        energy sum_j (double)x_j.  Rows are read where they lie.
//   mom_select_kernel    one workgroup per segment: the largest energy (a maximum has no order), whether every energy is finite,
//                        and one byte per frame: mask and gate.
//   mom_chunk_kernel     PASS 1 / 2, one workgroup per (segment, chunk of kMomChunk frames): the chunk's feature vectors (cepstra and,
//                        asked for, their deltas over clamped frame indices; PASS 2: minus the mean) go to LDS, then ONE thread sums
//                        an entry -- a mean entry, or an entry (p, q) of the upper triangle -- over the chunk's selected frames
//                        ascending.
//   mom_fold_kernel      PASS 1 / 2, one thread per entry of a segment: the chunk partials, chunk ascending.
//   gauss_pair_kernel    one workgroup of 64 threads per pair: both Cholesky factors column by column (thread r owns row r), X = L_i^-1
//                        L_j and Y = L_j^-1 L_i by forward substitution (thread c owns column c), the two mean terms by threads 0
//                        and 1, everything packed lower-triangular in LDS.
// No atomics, no host read; the per-call tables go through one pinned slot into the workspace of the handle-less calls (CallState).
#include <cmath>
#include <cstdint>

#include "internal.h"

#define fail f5_fail

namespace {
constexpr int kMomChunk = 64;                       // frames of a chunk: the unit of the fixed summation order
static_assert(kMomChunk == F5_MOM_CHUNK, "the header names the chunk");
constexpr int kMomThreads = 256;
constexpr int kCepThreads = 256;
constexpr int kCepChunk = 32;                       // mel bins of the DCT table in LDS at a time
constexpr int kSelThreads = 256;
constexpr int kMaxSegs = 65535, kMaxFrames = 4096, kMaxCep = 32, kMinMels = 2, kMaxMels = 256;
constexpr int kMaxDim = 64;                         // C = n_cep (1 + deltas) at most
constexpr int kTri = kMaxDim * (kMaxDim + 1) / 2;   // entries of a packed triangle at most
constexpr long long kMaxValues = 1LL << 28;         // cepstral values, and chunk partials, of one call
constexpr int kPairThreads = 64;

struct Seg {                                        // one segment: `frames` rows of n_mels f32
    long long start;
    int first_row, frames;                          // its first row among the rows of the call
    int first_chunk, pad;                           // its first chunk among the chunks of the call
};
static_assert(sizeof(Seg) == 24, "table layout");

__host__ __device__ __forceinline__ int tri_count(int C) { return C * (C + 1) / 2; }

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

// cep: [rows][n_cep]; energy: [rows]
__global__ __launch_bounds__(kCepThreads) void mom_cepstra_kernel(const float* __restrict__ base, const Seg* __restrict__ segs, int nseg,
                                                                  long long stride, const double* __restrict__ table /* [n_mels][n_cep] */,
                                                                  int n_mels, int n_cep, long long total, double* __restrict__ cep,
                                                                  double* __restrict__ energy) {
    __shared__ double tile[kCepChunk * kMaxCep];
    const int slots = n_cep + 1;
    const long long idx = (long long)blockIdx.x * kCepThreads + threadIdx.x;
    const bool live = idx < total;
    const int row = live ? (int)(idx / slots) : 0, k = live ? (int)(idx % slots) : 0;
    const float* x = nullptr;
    if (live) {
        const Seg g = segs[seg_of_row(segs, nseg, row)];
        x = base + g.start + (long long)(row - g.first_row) * stride;
    }
    const bool is_energy = k == n_cep;
    double acc = 0.0;
    for (int j0 = 0; j0 < n_mels; j0 += kCepChunk) {    // (uniform over the block)
        const int cnt = min(kCepChunk, n_mels - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * n_cep; e += kCepThreads) tile[e] = table[(size_t)j0 * n_cep + e];
        __syncthreads();
        if (live) {
            if (is_energy)
                for (int jj = 0; jj < cnt; ++jj) acc += (double)x[j0 + jj];
            else
                for (int jj = 0; jj < cnt; ++jj) acc += (double)x[j0 + jj] * tile[jj * n_cep + k];
        }
    }
    if (live) {
        if (is_energy) energy[row] = acc;
        else cep[(size_t)row * n_cep + k] = acc;
    }
}

// sel[row] = 1 where the frame counts; bad[s] = 1 where an energy of the segment is not finite
__global__ __launch_bounds__(kSelThreads) void mom_select_kernel(const Seg* __restrict__ segs, const double* __restrict__ energy,
                                                                 const uint8_t* __restrict__ mask, double gate_sum,
                                                                 uint8_t* __restrict__ sel, int* __restrict__ bad) {
    __shared__ double mx_s[kSelThreads];
    __shared__ int bad_s[kSelThreads];
    const Seg g = segs[blockIdx.x];
    const int t0 = threadIdx.x;
    double mx = -__builtin_huge_val();
    int nonfinite = 0;
    for (int t = t0; t < g.frames; t += kSelThreads) {
        const double e = energy[g.first_row + t];
        if (!(e - e == 0.0)) nonfinite = 1;
        if (e > mx) mx = e;
    }
    mx_s[t0] = mx;
    bad_s[t0] = nonfinite;
    __syncthreads();
    for (int w = kSelThreads / 2; w > 0; w >>= 1) {
        if (t0 < w) {
            if (mx_s[t0 + w] > mx_s[t0]) mx_s[t0] = mx_s[t0 + w];
            bad_s[t0] |= bad_s[t0 + w];
        }
        __syncthreads();
    }
    const double floor_e = mx_s[0] - gate_sum;
    if (t0 == 0) bad[blockIdx.x] = bad_s[0];
    for (int t = t0; t < g.frames; t += kSelThreads) {
        const int r = g.first_row + t;
        const bool m = mask ? mask[r] != 0 : true;
        const bool gate = gate_sum < 0.0 ? true : energy[r] >= floor_e;
        sel[r] = m && gate ? 1 : 0;
    }
}

// entry e of the packed upper triangle of a C x C matrix as (p, q), p <= q
__device__ __forceinline__ void tri_entry(int e, int C, int* p, int* q) {
    int r = 0;
    while (e >= C - r) e -= C - r, ++r;
    *p = r, *q = r + e;
}

// PASS 1: part_n[chunk] and part_sum[chunk][C]; PASS 2: part_sc[chunk][C (C + 1) / 2] with the features centred on mean[s]
template <int PASS>
__global__ __launch_bounds__(kMomThreads) void mom_chunk_kernel(const Seg* __restrict__ segs, const double* __restrict__ cep,
                                                                const uint8_t* __restrict__ sel, const int* __restrict__ bad,
                                                                int n_cep, int deltas, const double* __restrict__ mean,
                                                                int* __restrict__ part_n, double* __restrict__ part_sum,
                                                                double* __restrict__ part_sc) {
    __shared__ double feat[kMomChunk * kMaxDim];    // [t][C]
    __shared__ uint8_t sel_s[kMomChunk];
    const int s = blockIdx.y, ch = blockIdx.x;
    const Seg g = segs[s];
    const int t_lo = ch * kMomChunk;
    if (t_lo >= g.frames || bad[s]) return;         // (uniform over the block)
    const int cnt = min(kMomChunk, g.frames - t_lo), C = n_cep * (1 + deltas), F = g.frames;
    const double* c = cep + (size_t)g.first_row * n_cep;
    for (int e = threadIdx.x; e < cnt * C; e += kMomThreads) {
        const int t = t_lo + e / C, p = e % C, k = p % n_cep;
        double v;
        if (p < n_cep) {
            v = c[(size_t)t * n_cep + k];
        } else {
            const int a1 = min(t + 1, F - 1), b1 = max(t - 1, 0), a2 = min(t + 2, F - 1), b2 = max(t - 2, 0);
            const double d1 = c[(size_t)a1 * n_cep + k] - c[(size_t)b1 * n_cep + k];
            const double d2 = c[(size_t)a2 * n_cep + k] - c[(size_t)b2 * n_cep + k];
            v = (d1 + 2.0 * d2) / 10.0;
        }
        if (PASS == 2) v = v - mean[(size_t)s * C + p];
        feat[e] = v;
    }
    if (threadIdx.x < cnt) sel_s[threadIdx.x] = sel[g.first_row + t_lo + threadIdx.x];
    __syncthreads();
    const size_t chunk = (size_t)g.first_chunk + ch;
    if (PASS == 1) {
        if (threadIdx.x < C) {
            double acc = 0.0;
            for (int t = 0; t < cnt; ++t)
                if (sel_s[t]) acc += feat[t * C + threadIdx.x];
            part_sum[chunk * C + threadIdx.x] = acc;
        }
        if (threadIdx.x == kMomThreads - 1) {
            int n = 0;
            for (int t = 0; t < cnt; ++t) n += sel_s[t];
            part_n[chunk] = n;
        }
    } else {
        const int T = tri_count(C);
        for (int e = threadIdx.x; e < T; e += kMomThreads) {
            int p, q;
            tri_entry(e, C, &p, &q);
            double acc = 0.0;
            for (int t = 0; t < cnt; ++t)
                if (sel_s[t]) acc += feat[t * C + p] * feat[t * C + q];
            part_sc[chunk * T + e] = acc;
        }
    }
}

// PASS 1: count[s] and mean[s][C]; PASS 2: scatter[s][T].  grid (ceil(entries / kMomThreads), S)
template <int PASS>
__global__ __launch_bounds__(kMomThreads) void mom_fold_kernel(const Seg* __restrict__ segs, const int* __restrict__ bad, int C,
                                                               const int* __restrict__ part_n, const double* __restrict__ part_sum,
                                                               const double* __restrict__ part_sc, int* __restrict__ count,
                                                               double* __restrict__ mean, double* __restrict__ scatter) {
    const int s = blockIdx.y, e = blockIdx.x * kMomThreads + threadIdx.x;
    const int T = tri_count(C), entries = PASS == 1 ? C : T;
    if (e >= entries) return;
    const Seg g = segs[s];
    const int chunks = (g.frames + kMomChunk - 1) / kMomChunk;
    double* dst = PASS == 1 ? mean + (size_t)s * C + e : scatter + (size_t)s * T + e;
    if (bad[s]) {
        *dst = __builtin_nan("");
        if (PASS == 1 && e == 0) count[s] = -1;
        return;
    }
    double acc = 0.0;
    if (PASS == 1) {
        int n = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            n += part_n[g.first_chunk + ch];
            acc += part_sum[((size_t)g.first_chunk + ch) * C + e];
        }
        *dst = n > 0 ? acc / (double)n : 0.0;
        if (e == 0) count[s] = n;
    } else {
        for (int ch = 0; ch < chunks; ++ch) acc += part_sc[((size_t)g.first_chunk + ch) * T + e];
        *dst = acc;
    }
}

// ---------------------------------------------------------------------------------------------------- the divergence
__device__ __forceinline__ int low(int r, int c) { return r * (r + 1) / 2 + c; }             // packed lower triangle, r >= c
__device__ __forceinline__ int up(int p, int q, int C) { return p * C - p * (p - 1) / 2 + (q - p); }   // the records' packed upper, p <= q

// x = L^-1 rhs for one column: rows r = c0 .. C - 1 of `x` (stride xs between rows: a packed column, or a vector), the rows above
// c0 being zero; returns the sum of x_r^2, r ascending.  rhs_r is read from x's own slot, where the caller has put it.
__device__ __forceinline__ double solve_column(const double* __restrict__ L, int C, int c0, double* x, bool packed) {
    double sum = 0.0;
    for (int r = c0; r < C; ++r) {
        double* xr = packed ? x + low(r, c0) : x + r;
        double s = *xr;
        for (int k = c0; k < r; ++k) s = s - L[low(r, k)] * (packed ? x[low(k, c0)] : x[k]);
        const double v = s / L[low(r, r)];
        *xr = v;
        sum += v * v;
    }
    return sum;
}

__global__ __launch_bounds__(kPairThreads) void gauss_pair_kernel(const int* __restrict__ a_count, const double* __restrict__ a_mean,
                                                                  const double* __restrict__ a_scatter, const int* __restrict__ b_count,
                                                                  const double* __restrict__ b_mean, const double* __restrict__ b_scatter,
                                                                  int C, const int* __restrict__ ii, const int* __restrict__ jj,
                                                                  double* __restrict__ terms, int* __restrict__ status) {
    __shared__ double Li[kTri], Lj[kTri], X[kTri];
    __shared__ double zi[kMaxDim], zj[kMaxDim], col[kMaxDim], diag[2], out_s[4];
    __shared__ int singular;
    const int p = blockIdx.x, t = threadIdx.x, T = tri_count(C);
    const int i = ii[p], j = jj[p];
    const int ni = a_count[i], nj = b_count[j];
    if (t == 0) singular = ni <= C || nj <= C ? 1 : 0;
    __syncthreads();
    if (singular) {                                 // (uniform over the block)
        if (t < 4) terms[(size_t)p * 4 + t] = __builtin_nan("");
        if (t == 0) status[p] = 1;
        return;
    }
    __syncthreads();                                // every thread has read `singular` before a pivot below may set it
    const double* Si = a_scatter + (size_t)i * T;
    const double* Sj = b_scatter + (size_t)j * T;
    const double dni = (double)ni, dnj = (double)nj;
    // both factors, column by column; thread t owns row t
    for (int c = 0; c < C; ++c) {
        double si = 0.0, sj = 0.0;
        if (t >= c && t < C) {
            si = Si[up(c, t, C)] / dni;
            sj = Sj[up(c, t, C)] / dnj;
            for (int k = 0; k < c; ++k) {
                si = si - Li[low(t, k)] * Li[low(c, k)];
                sj = sj - Lj[low(t, k)] * Lj[low(c, k)];
            }
        }
        if (t == c) {
            if (!(si > 0.0) || !(si - si == 0.0) || !(sj > 0.0) || !(sj - sj == 0.0)) singular = 1;
            diag[0] = sqrt(si), diag[1] = sqrt(sj);
            Li[low(c, c)] = diag[0], Lj[low(c, c)] = diag[1];
        }
        __syncthreads();
        if (t > c && t < C) {
            Li[low(t, c)] = si / diag[0];
            Lj[low(t, c)] = sj / diag[1];
        }
        __syncthreads();
    }
    if (singular) {
        if (t < 4) terms[(size_t)p * 4 + t] = __builtin_nan("");
        if (t == 0) status[p] = 1;
        return;
    }
    // X = Li^-1 Lj, then Y = Lj^-1 Li, in the same buffer; thread c owns column c
    for (int side = 0; side < 2; ++side) {
        const double* L = side ? Lj : Li;
        const double* R = side ? Li : Lj;
        if (t < C) {
            for (int r = t; r < C; ++r) X[low(r, t)] = R[low(r, t)];
            col[t] = solve_column(L, C, t, X, true);
        }
        __syncthreads();
        if (t == 0) {
            double tr = 0.0;
            for (int c = 0; c < C; ++c) tr += col[c];
            out_s[side] = tr;
        }
        __syncthreads();
    }
    if (t < 2) {                                    // the mean terms: thread 0 with Li, thread 1 with Lj
        double* z = t ? zj : zi;
        for (int r = 0; r < C; ++r) z[r] = a_mean[(size_t)i * C + r] - b_mean[(size_t)j * C + r];
        out_s[2 + t] = solve_column(t ? Lj : Li, C, 0, z, false);
    }
    __syncthreads();
    if (t < 4) terms[(size_t)p * 4 + t] = out_s[t];
    if (t == 0) status[p] = 0;
}

// ---------------------------------------------------------------------------------------------------- host side
struct Counts {
    long long rows, chunks;
    int max_chunks;
};

int check_counts(const char* who, int S, const int32_t* frames_host, int n_cep, int deltas, Counts* out) {
    if (S < 1 || S > kMaxSegs) return fail(F5_EINVAL, "%s: need 1 <= S <= %d segments (S = %d)", who, kMaxSegs, S);
    if (!frames_host) return fail(F5_EINVAL, "%s: null frames_host", who);
    if (n_cep < 1 || n_cep > kMaxCep) return fail(F5_EINVAL, "%s: n_cep = %d (need 1 <= n_cep <= min(%d, n_mels - 1))", who, n_cep, kMaxCep);
    if (deltas != 0 && deltas != 1) return fail(F5_EINVAL, "%s: deltas = %d (need 0 or 1)", who, deltas);
    const int C = n_cep * (1 + deltas);
    const long long per_chunk = C + tri_count(C);
    Counts c{0, 0, 0};
    for (int s = 0; s < S; ++s) {
        const int f = frames_host[s];
        if (f < 1 || f > kMaxFrames) return fail(F5_EINVAL, "%s: segment %d has frames = %d (need 1 <= frames <= %d)", who, s, f, kMaxFrames);
        const int ch = (f + kMomChunk - 1) / kMomChunk;
        c.rows += f;
        c.chunks += ch;
        c.max_chunks = std::max(c.max_chunks, ch);
        if (c.rows * (n_cep + 1) > kMaxValues || c.chunks * per_chunk > kMaxValues)
            return fail(F5_EINVAL, "%s: more than 2^28 cepstral or partial values in one call at segment %d (split the batch)", who, s);
    }
    *out = c;
    return F5_OK;
}

// the tables of one call, table[n_mels * n_cep] | segs[S]: one layout for slot and device.  The workspace keeps room for the table of
// kMaxMels bins, so that the plan needs no n_mels.
size_t table_bytes(int S, int n_mels, int n_cep) { return (size_t)n_mels * n_cep * 8 + (size_t)S * sizeof(Seg); }

struct Carve {
    double *cep, *energy, *part_sum, *part_sc;
    int *part_n, *bad;
    uint8_t* sel;
    char* tab;
};
size_t carve(Arena& a, const Counts& c, int S, int n_cep, int deltas, Carve* out) {
    const int C = n_cep * (1 + deltas);
    a.reset();
    out->cep = a.take<double>((size_t)c.rows * n_cep);
    out->energy = a.take<double>((size_t)c.rows);
    out->part_sum = a.take<double>((size_t)c.chunks * C);
    out->part_sc = a.take<double>((size_t)c.chunks * tri_count(C));
    out->part_n = a.take<int>((size_t)c.chunks);
    out->bad = a.take<int>((size_t)S);
    out->sel = a.take<uint8_t>((size_t)c.rows);
    out->tab = a.take<char>(table_bytes(S, kMaxMels, n_cep));
    return align_up(a.off, 256) + 256;
}
}  // namespace

extern "C" int f5_cep_moments_plan(int32_t S, const int32_t* frames_host, int32_t n_cep, int32_t deltas, int64_t* workspace_bytes_out) {
    const char* who = "f5_cep_moments_plan";
    if (!workspace_bytes_out) return fail(F5_EINVAL, "%s: null workspace_bytes_out", who);
    Counts c;
    CHK(check_counts(who, S, frames_host, n_cep, deltas, &c));
    Arena dry;
    Carve cv;
    *workspace_bytes_out = (int64_t)carve(dry, c, S, n_cep, deltas, &cv);
    return F5_OK;
}

extern "C" int f5_cep_moments(const float* base, int32_t S, const int64_t* start_host, const int32_t* frames_host, int64_t row_stride,
                              int32_t n_mels, int32_t n_cep, int32_t deltas, const uint8_t* mask, double gate_sum, int32_t* count,
                              double* mean, double* scatter, f5_stream stream) {
    const char* who = "f5_cep_moments";
    hipStream_t s = (hipStream_t)stream;
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!count) return fail(F5_EINVAL, "%s: null count", who);
    if (!mean) return fail(F5_EINVAL, "%s: null mean", who);
    if (!scatter) return fail(F5_EINVAL, "%s: null scatter", who);
    if (n_mels < kMinMels || n_mels > kMaxMels)
        return fail(F5_EINVAL, "%s: n_mels = %d (need %d <= n_mels <= %d)", who, n_mels, kMinMels, kMaxMels);
    if (n_cep > n_mels - 1) return fail(F5_EINVAL, "%s: n_cep = %d (need 1 <= n_cep <= min(%d, n_mels - 1))", who, n_cep, kMaxCep);
    if (row_stride < n_mels) return fail(F5_EINVAL, "%s: row_stride = %lld is less than n_mels = %d", who, (long long)row_stride, n_mels);
    if (gate_sum != gate_sum) return fail(F5_EINVAL, "%s: gate_sum is NaN (negative: no gate)", who);
    Counts c;
    CHK(check_counts(who, S, frames_host, n_cep, deltas, &c));
    for (int g = 0; g < S; ++g)
        if (start_host[g] < 0) return fail(F5_EINVAL, "%s: segment %d has start = %lld < 0", who, g, (long long)start_host[g]);
    const int C = n_cep * (1 + deltas), T = tri_count(C);
    const long long total = c.rows * (n_cep + 1);   // one thread per (row, k) and one per row's energy
    const size_t tab_bytes = table_bytes(S, n_mels, n_cep);

    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    Arena dry;
    Carve cv;
    CHK(st->arena.reserve(carve(dry, c, S, n_cep, deltas, &cv)));
    (void)carve(st->arena, c, S, n_cep, deltas, &cv);
    CHK(st->enter(s));
    CHK(st->stage.upload(cv.tab, tab_bytes, s, [&](char* host) {
        double* table = reinterpret_cast<double*>(host);
        Seg* segs = reinterpret_cast<Seg*>(table + (size_t)n_mels * n_cep);
        const double norm = std::sqrt(2.0 / n_mels);
        for (int j = 0; j < n_mels; ++j)
            for (int k = 1; k <= n_cep; ++k) table[(size_t)j * n_cep + (k - 1)] = norm * std::cos(M_PI * k * (j + 0.5) / n_mels);
        int row = 0, chunk = 0;
        for (int g = 0; g < S; ++g) {
            segs[g] = Seg{start_host[g], row, frames_host[g], chunk, 0};
            row += frames_host[g];
            chunk += (frames_host[g] + kMomChunk - 1) / kMomChunk;
        }
    }));
    const double* table = reinterpret_cast<const double*>(cv.tab);
    const Seg* segs = reinterpret_cast<const Seg*>(table + (size_t)n_mels * n_cep);
    const unsigned grid = (unsigned)((total + kCepThreads - 1) / kCepThreads);
    mom_cepstra_kernel<<<dim3(grid), kCepThreads, 0, s>>>(base, segs, S, row_stride, table, n_mels, n_cep, total, cv.cep, cv.energy);
    KCHK();
    mom_select_kernel<<<dim3((unsigned)S), kSelThreads, 0, s>>>(segs, cv.energy, mask, gate_sum, cv.sel, cv.bad);
    KCHK();
    const dim3 chunks((unsigned)c.max_chunks, (unsigned)S);
    mom_chunk_kernel<1><<<chunks, kMomThreads, 0, s>>>(segs, cv.cep, cv.sel, cv.bad, n_cep, deltas, nullptr, cv.part_n, cv.part_sum, nullptr);
    KCHK();
    mom_fold_kernel<1><<<dim3(1, (unsigned)S), kMomThreads, 0, s>>>(segs, cv.bad, C, cv.part_n, cv.part_sum, nullptr, count, mean, nullptr);
    KCHK();
    mom_chunk_kernel<2><<<chunks, kMomThreads, 0, s>>>(segs, cv.cep, cv.sel, cv.bad, n_cep, deltas, mean, nullptr, nullptr, cv.part_sc);
    KCHK();
    mom_fold_kernel<2><<<dim3((unsigned)((T + kMomThreads - 1) / kMomThreads), (unsigned)S), kMomThreads, 0, s>>>(
        segs, cv.bad, C, nullptr, nullptr, cv.part_sc, nullptr, nullptr, scatter);
    KCHK();
    return st->leave(s);
}

extern "C" int f5_gauss_divergence(const int32_t* a_count, const double* a_mean, const double* a_scatter, int32_t a_records,
                                   const int32_t* b_count, const double* b_mean, const double* b_scatter, int32_t b_records, int32_t C,
                                   int32_t P, const int32_t* i_host, const int32_t* j_host, double* terms, int32_t* status,
                                   f5_stream stream) {
    const char* who = "f5_gauss_divergence";
    hipStream_t s = (hipStream_t)stream;
    if (!a_count) return fail(F5_EINVAL, "%s: null a_count", who);
    if (!a_mean) return fail(F5_EINVAL, "%s: null a_mean", who);
    if (!a_scatter) return fail(F5_EINVAL, "%s: null a_scatter", who);
    if (!b_count) return fail(F5_EINVAL, "%s: null b_count", who);
    if (!b_mean) return fail(F5_EINVAL, "%s: null b_mean", who);
    if (!b_scatter) return fail(F5_EINVAL, "%s: null b_scatter", who);
    if (!i_host) return fail(F5_EINVAL, "%s: null i_host", who);
    if (!j_host) return fail(F5_EINVAL, "%s: null j_host", who);
    if (!terms) return fail(F5_EINVAL, "%s: null terms", who);
    if (!status) return fail(F5_EINVAL, "%s: null status", who);
    if (C < 1 || C > kMaxDim) return fail(F5_EINVAL, "%s: C = %d (need 1 <= C <= %d)", who, C, kMaxDim);
    if (P < 1 || P > kMaxSegs) return fail(F5_EINVAL, "%s: need 1 <= P <= %d pairs (P = %d)", who, kMaxSegs, P);
    if (a_records < 1) return fail(F5_EINVAL, "%s: a_records = %d (need at least one)", who, a_records);
    if (b_records < 1) return fail(F5_EINVAL, "%s: b_records = %d (need at least one)", who, b_records);
    for (int p = 0; p < P; ++p) {
        if (i_host[p] < 0 || i_host[p] >= a_records)
            return fail(F5_EINVAL, "%s: pair %d has i = %d outside the %d records of a", who, p, i_host[p], a_records);
        if (j_host[p] < 0 || j_host[p] >= b_records)
            return fail(F5_EINVAL, "%s: pair %d has j = %d outside the %d records of b", who, p, j_host[p], b_records);
    }
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    const size_t bytes = 2 * (size_t)P * sizeof(int32_t);
    CHK(st->reserve_tables(bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, bytes, s, [&](char* host) {
        int32_t* h = reinterpret_cast<int32_t*>(host);
        for (int p = 0; p < P; ++p) h[p] = i_host[p], h[P + p] = j_host[p];
    }));
    const int* d = reinterpret_cast<const int*>(tab);
    gauss_pair_kernel<<<dim3((unsigned)P), kPairThreads, 0, s>>>(a_count, a_mean, a_scatter, b_count, b_mean, b_scatter, C, d, d + P, terms,
                                                                 status);
    KCHK();
    return st->leave(s);
}
