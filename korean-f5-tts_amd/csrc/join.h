// The join of f5_wave_join (include/f5_hip.h), once, for the kernels that fold pieces into a waveform: wave.hip writes the joined
// waveform out, emit.hip folds the samples a block of the delivery stage needs straight into its window.  The piece table, its
// host plan in exact integers, the bisection to the first piece of a span, and one piece folded into the four samples of a thread.
#pragma once
#include <algorithm>

#include "segments.h"

namespace f5 {
constexpr int JOIN_PER_THREAD = 4;                  // consecutive samples per thread: one 16-byte store

// One entry per piece, in a pinned slot and then in the workspace (internal.h)
struct JoinPiece {
    long long src;               // first sample, in elements from base
    long long off;               // position of the piece's first sample in the output
    long long end;               // off + len = L_i: never decreases with i
    long long low;               // min of off over this piece and every later one
    double step;
    int n, len;
};

// The host plan piece by piece: L the result so far, R the run so far.  place() fills everything of a piece but `low`, which
// close() fills over the finished table.
struct JoinRun {
    long long L = 0, R = 0;
    void place(bool first, long long src, int len, int fade, JoinPiece* pc) {
        const bool opens = first || fade == 0;                     // a piece that does not fade opens a run
        const long long n = opens ? 0 : std::min<long long>(std::min<long long>(fade, R), len);
        pc->src = src;
        pc->off = L - n;
        pc->end = L = pc->off + len;
        pc->step = n > 1 ? 1.0 / (double)(n - 1) : 0.0;
        pc->n = (int)n, pc->len = len;
        R = opens ? len : R - n + len;
    }
    void close(JoinPiece* pieces, int B) const {
        long long low = L;
        for (int i = B - 1; i >= 0; --i) pieces[i].low = low = std::min(low, pieces[i].off);
    }
};

// One piece folded into the four samples [p0, p0 + 4) a thread holds: piece x covers [off, off + len) of the output and its first n
// samples fade in over what v holds (the contract in include/f5_hip.h).  Nothing outside [0, len) of x is read.
__device__ __forceinline__ void fold_piece(const float* __restrict__ x, long long off, int len, int n, double step, long long p0,
                                           double (&v)[JOIN_PER_THREAD]) {
    const long long j0 = p0 - off;
    if (j0 >= len || j0 + JOIN_PER_THREAD <= 0) return;
    float xv[JOIN_PER_THREAD];
    if (j0 >= 0 && j0 + JOIN_PER_THREAD <= len) {
        __builtin_memcpy(xv, x + j0, sizeof(xv));                 // 4-byte aligned, inside the piece
    } else {
#pragma unroll
        for (int e = 0; e < JOIN_PER_THREAD; ++e) {
            const long long j = j0 + e;
            xv[e] = (j >= 0 && j < len) ? x[j] : 0.0f;
        }
    }
#pragma unroll
    for (int e = 0; e < JOIN_PER_THREAD; ++e) {
        const long long j = j0 + e;
        if (j < 0 || j >= len) continue;
        if (j < n) {
            double fi, fo;
            fade_weights(j, n, step, &fi, &fo);
            v[e] = v[e] * fo + (double)xv[e] * fi;
        } else {
            v[e] = (double)xv[e];
        }
    }
}

// the first piece that ends behind t0 (the last piece where none does: nothing of it is folded then)
__device__ __forceinline__ int first_piece(const JoinPiece* __restrict__ pieces, int B, long long t0) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pieces[mid].end > t0) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The fold of the joined waveform at [p0, p0 + 4) into v (zeros on entry), for a thread of a block whose span ends at t1 and whose
// first piece is `lo` (first_piece of the span's start): walks up while a later piece can still start inside the span.  The loop
// is block-uniform up to fold_piece.
__device__ __forceinline__ void fold_pieces(const float* __restrict__ base, const JoinPiece* __restrict__ pieces, int B, int lo, long long t1,
                                            long long p0, double (&v)[JOIN_PER_THREAD]) {
    for (int i = lo; i < B; ++i) {
        const JoinPiece pc = pieces[i];
        if (pc.low >= t1) break;                              // neither this piece nor a later one starts inside the span
        if (pc.off >= t1) continue;
        fold_piece(base + pc.src, pc.off, pc.len, pc.n, pc.step, p0, v);
    }
}
}  // namespace f5
