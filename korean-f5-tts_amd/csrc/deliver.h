// The delivery stage of include/f5_hip.h, once, for the two kernels that run it: deliver.hip reads a block's window from a buffer,
// emit.hip folds it from a stream's pieces (join.h).  The per-item geometry, the host arithmetic (rate, lengths, blocks), the store
// of a thread's four samples in the item's format, and what a block does once its window stands in LDS.
#pragma once
#include <algorithm>

#include "resample.h"
#include "segments.h"

namespace f5 {
constexpr int DELIVER_STREAM_RATE = 24000;
constexpr long long DELIVER_MAX_UNITS = 1LL << 30;   // blocks of one call

struct DeliverItem {
    long long in_start, out_start, o0, o1;    // elements from base / out; the output range in samples of the resampled stream
    const float* bank;                        // [K, new], null for a stream at the output rate
    int n, orig, nw, width, K, F;             // F frames per block
};

// the rate geometry of 24 kHz -> out_rate, or the refusal
inline int deliver_rate(const char* who, int out_rate, RatePair* r) {
    if (out_rate < 8000 || out_rate > 192000) return f5_fail(F5_EINVAL, "%s: out_rate = %d (need 8000 <= out_rate <= 192000)", who, out_rate);
    if (!rate_pair(DELIVER_STREAM_RATE, out_rate, r) || (!r->same() && r->K > RS_LDS_FLOATS))
        return f5_fail(F5_EINVAL, "%s: the resample bank of %d Hz -> %d Hz has more than 2^20 elements", who, DELIVER_STREAM_RATE, out_rate);
    return F5_OK;
}
inline long long deliver_floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline void deliver_lengths(const RatePair& r, long long n, bool final, long long* len, long long* ready) {
    *len = (r.nw * n + r.orig - 1) / r.orig;
    // output frame i reads inputs up to i * orig + width + orig - 1
    *ready = final ? *len : std::min(r.nw * std::max(0LL, deliver_floor_div(n - r.width - r.orig, r.orig) + 1), *len);
}
// blocks the non-empty range [o0, o1) takes with F frames per block (F = 0: a stream at the output rate)
inline long long deliver_blocks(const RatePair& r, int F, long long o0, long long o1) {
    if (r.same()) return (o1 - o0 + RS_OUT_TILE - 1) / RS_OUT_TILE;
    return ((o1 + r.nw - 1) / r.nw - o0 / r.nw + F - 1) / F;
}

// four consecutive samples at element d of the item's output: one vector store where all four are inside [d0, d1) and the address
// allows, element stores otherwise
static __device__ __forceinline__ void store_quad(void* __restrict__ out, int format, long long at, long long d, long long d0, long long d1,
                                                  const float (&v)[4]) {
    const bool full = d >= d0 && d + 4 <= d1;
    if (format == F5_PCM_F32) {
        float* dst = reinterpret_cast<float*>(out) + at + d;
        if (full && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int q = 0; q < 4; ++q)
                if (d + q >= d0 && d + q < d1) dst[q] = v[q];
        }
    } else {
        short* dst = reinterpret_cast<short*>(out) + at + d;
        short s[4];
        for (int q = 0; q < 4; ++q) s[q] = (short)quantise(v[q], 32767.0f);
        if (full && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
            *reinterpret_cast<short4*>(dst) = make_short4(s[0], s[1], s[2], s[3]);
        } else {
            for (int q = 0; q < 4; ++q)
                if (d + q >= d0 && d + q < d1) dst[q] = s[q];
        }
    }
}

// A block's window: the frames from frame0 on, `win` samples of the unpadded stream from position win0 (which may be negative or
// reach past n: the zero padding, by index logic)
struct DeliverWindow {
    long long frame0, win0;
    int win;                                  // <= RS_LDS_FLOATS by the host's choice of F
};
static __device__ __forceinline__ DeliverWindow deliver_window(const DeliverItem& it, long long tile) {
    DeliverWindow w;
    w.frame0 = it.o0 / it.nw + tile * it.F;
    w.win0 = w.frame0 * it.orig - it.width;
    w.win = (it.F - 1) * it.orig + it.K;
    return w;
}

// The block's outputs from its window xs (staged, and the block synchronised): per output sample the taps in ascending order.  A
// thread's four samples are aligned to the item's destination.
static __device__ __forceinline__ void deliver_from_window(const DeliverItem& it, long long frame0, const float* xs, int format,
                                                           void* __restrict__ out) {
    const long long d0 = max(it.o0, frame0 * it.nw) - it.o0;
    const long long d1 = min(it.o1, (frame0 + it.F) * it.nw) - it.o0;
    for (long long d = (d0 & ~3LL) + 4 * (long long)threadIdx.x; d < d1; d += RS_OUT_TILE) {
        int xi[4], bp[4];
        for (int q = 0; q < 4; ++q) {
            const long long dq = (d + q >= d0 && d + q < d1) ? d + q : d0;   // a lane outside the range repeats a valid sample and stores nothing
            const long long o = it.o0 + dq;
            const long long f = o / it.nw;
            xi[q] = (int)(f - frame0) * it.orig;
            bp[q] = (int)(o - f * it.nw);
        }
        float acc[4];
        resample_taps(it.bank, it.nw, it.K, xi, bp, [&](int e) { return xs[e]; }, acc);
        store_quad(out, format, it.out_start, d, d0, d1, acc);
    }
}
}  // namespace f5
