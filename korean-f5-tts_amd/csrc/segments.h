// The segment table of the waveform stages (edit.hip, silence.hip), the linspace fade (wave.hip, edit.hip) and the 16-bit view of a
// sample (silence.hip, deliver.hip), once: the triple as the caller writes it, the host check every entry point runs over an item's
// table, the device lookup, the quantiser, the fade weights.
#pragma once
#include <cstdint>

#include "internal.h"

struct Seg {                                        // frames [dst, dst + frames) of the result <- [src, src + frames) of the item
    int dst, src, frames;                           // src = -1 (f5_edit_assemble only): an EDIT segment, zero frames
};

// Item b's table as the caller hands it over (three int32 per segment): at least one frame per segment, destinations ascending and
// disjoint and within dst_limit (<= INT32_MAX), no source below min_src (0, or -1 where EDIT segments may come), nothing past 32 bits.
inline int check_segments(const char* who, int b, const int32_t* segs, int count, int min_src, long long dst_limit) {
    long long prev_end = 0;
    for (int s = 0; s < count; ++s) {
        const long long dst = segs[3 * s], src = segs[3 * s + 1], frames = segs[3 * s + 2];
        if (frames < 1) return f5_fail(F5_EINVAL, "%s: item %d segment %d has %lld frames; need at least 1", who, b, s, frames);
        if (src < min_src || src + frames > INT32_MAX)
            return f5_fail(F5_EINVAL, "%s: item %d segment %d has source frame %lld", who, b, s, src);
        if (dst < prev_end)
            return f5_fail(F5_EINVAL, "%s: item %d segment %d starts at frame %lld, inside or before the segment in front of it", who, b,
                           s, dst);
        if (dst + frames > dst_limit)
            return f5_fail(F5_EINVAL, "%s: item %d segment %d ends at frame %lld; the limit is %lld", who, b, s, dst + frames, dst_limit);
        prev_end = dst + frames;
    }
    return F5_OK;
}

// the source frame of frame v of the result, -1 where no segment or an EDIT segment covers it; *hint: the segment found last (or -1)
__device__ __forceinline__ int source_frame(const Seg* __restrict__ segs, int count, int v, int* hint) {
    int k = *hint;
    if (k < 0 || v < segs[k].dst || (k + 1 < count && v >= segs[k + 1].dst)) {
        if (count < 1 || v < segs[0].dst) return -1;
        int lo = 0, hi = count - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[mid].dst <= v) lo = mid;
            else hi = mid - 1;
        }
        k = lo;
        *hint = k;
    }
    const Seg g = segs[k];
    return v < g.dst + g.frames && g.src >= 0 ? g.src + (v - g.dst) : -1;
}

// the 16-bit view of a sample (include/f5_hip.h): f32 multiply, round to nearest even, clamp; NaN is 0
__device__ __forceinline__ int quantise(float x, float qscale) {
    if (!(x == x)) return 0;
    float v = rintf(x * qscale);
    v = fminf(fmaxf(v, -32768.0f), 32767.0f);
    return (int)v;
}

// numpy's linspace(0, 1, n)[j] (*fi) and linspace(1, 0, n)[j] (*fo), j < n, step = 1 / (n - 1) from the host (0 for n < 2): separate
// IEEE double operations (-ffp-contract=off), as written
__device__ __forceinline__ void fade_weights(long long j, int n, double step, double* fi, double* fo) {
    if (n == 1) {
        *fi = 0.0, *fo = 1.0;
    } else if (j == n - 1) {
        *fi = 1.0, *fo = 0.0;                       // linspace sets its last element to `stop`
    } else {
        *fi = (double)j * step + 0.0;
        *fo = (double)j * (-step) + 1.0;
    }
}
