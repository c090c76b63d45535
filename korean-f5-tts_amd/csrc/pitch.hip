// YIN pitch tracks of a ragged batch of waveforms on gfx950 (the contract is in include/f5_hip.h): the F0 of what the vocoder made of
// sample()'s output and of the recording it is scored against, frame for frame on the mel front-end's grid, on the device.
//   pitch_track_kernel   one workgroup of kPitchThreads per frame.  The frame's L = W + tau_max + 1 samples go to LDS as f32 (a sample
//                        outside the item reads as 0).  The difference function: one thread per lag tau (lags kPitchThreads apart
//                        when there are more), d(tau) = sum_j (x[j] - x[j + tau])^2 in f64, j ascending -- every lane reads x[j] as
//                        an LDS broadcast and x[j + tau] at consecutive addresses, so no bank is hit twice -- with no cross-lane
//                        reduction: the order of the sum is the contract's.  Thread 0 then runs the cumulative sum S over the lags
//                        (the only dependent chain: tau_max + 1 additions), every thread normalises its own lags, d'(tau) =
//                        d(tau) tau / S(tau), and thread 0 makes the choice and the parabolic step.  Everything after the samples
//                        is f64, compiled without contraction: adds, multiplies, divides and compares in the contract's order.
// Stand-alone like the silence stage and the DTW: no handle, the per-device workspace of the handle-less calls for the item table,
// one table copy through a pinned slot, no host read, no synchronisation except the growth of that workspace, no atomics.  A frame
// reads its own item only, so an item's track is the same alone and in any batch.
#include <cmath>
#include <cstdint>

#include "internal.h"

#define fail f5_fail

namespace {
constexpr int kPitchThreads = 256;
constexpr int kMaxItems = 65535, kMinWindow = 64, kMaxWindow = 2048, kMinTau = 2, kMaxTau = 1024;
constexpr int kMaxSamples = kMaxWindow + kMaxTau + 1;   // L at most
constexpr long long kMaxTrackFrames = 1LL << 22;        // frames of one call
constexpr int kMaxHop = 1 << 20, kMaxCentre = 1 << 30, kMaxRate = 1 << 20;

struct Item {
    long long start;                                // the item's first sample, in elements from base
    int len, frames;
    int first_frame, pad;                           // its first frame among the frames of the call
};
static_assert(sizeof(Item) == 24, "table layout");

// the last entry of items[0 .. n) whose first_frame is <= f (ascending, items[0].first_frame = 0)
__device__ __forceinline__ int item_of_frame(const Item* __restrict__ items, int n, int f) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].first_frame <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kPitchThreads) void pitch_track_kernel(const float* __restrict__ base, const Item* __restrict__ items, int P,
                                                                    double rate, int hop, int first_centre, int W, int tau_min,
                                                                    int tau_max, double threshold, double* __restrict__ f0,
                                                                    double* __restrict__ ap) {
    __shared__ float x[kMaxSamples];
    __shared__ double d[kMaxTau + 2];               // d(tau), then d'(tau), tau = 1 .. tau_max + 1 (slot 0 unused)
    __shared__ double S[kMaxTau + 2];
    const int frame = blockIdx.x, t = threadIdx.x;
    const Item it = items[item_of_frame(items, P, frame)];
    const int L = W + tau_max + 1;
    const long long s0 = (long long)first_centre + (long long)(frame - it.first_frame) * hop - L / 2;
    const float* src = base + it.start;
    for (int e = t; e < L; e += kPitchThreads) {
        const long long idx = s0 + e;
        x[e] = idx >= 0 && idx < it.len ? src[idx] : 0.0f;
    }
    __syncthreads();
    for (int tau = 1 + t; tau <= tau_max + 1; tau += kPitchThreads) {
        const float* y = x + tau;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < W; ++j) {
            const double diff = (double)x[j] - (double)y[j];
            acc += diff * diff;
        }
        d[tau] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        for (int tau = 1; tau <= tau_max + 1; ++tau) {
            run += d[tau];
            S[tau] = run;
        }
    }
    __syncthreads();
    for (int tau = 1 + t; tau <= tau_max + 1; tau += kPitchThreads) {
        const double s = S[tau];
        d[tau] = s > 0.0 ? (d[tau] * (double)tau) / s : 1.0;
    }
    __syncthreads();
    if (t != 0) return;
    int tau = 0;
    for (int k = tau_min; k <= tau_max; ++k)
        if (d[k] < threshold) {
            tau = k;
            break;
        }
    double pitch = 0.0, aper;
    if (tau) {
        while (tau + 1 <= tau_max && d[tau + 1] < d[tau]) ++tau;
        const double a = d[tau - 1], b = d[tau], c = d[tau + 1];
        const double den = a - 2.0 * b + c;
        double delta = den > 0.0 ? (0.5 * (a - c)) / den : 0.0;
        delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
        pitch = rate / ((double)tau + delta);
        aper = b;
    } else {
        aper = d[tau_min];
        for (int k = tau_min + 1; k <= tau_max; ++k)
            if (d[k] < aper) aper = d[k];
    }
    f0[frame] = pitch;
    ap[frame] = aper;
}
}  // namespace

extern "C" int f5_pitch_track(const float* base, int32_t P, const int64_t* start_host, const int32_t* len_host, int32_t sample_rate,
                              int32_t hop, int32_t first_centre, const int32_t* frames_host, int32_t window, int32_t tau_min,
                              int32_t tau_max, double threshold, double* f0, double* ap, f5_stream stream) {
    const char* who = "f5_pitch_track";
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!len_host) return fail(F5_EINVAL, "%s: null len_host", who);
    if (!frames_host) return fail(F5_EINVAL, "%s: null frames_host", who);
    if (!f0) return fail(F5_EINVAL, "%s: null f0", who);
    if (!ap) return fail(F5_EINVAL, "%s: null ap", who);
    if (P < 1 || P > kMaxItems) return fail(F5_EINVAL, "%s: need 1 <= P <= %d items (P = %d)", who, kMaxItems, P);
    if (sample_rate < 1 || sample_rate > kMaxRate) return fail(F5_EINVAL, "%s: sample_rate = %d (need 1 <= sample_rate <= %d)", who, sample_rate, kMaxRate);
    if (hop < 1 || hop > kMaxHop) return fail(F5_EINVAL, "%s: hop = %d (need 1 <= hop <= %d)", who, hop, kMaxHop);
    if (first_centre < 0 || first_centre > kMaxCentre)
        return fail(F5_EINVAL, "%s: first_centre = %d (need 0 <= first_centre <= %d)", who, first_centre, kMaxCentre);
    if (window < kMinWindow || window > kMaxWindow)
        return fail(F5_EINVAL, "%s: window = %d (need %d <= window <= %d)", who, window, kMinWindow, kMaxWindow);
    if (tau_min < kMinTau || tau_min >= tau_max || tau_max > kMaxTau)
        return fail(F5_EINVAL, "%s: tau_min = %d, tau_max = %d (need %d <= tau_min < tau_max <= %d)", who, tau_min, tau_max, kMinTau, kMaxTau);
    if (!(threshold > 0.0) || !(threshold <= 1.0)) return fail(F5_EINVAL, "%s: threshold = %g (need 0 < threshold <= 1)", who, threshold);
    long long total = 0;
    for (int p = 0; p < P; ++p) {
        if (start_host[p] < 0) return fail(F5_EINVAL, "%s: item %d has start = %lld < 0", who, p, (long long)start_host[p]);
        if (len_host[p] < 1) return fail(F5_EINVAL, "%s: item %d has len = %d (need len >= 1)", who, p, len_host[p]);
        if (frames_host[p] < 1) return fail(F5_EINVAL, "%s: item %d has frames = %d (need frames >= 1)", who, p, frames_host[p]);
        total += frames_host[p];
        if (total > kMaxTrackFrames)
            return fail(F5_EINVAL, "%s: more than %lld frames in one call at item %d (split the batch)", who, kMaxTrackFrames, p);
    }
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    const size_t tab_bytes = (size_t)P * sizeof(Item);
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        Item* h = reinterpret_cast<Item*>(host);
        int first = 0;
        for (int p = 0; p < P; ++p) {
            h[p] = Item{start_host[p], len_host[p], frames_host[p], first, 0};
            first += frames_host[p];
        }
    }));
    pitch_track_kernel<<<dim3((unsigned)total), kPitchThreads, 0, s>>>(base, reinterpret_cast<const Item*>(tab), P, (double)sample_rate,
                                                                       hop, first_centre, window, tau_min, tau_max, threshold, f0, ap);
    KCHK();
    return st->leave(s);
}
