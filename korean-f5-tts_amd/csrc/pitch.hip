// YIN and pYIN pitch tracks of a ragged batch of waveforms on gfx950 (the contracts are in include/f5_hip.h): the F0 of what the
// vocoder made of sample()'s output and of the recording it is scored against, frame for frame on the mel front-end's grid, on the
// device.
//   pitch_track_kernel   one workgroup of kPitchThreads per frame.  The frame's L = W + tau_max + 1 samples go to LDS as f32 (a sample
//                        outside the item reads as 0).  The difference function: one thread per lag tau (lags kPitchThreads apart
//                        when there are more), d(tau) = sum_j (x[j] - x[j + tau])^2 in f64, j ascending -- every lane reads x[j] as
//                        an LDS broadcast and x[j + tau] at consecutive addresses, so no bank is hit twice -- with no cross-lane
//                        reduction: the order of the sum is the contract's.  Thread 0 then runs the cumulative sum S over the lags
//                        (the only dependent chain: tau_max + 1 additions), every thread normalises its own lags, d'(tau) =
//                        d(tau) tau / S(tau), and thread 0 makes the choice and the parabolic step.  Everything after the samples
//                        is f64, compiled without contraction: adds, multiplies, divides and compares in the contract's order.
//   pitch_candidates_kernel
//                        pYIN's stage 1 on the same d' (frame_difference is the one body of both): a thread per threshold i / N
//                        makes YIN's choice, one lane adds the weights to the chosen lags in ascending i -- the order of every sum
//                        is the contract's -- and gathers the lags that got votes; a thread per candidate refines and stores it.
//   pitch_decode_kernel  pYIN's stage 2: one workgroup per item, a thread per pitch bin carrying both voicings, frames the only
//                        sequential axis.  Per frame: the candidates' bins by binary search in the LDS copy of the edges, the
//                        observation summed in array order by every bin for itself, the band maximum over delta of the previous
//                        frame (LDS, ping-pong) times the transition row (global, consecutive bins at consecutive addresses), the
//                        voicing step, one back-pointer byte per state to the caller's workspace, the frame's maximum by a wave
//                        shuffle and an LDS slot per wave (a maximum of exact values: order-free), the division.  Two barriers a
//                        frame; the next frame's candidates are loaded under the band loop and reach LDS a frame ahead.  Then one
//                        lane finds the end state and walks the bytes back, leaving the state in f0, and the workgroup turns
//                        states into the f0 of the chosen candidate.  No transcendental function: every table (weights, edges,
//                        centres, transitions) comes from the host.
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

// The frame's samples into x and its d'(tau), tau = 1 .. tau_max + 1, into d (slot 0 unused; S holds the cumulative sum): the part of
// the contract that f5_pitch_track and f5_pitch_candidates share, by one body.  Every thread of the workgroup calls it and returns
// behind a barrier.
__device__ __forceinline__ void frame_difference(const float* __restrict__ base, const Item* __restrict__ items, int P, int hop,
                                                 int first_centre, int W, int tau_max, float* x, double* d, double* S) {
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
}

// the contract's refinement: the parabola through d'(tau - 1), d'(tau), d'(tau + 1)
__device__ __forceinline__ double refined_f0(const double* d, int tau, double rate) {
    const double a = d[tau - 1], b = d[tau], c = d[tau + 1];
    const double den = a - 2.0 * b + c;
    double delta = den > 0.0 ? (0.5 * (a - c)) / den : 0.0;
    delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
    return rate / ((double)tau + delta);
}

__global__ __launch_bounds__(kPitchThreads) void pitch_track_kernel(const float* __restrict__ base, const Item* __restrict__ items, int P,
                                                                    double rate, int hop, int first_centre, int W, int tau_min,
                                                                    int tau_max, double threshold, double* __restrict__ f0,
                                                                    double* __restrict__ ap) {
    __shared__ float x[kMaxSamples];
    __shared__ double d[kMaxTau + 2];               // d(tau), then d'(tau), tau = 1 .. tau_max + 1 (slot 0 unused)
    __shared__ double S[kMaxTau + 2];
    frame_difference(base, items, P, hop, first_centre, W, tau_max, x, d, S);
    const int frame = blockIdx.x, t = threadIdx.x;
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
        pitch = refined_f0(d, tau, rate);
        aper = d[tau];
    } else {
        aper = d[tau_min];
        for (int k = tau_min + 1; k <= tau_max; ++k)
            if (d[k] < aper) aper = d[k];
    }
    f0[frame] = pitch;
    ap[frame] = aper;
}

// ---------------------------------------------------------------------------------------------------- pYIN, stage 1
constexpr int kMaxThresholds = 256;                 // N at most: one thread per threshold
static_assert(kMaxThresholds <= kPitchThreads, "a thread per threshold");

__global__ __launch_bounds__(kPitchThreads) void pitch_candidates_kernel(const float* __restrict__ base, const Item* __restrict__ items,
                                                                         int P, double rate, int hop, int first_centre, int W,
                                                                         int tau_min, int tau_max, int N, const double* __restrict__ w,
                                                                         double p_absent, int* __restrict__ cand_count,
                                                                         int* __restrict__ cand_lag, double* __restrict__ cand_f0,
                                                                         double* __restrict__ cand_prob) {
    __shared__ float x[kMaxSamples];
    __shared__ double d[kMaxTau + 2];
    __shared__ double S[kMaxTau + 2];               // the cumulative sum, then prob(tau)
    __shared__ double ws[kMaxThresholds];
    __shared__ int vote[kMaxThresholds];            // tau_i, 0: no lag under threshold i
    __shared__ int lags[kMaxThresholds];            // the lags with prob > 0, ascending
    __shared__ int found;
    frame_difference(base, items, P, hop, first_centre, W, tau_max, x, d, S);
    const int frame = blockIdx.x, t = threadIdx.x;
    int bad = 0;
    for (int tau = 1 + t; tau <= tau_max + 1; tau += kPitchThreads) {
        bad |= d[tau] != d[tau];
        S[tau] = 0.0;
    }
    if (t < N) ws[t] = w[t];
    bad = __syncthreads_or(bad);
    const size_t slot0 = (size_t)frame * N;
    if (bad) {                                      // a NaN in d': no candidates
        if (t == 0) cand_count[frame] = 0;
        if (t < N) {
            cand_lag[slot0 + t] = 0;
            cand_f0[slot0 + t] = 0.0;
            cand_prob[slot0 + t] = 0.0;
        }
        return;
    }
    if (t < N) {                                    // YIN's choice at threshold (t + 1) / N
        const double s = (double)(t + 1) / (double)N;
        int tau = 0;
        for (int k = tau_min; k <= tau_max; ++k)
            if (d[k] < s) {
                tau = k;
                break;
            }
        if (tau)
            while (tau + 1 <= tau_max && d[tau + 1] < d[tau]) ++tau;
        vote[t] = tau;
    }
    __syncthreads();
    if (t == 0) {                                   // the votes in ascending i: the order of every lag's sum is the contract's
        int tau_g = 0;
        for (int i = 0; i < N; ++i) {
            const int tau = vote[i];
            if (tau) {
                S[tau] += ws[i];
                continue;
            }
            if (!tau_g) {
                tau_g = tau_min;
                for (int k = tau_min + 1; k <= tau_max; ++k)
                    if (d[k] < d[tau_g]) tau_g = k;
            }
            S[tau_g] += ws[i] * p_absent;
        }
        int n = 0;
        for (int k = tau_min; k <= tau_max; ++k)
            if (S[k] > 0.0) lags[n++] = k;          // (at most one lag per vote: n <= N)
        found = n;
        cand_count[frame] = n;
    }
    __syncthreads();
    if (t >= N) return;
    const bool live = t < found;
    const int tau = live ? lags[t] : 0;
    cand_lag[slot0 + t] = tau;
    cand_f0[slot0 + t] = live ? refined_f0(d, tau, rate) : 0.0;
    cand_prob[slot0 + t] = live ? S[tau] : 0.0;
}

// ---------------------------------------------------------------------------------------------------- pYIN, stage 2
constexpr int kMaxBins = 512, kMinBins = 2, kMaxReach = 63;
constexpr double kObsFloor = 0x1p-60;

struct Span {
    int frames, first_frame;                        // an item's frames among the frames of the call
};
static_assert(sizeof(Span) == 8, "table layout");

// the number of j in [1, M - 1] with edge[j] <= f (edge ascending): 0 for a NaN
__device__ __forceinline__ int bin_of(const double* edge, int M, double f) {
    int lo = 0, hi = M - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (edge[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int clamped(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One workgroup per item, blockDim.x = M rounded up to whole waves; thread j owns bin j in both voicings.
__global__ __launch_bounds__(kMaxBins) void pitch_decode_kernel(const Span* __restrict__ spans, const int* __restrict__ cand_count,
                                                                const double* __restrict__ cand_f0, const double* __restrict__ cand_prob,
                                                                int N, int M, const double* __restrict__ edge,
                                                                const double* __restrict__ centre, int reach,
                                                                const double* __restrict__ trans, double stay, double p_switch,
                                                                unsigned char* __restrict__ trace, double* f0, double* __restrict__ vp) {
    __shared__ double edge_s[kMaxBins + 1];
    __shared__ double delta[2][2][kMaxBins];        // [ping-pong][voicing: 0 unvoiced, 1 voiced][bin]
    __shared__ double cprob[2][kMaxThresholds];     // a frame's candidates: prob and bin, this frame's and the next one's
    __shared__ int cbin[2][kMaxThresholds];
    __shared__ double wave_max[kMaxBins / 64];
    const Span it = spans[blockIdx.x];
    const int t = threadIdx.x, T = blockDim.x;
    for (int e = t; e <= M; e += T) edge_s[e] = edge[e];
    if (t < M) delta[0][0][t] = delta[0][1][t] = 1.0;
    const int lo = t - reach > 0 ? t - reach : 0, hi = t + reach < M - 1 ? t + reach : M - 1;
    const double* tr = trans + t + reach;           // trans[i][t - i + reach] is tr[i * 2 * reach]
    const size_t step = 2 * (size_t)reach;
    unsigned char* tb = trace + (size_t)it.first_frame * 2 * M;   // [frame][destination voicing][bin]
    int cur = 0;
    __syncthreads();
    // A frame's candidates go to LDS one frame ahead: their loads are issued before the band loop of the frame before and land
    // behind it, off the chain from frame to frame.  Thread t holds slots t, t + T, ... (at most kSlots, as T >= 64).
    constexpr int kSlots = kMaxThresholds / 64;
    int cnt = clamped(cand_count[it.first_frame], N);
    for (int c = t; c < cnt; c += T) {
        cprob[0][c] = cand_prob[(size_t)it.first_frame * N + c];
        cbin[0][c] = bin_of(edge_s, M, cand_f0[(size_t)it.first_frame * N + c]);
    }
    __syncthreads();
    for (int f = 0; f < it.frames; ++f) {
        const size_t g = (size_t)it.first_frame + f;
        const bool more = f + 1 < it.frames;
        int next_cnt = 0;
        double next_f0[kSlots], next_prob[kSlots];
        if (more) {
            next_cnt = clamped(cand_count[g + 1], N);
#pragma unroll
            for (int k = 0; k < kSlots; ++k) {
                const int c = t + k * T;
                next_f0[k] = c < N ? cand_f0[(g + 1) * N + c] : 0.0;
                next_prob[k] = c < N ? cand_prob[(g + 1) * N + c] : 0.0;
            }
        }
        const double* prob_s = cprob[f & 1];
        const int* bin_s = cbin[f & 1];
        double nu = 0.0, nv = 0.0, mx = 0.0;
        if (t < M) {
            double ov = 0.0, tot = 0.0;
            for (int c = 0; c < cnt; ++c) {
                const double p = prob_s[c];
                if (bin_s[c] == t) ov += p;
                tot += p;
            }
            if (t == 0) vp[g] = tot;
            double ou = 1.0 - tot;
            ou = (ou > 0.0 ? ou : 0.0) / (double)M;
            ou = ou > kObsFloor ? ou : kObsFloor;
            ov = ov > kObsFloor ? ov : kObsFloor;
            const double* du = delta[cur][0];
            const double* dv = delta[cur][1];
            double bu = -1.0, bv = -1.0;            // (every product is >= 0: the first i always takes over)
            int iu = lo, iv = lo;
#pragma unroll 4
            for (int i = lo; i <= hi; ++i) {
                const double a = tr[i * step];
                const double pu = du[i] * a, pv = dv[i] * a;
                if (pu > bu) {
                    bu = pu;
                    iu = i;
                }
                if (pv > bv) {
                    bv = pv;
                    iv = i;
                }
            }
            double c0 = bu * stay, c1 = bv * stay;  // into unvoiced, into voiced: the same voicing unless the other is larger
            int s0 = 0, s1 = 1, i0 = iu, i1 = iv;
            const double x0 = bv * p_switch, x1 = bu * p_switch;
            if (x0 > c0) {
                c0 = x0;
                s0 = 1;
                i0 = iv;
            }
            if (x1 > c1) {
                c1 = x1;
                s1 = 0;
                i1 = iu;
            }
            nu = ou * c0;
            nv = ov * c1;
            unsigned char* row = tb + (size_t)f * 2 * M;
            row[t] = (unsigned char)((s0 << 7) | (i0 - t + reach));
            row[M + t] = (unsigned char)((s1 << 7) | (i1 - t + reach));
            mx = nu > nv ? nu : nv;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
        if ((t & 63) == 0) wave_max[t >> 6] = mx;
        if (more) {                                 // (the other buffer was last read a frame ago, two barriers back)
#pragma unroll
            for (int k = 0; k < kSlots; ++k) {
                const int c = t + k * T;
                if (c < next_cnt) {
                    cprob[(f + 1) & 1][c] = next_prob[k];
                    cbin[(f + 1) & 1][c] = bin_of(edge_s, M, next_f0[k]);
                }
            }
        }
        cnt = next_cnt;
        __syncthreads();
        double top = wave_max[0];
        for (int k = 1; k < (T >> 6); ++k) top = wave_max[k] > top ? wave_max[k] : top;
        if (t < M) {
            delta[cur ^ 1][0][t] = top > 0.0 ? nu / top : nu;
            delta[cur ^ 1][1][t] = top > 0.0 ? nv / top : nv;
        }
        cur ^= 1;
        __syncthreads();
    }
    if (t == 0) {                                   // the end state, then the walk back: f0 holds 0 or the voiced bin + 1 for now
        const double* du = delta[cur][0];
        const double* dv = delta[cur][1];
        double best = du[0];
        int v = 0, m = 0;
        for (int i = 1; i < M; ++i)
            if (du[i] > best) {
                best = du[i];
                m = i;
            }
        for (int i = 0; i < M; ++i)
            if (dv[i] > best) {
                best = dv[i];
                v = 1;
                m = i;
            }
        for (int f = it.frames - 1;; --f) {
            f0[(size_t)it.first_frame + f] = v ? (double)(m + 1) : 0.0;
            if (f == 0) break;
            const int b = tb[((size_t)f * 2 + v) * M + m];
            v = b >> 7;
            m = clamped(m + (b & 127) - reach, M - 1);
        }
    }
    __syncthreads();
    for (int f = t; f < it.frames; f += T) {
        const size_t g = (size_t)it.first_frame + f;
        const double state = f0[g];
        if (state == 0.0) continue;
        const int m = (int)state - 1;
        const int cnt = clamped(cand_count[g], N);
        double out = centre[m], top = 0.0;
        bool any = false;
        for (int c = 0; c < cnt; ++c) {
            const double fc = cand_f0[g * N + c];
            if (bin_of(edge_s, M, fc) != m) continue;
            const double p = cand_prob[g * N + c];
            if (!any || p > top) {
                any = true;
                top = p;
                out = fc;
            }
        }
        f0[g] = out;
    }
}

// The refusals that the entry points share, in f5_pitch_track's order: the input pointers, the frame grid and the lag range, the items.
int check_inputs(const char* who, const void* base, const void* start_host, const void* len_host, const void* frames_host) {
    if (!base) return fail(F5_EINVAL, "%s: null base", who);
    if (!start_host) return fail(F5_EINVAL, "%s: null start_host", who);
    if (!len_host) return fail(F5_EINVAL, "%s: null len_host", who);
    if (!frames_host) return fail(F5_EINVAL, "%s: null frames_host", who);
    return F5_OK;
}

int check_grid(const char* who, int P, int sample_rate, int hop, int first_centre, int window, int tau_min, int tau_max) {
    if (P < 1 || P > kMaxItems) return fail(F5_EINVAL, "%s: need 1 <= P <= %d items (P = %d)", who, kMaxItems, P);
    if (sample_rate < 1 || sample_rate > kMaxRate) return fail(F5_EINVAL, "%s: sample_rate = %d (need 1 <= sample_rate <= %d)", who, sample_rate, kMaxRate);
    if (hop < 1 || hop > kMaxHop) return fail(F5_EINVAL, "%s: hop = %d (need 1 <= hop <= %d)", who, hop, kMaxHop);
    if (first_centre < 0 || first_centre > kMaxCentre)
        return fail(F5_EINVAL, "%s: first_centre = %d (need 0 <= first_centre <= %d)", who, first_centre, kMaxCentre);
    if (window < kMinWindow || window > kMaxWindow)
        return fail(F5_EINVAL, "%s: window = %d (need %d <= window <= %d)", who, window, kMinWindow, kMaxWindow);
    if (tau_min < kMinTau || tau_min >= tau_max || tau_max > kMaxTau)
        return fail(F5_EINVAL, "%s: tau_min = %d, tau_max = %d (need %d <= tau_min < tau_max <= %d)", who, tau_min, tau_max, kMinTau, kMaxTau);
    return F5_OK;
}

// start_host and len_host may be null (f5_pitch_decode has frame counts alone)
int check_items(const char* who, int P, const int64_t* start_host, const int32_t* len_host, const int32_t* frames_host, long long* total_out) {
    long long total = 0;
    for (int p = 0; p < P; ++p) {
        if (start_host && start_host[p] < 0) return fail(F5_EINVAL, "%s: item %d has start = %lld < 0", who, p, (long long)start_host[p]);
        if (len_host && len_host[p] < 1) return fail(F5_EINVAL, "%s: item %d has len = %d (need len >= 1)", who, p, len_host[p]);
        if (frames_host[p] < 1) return fail(F5_EINVAL, "%s: item %d has frames = %d (need frames >= 1)", who, p, frames_host[p]);
        total += frames_host[p];
        if (total > kMaxTrackFrames)
            return fail(F5_EINVAL, "%s: more than %lld frames in one call at item %d (split the batch)", who, kMaxTrackFrames, p);
    }
    *total_out = total;
    return F5_OK;
}

void fill_items(Item* h, int P, const int64_t* start_host, const int32_t* len_host, const int32_t* frames_host) {
    int first = 0;
    for (int p = 0; p < P; ++p) {
        h[p] = Item{start_host[p], len_host[p], frames_host[p], first, 0};
        first += frames_host[p];
    }
}

// a table of n doubles, all finite (and none negative where `sign`)
int check_table(const char* who, const char* name, const double* v, long long n, bool sign) {
    if (!v) return fail(F5_EINVAL, "%s: null %s", who, name);
    for (long long i = 0; i < n; ++i) {
        if (!std::isfinite(v[i])) return fail(F5_EINVAL, "%s: %s[%lld] is not finite", who, name, i);
        if (sign && v[i] < 0.0) return fail(F5_EINVAL, "%s: %s[%lld] = %g is negative", who, name, i, v[i]);
    }
    return F5_OK;
}
}  // namespace

extern "C" int f5_pitch_track(const float* base, int32_t P, const int64_t* start_host, const int32_t* len_host, int32_t sample_rate,
                              int32_t hop, int32_t first_centre, const int32_t* frames_host, int32_t window, int32_t tau_min,
                              int32_t tau_max, double threshold, double* f0, double* ap, f5_stream stream) {
    const char* who = "f5_pitch_track";
    CHK(check_inputs(who, base, start_host, len_host, frames_host));
    if (!f0) return fail(F5_EINVAL, "%s: null f0", who);
    if (!ap) return fail(F5_EINVAL, "%s: null ap", who);
    CHK(check_grid(who, P, sample_rate, hop, first_centre, window, tau_min, tau_max));
    if (!(threshold > 0.0) || !(threshold <= 1.0)) return fail(F5_EINVAL, "%s: threshold = %g (need 0 < threshold <= 1)", who, threshold);
    long long total = 0;
    CHK(check_items(who, P, start_host, len_host, frames_host, &total));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    const size_t tab_bytes = (size_t)P * sizeof(Item);
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) { fill_items(reinterpret_cast<Item*>(host), P, start_host, len_host, frames_host); }));
    pitch_track_kernel<<<dim3((unsigned)total), kPitchThreads, 0, s>>>(base, reinterpret_cast<const Item*>(tab), P, (double)sample_rate,
                                                                       hop, first_centre, window, tau_min, tau_max, threshold, f0, ap);
    KCHK();
    return st->leave(s);
}

extern "C" int f5_pitch_candidates(const float* base, int32_t P, const int64_t* start_host, const int32_t* len_host, int32_t sample_rate,
                                   int32_t hop, int32_t first_centre, const int32_t* frames_host, int32_t window, int32_t tau_min,
                                   int32_t tau_max, int32_t N, const double* w_host, double p_absent, int32_t* cand_count,
                                   int32_t* cand_lag, double* cand_f0, double* cand_prob, f5_stream stream) {
    const char* who = "f5_pitch_candidates";
    CHK(check_inputs(who, base, start_host, len_host, frames_host));
    if (!cand_count) return fail(F5_EINVAL, "%s: null cand_count", who);
    if (!cand_lag) return fail(F5_EINVAL, "%s: null cand_lag", who);
    if (!cand_f0) return fail(F5_EINVAL, "%s: null cand_f0", who);
    if (!cand_prob) return fail(F5_EINVAL, "%s: null cand_prob", who);
    CHK(check_grid(who, P, sample_rate, hop, first_centre, window, tau_min, tau_max));
    if (N < 1 || N > kMaxThresholds) return fail(F5_EINVAL, "%s: N = %d thresholds (need 1 <= N <= %d)", who, N, kMaxThresholds);
    CHK(check_table(who, "w_host", w_host, N, true));
    if (!(p_absent >= 0.0) || !(p_absent <= 1.0)) return fail(F5_EINVAL, "%s: p_absent = %g (need 0 <= p_absent <= 1)", who, p_absent);
    long long total = 0;
    CHK(check_items(who, P, start_host, len_host, frames_host, &total));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    const size_t w_bytes = (size_t)N * sizeof(double), tab_bytes = w_bytes + (size_t)P * sizeof(Item);   // the weights, then the items
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        std::copy(w_host, w_host + N, reinterpret_cast<double*>(host));
        fill_items(reinterpret_cast<Item*>(host + w_bytes), P, start_host, len_host, frames_host);
    }));
    pitch_candidates_kernel<<<dim3((unsigned)total), kPitchThreads, 0, s>>>(
        base, reinterpret_cast<const Item*>(tab + w_bytes), P, (double)sample_rate, hop, first_centre, window, tau_min, tau_max, N,
        reinterpret_cast<const double*>(tab), p_absent, cand_count, cand_lag, cand_f0, cand_prob);
    KCHK();
    return st->leave(s);
}

extern "C" int64_t f5_pitch_decode_bytes(int64_t frames_total, int32_t M) {
    return frames_total < 0 || M < 0 ? 0 : 2 * (int64_t)M * frames_total;
}

extern "C" int f5_pitch_decode(const int32_t* cand_count, const double* cand_f0, const double* cand_prob, int32_t N, int32_t P,
                               const int32_t* frames_host, int32_t M, const double* edge_host, const double* centre_host, int32_t reach,
                               const double* trans_host, double p_switch, void* workspace, int64_t workspace_bytes, double* f0,
                               double* voiced_prob, f5_stream stream) {
    const char* who = "f5_pitch_decode";
    if (!cand_count) return fail(F5_EINVAL, "%s: null cand_count", who);
    if (!cand_f0) return fail(F5_EINVAL, "%s: null cand_f0", who);
    if (!cand_prob) return fail(F5_EINVAL, "%s: null cand_prob", who);
    if (!frames_host) return fail(F5_EINVAL, "%s: null frames_host", who);
    if (!workspace) return fail(F5_EINVAL, "%s: null workspace", who);
    if (!f0) return fail(F5_EINVAL, "%s: null f0", who);
    if (!voiced_prob) return fail(F5_EINVAL, "%s: null voiced_prob", who);
    if (N < 1 || N > kMaxThresholds) return fail(F5_EINVAL, "%s: N = %d candidate slots per frame (need 1 <= N <= %d)", who, N, kMaxThresholds);
    if (P < 1 || P > kMaxItems) return fail(F5_EINVAL, "%s: need 1 <= P <= %d items (P = %d)", who, kMaxItems, P);
    if (M < kMinBins || M > kMaxBins) return fail(F5_EINVAL, "%s: M = %d bins (need %d <= M <= %d)", who, M, kMinBins, kMaxBins);
    if (reach < 1 || reach > kMaxReach) return fail(F5_EINVAL, "%s: reach = %d (need 1 <= reach <= %d)", who, reach, kMaxReach);
    if (!(p_switch > 0.0) || !(p_switch < 1.0)) return fail(F5_EINVAL, "%s: p_switch = %g (need 0 < p_switch < 1)", who, p_switch);
    const int band = 2 * reach + 1;
    CHK(check_table(who, "edge_host", edge_host, M + 1, false));
    for (int m = 0; m < M; ++m)
        if (!(edge_host[m] < edge_host[m + 1]))
            return fail(F5_EINVAL, "%s: edge_host is not strictly ascending at %d (%g, %g)", who, m, edge_host[m], edge_host[m + 1]);
    CHK(check_table(who, "centre_host", centre_host, M, false));
    CHK(check_table(who, "trans_host", trans_host, (long long)M * band, true));
    long long total = 0;
    CHK(check_items(who, P, nullptr, nullptr, frames_host, &total));
    const int64_t need = f5_pitch_decode_bytes(total, M);
    if (workspace_bytes < need)
        return fail(F5_EINVAL, "%s: workspace_bytes = %lld (need %lld for %lld frames of %d bins)", who, (long long)workspace_bytes,
                    (long long)need, total, M);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(call_state_mutex());
    CallState* st = nullptr;
    CHK(call_state_of_current_device(&st));
    char* tab = nullptr;
    // the tables of doubles first (edge, centre, trans), then the items
    const size_t n_edge = (size_t)M + 1, n_centre = (size_t)M, n_trans = (size_t)M * band;
    const size_t f64_bytes = (n_edge + n_centre + n_trans) * sizeof(double), tab_bytes = f64_bytes + (size_t)P * sizeof(Span);
    CHK(st->reserve_tables(tab_bytes, &tab));
    CHK(st->enter(s));
    CHK(st->stage.upload(tab, tab_bytes, s, [&](char* host) {
        double* h = reinterpret_cast<double*>(host);
        std::copy(edge_host, edge_host + n_edge, h);
        std::copy(centre_host, centre_host + n_centre, h + n_edge);
        std::copy(trans_host, trans_host + n_trans, h + n_edge + n_centre);
        Span* sp = reinterpret_cast<Span*>(host + f64_bytes);
        int first = 0;
        for (int p = 0; p < P; ++p) {
            sp[p] = Span{frames_host[p], first};
            first += frames_host[p];
        }
    }));
    const double* dev = reinterpret_cast<const double*>(tab);
    pitch_decode_kernel<<<dim3((unsigned)P), round_up(M, 64), 0, s>>>(reinterpret_cast<const Span*>(tab + f64_bytes), cand_count, cand_f0,
                                                                     cand_prob, N, M, dev, dev + n_edge, reach, dev + n_edge + n_centre,
                                                                     1.0 - p_switch, p_switch, static_cast<unsigned char*>(workspace), f0,
                                                                     voiced_prob);
    KCHK();
    return st->leave(s);
}
