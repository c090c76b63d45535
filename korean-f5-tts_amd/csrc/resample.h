// The polyphase windowed-sinc resampler of the audio stages, once: the rate geometry as infer.sinc_resample computes it, the block
// shape, and the tap loop of step 4 of the f5_mel_prepare_ragged contract (include/f5_hip.h) with the sample source as a
// parameter.  prompt.hip resamples levelled prompts up or down to the model's rate with it, deliver.hip the generated stream to
// the client's rate; both stage a block's window in LDS and read the banks transposed, [K, new].
#pragma once
#include <cmath>
#include <numeric>

#include "internal.h"

namespace f5 {
constexpr int RS_OUT_TILE = 1024;      // output samples a block aims at: 256 threads x 4
constexpr int RS_LDS_FLOATS = 8192;    // the staged window of a block, (F - 1) * orig + K samples, fits this
constexpr long long RS_MAX_BANK = 1LL << 20;

struct RatePair {
    int orig = 1, nw = 1, width = 0, K = 1;   // orig == nw (== 1): the signal is at the target rate already
    bool same() const { return orig == nw; }
};
// orig, new and width exactly as infer.sinc_resample computes them (python evaluates the width in double); false: the bank
// new * (2 width + orig) has more than 2^20 elements
inline bool rate_pair(int sr, int target, RatePair* r) {
    const int g = std::gcd(sr, target);
    const int orig = sr / g, nw = target / g;
    if (orig == nw) {
        *r = RatePair();
        return true;
    }
    const double base_freq = (double)std::min(orig, nw) * 0.99;
    const double width = std::ceil((double)(6LL * orig) / base_freq);
    if (width > (double)RS_MAX_BANK) return false;
    const long long K = 2 * (long long)width + orig;
    if (K > RS_MAX_BANK || K * nw > RS_MAX_BANK) return false;
    r->orig = orig; r->nw = nw; r->width = (int)width; r->K = (int)K;
    return true;
}
// frames a block takes when its window is staged (K <= RS_LDS_FLOATS): about RS_OUT_TILE outputs, and a window that fits
inline int frames_per_block(const RatePair& r) {
    return std::min(std::max(1, RS_OUT_TILE / r.nw), (RS_LDS_FLOATS - r.K) / r.orig + 1);
}

// Four output samples of one block: sample q is phase bp[q] of the frame whose window starts xi[q] samples into the block's
// window.  acc[q] = sum_k bank[k][bp[q]] * src(xi[q] + k), k ascending from +0.0, an f32 multiply then an f32 add per tap (the
// library is built with -ffp-contract=off).
template <typename Src>
__device__ __forceinline__ void resample_taps(const float* __restrict__ bank, int nw, int K, const int (&xi)[4], const int (&bp)[4], Src src,
                                              float (&acc)[4]) {
    for (int q = 0; q < 4; ++q) acc[q] = 0.f;
    for (int k = 0; k < K; ++k) {
        const float* row = bank + (size_t)k * nw;
        for (int q = 0; q < 4; ++q) acc[q] = acc[q] + row[bp[q]] * src(xi[q] + k);
    }
}
}  // namespace f5
