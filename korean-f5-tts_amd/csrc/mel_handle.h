// The handle of the prompt stages (f5_mel): the mel front-end (mel.hip), the preparation in front of it (prompt.hip) and the
// delivery of generated audio at a client's rate (deliver.hip, which resamples with the same banks) share its workspace and
// staging ring; each call carves the arena anew, and calls on one handle are ordered by the caller's stream.
#pragma once
#include <map>
#include <utility>
#include <vector>

#include "internal.h"

struct f5_mel {
    int n_fft = 0, hop = 0, n_mels = 0, F = 0, ns = 0, kf = 0;
    float *basis = nullptr, *fb = nullptr;
    Arena arena;
    Staging stage;                    // pinned slots for the ragged calls' per-item tables
    std::vector<int32_t> plan_rows;   // ragged call: row_start[B + 1] | frames[B] (host; grows, never shrinks)
    // prepare stage: the resample banks, f32 [K, new] per (orig, new), uploaded once each and freed with the handle
    DevPool banks;
    std::map<std::pair<int, int>, const float*> bank_of;
    std::vector<int64_t> plan_out;    // prepare call: len[B] | start[B] (host; grows, never shrinks)
    ~f5_mel() {
        if (basis) (void)hipFree(basis);
        if (fb) (void)hipFree(fb);
    }
};
