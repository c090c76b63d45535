// Stand-alone check of the host side of csrc/edit.hip under the sanitizers: f5_edit_assemble and f5_wave_splice with bad and
// boundary arguments only, so that every call ends in the validation and nothing is staged or launched (no GPU is needed).
// The boundary calls fill the segment tables to their last entry (64 items of 33 segments) and fail on the very last segment.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined korean-f5-tts_amd/csrc/edit.hip tools/edit_host_check.cpp -o edit_host_check
//   ./edit_host_check
//
// It brings its own f5_fail / f5_last_error (the library's live in engine.hip, which this program does not link).
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/f5_hip.h"

static char g_msg[512];

int f5_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char* f5_last_error(void) { return g_msg; }

static int g_bad = 0;

static void expect(int rc, const char* fn, const char* what) {
    const bool ok = rc == F5_EINVAL && strncmp(g_msg, fn, strlen(fn)) == 0;
    printf("%-4s %s, %s: rc %d, \"%s\"\n", ok ? "ok" : "BAD", fn, what, rc, g_msg);
    if (!ok) ++g_bad;
    g_msg[0] = 0;
}

int main() {
    float* dev = reinterpret_cast<float*>(0x1000);   // never dereferenced: validation reads host arrays only
    {
        const char* fn = "f5_edit_assemble";
        int32_t frames[1] = {8}, counts[1] = {2}, segs[6] = {0, 0, 3, 3, -1, 2}, dur[1] = {5};
        auto call = [&](const float* mel, int B, int64_t stride, int row, const int32_t* f, const int32_t* c, const int32_t* s,
                        const int32_t* d, float* cond, int D_max) {
            return f5_edit_assemble(mel, B, stride, row, f, c, s, d, cond, D_max, nullptr);
        };
        expect(call(nullptr, 1, 800, 100, frames, counts, segs, dur, dev, 5), fn, "mel null");
        expect(call(dev, 1, 800, 100, nullptr, counts, segs, dur, dev, 5), fn, "frames_host null");
        expect(call(dev, 1, 800, 100, frames, nullptr, segs, dur, dev, 5), fn, "seg_count_host null");
        expect(call(dev, 1, 800, 100, frames, counts, nullptr, dur, dev, 5), fn, "segs_host null");
        expect(call(dev, 1, 800, 100, frames, counts, segs, nullptr, dev, 5), fn, "dur_host null");
        expect(call(dev, 1, 800, 100, frames, counts, segs, dur, nullptr, 5), fn, "cond null");
        expect(call(dev, 0, 800, 100, frames, counts, segs, dur, dev, 5), fn, "B = 0");
        expect(call(dev, 65, 800, 100, frames, counts, segs, dur, dev, 5), fn, "B = 65");
        expect(call(dev, INT_MIN, 800, 100, frames, counts, segs, dur, dev, 5), fn, "B = INT_MIN");
        expect(call(dev, 1, 800, 100, frames, counts, segs, dur, dev, 4), fn, "D_b above D_max");
        expect(call(dev, 1, 799, 100, frames, counts, segs, dur, dev, 5), fn, "stride below T rows");
        int32_t far_src[6] = {0, 6, 3, 3, -1, 2}, far_dst[6] = {0, 0, 3, 3, -1, 3}, huge[6] = {0, 0, 3, INT_MAX, -1, INT_MAX};
        int32_t neg[6] = {INT_MIN, 0, 3, 3, -1, 2}, big_src[6] = {0, INT_MAX, 3, 3, -1, 2}, many[1] = {34};
        expect(call(dev, 1, 800, 100, frames, counts, far_src, dur, dev, 5), fn, "source [6, 9) of 8");
        expect(call(dev, 1, 800, 100, frames, counts, far_dst, dur, dev, 5), fn, "destination [3, 6) of 5");
        expect(call(dev, 1, 800, 100, frames, counts, huge, dur, dev, 5), fn, "destination past 2^31");
        expect(call(dev, 1, 800, 100, frames, counts, neg, dur, dev, 5), fn, "dst = INT_MIN");
        expect(call(dev, 1, 800, 100, frames, counts, big_src, dur, dev, 5), fn, "src = INT_MAX");
        expect(call(dev, 1, 800, 100, frames, many, segs, dur, dev, 5), fn, "34 segments");
        // the full table: 64 items of 33 one-frame segments, the last one reading one frame past its item
        const int B = 64, S = 33;
        std::vector<int32_t> fr(B, S), cn(B, S), du(B, S), sg;
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < S; ++s) {
                sg.push_back(s);
                sg.push_back(s % 2 ? -1 : s);
                sg.push_back(1);
            }
        sg[3 * (B * S - 1) + 1] = S;
        expect(call(dev, B, S * 100, 100, fr.data(), cn.data(), sg.data(), du.data(), dev, S), fn, "64 x 33 segments, the last one out of range");
    }
    {
        const char* fn = "f5_wave_splice";
        int32_t lens[1] = {1024}, a_len[1] = {2048}, counts[1] = {1}, segs[3] = {0, 0, 2};
        int64_t a_start[1] = {0};
        auto call = [&](const float* gen, int B, int64_t gs, const int32_t* l, const float* a, const int64_t* as, const int32_t* al,
                        const int32_t* c, const int32_t* s, int hop, int cf, float* out, int64_t os) {
            return f5_wave_splice(gen, B, gs, l, a, as, al, c, s, hop, cf, out, os, nullptr);
        };
        expect(call(nullptr, 1, 1024, lens, dev, a_start, a_len, counts, segs, 256, 240, dev, 1024), fn, "gen null");
        expect(call(dev, 1, 1024, nullptr, dev, a_start, a_len, counts, segs, 256, 240, dev, 1024), fn, "len_host null");
        expect(call(dev, 1, 1024, lens, nullptr, a_start, a_len, counts, segs, 256, 240, dev, 1024), fn, "a_base null");
        expect(call(dev, 1, 1024, lens, dev, nullptr, a_len, counts, segs, 256, 240, dev, 1024), fn, "a_start_host null");
        expect(call(dev, 1, 1024, lens, dev, a_start, nullptr, counts, segs, 256, 240, dev, 1024), fn, "a_len_host null");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, nullptr, segs, 256, 240, dev, 1024), fn, "seg_count_host null");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, nullptr, 256, 240, dev, 1024), fn, "segs_host null");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, segs, 256, 240, nullptr, 1024), fn, "out null");
        expect(call(dev, 0, 1024, lens, dev, a_start, a_len, counts, segs, 256, 240, dev, 1024), fn, "B = 0");
        expect(call(dev, 65, 1024, lens, dev, a_start, a_len, counts, segs, 256, 240, dev, 1024), fn, "B = 65");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, segs, 0, 240, dev, 1024), fn, "hop = 0");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, segs, INT_MAX, 240, dev, 1024), fn, "hop = INT_MAX");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, segs, 256, -1, dev, 1024), fn, "cross_fade_samples = -1");
        expect(call(dev, 1, 1023, lens, dev, a_start, a_len, counts, segs, 256, 240, dev, 1024), fn, "L above gen_stride");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, segs, 256, 240, dev, 1023), fn, "L above out_stride");
        int32_t edit[3] = {0, -1, 2}, neg[3] = {-1, 0, 2}, empty[3] = {0, 0, 0}, huge[3] = {INT_MAX, INT_MAX, INT_MAX};
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, edit, 256, 240, dev, 1024), fn, "an EDIT segment");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, neg, 256, 240, dev, 1024), fn, "dst = -1");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, empty, 256, 240, dev, 1024), fn, "an empty segment");
        expect(call(dev, 1, 1024, lens, dev, a_start, a_len, counts, huge, 65536, INT_MAX, dev, 1024), fn, "a segment past 2^31 frames");
        const int B = 64, S = 33;
        std::vector<int32_t> ln(B, INT_MAX), al(B, INT_MAX), cn(B, S), sg;
        std::vector<int64_t> as(B, INT64_MAX);
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < S; ++s) {
                sg.push_back(INT_MAX / 2 - S + s);      // the largest frame numbers the checks let through, at the largest hop
                sg.push_back(INT_MAX - 1);
                sg.push_back(1);
            }
        sg[3 * (B * S - 1) + 1] = -1;
        expect(call(dev, B, INT64_MAX, ln.data(), dev, as.data(), al.data(), cn.data(), sg.data(), 65536, INT_MAX, dev, INT64_MAX), fn,
               "64 x 33 segments at the largest values, the last one out of range");
    }
    printf("%s\n", g_bad ? "FAILED" : "all calls were rejected in validation");
    return g_bad ? 1 : 0;
}
