// Stand-alone check of the host side of csrc/silence.hip under the sanitizers: f5_silence_plan at its limits, and
// f5_silence_analyse / f5_wave_gather with bad and boundary arguments only, so that every such call ends in the validation and
// nothing is staged or launched (no GPU is needed).  The boundary calls are full-size (65,535 items, 8 queries, long segment
// tables) and fail on the very last item or segment, after every table in front of it has been read.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined korean-f5-tts_amd/csrc/silence.hip tools/silence_host_check.cpp -o silence_host_check
//   ./silence_host_check
//
// It brings its own f5_fail / f5_last_error (the library's live in engine.hip, which this program does not link).
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

static void expect(bool ok, const char* what, int rc) {
    printf("%-4s %s: rc %d, \"%s\"\n", ok ? "ok" : "BAD", what, rc, g_msg);
    if (!ok) ++g_bad;
    g_msg[0] = 0;
}

int main() {
    float* dev = reinterpret_cast<float*>(0x1000);   // never dereferenced: validation reads host arrays only
    const int B = 65535, nq = 8;
    std::vector<int32_t> len((size_t)B, 1 << 24), queries;
    for (int k = 0; k < nq; ++k) {
        const int32_t q[4] = {k % 2 ? 1 : 1 << 24, k < 4 ? 1 : 7, 32767, k % 2};
        queries.insert(queries.end(), q, q + 4);
    }
    {   // the plan at every limit at once: 65,535 items of 2^24 ms, 8 queries
        std::vector<int32_t> count((size_t)B * nq);
        std::vector<int64_t> start((size_t)B * nq);
        int64_t total = -1;
        int rc = f5_silence_plan(B, len.data(), nq, queries.data(), count.data(), start.data(), &total);
        int64_t per_item = 0;
        for (int k = 0; k < nq; ++k) per_item += count[k];
        expect(rc == F5_OK && total == per_item * B && start.back() + count.back() == total, "f5_silence_plan, every limit", rc);
        len[B - 1] = (1 << 24) + 1;
        rc = f5_silence_plan(B, len.data(), nq, queries.data(), count.data(), start.data(), &total);
        expect(rc == F5_EINVAL && strstr(g_msg, "item 65534"), "f5_silence_plan, the last item too long", rc);
        len[B - 1] = 1 << 24;
    }
    {   // analyse: short items, a table per item, the last item's last segment out of order
        std::vector<int32_t> small((size_t)B, 40), ch((size_t)B, 2), fr((size_t)B, 1000), rate((size_t)B, 24000), segc((size_t)B, 3), segs;
        std::vector<int64_t> start((size_t)B);
        for (int b = 0; b < B; ++b) {
            start[b] = 2000LL * b;
            const int32_t s[9] = {0, 10, 100, 100, 990, 100, 250, 0, 400};
            segs.insert(segs.end(), s, s + 9);
        }
        uint8_t* flags = reinterpret_cast<uint8_t*>(dev);
        segs[segs.size() - 3] = 199;
        int rc = f5_silence_analyse(dev, B, start.data(), ch.data(), fr.data(), rate.data(), small.data(), 32768.0f, nq, queries.data(),
                                    segc.data(), segs.data(), flags, INT64_MAX, nullptr);
        expect(rc == F5_EINVAL && strstr(g_msg, "item 65534 segment 2"), "f5_silence_analyse, the last segment out of order", rc);
        segs[segs.size() - 3] = 250;
        rate[B - 1] = 11024;
        rc = f5_silence_analyse(dev, B, start.data(), ch.data(), fr.data(), rate.data(), small.data(), 32768.0f, nq, queries.data(),
                                segc.data(), segs.data(), flags, INT64_MAX, nullptr);
        expect(rc == F5_EINVAL && strstr(g_msg, "rate = 11024"), "f5_silence_analyse, the last rate too low", rc);
        rate[B - 1] = 24000;
        rc = f5_silence_analyse(dev, B, start.data(), ch.data(), fr.data(), rate.data(), len.data(), 32768.0f, nq, queries.data(), nullptr,
                                nullptr, flags, INT64_MAX, nullptr);
        expect(rc == F5_EINVAL && strstr(g_msg, "2^30"), "f5_silence_analyse, more than 2^30 milliseconds", rc);
        rc = f5_silence_analyse(dev, B, start.data(), ch.data(), fr.data(), rate.data(), small.data(), 32768.0f, nq, queries.data(), nullptr,
                                nullptr, flags, 7, nullptr);
        expect(rc == F5_EINVAL && strstr(g_msg, "flags_capacity"), "f5_silence_analyse, a flag buffer too small", rc);
        // gather: the same tables; the last item's last segment ends one frame past F_out
        std::vector<int32_t> outf((size_t)B, 650);
        std::vector<int64_t> outs((size_t)B);
        for (int b = 0; b < B; ++b) outs[b] = 1300LL * b;
        outf[B - 1] = 649;
        rc = f5_wave_gather(dev, B, start.data(), ch.data(), fr.data(), 32767.0f, segc.data(), segs.data(), outf.data(), outs.data(), dev,
                            1300LL * B, nullptr);
        expect(rc == F5_EINVAL && strstr(g_msg, "item 65534 segment 2"), "f5_wave_gather, the last segment past F_out", rc);
        outf[B - 1] = 650;
        rc = f5_wave_gather(dev, B, start.data(), ch.data(), fr.data(), 32767.0f, segc.data(), segs.data(), outf.data(), outs.data(), dev,
                            1300LL * B - 1, nullptr);
        expect(rc == F5_EINVAL && strstr(g_msg, "out_capacity"), "f5_wave_gather, the last item past out_capacity", rc);
    }
    printf(g_bad ? "%d BAD\n" : "all ok\n", g_bad);
    return g_bad ? 1 : 0;
}
