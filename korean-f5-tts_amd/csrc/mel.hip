// Prompt mel front-end: wav -> log-mel, the reference's MelSpec with mel_spec_type="vocos"
// (model/modules.py:78-146: torchaudio MelSpectrogram(n_fft=1024, win=1024, hop=256, n_mels=100, power=1, center=True,
// norm=None) -> clamp(min=1e-5).log()).
//   STFT  = reflect pad + framing as a STRIDED VIEW (row t = wav_pad[t*hop .. t*hop + n_fft), lda = hop: no im2col) x
//           windowed DFT basis [2F(+pad), n_fft] on the exact-f32 MFMA GEMM
//   |S|   = sqrt(re^2 + im^2)                               (elementwise)
//   mel   = |S| [T, F(+pad)] x filterbank [n_mels, F(+pad)]^T with a log(max(., 1e-5)) epilogue
// Output is [B, T, n_mels] -- the layout CFM.sample wants after its permute(0, 2, 1) (cfm.py:106-108).
// mel_spec_type="bigvgan" (modules.py:33-75, get_bigvgan_mel_spectrogram) is the same pipeline with reflect padding
// (n_fft - hop) / 2 and center=False (T = (nw + 2 pad - n_fft) / hop + 1), |S| = sqrt(re^2 + im^2 + 1e-9) and librosa's
// slaney filterbank as the loaded table: f5_mel_forward_ex(pad, eps).
#include <string>
#include <vector>

#include "elementwise.h"
#include "gemm_dispatch.h"
#include "internal.h"
#include "mel_handle.h"

using namespace f5;
#define fail f5_fail

// sample of a signal of nw samples that element j of its reflect-padded form reads, -pad <= j < nw + pad with pad < nw
static __device__ __forceinline__ int reflect_index(int j, int nw) {
    if (j < 0) j = -j;                   // reflect (no edge repeat), torch pad_mode="reflect"
    if (j >= nw) j = 2 * (nw - 1) - j;
    return j;
}
// out rows have stride `ls` >= nw + 2*pad (a multiple of 4 floats so that every row stays 16-byte aligned)
static __global__ void reflect_pad_kernel(const float* __restrict__ wav, float* __restrict__ out, int B, int nw, int pad, int ls) {
    const long total = (long)B * ls;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / ls);
        const int j = (int)(i % ls) - pad;
        float v = 0.f;
        if (j < nw + pad) v = wav[(size_t)b * nw + reflect_index(j, nw)];
        out[i] = v;
    }
}
// The packed signal of a ragged batch (f5_mel_ragged_plan): item b's reflect-padded samples start at element row_start[b] * hop
// and own the rows up to row_start[b + 1]; the slack behind its nw_b + 2 pad samples and the n_fft elements behind the last
// row are zeros, so that the frames that run out of an item (dead rows) are finite.  One block per packed row, striding: the
// row -> item search is block-uniform.  Every one of the R * hop + n_fft elements is written, nothing outside
// wav[wav_start[b] .. wav_start[b] + nw[b]) is read.
static __global__ __launch_bounds__(256) void reflect_pad_ragged_kernel(const float* __restrict__ wav, float* __restrict__ out,
                                                                        const long long* __restrict__ wav_start,
                                                                        const int* __restrict__ row_start, const int* __restrict__ nw,
                                                                        int B, int R, int hop, int pad, int n_fft) {
    const int rows = R + (n_fft + hop - 1) / hop;   // the tail behind row R - 1 as rows of its own
    const size_t total = (size_t)R * hop + n_fft;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = nullptr;
        int n = 0, first = 0;
        if (r < R) {
            const int b = segment_of_row(row_start, B, r);
            src = wav + wav_start[b];
            n = nw[b];
            first = (r - row_start[b]) * hop;   // < nw_b + 2 pad + hop: an int
        }
        for (int e = threadIdx.x; e < hop; e += blockDim.x) {
            const size_t i = (size_t)r * hop + e;
            if (i >= total) break;
            const int j = first + e - pad;
            float v = 0.f;
            if (src && j < n + pad) v = src[reflect_index(j, n)];
            out[i] = v;
        }
    }
}
// packed [R, C] -> out[b * stride_b + t * C + c] = t < frames[b] ? packed[row_start[b] + t, c] : +0.0 for t < T_out; one
// thread per 4 channels (C % 4 == 0), 16-byte accesses when out and stride_b allow them (VEC), one writer per element
template <bool VEC>
static __global__ __launch_bounds__(256) void mel_unpack_ragged_kernel(const float* __restrict__ packed, float* __restrict__ out,
                                                                       const int* __restrict__ row_start,
                                                                       const int* __restrict__ frames, int B, int T_out, int C,
                                                                       long stride_b) {
    const int c4 = C / 4;
    const long per_b = (long)T_out * c4, total = per_b * B;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / per_b);
        const long k = i % per_b;
        const int t = (int)(k / c4), q = (int)(k % c4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < frames[b]) v = reinterpret_cast<const float4*>(packed + ((size_t)row_start[b] + t) * C)[q];
        float* dst = out + (size_t)b * stride_b + (size_t)t * C + 4 * q;
        if (VEC) {
            *reinterpret_cast<float4*>(dst) = v;
        } else {
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
    }
}
// spec [T, lds] with re in [0, F), im in [F, 2F)  ->  mag [T, ldm], columns >= F zeroed
static __global__ void magnitude_kernel(const float* __restrict__ spec, int lds, float* __restrict__ mag, int ldm, long T, int F,
                                        float eps) {
    const long total = T * ldm;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldm);
        const long t = i / ldm;
        float v = 0.f;
        if (c < F) {
            const float re = spec[t * lds + c], im = spec[t * lds + F + c];
            v = sqrtf(re * re + im * im + eps);
        }
        mag[i] = v;
    }
}

extern "C" int f5_mel_create(int32_t n_fft, int32_t hop, int32_t n_mels, f5_mel** out) {
    if (!out || n_fft <= 0 || hop <= 0 || n_mels <= 0 || (n_fft % 32) || (hop % 4) || (n_mels % 4))
        return fail(F5_EINVAL, "f5_mel_create: need n_fft %% 32 == 0, hop %% 4 == 0, n_mels %% 4 == 0");
    f5_mel* m = new f5_mel();
    m->n_fft = n_fft; m->hop = hop; m->n_mels = n_mels;
    m->F = n_fft / 2 + 1;
    m->ns = round_up(2 * m->F, 4);     // spectrum row: [re | im | pad]
    m->kf = round_up(m->F, 32);        // magnitude row padded to whole f32 K-tiles
    *out = m;
    return F5_OK;
}
extern "C" int f5_mel_destroy(f5_mel* m) {
    if (m) {
        (void)hipDeviceSynchronize();
        delete m;
    }
    return F5_OK;
}
// name = "aux.dft_basis" f32[ns, n_fft] (rows: w*cos for f < F, then w*sin, zero pad) or "aux.mel_fb" f32[n_mels, kf]
extern "C" int f5_mel_load(f5_mel* m, const char* name, const void* dev, const int64_t* shape, int32_t ndim, f5_stream stream) {
    if (!m || !name || !dev || ndim != 2) return fail(F5_EINVAL, "f5_mel_load: bad arguments");
    const std::string n(name);
    float** dst = nullptr;
    if (n == "aux.dft_basis") {
        if (shape[0] != m->ns || shape[1] != m->n_fft) return fail(F5_EINVAL, "aux.dft_basis must be [%d, %d]", m->ns, m->n_fft);
        dst = &m->basis;
    } else if (n == "aux.mel_fb") {
        if (shape[0] != m->n_mels || shape[1] != m->kf) return fail(F5_EINVAL, "aux.mel_fb must be [%d, %d]", m->n_mels, m->kf);
        dst = &m->fb;
    } else {
        return fail(F5_EINVAL, "f5_mel_load: unknown tensor '%s'", name);
    }
    const size_t bytes = (size_t)shape[0] * shape[1] * 4;
    if (*dst) (void)hipFree(*dst);
    HIPCHK(hipMalloc((void**)dst, bytes));
    HIPCHK(hipMemcpyAsync(*dst, dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return F5_OK;
}
namespace {
// Workspace of one pass over R rows (frames): the rectangular call carves it for one item's T frames and reuses it item by
// item, the ragged one for the packed rows of the whole batch, with the packed mel and the per-item tables behind it
struct MelWork {
    float *wp, *spec, *mag, *pk;
    char* tab;
};
// The ragged call's per-item tables, wav_start[B] (int64) | row_start[B + 1] | nw[B] | frames[B]: one layout for the pinned
// slot and for MelWork::tab
struct MelTables {
    long long* wav_start;
    int *row_start, *nw, *frames;
    MelTables(char* base, int B)
        : wav_start(reinterpret_cast<long long*>(base)), row_start(reinterpret_cast<int*>(base + (size_t)B * 8)),
          nw(row_start + B + 1), frames(nw + B) {}
    static size_t bytes(int B) { return (size_t)B * 8 + ((size_t)3 * B + 1) * 4; }
};
}  // namespace

// carves the workspace out of the handle's arena (Arena::reserve: growth is the only synchronisation of a call)
static int mel_workspace(f5_mel* m, size_t signal_elems, int R, bool with_packed_out, size_t tab_bytes, MelWork* w) {
    auto plan = [&](Arena& a) {
        a.reset();
        w->wp = a.take<float>(signal_elems);
        w->spec = a.take<float>((size_t)R * m->ns);
        w->mag = a.take<float>((size_t)R * m->kf);
        w->pk = with_packed_out ? a.take<float>((size_t)R * m->n_mels) : nullptr;
        w->tab = a.take<char>(tab_bytes);
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(m->arena.reserve(plan(dry)));
    (void)plan(m->arena);
    return F5_OK;
}

// STFT GEMM -> magnitude -> mel GEMM with the log epilogue over R frames.  The frames are a strided view of the padded
// signal: row r starts at signal + r * hop (no im2col)
static int mel_rows(f5_mel* m, hipStream_t s, const MelWork& w, const float* signal, int R, float mag_eps, float* out, int ld_out) {
    HIPCHK(launch_gemm<float>(s, signal, m->hop, m->basis, m->n_fft, R, m->ns, m->n_fft, EpiStore<float>{w.spec, m->ns, nullptr, F5_ACT_NONE}));
    hipLaunchKernelGGL(magnitude_kernel, dim3(ew_blocks((long)R * m->kf)), dim3(256), 0, s, w.spec, m->ns, w.mag, m->kf, (long)R, m->F,
                       mag_eps);
    KCHK();
    HIPCHK(launch_gemm<float>(s, w.mag, m->kf, m->fb, m->kf, R, m->n_mels, m->kf, EpiStore<float>{out, ld_out, nullptr, F5_ACT_LOGCLAMP}));
    return F5_OK;
}

// wav f32[B, nw] -> out f32[B, T, n_mels], T = nw / hop + 1 (center=True)
extern "C" int f5_mel_forward(f5_mel* m, const float* wav, int32_t B, int32_t nw, float* out, f5_stream stream) {
    if (!m) return fail(F5_EINVAL, "f5_mel_forward: bad arguments");
    return f5_mel_forward_ex(m, wav, B, nw, m->n_fft / 2, 0.0f, out, stream);
}
// general form: reflect padding `pad` on both sides, frames at multiples of hop inside the padded signal
// (T = (nw + 2 pad - n_fft) / hop + 1), magnitude sqrt(re^2 + im^2 + mag_eps)
extern "C" int f5_mel_forward_ex(f5_mel* m, const float* wav, int32_t B, int32_t nw, int32_t pad, float mag_eps, float* out,
                                 f5_stream stream) {
    if (!m || !wav || !out || B <= 0 || pad < 0) return fail(F5_EINVAL, "f5_mel_forward: bad arguments");
    if (!m->basis || !m->fb) return fail(F5_ESTATE, "f5_mel_forward: aux.dft_basis / aux.mel_fb not loaded");
    if (nw <= pad || nw + 2 * pad < m->n_fft) return fail(F5_EINVAL, "f5_mel_forward: too few samples for the reflect padding / one frame");
    hipStream_t s = (hipStream_t)stream;
    const int T = (nw + 2 * pad - m->n_fft) / m->hop + 1, Lp = round_up(nw + 2 * pad, 4);
    MelWork w;
    CHK(mel_workspace(m, (size_t)B * Lp + m->n_fft, T, false, 0, &w));
    hipLaunchKernelGGL(reflect_pad_kernel, dim3(ew_blocks((long)B * Lp)), dim3(256), 0, s, wav, w.wp, B, nw, pad, Lp);
    KCHK();
    for (int b = 0; b < B; ++b) CHK(mel_rows(m, s, w, w.wp + (size_t)b * Lp, T, mag_eps, out + (size_t)b * T * m->n_mels, m->n_mels));
    return F5_OK;
}

// The row layout of the ragged front-end (pure host arithmetic): item b's padded signal of P_b = nw_b + 2 pad samples starts at
// sample row_start[b] * hop of the packed buffer and owns ceil(P_b / hop) rows, of which the first frames[b] are its frames.
extern "C" int f5_mel_ragged_plan(int32_t n_fft, int32_t hop, int32_t pad, int32_t B, const int32_t* nw_host, int32_t* row_start_out,
                                  int32_t* frames_out) {
    if (!nw_host || !row_start_out || !frames_out) return fail(F5_EINVAL, "f5_mel_ragged_plan: null nw_host / row_start_out / frames_out");
    if (n_fft <= 0 || hop <= 0) return fail(F5_EINVAL, "f5_mel_ragged_plan: need n_fft > 0 and hop > 0 (n_fft = %d, hop = %d)", n_fft, hop);
    if (B <= 0) return fail(F5_EINVAL, "f5_mel_ragged_plan: need B >= 1 items (B = %d)", B);
    if (pad < 0) return fail(F5_EINVAL, "f5_mel_ragged_plan: pad = %d < 0", pad);
    long rows = 0;
    for (int b = 0; b < B; ++b) {
        const long P = (long)nw_host[b] + 2L * pad;
        if (nw_host[b] <= pad || P < n_fft)
            return fail(F5_EINVAL, "f5_mel_ragged_plan: item %d has %d samples: too few for the reflect padding (%d) / one frame of %d", b,
                        nw_host[b], pad, n_fft);
        if (P > 0x7fffffffL - hop) return fail(F5_EINVAL, "f5_mel_ragged_plan: item %d has %d samples: its padded length overflows an int", b, nw_host[b]);
        row_start_out[b] = (int32_t)rows;
        frames_out[b] = (int32_t)((P - n_fft) / hop + 1);
        rows += (P + hop - 1) / hop;
        if (rows > (1L << 24))
            return fail(F5_EINVAL, "f5_mel_ragged_plan: more than 2^24 packed rows at item %d (the GEMMs index rows as int)", b);
    }
    row_start_out[B] = (int32_t)rows;
    return F5_OK;
}

// A list of prompts of unequal length -> the zero-padded mel batch, in ONE pass over the packed rows of every item:
// item b = wav[wav_start_host[b] .. + nw_host[b]) -> out[b * out_stride_b + t * n_mels + c], t < T_out (rows >= T_b are +0.0)
extern "C" int f5_mel_forward_ragged(f5_mel* m, const float* wav, int32_t B, const int64_t* wav_start_host, const int32_t* nw_host,
                                     int32_t pad, float mag_eps, float* out, int64_t out_stride_b, int32_t T_out, f5_stream stream) {
    if (!m) return fail(F5_EINVAL, "f5_mel_forward_ragged: null handle m");
    if (!wav) return fail(F5_EINVAL, "f5_mel_forward_ragged: null wav");
    if (!wav_start_host) return fail(F5_EINVAL, "f5_mel_forward_ragged: null wav_start_host");
    if (!nw_host) return fail(F5_EINVAL, "f5_mel_forward_ragged: null nw_host");
    if (!out) return fail(F5_EINVAL, "f5_mel_forward_ragged: null out");
    if (B <= 0) return fail(F5_EINVAL, "f5_mel_forward_ragged: need B >= 1 items (B = %d)", B);
    if (pad < 0) return fail(F5_EINVAL, "f5_mel_forward_ragged: pad = %d < 0", pad);
    for (int b = 0; b < B; ++b)
        if (wav_start_host[b] < 0)
            return fail(F5_EINVAL, "f5_mel_forward_ragged: item %d starts at wav_start = %lld < 0", b, (long long)wav_start_host[b]);
    m->plan_rows.resize((size_t)2 * B + 1);
    int32_t* rs = m->plan_rows.data();
    int32_t* frames = rs + B + 1;
    if (f5_mel_ragged_plan(m->n_fft, m->hop, pad, B, nw_host, rs, frames) != F5_OK) return F5_EINVAL;   // (its message names the item)
    const int R = rs[B];
    int tmax = 0;
    for (int b = 0; b < B; ++b) tmax = std::max(tmax, (int)frames[b]);
    if (T_out < tmax) return fail(F5_EINVAL, "f5_mel_forward_ragged: T_out = %d is less than the longest item's %d frames", T_out, tmax);
    if (out_stride_b < (int64_t)T_out * m->n_mels)
        return fail(F5_EINVAL, "f5_mel_forward_ragged: out_stride_b = %lld is less than T_out * n_mels = %lld", (long long)out_stride_b,
                    (long long)T_out * m->n_mels);
    if (!m->basis || !m->fb) return fail(F5_ESTATE, "f5_mel_forward_ragged: aux.dft_basis / aux.mel_fb not loaded");
    hipStream_t s = (hipStream_t)stream;
    MelWork w;
    CHK(mel_workspace(m, (size_t)R * m->hop + m->n_fft, R, true, MelTables::bytes(B), &w));
    // one pinned slot, one copy; the device tables are read by this call's kernels only
    CHK(m->stage.upload(w.tab, MelTables::bytes(B), s, [&](char* host) {
        const MelTables h(host, B);
        for (int b = 0; b < B; ++b) {
            h.wav_start[b] = wav_start_host[b];
            h.row_start[b] = rs[b];
            h.nw[b] = nw_host[b];
            h.frames[b] = frames[b];
        }
        h.row_start[B] = R;
    }));
    const MelTables d(w.tab, B);

    const int pad_rows = R + (m->n_fft + m->hop - 1) / m->hop;
    hipLaunchKernelGGL(reflect_pad_ragged_kernel, dim3((unsigned)std::min(pad_rows, 16384)), dim3(256), 0, s, wav, w.wp, d.wav_start,
                       d.row_start, d.nw, B, R, m->hop, pad, m->n_fft);
    KCHK();
    // (dead rows included: they cost a few rows per item)
    CHK(mel_rows(m, s, w, w.wp, R, mag_eps, w.pk, m->n_mels));
    const long quads = (long)B * T_out * (m->n_mels / 4);
    if ((reinterpret_cast<uintptr_t>(out) % 16) == 0 && out_stride_b % 4 == 0)
        hipLaunchKernelGGL((mel_unpack_ragged_kernel<true>), dim3(ew_blocks(quads)), dim3(256), 0, s, w.pk, out, d.row_start, d.frames, B, T_out,
                           m->n_mels, (long)out_stride_b);
    else
        hipLaunchKernelGGL((mel_unpack_ragged_kernel<false>), dim3(ew_blocks(quads)), dim3(256), 0, s, w.pk, out, d.row_start, d.frames, B, T_out,
                           m->n_mels, (long)out_stride_b);
    KCHK();
    return F5_OK;
}
