// Vocos (mel -> waveform) on gfx950: ConvNeXt backbone + ISTFT head, all f32 (the reference feeds the vocoder fp32,
// infer/utils_infer.py:699-703).  Every contraction is an exact-f32 MFMA GEMM (gemm.h):
//   embed Conv1d(C, dim, k=7)  = im2col (7*C columns) x W[dim, 7*C]
//   pwconv1 / pwconv2 / head   = nn.Linear
//   inverse real DFT + window  = S[T, 2F(+pad)] x Basis[n_fft, 2F(+pad)]^T   (Basis host-computed in float64 -> f32,
//                                hann window and 1/n_fft folded in; exact restatement of torch.istft's irfft * window)
// followed by overlap-add / window-envelope normalisation / centre trim (torch.istft(center=True)).
// f5_vocos_decode_ragged runs the same stages once over the packed frames of a batch of windows (ragged decode).
#include <string>
#include <vector>

#include "elementwise.h"
#include "gemm_dispatch.h"
#include "internal.h"

using namespace f5;
#define fail f5_fail

namespace {
struct VBlock {
    float *dwk, *dwb, *lnw, *lnb, *w1, *b1, *w2, *b2, *gamma;
};
// The ragged decode's per-item tables, row_start[B + 1] | mel_start[B] | gain[B]: one layout for the pinned slot and for VWork::tab
struct VTables {
    int *row_start, *mel_start;
    float* gain;
    VTables(void* base, int B) : row_start(static_cast<int*>(base)), mel_start(row_start + B + 1), gain(reinterpret_cast<float*>(mel_start + B)) {}
    static size_t words(int B) { return (size_t)3 * B + 1; }
};
}  // namespace

struct f5_vocos {
    f5_vocos_config cfg{};
    WeightStore raw;
    DevPool pool;   // what finalize built
    bool finalized = false;
    int F = 0, K2 = 0, kemb = 0, head_n = 0;
    float *emb_w = nullptr, *emb_b = nullptr, *n0w = nullptr, *n0b = nullptr, *fnw = nullptr, *fnb = nullptr;
    float *head_w = nullptr, *head_b = nullptr, *hann = nullptr, *basis = nullptr;
    std::vector<VBlock> blocks;
    Arena arena;
    Staging stage;   // pinned slots for the ragged decode's per-call tables
};

extern "C" int f5_vocos_create(const f5_vocos_config* c, f5_vocos** out) {
    if (!c || !out) return fail(F5_EINVAL, "f5_vocos_create: null argument");
    if (c->dim % 4 || c->dim > 2048 || c->intermediate_dim % 4 || c->input_channels % 4 || c->n_fft % 4 ||
        c->hop_length <= 0 || c->n_fft % c->hop_length)
        return fail(F5_EINVAL, "f5_vocos_create: unsupported dimensions");
    f5_vocos* v = new f5_vocos();
    v->cfg = *c;
    v->F = c->n_fft / 2 + 1;
    v->K2 = round_up(2 * v->F, 32);            // whole 128-byte K-tiles (f32) for the LDS-DMA GEMM
    v->kemb = round_up(7 * c->input_channels, 32);
    v->head_n = round_up(c->n_fft + 2, 4);
    *out = v;
    return F5_OK;
}
extern "C" int f5_vocos_destroy(f5_vocos* v) {
    if (v) {
        (void)hipDeviceSynchronize();
        delete v;
    }
    return F5_OK;
}
extern "C" int f5_vocos_load_weight(f5_vocos* v, const char* name, const void* dev, const int64_t* shape, int32_t ndim,
                                    f5_stream stream) {
    if (!v) return fail(F5_EINVAL, "f5_vocos_load_weight: bad arguments");
    CHK(v->raw.put("f5_vocos_load_weight", name, dev, shape, ndim, (hipStream_t)stream));
    v->finalized = false;
    return F5_OK;
}

extern "C" int f5_vocos_finalize(f5_vocos* v, f5_stream stream) {
    if (!v) return fail(F5_EINVAL, "null vocos");
    hipStream_t s = (hipStream_t)stream;
    const f5_vocos_config& c = v->cfg;
    const int C = c.input_channels, D = c.dim, I = c.intermediate_dim;
    v->pool.clear();
    auto copy = [&](const std::string& n, std::vector<int64_t> shape, float** out) { return v->pool.copy_of(v->raw, n, shape, "vocos", s, out); };
    // embed conv [D, C, 7] -> [D, 7*C]
    const Tensor* t = nullptr;
    CHK(v->raw.need("backbone.embed.weight", {D, C, 7}, "vocos", &t));
    {
        Scratch<float> tmp;  // [D, 7*C] tap-major, then zero-padded to kemb columns
        HIPCHK(tmp.alloc((size_t)D * 7 * C));
        hipLaunchKernelGGL((permute_last2_kernel<float>), dim3(ew_blocks((long)D * 7 * C)), dim3(256), 0, s, t->p, tmp.p,
                           (long)D, C, 7);
        CHK(v->pool.alloc((size_t)D * v->kemb, &v->emb_w));
        hipLaunchKernelGGL((cast_pad_kernel<float>), dim3(ew_blocks((long)D * v->kemb)), dim3(256), 0, s, tmp.p, 7 * C, D,
                           7 * C, v->emb_w, v->kemb, D);
        KCHK();
        HIPCHK(hipStreamSynchronize(s));
    }
    CHK(copy("backbone.embed.bias", {D}, &v->emb_b));
    CHK(copy("backbone.norm.weight", {D}, &v->n0w));
    CHK(copy("backbone.norm.bias", {D}, &v->n0b));
    CHK(copy("backbone.final_layer_norm.weight", {D}, &v->fnw));
    CHK(copy("backbone.final_layer_norm.bias", {D}, &v->fnb));
    v->blocks.resize(c.num_layers);
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string pf = "backbone.convnext." + std::to_string(i);
        VBlock& b = v->blocks[i];
        CHK(v->raw.need(pf + ".dwconv.weight", {D, 1, 7}, "vocos", &t));
        CHK(v->pool.alloc((size_t)7 * D, &b.dwk));
        hipLaunchKernelGGL((permute_last2_kernel<float>), dim3(ew_blocks(7L * D)), dim3(256), 0, s, t->p, b.dwk, 1L, D, 7);
        KCHK();
        CHK(copy(pf + ".dwconv.bias", {D}, &b.dwb));
        CHK(copy(pf + ".norm.weight", {D}, &b.lnw));
        CHK(copy(pf + ".norm.bias", {D}, &b.lnb));
        CHK(copy(pf + ".pwconv1.weight", {I, D}, &b.w1));
        CHK(copy(pf + ".pwconv1.bias", {I}, &b.b1));
        CHK(copy(pf + ".pwconv2.weight", {D, I}, &b.w2));
        CHK(copy(pf + ".pwconv2.bias", {D}, &b.b2));
        CHK(copy(pf + ".gamma", {D}, &b.gamma));
    }
    // head: [n_fft + 2, D] padded to head_n rows (zero rows / zero bias)
    CHK(v->raw.need("head.out.weight", {c.n_fft + 2, D}, "vocos", &t));
    CHK(v->pool.alloc((size_t)v->head_n * D, &v->head_w));
    hipLaunchKernelGGL((cast_pad_kernel<float>), dim3(ew_blocks((long)v->head_n * D)), dim3(256), 0, s, t->p, D, c.n_fft + 2,
                       D, v->head_w, D, v->head_n);
    KCHK();
    CHK(v->raw.need("head.out.bias", {c.n_fft + 2}, "vocos", &t));
    CHK(v->pool.alloc((size_t)v->head_n, &v->head_b));
    hipLaunchKernelGGL((cast_pad_kernel<float>), dim3(1), dim3(256), 0, s, t->p, c.n_fft + 2, 1, c.n_fft + 2, v->head_b,
                       v->head_n, 1);
    KCHK();
    CHK(copy("aux.hann", {c.n_fft}, &v->hann));
    CHK(copy("aux.idft_basis", {c.n_fft, v->K2}, &v->basis));
    HIPCHK(hipStreamSynchronize(s));
    v->raw.clear();
    v->finalized = true;
    return F5_OK;
}

extern "C" int f5_vocos_decode(f5_vocos* v, const float* mel, int32_t B, int32_t T, float* wav, f5_stream stream) {
    if (!v) return fail(F5_EINVAL, "f5_vocos_decode: null argument");
    return f5_vocos_decode_strided(v, mel, B, T, (int64_t)v->cfg.input_channels * T, T, 1, wav, stream);
}

namespace {
// Workspace of one decode over R rows (frames): the rectangular call has R = B * T, the ragged one R = sum of T_b packed rows
struct VWork {
    float *col, *x, *t1, *h, *hd, *S, *fr;
    int* tab;   // ragged only: VTables
};
}  // namespace

// carves the workspace out of the handle's arena (Arena::reserve: growth is the only synchronisation of a decode)
static int vocos_workspace(f5_vocos* v, long R, size_t ntab, VWork* w) {
    const f5_vocos_config& c = v->cfg;
    auto plan = [&](Arena& a) {
        a.reset();
        w->col = a.take<float>((size_t)R * v->kemb);
        w->x = a.take<float>((size_t)R * c.dim);
        w->t1 = a.take<float>((size_t)R * c.dim);
        w->h = a.take<float>((size_t)R * c.intermediate_dim);
        w->hd = a.take<float>((size_t)R * v->head_n);
        w->S = a.take<float>((size_t)R * v->K2);
        w->fr = a.take<float>((size_t)R * c.n_fft);
        w->tab = a.take<int>(ntab);
        return align_up(a.off, 256) + 256;
    };
    Arena dry;
    CHK(v->arena.reserve(plan(dry)));
    (void)plan(v->arena);
    return F5_OK;
}

// embed GEMM .. iDFT GEMM over the R rows of w.col -> w.fr.  Every stage but the depthwise conv works row by row; the conv
// sees B rows of T frames, or (row_start given) the segments of a packed batch.
static int vocos_rows(f5_vocos* v, hipStream_t s, const VWork& w, long R, int B, int T, const int* row_start) {
    const f5_vocos_config& c = v->cfg;
    const int D = c.dim, I = c.intermediate_dim, nfft = c.n_fft;
    float *col = w.col, *x = w.x, *t1 = w.t1, *h = w.h, *hd = w.hd, *S = w.S, *fr = w.fr;
    HIPCHK(launch_gemm<float>(s, col, v->kemb, v->emb_w, v->kemb, (int)R, D, v->kemb, EpiStore<float>{t1, D, v->emb_b, F5_ACT_NONE}));
    hipLaunchKernelGGL((layernorm_kernel<float>), dim3((R + 3) / 4), dim3(256), 0, s, t1, D, x, D, (int)R, D, 1e-6f, v->n0w,
                       v->n0b, 0, 0, 0, Prefetch{});
    KCHK();
    for (auto& b : v->blocks) {
        if (row_start)
            hipLaunchKernelGGL(dwconv7_ln_ragged_kernel, dim3((R + 3) / 4), dim3(256), 0, s, x, t1, b.dwk, b.dwb, b.lnw, b.lnb,
                               row_start, B, (int)R, D, 1e-6f);
        else
            hipLaunchKernelGGL(dwconv7_ln_kernel, dim3((R + 3) / 4), dim3(256), 0, s, x, t1, b.dwk, b.dwb, b.lnw, b.lnb, B, T, D,
                               (const int*)nullptr, 1e-6f);
        KCHK();
        HIPCHK(launch_gemm<float>(s, t1, D, b.w1, D, (int)R, I, D, EpiStore<float>{h, I, b.b1, F5_ACT_GELU_ERF}));
        // x = x + gamma * (pwconv2(h) + bias)   (layer scale == a gate vector shared by every row)
        HIPCHK(launch_gemm<float>(s, h, I, b.w2, I, (int)R, D, I, EpiGateRes{x, x, D, b.b2, b.gamma, 0, (int)R + 1, nullptr}));
    }
    hipLaunchKernelGGL((layernorm_kernel<float>), dim3((R + 3) / 4), dim3(256), 0, s, x, D, t1, D, (int)R, D, 1e-6f, v->fnw,
                       v->fnb, 0, 0, 0, Prefetch{});
    KCHK();
    HIPCHK(launch_gemm<float>(s, t1, D, v->head_w, D, (int)R, v->head_n, D, EpiStore<float>{hd, v->head_n, v->head_b, F5_ACT_NONE}));
    hipLaunchKernelGGL(istft_spec_kernel, dim3(ew_blocks(R * v->K2)), dim3(256), 0, s, hd, v->head_n, S, v->K2, R, v->F);
    KCHK();
    HIPCHK(launch_gemm<float>(s, S, v->K2, v->basis, v->K2, (int)R, nfft, v->K2, EpiStore<float>{fr, nfft, nullptr, F5_ACT_NONE}));
    return F5_OK;
}

extern "C" int f5_vocos_decode_strided(f5_vocos* v, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_c,
                                       int64_t stride_t, float* wav, f5_stream stream) {
    if (!v || !mel || !wav) return fail(F5_EINVAL, "f5_vocos_decode: null argument");
    if (!v->finalized) return fail(F5_ESTATE, "f5_vocos_finalize has not been called");
    if (B <= 0 || T < 2) return fail(F5_EINVAL, "f5_vocos_decode: need B >= 1 and T >= 2 frames");
    hipStream_t s = (hipStream_t)stream;
    const f5_vocos_config& c = v->cfg;
    const long R = (long)B * T;
    VWork w;
    CHK(vocos_workspace(v, R, 0, &w));
    hipLaunchKernelGGL(im2col7_kernel, dim3(ew_blocks(R * v->kemb)), dim3(256), 0, s, mel, (long)stride_b, (long)stride_c,
                       (long)stride_t, w.col, B, c.input_channels, T, v->kemb);
    KCHK();
    CHK(vocos_rows(v, s, w, R, B, T, nullptr));
    hipLaunchKernelGGL(istft_ola_kernel, dim3(ew_blocks((long)B * (T - 1) * c.hop_length)), dim3(256), 0, s, w.fr, v->hann, wav,
                       B, T, c.n_fft, c.hop_length);
    KCHK();
    return F5_OK;
}

extern "C" int f5_vocos_decode_ragged(f5_vocos* v, const float* mel, int32_t B, int64_t stride_b, int64_t stride_c,
                                      int64_t stride_t, const int32_t* starts_host, const int32_t* ends_host,
                                      const float* gain_host, float* wav, int64_t wav_stride, f5_stream stream) {
    if (!v || !mel || !ends_host || !wav) return fail(F5_EINVAL, "f5_vocos_decode_ragged: null argument");
    if (!v->finalized) return fail(F5_ESTATE, "f5_vocos_finalize has not been called");
    if (B <= 0 || B > 65535) return fail(F5_EINVAL, "f5_vocos_decode_ragged: need 1 <= B <= 65535 items (B = %d)", B);
    const f5_vocos_config& c = v->cfg;
    long R = 0, lmax = 0;
    for (int b = 0; b < B; ++b) {
        const int st = starts_host ? starts_host[b] : 0, Tb = ends_host[b] - st;
        if (st < 0) return fail(F5_EINVAL, "f5_vocos_decode_ragged: item %d starts at frame %d < 0", b, st);
        if (Tb < 2)
            return fail(F5_EINVAL, "f5_vocos_decode_ragged: item %d has %ld frame(s) (frames [%d, %d)); need at least 2", b,
                        std::max(0L, (long)ends_host[b] - st), st, ends_host[b]);
        R += Tb;
        lmax = std::max(lmax, (long)(Tb - 1) * c.hop_length);
    }
    if (wav_stride < lmax)
        return fail(F5_EINVAL, "f5_vocos_decode_ragged: wav_stride %lld is less than the longest waveform (%ld samples)",
                    (long long)wav_stride, lmax);
    if (R > (1L << 24)) return fail(F5_EINVAL, "f5_vocos_decode_ragged: %ld frames in one call (at most 2^24: the GEMMs index rows as int)", R);
    hipStream_t s = (hipStream_t)stream;
    VWork w;
    CHK(vocos_workspace(v, R, VTables::words(B), &w));
    // the segment table, the window starts and the gains go down through one pinned slot; the device copy is read by this
    // call's kernels only, which are ahead of the next call's copy on the stream
    CHK(v->stage.upload(w.tab, VTables::words(B) * 4, s, [&](char* host) {
        const VTables h(host, B);
        h.row_start[0] = 0;
        for (int b = 0; b < B; ++b) {
            h.mel_start[b] = starts_host ? starts_host[b] : 0;
            h.row_start[b + 1] = h.row_start[b] + (ends_host[b] - h.mel_start[b]);
            h.gain[b] = gain_host ? gain_host[b] : 1.0f;
        }
    }));
    const VTables d(w.tab, B);
    const int *row_start = d.row_start, *mel_start = d.mel_start;
    const float* gain = d.gain;

    hipLaunchKernelGGL(im2col7_ragged_kernel, dim3((unsigned)std::min(R, 16384L)), dim3(256), 0, s, mel, (long)stride_b,
                       (long)stride_c, (long)stride_t, row_start, mel_start, w.col, B, c.input_channels, (int)R, v->kemb);
    KCHK();
    CHK(vocos_rows(v, s, w, R, B, 0, row_start));
    hipLaunchKernelGGL(istft_ola_ragged_kernel, dim3(ew_blocks(wav_stride), B), dim3(256), 0, s, w.fr, v->hann, row_start, gain,
                       wav, (long)wav_stride, c.n_fft, c.hop_length);
    KCHK();
    return F5_OK;
}
