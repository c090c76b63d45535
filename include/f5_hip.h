/* f5_hip.h -- C ABI of libf5hip.so, the MI355X (gfx950) engine for the F5-TTS inference hot path.
 *
 * Plain C: opaque handles, raw device pointers, sizes and a hipStream_t passed as void*.  No torch / C++ types.
 * Every entry point returns 0 on success or a negative F5_E* code; f5_last_error() returns the message of the last
 * failure on the calling thread.  All work is enqueued on the caller's stream; the library never synchronises the
 * device except where a function's comment says so.  Device pointers are borrowed for the duration of the call
 * (weights are copied / repacked into engine-owned memory by f5_load_weight + f5_finalize).
 *
 * Each function names the reference interface it replaces (paths relative to the reference's src/f5_tts/):
 *   f5_sample        <- CFM.sample's ODE solve                       model/cfm.py:151-223 (odeint call :218)
 *   f5_sample_ode    <- the same with odeint_kwargs=dict(method="euler" | "midpoint")  model/cfm.py:42,218
 *   f5_dit_forward   <- DiT.forward / UNetT.forward                  model/backbones/dit.py:278-329, unett.py:217-280
 *   f5_flow_loss     <- CFM.forward (inference mode)                  model/cfm.py:231-302
 *   f5_text_embed    <- TextEmbedding.forward (+ per-sample loop)    model/backbones/dit.py:86-115,244-258
 *   f5_vocos_decode  <- vocoder.decode(mel)                          infer/utils_infer.py:702-703 (third-party vocos)
 *   f5_vocos_decode_ragged <- the per-item vocoder loop of a batch   eval/eval_infer_batch.py:202-212
 *   f5_bigvgan_forward <- vocoder(mel) (third-party BigVGAN v2)      infer/utils_infer.py:138-152,705
 *   f5_wave_crossfade <- the cross-fade concatenation of the chunks  infer/utils_infer.py:734-775
 *   f5_wave_join <- infer_cli.py:363-415, the multi-voice script: per-stretch cross-fades, np.concatenate between stretches
 *   f5_edit_assemble <- speech editing's mel_cond torch.cat chain    infer/speech_edit.py:157-195
 *   f5_wave_splice   <- (no counterpart) the original recording outside the edited spans of speech_edit.py's output
 *   f5_mel_forward   <- MelSpec.forward (vocos / bigvgan type)       model/modules.py:33-146
 *   f5_mel_forward_ragged <- the per-prompt MelSpec loop + padded_mel_batch  eval/utils_eval.py:109-148
 *   f5_mel_prepare_ragged <- the per-prompt mono mix, RMS, level and resample  infer/utils_infer.py:523-533, eval/utils_eval.py:111-118
 *   f5_load_weight   <- load_checkpoint's state-dict assignment      infer/utils_infer.py:242-286
 * The reference-side binding (ctypes) is shown in INTEGRATION.md.
 */
#ifndef F5_HIP_H
#define F5_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F5_OK 0
#define F5_EINVAL (-1)   /* bad argument / shape / unsupported configuration */
#define F5_EHIP (-2)     /* a HIP runtime call failed */
#define F5_ESTATE (-3)   /* call order violated (e.g. compute before f5_finalize) */
#define F5_ENOMEM (-4)

#define F5_PREC_F32 0    /* exact-f32 MFMA everywhere ("parity" mode) */
#define F5_PREC_BF16 1   /* bf16 MFMA operands, f32 accumulate, f32 residual stream / ODE state / norms */
#define F5_PREC_F16 2    /* fp16 MFMA operands (the reference's own GPU dtype, infer/utils_infer.py:243-251; same MFMA rate as
                            bf16, 3 more mantissa bits), f32 accumulate, f32 residual stream / ODE state / norms */
#define F5_PREC_F16X3 3  /* f32 data flow (activations, attention, norms as F5_PREC_F32); each GEMM operand is split into two fp16
                            halves (hi + lo, 22 bits) and the product takes three fp16 MFMAs: f32-level results; the backbone GEMMs run
                            at ~2.5-3x the f32 MFMA rate, a C2 utterance in 0.41x the f32 time.  The two attention products
                            use the hi halves only (plain fp16 products: measured harmless; F5_X3_ATTN_SPLIT=1 for three).
                            |activation| < 65504 as for F5_PREC_F16 */

#define F5_PREC_F16P 4   /* F5_PREC_F16 in the transformer blocks (fp16 MFMA operands, f32 accumulate / residual / norms) with the
                            model's input and output layers -- input projection, conv position embedding, final norm + output
                            projection -- as split-fp16 products on f32 operands (as F5_PREC_F16X3): the rounding of the ODE state
                            entering and of the flow prediction leaving the backbone is what dominates F5_PREC_F16's error (DESIGN.md
                            section 3, tools/x3_ablate.py); meets the 1e-3 parity bar at ~F5_PREC_F16 speed */

#define F5_PREC_F8 5     /* F5_PREC_F16P with the operands of the four GEMMs of every DiT block -- QKV, attention out-projection, FF1, FF2 --
                            in OCP e4m3 (e4m3fn, never fnuz) on gfx950's block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4: twice the
                            fp16 rate per clock, half the operand bytes).  Everything else as F5_PREC_F16P: fp16 attention, split-fp16
                            input embedding and output projection, f32 residual stream / norms / ODE state, time path, text path and
                            conv position embedding untouched.  DiT backbone only, not with F5_OPT_ADAPTERS; heads even and
                            ff_dim % 128 == 0 (every K a whole number of 128-element tiles).
                            The f8 arithmetic contract (csrc/e4m3.h, quant8.h, gemm8.h):
                              Scales   powers of two, one e8m0 byte b (value 2^(b - 127)) per ROW of an A operand and per OUTPUT
                                       CHANNEL of a weight: the smallest power of two s with amax / s <= 448, amax over the row's K real
                                       elements (pad columns do not count); amax == 0 gives b = 127.  Dynamic and per row, so a row's
                                       result depends on that row alone: isolated rows, packed == padded, bucketed graph == exact and
                                       replay == eager hold under f8 as under every other precision.
                              Codes    code = e4m3(x / s), round to nearest even, saturating at +-448; x / s is exact, so the code is a
                                       pure function of x.  NaN / Inf inputs are outside the contract.
                              Product  C[m][n] = 2^(ba[m] + bw[n] - 254) * sum_k codeA[m][k] codeW[n][k], accumulated in f32 by the MFMA.
                                       The instruction's own scale operands are fed 2^0; the two powers of two are MULTIPLIED ONTO THE
                                       ACCUMULATORS before the epilogue (exact), which then runs unchanged (EpiQKV, EpiStore + GELU-tanh,
                                       EpiGateRes / EpiGateResRows).
                              Rounding points
                                       xn (QKV / FF1 operand): quantised from the f32 value LN(x)(1 + scale) + shift inside the LayerNorm
                                       kernel, with no fp16 step between.
                                       ao (attention output) and ffh (FF hidden, after GELU): ROUNDED TO FP16 FIRST -- the attention kernel
                                       and FF1's epilogue write today's fp16 buffers -- and quantised from those by the stand-alone
                                       row quantiser.
                                       Weights: from the f32 master at f5_finalize; K padding is zero codes; no fp16 copy is kept. */

#define F5_OPT_QK_RMSNORM 1        /* qk_norm="rms_norm" (modules.py:397-404,481-484): weights ...attn.q_norm.weight / k_norm.weight [64] */
#define F5_OPT_LONG_SKIP 2         /* long_skip_connection=True (dit.py:205,313-324): long_skip_connection.weight [D, 2D] */
#define F5_OPT_TEXT_AVG_UPSAMPLE 4 /* text_embedding_average_upsampling=True (dit.py:54-84; needs text_mask_padding) */
#define F5_OPT_ADAPTERS 8          /* resident LoRA adapters (f5_adapter_*, f5_set_adapter below): f5_finalize keeps the fp32 masters
                                      of the adaptable tensors.  Not a constructor option of the reference: its counterpart is
                                      train/train_lora.py's recipe + the merge of infer/utils_infer.py:198-239 */

#define F5_BACKBONE_DIT 0
#define F5_BACKBONE_UNETT 1
#define F5_BACKBONE_MMDIT 2 /* MMDiT(...) (mmdit.py:85-127): two streams -- text c [B, nt, D], audio x [B, N, D] -- with their own weights and
                               AdaLN vectors, joined in one attention over nt + N keys.  Read from f5_config: dim, depth, heads, dim_head, ff_dim,
                               mel_dim, text_num_embeds, text_mask_padding and F5_OPT_QK_RMSNORM (text_dim, conv_layers, pe_attn_head and
                               attn_mask_enabled are not: the text is embedded at width dim, every head is rotated, a mask that is given
                               is always applied).  aux.text_pos [>= nt, dim] is its sinus table.  A batch runs rectangular, padding rows
                               computed (its input conv is unmasked).  f5_text_embed writes [B, nt, dim] and ignores N and lens.  Refused,
                               with the reason: the other F5_OPT_* bits, texts of more than 1024 tokens, F5_SPLIT_CFG=1, length buckets,
                               isolated rows, f5_sample_items, f5_sample_span, f5_prepare_sample and the adapter calls. */

typedef struct f5_engine f5_engine;
typedef struct f5_vocos f5_vocos;
typedef void* f5_stream; /* hipStream_t */

/* Arch of the backbone: the keyword arguments of DiT(...) / UNetT(...) (dit.py:147-168, unett.py:107-128). */
typedef struct f5_config {
    int32_t backbone;          /* F5_BACKBONE_* */
    int32_t precision;         /* F5_PREC_* */
    int32_t dim;               /* model width D: 256, 512, 768 or 1024 */
    int32_t depth;
    int32_t heads;
    int32_t dim_head;          /* must be 64 */
    int32_t ff_dim;            /* int(dim * ff_mult) */
    int32_t text_dim;
    int32_t conv_layers;       /* ConvNeXt-V2 text blocks */
    int32_t pe_attn_head;      /* heads that receive rotary; <0 = all (pe_attn_head=None) */
    int32_t text_mask_padding; /* dit.py:39,90-91,104-108 */
    int32_t attn_mask_enabled; /* modules.py:501-506 */
    int32_t text_num_embeds;   /* constructor argument; the table has text_num_embeds + 1 rows */
    int32_t mel_dim;           /* 100 */
    int32_t max_pos;           /* rows of the rotary table given as aux.rope_cos/sin (>= longest sequence) */
    int32_t options;           /* F5_OPT_* bits: the DiT constructor options no shipped config switches on */
    int32_t reserved[4];
} f5_config;

const char* f5_last_error(void);
/* Build id string ("f5hip <n> gfx950"). */
const char* f5_version(void);

int f5_create(const f5_config* cfg, f5_engine** out);
int f5_destroy(f5_engine* e);

/* Copies one tensor (fp32, contiguous, device memory) into the engine under its reference state-dict name, e.g.
 * "transformer_blocks.3.attn.to_q.weight" (names: model/backbones/dit.py, unett.py; convert_checkpoint.py:129-145).
 * Host-computed constant tables travel the same way under reserved names:
 *   aux.rope_cos / aux.rope_sin [max_pos, 32]   rotary angles n * 10000^(-2j/64)          (x_transformers RotaryEmbedding)
 *   aux.time_freqs [128]                         exp(-k ln(1e4)/127)                       (modules.py:159-161)
 *   aux.text_pos [P, text_dim]                   precompute_freqs_cis(text_dim, P)         (modules.py:202-213)   */
int f5_load_weight(f5_engine* e, const char* name, const void* dev_f32, const int64_t* shape, int32_t ndim,
                   f5_stream stream);
/* Checks that every tensor the arch needs is present and repacks (fused QKV, stacked AdaLN, conv tap-major, bf16).
 * Synchronises the stream once. */
int f5_finalize(f5_engine* e, f5_stream stream);

/* text i64[B, nt] (device, padded with -1) -> out f32[B, N, text_dim] (device).  lens (HOST int32[B] or NULL): each
 * sample is embedded at its own length and zero padded to N, as dit.py:247-258 does when an audio mask is given. */
int f5_text_embed(f5_engine* e, const int64_t* text, int32_t B, int32_t nt, const int32_t* lens_host, int32_t N,
                  int32_t drop_text, float* out, f5_stream stream);

/* One backbone forward (dit.py:278-329).  x, cond f32[B, N, mel]; text i64[B, nt]; time HOST f32[B];
 * lens HOST int32[B] or NULL (= the reference's mask=None).  cfg_infer != 0 packs cond + uncond: out f32[2B, N, mel],
 * else out f32[B, N, mel] with the given drop flags.  Text embeddings are recomputed on every call (cache=False). */
int f5_dit_forward(f5_engine* e, const float* x, const float* cond, const int64_t* text, int32_t nt,
                   const float* time_host, const int32_t* lens_host, int32_t B, int32_t N, int32_t cfg_infer,
                   int32_t drop_audio_cond, int32_t drop_text, float* out, f5_stream stream);

/* The teacher-forced flow-matching loss of CFM.forward (cfm.py:261-302) around ONE backbone evaluation, in inference mode (no gradient):
 *   phi = (1 - time[b]) * x0 + time[b] * x1;  cond = x1 with the frames of span[b] zeroed;  pred = backbone(phi, cond, text, time, drops);
 *   sq_sum[b] = sum over the frames of span[b] and over mel of (pred - (x1 - x0))^2, accumulated in f64.
 *   x1 (the mel), x0 (the noise) f32[B, N, mel] and text i64[B, nt] on the device; time HOST f32[B]; lens HOST int32[B] or NULL (= the
 *   reference's lens=None: every item has N frames), each in (0, N]; span HOST int32[B][2] = (start, end) in frames with
 *   0 <= start <= end <= lens[b] -- the one interval that the reference's rand_span_mask & mask is; drop_audio_cond, drop_text: cfm.py:286-291.
 *   sq_sum f64[B] and count int32[B] (= end - start) on the device; pred, cond f32[B, N, mel] and frame_err f32[B, N] on the device, each
 *   NULL or written: frame_err[b, n] = the frame's mean over mel of the squared error inside the span, +0.0 outside it.
 * The reference's loss is sum(sq_sum) / (sum(count) * mel), which the caller forms where it wants it: nothing is read back and the host
 * is not synchronised.  A frame outside span[b] is never read for the loss.  Frames at or past lens[b] get phi and cond as any other
 * frame (cfm.py:279-283) and the backbone treats them as f5_dit_forward does.  Every backbone f5_dit_forward runs is accepted; the
 * arithmetic of the glue is written out in csrc/flow.h.  Not captured in a graph.
 * F5_EINVAL with a message naming the item, before the engine is touched: a non-finite time, lens[b] outside (0, N], a span outside
 * 0 <= start <= end <= lens[b]. */
int f5_flow_loss(f5_engine* e, const float* x1, const float* x0, const int64_t* text, int32_t nt, const float* time_host,
                 const int32_t* lens_host, const int32_t* span_host, int32_t B, int32_t N, int32_t drop_audio_cond, int32_t drop_text,
                 double* sq_sum, int32_t* count, float* pred, float* cond, float* frame_err, f5_stream stream);

/* The ODE solve of CFM.sample (cfm.py:151-223): step_cond = where(cond_mask, cond, 0); `steps` Euler steps over the
 * HOST time grid t[steps + 1] with classifier-free guidance (cfg_strength < 1e-5 -> single conditional forward);
 * out = where(cond_mask, cond, y_final).
 *   cond f32[B, cond_frames, mel] (cond_frames <= N; the frames cond_frames .. N-1 read as zero: the reference's
 *   F.pad(cond, (0, 0, 0, N - cond_seq_len)), cfm.py:145; cond_frames = 0 is no_ref_audio), cond_mask u8[B, N], y0 f32[B, N, mel],
 *   text i64[B, nt], lens HOST int32[B] = per-sample durations or NULL when B == 1 (cfm.py:155-158),
 *   out f32[B, N, mel], traj f32[steps + 1, B, N, mel] or NULL.
 * The text embeddings are computed once per call (the reference's per-sample() cache, dit.py:244-269).
 * Frames past a sample's own length: with attn_mask_enabled and B > 1 the backbone runs on the valid rows only (RowPack), and those
 * frames keep y0's value in `out` / `traj` (the reference integrates them to values nobody reads, cfm.py:160-191); F5_PACK_ROWS=0
 * computes them as the reference does.  With attn_mask_enabled = 0 (every shipped config) all frames match the reference. */
int f5_sample(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y0,
              const int64_t* text, int32_t nt, const float* t_host, int32_t steps, float cfg_strength,
              const int32_t* lens_host, int32_t B, int32_t N, float* out, float* traj, f5_stream stream);

/* Fixed-grid ODE solvers of f5_sample_ode (torchdiffeq's odeint(method=...), cfm.py:42,218). */
#define F5_ODE_EULER 0     /* y += dt * f(t[i], y): 1 backbone evaluation per step */
#define F5_ODE_MIDPOINT 1  /* y_mid = y + f(t[i], y) * dt/2; y += dt * f(t[i] + dt/2, y_mid): 2 evaluations per step (NFE = 2 * steps);
                            * the trajectory holds the grid points only */

/* f5_sample with the solver chosen by `method` (F5_ODE_*); f5_sample is f5_sample_ode(..., F5_ODE_EULER).  An unknown
 * method fails with F5_EINVAL. */
int f5_sample_ode(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y0,
                  const int64_t* text, int32_t nt, const float* t_host, int32_t steps, float cfg_strength,
                  const int32_t* lens_host, int32_t B, int32_t N, float* out, float* traj, f5_stream stream, int32_t method);

/* f5_sample_ode with per-item sampler settings: every utterance of one ragged batch has its own time grid, step count and guidance.
 *   t_items HOST f32[B][steps_max + 1]: item b integrates over t_items[b][0 .. steps_items[b]]; later entries are ignored.
 *   steps_items HOST int32[B], each in [1, steps_max], the largest equal to steps_max.  cfg_items HOST f32[B].
 *   method: F5_ODE_EULER or F5_ODE_MIDPOINT, for the whole batch.  The other arguments are f5_sample_ode's.
 * The batch runs steps_max steps.  For i >= steps_items[b] item b's state is not touched -- the update is skipped, not multiplied by a
 * zero dt -- and trajectory slot i + 1 receives the item's final state: traj f32[steps_max + 1, B, N, mel] or NULL.
 * An item with cfg_items[b] < 1e-5f takes v = p, as cfm.py:167-178 does, for that item alone; if every item is below 1e-5f the
 * backbone runs the conditional half only, as f5_sample_ode does.
 * The values travel in device tables, so a captured graph is keyed on the shape (B, N, nt, steps_max, the number of distinct evaluation
 * times, halves, lens, traj, chunking, method) and serves every guidance and every grid of that shape.  The body is the rectangular one:
 * no RowPack (an attn_mask_enabled engine runs the masked padded form of F5_PACK_ROWS=0), no length bucket, no F5_SPLIT_CFG chains.
 * A uniform call computes, bit for bit, what f5_sample_ode computes on its rectangular body.
 * F5_EINVAL, with a message naming the item: a non-finite t or cfg, steps_items[b] outside [1, steps_max], max(steps_items) != steps_max;
 * and f5_sample_ode's own rules (lens required when B > 1, lens in (0, N], an unknown method). */
int f5_sample_items(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y0,
                    const int64_t* text, int32_t nt, const float* t_items, const int32_t* steps_items, int32_t steps_max,
                    const float* cfg_items, const int32_t* lens_host, int32_t B, int32_t N, float* out, float* traj, f5_stream stream,
                    int32_t method);

/* Some steps of an f5_sample_items solve as a call of their own, so that a batch can be re-formed between two slices: the state stays
 * in device memory, rows that have made their steps leave, new rows join, N follows the rows that are there.
 *   t_items HOST f32[B][count + 1]: the sub-grid of this slice, item b's full grid from the step it is at; steps_items HOST int32[B],
 *   each in [1, count], the largest equal to count: the steps item b makes here.  cfg_items, lens_host, method: f5_sample_items'.
 *   rows_host HOST int32[B]: the row of prev_state f32[prev_B, prev_N, mel] (a previous call's state_out) item b continues from, or
 *   -1 for an item that begins here and takes y_new[b] (y_new f32[B, N, mel]; rows of continuing items are not read).
 *   prev_state may be NULL when every row is -1, y_new when none is.
 * The start state is staged by one launch: y[b, n] = prev_state[rows[b], n] for n < min(N, prev_N), +0.0 for n >= prev_N (frames the
 * previous batch did not have start as the zero padding of y0 does), frames n >= N of the previous state are dropped.  A continuing
 * row keeps every frame it had, pad frames included, so a chain of slices at fixed composition computes bit for bit what the one
 * f5_sample_items call computes.  prev_state is the caller's tensor, never the arena: other engine calls may run between two slices.
 *   state_out f32[B, N, mel]: the raw state after the slice.  out = where(cond_mask, cond, state): meaningful for the items whose
 *   last step was in this slice.
 * The time path runs over the distinct evaluation times of the slice.  The body and its graph key are f5_sample_items' without a
 * trajectory (count in the place of steps_max): the key holds no position in a grid, no guidance and nothing of prev_*, the staging
 * is eager like every input copy, and one captured graph serves every slice of a shape.
 * F5_EINVAL, with a message naming the item, nothing launched and nothing staged: count < 1, steps_items[b] outside [1, count],
 * max(steps_items) != count, rows_host[b] outside [-1, prev_B), a previous row named twice, a row >= 0 with prev_state NULL, a -1
 * with y_new NULL; and f5_sample_items' own rules. */
int f5_sample_span(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y_new,
                   const float* prev_state, int32_t prev_B, int32_t prev_N, const int32_t* rows_host, const int64_t* text, int32_t nt,
                   const float* t_items, const int32_t* steps_items, int32_t count, const float* cfg_items, const int32_t* lens_host,
                   int32_t B, int32_t N, float* out, float* state_out, f5_stream stream, int32_t method);

/* Pre-sizes the activation arena (otherwise it grows on first use, which calls hipMalloc inside f5_sample).  The plan for
 * max_steps covers both solvers: a midpoint call with steps <= max_steps needs no regrowth. */
int f5_reserve(f5_engine* e, int32_t max_batch, int32_t max_frames, int32_t max_steps);

/* --------------------------------------------------------------------------------------- length buckets
 * A serving stream gives f5_sample a different N on almost every call, and a captured HIP graph is keyed on the exact shape: such a
 * stream never replays.  With a length bucket of `granule` frames an eligible call is planned at N_cap = N rounded up to the granule
 * -- arena layout, launch grids and the graph key use N_cap -- while the true N reaches the kernels through the device-side length
 * tables of the packed (RowPack) body and through the copies around it, so one captured graph serves every N of a bucket and every
 * text length.  The frames N .. N_cap-1 are never copied out, and `out` / `traj` are, bit for bit, what the exact path computes.
 *
 * Eligible: the DiT backbone; lens_host NULL or every entry equal to N; F5_SPLIT_CFG off; the profiler off; no
 * F5_OPT_TEXT_AVG_UPSAMPLE; N_cap inside the rotary and text position tables.  Every other call takes the exact path under its
 * exact key, silently.  The unconditional text embedding is computed inside the body on every bucketed call (no per-N cache).
 *
 * granule: 0 = off (the default; F5_LEN_BUCKET=<granule> sets it at f5_create), else a multiple of 8 in [8, 1024]; anything else is
 * F5_EINVAL.  Clears the graph cache. */
int f5_set_length_buckets(f5_engine* e, int32_t granule);
/* Captures and instantiates, without launching anything, one graph per bucket that the lengths n_min .. n_max touch, for f5_sample_ode
 * calls with this B, steps, cfg_strength, method and traj != NULL (want_traj), and any text of at most nt_max tokens; sizes the arena for
 * the largest bucket first.  Afterwards the first eligible call at any N of the range replays.  Calls outside these arguments
 * that grow the arena (a larger B, N, steps or text) drop the prepared graphs, as they drop every graph.  The graph cache holds 16
 * graphs, or as many as one f5_prepare_sample call asked for, 64 at most: a range of more buckets is F5_EINVAL, and so is one whose
 * largest bucket exceeds max_pos.  F5_ESTATE with buckets off, before f5_finalize, with F5_HIP_GRAPH=0 or when no call of this
 * engine can be eligible.  Host work only (allocates); `stream` is not used. */
int f5_prepare_sample(f5_engine* e, int32_t B, int32_t n_min, int32_t n_max, int32_t nt_max, int32_t steps, float cfg_strength,
                      int32_t method, int32_t want_traj, f5_stream stream);
/* ---------------------------------------------------------------------------------------- isolated rows
 * With the shipped configs (attn_mask_enabled = 0) a row of a rectangular batch attends over the batch's padding and has its text
 * embedded at the batch's N, so what f5_sample_items / f5_sample_span compute for an item depends on the items beside it.  With
 * isolated rows on, both run on the packed (RowPack) body with every row's own length in the device tables: the text is embedded per
 * row at lens[b], conv-pos and attention keys are masked at lens[b] whatever attn_mask_enabled says, and everything else is row-wise
 * -- inside its own frames every row is, bit for bit, what the same item gives alone at B = 1, in any batch and any row order.
 * Frames past lens[b] of out / state_out / traj keep their staged value.  lens_host == NULL means every row has N frames.
 *
 * With f5_set_length_buckets on, an isolated call is planned at N_cap = N rounded up to the granule (rows staged at the arena's
 * pitch, frames N .. N_cap-1 of state and mask zero, the text in rows of filler) and at the distinct evaluation times rounded up to
 * a power of two (the rows behind the call's own repeat its last time; no index points at them), so that the graph key
 * "P B|N_cap|steps|U_cap|halves|traj|chunk|method" holds no exact length, text length or time count.  With buckets off the key takes
 * the same form at N rounded up to 4 (the granule of a packed batch row: rows that fill their N would otherwise pack into more
 * rows than B x N), with the exact text length appended.
 *
 * Isolation is a promise: an f5_sample_items / f5_sample_span call that cannot keep it is F5_EINVAL with a message naming the
 * reason and nothing launched -- the UNetT backbone, F5_SPLIT_CFG=1, F5_OPT_TEXT_AVG_UPSAMPLE, or N_cap outside the rotary or text
 * position tables.  F5_PACK_ROWS=0 does not turn it off (that switch is about f5_sample).  f5_sample, f5_sample_ode and
 * f5_prepare_sample are untouched.  on: 0 = off (the default: every key, launch and result as without this function). */
int f5_set_isolated_rows(f5_engine* e, int32_t on);
/* ------------------------------------------------------------------------------------------ graph cache
 * The body of every sampler call (f5_sample, f5_sample_ode, f5_sample_items, f5_sample_span) is cached as a HIP graph under the
 * call's signature: everything the launches depend on and nothing else (tests/graph_cache_oracle.py restates these rules).
 *   - A call takes one of three paths.  The first sighting of a signature launches eagerly and marks it warm; the next sighting
 *     of a warm signature that has no graph captures one and launches it; a signature that has a graph replays it.  The three
 *     results are bit-equal.
 *   - The cache holds `capacity` graphs, 16 by default.  A capture into a full cache pushes out the graph that was captured
 *     first (first in, first out: a replay does not renew an entry).  A signature whose graph was pushed out is still warm, so
 *     its next sighting captures again.
 *   - A clear drops every graph and forgets which signatures were warm: the next sighting of any signature is eager again.  A
 *     clear pushes nothing out: it does not count as an eviction.  These clear: growth of the reserved batch, frames or steps
 *     (f5_reserve, or any call larger than what is reserved; with length buckets a call reserves its bucket's ceiling); a text
 *     longer than any before (f5_prepare_sample's nt_max counts); the first per-item call (f5_sample_items, f5_sample_span) and
 *     every per-item call with more distinct evaluation times than any before; f5_set_length_buckets; f5_load_weight and
 *     f5_finalize.  A call that fits what is reserved clears nothing.
 *   - The unconditional text embedding of a single utterance is kept between calls where it depends on nothing but the weights
 *     and N: B = 1, guidance on (cfg_strength >= 1e-5), lens_host NULL and no length bucket, the DiT or the UNetT, no
 *     text_mask_padding with conv_layers > 0 and no F5_OPT_TEXT_AVG_UPSAMPLE.  One embedding is kept, for the N of the call that
 *     stored it.  Such a call's signature carries whether it reads the kept embedding ("|uc"; every other call's ends in
 *     "|nouc"), and a call that has to compute and store it -- the first at its N, the first after another N -- always launches
 *     eagerly, whatever is warm or captured.  Growth of the reserved batch, frames or steps, a first or larger per-item call,
 *     f5_load_weight and f5_finalize forget the embedding; a longer text alone leaves it, and the call behind that clear is eager
 *     in any case.
 *   - A call returns without waiting for the device, so a graph can be pushed out or cleared while its last launch is still
 *     running: the engine waits for that launch (an event behind it, on the call's stream) before it destroys the graph.  The
 *     host never waits otherwise.
 *
 * f5_set_graph_capacity: the cache holds n graphs, 16 (the default) <= n <= 64; anything else is F5_EINVAL.  For an engine whose
 * calls vary in B as well as in length bucket.  Shrinking below the number held pushes out the oldest captures at once, each an
 * eviction.  f5_set_length_buckets clears the cache and puts the capacity back to 16; f5_prepare_sample only ever raises it, to the
 * number of buckets it was asked for, and evicts like any capture when its range does not fit beside what is held.  A prepared
 * signature counts as seen (warm): when its graph is pushed out, the next call in that bucket captures again. */
int f5_set_graph_capacity(f5_engine* e, int32_t n);
/* out[0..3] = f5_sample bodies captured into a graph (the capturing call launches its graph, and counts here only), replayed from the
 * cache, launched eagerly, and graphs pushed out of the cache by a newer one -- since f5_create or the last reset.  out == NULL
 * resets the four counters.  Reads four integers: no device work. */
int f5_graph_stats(f5_engine* e, int32_t* out);

/* ------------------------------------------------------------------------------------- resident adapters
 * One resident base model, many LoRA fine-tunes of it (train/train_lora.py: low-rank pairs on the attention linears of every
 * DiT block and on input_embed.proj, the text encoder trained in full).  Switching MERGES, as the reference does before it runs
 * (infer/utils_infer.py:198-239): f5_set_adapter rewrites, in place, the packed GEMM operands of the tensors an adapter
 * touches, so a forward costs what it cost before and the captured HIP graphs of f5_sample stay valid (no address moves).
 *
 * Needs F5_OPT_ADAPTERS in f5_config.options (DiT only): f5_finalize then keeps the fp32 masters of every adaptable tensor in
 * engine-owned memory (4 * depth * dim * heads * 64 + dim * (2 * mel_dim + text_dim) + the text encoder, in floats: 0.39 GB at
 * Base size) and builds the device-side descriptor table a switch reads.  Without the bit nothing is kept and
 * f5_adapter_create / f5_set_adapter fail with F5_ESTATE.
 *
 * Adaptable by a low-rank pair (any other name is F5_EINVAL):
 *   transformer_blocks.<i>.attn.{to_q,to_k,to_v,to_out.0}.weight      input_embed.proj.weight
 * Replaceable in full: every tensor whose name starts with "text_embed." (table, ConvNeXt-V2 blocks), at the engine's shapes.
 *
 * The merge arithmetic is fixed, per element and in fp32, without fused multiply-add:
 *   acc = 0;  for r = 0 .. rank-1: acc = acc + B[o][r] * A[r][i]   (product rounded, then added; ascending r)
 *   W'[o][i] = W[o][i] + acc * scale
 * followed by exactly the conversion f5_finalize applies to a plain weight of the engine's precision (rounding to bf16 / f16,
 * zero K padding, the hi / lo split of F5_PREC_F16X3 and of F5_PREC_F16P's input layer).  An engine switched to an adapter
 * therefore holds, bit for bit, the packed weights of a fresh engine loaded with the state dict merged by this rule. */
typedef struct f5_adapter f5_adapter;
/* An empty adapter bound to `e` (finalized, F5_OPT_ADAPTERS).  It stays usable until f5_destroy(e) or the next
 * f5_load_weight / f5_finalize on e (after which every call on it except f5_adapter_destroy fails with F5_ESTATE). */
int f5_adapter_create(f5_engine* e, f5_adapter** out);
/* Fails with F5_ESTATE while the adapter is the engine's active one (set another, or NULL, first). */
int f5_adapter_destroy(f5_adapter* a);
/* One low-rank pair for the weight `name` [out, in]: A f32[rank, in], B f32[out, rank] (device, contiguous), 1 <= rank <= 128,
 * any per-pair rank.  The adapter keeps copies (made on `stream`; allocates and synchronises).  A second put of a name
 * replaces the first.  F5_EINVAL, with a message that names the tensor, for an unknown target, a rank out of range or
 * mismatching shapes; F5_ESTATE while the adapter is active. */
int f5_adapter_put_lora(f5_adapter* a, const char* name, const void* A_dev_f32, const int64_t* a_shape, int32_t a_ndim,
                        const void* B_dev_f32, const int64_t* b_shape, int32_t b_ndim, float scale, f5_stream stream);
/* One full replacement of the tensor `name` (fp32, device, contiguous; the shape must equal the engine's).  Same rules. */
int f5_adapter_put_tensor(f5_adapter* a, const char* name, const void* dev_f32, const int64_t* shape, int32_t ndim,
                          f5_stream stream);
/* Makes `a` (NULL: the base model) the model the engine computes with: rewrites the packed form of every tensor `a` touches and
 * restores from the masters every tensor the previously active adapter touched and `a` does not.  Enqueues one kernel launch per
 * 512 tensors to rewrite on `stream` and nothing else: no allocation, no copy from the host, no synchronisation, no graph
 * invalidation.  The cached unconditional text embedding is dropped.  Calls that follow on the same stream see the new model. */
int f5_set_adapter(f5_engine* e, f5_adapter* a, f5_stream stream);

/* ------------------------------------------------------------------------------------------------ Vocos */
typedef struct f5_vocos_config {
    int32_t input_channels; /* 100 */
    int32_t dim;            /* 512 */
    int32_t intermediate_dim; /* 1536 */
    int32_t num_layers;     /* 8 */
    int32_t n_fft;          /* 1024 */
    int32_t hop_length;     /* 256 */
    int32_t reserved[4];
} f5_vocos_config;

int f5_vocos_create(const f5_vocos_config* cfg, f5_vocos** out);
int f5_vocos_destroy(f5_vocos* v);
/* names: backbone.embed.weight, backbone.convnext.N.{dwconv,norm,pwconv1,pwconv2}.{weight,bias}, ...gamma, head.out.*;
 * aux.hann [n_fft], aux.idft_basis [n_fft, 2*(n_fft/2+1) rounded up to a multiple of 32] (window folded in). */
int f5_vocos_load_weight(f5_vocos* v, const char* name, const void* dev_f32, const int64_t* shape, int32_t ndim,
                         f5_stream stream);
int f5_vocos_finalize(f5_vocos* v, f5_stream stream);
/* mel f32[B, C, T] -> wav f32[B, (T - 1) * hop]   (Vocos.decode: backbone -> ISTFTHead, padding="center") */
int f5_vocos_decode(f5_vocos* v, const float* mel, int32_t B, int32_t T, float* wav, f5_stream stream);
/* The same with mel addressed as mel[b * stride_b + c * stride_c + t * stride_t] (element strides): the callers'
 * `vocoder.decode(generated.permute(0, 2, 1))` (utils_infer.py:702-703) passes a transposed VIEW of sample()'s [B, T, C]
 * output, which is decoded in place instead of through a transposing copy. */
int f5_vocos_decode_strided(f5_vocos* v, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_c,
                            int64_t stride_t, float* wav, f5_stream stream);
/* A ragged batch in one pass: item b is frames [starts_host[b], ends_host[b]) of batch row b (T_b = end - start >= 2), e.g. the
 * generated part of each row of sample()'s output behind its prompt (the reference's batch driver decodes these one by one,
 * eval/eval_infer_batch.py:202-212).  The items run as sum(T_b) packed rows; each is convolved, overlap-added and trimmed
 * inside its own window, and frames outside it are never read, so item b's waveform is bit-identical to
 * f5_vocos_decode_strided on that slice alone with B = 1.
 *   wav[b * wav_stride + j], j < (T_b - 1) * hop : the waveform, times gain_host[b] where gains are given (one f32 multiply)
 *   (T_b - 1) * hop <= j < wav_stride            : 0.0f
 * wav_stride >= max_b (T_b - 1) * hop.  F5_EINVAL, with nothing launched, for T_b < 2 (the message names the item), a
 * negative start, too small a wav_stride, B <= 0 or a null mel / ends_host / wav.  The host tables are copied before the
 * call returns.  No synchronisation except when the workspace grows. */
int f5_vocos_decode_ragged(f5_vocos* v, const float* mel, int32_t B, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                           const int32_t* starts_host /* NULL: all 0 */, const int32_t* ends_host,
                           const float* gain_host /* NULL: 1 */, float* wav, int64_t wav_stride, f5_stream stream);

/* ------------------------------------------------------------------------------------- cross-fade concatenation
 * The last stage of infer_batch_process (infer/utils_infer.py:734-775): the pieces of one long text, cross-faded into one
 * waveform.  Piece i is wav[i * wav_stride + j], j < lens_host[i] (f32, device); nothing past lens_host[i] in a row is read.
 * The result is the reference's left fold over the pieces.  Host plan, in exact integers:
 *   L_0 = len_0;  for i >= 1: n_i = min(cross_fade_samples, L_{i-1}, len_i) (0 when cross_fade_samples <= 0),
 *   off_i = L_{i-1} - n_i,  L_i = off_i + len_i;  total = L_{B-1}.
 * Output sample p is a fold, in double, over the pieces that cover it (j = p - off_i, 0 <= j < len_i), in ascending i:
 *   i > 0 and j < n_i:  v = v * fo + (double)x_i[j] * fi        otherwise:  v = (double)x_i[j];      out[p] = (float)v
 * with numpy's linspace weights fi = j * step_i + 0.0, fo = j * (-step_i) + 1.0, step_i = 1.0 / (n_i - 1) computed on the host,
 * the last fade element exactly fi = 1, fo = 0, and fo = 1, fi = 0 for n_i == 1.  Multiplies and adds are separate IEEE double
 * operations, so out is, bit for bit, numpy's float64 result cast to float32 -- also where pieces shorter than the fade put
 * more than two pieces over one sample.
 * out[0, total) is written, each sample by one thread (deterministic); nothing at or past total is.  *out_len_host (may be NULL)
 * receives total.  One kernel launch that takes the per-piece table as its argument: no allocation, no copy, no synchronisation,
 * capturable; lens_host is free when the call returns.  That bounds B: 1 <= B <= 64.  F5_EINVAL, with nothing launched and a
 * message naming the argument, for B out of range, a null wav / lens_host / out, a lens_host[i] < 1, wav_stride below the
 * longest piece or out_cap < total. */
int f5_wave_crossfade(const float* wav, int32_t B, int64_t wav_stride, const int32_t* lens_host, int32_t cross_fade_samples,
                      float* out, int64_t out_cap, int64_t* out_len_host, f5_stream stream);

/* f5_wave_join: pieces joined into one waveform with a fade request per piece -- the multi-voice script of infer/infer_cli.py:363-415,
 * where the chunks of one tagged stretch are cross-faded (infer/utils_infer.py:734-775) and the stretches are concatenated.
 * Piece i is base[start_host[i] + j], j < lens_host[i] (f32, device): the pieces may lie in any order and in several tensors under
 * one base pointer (f5_wave_gather's placement).  fade_host[i] >= 0 is the cross-fade requested, in samples, into what stands in
 * front of piece i.  Host plan, in exact integers; R is the length of the current run:
 *   piece 0, and every piece with fade_host[i] == 0, opens a run:  n_i = 0,  off_i = L_{i-1} (0 for i = 0),  R = len_i;
 *   otherwise:  n_i = min(fade_host[i], R, len_i),  off_i = L_{i-1} - n_i,  R = R - n_i + len_i;
 *   in both cases L_i = off_i + len_i;  total = L_{B-1}.
 * R restarts with every run, so a run is the reference's left fold over that run alone (its len(final) is the stretch's length,
 * not the script's).  Output sample p is a fold, in double, over the pieces that cover it (j = p - off_i, 0 <= j < len_i), in
 * ascending i:
 *   j < n_i:  v = v * fo + (double)x_i[j] * fi        otherwise:  v = (double)x_i[j];      out[p] = (float)v
 * with numpy's linspace weights fi = j * step_i + 0.0, fo = j * (-step_i) + 1.0, step_i = 1.0 / (n_i - 1) computed on the host,
 * the last fade element exactly fi = 1, fo = 0, and fo = 1, fi = 0 for n_i == 1.  Multiplies and adds are separate IEEE double
 * operations and the result is rounded to f32 once, so out is, bit for bit, the concatenation of numpy's float64 fold of every
 * run, cast to float32 -- also where pieces shorter than the fade put more than two pieces over one sample.
 * out[0, total) is written, each sample by one thread (deterministic), with 16-byte stores where the address allows (the same
 * bits either way); nothing at or past total is written and nothing outside [0, len_i) of a piece is read.  *out_len_host (may
 * be NULL) receives total.  L_i never decreases (L_i - L_{i-1} = len_i - n_i >= 0) while off_i may (a short piece in front of a
 * long fade), so a tile of the output finds its first piece by bisection over L and walks up while the minimum of off over the
 * pieces still to come lies inside it: no tile loops over all pieces.  1 <= B <= 65535.
 * The table goes through a pinned slot of the per-device ring into the workspace of the handle-less calls: ONE launch and one small
 * host-to-device copy on `stream`, no synchronisation except when that workspace grows, every host array free when the call
 * returns; not capturable into a graph.  F5_EINVAL, with nothing launched or staged and a message that starts with "f5_wave_join:"
 * and names the argument or the piece: a null base / start_host / lens_host / fade_host / out, B out of range, a lens_host[i] < 1,
 * a fade_host[i] < 0, a start_host[i] < 0, out_cap < total. */
int f5_wave_join(const float* base, int32_t B, const int64_t* start_host, const int32_t* lens_host, const int32_t* fade_host,
                 float* out, int64_t out_cap, int64_t* out_len_host, f5_stream stream);

/* --------------------------------------------------------------------------------------------- speech editing
 * The data movement around CFM.sample(edit_mask=...) for a batch of recordings (infer/speech_edit.py).  A recording's edited
 * timeline is a list of segments (dst, src, frames) in mel frames, three int32 each, ascending and disjoint in dst:
 *   KEEP  src >= 0: frames [dst, dst + frames) of the result are frames [src, src + frames) of the original;
 *   EDIT  src = -1: frames [dst, dst + frames) are zero frames that sample() fills in.
 * Both calls read the tables of all items from host arrays (seg_count_host[b] segments for item b, packed one item after the other
 * in segs_host), check them, and stage them for the kernel in a pinned slot of a per-device ring: ONE launch and one small
 * host-to-device copy on `stream`, no synchronisation (a slot is waited for only when the call eight calls ago has not run yet),
 * every host array free when the call returns; not capturable into a graph.  At most 64 items of at most 33 segments.
 * F5_EINVAL, with nothing launched or staged and a message that starts with the function's name: a null pointer, B outside 1..64,
 * a segment with frames < 1, with dst inside or before the segment in front of it, with a source range that leaves [0, T_b)
 * (f5_wave_splice: src < 0), or with a destination range that leaves [0, D_b), D_b <= D_max (f5_wave_splice clips instead, below).
 *
 * f5_edit_assemble: cond f32 [B, D_max, row] (contiguous) from the packed original mels, item b at mel + b * mel_stride with
 * frames_host[b] = T_b rows of `row` elements (T_b * row <= mel_stride).  Every output frame d of item b is
 *   a bit copy of source frame src + (d - dst) where a KEEP segment covers d,  +0.0 in every element otherwise
 * (an EDIT segment, a frame no segment covers, a frame at or behind dur_host[b] = D_b).  16-byte loads and stores when row and
 * mel_stride are multiples of 4 and both bases are 16-byte aligned, element-wise otherwise; the same bits either way. */
int f5_edit_assemble(const float* mel, int32_t B, int64_t mel_stride, int32_t row, const int32_t* frames_host,
                     const int32_t* seg_count_host, const int32_t* segs_host, const int32_t* dur_host, float* cond, int32_t D_max,
                     f5_stream stream);

/* f5_wave_splice: out row b (out + b * out_stride, out_stride samples, all written) from the decoded waveform g = gen + b * gen_stride
 * (L = len_host[b] samples, L <= gen_stride and L <= out_stride), the prepared original a = a_base + a_start_host[b]
 * (n = a_len_host[b] samples at the model's rate) and the item's KEEP segments only.  Contract, in exact integers:
 *   a KEEP segment (dst, src, frames) claims out[p0, p1):  p0 = dst * hop,  p1 = min((dst + frames) * hop, L, p0 + n - src * hop);
 *   the source sample of p is q = src * hop + (p - p0); a segment with p1 <= p0 is dropped;
 *   m = min(cross_fade_samples, (p1 - p0) / 2) (integer division); the head fades in over its first m samples if p0 > 0, the tail
 *   fades out over its last m samples if p1 < L; at a fading position j = p - p0 (head) or j = p1 - 1 - p (tail)
 *       out[p] = (float)((double)g[p] * fo + (double)a[q] * fi)
 *   with f5_wave_crossfade's restatement of linspace(0, 1, m) and linspace(1, 0, m): m == 1: fi = 0, fo = 1; j == m - 1: fi = 1,
 *   fo = 0; otherwise fi = j * step + 0.0, fo = j * (-step) + 1.0, step = 1.0 / (m - 1) computed on the host; multiplies and
 *   adds are separate IEEE double operations;
 *   every other claimed sample is a[q] bit for bit, every unclaimed sample of [0, L) is g[p] bit for bit, every sample of the row
 *   at or behind L is +0.0.
 * Nothing outside [0, L) of g or [0, n) of a is read.  Each sample is written by one thread (deterministic); a 16-byte store where
 * the address allows, else per element.  1 <= hop <= 65536, cross_fade_samples >= 0. */
int f5_wave_splice(const float* gen, int32_t B, int64_t gen_stride, const int32_t* len_host, const float* a_base,
                   const int64_t* a_start_host, const int32_t* a_len_host, const int32_t* seg_count_host, const int32_t* segs_host,
                   int32_t hop, int32_t cross_fade_samples, float* out, int64_t out_stride, f5_stream stream);

/* ---------------------------------------------------------------------------------------------- BigVGAN
 * The vocoder of mel_spec_type="bigvgan" (infer/utils_infer.py:138-152: bigvgan.BigVGAN.from_pretrained(
 * "nvidia/bigvgan_v2_24khz_100band_256x"), remove_weight_norm(); called as vocoder(mel[B, 100, T]) -> wav[B, 1, 256 T]
 * at :705).  The reference takes it from an un-vendored submodule: the architecture is restated from the published
 * BigVGAN v2 (see csrc/bigvgan.hip; checker: tests/test_bigvgan.py) -- parity unpinned. */
typedef struct f5_bigvgan f5_bigvgan;
typedef struct f5_bigvgan_config {
    int32_t num_mels;                 /* 100 */
    int32_t upsample_initial_channel; /* 1536; halves at every upsample stage */
    int32_t num_upsamples;            /* 6 */
    int32_t upsample_rates[8];        /* 4, 4, 2, 2, 2, 2 */
    int32_t upsample_kernel_sizes[8]; /* 8, 8, 4, 4, 4, 4 */
    int32_t num_kernels;              /* 3 AMP blocks per stage ... */
    int32_t resblock_kernel_sizes[4]; /* ... with kernels 3, 7, 11 */
    int32_t num_dilations;            /* 3 (conv, conv) pairs per AMP block ... */
    int32_t resblock_dilations[4];    /* ... with dilations 1, 3, 5 on the first conv of each pair */
    int32_t use_tanh_at_final;        /* 0: clamp(-1, 1) */
    int32_t use_bias_at_final;        /* 0 */
    int32_t precision;                /* F5_PREC_F32 (0) or F5_PREC_F16X3: the wide stages' convolutions as split-f16 products */
    int32_t reserved[3];
} f5_bigvgan_config;
int f5_bigvgan_create(const f5_bigvgan_config* cfg, f5_bigvgan** out);
int f5_bigvgan_destroy(f5_bigvgan* v);
/* names (after remove_weight_norm): conv_pre.{weight,bias}, ups.N.0.{weight,bias}, resblocks.N.convs1.M.{weight,bias},
 * resblocks.N.convs2.M.{weight,bias}, resblocks.N.activations.A.act.{alpha,beta}, activation_post.act.{alpha,beta},
 * conv_post.weight (+ .bias); host-computed aux.up_filter / aux.down_filter [12] (kaiser-sinc filters of Activation1d). */
int f5_bigvgan_load_weight(f5_bigvgan* v, const char* name, const void* dev_f32, const int64_t* shape, int32_t ndim,
                           f5_stream stream);
int f5_bigvgan_finalize(f5_bigvgan* v, f5_stream stream);
/* mel addressed as mel[b * stride_b + c * stride_c + t * stride_t] (element strides) -> wav f32[B, T * prod(rates)] */
int f5_bigvgan_forward(f5_bigvgan* v, const float* mel, int32_t B, int32_t T, int64_t stride_b, int64_t stride_c,
                       int64_t stride_t, float* wav, f5_stream stream);
/* A ragged batch in ONE pass (the contract of f5_vocos_decode_ragged): item b is frames [starts_host[b], ends_host[b]) of batch
 * row b of mel, T_b = end - start >= 1.  wav[b * wav_stride + i], i < T_b * prod(rates), is bit-identical to f5_bigvgan_forward on
 * that slice alone (B = 1) in both precisions, times gain_host[b] as a separate f32 multiply (x 1.0f without gains); +0.0 fills
 * the row up to wav_stride.  Frames outside an item's window and other items' frames are never read.  The items share one packed
 * time axis (f5_bigvgan_ragged_plan).  The host tables go down in one copy through a pinned slot and are free when
 * the call returns; no synchronisation except when the workspace grows.  F5_EINVAL with nothing launched, the message naming the
 * item: T_b < 1, start < 0, wav_stride below the longest waveform, B <= 0 or B > 65535 (the grid's y range), a null mel / ends_host /
 * wav, more than 2^24 packed rows at the last stage (the GEMMs index rows as int).  F5_ESTATE before finalize. */
int f5_bigvgan_forward_ragged(f5_bigvgan* v, const float* mel, int32_t B, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                              const int32_t* starts_host /* NULL: all 0 */, const int32_t* ends_host,
                              const float* gain_host /* NULL: 1 */, float* wav, int64_t wav_stride, f5_stream stream);
/* The packed axis of that call, pure host arithmetic (no HIP call): item b of frames_host[b] >= 1 frames starts at frame
 * row_start_out[b] (B + 1 entries; [B] = the packed frame count) and is followed by at least *gap_frames_out dead frames, where
 * gap * rates[0] >= the widest resblock convolution's reach max (k - 1) / 2 * d; starts are rounded up so that an item's first row
 * at every stage is a multiple of 8 (the activation kernel's tile).  F5_EINVAL as above (null pointer, B, T_b < 1, 2^24 rows). */
int f5_bigvgan_ragged_plan(const f5_bigvgan_config* cfg, int32_t B, const int32_t* frames_host, int32_t* row_start_out,
                           int32_t* gap_frames_out);

/* ------------------------------------------------------------------------------------- prompt mel front-end
 * MelSpec.forward, mel_spec_type="vocos" (model/modules.py:78-146): wav f32[B, nw] -> log-mel f32[B, T, n_mels],
 * T = nw / hop + 1.  Constant tables are host-computed and loaded once:
 *   aux.dft_basis f32[round_up(2*(n_fft/2+1), 4), n_fft]  rows w*cos(2 pi f j / n_fft) for f <= n_fft/2, then w*sin(..)
 *   aux.mel_fb    f32[n_mels, round_up(n_fft/2+1, 32)]    HTK mel filterbank, norm=None (torchaudio melscale_fbanks)   */
typedef struct f5_mel f5_mel;
int f5_mel_create(int32_t n_fft, int32_t hop_length, int32_t n_mels, f5_mel** out);
int f5_mel_destroy(f5_mel* m);
int f5_mel_load(f5_mel* m, const char* name, const void* dev_f32, const int64_t* shape, int32_t ndim, f5_stream stream);
int f5_mel_forward(f5_mel* m, const float* wav, int32_t B, int32_t nw, float* out, f5_stream stream);
/* General form (mel_spec_type="bigvgan", model/modules.py:33-75: pad = (n_fft - hop) / 2, center=False, mag_eps = 1e-9,
 * aux.mel_fb = librosa's slaney filterbank): reflect padding `pad` on both sides, T = (nw + 2 pad - n_fft) / hop + 1 frames,
 * |S| = sqrt(re^2 + im^2 + mag_eps).  f5_mel_forward is pad = n_fft / 2, mag_eps = 0. */
int f5_mel_forward_ex(f5_mel* m, const float* wav, int32_t B, int32_t nw, int32_t pad, float mag_eps, float* out,
                      f5_stream stream);
/* Ragged form (the prompts of eval/utils_eval.py:109-148, padded_mel_batch): B prompts of unequal length in ONE pass -- one
 * reflect-pad launch, one DFT GEMM, one magnitude launch and one mel GEMM over the packed rows of every item, one unpack launch.
 * Item b is wav[wav_start_host[b] .. wav_start_host[b] + nw_host[b]) and has T_b = (nw_b + 2 pad - n_fft) / hop + 1 frames;
 * out[b * out_stride_b + t * n_mels + c] holds its log-mel for t < T_b, bit for bit what f5_mel_forward_ex(B = 1) gives for that
 * item alone, and +0.0 for T_b <= t < T_out (F.pad(..., value=0)); nothing at or past b * out_stride_b + T_out * n_mels is written,
 * nothing outside an item's samples is read.  pad and mag_eps as in f5_mel_forward_ex.  The host tables are free when the call
 * returns (they go down in one copy through a pinned slot); no synchronisation and no allocation except the growth of the
 * handle's workspace.
 * f5_mel_ragged_plan is the row layout as pure host arithmetic (no HIP call): item b's padded signal of P_b = nw_b + 2 pad samples
 * starts at sample row_start[b] * hop of one packed buffer and owns ceil(P_b / hop) rows (the first T_b are its frames, the rest
 * are dead rows); row_start_out has B + 1 entries (the last is the row count R), frames_out[b] = T_b.
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the item: a null pointer, B <= 0, pad < 0,
 * wav_start_b < 0, an item with nw_b <= pad or nw_b + 2 pad < n_fft, T_out < max T_b, out_stride_b < T_out * n_mels, R > 2^24.
 * F5_ESTATE when the tables are not loaded. */
int f5_mel_ragged_plan(int32_t n_fft, int32_t hop, int32_t pad, int32_t B, const int32_t* nw_host, int32_t* row_start_out,
                       int32_t* frames_out);
int f5_mel_forward_ragged(f5_mel* m, const float* wav, int32_t B, const int64_t* wav_start_host, const int32_t* nw_host, int32_t pad,
                          float mag_eps, float* out, int64_t out_stride_b, int32_t T_out, f5_stream stream);

/* ------------------------------------------------------------------------------------- prompt preparation
 * What both drivers do to a prompt before its mel (infer/utils_infer.py:523-533, eval/utils_eval.py:111-118: mono mix, RMS, the
 * gain up to target_rms, torchaudio Resample to the model's rate) for B prompts of any channel count, length and rate in ONE pass:
 * a partial-sum launch, a finishing launch and a resample launch, one table copy, no host read.  Item b has C_b channels of n_b
 * samples at sr_b Hz, laid out [C_b, n_b] row-major from base[start_host[b]].  The arithmetic contract, per item:
 *   1. mono    m[j] = (x[0][j] + x[1][j] + ... in ascending channel order, f32) / C_b; the sample itself for C_b = 1
 *              (bit for bit torch.mean(audio, dim=0) for C_b = 2, and for C_b = 3 on every one of 10^6 random triples)
 *   2. rms     S = sum_j (double)m[j] * (double)m[j] in f64, in a fixed order: tiles of 2048 samples, inside a tile each of 256
 *              threads adds its samples j = t, t + 256, ... and a fixed tree adds the threads; the tiles' sums are added in
 *              ascending tile order by one thread.  No floating atomics: the value depends on the item alone.
 *              rms_b = (float)sqrt(S / n_b) -> rms_out[b]
 *   3. level   v[j] = (m[j] * target_rms) / rms_b where rms_b < target_rms (two f32 operations, as `audio * target_rms / rms`
 *              evaluates), else v = m; decided on the device.  An all-zero prompt gives NaN, as those operations do.
 *   4. resample (sr_b != target_sr)  g = gcd(sr_b, target_sr), orig = sr_b / g, new = target_sr / g,
 *              width = ceil(6 * orig / (0.99 * min(orig, new))) evaluated in double, K = 2 width + orig taps:
 *              y[i * new + p] = sum_k bank[p][k] * vpad[i * orig + k], k ascending from an accumulator of +0.0, every step an f32
 *              multiply then an f32 add (no fused multiply-add); vpad is v behind `width` zeros and in front of zeros, the zeros
 *              made by index logic.  L_b = ceil(new * n_b / orig) samples.  sr_b == target_sr: y = v, L_b = n_b.
 * bank is the f32 cast of the float64 windowed-sinc kernel of torchaudio's Resample defaults (sinc_interp_hann, lowpass_filter_width 6,
 * rolloff 0.99), computed by the caller on the host and handed over once per rate pair with f5_mel_resample_bank as f32[new, K]
 * (row p = phase p); the handle keeps a device copy laid out [K, new] per (orig, new) until it is destroyed.  A pair that is
 * already there is left alone (nothing is copied); *uploads_out of f5_mel_resample_bank_count counts the copies made so far.
 * f5_mel_resample_bank synchronises (a copy from pageable memory, once per pair).
 * f5_mel_prepare_plan is the packing as pure host arithmetic (no HIP call): len_out[b] = L_b, start_out[b] = the element of the
 * packed output where item b starts (each rounded up to a multiple of 4), *total_out = the elements the packed output needs.
 * f5_mel_prepare_ragged writes out[start_b .. start_b + L_b) for every item and rms_out[0 .. B); nothing else of out is written,
 * nothing outside an item's C_b * n_b samples is read.  The host tables are free when the call returns (one copy through a
 * pinned slot); no synchronisation and no allocation except the growth of the handle's workspace.
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the item: a null pointer, B < 1 or B > 65535,
 * target_sr < 1, target_rms <= 0 (or NaN), start_b < 0, channels_b < 1, n_b < 1, sr_b < 1, a rate pair whose bank new * K exceeds 2^20
 * elements (e.g. 24001 Hz), more than 2^30 tiles of work in one call, out_capacity below the plan's total, a bank of the
 * wrong size.  F5_ESTATE: an item's rate pair has no bank yet. */
int f5_mel_prepare_plan(int32_t B, const int32_t* n_host, const int32_t* sr_host, int32_t target_sr, int64_t* len_out,
                        int64_t* start_out, int64_t* total_out);
int f5_mel_resample_bank(f5_mel* m, int32_t sr, int32_t target_sr, const float* bank_host, int64_t numel, f5_stream stream);
int f5_mel_resample_bank_count(f5_mel* m, int32_t* uploads_out);
int f5_mel_prepare_ragged(f5_mel* m, const float* base, int32_t B, const int64_t* start_host, const int32_t* channels_host,
                          const int32_t* n_host, const int32_t* sr_host, int32_t target_sr, float target_rms, float* out,
                          int64_t out_capacity, float* rms_out, f5_stream stream);

/* ------------------------------------------------------------------------------------- delivery at the client's rate
 * What stands between generated audio and a client (the reference's clients and eval/utils_eval.py:403-411 resample every generated
 * file; a socket wants PCM16): a ragged batch of B <= 65535 streams of 24 kHz f32 audio, each read where it lies, resampled to
 * out_rate and stored as f32 or 16-bit PCM in ONE launch.  Item b has n_b >= 0 samples from base[start_host[b]]; final_host[b] != 0
 * says that the stream ends there, 0 that more samples will follow.  The arithmetic contract, per item:
 *   geometry   g = gcd(24000, out_rate), orig = 24000 / g, new = out_rate / g, width = ceil(6 * orig / (0.99 * min(orig, new))) in
 *              double, K = 2 width + orig (step 4 of f5_mel_prepare_ragged).
 *   resample   y[i * new + p] = sum_k bank[p][k] * xpad[i * orig + k]: step 4 of f5_mel_prepare_ragged verbatim -- k ascending from
 *              +0.0, an f32 multiply then an f32 add per tap, no fused multiply-add, bank the handle's (24000 -> out_rate) pair from
 *              f5_mel_resample_bank.  xpad is the stream behind `width` zeros, and in front of zeros where it is final; the zeros are
 *              index logic.  y[i * new + p] depends on the samples [i * orig - width, i * orig + width + orig - 1] alone.
 *              out_rate == 24000: y = x.
 *   lengths    len = ceil(new * n / orig) samples in all.  ready = the leading outputs whose taps are all there: len for a final
 *              stream, else min(new * max(0, floor((n - width - orig) / orig) + 1), len).  An output below `ready` never changes as
 *              the stream grows, so a stream delivered range by range is the finished stream delivered at once.
 *   format     F5_PCM_F32 stores y.  F5_PCM_S16 stores the 16-bit view of generated audio (the silence stage's, qscale 32767):
 *              t = y * 32767.f in f32; NaN gives 0, t <= -32768 gives -32768, t >= 32767 gives 32767, else (int)rintf(t) (ties to even).
 *   output     the range [o0_b, o1_b) of y, 0 <= o0_b <= o1_b <= ready_b, goes to out elements [at_b, at_b + o1_b - o0_b), where at_b is
 *              the running total rounded up to 16 bytes (4 f32 or 8 s16 elements): out_start_out[b] = at_b.  out_capacity counts
 *              elements of the format.  Nothing else of out is written, nothing outside [0, n_b) of an item is read; each sample is
 *              written by one thread, no atomics.  An empty range writes nothing.
 * f5_wave_deliver_plan is len and ready for one stream as pure host arithmetic (no HIP call).
 * The host tables are free when f5_wave_deliver returns (one copy through a pinned slot of the handle); no synchronisation and no
 * allocation except the growth of the handle's workspace.  Calls on one handle are ordered by the caller's stream.
 * F5_EINVAL, with nothing launched or staged and a message that starts with the function's name: a null pointer, B < 1 or
 * B > 65535, out_rate outside [8000, 192000], a rate whose bank new * K exceeds 2^20 elements (8001 Hz is one), start_b < 0, n_b < 0,
 * a range outside [0, ready_b], an unknown format, out_capacity below the plan's total.  F5_ESTATE: the pair has no bank yet. */
#define F5_PCM_F32 0
#define F5_PCM_S16 1
int f5_wave_deliver_plan(int32_t out_rate, int64_t n, int32_t final, int64_t* len_out, int64_t* ready_out);
int f5_wave_deliver(f5_mel* m, const float* base, int32_t B, const int64_t* start_host, const int32_t* n_host,
                    const int32_t* final_host, const int64_t* o0_host, const int64_t* o1_host, int32_t out_rate, int32_t format,
                    void* out, int64_t out_capacity, int64_t* out_start_out, f5_stream stream);

/* ------------------------------------------------------------------------------------- join and delivery for many streams
 * What one tick of a server with many clients needs: for each of S <= 65535 streams, the pieces it has so far joined as
 * f5_wave_join joins them, and of that joined stream a range delivered as f5_wave_deliver delivers it, each stream at its own rate
 * and in its own format -- in ONE launch, without the joined stream or any per-rate buffer ever being written.  Stream s has
 * piece_count_host[s] >= 1 pieces; start_host / lens_host / fade_host hold the pieces of all streams, stream after stream (at most
 * 65535 in all), each as f5_wave_join takes it: base[start + j], j < len, f32 on the device, read where it lies.  Per stream:
 *   joined    J_s is what f5_wave_join defines for the stream's pieces alone (its first piece, and every piece with a fade of 0,
 *             opens a run; R restarts with every run): per sample the fold in double over the covering pieces in ascending order,
 *             rounded to f32 once.  total_s is its length.
 *   settled   n = settled_host[s], 0 <= n <= total_s (and below 2^31): the stream that is delivered is J_s[0, n).  final_host[s] != 0
 *             says that it ends there.  A caller whose later pieces fade over at most f samples passes total_s - f while the stream
 *             grows: no later piece reaches further back.
 *   delivery  exactly f5_wave_deliver's for an item of n samples at rate_host[s] in format_host[s] (F5_PCM_F32 / F5_PCM_S16):
 *             geometry, taps in ascending order from +0.0 with an f32 multiply then an f32 add, lengths and ready, the 16-bit view;
 *             the range [o0_host[s], o1_host[s]) lies inside [0, ready_s].  The banks are the handle's (f5_mel_resample_bank), one
 *             per rate that occurs.
 *   output    the stream's bytes go to out + out_start_bytes_out[s], the running byte total rounded up to 16; out_capacity_bytes
 *             counts bytes.  Nothing else of out is written, nothing outside a piece is read; each sample is written by one
 *             thread, no atomics.  An empty range writes nothing.
 * The bytes of stream s are, bit for bit, what f5_wave_deliver gives on the first n samples of f5_wave_join's result for the same
 * pieces -- alone or in any batch, whatever the other streams are.  A block stages its window by folding it from the pieces
 * (bisection to the first piece that reaches into it) where f5_wave_deliver loads it.
 * ONE launch and one table copy through a pinned slot of the handle on `stream`, every host array free when the call returns; no
 * synchronisation and no allocation except the growth of the handle's workspace.  Calls on one handle are ordered by the caller's
 * stream.  F5_EINVAL, with nothing launched or staged and a message that starts with "f5_wave_emit:" and names the argument, the
 * stream or the piece: every refusal of the two calls it composes (a null pointer, S out of range, a length < 1, a fade < 0, a
 * start < 0, a rate outside [8000, 192000] or with a bank above 2^20 elements, an unknown format, a range outside [0, ready_s]), a
 * piece_count < 1, more than 65535 pieces, settled outside [0, total_s], out_capacity_bytes below the plan's total.  F5_ESTATE: a
 * rate has no bank yet. */
int f5_wave_emit(f5_mel* m, const float* base, int32_t S, const int32_t* piece_count_host, const int64_t* start_host,
                 const int32_t* lens_host, const int32_t* fade_host, const int64_t* settled_host, const int32_t* final_host,
                 const int64_t* o0_host, const int64_t* o1_host, const int32_t* rate_host, const int32_t* format_host, void* out,
                 int64_t out_capacity_bytes, int64_t* out_start_bytes_out, f5_stream stream);

/* ------------------------------------------------------------------------------------- silence clipping
 * What the reference drivers do to every prompt before anything else sees it (infer/utils_infer.py:348-361, 385-419: cut at pauses
 * to at most 12 s, trim the silent edges, append 50 ms of silence) and, on request, to the result (:784-793, remove_silence), both
 * through pydub on 16-bit samples.  The decisions are restated here as exact integer arithmetic; the range logic on top of the
 * flags is host arithmetic (silence.py).  Item b has C channels of F frames at R Hz, laid out [C, F] row-major from
 * base[start_host[b]], f32 (the layout of f5_mel_prepare_ragged).  The arithmetic contract:
 *   16-bit view   q = clamp((int)rintf(x * qscale), -32768, 32767): an f32 multiply, round to nearest even; NaN gives 0.
 *                 qscale = 32768 for prompts (the inverse of how a 16-bit file is loaded: exact for such files), 32767 for generated
 *                 waves (libsndfile's float -> PCM_16 rule).
 *   grid          pos(ms) = (R * ms) / 1000 in integers.  L = round(1000 * (F / R)) with Python's round on that double expression,
 *                 computed by the caller (len_ms_host).  The analysis sees frames [0, pos(L)); frames at or past F read as 0 (pydub
 *                 pads a slice's missing frames with silence); frames at or past pos(L) are never read.
 *   energy        E(a, b) = sum of q^2 over all channels and frames [pos(a), pos(b)), in int64 (exact);
 *                 cnt(a, b) = C * (pos(b) - pos(a)).  A window is silent at the integer threshold T iff E(a, b) < cnt(a, b) * (T + 1)^2,
 *                 which is audioop.rms(window) <= T (rms 0 included).  T comes from the caller: floor(10^(dB / 20) * 32768) for
 *                 detect_silence (-50 dB: 103, -40 dB: 327), the largest r with 20 * log10(r / 32768) < dB for the edge trim (-42 dB: 260).
 *   query         (W, s, T, kind), W and s in ms, four int32 each in queries_host.  kind 0 (detect_silence): no start if L < W, else
 *                 the starts 0, s, 2 s, ... <= L - W, and L - W itself behind them if (L - W) % s != 0; the window is [a, a + W).
 *                 kind 1 (chunk grid): the starts 0, s, ... < L, the window [a, min(a + W, L)) (W = s = 10: detect_leading_silence;
 *                 W = s = 1: the per-millisecond loop of remove_silence_edges).  One byte per start: 1 = silent.
 *   segments      (dst, src, frames) triples in frames, ascending and disjoint in dst: frames [dst, dst + frames) of the signal are
 *                 frames [src, src + frames) of the item; a source frame at or past F reads as 0, and so does every frame of the
 *                 signal that no segment covers.
 *   gather        out frame j of channel c = (float)q / 32768.0f of its source frame, +0.0 where that is at or past F or where no
 *                 segment covers j; item b's output is [C, F_out] row-major from out[out_start_host[b]].  Nothing outside
 *                 [0, C * F_out) of an item is written; one thread writes each sample.
 * f5_silence_plan is the flag layout as pure host arithmetic (no HIP call): count_out[b * nq + k] flags of item b and query k start
 * at start_out[b * nq + k] of the packed flag buffer, *total_out flags in all.
 * f5_silence_analyse writes exactly those flags for a ragged batch: per-millisecond energies (the only launch that reads the
 * audio), the exclusive prefix per item as a plain three-phase scan (tile sums inside the energy launch, a scan of the tile sums,
 * an apply launch), and one flag launch for every query: four launches, one table copy through a pinned slot, no host read and no
 * synchronisation except the growth of the per-device workspace.  No atomics: integer sums are exact in any order, so an item's
 * flags are the same alone and in a batch.  seg_count_host != NULL: item b is read through its seg_count_host[b] segments (segs_host
 * holds every item's triples one after the other) -- the signal is then the concatenation the table describes, not materialised.
 * f5_wave_gather is the gather for the batch in one launch (16-byte stores where the destination is aligned).
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the item: a null pointer, B < 1 or B > 65535,
 * nq < 1 or nq > 8, W or s outside [1, 2^24], T outside [0, 32767], kind not 0 or 1, L < 0 or L > 2^24, start_b < 0, C < 1, F < 1,
 * C * F >= 2^31, R < 11025 or R > 384000 (below 11025 Hz pydub would resample the prompt up to its silent segments' rate: not
 * built), qscale outside (0, 32768], more than 2^30 milliseconds in one call, a segment with frames < 1, src < 0, a dst inside or
 * before the segment in front of it or (gather) an end past F_out, F_out < 0, an output range outside out_capacity,
 * flags_capacity below the plan's total. */
int f5_silence_plan(int32_t B, const int32_t* len_ms_host, int32_t nq, const int32_t* queries_host, int32_t* count_out,
                    int64_t* start_out, int64_t* total_out);
int f5_silence_analyse(const float* base, int32_t B, const int64_t* start_host, const int32_t* channels_host,
                       const int32_t* frames_host, const int32_t* rate_host, const int32_t* len_ms_host, float qscale, int32_t nq,
                       const int32_t* queries_host, const int32_t* seg_count_host, const int32_t* segs_host, uint8_t* flags,
                       int64_t flags_capacity, f5_stream stream);
int f5_wave_gather(const float* base, int32_t B, const int64_t* start_host, const int32_t* channels_host, const int32_t* frames_host,
                   float qscale, const int32_t* seg_count_host, const int32_t* segs_host, const int32_t* out_frames_host,
                   const int64_t* out_start_host, float* out, int64_t out_capacity, f5_stream stream);

/* ----------------------------------------------------------------- DTW-aligned mel-cepstral distance
 * A measure of the engine's own free-running output against a recording that needs nothing but the two mels: mel-cepstral distortion
 * between the generated and the recorded utterance, aligned by dynamic time warping.  For a pair (a, b), a has n frames and b has m,
 * each frame n_mels f32 log-mel values (the model's natural-log mel).  The arithmetic contract:
 *   cepstra       c_k(x) = sum_{j = 0 .. n_mels-1} (double)x_j * T[k][j] for k = 1 .. n_cep, T[k][j] = sqrt(2 / n_mels) *
 *                 cos(pi k (j + 0.5) / n_mels): the orthonormal DCT-II without coefficient 0 (the energy).  The table is built on the
 *                 host in double and uploaded (no device cos).  The sum is f64, j ascending, multiply then add, uncontracted; one
 *                 thread produces one (row, k) value, so there is no reduction order beside the contract's.  Cepstra stay f64.
 *   distance      d(i, j) = (10 / ln 10) * sqrt(2 * sum_{k = 1 .. n_cep} (c_k(a_i) - c_k(b_j))^2) in f64, k ascending, with the double
 *                 4.3429448190325175 for 10 / ln 10.  d is bit-symmetric in its two arguments.
 *   alignment     the symmetric step pattern with weights (1, 2, 1): D(0, 0) = 2 d(0, 0) and D(i, j) = min(D(i-1, j) + d(i, j),
 *                 D(i-1, j-1) + 2 d(i, j), D(i, j-1) + d(i, j)), cells outside the grid counting as +inf.  Every path then has total
 *                 weight exactly n + m, so the pair's value is D(n-1, m-1) / (n + m), in dB: continuous in the inputs and
 *                 independent of tie-breaking (a division by the path's length would be neither).  A cell is one addition per
 *                 candidate and a three-way minimum: no order of evaluation changes a bit, a pair's value is the same alone and in
 *                 any batch, and value(a, b) == value(b, a) bit for bit.
 * What the number is: an MFCC-style distance with MCD's scale constant.  It compares checkpoints, precisions and sampler settings on
 * the same held-out set; it is NOT comparable to published MCD figures, which use WORLD / SPTK mel-generalised cepstra.
 * Pair p's a is a_frames_host[p] rows of n_mels f32, a_row_stride elements apart, the first at a_base[a_start_host[p]]; b likewise.
 * Both sides are read where they lie (frames [lens_b, dur_b) of item b of sample()'s [B, N, mel] output are a pair's a without a
 * copy); a_base and b_base may be the same buffer.  out: f64 [P] on the device.  A non-finite mel value makes its own pair's result
 * non-finite and touches no other pair's.
 * f5_mel_distance_plan is pure host arithmetic (no HIP call): order_out[0 .. P) is the order in which the workgroups take the pairs
 * -- largest n * m first, ties by index, so that the long pairs do not form the tail -- and *workspace_bytes_out what the call holds
 * of the per-device workspace: the cepstra, (sum n + sum m) * n_cep * 8 bytes with the shorter side of every pair rounded up to
 * whole strips of columns (at most 15 frames more), and the tables (the DCT table sized for 256 mel bins).  Never an n x m matrix:
 * one 4096 x 4096 pair at n_cep = 13 plans under 2 MiB.
 * f5_mel_distance is two launches: the cepstra (one thread per (row, k) over the packed rows of both sides, the table through LDS)
 * and the recurrence (one workgroup per pair over anti-diagonals: a thread owns a strip of adjacent columns of the shorter side,
 * keeps its D(i-1, j) in registers, gets D(i, j-1) and D(i-1, j-1) from its left neighbour by a lane shift, across waves through a
 * two-slot LDS ring with one barrier per step; d(i, j) is computed a step ahead, off the dependency chain).  Stand-alone like the
 * silence stage: no handle, the per-device workspace, one table copy through a pinned slot, no host read, no synchronisation except
 * the growth of the workspace, no atomics.
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the pair: a null pointer, P < 1 or P > 65535,
 * a_frames or b_frames outside [1, 4096], n_cep outside [1, min(64, n_mels - 1)], n_mels outside [2, 256], a row stride below n_mels,
 * a start below 0, more than 2^28 cepstral values in one call. */
int f5_mel_distance_plan(int32_t P, const int32_t* a_frames_host, const int32_t* b_frames_host, int32_t n_cep, int32_t* order_out,
                         int64_t* workspace_bytes_out);
int f5_mel_distance(const float* a_base, const float* b_base, int32_t P, const int64_t* a_start_host, const int32_t* a_frames_host,
                    int64_t a_row_stride, const int64_t* b_start_host, const int32_t* b_frames_host, int64_t b_row_stride,
                    int32_t n_mels, int32_t n_cep, double* out /* [P], device */, f5_stream stream);

/* ----------------------------------------------------------------- the alignment itself: f5_mel_distance with its path
 * f5_mel_align takes f5_mel_distance's arguments and computes the same D; beside it, it names the path that D(n-1, m-1) belongs to,
 * so that anything per frame (the pitch tracks below) can be compared along it.  One rule is added to the contract above:
 *   predecessor   the predecessor of cell (i, j), i a frame of a and j a frame of b, is the candidate whose sum is the minimum of
 *                 D(i-1, j-1) + 2 d(i, j), D(i-1, j) + d(i, j), D(i, j-1) + d(i, j); on equal sums the diagonal (i-1, j-1) wins
 *                 first, then (i-1, j), then (i, j-1).  The rule is in terms of a and b: the kernel puts the shorter side on the
 *                 columns and honours it after that swap.  The path is the chain of predecessors from (n-1, m-1) to (0, 0).
 * Outputs, all on the device: dist f64 [P], bit for bit what f5_mel_distance writes for the same pairs; path_len i32 [P]; path, i32
 * pairs (i, j): pair p's path starts at pair sum_{q < p} (n_q + m_q - 1) (2 int32 each) and runs in forward order from (0, 0) to
 * (n-1, m-1), path_len[p] cells, max(n, m) <= path_len <= n + m - 1; the slots behind it up to the next pair's start are scratch.
 * A pair whose D(n-1, m-1) is not finite gets path_len = 0.  A pair's path does not depend on the batch it is aligned in.
 * Three launches: the cepstra, the recurrence in its pointer form (the same body; 2 bits per cell, a thread gathers the codes of its
 * strip of columns over 16 / W rows into one 32-bit word and stores it when it is full -- the layout is internal) and the backtrack
 * (one wave per pair, one walking lane, then the wave turns the path forward).  f5_mel_align_plan is f5_mel_distance_plan for this
 * call: the same order, and a workspace that also holds the back-pointers, ceil(max(n, m) / (16 / W)) * T words of 4 bytes per pair
 * (W, T: the pair's strip and thread count; 4 MiB for one 4096 x 4096 pair).
 * F5_EINVAL as f5_mel_distance, and: a null path_len or path, more than 2^26 bytes of back-pointers in one call (split the batch). */
int f5_mel_align_plan(int32_t P, const int32_t* a_frames_host, const int32_t* b_frames_host, int32_t n_cep, int32_t* order_out,
                      int64_t* workspace_bytes_out);
int f5_mel_align(const float* a_base, const float* b_base, int32_t P, const int64_t* a_start_host, const int32_t* a_frames_host,
                 int64_t a_row_stride, const int64_t* b_start_host, const int32_t* b_frames_host, int64_t b_row_stride, int32_t n_mels,
                 int32_t n_cep, double* dist /* [P], device */, int32_t* path_len /* [P], device */,
                 int32_t* path /* [sum (n + m - 1)][2], device */, f5_stream stream);

/* ----------------------------------------------------------------- pitch tracks: YIN on a ragged batch of waveforms
 * The F0 track of every item of a ragged batch of mono f32 waveforms, on the frame grid of the mel front-end, by the YIN estimator
 * (de Cheveigne and Kawahara 2002: difference function, cumulative mean normalisation, absolute threshold, parabolic
 * interpolation), with no smoothing over time, no octave correction and no voicing model beside the threshold.  Item p is
 * len_host[p] samples from base[start_host[p]], read where they lie.  Frame t of an item, t = 0 .. frames_host[p] - 1, is centred
 * on sample first_centre + t * hop: frame t of MelSpec for the same wave with first_centre = 0 and len / hop + 1 frames (the
 * vocos front-end), with first_centre = hop / 2 and len / hop frames (bigvgan's).  The arithmetic contract, everything f64 and
 * uncontracted, W = window:
 *   samples       L = W + tau_max + 1, s0 = first_centre + t * hop - L / 2 (integer division); x[j] is sample s0 + j of the item,
 *                 0 where s0 + j is outside [0, len).
 *   difference    d(tau) = sum_{j = 0 .. W-1} ((double)x[j] - (double)x[j + tau])^2 for tau = 1 .. tau_max + 1: j ascending,
 *                 subtract, multiply, then add.
 *   cumulative    S(tau) = S(tau - 1) + d(tau), S(0) = 0, strictly in ascending tau.
 *   normalised    d'(tau) = (d(tau) * (double)tau) / S(tau) if S(tau) > 0, else 1.
 *   choice        the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; from there, while tau + 1 <= tau_max and
 *                 d'(tau + 1) < d'(tau), tau advances.  No such tau: the frame is unvoiced, f0 = 0 and ap = the minimum of d' over
 *                 [tau_min, tau_max] (the first one, scanned ascending with <).
 *   refinement    a, b, c = d'(tau - 1), d'(tau), d'(tau + 1), den = a - 2 b + c; delta = (0.5 (a - c)) / den if den > 0, else 0,
 *                 clamped to [-0.5, 0.5]; f0 = (double)sample_rate / ((double)tau + delta), ap = b.
 * f0 and ap: f64, packed item after item, frames_host[p] values each.  A non-finite sample reaches only the frames of its own item
 * that read it: a frame that holds it inside its first W samples is unvoiced (S is NaN, so d' = 1 at every lag), one that holds
 * it further out follows the contract on the lags the sample does not reach.  No other item is touched.
 * One launch (a workgroup per frame, a thread per lag, the samples in LDS), one table copy through a pinned slot, no host read, no
 * synchronisation except the growth of the per-device workspace, no atomics.
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the item: a null pointer, P < 1 or P > 65535,
 * window outside [64, 2048], not 2 <= tau_min < tau_max <= 1024, threshold outside (0, 1], sample_rate or hop outside [1, 2^20],
 * first_centre outside [0, 2^30], start_p < 0, len_p < 1, frames_p < 1, more than 2^22 frames in one call. */
int f5_pitch_track(const float* base, int32_t P, const int64_t* start_host, const int32_t* len_host, int32_t sample_rate, int32_t hop,
                   int32_t first_centre, const int32_t* frames_host, int32_t window, int32_t tau_min, int32_t tau_max,
                   double threshold, double* f0 /* device */, double* ap /* device */, f5_stream stream);

/* ----------------------------------------------------------------- smoothed pitch tracks: pYIN candidates and a Viterbi decode
 * pYIN (Mauch and Dixon 2014) in two calls.  Stage 1 lets every threshold of a prior distribution make YIN's choice, which gives a
 * frame a few weighted lag candidates; stage 2 decodes one candidate per frame, or "unvoiced", over pitch-bin x voicing states, so
 * that a jump of an octave for a few frames, outside the transition band, cannot win.  Everything is f64 and uncontracted; every
 * table is built on the host and passed down, so that the device only adds, multiplies, divides and compares, in the order below.
 *
 * Stage 1, f5_pitch_candidates, per frame.  The samples, d(tau), S(tau) and d'(tau) are f5_pitch_track's, by the same code.
 *   thresholds    s_i = (double)i / (double)N for i = 1 .. N, with the weights w_host[i - 1] (f64, finite, >= 0).
 *   votes         for i ascending, tau_i is f5_pitch_track's choice at threshold s_i (the smallest tau in [tau_min, tau_max] with
 *                 d'(tau) < s_i, then on while tau + 1 <= tau_max and d'(tau + 1) < d'(tau)), and prob(tau_i) = prob(tau_i) + w_i.
 *                 No such tau: prob(tau_g) = prob(tau_g) + w_i * p_absent, tau_g the arg-min of d' over [tau_min, tau_max] (the
 *                 first one, scanned ascending with <).  prob starts at 0; a lag's sum runs in ascending i.
 *   candidates    every lag with prob > 0, in ascending lag, is a candidate (tau, f0, prob), f0 by f5_pitch_track's refinement at
 *                 tau.  A frame whose d'(tau) is NaN at any tau in [1, tau_max + 1] has no candidates.
 * Outputs on the device, frames packed item after item as f5_pitch_track packs them, N slots per frame: cand_count i32 [frames],
 * cand_lag i32 [frames][N], cand_f0 and cand_prob f64 [frames][N]; the slots behind a frame's count are written as zeros.  One
 * launch, a workgroup per frame; a thread per threshold finds tau_i, one lane adds the votes in order.  Otherwise as
 * f5_pitch_track: one table copy through a pinned slot, no host read, no atomics; an item reads its own samples only.
 * F5_EINVAL as f5_pitch_track (without the threshold), and: N outside [1, 256], a null w_host, a weight that is not finite or is
 * negative, p_absent outside [0, 1], a null output.
 *
 * Stage 2, f5_pitch_decode, per item, over frames t = 0 .. frames_host[p] - 1 of the candidate arrays (packed as stage 1 writes
 * them; a frame's count is taken as clamped to [0, N], its candidates in array order, which is ascending lag).
 *   bins          M pitch bins: edge_host[M + 1] in Hz, strictly ascending, and centre_host[M].  A candidate's bin is the number of
 *                 j in [1, M - 1] with edge[j] <= f0: compares alone, in [0, M - 1] whatever f0 is.
 *   transitions   trans_host[M][2 * reach + 1]: entry [i][k] is the weight of going from bin i to bin i + k - reach (a destination
 *                 outside [0, M - 1] is never read).  stay = 1 - p_switch, computed on the host in f64.
 *   observation   ov(m) = the sum of prob over the frame's candidates in bin m, in array order; tot = the sum over all of them, in
 *                 array order; ou = max(0, 1 - tot) / (double)M.  obs(voiced, m) = max(ov(m), 2^-60), obs(unvoiced, m) =
 *                 max(ou, 2^-60).
 *   recurrence    delta(v, m) = 1 before frame 0.  inner_v(j) = max over i in [max(0, j - reach), min(M - 1, j + reach)] of
 *                 delta_prev(v, i) * trans[i][j - i + reach], i ascending, the smallest i winning ties.  For a destination
 *                 voicing v': c = inner_v'(j) * stay, and the other voicing u replaces it only if inner_u(j) * p_switch > c.
 *                 delta(v', j) = obs(v', j) * c.  Then every delta of the frame is divided by the frame's maximum (an order-free
 *                 maximum of exact values), where that maximum is > 0.
 *   end state     the largest delta of the last frame: unvoiced states scanned before voiced ones, bins ascending, with >.
 *   path          one back-pointer byte per state and frame (bit 7: the source's voicing, bits 0 .. 6: i - j + reach), walked back
 *                 from the end state.
 * Outputs, f64 [frames] on the device, packed like the candidates: f0 -- 0 where the frame's state is unvoiced, otherwise the f0 of
 * the frame's candidate in the state's bin with the largest prob (the first one in array order on ties), or centre[m] where the bin
 * holds no candidate of that frame -- and voiced_prob = tot.  An item reads its own frames only: its track is the same alone, in
 * any batch and in any order.
 * workspace: device memory for the back-pointers, at least f5_pitch_decode_bytes(frames of the call, M) = 2 * M * frames bytes
 * (the layout is internal); it is the caller's and can be reused by the next call on the stream.  One launch: a workgroup per
 * item, a thread per bin carrying both voicings, delta ping-ponging in LDS, the frame's maximum by a wave and LDS max-reduction;
 * one lane walks the path back, then the workgroup writes the outputs.  The tables go down in one copy through a pinned slot; no
 * host read, no synchronisation except the growth of the per-device workspace that holds the tables, no atomics.
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the item: a null pointer, N outside [1, 256], P < 1
 * or P > 65535, frames_p < 1, more than 2^22 frames in one call, M outside [2, 512], reach outside [1, 63], p_switch outside (0, 1),
 * a table value that is not finite, a negative transition, edges not strictly ascending, workspace_bytes below the need. */
int f5_pitch_candidates(const float* base, int32_t P, const int64_t* start_host, const int32_t* len_host, int32_t sample_rate,
                        int32_t hop, int32_t first_centre, const int32_t* frames_host, int32_t window, int32_t tau_min,
                        int32_t tau_max, int32_t N, const double* w_host, double p_absent, int32_t* cand_count /* device */,
                        int32_t* cand_lag /* device */, double* cand_f0 /* device */, double* cand_prob /* device */,
                        f5_stream stream);
int64_t f5_pitch_decode_bytes(int64_t frames_total, int32_t M);
int f5_pitch_decode(const int32_t* cand_count, const double* cand_f0, const double* cand_prob, int32_t N, int32_t P,
                    const int32_t* frames_host, int32_t M, const double* edge_host, const double* centre_host, int32_t reach,
                    const double* trans_host, double p_switch, void* workspace /* device */, int64_t workspace_bytes,
                    double* f0 /* device */, double* voiced_prob /* device */, f5_stream stream);

/* ----------------------------------------------------------------- speaker similarity: Gaussian cepstral divergence
 * A text-independent measure of whether two sets of mel frames come from one voice, with no model: one full-covariance Gaussian per
 * side over cepstral vectors, and a second-order divergence between the two (Bimbot, Magrin-Chagnolleau and Mathan 1995).  Two calls:
 * f5_cep_moments gives count, mean and centred scatter of every segment of a ragged set -- additive statistics, which the caller
 * pools over items into speakers --, f5_gauss_divergence the four raw terms of the divergence for pairs of such records.  Everything
 * is f64 and uncontracted; the device adds, subtracts, multiplies, divides, takes square roots and compares, in the order below.
 *
 * f5_cep_moments.  Segment s is frames_host[s] rows of n_mels f32, row_stride elements apart, the first at base[start_host[s]], read
 * where it lies (f5_mel_distance's addressing of a side); F = frames_host[s], frames t = 0 .. F - 1.
 *   cepstra       c_k(t) for k = 1 .. n_cep is f5_mel_distance's: sum_j (double)x_j * T[k][j], j ascending, multiply then add, with
 *                 T[k][j] = sqrt(2.0 / n_mels) * cos(pi * k * (j + 0.5) / n_mels) evaluated on the host in double in exactly that
 *                 order of operations (pi * k, times (j + 0.5), divided by n_mels; the cosine is the host C library's).
 *   deltas        with deltas = 1, dc_k(t) = ((c_k(t+1) - c_k(t-1)) + 2.0 * (c_k(t+2) - c_k(t-2))) / 10.0, every frame index clamped
 *                 to [0, F - 1].  Deltas are taken over the segment's own frames, whatever the selection below.  The feature vector
 *                 of a frame is v = [c_1 .. c_n_cep] or [c_1 .. c_n_cep, dc_1 .. dc_n_cep]: C = n_cep * (1 + deltas) entries.
 *   energy        e(t) = sum_j (double)x_j, j ascending, from 0.
 *   selection     frame t counts iff (mask == NULL or mask[r] != 0) and (gate_sum < 0 or e(t) >= emax - gate_sum), where r is the
 *                 frame's index among the frames of the call (segment after segment) and emax the largest e of the segment (a
 *                 maximum of doubles has no order).  If any e(t) of a segment is not finite, that segment alone reports
 *                 count = -1 and NaN in every entry of mean and scatter.
 *   chunks        the frames of a segment are cut into chunks of kMomChunk = 64 consecutive frames (the last one shorter).
 *   pass 1        a chunk's partial of entry p is the sum of v_p over the chunk's selected frames, t ascending, from 0; the
 *                 segment's sum is the sum of the chunk partials, chunk ascending, from 0.  n = the selected frames;
 *                 mean_p = sum_p / (double)n.
 *   pass 2        for p <= q, a chunk's partial is the sum of (v_p - mean_p) * (v_q - mean_q) over the chunk's selected frames, t
 *                 ascending, from 0 (subtract, subtract, multiply, then add); scatter_pq is the sum of the chunk partials, chunk
 *                 ascending, from 0.  Centred sums, never raw second moments.
 *   empty         n = 0: count = 0, every entry of mean and scatter is +0.
 * Outputs on the device: count i32 [S]; mean f64 [S][C]; scatter f64 [S][C (C + 1) / 2], the upper triangle packed row-major
 * ((0,0), (0,1) .. (0,C-1), (1,1) ..).  A segment's record depends on its own frames (and mask entries) alone: it is the same alone
 * and in any batch.
 * Six launches: the cepstra and energies (one thread per (row, k), the table through LDS), the selection (a workgroup per segment),
 * and twice a chunk launch (a workgroup per (segment, chunk) with the chunk's feature vectors in LDS; ONE thread sums an entry over
 * the chunk's frames) followed by a fold (one thread per entry, chunk ascending).  Stand-alone like f5_mel_distance: no handle, the
 * per-device workspace, one table copy through a pinned slot, no host read, no synchronisation except the growth of the workspace,
 * no atomics.  f5_cep_moments_plan is pure host arithmetic (no HIP call): *workspace_bytes_out is what the call holds of the
 * workspace -- (n_cep + 1) doubles and one byte per frame, C + C (C + 1) / 2 doubles and one int per chunk, and the tables (the DCT
 * table sized for 256 mel bins).
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the segment: a null pointer (mask may be null),
 * S < 1 or S > 65535, frames outside [1, 4096], n_mels outside [2, 256], n_cep outside [1, min(32, n_mels - 1)], deltas not 0 or 1,
 * a row stride below n_mels, a start below 0, a gate_sum that is NaN, more than 2^28 cepstral or partial values in one call.
 *
 * f5_gauss_divergence.  Records as f5_cep_moments writes them, two sets: a (a_records of them) and b (b_records; the same arrays
 * may be passed for both).  Pair p is record i = i_host[p] of a against record j = j_host[p] of b.  With A = scatter / (double)n
 * entry by entry (the covariance of a record with count n):
 *   factor        the Cholesky factor L (lower) of A, column c = 0 .. C - 1 in turn: for r >= c, s = A_rc, then s = s - L_rk * L_ck
 *                 for k = 0 .. c - 1 ascending; L_cc = sqrt(s) and, for r > c, L_rc = s / L_cc: one square root or one division per
 *                 element.  The s of a diagonal element is the column's pivot.
 *   X, Y          X = L_i^-1 L_j by forward substitution, column c in turn down its rows r = c .. C - 1: s = (L_j)_rc, then
 *                 s = s - (L_i)_rk * X_kc for k = c .. r - 1 ascending, X_rc = s / (L_i)_rr (X is lower triangular; nothing above
 *                 the diagonal enters a sum).  Y = L_j^-1 L_i likewise.
 *   traces        the column sum of X_rc * X_rc over r = c .. C - 1 ascending, from 0; tr_ij = the column sums added c ascending,
 *                 from 0.  That is trace(A_i^-1 A_j).  tr_ji likewise from Y.
 *   means         d = mean_i - mean_j; z = L_i^-1 d by the same substitution (s = d_r, k = 0 .. r - 1); q_i = the sum of z_r * z_r, r
 *                 ascending, from 0.  q_j likewise with L_j (and the same d).
 * terms: f64 [P][4] on the device, (tr_ij, tr_ji, q_i, q_j); status i32 [P].  A pair is singular iff either record has count <= C
 * or a pivot of either factor is <= 0 or not finite: it gets four NaNs and status 1 (otherwise status 0).  That is never an error
 * and touches no other pair.  A record against itself gives exactly (C, C, 0, 0); (i, j) and (j, i) give the same bits, swapped.
 * What callers make of the terms (metrics.speaker_numbers): the symmetric Kullback-Leibler divergence in nats, 0.5 ((tr_ij + tr_ji)
 * - 2 C) + 0.5 (q_i + q_j) -- the log-determinants cancel --, and the arithmetic-harmonic sphericity log(tr_ij tr_ji / C^2).  Neither
 * is SIM, an embedding cosine, or comparable with any published figure.
 * One launch: a workgroup of 64 threads per pair, both factors and X (then Y) packed in LDS, thread r owning row r of both factors
 * and column r of X and Y.  The index tables go down in one copy through a pinned slot; otherwise as f5_cep_moments.
 * F5_EINVAL, with nothing launched or staged and a message naming the argument or the pair: a null pointer, C outside [1, 64], P < 1
 * or P > 65535, a_records or b_records < 1, an index outside its records. */
#define F5_MOM_CHUNK 64 /* kMomChunk: frames of a chunk of f5_cep_moments */
int f5_cep_moments_plan(int32_t S, const int32_t* frames_host, int32_t n_cep, int32_t deltas, int64_t* workspace_bytes_out);
int f5_cep_moments(const float* base, int32_t S, const int64_t* start_host, const int32_t* frames_host, int64_t row_stride,
                   int32_t n_mels, int32_t n_cep, int32_t deltas, const uint8_t* mask /* device, one per frame, or NULL */,
                   double gate_sum, int32_t* count /* [S], device */, double* mean /* [S][C], device */,
                   double* scatter /* [S][C (C + 1) / 2], device */, f5_stream stream);
int f5_gauss_divergence(const int32_t* a_count, const double* a_mean, const double* a_scatter, int32_t a_records,
                        const int32_t* b_count, const double* b_mean, const double* b_scatter, int32_t b_records, int32_t C,
                        int32_t P, const int32_t* i_host, const int32_t* j_host, double* terms /* [P][4], device */,
                        int32_t* status /* [P], device */, f5_stream stream);

/* ----------------------------------------------------------------------------- kernel-level entry points
 * Used by tests/ (parity of each kernel against a torch fp32 restatement) and by the micro-benchmarks.  fp32 in/out;
 * the operands are converted to the requested MFMA precision internally.  They allocate scratch and synchronise. */
int f5k_gemm(int32_t prec, const float* A, const float* W, const float* bias, int32_t act, float* out, int32_t M,
             int32_t N, int32_t K, int32_t tile_m, int32_t tile_n, f5_stream stream);
/* What launch_gemm decides for one problem, as pure host arithmetic (no HIP call, nothing launched): element size 1 (e4m3 codes:
 * plain operands, no conv, K % 128 == 0, tile ids 2, 8, 13 only -- anything else is refused), 2 or 4, the
 * device row count present or not and the row count expected behind it (m_hint, 0: none), the operand form (0 plain, 1 W pre-split,
 * 2 A and W pre-split), implicit conv or not, whether the epilogue admits the ping-pong tile, the forced cfg (-1 auto, -2 the
 * register-staged kernel, else a tile id) and the values of F5_GEMM_CFG (-1: unset) / F5_GEMM_CFG_N (0: every N).
 * plan[0] = number of launches (0: nothing to do, -1: the problem is refused), then per launch {kernel family (1 register-staged,
 * 2 LDS-DMA ring, 3 ping-pong), tile id (family 1: BM * 1000 + BN), first row, row count}; unused entries are 0.  plan: int32[9]. */
int f5k_gemm_plan(int32_t elem_size, int32_t M, int32_t N, int32_t K, int32_t has_m_limit, int32_t m_hint, int32_t operand_form,
                  int32_t conv, int32_t pp_epilogue, int32_t force_cfg, int32_t env_cfg, int32_t env_cfg_n, int32_t* plan);
/* q, k, v f32[Bp, H, N, 64] (q unscaled) -> out f32[Bp, N, H*64]; kv_lens HOST int32[Bp] or NULL */
int f5k_attention(int32_t prec, const float* q, const float* k, const float* v, const int32_t* kv_lens_host,
                  float* out, int32_t Bp, int32_t H, int32_t N, f5_stream stream);
/* x f32[Bp, N, D]; w f32[D, D/16, 31]; y = mish(conv(x) + bias) (+ res); lens HOST int32[Bp] or NULL */
int f5k_convpos(int32_t prec, const float* x, const float* w, const float* bias, const float* res,
                const int32_t* lens_host, float* y, int32_t Bp, int32_t N, int32_t D, f5_stream stream);
/* The attention launch in the forms the engine's attention_block makes it (csrc/engine_impl.h): batch row b reads
 * lens[b % nlens], query blocks wholly past q_lens exit at once, packed output rows (RowPack).  f5k_attention is this call with
 * kv_lens only, nlens = Bp, an f32 output of Bp * N rows and a zero fill. */
typedef struct f5k_attn {
    const int32_t* kv_lens_host;   /* HOST int32[nlens] or NULL: key-padding mask */
    const int32_t* q_lens_host;    /* HOST int32[nlens] or NULL: query blocks wholly past it are not computed */
    const int32_t* row_start_host; /* HOST int32[Bp + 1] or NULL: batch row b writes output rows row_start[b] + (0 .. min(N, span_b) - 1);
                                      starts at 0, multiples of 4, spans <= round_up(N, 4) */
    int32_t nlens;       /* entries of kv_lens_host / q_lens_host, 1 .. Bp (the CFG halves share one table: nlens = Bp / 2) */
    int32_t mode;        /* 0: the precision's own kernel, output in its operand type (f32 for F5_PREC_F32 / F5_PREC_F16X3);
                            1: F5_PREC_F16X3 only -- the f16 kernel on f16 q / k / v^T, output as pre-split f32 rows (store4_planar) */
    int32_t hi_only;     /* F5_PREC_F16X3, mode 0: bit 0 = K Q^T as the plain f16 product, bit 1 = V^T P^T likewise */
    int32_t o_planar;    /* F5_PREC_F16X3, mode 0: the f32 output rows stored pre-split */
    float vt_pad_fill;   /* what V^T columns [N, round_up(N, 64)) hold (the engine never writes them); finite */
    int32_t pad0;
    void* out;           /* caller-owned [row_start[Bp] or Bp * N, H * 64] */
    float* out_f32;      /* f32 copy of a 16-bit out over n_out elements, or NULL */
    int64_t n_out;       /* elements of out (>= the rows above) */
} f5k_attn;
int f5k_attention_ex(int32_t prec, const float* q, const float* k, const float* v, int32_t Bp, int32_t H, int32_t N,
                     const f5k_attn* p, f5_stream stream);
/* The conv position embedding in the forms embed_input launches it: lens[b % nlens], packed rows of x / res / y. */
typedef struct f5k_conv {
    const int32_t* lens_host;      /* HOST int32[nlens] or NULL */
    const int32_t* row_start_host; /* HOST int32[Bp + 1] or NULL: batch row b owns rows row_start[b] .. row_start[b + 1] - 1 of x / res / y;
                                      starts at 0, multiples of 4, min(N, len_b) <= span_b <= round_up(N, 4) */
    int32_t nlens;       /* entries of lens_host, 1 .. Bp */
    int32_t pad0;
    int64_t rows;        /* rows of x / res / y as allocated (>= row_start[Bp] or Bp * N) */
} f5k_conv;
int f5k_convpos_ex(int32_t prec, const float* x, const float* w, const float* bias, const float* res, float* y, int32_t Bp,
                   int32_t N, int32_t D, const f5k_conv* p, f5_stream stream);
/* LayerNorm(no affine, eps) * (1 + scale[b]) + shift[b]; x f32[R, D], scale/shift f32[R / rows_per_batch, D] */
int f5k_layernorm_mod(const float* x, const float* scale, const float* shift, float* out, int32_t R, int32_t D,
                      int32_t rows_per_batch, float eps, f5_stream stream);
/* LayerNorm modulate as f5k_layernorm_mod, through the instantiation the engine uses for an operand precision: out is f32
 * (F5_PREC_F32 / F5_PREC_F16X3; planar 1: stored pre-split, 2: plain rows split afterwards by split_planar_kernel; D % 32 == 0)
 * or bf16 / f16 [R, D], caller-owned; out_f32
 * (or NULL) receives an f32 copy of a 16-bit out.  m_limit >= 0: device-side row count (rows >= m_limit are not written). */
int f5k_layernorm_mod_ex(int32_t prec, const float* x, const float* scale, const float* shift, void* out, float* out_f32,
                         int32_t R, int32_t D, int32_t rows_per_batch, float eps, int32_t m_limit, int32_t planar,
                         f5_stream stream);
/* F5_PREC_F8 through f5k_layernorm_mod_ex: out = uint8 [R * D] e4m3 codes followed by R scale bytes (out_f32 NULL, planar 0); it is
 * f5k_layernorm_q8 below without the packed form. */
/* The e4m3 output form of the AdaLN LayerNorm (F5_PREC_F8: the A operand of QKV / FF1): codes uint8 [R, D] and one e8m0 scale byte per
 * row, quantised from the f32 value.  batch_of_row_host (HOST int32[R], or NULL): the packed form, row r takes the scale / shift rows
 * of batch row batch_of_row_host[r] (rows D apart) instead of r / rows_per_batch.  m_limit >= 0: rows at or past it are not written. */
int f5k_layernorm_q8(const float* x, const float* scale, const float* shift, uint8_t* codes, uint8_t* scales, int32_t R, int32_t D,
                     int32_t rows_per_batch, float eps, int32_t m_limit, const int32_t* batch_of_row_host, f5_stream stream);
/* The stand-alone row quantiser of F5_PREC_F8 on caller-owned DEVICE buffers: x [R, ld] of f32 (prec F5_PREC_F32), bf16 or f16 values,
 * K real elements per row (K % 4 == 0) -> codes uint8 [R, ldc] (ldc >= K, ldc % 4 == 0; columns past K are not written) and scales
 * uint8 [R].  m_limit >= 0: device-side row count, rows at or past it are neither read nor written; -1: every row. */
int f5k_quant_rows_e4m3(int32_t prec, const void* x, int64_t ld, int32_t R, int32_t K, uint8_t* codes, int64_t ldc, uint8_t* scales,
                        int32_t m_limit, f5_stream stream);

/* One backbone GEMM C = A W^T (A f32 [M, K], W f32 [N, K], bias f32 [N], all cast to the operand type of `prec`) through a
 * production epilogue of csrc/gemm.h, built as the engine builds it.  Outputs go to caller-owned device buffers.
 * F5_PREC_F8: A and W are quantised row by row per the f8 contract (what f5k_quant_rows_e4m3 returns for them; K % 4 == 0) and
 * multiplied by the e4m3 kernel; cfg -1, 2, 8 or 13; 16-bit outputs (out16 STORE, q / k / v^T) are f16. */
#define F5K_EPI_STORE 0    /* EpiStore: out0 = act(C + bias) [M, N], f32 or (out16) the 16-bit operand type             */
#define F5K_EPI_GATE_RES 1 /* EpiGateRes: out0 = x f32 [M, N] = res + gate[b] * (C + bias); rows past lens[b] keep res     */
#define F5K_EPI_QKV 2      /* EpiQKV: out0 = q, out1 = k [Bp, H, Nseq, 64], out2 = v^T [Bp, H, 64, Npad]                   */
#define F5K_EPI_QKNORM 3   /* EpiQKV without rotary / scale, then qknorm_rope_kernel in place (qk_norm = "rms_norm")     */
typedef struct f5k_epi {
    int32_t kind;        /* F5K_EPI_* */
    int32_t cfg;         /* -1: launch_gemm's own dispatch (remainder split included); else a forced GemmCfg 2, 8, 9, 10, 13, 20 */
    int32_t a_presplit;  /* F5_PREC_F16X3: A is handed over pre-split (what the store4_planar producers write) */
    int32_t m_limit;     /* >= 0: device-side row count <= M; -1: none (QKV with row_start sets it itself) */
    int32_t out16;       /* STORE: output in the 16-bit operand type; QKV on f32 / f16x3 operands: q / k / v^T as f16 */
    int32_t act;         /* STORE: F5_ACT_* (engine: none, GELU-tanh) */
    int32_t planar;      /* STORE, f32 output under F5_PREC_F16X3: 1 stored pre-split by the epilogue, 2 plain store split afterwards
                            by split_planar_kernel (N % 32 == 0) */
    int32_t gate_stride; /* GATE_RES: floats between the gate vectors of consecutive batch rows (0: one vector) */
    int32_t rows_per_batch;
    int32_t nlens;       /* GATE_RES: entries of lens_host (>= the batch rows M spans) */
    const float* res;    /* GATE_RES: residual [M, N] (may be out0) */
    const float* gate;   /* GATE_RES: gate vectors or NULL (1) */
    const int32_t* lens_host;
    int32_t H, Nseq, Npad, pe_heads;   /* QKV / QKNORM: N == 3 * H * 64; Npad % 8 == 0, Npad >= Nseq */
    float q_scale;
    int32_t maxpos;      /* rows of rope_cos / rope_sin [maxpos, 32] (>= Nseq) */
    const float* rope_cos;
    const float* rope_sin;
    const int32_t* row_start_host; /* QKV: packed rows (RowPack) [Bp + 1], multiples of 4, or NULL (M == Bp * Nseq) */
    int32_t Bp;
    int32_t pad0;
    const float* gq;     /* QKNORM: RMSNorm gains [64] of q and k */
    const float* gk;
    void* out0;
    void* out1;
    void* out2;
    float* out0_f32;     /* f32 copies of 16-bit outputs (NULL: none) over n0 / n1 / n2 elements */
    float* out1_f32;
    float* out2_f32;
    int64_t n0, n1, n2;
} f5k_epi;
int f5k_gemm_epi(int32_t prec, const float* A, const float* W, const float* bias, int32_t M, int32_t N, int32_t K,
                 const f5k_epi* p, f5_stream stream);
/* ---- The step glue of sample() (csrc/elementwise.h), each through the launch helper csrc/engine_impl.h itself calls.  Every pointer is
 * a caller-owned DEVICE buffer of the stated shape (nothing is staged or copied); the call synchronises the stream.
 * `prec` selects the element type T of a typed buffer: F5_PREC_F32 / F5_PREC_F16X3 float, F5_PREC_BF16 bf16, F5_PREC_F16 f16. */
/* out T[rows, ldo] <- [x | cond or 0 | text] (pack_input_kernel): x, cond f32[B, N, mel], text_c / text_u f32[B, N, Dt]; batch rows
 * b' >= B are the unconditional half.  rowmap NULL: the padded form, Bp * N rows.  Else the RowPack form: rowmap int2[*row_limit],
 * row_limit int[1], lens int[B]; rows >= *row_limit and columns >= 2 mel + Dt are not written. */
int f5k_pack_input(int32_t prec, const float* x, const float* cond, const float* text_c, const float* text_u, void* out, int32_t ldo,
                   int32_t B, int32_t Bp, int32_t N, int32_t mel, int32_t Dt, int32_t drop_cond_first, const void* rowmap,
                   const int32_t* row_limit, const int32_t* lens, f5_stream stream);
/* rowmap int2[row_start[Bp]] <- (b', n) for every row of every segment; row_start int[Bp + 1] */
int f5k_fill_rowmap(const int32_t* row_start, void* rowmap, int32_t Bp, f5_stream stream);
/* One ODE update of y f32[B, N, mel] with dt = tgrid[step + 1] - tgrid[step] (tgrid f32, device) and v = p + (p - u) * cfg (use_cfg) or p:
 * f5k_euler_cfg: y += dt * v in place, the new y also into traj_slot (or NULL); f5k_midpoint_half_cfg: y_mid = y + v * (dt / 2).
 * row_start NULL: pred f32[(use_cfg ? 2 : 1), B, N, mel].  Else the RowPack form: pred f32[rows, mel] with the rows of batch row b' at
 * row_start[b'] (int[(use_cfg ? 2 : 1) * B + 1]), lens int[B]; frames n >= lens[b] keep y (traj_slot / y_mid receive it). */
int f5k_euler_cfg(float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start, const int32_t* lens,
                  const float* tgrid, int32_t step, float cfg, int32_t use_cfg, float* traj_slot, f5_stream stream);
int f5k_midpoint_half_cfg(const float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start,
                          const int32_t* lens, const float* tgrid, int32_t step, float cfg, int32_t use_cfg, float* y_mid, f5_stream stream);
/* The updates of f5_sample_items: pred f32[(use_cfg ? 2 : 1), B, N, mel]; t_items f32[B, steps_max + 1], cfg_items f32[B], steps_items
 * int[B] on the device.  Item b with step < steps_items[b]: dt from its own grid, v = p + (p - u) * cfg_items[b] (use_cfg and
 * cfg_items[b] >= 1e-5) or p; else y is not touched (traj_slot / y_mid receive it). */
int f5k_euler_cfg_items(float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const float* t_items, const float* cfg_items,
                        const int32_t* steps_items, int32_t steps_max, int32_t step, int32_t use_cfg, float* traj_slot, f5_stream stream);
int f5k_midpoint_half_cfg_items(const float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const float* t_items,
                                const float* cfg_items, const int32_t* steps_items, int32_t steps_max, int32_t step, int32_t use_cfg,
                                float* y_mid, f5_stream stream);
/* The updates of an isolated f5_sample_items call (f5_set_isolated_rows): the per-item rules above on the RowPack form of f5k_euler_cfg --
 * pred f32[rows, mel] with the rows of batch row b' at row_start[b'] (int[(use_cfg ? 2 : 1) * B + 1]), lens int[B], both required.
 * Item b with step < steps_items[b], frames n < lens[b]: updated; everything else of y is not written (traj_slot / y_mid receive y). */
int f5k_euler_cfg_items_packed(float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start, const int32_t* lens,
                               const float* t_items, const float* cfg_items, const int32_t* steps_items, int32_t steps_max, int32_t step,
                               int32_t use_cfg, float* traj_slot, f5_stream stream);
int f5k_midpoint_half_cfg_items_packed(const float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start,
                                       const int32_t* lens, const float* t_items, const float* cfg_items, const int32_t* steps_items,
                                       int32_t steps_max, int32_t step, int32_t use_cfg, float* y_mid, f5_stream stream);
/* The staging of f5_sample_span: y f32[B, N, mel] = prev_state[rows[b], n] (n < prev_N, else +0.0) where rows[b] >= 0, y_new[b, n]
 * where rows[b] == -1.  rows int32[B] on the device, rows_host the same table on the host (the rules of f5_sample_span's rows_host
 * are checked on it); prev_state f32[prev_B, prev_N, mel] and y_new f32[B, N, mel] on the device, NULL where no row reads them. */
int f5k_span_stage(float* y, const float* prev_state, int32_t prev_B, int32_t prev_N, const float* y_new, const int32_t* rows,
                   const int32_t* rows_host, int32_t B, int32_t N, int32_t mel, f5_stream stream);
/* The same into rows `pitch` >= N frames apart (a length bucket's arena): y f32[B, pitch, mel], of which the frames n < N of every row
 * are written and the others are not touched.  prev_state and y_new keep their own pitches, prev_N and N. */
int f5k_span_stage_pitched(float* y, int32_t pitch, const float* prev_state, int32_t prev_B, int32_t prev_N, const float* y_new,
                           const int32_t* rows, const int32_t* rows_host, int32_t B, int32_t N, int32_t mel, f5_stream stream);
/* The glue of f5_flow_loss (csrc/flow.h).  span int32[B][2] on the device, span_host the same table on the host (checked: 0 <= start <=
 * end <= N); t f32[B] on the device.  f5k_flow_mix: phi f32[B, N, mel] = (1 - t[b]) * x0 + t[b] * x1, cond (or NULL) = x1 with the span's
 * frames +0.0.  f5k_flow_loss_reduce: sq_sum f64[B], count int32[B], frame_err f32[B, N] or NULL from pred, x0, x1 f32[B, N, mel];
 * part: scratch of B * ceil(N / 64) doubles. */
int f5k_flow_mix(const float* x0, const float* x1, const float* t, const int32_t* span, const int32_t* span_host, float* phi, float* cond,
                 int32_t B, int32_t N, int32_t mel, f5_stream stream);
int f5k_flow_loss_reduce(const float* pred, const float* x0, const float* x1, const int32_t* span, const int32_t* span_host, double* part,
                         double* sq_sum, int32_t* count, float* frame_err, int32_t B, int32_t N, int32_t mel, f5_stream stream);
/* dst f32[rows, width] = src[idx[r % nidx], :]; idx int[nidx] (device), width % 4 == 0.  The caller keeps idx inside src. */
int f5k_mod_gather(const float* src, const int32_t* idx, float* dst, int32_t rows, int32_t nidx, int32_t width, f5_stream stream);
/* The time rows of an f5_sample_items call (host arithmetic, no device needed): the evaluation times of every live item -- Euler t[b][i];
 * midpoint t[b][i] and t[b][i] + 0.5f * (t[b][i+1] - t[b][i]) -- walked evaluation-major, then item-major, deduplicated by f32 bit pattern
 * in first-appearance order.  times_out f32[evals * steps_max * B] (the first *U are written), idx_out int32[evals * steps_max][B]: the
 * row of every (evaluation, item), 0 for a finished item.  The table rules of f5_sample_items apply. */
int f5k_item_time_rows(const float* t_items, const int32_t* steps_items, int32_t steps_max, int32_t B, int32_t method, float* times_out,
                       int32_t* idx_out, int32_t* U);
/* out f32[rows, C] = rowmask[r] ? a[r] : (b ? b[r] : 0); rowmask uint8[rows]; out may be b */
int f5k_select_rows(const float* a, const float* b, const uint8_t* rowmask, float* out, int64_t rows, int32_t C, f5_stream stream);
/* feat f32[S, 256] = [sin | cos] of (1000 t[s]) * freq[j]; t f32[S], freq f32[128] */
int f5k_time_sinus(const float* t, const float* freq, float* feat, int32_t S, f5_stream stream);
/* x_transformers RMSNorm: out T[R, D] = x / max(|x|_2, 1e-12) * sqrt(D) * g; x f32[R, D], g f32[D]; D % 4 == 0, D <= 2048.
 * planar (T float, D % 32 == 0): rows stored pre-split */
int f5k_xrmsnorm(int32_t prec, const float* x, void* out, int32_t R, int32_t D, const float* g, int32_t planar, f5_stream stream);
/* UNetT glue.  assemble: x f32[Bp, N + 1, D] = [temb[b' * temb_stride] ; h[b']], h f32[Bp, N, D]; cat2: out T[rows, 2 D] = [x | skip]
 * (planar as above); strip: out f32[Bp, N, C] = in[Bp, 1 + n, C] */
int f5k_unett_assemble(const float* h, const float* temb, int32_t temb_stride, float* x, int32_t Bp, int32_t N, int32_t D, f5_stream stream);
int f5k_cat2(int32_t prec, const float* x, const float* skip, void* out, int32_t rows, int32_t D, int32_t planar, f5_stream stream);
int f5k_strip_first_token(const float* in, float* out, int32_t Bp, int32_t N, int32_t C, f5_stream stream);

/* The work-buffer plan of an engine of config c, as pure host arithmetic (no HIP call, nothing launched, no device needed): the engine's
 * own carve for the reservation (B, N, S) and its own placement of the side chain of a split-CFG (F5_SPLIT_CFG=1) call of
 * call_B <= B utterances of call_N <= N frames, both on a dry-run arena.  *total_bytes: the arena size.  main_off / side_off
 * int64[F5K_WORK_BUFFERS]: byte offset of each buffer in the order of F5K_WORK_NAMES, -1 where the config has no such buffer (and for the buffers of f5_sample_items, which
 * an engine carves only once such a call has been made);
 * side_off equals main_off for a buffer both chains share.  a8 / a8s (F5_PREC_F8 only, else -1): the e4m3 codes of the block GEMM's A
 * operand, rows * max(dim, ff_dim, heads * 64) bytes, and its row scale bytes. */
#define F5K_WORK_BUFFERS 46
#define F5K_WORK_NAMES                                                                                                              \
    "tdev feat th temb st mod lens lens_plain row_start rowmap step_cond text_c text_u tx_a tx_b tx_h1 grn_part uc acat h c1 x pred " \
    "xn q k ao vt ffh a8 a8s in_cond y y_mid out_buf traj_buf in_mask in_text cat2 skips pred_all mod_rows it_t it_cfg it_steps it_idx"
int f5k_work_plan(const f5_config* c, int32_t B, int32_t N, int32_t S, int32_t call_B, int32_t call_N, int64_t* total_bytes,
                  int64_t* main_off, int64_t* side_off);
/* Diagnostic taps of the MMDiT forward (tests): `taps` (device f32, or NULL to switch them off) receives, from every later
 * f5_dit_forward of this engine, the audio embedding [Bp, N, D], then per block the text stream c [Bp, nt, D] (not in the last block,
 * which drops it) and the audio stream x [Bp, N, D], back to back; Bp = B, or 2 B with cfg_infer.  sample() never writes them. */
int f5k_mmdit_taps(f5_engine* e, float* taps);
/* repeated-launch timing of one GEMM shape (for bench/roofline): returns average microseconds per launch.  F5_PREC_F8: the e4m3
 * kernel on random codes into f16 rows (K % 128 == 0; tile_m 0 or -(2 | 8 | 13)); tile_n == 1 adds the stand-alone row quantiser of
 * an f16 A operand to every timed launch, as the engine runs it in front of the out-projection and FF2. */
int f5k_gemm_time(int32_t prec, int32_t M, int32_t N, int32_t K, int32_t tile_m, int32_t tile_n, int32_t iters,
                  float* avg_us, f5_stream stream);

/* Per-launch HIP-event timing of the last f5_sample call when enabled: one (start, stop) event pair per kernel launch
 * on the launch stream, summed by kernel class; flops = algorithmic FLOPs of the bracketed launches (MFMA classes).
 * Off by default.  classes: 0 gemm, 1 attention, 2 layernorm, 3 convpos, 4 pack/euler/select, 5 text encoder
 * (whole sub-graph), 6 time-MLP + AdaLN precompute (whole sub-graph). */
int f5_profile_enable(f5_engine* e, int32_t on);
int f5_profile_read(f5_engine* e, float* ms_by_class, int32_t* launches_by_class, double* flops_by_class,
                    int32_t nclass);

#ifdef __cplusplus
}
#endif
#endif /* F5_HIP_H */
