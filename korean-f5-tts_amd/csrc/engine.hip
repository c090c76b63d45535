// libf5hip.so -- engine + C ABI (include/f5_hip.h) for the F5-TTS inference hot path on MI355X / gfx950.
//
// Data layout in HBM (everything token-major, one arena per engine, sized for the largest (batch, frames) seen):
//   ODE state y, step_cond, pred     f32 [B | 2B, N, mel]
//   residual stream x, embed h, c1   f32 [2B*N, D]
//   xn (LN-modulated), attn out, ffh T   [2B*N, D | inner | F]          T = bf16 / f16 (speed) or f32 (parity)
//   q, k                             T   [2B, H, N, 64]      v^T  T [2B, H, 64, Npad]
//   mod                              f32 [evals, (6*depth + 2) * D]     all AdaLN vectors of all layers for ALL backbone
//                                                                       evaluations (steps, or 2 * steps for midpoint)
// Weights are engine-owned copies: GEMM operands in T ([out, in], K padded to whole 128-byte K-tiles), everything that feeds
// fp32-only stages (time MLP, AdaLN stack, text encoder, norms, biases) in f32.
//
// What is restructured w.r.t. the reference (results identical up to fp rounding):
//   * AdaLN / time-embedding work depends only on t, not on x: it is hoisted out of the ODE loop and computed for all
//     NFE steps by three GEMMs before the first step (the reference recomputes 22 x [D -> 6D] per forward).
//   * q/k/v projections are one fused GEMM whose epilogue applies bias, rotary, the softmax scale and the head split.
//   * gate * f(x) + residual and the padded-row mask are GEMM epilogues; GELU is an epilogue; no [B,D,N] permutes.
//
// This file: the C ABI and the precision-independent host logic.  The kernels and the per-call graph of launches are
// templates over the MFMA operand type (engine_impl.h), instantiated in engine_{bf16,f16,f32}.hip.
#include "engine_types.h"

// precision dispatch of one EngineOps<T> member (prec_info, internal.h)
#define F5_OPS(e, CALL)                                                             \
    (prec_info((e)->cfg.precision).elem == PE_BF16  ? EngineOps<bf16_t>::CALL       \
     : prec_info((e)->cfg.precision).elem == PE_F16 ? EngineOps<f16_t>::CALL        \
                                                    : EngineOps<float>::CALL)

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int f5_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* f5_last_error(void) { return g_err; }
extern "C" const char* f5_version(void) { return "f5hip 2 gfx950"; }
// ----------------------------------------------------------------------------------------------- create
// the switches of one engine (engine_types.h Switches): the environment as f5_create finds it
static Switches read_switches(const f5_config& c) {
    auto flag = [](const char* name, bool dflt) {   // "0" switches off, "1" switches on
        const char* v = getenv(name);
        return (v && v[0] == (dflt ? '0' : '1')) ? !dflt : dflt;
    };
    Switches sw;
    sw.graphs = flag("F5_HIP_GRAPH", true);
    sw.split_cfg = flag("F5_SPLIT_CFG", false);
    sw.pack_rows = flag("F5_PACK_ROWS", true);
    if (const char* v = getenv("F5_CHUNK_ROWS")) sw.chunk_rows = std::max(1L, atol(v));   // (a budget below one utterance: one utterance)
    sw.weight_prefetch = flag("F5_WEIGHT_PREFETCH", true);
    if (const char* v = getenv("F5_X3_ABLATE")) sw.x3_ablate = c.precision == F5_PREC_F16X3 ? atoi(v) : 0;
    sw.x3_attn_split = flag("F5_X3_ATTN_SPLIT", false);
    if (const char* v = getenv("F5_STORE_WT")) sw.store_wt = atoi(v) & F5_WT_ALL;
    if (const char* v = getenv("F5_LEN_BUCKET")) sw.len_bucket = (int)std::min(std::max(atol(v), -1L), 1L << 20);   // (f5_create refuses a bad granule)
    return sw;
}
extern "C" int f5_create(const f5_config* c, f5_engine** out) {
    if (!c || !out) return fail(F5_EINVAL, "f5_create: null argument");
    if (c->dim_head != 64) return fail(F5_EINVAL, "dim_head must be 64 (got %d)", c->dim_head);
    if (c->dim % 256 != 0 || (c->dim / 16 != 16 && c->dim / 16 != 32 && c->dim / 16 != 48 && c->dim / 16 != 64))
        return fail(F5_EINVAL, "dim must be 256, 512, 768 or 1024 (got %d)", c->dim);
    if (c->heads <= 0 || (c->heads * 64) % 64 != 0 || c->depth <= 0) return fail(F5_EINVAL, "bad heads/depth");
    if (c->mel_dim % 4 || c->text_dim % 4 || c->ff_dim % 8) return fail(F5_EINVAL, "mel_dim/text_dim %% 4, ff_dim %% 8 required");
    if ((2 * c->mel_dim + c->text_dim) % 4) return fail(F5_EINVAL, "2*mel_dim + text_dim must be a multiple of 4");
    const PrecInfo prec = prec_info(c->precision);
    if (!prec.valid) return fail(F5_EINVAL, "bad precision");
    if (c->precision == F5_PREC_F16X3 && c->ff_dim % 32)
        return fail(F5_EINVAL, "F5_PREC_F16X3 needs ff_dim %% 32 == 0 (whole 32-element blocks of the split operand layout; got %d)", c->ff_dim);
    if (c->backbone != F5_BACKBONE_DIT && c->backbone != F5_BACKBONE_UNETT && c->backbone != F5_BACKBONE_MMDIT) return fail(F5_EINVAL, "bad backbone");
    if (c->backbone == F5_BACKBONE_UNETT && (c->depth % 2)) return fail(F5_EINVAL, "UNetT depth must be even");
    if (c->text_dim > 2048 || c->dim > 2048) return fail(F5_EINVAL, "dims > 2048 unsupported");
    if (c->options & ~(F5_OPT_QK_RMSNORM | F5_OPT_LONG_SKIP | F5_OPT_TEXT_AVG_UPSAMPLE | F5_OPT_ADAPTERS)) return fail(F5_EINVAL, "unknown option bits %d", c->options);
    if (c->backbone == F5_BACKBONE_MMDIT) {   // mmdit.py:86-99: of the options only qk_norm is a constructor argument
        if (c->options & F5_OPT_LONG_SKIP) return fail(F5_EINVAL, "f5_create: the MMDiT backbone has no long skip connection (F5_OPT_LONG_SKIP is a DiT option)");
        if (c->options & F5_OPT_TEXT_AVG_UPSAMPLE)
            return fail(F5_EINVAL, "f5_create: the MMDiT backbone does not stretch its text to the audio length (F5_OPT_TEXT_AVG_UPSAMPLE is a DiT option)");
        if (c->options & F5_OPT_ADAPTERS) return fail(F5_EINVAL, "f5_create: resident adapters (F5_OPT_ADAPTERS) are built for the DiT backbone, not the MMDiT");
        const char* sc = getenv("F5_SPLIT_CFG");
        if (sc && sc[0] == '1') return fail(F5_EINVAL, "f5_create: F5_SPLIT_CFG=1 steps the DiT's halves as two chains; the MMDiT backbone runs packed CFG only");
    } else if (c->options && c->backbone != F5_BACKBONE_DIT) return fail(F5_EINVAL, "F5_OPT_* are options of the DiT backbone (dit.py:160-166)");
    if ((c->options & F5_OPT_TEXT_AVG_UPSAMPLE) && !c->text_mask_padding)
        return fail(F5_EINVAL, "text_embedding_average_upsampling requires text_mask_padding to be True (dit.py:41-42)");
    if (c->precision == F5_PREC_F8) {
        if (c->backbone != F5_BACKBONE_DIT)
            return fail(F5_EINVAL, "f5_create: F5_PREC_F8 is built for the DiT backbone, not the %s", c->backbone == F5_BACKBONE_UNETT ? "UNetT" : "MMDiT");
        if (c->options & F5_OPT_ADAPTERS)
            return fail(F5_EINVAL, "f5_create: F5_PREC_F8 cannot be combined with F5_OPT_ADAPTERS (a switch merges into packed 16-bit operands; re-quantising on a switch is not built)");
        if (c->heads % 2 || c->ff_dim % 128)
            return fail(F5_EINVAL, "f5_create: F5_PREC_F8 needs every block GEMM's K to be whole 128-element tiles: heads even (heads * 64 = %d) and ff_dim %% 128 == 0 (ff_dim = %d)",
                        c->heads * 64, c->ff_dim);
    }
    f5_engine* e = new f5_engine();
    e->cfg = *c;
    e->inner = c->heads * 64;
    const bool mmdit = c->backbone == F5_BACKBONE_MMDIT;
    if (mmdit) e->cfg.text_dim = c->dim;   // (the text stream has the model's width; f5_config.text_dim is not read)
    if (mmdit) e->cfg.conv_layers = 0;     // (mmdit.py:30-61: no ConvNeXt blocks behind the lookup)
    e->kin = 2 * c->mel_dim + (mmdit ? 0 : c->text_dim);   // mmdit.py:70: the text has no part in the input projection
    e->kin_pad = round_up(e->kin, 64);  // whole 128-byte K-tiles for the LDS-DMA GEMM (pad columns stay zero)
    // per block 6 D (DiT), or x's 6 D then c's 6 D -- 2 D in the last, context_pre_only block -- (MMDiT); then the final norm's 2 D
    e->modN = (mmdit ? 12 * c->depth - 2 : 6 * c->depth + 2) * c->dim;
    e->split16 = prec.split16;
    e->f8 = prec.f8;
    e->io_split = prec.io_split;
    e->sw = read_switches(*c);
    if (!valid_len_bucket(e->sw.len_bucket)) {
        const int g = e->sw.len_bucket;
        delete e;
        return fail(F5_EINVAL, "F5_LEN_BUCKET=%d: the granule is 0 (off) or a multiple of 8 in [8, 1024]", g);
    }
    e->adapters_on = (c->options & F5_OPT_ADAPTERS) != 0;
    if (e->adapters_on && e->sw.x3_ablate) {   // (the ablation zeroes lo halves once, at finalize: a switch would write them back)
        delete e;
        return fail(F5_EINVAL, "F5_OPT_ADAPTERS cannot be combined with the F5_X3_ABLATE diagnostic");
    }
    *out = e;
    return F5_OK;
}
extern "C" int f5_destroy(f5_engine* e) {
    if (e) {
        (void)hipDeviceSynchronize();
        delete e;
    }
    return F5_OK;
}
extern "C" int f5_load_weight(f5_engine* e, const char* name, const void* dev, const int64_t* shape, int32_t ndim,
                              f5_stream stream) {
    if (!e) return fail(F5_EINVAL, "null engine");
    e->finalized = false;
    e->uc_N = -1;
    e->clear_graphs();
    e->active = nullptr;   // the packed weights are about to be rebuilt: adapters made for them are stale
    e->adapt_gen++;
    return e->ws.put("f5_load_weight", name, dev, shape, ndim, (hipStream_t)stream);
}
extern "C" int f5_finalize(f5_engine* e, f5_stream stream) {
    if (!e) return fail(F5_EINVAL, "null engine");
    hipStream_t s = (hipStream_t)stream;
    e->clear_graphs();
    for (void* p : e->owned) (void)hipFree(p);
    e->owned.clear();
    e->pf = Packed<float>();
    e->pb = Packed<bf16_t>();
    e->ph = Packed<f16_t>();
    e->uc_N = -1;
    e->targets.clear();
    e->target_slot.clear();
    e->base_table = nullptr;
    e->active = nullptr;
    e->adapt_gen++;
    int r = F5_OPS(e, finalize(e, s));
    if (r != F5_OK) return r;
    if (e->adapters_on) {   // F5_OPT_ADAPTERS: the masters of the adaptable tensors stay (engine-owned), and so does the table a switch reads
        std::vector<MergeDesc> tab;
        for (auto& t : e->targets) {
            tab.push_back(t.base);
            auto it = e->ws.t.find(t.name);
            e->owned.push_back(it->second.p);
            e->ws.t.erase(it);
        }
        CHK(dev_alloc(e, &e->base_table, tab.size()));
        HIPCHK(hipMemcpy(e->base_table, tab.data(), tab.size() * sizeof(MergeDesc), hipMemcpyHostToDevice));
    }
    HIPCHK(hipStreamSynchronize(s));
    e->ws.clear();   // the raw fp32 copies are no longer needed
    e->finalized = true;
    return F5_OK;
}
int ensure_arena(f5_engine* e, int B, int N, int S) {
    B = std::max(B, e->res_B); N = std::max(N, e->res_N); S = std::max(S, e->res_S);
    const size_t need_b = F5_OPS(e, plan_bytes(e, B, N, S));
    bool replaced = false;
    CHK(e->arena.reserve(need_b, &replaced));
    // a new block or a new reservation (the carve offsets move with it): captured pointers are stale, and so is the cached
    // unconditional text embedding
    if (replaced || B != e->res_B || N != e->res_N || S != e->res_S) {
        e->clear_graphs();
        e->uc_N = -1;
    }
    e->res_B = B; e->res_N = N; e->res_S = S;
    return F5_OK;
}

extern "C" int f5_reserve(f5_engine* e, int32_t B, int32_t N, int32_t S) {
    if (!e || B <= 0 || N <= 0 || S <= 0) return fail(F5_EINVAL, "f5_reserve: bad arguments");
    return ensure_arena(e, B, N, S);
}
// The work-buffer plan of an engine of this config, as pure host arithmetic: the real carve_into and second_half on a dry-run arena.  The
// engine object lives for the call only; no HIP call is made.
extern "C" int f5k_work_plan(const f5_config* c, int32_t B, int32_t N, int32_t S, int32_t call_B, int32_t call_N, int64_t* total_bytes,
                             int64_t* main_off, int64_t* side_off) {
    if (!c || !total_bytes || !main_off || !side_off || B <= 0 || N <= 0 || S <= 0 || call_B <= 0 || call_B > B || call_N <= 0 || call_N > N)
        return fail(F5_EINVAL, "f5k_work_plan: bad arguments (0 < call_B <= B, 0 < call_N <= N, S > 0)");
    f5_engine* e = nullptr;
    CHK(f5_create(c, &e));
    *total_bytes = (int64_t)F5_OPS(e, work_plan(e, B, N, S, call_B, call_N, main_off, side_off));
    delete e;   // (nothing of it ever reached a device: no synchronisation, unlike f5_destroy)
    return F5_OK;
}
// Utterances per backbone call inside sample(): the ODE state of different utterances never interacts, so a large batch
// is stepped in chunks whose activations (x 4 B, xn, q, k, v, ffh 2 B per element: ~17 KB per row) stay inside the 256 MB
// Infinity Cache between the kernels of a block, instead of streaming every intermediate through HBM (C3: 65,536 rows).
// F5_CHUNK_ROWS overrides the row budget (tests force tiny chunks).  F5_SPLIT_CFG=1 steps the whole batch per half.
// With row packing (RowPack) an utterance costs its own length, not the padded one: the budget then counts the rows
// actually present (C3 with attn_mask_enabled: 2 chunks of 16 utterances ~ 22,600 valid rows each).
static int chunk_utts(const f5_engine* e, int B, int N, bool use_cfg, const int32_t* packed_lens) {
    if (e->sw.split_cfg) return B;
    // Equal chunks; how many is chosen by counting ROUNDS of GEMM tiles: a backbone call on R rows runs its N = 1024 GEMMs (out-proj, FF2) in
    // ceil(R / 16,384) rounds of 256 tiles of 256 x 256, so k chunks cost k * ceil(R_chunk / 16,384) rounds; among the cheapest counts
    // the one whose chunks are closest to 32,768 rows wins (the activations of such a chunk stay inside the Infinity Cache).  Measured:
    // C3 padded (65,536 rows; 1 / 2 / 4 chunks all 4 rounds): 4 x 16,384 1,338 ms, **2 x 32,768 1,271**, 1 x 65,536 1,289; C3 with packed rows
    // (45,200 valid rows): 2 x 22,600 (2 x 2 rounds) 1,103 ms, **1 x 45,200 (3 rounds) 1,018** -- round 2's fixed 32,768-row budget
    // chose the former.  F5_CHUNK_ROWS forces a fixed budget instead (tests use tiny chunks).
    long rows_per_utt = (long)(use_cfg ? 2 : 1) * (N + (e->cfg.backbone == F5_BACKBONE_UNETT ? 1 : 0));
    if (packed_lens) {
        long total = 0;
        for (int i = 0; i < B; ++i) total += (packed_lens[i] + 3) / 4 * 4;
        rows_per_utt = std::max(1L, (long)(use_cfg ? 2 : 1) * total / B);
    }
    if (e->sw.chunk_rows) {
        long bc = e->sw.chunk_rows / rows_per_utt;
        if (bc < 1) bc = 1;
        if (bc >= B) return B;
        const long nchunks = (B + bc - 1) / bc;
        return (int)((B + nchunks - 1) / nchunks);   // equal-sized chunks (8 utterances, budget 7 -> 4 + 4, not 7 + 1)
    }
    const long total_rows = rows_per_utt * B;
    const long kmin = std::max(1L, (total_rows + 65535) / 65536), kmax = std::min((long)B, std::max(kmin, total_rows / 12288));
    long best_k = kmin, best_cost = -1, best_dist = 0;
    for (long k = kmin; k <= kmax; ++k) {
        const long per = (B + k - 1) / k, r = per * rows_per_utt;      // utterances / rows of a (full) chunk
        const long kk = (B + per - 1) / per;                           // chunks that size actually gives
        const long cost = kk * ((r + 16383) / 16384);
        const long dist = std::labs(r - 32768);
        if (best_cost < 0 || cost < best_cost || (cost == best_cost && dist < best_dist)) { best_k = kk; best_cost = cost; best_dist = dist; }
    }
    return (int)((B + best_k - 1) / best_k);
}
PlanOptions plan_options(const SampleCall& c) {
    PlanOptions o;
    o.nt = c.nt; o.steps = c.steps; o.method = c.method; o.cfg_strength = c.cfg_strength;
    o.want_traj = c.traj != nullptr;
    if (c.per_item) {
        o.items = true;
        o.U = (int)c.items.rows->times.size();
        bool any_cfg = false;
        for (int b = 0; b < c.B; ++b) any_cfg = any_cfg || !(c.items.cfg_items[b] < 1e-5f);
        o.cfg_strength = any_cfg ? 1.f : 0.f;
    }
    return o;
}
SamplePlan plan_sample(const f5_engine* e, int B, int N, const int32_t* lens_host, const PlanOptions& o) {
    SamplePlan p;
    const int n_true = o.n_true;
    p.items = o.items;
    p.U = o.U;
    // a length-bucket plan: every utterance has n_true frames; the chunking follows the bucket's ceiling alone (it is part of the key)
    const std::vector<int32_t> own(n_true > 0 ? B : 0, n_true), cap(n_true > 0 || o.isolated ? B : 0, N);
    if (n_true > 0) lens_host = own.data();
    p.n_true = n_true;
    p.B = B; p.N = N; p.nt = o.nt; p.steps = o.steps; p.method = o.method; p.cfg_strength = o.cfg_strength;
    p.use_cfg = !(o.cfg_strength < 1e-5f);
    p.has_lens = lens_host != nullptr;
    p.want_traj = o.want_traj;
    p.halves = p.use_cfg ? 2 : 1;
    p.evals = o.method == F5_ODE_MIDPOINT ? 2 : 1;
    const bool dit = e->cfg.backbone == F5_BACKBONE_DIT;   // (the MMDiT runs rectangular on one chain: never packed, never split)
    // (a per-item call runs on one stream chain, and on the rectangular body -- batch row = row / N finds a row's time vectors -- unless
    //  it is isolated: then on packed rows, whatever F5_PACK_ROWS says, and the rowmap's batch row finds them)
    p.bucket = o.isolated && o.bucket;
    p.pack = o.isolated || (!o.items && (n_true > 0 || (p.has_lens && e->sw.pack_rows && e->cfg.attn_mask_enabled && dit && !e->sw.split_cfg)));
    p.split = !o.items && e->sw.split_cfg && p.use_cfg && dit && !e->prof.on;
    // (an isolated plan's key holds no length, so its chunking follows N alone, as a bucket plan's does)
    p.chunk = o.chunk ? o.chunk : chunk_utts(e, B, N, p.use_cfg, n_true > 0 || o.isolated ? cap.data() : p.pack ? lens_host : nullptr);
    for (int u0 = 0; u0 < B; u0 += p.chunk) {
        SamplePlan::Chunk k{(int)p.chunks.size(), u0, std::min(p.chunk, B - u0), 0, 0};
        for (int i = 0; lens_host && i < k.bc; ++i) {
            k.rows += (double)p.halves * round_up(lens_host[u0 + i], 4);
            k.sq += (double)p.halves * lens_host[u0 + i] * lens_host[u0 + i];
        }
        p.chunks.push_back(k);
    }
    return p;
}
// the signature a captured sample() body is cached under (F5_TRACE prints it; tools/pmc_one.py reads it)
std::string graph_key(const SamplePlan& p) {
    unsigned cfg_bits;
    memcpy(&cfg_bits, &p.cfg_strength, 4);
    char kb[160];
    // a per-item plan: guidance and grids live in device tables, so neither is part of the key -- one graph serves every setting of a shape
    // an isolated per-item plan: packed rows, every length in device tables; N is the bucket's ceiling and U the power-of-two ceiling of the
    // call's distinct times, so neither the call's own N, nor a length, nor its text length (the staging capacity; exact without buckets,
    // and then part of the key) is in it
    if (p.items && p.pack) {
        int n = snprintf(kb, sizeof(kb), "P%d|%d|%d|U%d|h%d|%d|%d|m%d", p.B, p.N, p.steps, p.U, p.halves, p.want_traj ? 1 : 0, p.chunk, p.method);
        if (!p.bucket) snprintf(kb + n, sizeof(kb) - n, "|t%d", p.nt);
        return kb;
    }
    if (p.items) {
        snprintf(kb, sizeof(kb), "I%d|%d|%d|%d|U%d|h%d|%d|%d|%d|m%d", p.B, p.N, p.nt, p.steps, p.U, p.halves, p.has_lens ? 1 : 0,
                 p.want_traj ? 1 : 0, p.chunk, p.method);
        return kb;
    }
    // a length-bucket plan: the bucket's ceiling stands for N, and neither the call's own length nor its text length is part of the key
    if (p.n_true > 0) snprintf(kb, sizeof(kb), "L%d|%d|%d|%08x|%d|%d|m%d", p.B, p.N, p.steps, cfg_bits, p.want_traj ? 1 : 0, p.chunk, p.method);
    else
    snprintf(kb, sizeof(kb), "%d|%d|%d|%d|%08x|%d|%d|%d|m%d", p.B, p.N, p.nt, p.steps, cfg_bits, p.has_lens ? 1 : 0, p.want_traj ? 1 : 0,
             p.chunk, p.method);
    return kb;
}
// What sample() uploads to Work::tdev: the evaluation times (one feature row each), then the grid t[0..steps].  Euler evaluates at
// t[0..steps-1], which IS the grid's head; midpoint at t[i] (row 2i) and t[i] + dt/2 (row 2i+1), and the grid follows at 2 steps.
std::vector<float> time_table(const float* t_host, int steps, int method) {
    std::vector<float> tt;
    for (int i = 0; method == F5_ODE_MIDPOINT && i < steps; ++i) {
        const float hdt = 0.5f * (t_host[i + 1] - t_host[i]);   // f32, in torchdiffeq's order
        tt.push_back(t_host[i]);
        tt.push_back(t_host[i] + hdt);
    }
    tt.insert(tt.end(), t_host, t_host + steps + 1);
    return tt;
}
ItemTimeRows item_time_rows(const float* t_items, const int32_t* steps_items, int steps_max, int B, int method) {
    const int evals = method == F5_ODE_MIDPOINT ? 2 : 1;
    ItemTimeRows r;
    r.idx.assign((size_t)evals * steps_max * B, 0);
    std::map<uint32_t, int> seen;   // f32 bit pattern -> row
    for (int ev = 0; ev < evals * steps_max; ++ev)
        for (int b = 0; b < B; ++b) {
            const int i = ev / evals;
            if (i >= steps_items[b]) continue;
            const float* t = t_items + (size_t)b * (steps_max + 1);
            float v = t[i];
            if (ev % evals) {
                const float hdt = 0.5f * (t[i + 1] - t[i]);   // f32, in time_table's order
                v = t[i] + hdt;
            }
            uint32_t bits;
            memcpy(&bits, &v, 4);
            auto it = seen.find(bits);
            if (it == seen.end()) {
                it = seen.emplace(bits, (int)r.times.size()).first;
                r.times.push_back(v);
            }
            r.idx[(size_t)ev * B + b] = it->second;
        }
    return r;
}
// the argument rules of the per-item tables (f5_sample_items, f5k_item_time_rows); messages name the item
static int check_items(const char* who, const float* t_items, const int32_t* steps_items, int steps_max, const float* cfg_items, int B,
                       int method) {
    if (method != F5_ODE_EULER && method != F5_ODE_MIDPOINT)
        return fail(F5_EINVAL, "%s: unknown ODE method %d (F5_ODE_EULER = 0, F5_ODE_MIDPOINT = 1)", who, method);
    if (!t_items || !steps_items || B <= 0 || steps_max <= 0) return fail(F5_EINVAL, "%s: bad arguments", who);
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        if (steps_items[b] < 1 || steps_items[b] > steps_max)
            return fail(F5_EINVAL, "%s: item %d: steps_items = %d outside [1, steps_max = %d]", who, b, steps_items[b], steps_max);
        mx = std::max(mx, steps_items[b]);
        for (int i = 0; i <= steps_items[b]; ++i)
            if (!std::isfinite(t_items[(size_t)b * (steps_max + 1) + i]))
                return fail(F5_EINVAL, "%s: item %d: t_items[%d] is not finite", who, b, i);
        if (cfg_items && !std::isfinite(cfg_items[b])) return fail(F5_EINVAL, "%s: item %d: cfg_items is not finite", who, b);
    }
    if (mx != steps_max) return fail(F5_EINVAL, "%s: the largest steps_items is %d, not steps_max = %d", who, mx, steps_max);
    return F5_OK;
}
extern "C" int f5k_item_time_rows(const float* t_items, const int32_t* steps_items, int32_t steps_max, int32_t B, int32_t method,
                                  float* times_out, int32_t* idx_out, int32_t* U) {
    if (!times_out || !idx_out || !U) return fail(F5_EINVAL, "f5k_item_time_rows: bad arguments");
    CHK(check_items("f5k_item_time_rows", t_items, steps_items, steps_max, nullptr, B, method));
    const ItemTimeRows r = item_time_rows(t_items, steps_items, steps_max, B, method);
    std::copy(r.times.begin(), r.times.end(), times_out);
    std::copy(r.idx.begin(), r.idx.end(), idx_out);
    *U = (int32_t)r.times.size();
    return F5_OK;
}
static int check_ready(const char* who, f5_engine* e, int B, int N) {
    if (!e) return fail(F5_EINVAL, "%s: null engine", who);
    if (!e->finalized) return fail(F5_ESTATE, "%s: f5_finalize has not been called", who);
    if (B <= 0 || N <= 0) return fail(F5_EINVAL, "%s: B and N must be positive", who);
    if (N + 1 > e->cfg.max_pos) return fail(F5_EINVAL, "%s: N=%d exceeds the rotary table (%d rows)", who, N, e->cfg.max_pos);
    return F5_OK;
}
// the MMDiT's text positions come from a sinus table of 1024 rows (mmdit.py:37-38)
static int check_mmdit_text(const char* who, const f5_engine* e, int nt) {
    if (e->cfg.backbone == F5_BACKBONE_MMDIT && nt > 1024)
        return fail(F5_EINVAL, "%s: nt=%d exceeds the MMDiT text position table (1024 rows)", who, nt);
    return F5_OK;
}
extern "C" int f5_text_embed(f5_engine* e, const int64_t* text, int32_t B, int32_t nt, const int32_t* lens_host,
                             int32_t N, int32_t drop_text, float* out, f5_stream stream) {
    CHK(check_ready("f5_text_embed", e, B, N));
    if (!text || !out || nt <= 0) return fail(F5_EINVAL, "f5_text_embed: bad arguments");
    CHK(check_mmdit_text("f5_text_embed", e, nt));
    hipStream_t s = (hipStream_t)stream;
    return F5_OPS(e, text_embed(e, text, B, nt, lens_host, N, drop_text, out, s));
}
extern "C" int f5_dit_forward(f5_engine* e, const float* x, const float* cond, const int64_t* text, int32_t nt,
                              const float* time_host, const int32_t* lens_host, int32_t B, int32_t N, int32_t cfg_infer,
                              int32_t drop_audio_cond, int32_t drop_text, float* out, f5_stream stream) {
    CHK(check_ready("f5_dit_forward", e, B, N));
    if (!x || !cond || !text || !time_host || !out || nt <= 0) return fail(F5_EINVAL, "f5_dit_forward: bad arguments");
    CHK(check_mmdit_text("f5_dit_forward", e, nt));
    hipStream_t s = (hipStream_t)stream;
    return F5_OPS(e, forward(e, x, cond, text, nt, time_host, lens_host, B, N, cfg_infer, drop_audio_cond, drop_text, out, s));
}
int check_flow_spans(const char* who, const int32_t* span_host, const int32_t* lens_host, int B, int N) {
    if (!span_host || B <= 0 || N <= 0) return fail(F5_EINVAL, "%s: bad arguments", who);
    for (int b = 0; b < B; ++b) {
        const int len = lens_host ? lens_host[b] : N, s0 = span_host[2 * b], s1 = span_host[2 * b + 1];
        if (len <= 0 || len > N) return fail(F5_EINVAL, "%s: lens[%d]=%d out of (0, N]", who, b, len);
        if (s0 < 0 || s0 > s1 || s1 > len)
            return fail(F5_EINVAL, "%s: item %d: span = [%d, %d) outside 0 <= start <= end <= %d frames", who, b, s0, s1, len);
    }
    return F5_OK;
}
// First what needs no engine (the tables: times, lengths, spans; messages name the item), then the engine, then pointers.
extern "C" int f5_flow_loss(f5_engine* e, const float* x1, const float* x0, const int64_t* text, int32_t nt, const float* time_host,
                            const int32_t* lens_host, const int32_t* span_host, int32_t B, int32_t N, int32_t drop_audio_cond,
                            int32_t drop_text, double* sq_sum, int32_t* count, float* pred, float* cond, float* frame_err, f5_stream stream) {
    if (!time_host || B <= 0 || B > 65535 || N <= 0) return fail(F5_EINVAL, "f5_flow_loss: bad arguments (0 < B <= 65535, N > 0)");
    for (int b = 0; b < B; ++b)
        if (!std::isfinite(time_host[b])) return fail(F5_EINVAL, "f5_flow_loss: item %d: time is not finite", b);
    CHK(check_flow_spans("f5_flow_loss", span_host, lens_host, B, N));
    CHK(check_ready("f5_flow_loss", e, B, N));
    if (!x1 || !x0 || !text || !sq_sum || !count || nt <= 0) return fail(F5_EINVAL, "f5_flow_loss: bad arguments");
    CHK(check_mmdit_text("f5_flow_loss", e, nt));
    hipStream_t s = (hipStream_t)stream;
    return F5_OPS(e, flow_loss(e, x1, x0, text, nt, time_host, lens_host, span_host, B, N, drop_audio_cond, drop_text, sq_sum, count, pred,
                               cond, frame_err, s));
}
// the rules of a slice's row table (f5_sample_span, f5k_span_stage); messages name the item
int check_span_rows(const char* who, const int32_t* rows_host, int B, const void* prev_state, int prev_B, int prev_N, const void* y_new) {
    if (!rows_host || B <= 0) return fail(F5_EINVAL, "%s: bad arguments", who);
    std::vector<char> taken(prev_B > 0 ? prev_B : 0, 0);
    for (int b = 0; b < B; ++b) {
        const int r = rows_host[b];
        if (r < -1 || r >= std::max(prev_B, 0))
            return fail(F5_EINVAL, "%s: item %d: rows = %d outside [-1, prev_B = %d)", who, b, r, prev_B);
        if (r < 0) {
            if (!y_new) return fail(F5_EINVAL, "%s: item %d begins here (rows = -1) but y_new is NULL", who, b);
            continue;
        }
        if (!prev_state || prev_N <= 0)
            return fail(F5_EINVAL, "%s: item %d continues row %d but there is no previous state (prev_state NULL or prev_N < 1)", who, b, r);
        if (taken[r]) return fail(F5_EINVAL, "%s: item %d: row %d of the previous state is named twice", who, b, r);
        taken[r] = 1;
    }
    return F5_OK;
}
// The argument rules of a sampler call; every message begins with the entry point's name.  First what needs no engine (the method, the
// per-item tables, a slice's rows), then the engine, then pointers and lengths.
static int check_sample_call(f5_engine* e, const SampleCall& c) {
    if (c.per_item) {
        if (c.span && c.steps < 1) return fail(F5_EINVAL, "%s: count = %d (a slice runs at least one step)", c.who, c.steps);
        if (!c.items.cfg_items) return fail(F5_EINVAL, "%s: bad arguments", c.who);
        CHK(check_items(c.who, c.items.t_items, c.items.steps_items, c.steps, c.items.cfg_items, c.B, c.method));
    } else if (c.method != F5_ODE_EULER && c.method != F5_ODE_MIDPOINT)
        return fail(F5_EINVAL, "%s: unknown ODE method %d (F5_ODE_EULER = 0, F5_ODE_MIDPOINT = 1)", c.who, c.method);
    if (c.span) CHK(check_span_rows(c.who, c.rows_host, c.B, c.prev_state, c.prev_B, c.prev_N, c.y_new));
    CHK(check_ready(c.who, e, c.B, c.N));
    const bool times_ok = c.per_item || (c.t_host && c.steps > 0);
    const bool ends_ok = c.span ? c.state_out != nullptr : c.y0 != nullptr;   // (a slice's start state: check_span_rows; a trajectory may be NULL)
    if ((!c.cond && c.cond_frames > 0) || !c.cond_mask || !c.text || !c.out || !times_ok || !ends_ok || c.nt <= 0 || c.cond_frames < 0 ||
        c.cond_frames > c.N)
        return fail(F5_EINVAL, "%s: bad arguments", c.who);
    if (c.B > 1 && !c.lens_host) return fail(F5_EINVAL, "%s: lens required when B > 1 (cfm.py:155-158)", c.who);
    for (int i = 0; c.lens_host && i < c.B; ++i)
        if (c.lens_host[i] <= 0 || c.lens_host[i] > c.N) return fail(F5_EINVAL, "%s: lens[%d]=%d out of (0, N]", c.who, i, c.lens_host[i]);
    return F5_OK;
}
static int run_sample_call(f5_engine* e, SampleCall& c) {
    if (e && c.per_item && e->cfg.backbone == F5_BACKBONE_MMDIT)
        return fail(F5_EINVAL, "%s: per-item and sliced solves are built for the DiT and UNetT backbones, not the MMDiT", c.who);
    CHK(check_sample_call(e, c));
    CHK(check_mmdit_text(c.who, e, c.nt));
    ItemTimeRows rows;
    if (c.per_item) {
        rows = item_time_rows(c.items.t_items, c.items.steps_items, c.steps, c.B, c.method);
        c.items.rows = &rows;
    }
    e->prof.clear();
    return F5_OPS(e, run_sample(e, c));
}
static void per_item_times(SampleCall& c, const float* t_items, const int32_t* steps_items, int steps_max, const float* cfg_items) {
    c.per_item = true;
    c.items.t_items = t_items; c.items.steps_items = steps_items; c.items.cfg_items = cfg_items;
    c.steps = steps_max;
}
static int sample_uniform(const char* who, f5_engine* e, const float* cond, int cond_frames, const uint8_t* cond_mask, const float* y0,
                          const int64_t* text, int nt, const float* t_host, int steps, float cfg_strength, const int32_t* lens_host, int B,
                          int N, float* out, float* traj, f5_stream stream, int method) {
    SampleCall c{who, cond, cond_frames, cond_mask, text, nt, lens_host, B, N, out, (hipStream_t)stream, method};
    c.t_host = t_host; c.steps = steps; c.cfg_strength = cfg_strength;
    c.y0 = y0;
    c.traj = traj;
    return run_sample_call(e, c);
}
extern "C" int f5_sample_ode(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y0,
                             const int64_t* text, int32_t nt, const float* t_host, int32_t steps, float cfg_strength,
                             const int32_t* lens_host, int32_t B, int32_t N, float* out, float* traj, f5_stream stream,
                             int32_t method) {
    return sample_uniform("f5_sample_ode", e, cond, cond_frames, cond_mask, y0, text, nt, t_host, steps, cfg_strength, lens_host, B, N, out,
                          traj, stream, method);
}
extern "C" int f5_sample(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y0,
                         const int64_t* text, int32_t nt, const float* t_host, int32_t steps, float cfg_strength,
                         const int32_t* lens_host, int32_t B, int32_t N, float* out, float* traj, f5_stream stream) {
    return sample_uniform("f5_sample", e, cond, cond_frames, cond_mask, y0, text, nt, t_host, steps, cfg_strength, lens_host, B, N, out, traj,
                          stream, F5_ODE_EULER);
}
extern "C" int f5_sample_items(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y0,
                               const int64_t* text, int32_t nt, const float* t_items, const int32_t* steps_items, int32_t steps_max,
                               const float* cfg_items, const int32_t* lens_host, int32_t B, int32_t N, float* out, float* traj,
                               f5_stream stream, int32_t method) {
    SampleCall c{"f5_sample_items", cond, cond_frames, cond_mask, text, nt, lens_host, B, N, out, (hipStream_t)stream, method};
    per_item_times(c, t_items, steps_items, steps_max, cfg_items);
    c.y0 = y0;
    c.traj = traj;
    return run_sample_call(e, c);
}
extern "C" int f5_sample_span(f5_engine* e, const float* cond, int32_t cond_frames, const uint8_t* cond_mask, const float* y_new,
                              const float* prev_state, int32_t prev_B, int32_t prev_N, const int32_t* rows_host, const int64_t* text,
                              int32_t nt, const float* t_items, const int32_t* steps_items, int32_t count, const float* cfg_items,
                              const int32_t* lens_host, int32_t B, int32_t N, float* out, float* state_out, f5_stream stream,
                              int32_t method) {
    SampleCall c{"f5_sample_span", cond, cond_frames, cond_mask, text, nt, lens_host, B, N, out, (hipStream_t)stream, method};
    per_item_times(c, t_items, steps_items, count, cfg_items);
    c.span = true;
    c.y_new = y_new; c.prev_state = prev_state; c.prev_B = prev_B; c.prev_N = prev_N; c.rows_host = rows_host;
    c.state_out = state_out;
    return run_sample_call(e, c);
}

extern "C" int f5k_mmdit_taps(f5_engine* e, float* taps) {
    if (!e) return fail(F5_EINVAL, "f5k_mmdit_taps: null engine");
    if (e->cfg.backbone != F5_BACKBONE_MMDIT) return fail(F5_EINVAL, "f5k_mmdit_taps: the engine's backbone is not the MMDiT");
    e->mm_taps = taps;
    return F5_OK;
}

// ------------------------------------------------------------------------------------- length buckets
extern "C" int f5_set_length_buckets(f5_engine* e, int32_t granule) {
    if (!e) return fail(F5_EINVAL, "null engine");
    if (!valid_len_bucket(granule))
        return fail(F5_EINVAL, "f5_set_length_buckets: granule %d is neither 0 (off) nor a multiple of 8 in [8, 1024]", granule);
    if (granule && e->cfg.backbone == F5_BACKBONE_MMDIT)
        return fail(F5_EINVAL, "f5_set_length_buckets: length buckets run on packed rows, which the MMDiT backbone does not have");
    e->sw.len_bucket = granule;
    e->clear_graphs();
    e->gc.capacity = GraphCache::DEFAULT_CAPACITY;
    return F5_OK;
}
extern "C" int f5_set_isolated_rows(f5_engine* e, int32_t on) {
    if (!e) return fail(F5_EINVAL, "f5_set_isolated_rows: null engine");
    if (on && e->cfg.backbone == F5_BACKBONE_MMDIT)
        return fail(F5_EINVAL, "f5_set_isolated_rows: isolated rows run on packed rows, which the MMDiT backbone does not have");
    e->sw.isolated_rows = on != 0;   // (the keys of isolated and rectangular plans differ: no graph goes stale)
    return F5_OK;
}
extern "C" int f5_set_graph_capacity(f5_engine* e, int32_t n) {
    if (!e) return fail(F5_EINVAL, "f5_set_graph_capacity: null engine");
    if (n < GraphCache::DEFAULT_CAPACITY || n > GraphCache::MAX_CAPACITY)
        return fail(F5_EINVAL, "f5_set_graph_capacity: %d graphs outside [%d, %d]", n, (int)GraphCache::DEFAULT_CAPACITY,
                    (int)GraphCache::MAX_CAPACITY);
    e->gc.capacity = (size_t)n;
    while (e->gc.graphs.size() > e->gc.capacity) {   // oldest out first, as a capture makes room
        e->gc.evict(0);
        e->gc.stats.evictions++;
    }
    return F5_OK;
}
extern "C" int f5_prepare_sample(f5_engine* e, int32_t B, int32_t n_min, int32_t n_max, int32_t nt_max, int32_t steps, float cfg_strength,
                                 int32_t method, int32_t want_traj, f5_stream stream) {
    if (!e) return fail(F5_EINVAL, "null engine");
    if (!e->finalized) return fail(F5_ESTATE, "f5_finalize has not been called");
    const int g = e->sw.len_bucket;
    if (g <= 0) return fail(F5_ESTATE, "f5_prepare_sample needs length buckets: call f5_set_length_buckets (or set F5_LEN_BUCKET) first");
    if (method != F5_ODE_EULER && method != F5_ODE_MIDPOINT)
        return fail(F5_EINVAL, "f5_prepare_sample: unknown ODE method %d (F5_ODE_EULER = 0, F5_ODE_MIDPOINT = 1)", method);
    if (B <= 0 || n_min <= 0 || n_max < n_min || nt_max <= 0 || steps <= 0)
        return fail(F5_EINVAL, "f5_prepare_sample: bad arguments (B %d, lengths %d .. %d, text %d, steps %d)", B, n_min, n_max, nt_max, steps);
    if (round_up(n_max, g) + 1 > e->cfg.max_pos)
        return fail(F5_EINVAL, "f5_prepare_sample: n_max=%d is planned at %d frames, which exceeds the rotary table (%d rows)", n_max,
                    round_up(n_max, g), e->cfg.max_pos);
    const int count = (round_up(n_max, g) - round_up(n_min, g)) / g + 1;
    if (count > GraphCache::MAX_CAPACITY)
        return fail(F5_EINVAL, "f5_prepare_sample: lengths %d .. %d at granule %d are %d buckets; the graph cache holds at most %d", n_min,
                    n_max, g, count, (int)GraphCache::MAX_CAPACITY);
    if (e->cfg.backbone != F5_BACKBONE_DIT) return fail(F5_EINVAL, "f5_prepare_sample: length buckets are built for the DiT backbone");
    if (e->sw.split_cfg || e->prof.on || (e->cfg.options & F5_OPT_TEXT_AVG_UPSAMPLE))
        return fail(F5_ESTATE, "f5_prepare_sample: no sample() call of this engine is eligible for a length bucket (F5_SPLIT_CFG, the "
                               "profiler or text_embedding_average_upsampling is on)");
    if (!e->sw.graphs || e->gc.disabled) return fail(F5_ESTATE, "f5_prepare_sample: HIP graphs are off (F5_HIP_GRAPH=0, or a capture failed)");
    (void)stream;   // nothing is enqueued: capture and instantiation are host work
    return F5_OPS(e, prepare(e, B, n_min, n_max, nt_max, steps, cfg_strength, method, want_traj != 0));
}
extern "C" int f5_graph_stats(f5_engine* e, int32_t* out) {
    if (!e) return fail(F5_EINVAL, "null engine");
    GraphCache::Stats& st = e->gc.stats;
    if (!out) {
        st = GraphCache::Stats();
        return F5_OK;
    }
    out[0] = st.captures; out[1] = st.replays; out[2] = st.eager; out[3] = st.evictions;
    return F5_OK;
}

extern "C" int f5_profile_enable(f5_engine* e, int32_t on) {
    if (!e) return fail(F5_EINVAL, "null engine");
    e->prof.on = on != 0;
    e->prof.clear();
    return F5_OK;
}
extern "C" int f5_profile_read(f5_engine* e, float* ms, int32_t* launches, double* flops, int32_t ncls) {
    if (!e || !ms || !launches) return fail(F5_EINVAL, "f5_profile_read: bad arguments");
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < ncls; ++i) {
        ms[i] = 0.f;
        launches[i] = 0;
        if (flops) flops[i] = 0.0;
    }
    for (int i = 0; i * 2 + 1 < e->prof.used; ++i) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, e->prof.ev[2 * i], e->prof.ev[2 * i + 1]));
        const int cidx = e->prof.cls[i];
        if (cidx < ncls) {
            ms[cidx] += t;
            launches[cidx] += 1;
            if (flops) flops[cidx] += e->prof.flops[i];
        }
    }
    return F5_OK;
}
