// Per-precision body of the engine (template definitions; included by engine_bf16.hip / engine_f16.hip / engine_f32.hip,
// each of which instantiates EngineOps<T> for one operand type).
#pragma once
#include "engine_types.h"
#include "quant8.h"

// --------------------------------------------------------------------------------------------- finalize
static int need(const WeightStore& ws, const std::string& n, std::initializer_list<int64_t> shape, const Tensor** out) {
    const Tensor* t = ws.get(n);
    if (!t) return fail(F5_ESTATE, "missing weight '%s'", n.c_str());
    std::vector<int64_t> want(shape);
    if (t->shape != want) {
        std::string got, exp;
        for (auto s : t->shape) got += std::to_string(s) + ",";
        for (auto s : want) exp += std::to_string(s) + ",";
        return fail(F5_EINVAL, "weight '%s' has shape [%s], expected [%s]", n.c_str(), got.c_str(), exp.c_str());
    }
    *out = t;
    return F5_OK;
}

// F5_PREC_F16X3: the backbone's GEMM weights (BB) are stored split into f16 hi / lo halves (elementwise.h split_planar_kernel)
template <typename T, bool BB> static int maybe_split_weight(f5_engine* e, hipStream_t s, T* w, size_t elems) {
    if constexpr (BB && std::is_same_v<T, float>) {
        if (e->split16 || e->io_split) {
            hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)(elems / 32))), dim3(256), 0, s, w, (long)(elems / 32));
            HIPCHK(hipGetLastError());
        }
    }
    return F5_OK;
}
// diagnostic F5_X3_ABLATE: a split-planar f32 operand (weights at finalize, a class's A operand in the forward) as plain f16 -- the lo
// halves of its 32-element blocks zeroed.  Only the float engine has such operands.
template <typename T> static void zero_lo_planar(hipStream_t s, T* p, size_t elems) {
    if constexpr (std::is_same_v<T, float>) {
        const long blocks = (long)(elems / 32);
        hipLaunchKernelGGL(zero_lo_planar_kernel, dim3(ew_blocks(blocks * 4)), dim3(256), 0, s, p, blocks);
    }
}
// the conv position embedding runs split too where its K blocks stay inside one tap (32 | channels per group: dim 512, 1024)
static inline bool conv_split(const f5_engine* e) { return e->split16 && convpos_can_split(e->cfg.dim); }
// every backbone GEMM goes through here (the time / text paths call launch_gemm<float> directly: always plain f32)
template <typename T, typename Epi>
static hipError_t egemm(const f5_engine* e, hipStream_t s, const T* A, int lda, const T* W, int ldw, int M, int N, int K, const Epi& epi,
                        const int* m_limit = nullptr, int m_hint = 0, bool a_split = false) {
    // a_split: the A operand was written pre-split by its producer (store4_planar: LayerNorm, attention, the GELU epilogue)
    const GemmOperands ops = !(std::is_same_v<T, float> && e->split16) ? GemmOperands::Plain : a_split ? GemmOperands::AWSplit : GemmOperands::WSplit;
    return launch_gemm<T>(s, A, lda, W, ldw, M, N, K, epi, {ops, -1, m_limit, m_hint});
}

// What a packed GEMM weight is for; with the engine's precision it decides the operand form.  Backbone: one of the backbone's own GEMM
// weights, split under F5_PREC_F16X3 (maybe_split_weight).  Block: one of the four GEMMs of a block -- a backbone weight, and under
// F5_PREC_F8 e4m3 codes + one scale byte per output channel, quantised from the f32 master (quant8.h), with no 16-bit copy (L->w stays null).
enum class WRole { Other, Backbone, Block };
// The linears pfx[i] + ".weight" [Ni, K] (+ ".bias"), concatenated row-wise, as one operand L [n Ni, ldw]: rows of T zero-padded to
// round_up(K, 64) elements, or e4m3 rows zero-padded to whole K-tiles.
template <typename T, WRole R = WRole::Other>
static int pack_concat(f5_engine* e, hipStream_t s, const std::vector<std::string>& pfx, int Ni, int K, LinW<T>* L, bool bias = true) {
    const int n = (int)pfx.size();
    const bool q8 = R == WRole::Block && e->f8;
    L->N = n * Ni;
    L->K = K;
    L->ldw = q8 ? round_up(K, GEMM_ROW_BYTES) : round_up(K, 64);
    if (q8) {   // (a channel's scale is its own row's, so the parts quantise independently; EpiScale8::col reads the scales as words)
        if (K % 4 || (n > 1 && Ni % 4)) return fail(F5_EINVAL, "F5_PREC_F8: weight '%s' [%d x %d, %d] cannot be packed as e4m3 rows", pfx[0].c_str(), n, Ni, K);
        L->q.pitch = L->ldw;
        CHK(dev_alloc(e, &L->q.codes, (size_t)L->N * L->ldw));
        CHK(dev_alloc(e, &L->q.scales, (size_t)round_up(L->N, 4)));
    } else {
        CHK(dev_alloc(e, &L->w, (size_t)L->N * L->ldw));
    }
    L->b = nullptr;
    if (bias) CHK(dev_alloc(e, &L->b, (size_t)L->N));
    for (int i = 0; i < n; ++i) {
        const Tensor *w = nullptr, *b = nullptr;
        CHK(need(e->ws, pfx[i] + ".weight", {Ni, K}, &w));
        if (q8)
            launch_quant_rows_e4m3<float>(s, w->p, K, Ni, K, L->q.from_row((size_t)i * Ni), nullptr);
        else
            hipLaunchKernelGGL((cast_pad_kernel<T>), dim3(ew_blocks((long)Ni * L->ldw)), dim3(256), 0, s, w->p, K, Ni, K,
                               L->w + (size_t)i * Ni * L->ldw, L->ldw, Ni);
        if (bias) {
            CHK(need(e->ws, pfx[i] + ".bias", {Ni}, &b));
            HIPCHK(hipMemcpyAsync(L->b + (size_t)i * Ni, b->p, (size_t)Ni * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    HIPCHK(hipGetLastError());
    if (q8) return F5_OK;
    return maybe_split_weight<T, R != WRole::Other>(e, s, L->w, (size_t)L->N * L->ldw);
}
// one linear `name`.weight [N, K] (+ .bias)
template <typename T, WRole R = WRole::Other>
static int pack_linear(f5_engine* e, hipStream_t s, const std::string& name, int N, int K, LinW<T>* L, bool bias = true) {
    return pack_concat<T, R>(e, s, std::vector<std::string>{name}, N, K, L, bias);
}

static int copy_vec(f5_engine* e, hipStream_t s, const std::string& name, std::initializer_list<int64_t> shape,
                    float** out) {
    const Tensor* t = nullptr;
    CHK(need(e->ws, name, shape, &t));
    CHK(dev_alloc(e, out, t->numel()));
    HIPCHK(hipMemcpyAsync(*out, t->p, t->numel() * sizeof(float), hipMemcpyDeviceToDevice, s));
    return F5_OK;
}

// F5_OPT_ADAPTERS: records one adaptable tensor as it is packed -- where its fp32 master lives and where (and in which layout) its
// packed form went -- for f5_adapter_put_* / f5_set_adapter (adapter.hip).  dst1: a second packed copy of the same tensor.
template <typename T> static int merge_kind(const f5_engine* e) {
    if constexpr (std::is_same_v<T, float>) return e->split16 ? MK_PLANAR : MK_F32;
    return std::is_same_v<T, bf16_t> ? MK_BF16 : MK_F16;
}
static int reg_target(f5_engine* e, const std::string& name, bool lowrank, int out, int in, int ldw, void* dst0, int kind0,
                      void* dst1 = nullptr, int kind1 = MK_NONE) {
    if (!e->adapters_on) return F5_OK;
    const Tensor* t = e->ws.get(name);
    if (!t) return fail(F5_ESTATE, "missing weight '%s'", name.c_str());
    if (kind0 != MK_TAPS && (in % 4 || ldw % 4 || ((kind0 == MK_PLANAR || kind1 == MK_PLANAR) && ldw % 32)))
        return fail(F5_EINVAL, "F5_OPT_ADAPTERS: '%s' [%d, %d] (row pitch %d) is not made of whole groups of four columns", name.c_str(), out, in, ldw);
    if (e->targets.size() >= MERGE_TABLE_BIT) return fail(F5_EINVAL, "F5_OPT_ADAPTERS: more than %d adaptable tensors", MERGE_TABLE_BIT);
    AdaptTarget a;
    a.name = name;
    a.shape = t->shape;
    a.lowrank = lowrank;
    a.base.W = t->p;
    a.base.A = a.base.B = nullptr;
    a.base.dst0 = dst0;
    a.base.dst1 = dst1;
    a.base.out = out; a.base.in = in; a.base.ldw = ldw; a.base.rank = 0;
    a.base.scale = 0.f;
    a.base.kind0 = kind0; a.base.kind1 = kind1; a.base.pad = 0;
    e->target_slot[name] = (int)e->targets.size();
    e->targets.push_back(a);
    return F5_OK;
}
static int reg_linear_f32(f5_engine* e, const std::string& p, const LinW<float>& L, int N, int K) {   // a text-encoder Linear: weight + bias
    CHK(reg_target(e, p + ".weight", false, N, K, L.ldw, L.w, MK_F32));
    return reg_target(e, p + ".bias", false, 1, N, N, L.b, MK_F32);
}

// One stream's weights of the block whose attention module is `at`: to_q / to_k / to_v + sfx fused, the out-projection `out`, the
// feed-forward `ff` and (qk_norm) the gains at + norm + "q_norm" / "k_norm".  pre_only: the stream ends in this block's attention.
template <typename T>
static int pack_stream(f5_engine* e, hipStream_t s, StreamW<T>& w, const std::string& at, const std::string& sfx, const std::string& out,
                       const std::string& ff, const std::string& norm, bool pre_only) {
    const int D = e->cfg.dim, F = e->cfg.ff_dim, inner = e->inner;
    constexpr WRole blk = WRole::Block;   // (the four e4m3 operands of F5_PREC_F8)
    CHK((pack_concat<T, blk>(e, s, {at + ".to_q" + sfx, at + ".to_k" + sfx, at + ".to_v" + sfx}, inner, D, &w.qkv)));
    if (!pre_only) {
        CHK((pack_linear<T, blk>(e, s, out, D, inner, &w.out)));
        CHK((pack_linear<T, blk>(e, s, ff + ".ff.0.0", F, D, &w.ff1)));
        CHK((pack_linear<T, blk>(e, s, ff + ".ff.2", D, F, &w.ff2)));
    }
    if (e->cfg.options & F5_OPT_QK_RMSNORM) {
        CHK(copy_vec(e, s, norm + "q_norm.weight", {64}, &w.qn));
        CHK(copy_vec(e, s, norm + "k_norm.weight", {64}, &w.kn));
    }
    return F5_OK;
}

template <typename T> static int finalize_t(f5_engine* e, Packed<T>& P, hipStream_t s) {
    const f5_config& c = e->cfg;
    const int D = c.dim, Dt = c.text_dim, inner = e->inner, mel = c.mel_dim;
    const bool dit = c.backbone == F5_BACKBONE_DIT, mmdit = c.backbone == F5_BACKBONE_MMDIT;
    // the input embedding's names: DiT / UNetT InputEmbedding (dit.py:121-140), MMDiT AudioEmbedding (mmdit.py:67-79)
    const std::string in_proj_n = mmdit ? "audio_embed.linear" : "input_embed.proj";
    const std::string conv_n = mmdit ? "audio_embed.conv_pos_embed.conv1d." : "input_embed.conv_pos_embed.conv1d.";
    // aux tables
    const Tensor* t = nullptr;
    if (!(t = e->ws.get("aux.rope_cos")) || t->shape.size() != 2 || t->shape[1] != 32 || t->shape[0] < 1)
        return fail(F5_ESTATE, "missing/invalid aux.rope_cos [max_pos, 32]");
    const int64_t maxpos = t->shape[0];
    e->cfg.max_pos = (int)maxpos;
    CHK(copy_vec(e, s, "aux.rope_cos", {maxpos, 32}, &P.rope_cos));
    CHK(copy_vec(e, s, "aux.rope_sin", {maxpos, 32}, &P.rope_sin));
    CHK(dev_alloc(e, &P.rope_frag, (size_t)maxpos * 64));
    hipLaunchKernelGGL(rope_frag_kernel, dim3(ew_blocks(maxpos * 16)), dim3(256), 0, s, P.rope_cos, P.rope_sin, P.rope_frag, (long)maxpos);
    KCHK();
    CHK(copy_vec(e, s, "aux.time_freqs", {128}, &P.time_freqs));
    // time MLP
    CHK(pack_linear<float>(e, s, "time_embed.time_mlp.0", D, 256, &P.time0));
    CHK(pack_linear<float>(e, s, "time_embed.time_mlp.2", D, D, &P.time2));
    // text encoder
    CHK(copy_vec(e, s, "text_embed.text_embed.weight", {c.text_num_embeds + 1, Dt}, &P.E));
    CHK(reg_target(e, "text_embed.text_embed.weight", false, c.text_num_embeds + 1, Dt, Dt, P.E, MK_F32));
    if (c.conv_layers > 0 || mmdit) {   // (the MMDiT adds the sinus row to the bare lookup, mmdit.py:50-56)
        if (!(t = e->ws.get("aux.text_pos")) || t->shape.size() != 2 || t->shape[1] != Dt)
            return fail(F5_ESTATE, "missing/invalid aux.text_pos [P, text_dim]");
        P.text_pos_rows = (int)t->shape[0];
        CHK(copy_vec(e, s, "aux.text_pos", {t->shape[0], Dt}, &P.text_pos));
    }
    P.tblocks.resize(c.conv_layers);
    for (int i = 0; i < c.conv_layers; ++i) {
        const std::string p = "text_embed.text_blocks." + std::to_string(i);
        TextBlockW& tb = P.tblocks[i];
        const Tensor* dw = nullptr;
        CHK(need(e->ws, p + ".dwconv.weight", {Dt, 1, 7}, &dw));
        CHK(dev_alloc(e, &tb.dwk, (size_t)7 * Dt));
        hipLaunchKernelGGL((permute_last2_kernel<float>), dim3(ew_blocks(7L * Dt)), dim3(256), 0, s, dw->p, tb.dwk, 1L, Dt, 7);
        CHK(copy_vec(e, s, p + ".dwconv.bias", {Dt}, &tb.dwb));
        CHK(copy_vec(e, s, p + ".norm.weight", {Dt}, &tb.lnw));
        CHK(copy_vec(e, s, p + ".norm.bias", {Dt}, &tb.lnb));
        CHK(copy_vec(e, s, p + ".grn.gamma", {1, 1, 2 * Dt}, &tb.gamma));
        CHK(copy_vec(e, s, p + ".grn.beta", {1, 1, 2 * Dt}, &tb.beta));
        CHK(pack_linear<float>(e, s, p + ".pwconv1", 2 * Dt, Dt, &tb.pw1));
        CHK(pack_linear<float>(e, s, p + ".pwconv2", Dt, 2 * Dt, &tb.pw2));
        CHK(reg_target(e, p + ".dwconv.weight", false, Dt, 7, 7, tb.dwk, MK_TAPS));
        CHK(reg_target(e, p + ".dwconv.bias", false, 1, Dt, Dt, tb.dwb, MK_F32));
        CHK(reg_target(e, p + ".norm.weight", false, 1, Dt, Dt, tb.lnw, MK_F32));
        CHK(reg_target(e, p + ".norm.bias", false, 1, Dt, Dt, tb.lnb, MK_F32));
        CHK(reg_target(e, p + ".grn.gamma", false, 1, 2 * Dt, 2 * Dt, tb.gamma, MK_F32));
        CHK(reg_target(e, p + ".grn.beta", false, 1, 2 * Dt, 2 * Dt, tb.beta, MK_F32));
        CHK(reg_linear_f32(e, p + ".pwconv1", tb.pw1, 2 * Dt, Dt));
        CHK(reg_linear_f32(e, p + ".pwconv2", tb.pw2, Dt, 2 * Dt));
    }
    // input embedding
    constexpr WRole bb = WRole::Backbone;
    CHK((pack_linear<T, bb>(e, s, in_proj_n, D, e->kin, &P.in_proj)));
    auto zlo = [&](int bit, LinW<T>& L) {   // diagnostic F5_X3_ABLATE: plain f16 weights (lo halves zeroed) for a class
        if (e->sw.x3_ablate & bit) zero_lo_planar(s, L.w, (size_t)L.N * L.ldw);
    };
    zlo(64, P.in_proj);
    const int cpg = D / 16;
    P.conv_kp = round_up(31 * cpg, GEMM_ROW_BYTES / (int)sizeof(T));   // whole K-tiles, zero padded (convpos.h)
    for (int j = 0; j < 2; ++j) {
        const std::string p = conv_n + std::to_string(j * 2);
        const Tensor* w = nullptr;
        CHK(need(e->ws, p + ".weight", {D, cpg, 31}, &w));
        CHK(dev_alloc(e, &P.conv_w[j], (size_t)D * P.conv_kp));
        hipLaunchKernelGGL((conv_pack_kernel<T>), dim3(ew_blocks((long)D * P.conv_kp)), dim3(256), 0, s, w->p,
                           P.conv_w[j], (long)D, cpg, 31, P.conv_kp);
        if (conv_split(e)) CHK((maybe_split_weight<T, true>(e, s, P.conv_w[j], (size_t)D * P.conv_kp)));   // F5_PREC_F16X3 (convpos.h SPLIT)
        if (conv_split(e) && (e->sw.x3_ablate & 128)) zero_lo_planar(s, P.conv_w[j], (size_t)D * P.conv_kp);
        CHK(copy_vec(e, s, p + ".bias", {D}, &P.conv_b[j]));
    }
    // transformer
    P.blocks.resize(c.depth);
    std::vector<std::string> modp;
    for (int i = 0; i < c.depth; ++i) {
        BlockW<T>& b = P.blocks[i];
        const std::string p = dit || mmdit ? "transformer_blocks." + std::to_string(i) : "layers." + std::to_string(i);
        const std::string at = dit || mmdit ? p + ".attn" : p + ".2";
        const std::string ff = dit ? p + ".ff" : mmdit ? p + ".ff_x" : p + ".4";
        CHK(pack_stream<T>(e, s, b.x, at, "", at + ".to_out.0", ff, at + ".", false));
        if (dit && e->adapters_on) {   // the reference's LoRA targets (train/train_lora.py); q / k / v are row ranges of the fused operand
            const char* qkv_names[3] = {".to_q.weight", ".to_k.weight", ".to_v.weight"};
            for (int j = 0; j < 3; ++j)
                CHK(reg_target(e, at + qkv_names[j], true, inner, D, b.x.qkv.ldw, b.x.qkv.w + (size_t)j * inner * b.x.qkv.ldw, merge_kind<T>(e)));
            CHK(reg_target(e, at + ".to_out.0.weight", true, D, inner, b.x.out.ldw, b.x.out.w, merge_kind<T>(e)));
        }
        zlo(1, b.x.qkv);
        zlo(8, b.x.out);
        zlo(16, b.x.ff1);
        zlo(32, b.x.ff2);
        HIPCHK(hipGetLastError());
        if (mmdit) {   // the text stream's own weights; the last block is context_pre_only (modules.py:721-739)
            CHK(pack_stream<T>(e, s, b.c, at, "_c", at + ".to_out_c", p + ".ff_c", at + ".c_", i == c.depth - 1));
            modp.push_back(p + ".attn_norm_x.linear");
            modp.push_back(p + ".attn_norm_c.linear");
        } else if (dit) {
            modp.push_back(p + ".attn_norm.linear");
        } else {
            CHK(copy_vec(e, s, p + ".1.g", {D}, &b.norm1_g));
            CHK(copy_vec(e, s, p + ".3.g", {D}, &b.norm2_g));
            if (i >= c.depth / 2 && e->ws.get(p + ".0.weight")) {
                CHK((pack_linear<T, bb>(e, s, p + ".0", D, 2 * D, &b.skip, false)));
                zlo(512, b.skip);   // diagnostic: the skip projection with plain f16 weights
                HIPCHK(hipGetLastError());
            }
        }
    }
    if (dit || mmdit) {
        // stacked AdaLN: rows [l*6D, (l+1)*6D) = layer l (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp);
        // last 2D rows = norm_out (scale, shift).  Always f32.
        // (MMDiT: per block attn_norm_x's 6 D then attn_norm_c's 6 D -- the last block's attn_norm_c is an AdaLayerNorm_Final of
        //  2 D, (scale, shift) -- so every slot but that one and norm_out has 6 D rows and the slots stay back to back)
        LinW<float>& M = P.mod;
        M.N = e->modN;
        M.K = D;
        M.ldw = D;
        CHK(dev_alloc(e, &M.w, (size_t)M.N * D));
        CHK(dev_alloc(e, &M.b, (size_t)M.N));
        modp.push_back("norm_out.linear");
        size_t row0 = 0;
        for (size_t i = 0; i < modp.size(); ++i) {
            const bool final2 = i + 1 == modp.size() || (mmdit && i + 2 == modp.size());
            const std::string& p = modp[i];
            const int rows = final2 ? 2 * D : 6 * D;
            const Tensor *w = nullptr, *b = nullptr;
            CHK(need(e->ws, p + ".weight", {rows, D}, &w));
            CHK(need(e->ws, p + ".bias", {rows}, &b));
            HIPCHK(hipMemcpyAsync(M.w + row0 * D, w->p, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(M.b + row0, b->p, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
            row0 += rows;
        }
        if ((int)row0 != e->modN) return fail(F5_ESTATE, "AdaLN stack: %zu rows packed, %d planned", row0, e->modN);
    } else {
        CHK(copy_vec(e, s, "norm_out.g", {D}, &P.norm_out_g));
    }
    CHK((pack_linear<T, bb>(e, s, "proj_out", mel, D, &P.proj_out)));
    if (c.options & F5_OPT_LONG_SKIP) {
        CHK((pack_linear<T, bb>(e, s, "long_skip_connection", D, 2 * D, &P.long_skip, false)));
        if (e->io_split) CHK((pack_linear<float, bb>(e, s, "long_skip_connection", D, 2 * D, &P.long_skip_f, false)));
    }
    if (e->io_split) {   // F5_PREC_F16P: the input / output layers once more, as split-planar f32 operands
        CHK((pack_linear<float, bb>(e, s, in_proj_n, D, e->kin, &P.in_proj_f)));
        CHK((pack_linear<float, bb>(e, s, "proj_out", mel, D, &P.proj_out_f)));
        P.conv_kp_f = round_up(31 * cpg, GEMM_ROW_BYTES / (int)sizeof(float));
        for (int j = 0; j < 2; ++j) {
            const std::string p = conv_n + std::to_string(j * 2);
            const Tensor* w = nullptr;
            CHK(need(e->ws, p + ".weight", {D, cpg, 31}, &w));
            CHK(dev_alloc(e, &P.conv_w_f[j], (size_t)D * P.conv_kp_f));
            hipLaunchKernelGGL((conv_pack_kernel<float>), dim3(ew_blocks((long)D * P.conv_kp_f)), dim3(256), 0, s, w->p,
                               P.conv_w_f[j], (long)D, cpg, 31, P.conv_kp_f);
            // (dims whose 32-deep K blocks straddle taps keep the exact-f32 MFMA kernel: convpos_can_split)
            if (convpos_can_split(D)) CHK((maybe_split_weight<float, true>(e, s, P.conv_w_f[j], (size_t)D * P.conv_kp_f)));
        }
    }
    zlo(256, P.proj_out);
    // (F5_PREC_F16P holds the input projection twice: f16 rows and the split-planar f32 operand the forward reads)
    CHK(reg_target(e, in_proj_n + ".weight", true, D, e->kin, P.in_proj.ldw, P.in_proj.w, merge_kind<T>(e),
                   e->io_split ? P.in_proj_f.w : nullptr, e->io_split ? MK_PLANAR : MK_NONE));
    HIPCHK(hipGetLastError());
    return F5_OK;
}
// F5_PREC_F8: the code bytes one row of Work::a8 is carved with -- the widest K of the four block GEMMs
static int a8_pitch(const f5_engine* e) { return std::max(std::max(e->cfg.dim, e->cfg.ff_dim), e->inner); }
template <typename T> static size_t carve_into(const f5_engine* e, Arena& a, Work<T>& w, int B, int N, int S) {
    const size_t NT = (size_t)std::max(e->res_nt, 1);
    const f5_config& c = e->cfg;
    a.reset();
    const size_t Bp = 2 * (size_t)B, D = c.dim, Dt = c.text_dim, F = c.ff_dim, mel = c.mel_dim;
    const size_t Nt = c.backbone == F5_BACKBONE_UNETT ? N + 1 : N;  // UNetT prepends the time token
    const size_t rows = Bp * Nt;
    // MMDiT: q / k / ao / vt hold the joint sequence of NT text and N audio positions per batch row; text_c / text_u the text stream's
    // embedding [B, NT, D] (there is no stretched [B, N, Dt] text)
    const bool mmdit = c.backbone == F5_BACKBONE_MMDIT;
    const size_t jrows = mmdit ? Bp * (Nt + NT) : rows, text_el = mmdit ? NT * D : (size_t)N * Dt;
    // time rows: one per backbone evaluation -- S (Euler) or 2 S (midpoint) in sample(), Bp in forward() -- and behind the
    // evaluation times in tdev the grid t[0..S] (sample_body: the dt of every step)
    // (a per-item call has one row per DISTINCT evaluation time of the batch: f5_engine::res_U)
    const size_t SS = (size_t)std::max(std::max(2 * S + 1, (int)Bp + 1), e->res_U);
    w.Npad = round_up((int)(mmdit ? Nt + NT : Nt), 64);
    w.tdev = a.take<float>(SS + (size_t)S + 1);
    w.feat = a.take<float>(SS * 256);
    w.th = a.take<float>(SS * D);
    w.temb = a.take<float>(SS * D);
    w.st = a.take<float>(SS * D);
    w.mod = a.take<float>(SS * e->modN);
    w.lens = a.take<int>(Bp + 16);
    w.lens_plain = a.take<int>(Bp + 16);
    w.row_start = a.take<int>(Bp + (size_t)B + 16);
    w.rowmap = a.take<int2>(Bp * (size_t)round_up(N, 4));
    w.step_cond = a.take<float>((size_t)B * N * mel);
    w.text_c = a.take<float>((size_t)B * text_el);
    w.text_u = a.take<float>((size_t)B * text_el);
    w.tx_a = a.take<float>((size_t)B * N * Dt);
    w.tx_b = a.take<float>((size_t)B * N * Dt);
    w.tx_h1 = a.take<float>((size_t)B * N * 2 * Dt);
    w.grn_part = a.take<float>((size_t)B * GRN_P * 2 * Dt);
    w.uc = a.take<float>((size_t)N * Dt);
    w.acat = a.take<T>(Bp * N * e->kin_pad * (e->io_split ? sizeof(float) / sizeof(T) : 1));   // (F5_PREC_F16P packs the input rows as f32)
    w.h = a.take<float>(rows * D);
    w.c1 = a.take<float>(rows * D);
    w.x = a.take<float>(rows * D);
    w.pred = a.take<float>(Bp * N * mel);
    w.xn = a.take<T>(rows * D);
    w.q = a.take<T>(jrows * e->inner);
    w.k = a.take<T>(jrows * e->inner);
    w.ao = a.take<T>(jrows * e->inner);
    w.vt = a.take<T>(Bp * c.heads * 64 * w.Npad);
    w.ffh = a.take<T>(rows * F);
    w.a8 = Rows8{};
    if (e->f8) {   // F5_PREC_F8 only: every other precision's plan is what it was
        w.a8.pitch = a8_pitch(e);
        w.a8.codes = a.take<unsigned char>(rows * w.a8.pitch);
        w.a8.scales = a.take<unsigned char>(rows + 16);
    }
    w.in_cond = a.take<float>((size_t)B * N * mel);
    w.y = a.take<float>((size_t)B * N * mel);
    w.y_mid = a.take<float>((size_t)B * N * mel);
    w.out_buf = a.take<float>((size_t)B * N * mel);
    w.traj_buf = a.take<float>((size_t)(S + 1) * B * N * mel);
    w.in_mask = a.take<unsigned char>((size_t)B * N + 16);
    w.in_text = a.take<long long>((size_t)B * NT + 2);
    w.cat2 = nullptr;
    w.skips = nullptr;
    w.pred_all = nullptr;
    if (c.options & F5_OPT_LONG_SKIP) w.cat2 = a.take<T>(rows * 2 * D * (e->io_split ? sizeof(float) / sizeof(T) : 1));
    if (c.backbone == F5_BACKBONE_UNETT) {
        w.cat2 = a.take<T>(rows * 2 * D);
        w.skips = a.take<float>(rows * D * (c.depth / 2));
        w.pred_all = a.take<float>(rows * mel);
    }
    w.mm_c = nullptr;
    w.mm_cn = w.mm_aox = w.mm_aoc = w.mm_ffc = nullptr;
    w.mm_lens = nullptr;
    if (mmdit) {
        w.mm_c = a.take<float>(Bp * NT * D);
        w.mm_cn = a.take<T>(Bp * NT * D);
        w.mm_aox = a.take<T>(rows * e->inner);
        w.mm_aoc = a.take<T>(Bp * NT * e->inner);
        w.mm_ffc = a.take<T>(Bp * NT * F);
        w.mm_lens = a.take<int>(Bp + 16);
    }
    // f5_sample_items: behind everything else, and only once a per-item call has asked (an engine that never does keeps its arena)
    w.mod_rows = w.it_t = w.it_cfg = nullptr;
    w.it_steps = w.it_idx = nullptr;
    if (e->res_items) {
        w.mod_rows = a.take<float>(Bp * (c.backbone == F5_BACKBONE_DIT ? (size_t)e->modN : D));
        w.it_t = a.take<float>((size_t)B * ((size_t)S + 1));
        w.it_cfg = a.take<float>((size_t)B);
        w.it_steps = a.take<int>((size_t)B);
        w.it_idx = a.take<int>(2 * (size_t)S * B);
    }
    return align_up(a.off, 256) + 256;
}
template <typename T> static void carve(f5_engine* e, Work<T>& w, int B, int N, int S) {
    (void)carve_into<T>(e, e->arena, w, B, N, S);
}

// ---------------------------------------------------------------------------------------------- sub-graphs

template <typename T> static Packed<T>& packed(f5_engine* e);
template <> inline Packed<float>& packed<float>(f5_engine* e) { return e->pf; }
template <> inline Packed<bf16_t>& packed<bf16_t>(f5_engine* e) { return e->pb; }
template <> inline Packed<f16_t>& packed<f16_t>(f5_engine* e) { return e->ph; }

// time features -> t_emb [S, D], silu(t_emb), and (DiT) all AdaLN vectors mod [S, modN]
template <typename T> static int run_time_path(f5_engine* e, Work<T>& w, int S, hipStream_t s) {
    Packed<T>& P = packed<T>(e);
    const int D = e->cfg.dim;
    return e->prof.timed(PC_TIME, s, [&]() -> int {
        launch_time_sinus(s, w.tdev, P.time_freqs, w.feat, S);
        KCHK();
        HIPCHK(launch_gemm<float>(s, w.feat, 256, P.time0.w, P.time0.ldw, S, D, 256,
                                  EpiStore<float>{w.th, D, P.time0.b, F5_ACT_SILU}));
        HIPCHK(launch_gemm<float>(s, w.th, D, P.time2.w, P.time2.ldw, S, D, D, EpiStore<float>{w.temb, D, P.time2.b, F5_ACT_NONE}));
        if (e->cfg.backbone != F5_BACKBONE_UNETT) {   // DiT and MMDiT: the whole AdaLN stack of every evaluation time
            hipLaunchKernelGGL(act_kernel, dim3(ew_blocks((long)S * D)), dim3(256), 0, s, w.temb, w.st, (long)S * D, F5_ACT_SILU);
            KCHK();
            HIPCHK(launch_gemm<float>(s, w.st, D, P.mod.w, P.mod.ldw, S, e->modN, D,
                                      EpiStore<float>{w.mod, e->modN, P.mod.b, F5_ACT_NONE}));
        }
        return F5_OK;
    });
}

// text ids -> text embedding [B, N, Dt] (dit.py:86-115 + per-sample lengths dit.py:247-258)
template <typename T>
static int run_text_embed(f5_engine* e, Work<T>& w, const int64_t* text, int B, int nt, const int* lens_dev, int N,
                          int drop_text, float* out, hipStream_t s) {
    Packed<T>& P = packed<T>(e);
    const f5_config& c = e->cfg;
    const int Dt = c.text_dim;
    const bool dit = c.backbone == F5_BACKBONE_DIT;
    if (c.backbone == F5_BACKBONE_MMDIT) {
        // mmdit.py:40-61: lookup + the sinus row of the token's own position + (mask_padding) zero rows where the ORIGINAL token is the
        // filler, drop_text replacing the tokens after that mask was taken: text_embed_kernel's arithmetic at "N" = nt, no lengths
        if (nt > P.text_pos_rows) return fail(F5_EINVAL, "nt=%d exceeds aux.text_pos (%d rows)", nt, P.text_pos_rows);
        return e->prof.timed(PC_TEXT, s, [&]() -> int {
            hipLaunchKernelGGL(text_embed_kernel, dim3(ew_blocks((long)B * nt * Dt / 4)), dim3(256), 0, s, (const long long*)text, nt, P.E,
                               P.text_pos, out, B, nt, Dt, (const int*)nullptr, drop_text, c.text_mask_padding, 1, P.text_pos_rows);
            KCHK();
            return F5_OK;
        });
    }
    const long rows = (long)B * N;
    if (c.conv_layers > 0 && dit && N > P.text_pos_rows) return fail(F5_EINVAL, "N=%d exceeds aux.text_pos rows", N);
    return e->prof.timed(PC_TEXT, s, [&]() -> int {
        float* cur = c.conv_layers > 0 ? w.tx_a : out;  // block input/output (updated in place); last block writes `out`
        const int pos_rows = P.text_pos_rows > 0 ? P.text_pos_rows : 1;
        hipLaunchKernelGGL(text_embed_kernel, dim3(ew_blocks(rows * Dt / 4)), dim3(256), 0, s, (const long long*)text, nt, P.E,
                           P.text_pos, cur, B, N, Dt, lens_dev, drop_text, c.text_mask_padding && c.conv_layers > 0,
                           c.conv_layers > 0, dit ? 1 << 30 : pos_rows);
        KCHK();
        for (int i = 0; i < c.conv_layers; ++i) {
            TextBlockW& tb = P.tblocks[i];
            float* nxt = (i == c.conv_layers - 1) ? out : cur;
            hipLaunchKernelGGL(dwconv7_ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, cur, w.tx_b, tb.dwk, tb.dwb, tb.lnw,
                               tb.lnb, B, N, Dt, lens_dev, 1e-6f);
            KCHK();
            HIPCHK(launch_gemm<float>(s, w.tx_b, Dt, tb.pw1.w, tb.pw1.ldw, (int)rows, 2 * Dt, Dt,
                                      EpiStore<float>{w.tx_h1, 2 * Dt, tb.pw1.b, F5_ACT_GELU_ERF}));
            hipLaunchKernelGGL(grn_partial_kernel, dim3((2 * Dt + 255) / 256, GRN_P, B), dim3(256), 0, s, w.tx_h1, w.grn_part,
                               N, 2 * Dt, lens_dev);
            KCHK();
            const int rpb = 16;
            hipLaunchKernelGGL(grn_apply_kernel, dim3((N + rpb - 1) / rpb, B), dim3(256), (2 * Dt + 8) * sizeof(float), s,
                               w.tx_h1, w.grn_part, tb.gamma, tb.beta, N, 2 * Dt, lens_dev, rpb);
            KCHK();
            // residual add: nxt = cur + pwconv2(h1)
            HIPCHK(launch_gemm<float>(s, w.tx_h1, 2 * Dt, tb.pw2.w, tb.pw2.ldw, (int)rows, Dt, 2 * Dt,
                                      EpiGateRes{nxt, cur, Dt, tb.pw2.b, nullptr, 0, N, nullptr}));
            if (c.text_mask_padding) {
                hipLaunchKernelGGL(zero_filler_rows_kernel, dim3(ew_blocks(rows * Dt / 4)), dim3(256), 0, s,
                                   (const long long*)text, nt, nxt, B, N, Dt);
                KCHK();
            }
            cur = nxt;
        }
        if (lens_dev && c.conv_layers > 0) {
            hipLaunchKernelGGL(zero_tail_rows_kernel, dim3(ew_blocks(rows * Dt / 4)), dim3(256), 0, s, out, B, N, Dt, lens_dev);
            KCHK();
        }
        if (c.options & F5_OPT_TEXT_AVG_UPSAMPLE) {   // dit.py:112-113: after the text blocks; the mask is that of the ORIGINAL ids
            hipLaunchKernelGGL(text_avg_upsample_kernel, dim3(B), dim3(256), (size_t)N * sizeof(int), s, (const long long*)text, nt, out, w.tx_b, N, Dt,
                               lens_dev);
            KCHK();
            HIPCHK(hipMemcpyAsync(out, w.tx_b, (size_t)rows * Dt * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return F5_OK;
    });
}

// ---------------------------------------------------------------------------------- stages shared by the three backbones
// The backbone GEMMs the stages run through FwdCtx::mul, by class.  A class fixes, in this one place: its F5_X3_ABLATE bit (0: no hook);
// whether its A operand arrives pre-split under F5_PREC_F16X3; and, where its weight holds e4m3 rows (F5_PREC_F8: the first four), whether
// the AdaLN LayerNorm in front of it wrote the e4m3 A operand (a_from_ln) or the stand-alone row quantiser runs first.
enum class GemmClass { QKV, OutProj, FF1, FF2, ProjOut, LongSkip, UNetTSkip };
struct GemmClassInfo { int ablate_bit; bool a_presplit, a_from_ln; };
constexpr GemmClassInfo gemm_class(GemmClass c) {
    switch (c) {
        case GemmClass::QKV: return {1, true, true};
        case GemmClass::OutProj: return {8, true, false};
        case GemmClass::FF1: return {16, true, true};
        case GemmClass::FF2: return {32, true, false};
        case GemmClass::ProjOut: return {256, true, false};
        case GemmClass::LongSkip: return {0, false, false};
        case GemmClass::UNetTSkip: return {512, true, false};   // (launch_cat2 writes the concat pre-split, so that the projection runs on pre-split operands too)
    }
    return {0, false, false};
}
// What the stages of one forward share: the engine, the stream, the geometry and (DiT) the tables of a packed batch.
struct FwdCtx {
    f5_engine* e;
    hipStream_t s;
    int B, Bp, N, rows;    // N: tokens per batch row (UNetT blocks: the frames + the time token); rows = Bp * N: launch geometry, the padded batch
    const int* lens_dev;   // per-batch-row lengths, or null
    RowPack pk;            // packed variable-length batch (rows present = *pk.rows_dev); empty: the padded batch as it is
    Rows8 a8;              // F5_PREC_F8 (the DiT's blocks): Work::a8, where the e4m3 A operand of the block GEMM about to run is written; else empty
    const int* ml() const { return pk.rows_dev; }              // device row count of a packed batch, or null
    int mh() const { return pk ? (int)pk.rows_host : 0; }      // rows expected (the call's own lengths): tile choice only
    int pl() const { return e->split16 ? 1 : 0; }              // F5_PREC_F16X3: xn / ao / ffh are written pre-split (the A operands of the block GEMMs)
    // write-through stores for class `bit` (F5_WT_*, Switches::store_wt): only in the latency-bound regime -- few rows, one round of tiles --
    // where a kernel's whole output would otherwise sit dirty in L2 when it ends (the condition of the weight prefetch)
    int wt(int bit) const { return rows <= 4096 && (e->sw.store_wt & bit) ? 1 : 0; }
    double gflops(double n, double k) const { return 2.0 * (pk ? pk.rows_host : (double)rows) * n * k; }
    // One backbone GEMM of class c over all rows, A [rows, L.K] times L into epi, as a profiled launch behind the class's diagnostic hook.
    // The weight's form is the product's: L.q -- e4m3 rows, the A operand in a8 at the pitch of L.K, left there by the LayerNorm or
    // quantised here from the 16-bit rows a.p (attention output, FF hidden) by the stand-alone launch -- else the rows of egemm.
    template <typename T, typename Epi> int mul(GemmClass c, ARows<T> a, const LinW<T>& L, const Epi& epi) const {
        const GemmClassInfo g = gemm_class(c);
        ablate(g.ablate_bit, a.p, L.K);
        if constexpr (std::is_same_v<T, f16_t>) {
            if (L.q) {
                if (!g.a_from_ln) {
                    const Rows8 q = a8.at_pitch(L.K);
                    HIPCHK(e->prof.timed(PC_MISC, s, [&] {
                        launch_quant_rows_e4m3<T>(s, a.p, L.K, rows, L.K, q, ml());
                        return hipGetLastError();
                    }));
                    a = ARows<T>(q);
                }
                if (!a.q) return fail(F5_ESTATE, "F5_PREC_F8: a block GEMM was not handed its e4m3 A operand");
                HIPCHK(e->prof.timed(PC_GEMM, s, gflops(L.N, L.K), [&] {
                    GemmOpts o{GemmOperands::Plain, -1, ml(), mh()};
                    o.a_scale = a.q.scales;
                    o.w_scale = L.q.scales;
                    return launch_gemm<e4m3_t>(s, a.q.e4m3(), a.q.pitch, L.q.e4m3(), L.q.pitch, rows, L.N, L.K, epi, o);
                }));
                return F5_OK;
            }
        }
        HIPCHK(e->prof.timed(PC_GEMM, s, gflops(L.N, L.K), [&] {
            return egemm<T>(e, s, a.p, L.K, L.w, L.ldw, rows, L.N, L.K, epi, ml(), mh(), g.a_presplit && pl());
        }));
        return F5_OK;
    }
    // the operand an AdaLN LayerNorm in front of a block's QKV / FF1 writes: e4m3 rows of D codes in a8 where there is one, else the rows xn
    template <typename T> ARows<T> ln_operand(T* xn) const { return a8 ? ARows<T>(a8.at_pitch(e->cfg.dim)) : ARows<T>(xn); }
    // diagnostic F5_X3_ABLATE: the class's A operand [rows, k] as plain f16 (lo halves zeroed).  The hooks of the shared stages act on the
    // x stream only: finalize_t never ablates the MMDiT text stream's weights, so the text stream's context turns them off (x3 = false)
    // and its activations stay whole too.
    bool x3 = true;
    template <typename T> void ablate(int bit, T* a, int k) const {
        if (x3 && (e->sw.x3_ablate & bit)) zero_lo_planar(s, a, (size_t)rows * k);
    }
};

// Input embedding: [y, cond, text] packed as rows of U, the input projection, and the conv position embedding (two grouped convs, the second
// with the projection as its residual) into dst.  U = T, or (F5_PREC_F16P, e->io_split) float: the rows packed as f32, input projection and
// convs as split-f16 products on f32 operands (what the f16 blocks then see is x, the f32 residual stream, exactly as in F5_PREC_F16X3).
// ablate: diagnostic F5_X3_ABLATE bits 64 / 128 on the activation side -- the unsplit f32 operands as f16 sees them (the DiT only).
template <typename T, typename U>
static int embed_input(const FwdCtx& f, Work<T>& w, const float* y, const float* cond, int drop_cond_first, const float* text_first,
                       const float* text_second, float* dst, bool ablate = false) {
    f5_engine* e = f.e;
    hipStream_t s = f.s;
    Packed<T>& P = packed<T>(e);
    Prof& pr = e->prof;
    const f5_config& c = e->cfg;
    const int D = c.dim, rows = f.rows, B = f.B, Bp = f.Bp, N = f.N;
    const RowPack& pk = f.pk;
    U* acat = reinterpret_cast<U*>(w.acat);
    const LinW<U>* ip;
    U* const* cw;
    int kp;
    bool cs;
    if constexpr (std::is_same_v<U, T>) {
        ip = &P.in_proj; cw = P.conv_w; kp = P.conv_kp; cs = conv_split(e);
    } else {
        ip = &P.in_proj_f; cw = P.conv_w_f; kp = P.conv_kp_f; cs = convpos_can_split(D);
    }
    HIPCHK(pr.timed(PC_MISC, s, [&] {
        launch_pack_input<U>(s, y, cond, text_first, text_second, acat, e->kin_pad, B, Bp, N, c.mel_dim, e->kin - 2 * c.mel_dim, drop_cond_first, pk.rowmap,
                             f.ml(), f.lens_dev);
        return hipGetLastError();
    }));
    auto ablate_round = [&](int bit, const float* src, float* to, long n) -> const float* {   // diagnostic F5_X3_ABLATE: an unsplit f32 operand as f16 sees it
        if (!ablate || !(e->sw.x3_ablate & bit)) return src;
        hipLaunchKernelGGL(round_f16_kernel, dim3(ew_blocks(n)), dim3(256), 0, s, src, to, n);
        return to;
    };
    if constexpr (std::is_same_v<U, float>) ablate_round(64, acat, acat, (long)rows * e->kin_pad);
    HIPCHK(pr.timed(PC_GEMM, s, f.gflops(D, e->kin), [&] {
        const EpiStore<float> epi{w.h, D, ip->b, F5_ACT_NONE};
        if constexpr (std::is_same_v<U, T>) return egemm<T>(e, s, acat, e->kin_pad, ip->w, ip->ldw, rows, D, e->kin_pad, epi, f.ml(), f.mh());
        else return launch_gemm<float>(s, acat, e->kin_pad, ip->w, ip->ldw, rows, D, e->kin_pad, epi, {GemmOperands::WSplit, -1, f.ml(), f.mh()});
    }));
    const double conv_fl = f.gflops(D, (D / 16) * 31);
    HIPCHK(pr.timed(PC_CONV, s, conv_fl, [&] {
        // (ablation: conv 1 reads a rounded COPY of h -- w.x is free until conv 2 writes it -- because h itself is conv 2's f32 residual)
        const float* conv1_in = ablate_round(128, w.h, w.x, (long)rows * D);
        return launch_convpos<U>(s, conv1_in, cw[0], kp, P.conv_b[0], nullptr, w.c1, Bp, N, D, f.lens_dev, B, pk.row_start, cs);
    }));
    ablate_round(128, w.c1, w.c1, (long)rows * D);
    HIPCHK(pr.timed(PC_CONV, s, conv_fl, [&] {
        return launch_convpos<U>(s, w.c1, cw[1], kp, P.conv_b[1], w.h, dst, Bp, N, D, f.lens_dev, B, pk.row_start, cs);
    }));
    return F5_OK;
}

// AdaLN LayerNorm of the residual stream x into out: out = LN(x) * (1 + scale) + shift, as rows of TO (planar: pre-split f32 rows) or as
// the e4m3 operand out.q.  mod_stride: distance between batch rows' vectors (0: shared).  A packed batch with its own vectors per batch
// row finds them through the rowmap.  pf: weights to prefetch from the launch (see layernorm_kernel).
template <typename TO>
static hipError_t adaln_norm(const FwdCtx& f, const float* x, const ARows<TO>& out, const float* scale, const float* shift, int mod_stride,
                             const Prefetch& pf, int planar) {
    const AdaLN a{x, scale, shift, f.rows, f.e->cfg.dim, mod_stride, f.N, 1e-6f, f.pk && mod_stride != 0 ? f.pk.rowmap : nullptr, pf, f.ml()};
    return f.e->prof.timed(PC_LN, f.s, [&] {
        if (out.q) launch_adaln_norm(f.s, a, out.q);
        else launch_adaln_norm(f.s, a, out.p, planar, f.wt(F5_WT_LN));
        return hipGetLastError();
    });
}

// The attention operands q / k / v^T in the type the QKV epilogue writes and the attention kernel reads them -- the one place that decides
// it.  F5_PREC_F16X3 with plain-f16 attention products (x3_attn_hi == 3, no qk_norm): f16, in the f32 buffers at half their size, and
// the fast 16-bit attention kernel writes its output pre-split for the out-projection.  Everything else: T.  fn(q, k, vt) is called once.
template <typename T, typename Fn> static int with_attn_operands(const f5_engine* e, const Work<T>& w, bool qk_norm, Fn&& fn) {
    if constexpr (std::is_same_v<T, float>) {
        if (e->split16 && e->sw.x3_attn_hi() == 3 && !qk_norm)
            return fn(reinterpret_cast<f16_t*>(w.q), reinterpret_cast<f16_t*>(w.k), reinterpret_cast<f16_t*>(w.vt));
    }
    return fn(w.q, w.k, w.vt);
}

// QKV projection of one stream's normed rows xn into q / k / v^T.  place: QKVOwnLayout -- the stream is the whole sequence (packed rows
// through f.pk's rowmap) -- or QKVJointLayout{L, off} -- the stream's f.N positions land at [off, off + f.N) of a joint sequence of L,
// every head rotated (the MMDiT's joint attention).  With qk_norm the epilogue leaves q / k raw and the norm-rope launch follows:
// RMSNorm comes BEFORE the rotary embedding (modules.py:481-497, 588-608).
template <typename T, typename Place>
static int qkv_project(const FwdCtx& f, Work<T>& w, const ARows<T>& xn, const StreamW<T>& sw, bool qk_norm, const Place& place) {
    constexpr bool joint = std::is_same_v<Place, QKVJointLayout>;
    f5_engine* e = f.e;
    Packed<T>& P = packed<T>(e);
    const f5_config& c = e->cfg;
    const int H = c.heads;
    const int pe_heads = joint || c.pe_attn_head < 0 ? H : c.pe_attn_head;
    int L = f.N, off = 0;
    if constexpr (joint) L = place.Lseq, off = place.off;
    return with_attn_operands<T>(e, w, qk_norm, [&](auto* q, auto* k, auto* vt) -> int {
        using TO = std::remove_pointer_t<decltype(q)>;
        CHK(f.mul(GemmClass::QKV, xn, sw.qkv,
                  EpiQKV<TO, joint>{q, k, vt, sw.qkv.b, P.rope_frag, f.N, w.Npad, H, qk_norm ? 0 : pe_heads,
                                    qk_norm ? 1.0f : attention_q_scale<TO>(), f.pk.rowmap, place}));
        if (qk_norm)
            HIPCHK(e->prof.timed(PC_MISC, f.s, [&] {
                return launch_qknorm_rope<TO>(f.s, q, k, sw.qn, sw.kn, P.rope_cos, P.rope_sin, f.Bp, H, f.N, L, off, pe_heads, attention_q_scale<TO>(), 1e-6f);
            }));
        return F5_OK;
    });
}

// Attention over L positions per batch row into w.ao.  kv_lens: key lengths of `len_rows` batch rows (batch row b reads entry
// b % len_rows), or null: every key; q_lens: query lengths, or null: every query row is computed.  Packed rows through f.pk.
template <typename T> static int attend(const FwdCtx& f, Work<T>& w, bool qk_norm, int L, const int* kv_lens, int len_rows, const int* q_lens) {
    f5_engine* e = f.e;
    const int H = e->cfg.heads, Bp = f.Bp;
    const double fl = 4.0 * H * 64 * (f.pk ? f.pk.sq_host : (double)Bp * L * L);
    return with_attn_operands<T>(e, w, qk_norm, [&](auto* q, auto* k, auto* vt) -> int {
        using TO = std::remove_pointer_t<decltype(q)>;
        HIPCHK(e->prof.timed(PC_ATTN, f.s, fl, [&] {
            if constexpr (std::is_same_v<TO, T>)
                return launch_attention_any(f.s, q, k, vt, w.ao, Bp, H, L, w.Npad, kv_lens, len_rows, q_lens, f.pk.row_start, e->split16, f.pl(),
                                            e->sw.x3_attn_hi(), f.wt(F5_WT_ATTN));
            else
                return launch_attention_v2<f16_t>(f.s, q, k, vt, nullptr, Bp, H, L, w.Npad, kv_lens, len_rows, q_lens, f.pk.row_start, w.ao);
        }));
        return F5_OK;
    });
}

// Out-projection of a stream's attention rows ao with the caller's residual epilogue.
template <typename T, typename Epi> static int out_project(const FwdCtx& f, T* ao, const StreamW<T>& sw, const Epi& out_epi) {
    return f.mul(GemmClass::OutProj, ARows<T>(ao), sw.out, out_epi);
}

// Attention sub-block of a backbone with one stream, on its normed rows xn: QKV projection, attention, out-projection.
template <typename T, typename Epi>
static int attention_block(const FwdCtx& f, Work<T>& w, const ARows<T>& xn, const StreamW<T>& sw, bool qk_norm, const Epi& out_epi) {
    // (a packed batch masks its keys whatever attn_mask_enabled says: a length-bucket plan packs utterances that fill their whole length,
    //  for which masked and unmasked attention coincide)
    const int* attn_lens = ((f.e->cfg.attn_mask_enabled || f.pk) && f.lens_dev) ? f.lens_dev : nullptr;
    CHK(qkv_project<T>(f, w, xn, sw, qk_norm, QKVOwnLayout{}));
    CHK(attend<T>(f, w, qk_norm, f.N, attn_lens, f.B, f.lens_dev));
    return out_project<T>(f, w.ao, sw, out_epi);
}

// Feed-forward pair on a stream's normed rows sb.xn: FF1 with GELU(tanh) into sb.ffh, FF2 with the caller's residual epilogue.
template <typename T, typename Epi> static int ff_block(const FwdCtx& f, const StreamBuf<T>& sb, const StreamW<T>& sw, const Epi& out_epi) {
    CHK(f.mul(GemmClass::FF1, sb.xn, sw.ff1, EpiStore<T>{sb.ffh, sw.ff1.N, sw.ff1.b, F5_ACT_GELU_TANH, f.pl(), f.wt(F5_WT_STORE16)}));
    return f.mul(GemmClass::FF2, ARows<T>(sb.ffh), sw.ff2, out_epi);
}

// Output projection of the normed stream xn into pred.  U = T: w.xn as the final norm left it; U = float (F5_PREC_F16P): pre-split f32
// rows, as a product of two pre-split operands.
template <typename T, typename U> static int project_out(const FwdCtx& f, U* xn, float* pred) {
    f5_engine* e = f.e;
    Packed<T>& P = packed<T>(e);
    const int D = e->cfg.dim, mel = e->cfg.mel_dim;
    if constexpr (std::is_same_v<U, T>) {
        return f.mul(GemmClass::ProjOut, ARows<T>(xn), P.proj_out, EpiStore<float>{pred, mel, P.proj_out.b, F5_ACT_NONE});
    } else {
        HIPCHK(e->prof.timed(PC_GEMM, f.s, f.gflops(mel, D), [&] {
            return launch_gemm<float>(f.s, xn, D, P.proj_out_f.w, P.proj_out_f.ldw, f.rows, mel, D,
                                      EpiStore<float>{pred, mel, P.proj_out_f.b, F5_ACT_NONE}, {GemmOperands::AWSplit, -1, f.ml(), f.mh()});
        }));
        return F5_OK;
    }
}

// The tail of every forward: final norm of the stream, output projection into pred.  norm(out, planar): the caller's AdaLN / RMSNorm of
// its residual stream.  F5_PREC_F16P (e->io_split): normed to pre-split f32 rows in free_f32, a buffer of [rows, D] floats the caller no
// longer needs, and projected as a product of two pre-split operands; otherwise through w.xn.
template <typename T, typename Norm> static int finish(const FwdCtx& f, Work<T>& w, float* free_f32, float* pred, const Norm& norm) {
    if (f.e->io_split) {
        HIPCHK(norm(free_f32, 1));
        return project_out<T, float>(f, free_f32, pred);
    }
    HIPCHK(norm(w.xn, f.pl()));
    return project_out<T, T>(f, w.xn, pred);
}

// What one backbone forward is called with (run_backbone).
struct ForwardArgs {
    const float *y, *cond;       // state and conditioning audio [B, N, mel]
    int B, Bp, N;                // Bp = B, or 2 B: the conditional half, then the unconditional half
    // time rows: the AdaLN vectors [modN] (DiT, MMDiT) or the time embedding [D] (UNetT) of batch row b at time_rows + b * time_stride;
    // stride 0: one row shared by every batch row, as in sample()
    const float* time_rows;
    int time_stride;
    const int* lens_dev;         // per-batch-row lengths, or null
    int drop_cond_first;         // whether the first half drops cond too (the second always does)
    const float *text_first, *text_second;   // text embeddings of the two halves: [B, N, Dt], MMDiT [B, nt, D]
    int nt;                      // MMDiT: the text stream's length (the other backbones stretch their text to N)
    RowPack pk;                  // packed variable-length batch (DiT only), or empty
    float* taps;                 // f5k_mmdit_taps (diagnostic), or null
};
// width of one time row, and the table sample() and forward() keep them in (run_time_path)
static int time_width(const f5_engine* e) { return e->cfg.backbone == F5_BACKBONE_UNETT ? e->cfg.dim : e->modN; }
template <typename T> static const float* time_table_dev(const f5_engine* e, const Work<T>& w) {
    return e->cfg.backbone == F5_BACKBONE_UNETT ? w.temb : w.mod;
}

// One DiT forward over Bp packed rows (dit.py:297-327).  a.time_rows: AdaLN vectors of this step.  A packed batch with a time stride (a
// per-item call on packed rows) finds a row's vectors through the rowmap's batch row: layernorm_rows_kernel and EpiGateResRows.
template <typename T> static int run_dit_forward(f5_engine* e, Work<T>& w, const ForwardArgs& a, hipStream_t s) {
    Packed<T>& P = packed<T>(e);
    const f5_config& c = e->cfg;
    const int D = c.dim, N = a.N, rows = a.Bp * N, mod_stride = a.time_stride;
    const RowPack& pk = a.pk;
    const FwdCtx f{e, s, a.B, a.Bp, N, rows, a.lens_dev, pk, w.a8};
    const int* ml = f.ml();
    const int mh = f.mh(), pl = f.pl();
    const int* gate_lens = pk ? nullptr : a.lens_dev; // (a packed batch has no padded rows to leave untouched)
    Prof& pr = e->prof;
    if (e->io_split) CHK((embed_input<T, float>(f, w, a.y, a.cond, a.drop_cond_first, a.text_first, a.text_second, w.x)));
    else CHK((embed_input<T, T>(f, w, a.y, a.cond, a.drop_cond_first, a.text_first, a.text_second, w.x, true)));
    const bool long_skip = (c.options & F5_OPT_LONG_SKIP) != 0;
    if (long_skip)   // residual = x (dit.py:313-314); h is free once the conv embedding has used it as its own residual
        HIPCHK(hipMemcpyAsync(w.h, w.x, (size_t)rows * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    const bool qk_norm = (c.options & F5_OPT_QK_RMSNORM) != 0;
    // weight prefetch from the LayerNorm launches (see layernorm_kernel): only where the GEMMs are latency-bound
    const bool wpf = rows <= 4096 && e->sw.weight_prefetch;
    auto prefetch = [&](const LinW<T>& g0, const LinW<T>& g1) {   // the weights of the two GEMMs behind a LayerNorm
        return wpf ? Prefetch{g0.bytes(), g0.nbytes(), g1.bytes(), g1.nbytes()} : Prefetch{};
    };
    const bool row_mods = pk && mod_stride != 0;   // every batch row of a packed batch has its own vectors
    const StreamBuf<T> sb{w.x, f.ln_operand(w.xn), w.ffh, w.ao};
    for (int l = 0; l < c.depth; ++l) {
        const StreamW<T>& sw = P.blocks[l].x;
        const float* m = a.time_rows + (size_t)l * 6 * D;  // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
        const EpiGateRes attn_epi{w.x, w.x, D, sw.out.b, m + 2 * D, mod_stride, N, gate_lens, f.wt(F5_WT_GATE_RES)};
        const EpiGateRes ff_epi{w.x, w.x, D, sw.ff2.b, m + 5 * D, mod_stride, N, nullptr, f.wt(F5_WT_GATE_RES)};
        HIPCHK(adaln_norm(f, w.x, sb.xn, m + D, m, mod_stride, prefetch(sw.qkv, sw.out), pl));
        if (row_mods) CHK(attention_block<T>(f, w, sb.xn, sw, qk_norm, EpiGateResRows{attn_epi, pk.rowmap}));
        else CHK(attention_block<T>(f, w, sb.xn, sw, qk_norm, attn_epi));
        HIPCHK(adaln_norm(f, w.x, sb.xn, m + 4 * D, m + 3 * D, mod_stride, prefetch(sw.ff1, sw.ff2), pl));
        if (row_mods) CHK(ff_block<T>(f, sb, sw, EpiGateResRows{ff_epi, pk.rowmap}));
        else CHK(ff_block<T>(f, sb, sw, ff_epi));
    }
    if (long_skip) {   // x = long_skip_connection(cat((x, residual), dim=-1))   (dit.py:323-324)
        auto cat_skip = [&](auto* cat) {
            return pr.timed(PC_MISC, s, [&] {
                launch_cat2(s, w.x, w.h, cat, rows, D, 0);
                return hipGetLastError();
            });
        };
        const EpiStore<float> epi{w.x, D, nullptr, F5_ACT_NONE};
        if (e->io_split) {
            float* cat_f = reinterpret_cast<float*>(w.cat2);
            HIPCHK(cat_skip(cat_f));
            HIPCHK(pr.timed(PC_GEMM, s, f.gflops(D, 2 * D), [&] {
                return launch_gemm<float>(s, cat_f, 2 * D, P.long_skip_f.w, P.long_skip_f.ldw, rows, D, 2 * D, epi, {GemmOperands::WSplit, -1, ml, mh});
            }));
        } else {
            HIPCHK(cat_skip(w.cat2));
            CHK(f.mul(GemmClass::LongSkip, ARows<T>(w.cat2), P.long_skip, epi));
        }
    }
    const float* mf = a.time_rows + (size_t)c.depth * 6 * D;  // (scale, shift)
    // (F5_PREC_F16P: the pre-split rows go to c1, free since the conv embedding)
    return finish<T>(f, w, w.c1, w.pred, [&](auto* out, int planar) { return adaln_norm(f, w.x, ARows(out), mf, mf + D, mod_stride, Prefetch{}, planar); });
}

// One UNetT forward over Bp packed rows (unett.py:217-280): time token prepended (N + 1 tokens per row), concat skip
// connections, x_transformers RMSNorm, no AdaLN.  a.time_rows: time embedding rows.
template <typename T> static int run_unett_forward(f5_engine* e, Work<T>& w, const ForwardArgs& a, hipStream_t s) {
    Packed<T>& P = packed<T>(e);
    const f5_config& c = e->cfg;
    const int D = c.dim, mel = c.mel_dim, B = a.B, Bp = a.Bp, N = a.N;
    const int Nt = N + 1;
    const int rows_in = Bp * N, rows = Bp * Nt;
    const int* lens_dev = a.lens_dev;
    Prof& pr = e->prof;
    float* emb = reinterpret_cast<float*>(w.cat2);  // [rows, 2D] of T >= [rows_in, D] f32; free until the first concat; conv input and output must not alias
    // the input embedding runs on the N frames of every row, unpacked and (unett.py:99-100: conv_pos_embed is called WITHOUT a mask) unmasked
    const FwdCtx in{e, s, B, Bp, N, rows_in, nullptr, RowPack{}, Rows8{}};
    if (e->io_split) CHK((embed_input<T, float>(in, w, a.y, a.cond, a.drop_cond_first, a.text_first, a.text_second, emb)));
    else CHK((embed_input<T, T>(in, w, a.y, a.cond, a.drop_cond_first, a.text_first, a.text_second, emb)));
    // The skip stack needs no copies: the stream entering block l < depth/2 is WRITTEN into skip slot l (by the assemble kernel / the
    // FF2 epilogue of block l - 1), the block's first residual update reads it there and writes w.x, and nothing writes the slot again.
    const int half = c.depth / 2;
    auto slot = [&](int l) { return w.skips + (size_t)l * rows * D; };
    HIPCHK(pr.timed(PC_MISC, s, [&] {
        launch_unett_assemble(s, emb, a.time_rows, a.time_stride, half > 0 ? slot(0) : w.x, Bp, N, D);
        return hipGetLastError();
    }));
    const FwdCtx f{e, s, B, Bp, Nt, rows, lens_dev, RowPack{}, Rows8{}};   // the blocks: N + 1 tokens per row; lens_dev holds len + 1 for UNetT
    const int pl = f.pl();
    auto rmsnorm = [&](const float* x, auto* out, const float* g, int planar) {   // out (rows of T, or pre-split f32 rows) = RMSNorm(x) * g
        return pr.timed(PC_LN, s, [&] {
            launch_xrmsnorm(s, x, out, rows, D, g, planar, f.wt(F5_WT_LN));
            return hipGetLastError();
        });
    };
    const StreamBuf<T> sb{w.x, w.xn, w.ffh, w.ao};
    for (int l = 0; l < c.depth; ++l) {
        BlockW<T>& bw = P.blocks[l];
        const float* x_in = l < half ? slot(l) : w.x;            // the stream entering the block (= skips.append(x), unett.py:258-259)
        float* x_out = l + 1 < half ? slot(l + 1) : w.x;         // where the block leaves it
        if (l >= half) {
            const float* skip = w.skips + (size_t)(c.depth - 1 - l) * rows * D;   // LIFO (skips.pop())
            HIPCHK(pr.timed(PC_MISC, s, [&] {
                launch_cat2(s, w.x, skip, w.cat2, rows, D, pl);   // (F5_PREC_F16X3: pre-split, so that the projection runs on pre-split operands too)
                return hipGetLastError();
            }));
            CHK(f.mul(GemmClass::UNetTSkip, ARows<T>(w.cat2), bw.skip, EpiStore<float>{w.x, D, nullptr, F5_ACT_NONE}));
        }
        HIPCHK(rmsnorm(x_in, w.xn, bw.norm1_g, pl));
        CHK(attention_block<T>(f, w, sb.xn, bw.x, false, EpiGateRes{w.x, x_in, D, bw.x.out.b, nullptr, 0, Nt, lens_dev, f.wt(F5_WT_GATE_RES)}));
        HIPCHK(rmsnorm(w.x, w.xn, bw.norm2_g, pl));
        CHK(ff_block<T>(f, sb, bw.x, EpiGateRes{x_out, w.x, D, bw.x.ff2.b, nullptr, 0, Nt, nullptr, f.wt(F5_WT_GATE_RES)}));
    }
    // (F5_PREC_F16P: the pre-split rows go to the skip stack's first slot: every skip has been popped)
    CHK(finish<T>(f, w, w.skips, w.pred_all, [&](auto* out, int planar) { return rmsnorm(w.x, out, P.norm_out_g, planar); }));
    HIPCHK(pr.timed(PC_MISC, s, [&] {
        launch_strip_first_token(s, w.pred_all, w.pred, Bp, N, mel);
        return hipGetLastError();
    }));
    return F5_OK;
}

// One MMDiT forward over Bp batch rows (mmdit.py:172-213, MMDiTBlock modules.py:743-771, JointAttnProcessor modules.py:555-645): the
// audio stream x [Bp, N, D] (w.x) and the text stream c [Bp, nt, D] (w.mm_c) have their own weights and AdaLN vectors and meet only
// inside one softmax over nt + N keys.  a.text_first / a.text_second: the text embeddings [B, nt, D] of the two halves.
//
// Joint layout (mmdit.h): TEXT FIRST -- positions [0, nt) are c, [nt, nt + N) are x -- so that the valid keys of batch row b, every
// text key (padded text rows included: the reference never masks them) and the audio keys below lens[b], are the prefix nt + lens[b]
// and the attention kernels run as they are.  q, k and v^T of both streams land in the joint image straight from the two QKV GEMM
// epilogues (qkv_project with a QKVJointLayout: destination offset and layout length apart from the rotary position, which counts from 0
// per stream).  The batch runs rectangular: the input conv is called without a mask (mmdit.py:78), so padded frames reach valid ones and
// are computed.
//
// Launches per block (a condition, not a measurement; tests/test_forward_launches_gpu.py holds it): 4 LayerNorm (x and c before the
// attention, x and c before the FF), 2 QKV, 1 attention, 1 split of its output into the two dense out-projection operands, 2
// out-projections, 4 FF GEMMs = 14, plus 2 norm-rope launches with qk_norm.  The last block (context_pre_only) has no text out-projection,
// LayerNorm or FF: 3 LayerNorm, 2 QKV, 1 attention, 1 split, 1 out-projection, 2 FF GEMMs = 10.  Per forward, ahead of the blocks: one
// launch that zeroes v^T (its Lpad tail columns and whatever the arena held are read by the attention's last key tile, multiplied by zero
// probabilities) and, with lengths, one launch that makes the joint key lengths.
template <typename T> static int run_mmdit_forward(f5_engine* e, Work<T>& w, const ForwardArgs& a, hipStream_t s) {
    Packed<T>& P = packed<T>(e);
    const f5_config& c = e->cfg;
    const int D = c.dim, inner = e->inner, H = c.heads, B = a.B, Bp = a.Bp, N = a.N, nt = a.nt, L = nt + N, mod_stride = a.time_stride;
    float* taps = a.taps;
    auto tap = [&](const float* src, size_t n) -> int {   // f5k_mmdit_taps (diagnostic): the next intermediate, behind the last one
        if (!taps) return F5_OK;
        HIPCHK(hipMemcpyAsync(taps, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        taps += n;
        return F5_OK;
    };
    if (nt <= 0 || nt > std::max(e->res_nt, 1) || L > w.Npad) return fail(F5_ESTATE, "MMDiT forward: nt=%d outside the arena's text reservation", nt);
    Prof& pr = e->prof;
    // the audio embedding: no text columns, the conv unmasked
    const FwdCtx in{e, s, B, Bp, N, Bp * N, nullptr, RowPack{}, Rows8{}};
    if (e->io_split) CHK((embed_input<T, float>(in, w, a.y, a.cond, a.drop_cond_first, nullptr, nullptr, w.x)));
    else CHK((embed_input<T, T>(in, w, a.y, a.cond, a.drop_cond_first, nullptr, nullptr, w.x)));
    CHK(tap(w.x, (size_t)Bp * N * D));
    const FwdCtx fx{e, s, B, Bp, N, Bp * N, a.lens_dev, RowPack{}, Rows8{}};           // the audio stream's rows
    const FwdCtx fc{e, s, B, Bp, nt, Bp * nt, nullptr, RowPack{}, Rows8{}, false};     // the text stream's rows (no F5_X3_ABLATE hooks: FwdCtx::x3)
    const StreamBuf<T> bx{w.x, w.xn, w.ffh, w.mm_aox}, bc{w.mm_c, w.mm_cn, w.mm_ffc, w.mm_aoc};
    // c = cat(c_cond, c_uncond) (mmdit.py:194), or the one half of a forward without cfg_infer
    const size_t half_c = (size_t)B * nt * D * sizeof(float);
    HIPCHK(hipMemcpyAsync(w.mm_c, a.text_first, half_c, hipMemcpyDeviceToDevice, s));
    if (Bp > B) HIPCHK(hipMemcpyAsync(w.mm_c + (size_t)B * nt * D, a.text_second, half_c, hipMemcpyDeviceToDevice, s));
    HIPCHK(pr.timed(PC_MISC, s, [&] {   // (Npad is a multiple of 64 elements: whole 16-byte pieces)
        const long n16 = (long)((size_t)Bp * H * 64 * w.Npad * sizeof(T) / 16);
        hipLaunchKernelGGL(zero_fill16_kernel, dim3(ew_blocks(n16)), dim3(256), 0, s, reinterpret_cast<uint4*>(w.vt), n16);
        return hipGetLastError();
    }));
    const int* kv_lens = nullptr;
    if (a.lens_dev) {   // mask = pad(mask, (0, nt), value=True) (modules.py:617), text first: the key prefix nt + len
        HIPCHK(pr.timed(PC_MISC, s, [&] {
            hipLaunchKernelGGL(joint_lens_kernel, dim3((Bp + 255) / 256), dim3(256), 0, s, a.lens_dev, w.mm_lens, Bp, nt);
            return hipGetLastError();
        }));
        kv_lens = w.mm_lens;
    }
    const bool qk_norm = (c.options & F5_OPT_QK_RMSNORM) != 0;
    // a stream's AdaLN LayerNorm (no prefetch), and the gated residual update of its stream by an out-projection or FF2
    auto norm = [&](const FwdCtx& f, const StreamBuf<T>& b, const float* scale, const float* shift) {
        return adaln_norm(f, b.x, b.xn, scale, shift, mod_stride, Prefetch{}, f.pl());
    };
    auto gate_res = [&](const FwdCtx& f, const StreamBuf<T>& b, const LinW<T>& lw, const float* gate, const int* lens) {
        return EpiGateRes{b.x, b.x, D, lw.b, gate, mod_stride, f.N, lens, f.wt(F5_WT_GATE_RES)};
    };
    const int row16 = inner * (int)sizeof(T) / 16;
    for (int l = 0; l < c.depth; ++l) {
        const StreamW<T>&wx = P.blocks[l].x, &wc = P.blocks[l].c;
        const bool last = l == c.depth - 1;   // context_pre_only: c is normed, attended to, and dropped
        const float* mx = a.time_rows + (size_t)l * 12 * D;   // x: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
        const float* mc = mx + 6 * D;                         // c: the same six; in the last block (scale, shift) of an AdaLayerNorm_Final
        HIPCHK(norm(fx, bx, mx + D, mx));
        HIPCHK(norm(fc, bc, last ? mc : mc + D, last ? mc + D : mc));
        CHK(qkv_project<T>(fc, w, bc.xn, wc, qk_norm, QKVJointLayout{L, 0}));
        CHK(qkv_project<T>(fx, w, bx.xn, wx, qk_norm, QKVJointLayout{L, nt}));
        // every query row is computed (q_lens null): no row of ao is left as the arena held it
        CHK(attend<T>(fx, w, qk_norm, L, kv_lens, Bp, nullptr));
        HIPCHK(pr.timed(PC_MISC, s, [&] {
            hipLaunchKernelGGL(joint_split_kernel, dim3(ew_blocks((long)Bp * L * row16)), dim3(256), 0, s, reinterpret_cast<const uint4*>(w.ao),
                               last ? nullptr : reinterpret_cast<uint4*>(bc.ao), reinterpret_cast<uint4*>(bx.ao), Bp, nt, N, row16);
            return hipGetLastError();
        }));
        if (!last) {   // the text stream: never gated by length (modules.py:643)
            CHK(out_project<T>(fc, bc.ao, wc, gate_res(fc, bc, wc.out, mc + 2 * D, nullptr)));
            HIPCHK(norm(fc, bc, mc + 4 * D, mc + 3 * D));
            CHK(ff_block<T>(fc, bc, wc, gate_res(fc, bc, wc.ff2, mc + 5 * D, nullptr)));
        }
        // the audio stream: padded rows get no attention residual (x.masked_fill(~mask, 0), modules.py:640-642) but do get the FF's
        CHK(out_project<T>(fx, bx.ao, wx, gate_res(fx, bx, wx.out, mx + 2 * D, a.lens_dev)));
        HIPCHK(norm(fx, bx, mx + 4 * D, mx + 3 * D));
        CHK(ff_block<T>(fx, bx, wx, gate_res(fx, bx, wx.ff2, mx + 5 * D, nullptr)));
        if (!last) CHK(tap(bc.x, (size_t)Bp * nt * D));
        CHK(tap(bx.x, (size_t)Bp * N * D));
    }
    const float* mf = a.time_rows + ((size_t)c.depth * 12 - 4) * D;   // norm_out: (scale, shift)
    // (F5_PREC_F16P: the pre-split rows go to c1, free since the conv embedding)
    return finish<T>(fx, w, w.c1, w.pred, [&](auto* out, int planar) { return adaln_norm(fx, w.x, ARows(out), mf, mf + D, mod_stride, Prefetch{}, planar); });
}

// One backbone forward.  What a backbone cannot run is refused here, by name, and never falls through to another backbone's body: packed
// rows exist for the DiT only (the API refuses such calls before anything is planned, engine.hip; this is the backstop).
template <typename T> static int run_backbone(f5_engine* e, Work<T>& w, const ForwardArgs& a, hipStream_t s) {
    switch (e->cfg.backbone) {
        case F5_BACKBONE_DIT: return run_dit_forward<T>(e, w, a, s);
        case F5_BACKBONE_UNETT:
            if (a.pk) return fail(F5_ESTATE, "the UNetT backbone cannot run a packed batch");
            return run_unett_forward<T>(e, w, a, s);
        case F5_BACKBONE_MMDIT:
            if (a.pk) return fail(F5_ESTATE, "the MMDiT backbone cannot run a packed batch");
            return run_mmdit_forward<T>(e, w, a, s);
    }
    return fail(F5_ESTATE, "unknown backbone %d", e->cfg.backbone);
}
// the text staging buffer is part of the arena plan: a longer text moves the carve offsets
static void reserve_text(f5_engine* e, int nt) {
    if (nt > e->res_nt) {
        e->res_nt = nt;
        e->clear_graphs();
    }
}
// uploads a call's small tables through pinned staging: nT times to w.tdev and, where lengths are given, the plan's lens and
// row_start tables (SamplePlan::Chunk) and lens_plain; for a per-item sampler call the grids, guidance, step counts and time-row
// indices, and a slice's row table.  call: the sampler call, or null (text_embed, forward: times and lengths are all there is)
template <typename T>
static int upload_small(f5_engine* e, Work<T>& w, const SamplePlan& p, const float* t_host, int nT, const int32_t* lens_host,
                        const SampleCall* call, hipStream_t s) {
    const ItemTables* it = call && call->per_item ? &call->items : nullptr;
    const int B = p.B;
    const size_t n_grid = it ? (size_t)B * (p.steps + 1) : 0, n_idx = it ? it->rows->idx.size() : 0;
    const size_t small_bytes = (size_t)nT * 4 + (size_t)3 * B * 4 + ((size_t)3 * B + 16) * 4 + 64;
    const size_t bytes = small_bytes + (it ? (n_grid + 3 * (size_t)B + n_idx) * 4 : 0);
    char* hb = nullptr;
    int slot = 0;
    CHK(e->stage.acquire(bytes, &hb, &slot));
    float* th = reinterpret_cast<float*>(hb);
    int* lh = reinterpret_cast<int*>(hb + (size_t)nT * 4);
    if (nT > 0) {
        memcpy(th, t_host, (size_t)nT * 4);
        HIPCHK(hipMemcpyAsync(w.tdev, th, (size_t)nT * 4, hipMemcpyHostToDevice, s));
    }
    if (lens_host) {
        const int add = e->cfg.backbone == F5_BACKBONE_UNETT ? 1 : 0;  // UNetT masks are left-padded for the time token
        int* rs = lh + 3 * B;
        int nrs = 0;
        for (const SamplePlan::Chunk& k : p.chunks) {
            // chunk-major: [cond lens of the chunk][uncond lens of the chunk]
            int* l = lh + p.lens_at(k);
            for (int i = 0; i < k.bc; ++i) l[i] = l[k.bc + i] = lens_host[k.u0 + i] + add;
            // RowPack table: `halves` x bc batch rows (cond half, then uncond half), each rounded up to 4 rows
            int* t = rs + p.row_start_at(k);
            t[0] = 0;
            for (int q = 0; q < p.halves * k.bc; ++q) t[q + 1] = t[q] + round_up(lens_host[k.u0 + q % k.bc], 4);
            nrs = p.row_start_at(k) + p.halves * k.bc + 1;
        }
        for (int i = 0; i < B; ++i) lh[2 * B + i] = lens_host[i] + add;
        HIPCHK(hipMemcpyAsync(w.lens, lh, (size_t)2 * B * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(w.lens_plain, lh + 2 * B, (size_t)B * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(w.row_start, rs, (size_t)nrs * 4, hipMemcpyHostToDevice, s));
    }
    if (it) {
        float* gh = reinterpret_cast<float*>(hb + small_bytes);
        float* ch = gh + n_grid;
        int* sh = reinterpret_cast<int*>(ch + B);
        int* ih = sh + B;
        memcpy(gh, it->t_items, n_grid * 4);
        memcpy(ch, it->cfg_items, (size_t)B * 4);
        memcpy(sh, it->steps_items, (size_t)B * 4);
        memcpy(ih, it->rows->idx.data(), n_idx * 4);
        HIPCHK(hipMemcpyAsync(w.it_t, gh, n_grid * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(w.it_cfg, ch, (size_t)B * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(w.it_steps, sh, (size_t)B * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(w.it_idx, ih, n_idx * 4, hipMemcpyHostToDevice, s));
        if (call->span) {   // the staging kernel's row table, in the rowmap (the staging runs before the body, which fills the rowmap of a packed plan)
            int* rh = ih + n_idx;
            memcpy(rh, call->rows_host, (size_t)B * 4);
            HIPCHK(hipMemcpyAsync(w.rowmap, rh, (size_t)B * 4, hipMemcpyHostToDevice, s));
        }
    }
    return e->stage.release(slot, s);
}
template <typename T>
int EngineOps<T>::text_embed(f5_engine* e, const int64_t* text, int B, int nt, const int32_t* lens_host, int N, int drop_text,
                             float* out, hipStream_t s) {
    if (e->cfg.backbone == F5_BACKBONE_MMDIT) reserve_text(e, nt);   // (its text buffers are sized by the longest text seen)
    CHK(ensure_arena(e, B, N, 1));
    Work<T> w;
    carve<T>(e, w, e->res_B, e->res_N, e->res_S);
    CHK(upload_small<T>(e, w, plan_sample(e, B, N, lens_host, PlanOptions::whole_batch(B)), nullptr, 0, lens_host, nullptr, s));
    const bool per_sample = lens_host && e->cfg.backbone == F5_BACKBONE_DIT;  // unett.py embeds at the padded length
    return run_text_embed<T>(e, w, text, B, nt, per_sample ? w.lens_plain : nullptr, N, drop_text, out, s);
}
// One backbone evaluation on a carved arena (f5_dit_forward, f5_flow_loss): the call's tables go up, the time path and the text
// encoder run, the prediction is left in w.pred [Bp, N, mel].
template <typename T>
static int forward_into_pred(f5_engine* e, Work<T>& w, const float* x, const float* cond, const int64_t* text, int nt, const float* time_host,
                             const int32_t* lens_host, int B, int N, int cfg_infer, int drop_audio_cond, int drop_text, hipStream_t s) {
    const int Bp = cfg_infer ? 2 * B : B;
    std::vector<float> tt(Bp);
    for (int i = 0; i < Bp; ++i) tt[i] = time_host[i % B];
    CHK(upload_small<T>(e, w, plan_sample(e, B, N, lens_host, PlanOptions::whole_batch(B)), tt.data(), Bp, lens_host, nullptr, s));
    const int* lens_dev = lens_host ? w.lens : nullptr;
    CHK(run_time_path<T>(e, w, Bp, s));
    // UNetT embeds text at the padded length for every sample (unett.py:196-215), DiT at each sample's own length
    const int* tlens = (e->cfg.backbone == F5_BACKBONE_DIT && lens_host) ? w.lens_plain : nullptr;
    // every batch row has its own time: row b of the time table
    ForwardArgs a{x, cond, B, Bp, N, time_table_dev<T>(e, w), time_width(e), lens_dev, 0, w.text_c, w.text_u, nt, RowPack{}, e->mm_taps};
    CHK(run_text_embed<T>(e, w, text, B, nt, tlens, N, cfg_infer ? 0 : drop_text, w.text_c, s));
    if (cfg_infer) CHK(run_text_embed<T>(e, w, text, B, nt, tlens, N, 1, w.text_u, s));
    else a.drop_cond_first = drop_audio_cond, a.text_second = w.text_c;
    return run_backbone<T>(e, w, a, s);
}
template <typename T>
int EngineOps<T>::forward(f5_engine* e, const float* x, const float* cond, const int64_t* text, int nt, const float* time_host,
                          const int32_t* lens_host, int B, int N, int cfg_infer, int drop_audio_cond, int drop_text, float* out,
                          hipStream_t s) {
    const int Bp = cfg_infer ? 2 * B : B;
    if (e->cfg.backbone == F5_BACKBONE_MMDIT) reserve_text(e, nt);
    CHK(ensure_arena(e, B, N, Bp));
    Work<T> w;
    carve<T>(e, w, e->res_B, e->res_N, e->res_S);
    CHK(forward_into_pred<T>(e, w, x, cond, text, nt, time_host, lens_host, B, N, cfg_infer, drop_audio_cond, drop_text, s));
    HIPCHK(hipMemcpyAsync(out, w.pred, (size_t)Bp * N * e->cfg.mel_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    return F5_OK;
}
// f5_flow_loss: the glue of csrc/flow.h around forward_into_pred.  Buffers the forward's rectangular body leaves alone carry the glue:
// w.y the mixed input phi, w.step_cond the masked conditioning (the caller's `cond` where one is given), w.rowmap the span table
// (int2[B]: a forward has no packed rows), w.y_mid the loss kernel's f64 block sums; the times are the forward's own table in w.tdev.
template <typename T>
int EngineOps<T>::flow_loss(f5_engine* e, const float* x1, const float* x0, const int64_t* text, int nt, const float* time_host,
                            const int32_t* lens_host, const int32_t* span_host, int B, int N, int drop_audio_cond, int drop_text, double* sq_sum,
                            int32_t* count, float* pred, float* cond, float* frame_err, hipStream_t s) {
    const int mel = e->cfg.mel_dim;
    if (e->cfg.backbone == F5_BACKBONE_MMDIT) reserve_text(e, nt);
    CHK(ensure_arena(e, B, N, B));
    Work<T> w;
    carve<T>(e, w, e->res_B, e->res_N, e->res_S);
    static_assert(sizeof(int2) == 2 * sizeof(int32_t), "a span is one int2");
    CHK(e->stage.upload(w.rowmap, (size_t)B * sizeof(int2), s, [&](char* hb) { memcpy(hb, span_host, (size_t)B * sizeof(int2)); }));
    // (the times are needed before the forward uploads them: the same values, to the same place)
    CHK(e->stage.upload(w.tdev, (size_t)B * sizeof(float), s, [&](char* hb) { memcpy(hb, time_host, (size_t)B * sizeof(float)); }));
    float* cond_buf = cond ? cond : w.step_cond;
    launch_flow_mix(s, x0, x1, w.tdev, w.rowmap, w.y, cond_buf, B, N, mel);
    KCHK();
    CHK(forward_into_pred<T>(e, w, w.y, cond_buf, text, nt, time_host, lens_host, B, N, 0, drop_audio_cond, drop_text, s));
    launch_flow_loss(s, w.pred, x0, x1, w.rowmap, reinterpret_cast<double*>(w.y_mid), sq_sum, count, frame_err, B, N, mel);
    KCHK();
    if (pred) HIPCHK(hipMemcpyAsync(pred, w.pred, (size_t)B * N * mel * sizeof(float), hipMemcpyDeviceToDevice, s));
    return F5_OK;
}
// the second (unconditional) half of every [2B ...] activation buffer a DiT forward writes, as a Work of its own: behind the B * N rows
// of the first half, in the element type the forward writes each buffer in (F5_PREC_F16P: acat and the long-skip cat2 hold f32 rows)
template <typename T> static Work<T> second_half(const f5_engine* e, const Work<T>& w, int B, int N) {
    const f5_config& c = e->cfg;
    const size_t rows = (size_t)B * N;
    Work<T> h = w;
    const size_t io = e->io_split ? sizeof(float) / sizeof(T) : 1;
    h.acat = w.acat + rows * e->kin_pad * io;
    h.h = w.h + rows * c.dim;
    h.c1 = w.c1 + rows * c.dim;
    h.x = w.x + rows * c.dim;
    h.pred = w.pred + rows * c.mel_dim;
    h.xn = w.xn + rows * c.dim;
    h.q = w.q + rows * e->inner;
    h.k = w.k + rows * e->inner;
    h.ao = w.ao + rows * e->inner;
    h.vt = w.vt + (size_t)B * c.heads * 64 * w.Npad;
    h.ffh = w.ffh + rows * c.ff_dim;
    if (e->f8) h.a8 = w.a8.at_pitch(a8_pitch(e)).from_row(rows);   // (rows of the widest K, and one scale byte per row)
    if (c.options & F5_OPT_LONG_SKIP) h.cat2 = w.cat2 + rows * 2 * c.dim * io;
    return h;
}
// The unconditional text embedding (every token replaced by the filler) of a single utterance depends only on the weights
// and N -- unless text_mask_padding zeroes the rows whose ORIGINAL token is the filler (dit.py:90-91,104-108: the mask is
// taken before drop_text), which makes it a function of the call's text: no cache then.
static bool uc_cacheable(const f5_engine* e, int B, bool has_lens) {
    if (e->cfg.backbone == F5_BACKBONE_MMDIT) return false;   // (its text stream is [nt, D], a lookup: nothing worth keeping)
    return B == 1 && !has_lens && !(e->cfg.text_mask_padding && e->cfg.conv_layers > 0) && !(e->cfg.options & F5_OPT_TEXT_AVG_UPSAMPLE);
}

// the stream-ordered body of sample(): everything between "inputs are in the arena" and "outputs are in the arena".
// w.tdev holds the evaluation times (feature rows) and then the grid (engine.hip time_table).
template <typename T> static int sample_body(f5_engine* e, Work<T>& w, const SamplePlan& p, hipStream_t s) {
    const f5_config& c = e->cfg;
    const int mel = c.mel_dim, B = p.B, N = p.N;
    const bool mid = p.method == F5_ODE_MIDPOINT;
    const float* tgrid = mid ? w.tdev + 2 * p.steps : w.tdev;
    const int* lens_dev = p.has_lens ? w.lens : nullptr;
    const long half = (long)B * N * mel;
    const int64_t* text = reinterpret_cast<const int64_t*>(w.in_text);
    // step_cond = where(cond_mask, cond, 0)   (cfm.py:151-153)
    HIPCHK(e->prof.timed(PC_MISC, s, [&] {
        launch_select_rows(s, w.in_cond, nullptr, w.in_mask, w.step_cond, (long)B * N, mel);
        return hipGetLastError();
    }));
    CHK(run_time_path<T>(e, w, p.items ? p.U : p.evals * p.steps, s));  // features of every evaluation time
    const int* tlens = (c.backbone == F5_BACKBONE_DIT && p.has_lens) ? w.lens_plain : nullptr;
    CHK(run_text_embed<T>(e, w, text, B, p.nt, tlens, N, 0, w.text_c, s));
    if (p.use_cfg) {
        const size_t ucn = (size_t)N * c.text_dim;
        if (uc_cacheable(e, B, p.has_lens) && e->uc_N == N) {
            HIPCHK(hipMemcpyAsync(w.text_u, w.uc, ucn * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            CHK(run_text_embed<T>(e, w, text, B, p.nt, tlens, N, 1, w.text_u, s));
            if (uc_cacheable(e, B, p.has_lens)) {   // (never reached under capture: a cache miss always runs eagerly)
                HIPCHK(hipMemcpyAsync(w.uc, w.text_u, ucn * sizeof(float), hipMemcpyDeviceToDevice, s));
                e->uc_N = N;
            }
        }
    }
    if (p.want_traj) HIPCHK(hipMemcpyAsync(w.traj_buf, w.y, half * sizeof(float), hipMemcpyDeviceToDevice, s));
    Work<T> w2 = w;
    if (p.split) {
        w2 = second_half<T>(e, w, B, N);
        if (!e->side_stream) HIPCHK(hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking));
        if (!e->ev_fork) HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        if (!e->ev_join) HIPCHK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }
    // packed variable-length batch (RowPack): the row tables of every chunk, built once from the uploaded prefix sums
    std::vector<RowPack> packs(p.chunks.size());
    for (const SamplePlan::Chunk& k : p.chunks) {
        if (!p.pack) break;
        const int* rs = w.row_start + p.row_start_at(k);
        packs[k.idx] = RowPack{rs, w.rowmap + p.rowmap_at(k), rs + p.halves * k.bc, k.rows, k.sq};
        launch_fill_rowmap(s, rs, w.rowmap + p.rowmap_at(k), p.halves * k.bc);
        KCHK();
    }
    // one (CFG) evaluation of a chunk at state x with the vectors of time row `row`, into w.pred
    auto eval = [&](const SamplePlan::Chunk& k, const RowPack& pk, const float* x, int row) -> int {
        const bool mmdit = c.backbone == F5_BACKBONE_MMDIT;   // (its text embeddings are [B, nt, D])
        const size_t yo = p.frame_at(k) * mel, to = mmdit ? (size_t)k.u0 * p.nt * c.dim : p.frame_at(k) * c.text_dim;
        const float *cond = w.step_cond + yo, *tc = w.text_c + to, *tu = w.text_u + to;
        const int* lens = lens_dev ? lens_dev + p.lens_at(k) : nullptr;
        const int tw = time_width(e);
        // both halves in one batch, every batch row at time row `row`
        ForwardArgs a{x, cond, k.bc, p.halves * k.bc, N, time_table_dev<T>(e, w) + (size_t)row * tw, 0, lens, 0, tc, p.use_cfg ? tu : tc, p.nt, pk, nullptr};
        if (p.items) {   // per-item times: evaluation `row` reads, for every batch row of the chunk, the time row its item is at
            HIPCHK(e->prof.timed(PC_MISC, s, [&] {
                launch_mod_gather(s, time_table_dev<T>(e, w), w.it_idx + (size_t)row * B + k.u0, w.mod_rows, a.Bp, k.bc, tw);
                return hipGetLastError();
            }));
            a.time_rows = w.mod_rows;
            a.time_stride = tw;
        }
        if (!p.split) return run_backbone<T>(e, w, a, s);
        // conditional chain on s, unconditional chain (cond dropped, filler text) on the side stream: each half a batch of its own
        hipStream_t s1 = e->side_stream;
        HIPCHK(hipEventRecord(e->ev_fork, s));            // x (and, first time, the text embeddings) ready
        HIPCHK(hipStreamWaitEvent(s1, e->ev_fork, 0));
        a.Bp = k.bc;
        a.pk = RowPack{};
        a.text_second = tc;
        CHK(run_backbone<T>(e, w, a, s));
        a.drop_cond_first = 1;
        a.text_first = a.text_second = tu;
        CHK(run_backbone<T>(e, w2, a, s1));
        HIPCHK(hipEventRecord(e->ev_join, s1));
        HIPCHK(hipStreamWaitEvent(s, e->ev_join, 0));
        return F5_OK;
    };
    // y_mid = y + f(t[i], y) * dt/2
    auto half_update = [&](const SamplePlan::Chunk& k, const RowPack& pk, int i) {
        const size_t yo = p.frame_at(k) * mel;
        return e->prof.timed(PC_MISC, s, [&] {
            if (p.items) {
                launch_midpoint_half_cfg_items(s, w.y + yo, w.pred, k.bc, N, mel, pk.row_start, pk ? lens_dev + p.lens_at(k) : nullptr,
                                               w.it_t + (size_t)k.u0 * (p.steps + 1), w.it_cfg + k.u0, w.it_steps + k.u0, p.steps, i,
                                               p.use_cfg ? 1 : 0, w.y_mid + yo);
                return hipGetLastError();
            }
            launch_midpoint_half_cfg(s, w.y + yo, w.pred, k.bc, N, mel, pk.row_start, pk ? lens_dev + p.lens_at(k) : nullptr, tgrid, i,
                                     p.cfg_strength, p.use_cfg ? 1 : 0, w.y_mid + yo);
            return hipGetLastError();
        });
    };
    // y += f * dt (f: Euler at t[i], y; midpoint at t[i] + dt/2, y_mid), copied to the trajectory slot of step i + 1
    auto full_update = [&](const SamplePlan::Chunk& k, const RowPack& pk, int i) {
        const size_t yo = p.frame_at(k) * mel;
        float* slot = p.want_traj ? w.traj_buf + (size_t)(i + 1) * half + yo : nullptr;
        return e->prof.timed(PC_MISC, s, [&] {
            if (p.items) {
                launch_euler_cfg_items(s, w.y + yo, w.pred, k.bc, N, mel, pk.row_start, pk ? lens_dev + p.lens_at(k) : nullptr,
                                       w.it_t + (size_t)k.u0 * (p.steps + 1), w.it_cfg + k.u0, w.it_steps + k.u0, p.steps, i,
                                       p.use_cfg ? 1 : 0, slot);
                return hipGetLastError();
            }
            launch_euler_cfg(s, w.y + yo, w.pred, k.bc, N, mel, pk.row_start, pk ? lens_dev + p.lens_at(k) : nullptr, tgrid, i, p.cfg_strength,
                             p.use_cfg ? 1 : 0, slot);
            return hipGetLastError();
        });
    };
    for (int i = 0; i < p.steps; ++i)
        for (const SamplePlan::Chunk& k : p.chunks) {
            const RowPack& pk = packs[k.idx];
            const size_t yo = p.frame_at(k) * mel;
            CHK(eval(k, pk, w.y + yo, p.evals * i));
            if (mid) {
                HIPCHK(half_update(k, pk, i));
                CHK(eval(k, pk, w.y_mid + yo, 2 * i + 1));
            }
            HIPCHK(full_update(k, pk, i));
        }
    // out = where(cond_mask, cond, y)   (cfm.py:221-223)
    HIPCHK(e->prof.timed(PC_MISC, s, [&] {
        launch_select_rows(s, w.in_cond, w.y, w.in_mask, w.out_buf, (long)B * N, mel);
        return hipGetLastError();
    }));
    return F5_OK;
}
// Whether a sample() call takes a length bucket (Switches::len_bucket), and the ceiling it is planned at.  Eligible: the DiT, every
// utterance as long as the batch (lens NULL or all equal to N: masked and unmasked semantics then coincide, so the packed body serves
// both), one stream chain, no profiler, and a ceiling inside the rotary / text position tables.  text_embedding_average_upsampling
// stays on the exact path.  Everything else takes the exact path with the exact key, silently.
template <typename T> static bool bucket_eligible(f5_engine* e, const int32_t* lens_host, int B, int N, int* n_cap) {
    const f5_config& c = e->cfg;
    const int g = e->sw.len_bucket;
    if (g <= 0 || c.backbone != F5_BACKBONE_DIT || e->sw.split_cfg || e->prof.on || (c.options & F5_OPT_TEXT_AVG_UPSAMPLE)) return false;
    for (int i = 0; lens_host && i < B; ++i)
        if (lens_host[i] != N) return false;
    const int nc = round_up(N, g);
    if (nc + 1 > c.max_pos || (c.conv_layers > 0 && nc > packed<T>(e).text_pos_rows)) return false;
    *n_cap = nc;
    return true;
}
// An isolated per-item call (Switches::isolated_rows): every row as if it were alone in the batch, which the packed body gives -- the text
// embedded per row at its own length, conv-pos and attention keys masked there, everything else row-wise.  That is a promise, so a call
// that cannot run on the packed body is refused, naming the reason, instead of running rectangular: the UNetT (never packed),
// F5_SPLIT_CFG (steps padded rows per half), text_embedding_average_upsampling (stays on the exact path, as for length buckets) and a
// ceiling outside the rotary or text position tables.  *n_cap: the frames the call is planned at -- its length bucket's ceiling, or N rounded up to 4.
template <typename T> static int isolated_ceiling(f5_engine* e, const char* who, int N, int* n_cap) {
    const f5_config& c = e->cfg;
    if (c.backbone != F5_BACKBONE_DIT)
        return fail(F5_EINVAL, "%s: isolated rows (f5_set_isolated_rows) run on packed rows, which the UNetT backbone does not have", who);
    if (e->sw.split_cfg) return fail(F5_EINVAL, "%s: isolated rows (f5_set_isolated_rows) cannot run with F5_SPLIT_CFG=1 (it steps padded rows)", who);
    if (c.options & F5_OPT_TEXT_AVG_UPSAMPLE)
        return fail(F5_EINVAL, "%s: isolated rows (f5_set_isolated_rows) cannot run with text_embedding_average_upsampling "
                               "(F5_OPT_TEXT_AVG_UPSAMPLE stays on the exact path)", who);
    // Without buckets the ceiling is N rounded up to 4, the granule of a packed batch row: the launch geometry is that of B rows of the
    // ceiling, and rows that fill their N (a B = 1 call always does) would otherwise pack into more rows than it has.
    const int g = e->sw.len_bucket, nc = round_up(N, g > 0 ? g : 4);
    if (nc + 1 > c.max_pos)
        return fail(F5_EINVAL, "%s: isolated rows: N=%d is planned at %d frames, which exceeds the rotary table (max_pos = %d rows)", who, N, nc,
                    c.max_pos);
    if (c.conv_layers > 0 && nc > packed<T>(e).text_pos_rows)
        return fail(F5_EINVAL, "%s: isolated rows: N=%d is planned at %d frames, which exceeds aux.text_pos (%d rows)", who, N, nc,
                    packed<T>(e).text_pos_rows);
    *n_cap = nc;
    return F5_OK;
}
// The body of one planned call whose inputs are in the arena: replay the captured graph of its key, capture it when the signature has run
// before, else run eagerly (and remember it).  N: the call's own frame count (the cached unconditional text embedding is kept per N).
template <typename T> static int launch_sample_body(f5_engine* e, Work<T>& w, const SamplePlan& p, int N, hipStream_t s) {
    const int B = p.B;
    // ---- key: the signature, and whether the body reads the cached unconditional text embedding (a call that stores it runs eagerly)
    const bool uc_ok = p.use_cfg && uc_cacheable(e, B, p.has_lens);
    const bool uc_hit = uc_ok && e->uc_N == N;
    const std::string base_key = graph_key(p), key = base_key + (uc_hit ? "|uc" : "|nouc");
    // ---- body: replay the captured graph of this key, capture it when the signature has run before, else run eagerly (and remember it)
    static const bool trace = getenv("F5_TRACE") && getenv("F5_TRACE")[0] == '1';   // diagnostic: which path a call takes
    const auto t_body = std::chrono::steady_clock::now();
    hipGraphExec_t exec = nullptr;
    const char* how = "eager launches";
    if (e->sw.graphs && !e->gc.disabled && !e->prof.on && !(uc_ok && !uc_hit)) {
        if ((exec = e->gc.find(key))) {
            how = "graph replay";
            e->gc.stats.replays++;
        } else if (e->gc.is_warm(base_key)) {
            CHK(e->gc.capture(key, [&](hipStream_t cs) { return sample_body<T>(e, w, p, cs); }, &exec));
            if (exec) how = "graph capture + instantiate + launch";
        }
    }
    if (exec) {
        HIPCHK(hipGraphLaunch(exec, s));
        CHK(e->gc.launched(exec, s));
    } else {
        CHK(sample_body<T>(e, w, p, s));
        e->gc.stats.eager++;
    }
    if (trace)
        fprintf(stderr, "libf5hip: sample %s [%s]: host %.3f ms\n", key.c_str(), how,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_body).count());
    if (!exec) e->gc.mark_warm(base_key);
    return F5_OK;
}
// a per-item call's buffers and its time rows (one per distinct evaluation time) are part of the arena plan: a first call, or more rows, moves the carve offsets
static void reserve_items(f5_engine* e, int U) {
    if (!e->res_items || U > e->res_U) {
        e->res_items = true;
        e->res_U = std::max(e->res_U, U);
        e->clear_graphs();
        e->uc_N = -1;
    }
}
// `rows` rows of `width` bytes from pitch `spitch` to pitch `dpitch`, device to device: one flat copy where both pitches are the width
static hipError_t copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t s) {
    if (dpitch == width && spitch == width) return hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToDevice, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, s);
}
// Every sampler call (f5_sample, f5_sample_ode, f5_sample_items, f5_sample_span): plan, stage the inputs into the arena, key, replay /
// capture / eager (launch_sample_body), copy the outputs.  The staging is eager, on the caller's stream, so none of it is part of the
// body's key: one captured graph serves every setting of a per-item shape, and every slice of it.
template <typename T> int EngineOps<T>::run_sample(f5_engine* e, const SampleCall& c) {
    const int B = c.B, N = c.N, nt = c.nt, mel = e->cfg.mel_dim;
    hipStream_t s = c.stream;
    // ---- (a) the plan: per-item tables on the rectangular body at the exact N -- or, isolated, on packed rows with every row's own length --
    // or one grid for the batch; in N's length bucket if the call takes one
    int Nc = N;   // frames per utterance in the arena: N, or the ceiling of N's length bucket
    const bool iso = c.per_item && e->sw.isolated_rows;
    if (iso) CHK(isolated_ceiling<T>(e, c.who, N, &Nc));   // (refused before anything is reserved, staged or launched)
    reserve_text(e, nt);
    const bool bucket = iso ? e->sw.len_bucket > 0 : !c.per_item && bucket_eligible<T>(e, c.lens_host, B, N, &Nc);
    PlanOptions o = plan_options(c);
    if (bucket) o.nt = e->res_nt;
    if (bucket && !iso) o.n_true = N;
    std::vector<float> times_iso;     // an isolated call's time rows, the last one repeated up to the next power of two
    std::vector<int32_t> lens_iso;    // ... and its lengths (lens_host NULL: every row has N frames)
    if (iso) {
        o.isolated = true;
        o.bucket = bucket;
        while (o.U & (o.U - 1)) o.U += o.U & -o.U;
        times_iso = c.items.rows->times;
        times_iso.resize((size_t)o.U, times_iso.back());
        lens_iso = c.lens_host ? std::vector<int32_t>(c.lens_host, c.lens_host + B) : std::vector<int32_t>((size_t)B, N);
    }
    const SamplePlan p = plan_sample(e, B, Nc, iso ? lens_iso.data() : c.lens_host, o);
    if (c.per_item) reserve_items(e, p.U);
    CHK(ensure_arena(e, B, Nc, c.steps));
    Work<T> w;
    carve<T>(e, w, e->res_B, e->res_N, e->res_S);
    // ---- inputs -> arena
    const std::vector<float> grid = c.per_item ? std::vector<float>() : time_table(c.t_host, c.steps, c.method);
    const std::vector<float>& times = iso ? times_iso : c.per_item ? c.items.rows->times : grid;
    const std::vector<int32_t> own(bucket && !iso ? B : 0, N);
    CHK(upload_small<T>(e, w, p, times.data(), (int)times.size(), iso ? lens_iso.data() : bucket ? own.data() : c.lens_host, &c, s));
    const size_t frame = (size_t)mel * sizeof(float), row_in = N * frame, row_arena = Nc * frame;   // one utterance, caller's / arena's
    const size_t half = (size_t)B * row_arena;
    if (c.cond_frames < Nc) HIPCHK(hipMemsetAsync(w.in_cond, 0, half, s));   // F.pad(cond, ..., N - cond_seq_len) (cfm.py:145)
    if (c.cond_frames > 0)   // (the prompt's own pitch is its frame count)
        HIPCHK(hipMemcpy2DAsync(w.in_cond, row_arena, c.cond, c.cond_frames * frame, c.cond_frames * frame, B, hipMemcpyDeviceToDevice, s));
    // A bucket's frames N .. Nc-1 of state and mask are written as zero (the two select_rows launches of the body read them; nothing reads
    // what they produce), and its text sits in rows of res_nt tokens filled with -1: the filler, which is what a shorter text is
    // padded with anyway (dit.py:87-89), so the body reads the same tokens whatever the call's own text length.
    if (N < Nc) {
        HIPCHK(hipMemsetAsync(w.y, 0, half, s));
        HIPCHK(hipMemsetAsync(w.in_mask, 0, (size_t)B * Nc, s));
    }
    // ---- (b) the start state: the caller's y0, or the rows of a previous state (another N, another row order) and of y_new, by one launch
    if (c.span) {
        launch_span_stage(s, w.y, c.prev_state, c.y_new, reinterpret_cast<const int*>(w.rowmap), B, N, c.prev_N, mel, Nc);
        KCHK();
    } else
        HIPCHK(copy_rows(w.y, row_arena, c.y0, row_in, row_in, B, s));
    HIPCHK(copy_rows(w.in_mask, (size_t)Nc, c.cond_mask, (size_t)N, (size_t)N, B, s));
    if (nt < p.nt) HIPCHK(hipMemsetAsync(w.in_text, 0xFF, (size_t)B * p.nt * sizeof(int64_t), s));
    HIPCHK(copy_rows(w.in_text, p.nt * sizeof(int64_t), c.text, nt * sizeof(int64_t), nt * sizeof(int64_t), B, s));
    CHK(launch_sample_body<T>(e, w, p, N, s));
    // ---- outputs -> caller (a bucket's rows N .. Nc-1 stay behind)
    HIPCHK(copy_rows(c.out, row_in, w.out_buf, row_arena, row_in, B, s));
    // ---- (c) beside `out`: a slice's raw state, or the trajectory
    if (c.span) HIPCHK(copy_rows(c.state_out, row_in, w.y, row_arena, row_in, B, s));
    else if (c.traj)
        HIPCHK(copy_rows(c.traj, row_in, w.traj_buf, row_arena, row_in, (size_t)(c.steps + 1) * B, s));
    return F5_OK;
}
// f5_prepare_sample: one graph per length bucket of [n_min, n_max], captured and instantiated without a launch.  The arena is sized for
// the largest bucket first, so that no call inside the range moves it (and with it every captured pointer).
template <typename T>
int EngineOps<T>::prepare(f5_engine* e, int B, int n_min, int n_max, int nt_max, int steps, float cfg_strength, int method, bool want_traj) {
    const int g = e->sw.len_bucket, c0 = round_up(n_min, g), c1 = round_up(n_max, g);
    if (e->cfg.conv_layers > 0 && c1 > packed<T>(e).text_pos_rows)
        return fail(F5_EINVAL, "f5_prepare_sample: n_max=%d is planned at %d frames, which exceeds aux.text_pos (%d rows)", n_max, c1,
                    packed<T>(e).text_pos_rows);
    reserve_text(e, nt_max);
    CHK(ensure_arena(e, B, c1, steps));
    e->gc.capacity = std::max<size_t>(e->gc.capacity, (size_t)(c1 - c0) / g + 1);
    Work<T> w;
    carve<T>(e, w, e->res_B, e->res_N, e->res_S);
    PlanOptions o;   // the plan run_sample makes of a call of nc frames in the bucket of ceiling nc
    o.nt = e->res_nt; o.steps = steps; o.method = method; o.cfg_strength = cfg_strength; o.want_traj = want_traj;
    for (int nc = c0; nc <= c1; nc += g) {
        o.n_true = nc;
        const SamplePlan p = plan_sample(e, B, nc, nullptr, o);
        const std::string key = graph_key(p) + "|nouc";
        e->gc.mark_warm(graph_key(p));   // prepared counts as seen: a bucket whose graph is pushed out captures again on its next call
        if (e->gc.find(key)) continue;
        hipGraphExec_t exec = nullptr;
        CHK(e->gc.capture(key, [&](hipStream_t cs) { return sample_body<T>(e, w, p, cs); }, &exec));
        if (!exec) return fail(F5_EHIP, "f5_prepare_sample: the HIP graph of bucket %d could not be captured", nc);
    }
    return F5_OK;
}

// ------------------------------------------------------------------------------------------ EngineOps<T>
template <typename T> int EngineOps<T>::finalize(f5_engine* e, hipStream_t s) { return finalize_t<T>(e, packed<T>(e), s); }
template <typename T> size_t EngineOps<T>::plan_bytes(const f5_engine* e, int B, int N, int S) {
    Arena dry;  // base == nullptr: measures only
    Work<T> w;
    return carve_into<T>(e, dry, w, B, N, S);
}
// f5k_work_plan: where carve_into puts every buffer of Work<T> for the reservation (B, N, S), and where second_half puts the side chain of a
// split-CFG call of call_B x call_N, as byte offsets into the arena (-1: not carved), in the order of F5K_WORK_NAMES (include/f5_hip.h)
template <typename T>
size_t EngineOps<T>::work_plan(const f5_engine* e, int B, int N, int S, int call_B, int call_N, int64_t* main_off, int64_t* side_off) {
    Arena dry;
    dry.base = reinterpret_cast<char*>((size_t)1 << 30);   // a dry run from a non-null address (nothing is dereferenced): null then means "not carved"
    Work<T> w;
    const size_t total = carve_into<T>(e, dry, w, B, N, S);
    const Work<T> h = second_half<T>(e, w, call_B, call_N);
    auto put = [&](int64_t* out, const Work<T>& v) {
        const void* p[] = {v.tdev, v.feat, v.th, v.temb, v.st, v.mod, v.lens, v.lens_plain, v.row_start, v.rowmap, v.step_cond, v.text_c, v.text_u,
                           v.tx_a, v.tx_b, v.tx_h1, v.grn_part, v.uc, v.acat, v.h, v.c1, v.x, v.pred, v.xn, v.q, v.k, v.ao, v.vt, v.ffh, v.a8.codes,
                           v.a8.scales, v.in_cond, v.y, v.y_mid, v.out_buf, v.traj_buf, v.in_mask, v.in_text, v.cat2, v.skips, v.pred_all, v.mod_rows,
                           v.it_t, v.it_cfg, v.it_steps, v.it_idx};
        static_assert(sizeof(p) / sizeof(p[0]) == F5K_WORK_BUFFERS, "one entry per name of F5K_WORK_NAMES");
        for (int i = 0; i < F5K_WORK_BUFFERS; ++i) out[i] = p[i] ? (int64_t)(static_cast<const char*>(p[i]) - dry.base) : -1;
    };
    put(main_off, w);
    put(side_off, h);
    dry.base = nullptr;   // (not an allocation: nothing to free)
    return total;
}
