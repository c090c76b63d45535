// Kernel-level C entry points (f5k_*): each runs ONE kernel of the engine on fp32 inputs so that tests/ can compare it
// with a torch fp32 restatement, and the micro-benchmarks can time it.  Scratch is allocated per call; every function
// synchronises the stream before returning.
#include "kapi_common.h"

// tile_m / tile_n of f5k_gemm / f5k_gemm_time as a forced cfg: tile_m > 0 a v1 tile (BM, BN), tile_m < 0 the tile id -tile_m, 0 auto
static int forced_cfg(int tm, int tn) { return tm > 0 ? tm * 1000 + tn : tm < 0 ? -tm : -1; }
static bool v1_tile(int cfg) { return gemm_tile(cfg) && gemm_tile(cfg)->family == GEMM_V1; }   // (K is then padded to 16 bytes only)

template <typename T>
static int gemm_impl(const float* A, const float* W, const float* bias, int act, float* out, int M, int N, int K, int cfg, GemmOperands ops,
                     hipStream_t s) {
    const int Kp = round_up(K, v1_tile(cfg) ? 8 : GEMM_ROW_BYTES / (int)sizeof(T));
    if (cfg == G3_256x256_PP && !gemm_has_pingpong(sizeof(T), ops)) return fail(F5_EINVAL, "f5k_gemm: no ping-pong kernel (cfg 20) for these operands");
    GemmStage<T> g;
    CHK(g.stage(s, A, K, W, K, M, N, K, Kp, ops));
    HIPCHK(launch_gemm<T>(s, g.a.p, Kp, g.w.p, Kp, M, N, Kp, EpiStore<float>{out, N, bias, act}, {ops, cfg}));
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

extern "C" int f5k_gemm(int32_t prec, const float* A, const float* W, const float* bias, int32_t act, float* out, int32_t M,
                        int32_t N, int32_t K, int32_t tm, int32_t tn, f5_stream stream) {
    if (!A || !W || !out || M <= 0 || N <= 0 || K <= 0 || (N % 4)) return fail(F5_EINVAL, "f5k_gemm: bad arguments (N %% 4 == 0)");
    const int cfg = forced_cfg(tm, tn);
    if (tm != 0 && (!gemm_tile(cfg) || v1_tile(cfg) != (tm > 0))) return fail(F5_EINVAL, "f5k_gemm: bad tile (tile_m > 0) or tile id (tile_m < 0)");
    // F5_PREC_F16X3: the f32 instantiation with W pre-split; with tile_n == 5 A as well (what store4_planar producers hand the block GEMMs)
    const GemmOperands ops = prec != F5_PREC_F16X3 ? GemmOperands::Plain : (tm <= 0 && tn == 5) ? GemmOperands::AWSplit : GemmOperands::WSplit;
    if (ops != GemmOperands::Plain && tm > 0) return fail(F5_EINVAL, "f5k_gemm: the split-operand mode has no v1 kernel");
    return F5K_BY_PREC(prec, gemm_impl, A, W, bias, act, out, M, N, K, cfg, ops, (hipStream_t)stream);
}

// launch_gemm's decision for one problem, without launching (plan_gemm, gemm_dispatch.h): pure host arithmetic, no HIP call
extern "C" int f5k_gemm_plan(int32_t elem_size, int32_t M, int32_t N, int32_t K, int32_t has_m_limit, int32_t m_hint, int32_t operand_form,
                             int32_t conv, int32_t pp_epilogue, int32_t force_cfg, int32_t env_cfg, int32_t env_cfg_n, int32_t* plan) {
    if (!plan || (elem_size != 1 && elem_size != 2 && elem_size != 4) || operand_form < 0 || operand_form > 2) return fail(F5_EINVAL, "f5k_gemm_plan: bad arguments");
    const GemmPlan g = plan_gemm({elem_size, M, N, K, has_m_limit != 0, m_hint, (GemmOperands)operand_form, conv != 0, pp_epilogue != 0, force_cfg, env_cfg, env_cfg_n});
    plan[0] = g.ok ? g.n : -1;
    static_assert(sizeof(g.l) == 8 * sizeof(int32_t), "two launches of four ints");
    memcpy(plan + 1, g.l, sizeof(g.l));   // (launches past n are zero)
    return F5_OK;
}

// three warm-up launches of go(), then `iters` of them between two events: the average microseconds of one
template <typename F> static int time_launches(hipStream_t s, int iters, float* avg_us, F&& go) {
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) HIPCHK(go());
    HIPCHK(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) HIPCHK(go());
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.0f / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return F5_OK;
}

template <typename T>
static int gemm_time_impl(int M, int N, int K, int cfg, GemmOperands ops, int iters, float* avg_us, hipStream_t s) {
    const int Kp = round_up(K, v1_tile(cfg) ? 8 : GEMM_ROW_BYTES / (int)sizeof(T));
    if (cfg == G3_256x256_PP && !gemm_has_pingpong(sizeof(T), ops)) return fail(F5_EINVAL, "f5k_gemm_time: no ping-pong kernel (cfg 20) for these operands");
    Scratch<T> o;
    HIPCHK(o.alloc((size_t)M * N));
    // random-ish operand bits (bench on non-zero data: MI355X_MICROARCH "DVFS give-back")
    Scratch<float> tmp;
    const size_t nmax = std::max((size_t)M, (size_t)N) * Kp;
    HIPCHK(tmp.alloc(nmax));
    std::vector<float> h(nmax);
    unsigned x = 12345u;
    for (size_t i = 0; i < nmax; ++i) {
        x = x * 1664525u + 1013904223u;
        h[i] = ((x >> 8) & 0xFFFF) / 32768.0f - 1.0f;
    }
    HIPCHK(hipMemcpy(tmp.p, h.data(), nmax * 4, hipMemcpyHostToDevice));
    GemmStage<T> g;
    CHK(g.stage(s, tmp.p, Kp, tmp.p, Kp, M, N, Kp, Kp, GemmOperands::Plain));   // (timing only: the random W bits are used as they are)
    return time_launches(s, iters, avg_us, [&] { return launch_gemm<T>(s, g.a.p, Kp, g.w.p, Kp, M, N, Kp, EpiStore<T>{o.p, N, nullptr, 0}, {ops, cfg}); });
}

// F5_PREC_F8: the e4m3 kernel on random codes (scale bytes 127) into f16 rows; with_quant: the stand-alone row quantiser of an f16 A
// operand [M, K] runs inside the timed region, as FwdCtx::mul launches it in front of the out-projection and FF2
static int gemm_time_f8_impl(int M, int N, int K, int cfg, bool with_quant, int iters, float* avg_us, hipStream_t s) {
    if (K % GEMM_ROW_BYTES) return fail(F5_EINVAL, "f5k_gemm_time: F5_PREC_F8 needs K %% 128 == 0");
    Scratch<unsigned char> a8, w8, as, ws;
    Scratch<f16_t> o, a16;
    HIPCHK(a8.alloc((size_t)M * K));
    HIPCHK(w8.alloc((size_t)N * K));
    HIPCHK(as.alloc((size_t)M + 16));
    HIPCHK(ws.alloc((size_t)N + 16));
    HIPCHK(o.alloc((size_t)M * N));
    HIPCHK(a16.alloc((size_t)M * K));
    const size_t nmax = std::max((size_t)M, (size_t)N) * K;
    std::vector<unsigned char> h(nmax);
    unsigned x = 12345u;
    for (size_t i = 0; i < nmax; ++i) {   // random finite codes (exponent field below 15), non-zero data
        x = x * 1664525u + 1013904223u;
        h[i] = (unsigned char)((x >> 9) & 0xF7u);
    }
    HIPCHK(hipMemcpy(a8.p, h.data(), (size_t)M * K, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(w8.p, h.data(), (size_t)N * K, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(as.p, 127, (size_t)M + 16));
    HIPCHK(hipMemset(ws.p, 127, (size_t)N + 16));
    std::vector<uint16_t> h16((size_t)M * K);
    for (size_t i = 0; i < h16.size(); ++i) {   // f16 values in (-2, 2)
        x = x * 1664525u + 1013904223u;
        h16[i] = (uint16_t)(((x >> 8) & 0x83FFu) | 0x3C00u);
    }
    HIPCHK(hipMemcpy(a16.p, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
    const Rows8 a{a8.p, as.p, K}, w{w8.p, ws.p, K};
    return time_launches(s, iters, avg_us, [&] {
        if (with_quant) launch_quant_rows_e4m3<f16_t>(s, a16.p, K, M, K, a, nullptr);
        GemmOpts op{GemmOperands::Plain, cfg};
        op.a_scale = a.scales;
        op.w_scale = w.scales;
        return launch_gemm<e4m3_t>(s, a.e4m3(), K, w.e4m3(), K, M, N, K, EpiStore<f16_t>{o.p, N, nullptr, 0}, op);
    });
}

extern "C" int f5k_gemm_time(int32_t prec, int32_t M, int32_t N, int32_t K, int32_t tm, int32_t tn, int32_t iters,
                             float* avg_us, f5_stream stream) {
    if (!avg_us || M <= 0 || N <= 0 || K <= 0 || iters <= 0 || (N % 4)) return fail(F5_EINVAL, "f5k_gemm_time: bad arguments");
    if (prec == F5_PREC_F8) {   // tile_m: 0 auto or -(tile id 2, 8, 13); tile_n == 1: with the A operand's quantise launch
        if (tm > 0 || (tm < 0 && !gemm_tile_has_f8(-tm))) return fail(F5_EINVAL, "f5k_gemm_time: F5_PREC_F8 runs on tile ids 2, 8, 13 (tile_m = -id) or 0");
        return gemm_time_f8_impl(M, N, K, forced_cfg(tm, tn), tn == 1, iters, avg_us, (hipStream_t)stream);
    }
    const GemmOperands ops = prec == F5_PREC_F16X3 && tm <= 0 ? GemmOperands::WSplit : GemmOperands::Plain;   // (a v1 tile: plain f32)
    return F5K_BY_PREC(prec, gemm_time_impl, M, N, K, forced_cfg(tm, tn), ops, iters, avg_us, (hipStream_t)stream);
}

// packs fp32 [Bp,H,N,64] q/k/v into the engine layouts (q scaled, v transposed) -- test-side glue only
template <typename T>
__global__ void pack_qkv_test_kernel(const float* q, const float* k, const float* v, T* qo, T* ko, T* vto, long nrows, int N,
                                     int Npad, float qscale) {
    const long total = nrows * 64;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)(i % 64);
        const long row = i / 64;  // (b*H + h)*N + n
        const long bh = row / N;
        const int n = (int)(row % N);
        qo[i] = from_f32<T>(q[i] * qscale);
        ko[i] = from_f32<T>(k[i]);
        vto[(bh * 64 + d) * Npad + n] = from_f32<T>(v[i]);
    }
}
template <typename T> __global__ void to_f32_kernel(const T* in, float* out, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (float)in[i];
}

template <typename T> __global__ void fill_test_kernel(T* p, long n, float v) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = from_f32<T>(v);
}
template <typename TO> static int copy_f32(hipStream_t s, const void* src, float* dst, int64_t n) {
    if constexpr (!std::is_same_v<TO, float>) {
        if (dst && n > 0) {
            hipLaunchKernelGGL((to_f32_kernel<TO>), dim3(ew_blocks((long)n)), dim3(256), 0, s, static_cast<const TO*>(src), dst, (long)n);
            KCHK();
        }
    }
    return F5_OK;
}
// a host table of n ints on the device (null stays null)
static int upload_ints(Scratch<int>& d, const int32_t* host, int n) {
    if (!host) return F5_OK;
    HIPCHK(d.alloc((size_t)n));
    HIPCHK(hipMemcpy(d.p, host, (size_t)n * 4, hipMemcpyHostToDevice));
    return F5_OK;
}
// a RowPack table as the engine builds it: from 0, multiples of 4, every span within [min_span(b), round_up(N, 4)]
template <typename F> static bool row_start_ok(const int32_t* rs, int Bp, int N, F min_span) {
    if (rs[0] != 0) return false;
    for (int b = 0; b < Bp; ++b) {
        const int cnt = rs[b + 1] - rs[b];
        if (rs[b] % 4 || cnt < min_span(b) || cnt > round_up(N, 4)) return false;
    }
    return rs[Bp] % 4 == 0;
}

// One attention launch as attend (engine_impl.h) makes it.  T = the type of q / k / v^T; p.mode 1 (T = f16_t under
// F5_PREC_F16X3): the f16 kernel writes pre-split f32 rows (Of) instead of T rows.
template <typename T>
static int attn_body(const float* q, const float* k, const float* v, int Bp, int H, int N, const f5k_attn& p, bool split16, hipStream_t s) {
    const int Npad = round_up(N, 64);
    const long rows = (long)Bp * H * N;
    const size_t vt_elems = (size_t)Bp * H * 64 * Npad;
    Scratch<T> qd, kd, vd;
    Scratch<int> kl, ql, rs;
    HIPCHK(qd.alloc(rows * 64));
    HIPCHK(kd.alloc(rows * 64));
    HIPCHK(vd.alloc(vt_elems));
    CHK(upload_ints(kl, p.kv_lens_host, p.nlens));
    CHK(upload_ints(ql, p.q_lens_host, p.nlens));
    CHK(upload_ints(rs, p.row_start_host, Bp + 1));
    // (the engine's V^T columns [N, Npad) hold whatever the arena held: here a value of the caller's choice)
    hipLaunchKernelGGL((fill_test_kernel<T>), dim3(ew_blocks((long)vt_elems)), dim3(256), 0, s, vd.p, (long)vt_elems, p.vt_pad_fill);
    hipLaunchKernelGGL((pack_qkv_test_kernel<T>), dim3(ew_blocks(rows * 64)), dim3(256), 0, s, q, k, v, qd.p, kd.p, vd.p, rows,
                       N, Npad, attention_q_scale<T>());
    KCHK();
    if (p.mode == 1) {
        if constexpr (std::is_same_v<T, f16_t>)
            HIPCHK(launch_attention_v2<f16_t>(s, qd.p, kd.p, vd.p, nullptr, Bp, H, N, Npad, kl.p, p.nlens, ql.p, rs.p, static_cast<float*>(p.out)));
    } else {
        HIPCHK(launch_attention_any(s, qd.p, kd.p, vd.p, static_cast<T*>(p.out), Bp, H, N, Npad, kl.p, p.nlens, ql.p, rs.p, split16,
                                    p.o_planar != 0, p.hi_only, store_policy() & F5_WT_ATTN));
        CHK(copy_f32<T>(s, p.out, p.out_f32, p.n_out));
    }
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

static int attention_run(const char* who, int32_t prec, const float* q, const float* k, const float* v, int Bp, int H, int N,
                         const f5k_attn* p, hipStream_t s) {
    auto bad = [&](const char* what) { return fail(F5_EINVAL, "%s: %s", who, what); };
    if (!q || !k || !v || !p || !p->out || Bp <= 0 || H <= 0 || N <= 0) return bad("bad arguments");
    if (!prec_info(prec).plain()) return bad("precision must be f32, f16x3, bf16 or f16");
    const bool x3 = prec == F5_PREC_F16X3;
    if (p->mode != 0 && p->mode != 1) return bad("mode must be 0 (the precision's own kernel) or 1 (attn16)");
    if (p->mode == 1 && !x3) return bad("mode 1 (the f16 kernel writing pre-split f32 rows) exists under F5_PREC_F16X3 only");
    if (p->hi_only < 0 || p->hi_only > 3 || ((p->hi_only || p->o_planar) && (!x3 || p->mode != 0)))
        return bad("hi_only (0..3) and o_planar belong to the split kernel (F5_PREC_F16X3, mode 0)");
    if (!(p->vt_pad_fill == p->vt_pad_fill) || p->vt_pad_fill - p->vt_pad_fill != 0.f) return bad("vt_pad_fill must be finite");
    if ((p->kv_lens_host || p->q_lens_host) && (p->nlens < 1 || p->nlens > Bp)) return bad("nlens must be 1 .. Bp");
    if (p->row_start_host && !row_start_ok(p->row_start_host, Bp, N, [](int) { return 0; }))
        return bad("row_start must start at 0, in multiples of 4, at most round_up(N, 4) apart");
    const int64_t out_rows = p->row_start_host ? p->row_start_host[Bp] : (int64_t)Bp * N;
    if (p->n_out < out_rows * H * 64) return bad("out is smaller than the rows the launch may write");
    if (p->mode == 1) return attn_body<f16_t>(q, k, v, Bp, H, N, *p, false, s);
    return F5K_BY_PREC(prec, attn_body, q, k, v, Bp, H, N, *p, x3, s);
}

extern "C" int f5k_attention_ex(int32_t prec, const float* q, const float* k, const float* v, int32_t Bp, int32_t H, int32_t N,
                                const f5k_attn* p, f5_stream stream) {
    return attention_run("f5k_attention_ex", prec, q, k, v, Bp, H, N, p, (hipStream_t)stream);
}

extern "C" int f5k_attention(int32_t prec, const float* q, const float* k, const float* v, const int32_t* kv_lens_host,
                             float* out, int32_t Bp, int32_t H, int32_t N, f5_stream stream) {
    if (!out || Bp <= 0 || H <= 0 || N <= 0) return fail(F5_EINVAL, "f5k_attention: bad arguments");
    f5k_attn p{};
    p.kv_lens_host = kv_lens_host;
    p.nlens = Bp;
    p.n_out = (int64_t)Bp * N * H * 64;
    Scratch<uint16_t> o16;   // a 16-bit kernel's own output rows, copied to `out` as f32
    if (kernel_elem(prec) != PE_F32) {
        HIPCHK(o16.alloc((size_t)p.n_out));
        p.out = o16.p;
        p.out_f32 = out;
    } else {
        p.out = out;
    }
    return attention_run("f5k_attention", prec, q, k, v, Bp, H, N, &p, (hipStream_t)stream);
}

// One conv position embedding launch as embed_input (engine_impl.h) makes it.
template <typename T>
static int convpos_body(const float* x, const float* w, const float* bias, const float* res, float* y, int Bp, int N, int D,
                        const f5k_conv& p, bool split16, hipStream_t s) {
    const int cpg = D / 16, Kp = round_up(31 * cpg, GEMM_ROW_BYTES / (int)sizeof(T));
    Scratch<T> wp;
    Scratch<int> ld, rs;
    HIPCHK(wp.alloc((size_t)D * Kp));
    CHK(upload_ints(ld, p.lens_host, p.nlens));
    CHK(upload_ints(rs, p.row_start_host, Bp + 1));
    hipLaunchKernelGGL((conv_pack_kernel<T>), dim3(ew_blocks((long)D * Kp)), dim3(256), 0, s, w, wp.p, (long)D, cpg, 31, Kp);
    KCHK();
    const bool split = split16 && std::is_same_v<T, float> && convpos_can_split(D);
    if (split) HIPCHK(split_planes(s, wp.p, (size_t)D * Kp));
    HIPCHK(launch_convpos<T>(s, x, wp.p, Kp, bias, res, y, Bp, N, D, ld.p, p.nlens, rs.p, split));
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

static int convpos_run(const char* who, int32_t prec, const float* x, const float* w, const float* bias, const float* res, float* y,
                       int Bp, int N, int D, const f5k_conv* p, hipStream_t s) {
    auto bad = [&](const char* what) { return fail(F5_EINVAL, "%s: %s", who, what); };
    if (!x || !w || !bias || !y || !p || Bp <= 0 || N <= 0) return bad("bad arguments");
    if (D != 256 && D != 512 && D != 768 && D != 1024) return bad("D must be 256, 512, 768 or 1024");
    if (p->lens_host && (p->nlens < 1 || p->nlens > Bp)) return bad("nlens must be 1 .. Bp");
    auto len = [&](int b) { return p->lens_host ? std::min(N, std::max(0, (int)p->lens_host[b % p->nlens])) : N; };
    if (p->lens_host)
        for (int i = 0; i < p->nlens; ++i)
            if (p->lens_host[i] < 0) return bad("lens must not be negative");
    if (p->row_start_host && !row_start_ok(p->row_start_host, Bp, N, len))
        return bad("row_start must start at 0, in multiples of 4, each span from the row's length to round_up(N, 4)");
    if (p->rows < (p->row_start_host ? p->row_start_host[Bp] : (int64_t)Bp * N)) return bad("x / res / y have fewer rows than the launch touches");
    return F5K_BY_PREC(prec, convpos_body, x, w, bias, res, y, Bp, N, D, *p, prec == F5_PREC_F16X3, s);
}

extern "C" int f5k_convpos_ex(int32_t prec, const float* x, const float* w, const float* bias, const float* res, float* y, int32_t Bp,
                              int32_t N, int32_t D, const f5k_conv* p, f5_stream stream) {
    return convpos_run("f5k_convpos_ex", prec, x, w, bias, res, y, Bp, N, D, p, (hipStream_t)stream);
}

extern "C" int f5k_convpos(int32_t prec, const float* x, const float* w, const float* bias, const float* res,
                           const int32_t* lens_host, float* y, int32_t Bp, int32_t N, int32_t D, f5_stream stream) {
    f5k_conv p{};
    p.lens_host = lens_host;
    p.nlens = Bp;
    p.rows = (int64_t)Bp * N;
    return convpos_run("f5k_convpos", prec, x, w, bias, res, y, Bp, N, D, &p, (hipStream_t)stream);
}

extern "C" int f5k_layernorm_mod(const float* x, const float* scale, const float* shift, float* out, int32_t R, int32_t D,
                                 int32_t rows_per_batch, float eps, f5_stream stream) {
    if (!x || !out || R <= 0 || D <= 0 || D % 4 || D > 2048 || rows_per_batch <= 0) return fail(F5_EINVAL, "f5k_layernorm_mod: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    launch_adaln_norm(s, AdaLN{x, scale, shift, R, D, D, rows_per_batch, eps}, out, 0, 0);
    KCHK();
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

// ------------------------------------------------------------------------------------------- F5_PREC_F8 quantisers (quant8.h)
// The stand-alone row quantiser on caller-owned device buffers: x [R, ld] of f32 (F5_PREC_F32) or 16-bit values -> codes [R, ldc], scales [R].
extern "C" int f5k_quant_rows_e4m3(int32_t prec, const void* x, int64_t ld, int32_t R, int32_t K, uint8_t* codes, int64_t ldc, uint8_t* scales,
                                   int32_t m_limit, f5_stream stream) {
    if (!x || !codes || !scales || R <= 0 || K <= 0 || K % 4 || ld < K || ldc < K || ldc % 4 || m_limit < -1)
        return fail(F5_EINVAL, "f5k_quant_rows_e4m3: bad arguments (K %% 4 == 0, ld >= K, ldc >= K, ldc %% 4 == 0, m_limit -1 or >= 0)");
    if (!prec_info(prec).plain() || prec_info(prec).split16) return fail(F5_EINVAL, "f5k_quant_rows_e4m3: rows are f32, bf16 or f16");
    if (ld % 4 || ((size_t)x & (prec == F5_PREC_F32 ? 15 : 7)))
        return fail(F5_EINVAL, "f5k_quant_rows_e4m3: rows must start at whole groups of four elements (ld %% 4 == 0, aligned x)");
    hipStream_t s = (hipStream_t)stream;
    DevInt ml;
    CHK(ml.set(m_limit));
    const int* mlp = ml.get();
    const int Kc = round_up(K, 4);
    if (prec == F5_PREC_F32) launch_quant_rows_e4m3<float>(s, static_cast<const float*>(x), ld, R, K, codes, ldc, Kc, scales, mlp);
    else if (prec == F5_PREC_BF16) launch_quant_rows_e4m3<bf16_t>(s, static_cast<const bf16_t*>(x), ld, R, K, codes, ldc, Kc, scales, mlp);
    else launch_quant_rows_e4m3<f16_t>(s, static_cast<const f16_t*>(x), ld, R, K, codes, ldc, Kc, scales, mlp);
    KCHK();
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}
// The e4m3 output form of the AdaLN LayerNorm as adaln_norm launches it: codes [R, D] + scales [R].  batch_of_row_host (HOST int32[R], or
// NULL): the packed form -- row r takes the vectors of batch row batch_of_row[r] (layernorm_rows_q8_kernel; scale / shift rows are D apart).
extern "C" int f5k_layernorm_q8(const float* x, const float* scale, const float* shift, uint8_t* codes, uint8_t* scales, int32_t R, int32_t D,
                                int32_t rows_per_batch, float eps, int32_t m_limit, const int32_t* batch_of_row_host, f5_stream stream) {
    if (!x || !codes || !scales || R <= 0 || D <= 0 || D % 4 || D > 2048 || rows_per_batch <= 0 || m_limit < -1)
        return fail(F5_EINVAL, "f5k_layernorm_q8: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    DevInt ml;
    CHK(ml.set(m_limit));
    Scratch<int2> rowmap;
    if (batch_of_row_host) {
        std::vector<int2> h((size_t)R);
        for (int r = 0; r < R; ++r) {
            if (batch_of_row_host[r] < 0) return fail(F5_EINVAL, "f5k_layernorm_q8: negative batch row");
            h[r] = make_int2(batch_of_row_host[r], 0);
        }
        HIPCHK(rowmap.alloc((size_t)R));
        HIPCHK(hipMemcpy(rowmap.p, h.data(), (size_t)R * sizeof(int2), hipMemcpyHostToDevice));
    }
    launch_adaln_norm(s, AdaLN{x, scale, shift, R, D, D, rows_per_batch, eps, rowmap.p, Prefetch{}, ml.get()}, Rows8{codes, scales, D});
    KCHK();
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

template <typename TO>
static int layernorm_ex_impl(const float* x, const float* scale, const float* shift, void* out, float* out_f32, int R, int D,
                             int rows_per_batch, float eps, int m_limit, int planar, hipStream_t s) {
    DevInt ml;
    CHK(ml.set(m_limit));
    TO* o = static_cast<TO*>(out);
    launch_adaln_norm(s, AdaLN{x, scale, shift, R, D, D, rows_per_batch, eps, nullptr, Prefetch{}, ml.get()}, o, planar == 1,
                      wt_fits(store_policy() & F5_WT_LN, (size_t)R * D * sizeof(TO)));
    KCHK();
    if constexpr (std::is_same_v<TO, float>) {   // planar 2: the plain rows, then split_planar_kernel (what planar 1 must equal)
        if (planar == 2) {
            hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)R * D / 32)), dim3(256), 0, s, o, (long)R * D / 32);
            KCHK();
        }
    }
    if (!std::is_same_v<TO, float> && out_f32) {
        hipLaunchKernelGGL((to_f32_kernel<TO>), dim3(ew_blocks((long)R * D)), dim3(256), 0, s, o, out_f32, (long)R * D);
        KCHK();
    }
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

extern "C" int f5k_layernorm_mod_ex(int32_t prec, const float* x, const float* scale, const float* shift, void* out, float* out_f32,
                                    int32_t R, int32_t D, int32_t rows_per_batch, float eps, int32_t m_limit, int32_t planar,
                                    f5_stream stream) {
    if (!x || !out || R <= 0 || D <= 0 || D % 4 || D > 2048 || rows_per_batch <= 0 || m_limit < -1)
        return fail(F5_EINVAL, "f5k_layernorm_mod_ex: bad arguments");
    if (prec == F5_PREC_F8) {   // out: the e4m3 codes [R, D], then one scale byte per row
        if (out_f32 || planar) return fail(F5_EINVAL, "f5k_layernorm_mod_ex: F5_PREC_F8 writes uint8 codes [R, D] then R scale bytes into out (no out_f32, no planar)");
        return f5k_layernorm_q8(x, scale, shift, static_cast<uint8_t*>(out), static_cast<uint8_t*>(out) + (size_t)R * D, R, D, rows_per_batch, eps, m_limit,
                                nullptr, stream);
    }
    if (!prec_info(prec).plain()) return fail(F5_EINVAL, "f5k_layernorm_mod_ex: precision must be f32, f16x3, bf16, f16 or f8");
    if (planar < 0 || planar > 2 || (planar && (prec_info(prec).elem != PE_F32 || D % 32)) || (planar == 2 && m_limit >= 0))
        return fail(F5_EINVAL, "f5k_layernorm_mod_ex: planar needs an f32 output and D %% 32 == 0 (planar 2: every row)");
    return F5K_BY_PREC(prec, layernorm_ex_impl, x, scale, shift, out, out_f32, R, D, rows_per_batch, eps, m_limit, planar,
                       (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------- f5k_gemm_epi
// One GEMM through a production epilogue: EpiStore / EpiGateRes / EpiQKV constructed field for field as engine_impl.h does (EpiQKV: its
// qkv_project, own layout), the rotary table through rope_frag_kernel, packed rows through fill_rowmap_kernel, qk_norm through
// launch_qknorm_rope, the launcher qkv_project calls.
// (the staged operands g: rows of g.Kp, which is also the K of the launch)
template <typename T, typename Epi>
static int epi_gemm(hipStream_t s, const GemmStage<T>& g, int M, int N, const Epi& epi, int cfg, const int* ml, GemmOperands ops) {
    if (cfg == G3_256x256_PP && !(gemm_has_pingpong(sizeof(T), ops) && gemm3_epilogue_ok(epi)))
        return fail(F5_EINVAL, "f5k_gemm_epi: the ping-pong kernel (cfg 20) takes 16-bit or pre-split operands and a QKV split at 256 columns");
    GemmOpts o{ops, cfg, ml};
    o.a_scale = g.sa.p;   // (e4m3 operands: the scale bytes of their rows)
    o.w_scale = g.sw.p;
    HIPCHK(launch_gemm<T>(s, g.a.p, g.Kp, g.w.p, g.Kp, M, N, g.Kp, epi, o));
    return F5_OK;
}

template <typename T, typename TO>
static int epi_qkv(hipStream_t s, const GemmStage<T>& g, int M, int N, const float* bias, const f5k_epi& p, const int* ml, GemmOperands ops) {
    Scratch<float> frag;
    HIPCHK(frag.alloc((size_t)p.maxpos * 64));
    hipLaunchKernelGGL(rope_frag_kernel, dim3(ew_blocks((long)p.maxpos * 16)), dim3(256), 0, s, p.rope_cos, p.rope_sin, frag.p, (long)p.maxpos);
    KCHK();
    Scratch<int> rs;
    Scratch<int2> rowmap;
    if (p.row_start_host) {
        HIPCHK(rs.alloc((size_t)p.Bp + 1));
        HIPCHK(hipMemcpy(rs.p, p.row_start_host, ((size_t)p.Bp + 1) * 4, hipMemcpyHostToDevice));
        HIPCHK(rowmap.alloc((size_t)M));
        HIPCHK(hipMemsetAsync(rowmap.p, 0, (size_t)M * sizeof(int2), s));
        launch_fill_rowmap(s, rs.p, rowmap.p, p.Bp);
        KCHK();
        ml = rs.p + p.Bp;   // m_limit = row_start[Bp] (sample_body: RowPack::rows_dev)
    }
    const bool norm = p.kind == F5K_EPI_QKNORM;
    TO* q = static_cast<TO*>(p.out0);
    TO* k = static_cast<TO*>(p.out1);
    CHK(epi_gemm<T>(s, g, M, N,
                    EpiQKV<TO>{q, k, static_cast<TO*>(p.out2), bias, frag.p, p.Nseq, p.Npad, p.H, norm ? 0 : p.pe_heads,
                               norm ? 1.0f : p.q_scale, rowmap.p},
                    p.cfg, ml, ops));
    if (norm)   // (own layout: the stream is the whole sequence)
        HIPCHK(launch_qknorm_rope<TO>(s, q, k, p.gq, p.gk, p.rope_cos, p.rope_sin, p.Bp, p.H, p.Nseq, p.Nseq, 0, p.pe_heads, p.q_scale, 1e-6f));
    CHK(copy_f32<TO>(s, p.out0, p.out0_f32, p.n0));
    CHK(copy_f32<TO>(s, p.out1, p.out1_f32, p.n1));
    CHK(copy_f32<TO>(s, p.out2, p.out2_f32, p.n2));
    HIPCHK(hipStreamSynchronize(s));   // (the rotary table and the row map are freed on return)
    return F5_OK;
}

// T = e4m3_t (F5_PREC_F8): the e4m3 kernel on operands quantised per the contract (GemmStage); 16-bit outputs are f16, as in the engine.
template <typename T>
static int gemm_epi_impl(const float* A, const float* W, const float* bias, int M, int N, int K, const f5k_epi& p, GemmOperands ops,
                         hipStream_t s) {
    using T16 = typename Out16<T>::type;   // the type of a 16-bit STORE and of q / k / v^T (float operands: none, float)
    GemmStage<T> g;
    CHK(g.stage(s, A, K, W, K, M, N, K, round_up(K, GEMM_ROW_BYTES / (int)sizeof(T)), ops));
    DevInt ml;
    CHK(ml.set(p.m_limit));
    Scratch<int> lens;
    switch (p.kind) {
        case F5K_EPI_STORE:
            if (p.out16) {
                if constexpr (sizeof(T16) == 2) {
                    CHK(epi_gemm<T>(s, g, M, N, EpiStore<T16>{static_cast<T16*>(p.out0), N, bias, p.act, 0, wt_fits(store_policy() & F5_WT_STORE16, (size_t)M * N * sizeof(T16))},
                                    p.cfg, ml.get(), ops));
                    CHK(copy_f32<T16>(s, p.out0, p.out0_f32, p.n0));
                }
            } else {   // planar 2: the plain store, then split_planar_kernel over the whole output (what planar 1 must equal)
                CHK(epi_gemm<T>(s, g, M, N, EpiStore<float>{static_cast<float*>(p.out0), N, bias, p.act, p.planar == 1}, p.cfg, ml.get(), ops));
                if (p.planar == 2) {
                    hipLaunchKernelGGL(split_planar_kernel, dim3(ew_blocks((long)M * N / 32)), dim3(256), 0, s, static_cast<float*>(p.out0),
                                       (long)M * N / 32);
                    KCHK();
                }
            }
            break;
        case F5K_EPI_GATE_RES:
            if (p.lens_host) {
                HIPCHK(lens.alloc((size_t)p.nlens));
                HIPCHK(hipMemcpy(lens.p, p.lens_host, (size_t)p.nlens * 4, hipMemcpyHostToDevice));
            }
            CHK(epi_gemm<T>(s, g, M, N,
                            EpiGateRes{static_cast<float*>(p.out0), p.res, N, bias, p.gate, p.gate_stride, p.rows_per_batch, lens.p,
                                       wt_fits(store_policy() & F5_WT_GATE_RES, (size_t)M * N * 4)},
                            p.cfg, ml.get(), ops));
            break;
        default:   // QKV / QKNORM: the output type is the operand's (e4m3: f16), or f16 on f32 operands (the f16x3 attn16 path)
            if (p.out16) {
                if constexpr (std::is_same_v<T, float>) CHK((epi_qkv<T, f16_t>(s, g, M, N, bias, p, ml.get(), ops)));
            } else {
                CHK((epi_qkv<T, T16>(s, g, M, N, bias, p, ml.get(), ops)));
            }
            break;
    }
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}

extern "C" int f5k_gemm_epi(int32_t prec, const float* A, const float* W, const float* bias, int32_t M, int32_t N, int32_t K,
                            const f5k_epi* p, f5_stream stream) {
    if (!A || !W || !p || !p->out0 || M <= 0 || N <= 0 || K <= 0 || (N % 4)) return fail(F5_EINVAL, "f5k_gemm_epi: bad arguments (N %% 4 == 0)");
    const PrecInfo pi = prec_info(prec);
    if (!pi.plain() && !pi.f8) return fail(F5_EINVAL, "f5k_gemm_epi: precision must be f32, f16x3, bf16, f16 or f8");
    if (prec == F5_PREC_F8 && (K % 4 || (p->cfg != -1 && !gemm_tile_has_f8(p->cfg)) || p->planar))
        return fail(F5_EINVAL, "f5k_gemm_epi: F5_PREC_F8 needs K %% 4 == 0, cfg -1, 2, 8 or 13 and no planar output");
    if (p->cfg != -1 && (!gemm_tile(p->cfg) || v1_tile(p->cfg)))
        return fail(F5_EINVAL, "f5k_gemm_epi: cfg must be -1, 2, 8, 9, 10, 13 or 20");
    if (p->m_limit < -1 || p->m_limit > M) return fail(F5_EINVAL, "f5k_gemm_epi: m_limit must be -1 or 0..M");
    if (p->a_presplit && prec != F5_PREC_F16X3) return fail(F5_EINVAL, "f5k_gemm_epi: a_presplit needs F5_PREC_F16X3");
    const bool op16 = pi.elem != PE_F32;   // (f8: 16-bit outputs are f16)
    switch (p->kind) {
        case F5K_EPI_STORE:
            if (p->out16 && !op16) return fail(F5_EINVAL, "f5k_gemm_epi: a 16-bit STORE needs a 16-bit operand precision");
            if (p->planar < 0 || p->planar > 2 || (p->planar && (p->out16 || prec != F5_PREC_F16X3 || N % 32)) || (p->planar == 2 && p->m_limit >= 0))
                return fail(F5_EINVAL, "f5k_gemm_epi: planar needs an f32 output under f16x3 and N %% 32 == 0 (planar 2: every row)");
            if (p->act != F5_ACT_NONE && p->act != F5_ACT_GELU_TANH) return fail(F5_EINVAL, "f5k_gemm_epi: act must be none or GELU-tanh");
            break;
        case F5K_EPI_GATE_RES:
            if (p->out16 || p->rows_per_batch <= 0 || !p->res) return fail(F5_EINVAL, "f5k_gemm_epi: GATE_RES needs res and rows_per_batch > 0");
            if (p->lens_host && p->nlens < (M - 1) / p->rows_per_batch + 1) return fail(F5_EINVAL, "f5k_gemm_epi: lens shorter than the batch rows");
            break;
        case F5K_EPI_QKV:
        case F5K_EPI_QKNORM: {
            const bool norm = p->kind == F5K_EPI_QKNORM;
            if (!p->out1 || !p->out2 || !bias || !p->rope_cos || !p->rope_sin || p->H <= 0 || N != 3 * p->H * 64 || p->Nseq <= 0 ||
                p->Npad < p->Nseq || p->Npad % 8 || p->pe_heads < 0 || p->pe_heads > p->H || p->maxpos < p->Nseq || p->Bp <= 0)
                return fail(F5_EINVAL, "f5k_gemm_epi: bad QKV arguments");
            if (p->out16 && op16) return fail(F5_EINVAL, "f5k_gemm_epi: out16 QKV is the f16 output of f32 / f16x3 operands");
            if (norm && (p->out16 || !p->gq || !p->gk || p->row_start_host)) return fail(F5_EINVAL, "f5k_gemm_epi: bad QKNORM arguments");
            if (p->row_start_host) {
                if (p->m_limit != -1 || p->row_start_host[0] != 0 || p->row_start_host[p->Bp] > M)
                    return fail(F5_EINVAL, "f5k_gemm_epi: row_start must start at 0, end <= M and replaces m_limit");
                if (!row_start_ok(p->row_start_host, p->Bp, p->Nseq, [](int) { return 0; }))
                    return fail(F5_EINVAL, "f5k_gemm_epi: row_start entries must be multiples of 4, at most round_up(Nseq, 4) apart");
            } else if (M != p->Bp * p->Nseq) {
                return fail(F5_EINVAL, "f5k_gemm_epi: M must be Bp * Nseq without row_start");
            }
            break;
        }
        default: return fail(F5_EINVAL, "f5k_gemm_epi: unknown epilogue kind");
    }
    if (pi.f8) return gemm_epi_impl<e4m3_t>(A, W, bias, M, N, K, *p, GemmOperands::Plain, (hipStream_t)stream);
    const GemmOperands ops = prec != F5_PREC_F16X3 ? GemmOperands::Plain : p->a_presplit ? GemmOperands::AWSplit : GemmOperands::WSplit;
    return F5K_BY_PREC(prec, gemm_epi_impl, A, W, bias, M, N, K, *p, ops, (hipStream_t)stream);
}

// -------------------------------------------------------------------------------------------- step glue
// The glue kernels of sample() through the launch helpers of elementwise.h, the ones engine_impl.h calls: device buffers in, device
// buffers out, nothing staged.  Only the arguments' shape rules are checked here; the buffers' sizes are the caller's.
static int glue_done(hipStream_t s) {
    KCHK();
    HIPCHK(hipStreamSynchronize(s));
    return F5_OK;
}
static bool glue_prec_ok(int32_t prec) { return prec_info(prec).plain(); }

template <typename T>
static int pack_input_impl(const float* x, const float* cond, const float* tc, const float* tu, void* out, int ldo, int B, int Bp, int N, int mel,
                           int Dt, int drop, const int2* rowmap, const int* row_limit, const int* lens, hipStream_t s) {
    launch_pack_input<T>(s, x, cond, tc, tu, static_cast<T*>(out), ldo, B, Bp, N, mel, Dt, drop, rowmap, row_limit, lens);
    return glue_done(s);
}
extern "C" int f5k_pack_input(int32_t prec, const float* x, const float* cond, const float* text_c, const float* text_u, void* out, int32_t ldo,
                              int32_t B, int32_t Bp, int32_t N, int32_t mel, int32_t Dt, int32_t drop_cond_first, const void* rowmap,
                              const int32_t* row_limit, const int32_t* lens, f5_stream stream) {
    if (!x || !cond || !text_c || !text_u || !out || B <= 0 || (Bp != B && Bp != 2 * B) || N <= 0 || mel <= 0 || Dt <= 0 || mel % 4 || Dt % 4 ||
        ldo < 2 * mel + Dt || ldo % 4)
        return fail(F5_EINVAL, "f5k_pack_input: bad arguments (Bp = B or 2 B; mel, Dt, ldo %% 4 == 0; ldo >= 2 mel + Dt)");
    if (!glue_prec_ok(prec)) return fail(F5_EINVAL, "f5k_pack_input: precision must be f32, f16x3, bf16 or f16");
    if ((rowmap != nullptr) != (row_limit != nullptr) || (rowmap != nullptr) != (lens != nullptr))
        return fail(F5_EINVAL, "f5k_pack_input: rowmap, row_limit and lens come together (RowPack) or not at all");
    return F5K_BY_PREC(prec, pack_input_impl, x, cond, text_c, text_u, out, ldo, B, Bp, N, mel, Dt, drop_cond_first,
                       static_cast<const int2*>(rowmap), row_limit, lens, (hipStream_t)stream);
}
extern "C" int f5k_fill_rowmap(const int32_t* row_start, void* rowmap, int32_t Bp, f5_stream stream) {
    if (!row_start || !rowmap || Bp <= 0) return fail(F5_EINVAL, "f5k_fill_rowmap: bad arguments");
    launch_fill_rowmap((hipStream_t)stream, row_start, static_cast<int2*>(rowmap), Bp);
    return glue_done((hipStream_t)stream);
}
static int ode_args(const char* who, const void* y, const void* pred, int B, int N, int mel, const void* row_start, const void* lens,
                    const void* tgrid, int step, const void* out, bool need_out) {
    if (!y || !pred || !tgrid || (need_out && !out) || B <= 0 || N <= 0 || mel <= 0 || mel % 4 || step < 0 || (row_start != nullptr) != (lens != nullptr))
        return fail(F5_EINVAL, "%s: bad arguments (mel %% 4 == 0; row_start and lens come together)", who);
    return F5_OK;
}
extern "C" int f5k_euler_cfg(float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start, const int32_t* lens,
                             const float* tgrid, int32_t step, float cfg, int32_t use_cfg, float* traj_slot, f5_stream stream) {
    CHK(ode_args("f5k_euler_cfg", y, pred, B, N, mel, row_start, lens, tgrid, step, traj_slot, false));
    launch_euler_cfg((hipStream_t)stream, y, pred, B, N, mel, row_start, lens, tgrid, step, cfg, use_cfg ? 1 : 0, traj_slot);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_midpoint_half_cfg(const float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start,
                                     const int32_t* lens, const float* tgrid, int32_t step, float cfg, int32_t use_cfg, float* y_mid,
                                     f5_stream stream) {
    CHK(ode_args("f5k_midpoint_half_cfg", y, pred, B, N, mel, row_start, lens, tgrid, step, y_mid, true));
    launch_midpoint_half_cfg((hipStream_t)stream, y, pred, B, N, mel, row_start, lens, tgrid, step, cfg, use_cfg ? 1 : 0, y_mid);
    return glue_done((hipStream_t)stream);
}
static int items_args(const char* who, const void* y, const void* pred, int B, int N, int mel, const void* t_items, const void* cfg_items,
                      const void* steps_items, int steps_max, int step, const void* out, bool need_out) {
    if (!y || !pred || !t_items || !cfg_items || !steps_items || (need_out && !out) || B <= 0 || N <= 0 || mel <= 0 || mel % 4 || steps_max <= 0 ||
        step < 0 || step >= steps_max)
        return fail(F5_EINVAL, "%s: bad arguments (mel %% 4 == 0, 0 <= step < steps_max)", who);
    return F5_OK;
}
extern "C" int f5k_euler_cfg_items(float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const float* t_items, const float* cfg_items,
                                   const int32_t* steps_items, int32_t steps_max, int32_t step, int32_t use_cfg, float* traj_slot,
                                   f5_stream stream) {
    CHK(items_args("f5k_euler_cfg_items", y, pred, B, N, mel, t_items, cfg_items, steps_items, steps_max, step, traj_slot, false));
    launch_euler_cfg_items((hipStream_t)stream, y, pred, B, N, mel, nullptr, nullptr, t_items, cfg_items, steps_items, steps_max, step,
                           use_cfg ? 1 : 0, traj_slot);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_midpoint_half_cfg_items(const float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const float* t_items,
                                           const float* cfg_items, const int32_t* steps_items, int32_t steps_max, int32_t step,
                                           int32_t use_cfg, float* y_mid, f5_stream stream) {
    CHK(items_args("f5k_midpoint_half_cfg_items", y, pred, B, N, mel, t_items, cfg_items, steps_items, steps_max, step, y_mid, true));
    launch_midpoint_half_cfg_items((hipStream_t)stream, y, pred, B, N, mel, nullptr, nullptr, t_items, cfg_items, steps_items, steps_max, step,
                                   use_cfg ? 1 : 0, y_mid);
    return glue_done((hipStream_t)stream);
}
// (the packed forms: row_start and lens are device tables the caller owns, as for f5k_euler_cfg -- the caller keeps them inside pred)
extern "C" int f5k_euler_cfg_items_packed(float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start,
                                          const int32_t* lens, const float* t_items, const float* cfg_items, const int32_t* steps_items,
                                          int32_t steps_max, int32_t step, int32_t use_cfg, float* traj_slot, f5_stream stream) {
    CHK(items_args("f5k_euler_cfg_items_packed", y, pred, B, N, mel, t_items, cfg_items, steps_items, steps_max, step, traj_slot, false));
    if (!row_start || !lens) return fail(F5_EINVAL, "f5k_euler_cfg_items_packed: bad arguments (row_start and lens are required)");
    launch_euler_cfg_items((hipStream_t)stream, y, pred, B, N, mel, row_start, lens, t_items, cfg_items, steps_items, steps_max, step,
                           use_cfg ? 1 : 0, traj_slot);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_midpoint_half_cfg_items_packed(const float* y, const float* pred, int32_t B, int32_t N, int32_t mel, const int32_t* row_start,
                                                  const int32_t* lens, const float* t_items, const float* cfg_items,
                                                  const int32_t* steps_items, int32_t steps_max, int32_t step, int32_t use_cfg, float* y_mid,
                                                  f5_stream stream) {
    CHK(items_args("f5k_midpoint_half_cfg_items_packed", y, pred, B, N, mel, t_items, cfg_items, steps_items, steps_max, step, y_mid, true));
    if (!row_start || !lens) return fail(F5_EINVAL, "f5k_midpoint_half_cfg_items_packed: bad arguments (row_start and lens are required)");
    launch_midpoint_half_cfg_items((hipStream_t)stream, y, pred, B, N, mel, row_start, lens, t_items, cfg_items, steps_items, steps_max, step,
                                   use_cfg ? 1 : 0, y_mid);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_mod_gather(const float* src, const int32_t* idx, float* dst, int32_t rows, int32_t nidx, int32_t width, f5_stream stream) {
    if (!src || !idx || !dst || rows <= 0 || nidx <= 0 || width <= 0 || width % 4)
        return fail(F5_EINVAL, "f5k_mod_gather: bad arguments (width %% 4 == 0)");
    launch_mod_gather((hipStream_t)stream, src, idx, dst, rows, nidx, width);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_span_stage(float* y, const float* prev_state, int32_t prev_B, int32_t prev_N, const float* y_new, const int32_t* rows,
                              const int32_t* rows_host, int32_t B, int32_t N, int32_t mel, f5_stream stream) {
    if (!y || !rows || !rows_host || B <= 0 || N <= 0 || mel <= 0 || mel % 4)
        return fail(F5_EINVAL, "f5k_span_stage: bad arguments (mel %% 4 == 0)");
    CHK(check_span_rows("f5k_span_stage", rows_host, B, prev_state, prev_B, prev_N, y_new));
    launch_span_stage((hipStream_t)stream, y, prev_state, y_new, rows, B, N, prev_N, mel, N);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_span_stage_pitched(float* y, int32_t pitch, const float* prev_state, int32_t prev_B, int32_t prev_N, const float* y_new,
                                      const int32_t* rows, const int32_t* rows_host, int32_t B, int32_t N, int32_t mel, f5_stream stream) {
    if (!y || !rows || !rows_host || B <= 0 || N <= 0 || mel <= 0 || mel % 4 || pitch < N)
        return fail(F5_EINVAL, "f5k_span_stage_pitched: bad arguments (mel %% 4 == 0, pitch >= N)");
    CHK(check_span_rows("f5k_span_stage_pitched", rows_host, B, prev_state, prev_B, prev_N, y_new));
    launch_span_stage((hipStream_t)stream, y, prev_state, y_new, rows, B, N, prev_N, mel, pitch);
    return glue_done((hipStream_t)stream);
}
// the glue of f5_flow_loss (flow.h); lens null: a span may reach N
extern "C" int f5k_flow_mix(const float* x0, const float* x1, const float* t, const int32_t* span, const int32_t* span_host, float* phi,
                            float* cond, int32_t B, int32_t N, int32_t mel, f5_stream stream) {
    if (!x0 || !x1 || !t || !span || !phi || B <= 0 || N <= 0 || mel <= 0 || mel % 4)
        return fail(F5_EINVAL, "f5k_flow_mix: bad arguments (mel %% 4 == 0)");
    CHK(check_flow_spans("f5k_flow_mix", span_host, nullptr, B, N));
    launch_flow_mix((hipStream_t)stream, x0, x1, t, reinterpret_cast<const int2*>(span), phi, cond, B, N, mel);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_flow_loss_reduce(const float* pred, const float* x0, const float* x1, const int32_t* span, const int32_t* span_host,
                                    double* part, double* sq_sum, int32_t* count, float* frame_err, int32_t B, int32_t N, int32_t mel,
                                    f5_stream stream) {
    if (!pred || !x0 || !x1 || !span || !part || !sq_sum || !count || B <= 0 || B > 65535 || N <= 0 || mel <= 0 || mel % 4)
        return fail(F5_EINVAL, "f5k_flow_loss_reduce: bad arguments (mel %% 4 == 0, B <= 65535)");
    CHK(check_flow_spans("f5k_flow_loss_reduce", span_host, nullptr, B, N));
    launch_flow_loss((hipStream_t)stream, pred, x0, x1, reinterpret_cast<const int2*>(span), part, sq_sum, count, frame_err, B, N, mel);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_select_rows(const float* a, const float* b, const uint8_t* rowmask, float* out, int64_t rows, int32_t C, f5_stream stream) {
    if (!a || !rowmask || !out || rows <= 0 || C <= 0 || C % 4) return fail(F5_EINVAL, "f5k_select_rows: bad arguments (C %% 4 == 0)");
    launch_select_rows((hipStream_t)stream, a, b, rowmask, out, (long)rows, C);
    return glue_done((hipStream_t)stream);
}
extern "C" int f5k_time_sinus(const float* t, const float* freq, float* feat, int32_t S, f5_stream stream) {
    if (!t || !freq || !feat || S <= 0) return fail(F5_EINVAL, "f5k_time_sinus: bad arguments");
    launch_time_sinus((hipStream_t)stream, t, freq, feat, S);
    return glue_done((hipStream_t)stream);
}
template <typename TO> static int xrmsnorm_impl(const float* x, void* out, int R, int D, const float* g, int planar, hipStream_t s) {
    launch_xrmsnorm<TO>(s, x, static_cast<TO*>(out), R, D, g, planar, store_policy() & F5_WT_LN);
    return glue_done(s);
}
// planar: pre-split rows exist for f32 rows of whole 32-element blocks only
static bool planar_ok(int32_t prec, int planar, int D) {
    return planar == 0 || (planar == 1 && kernel_elem(prec) == PE_F32 && D % 32 == 0);
}
extern "C" int f5k_xrmsnorm(int32_t prec, const float* x, void* out, int32_t R, int32_t D, const float* g, int32_t planar, f5_stream stream) {
    if (!x || !out || !g || R <= 0 || D <= 0 || D % 4 || D > 2048 || !glue_prec_ok(prec) || !planar_ok(prec, planar, D))
        return fail(F5_EINVAL, "f5k_xrmsnorm: bad arguments (D %% 4 == 0, D <= 2048; planar: an f32 output and D %% 32 == 0)");
    return F5K_BY_PREC(prec, xrmsnorm_impl, x, out, R, D, g, planar, (hipStream_t)stream);
}
extern "C" int f5k_unett_assemble(const float* h, const float* temb, int32_t temb_stride, float* x, int32_t Bp, int32_t N, int32_t D,
                                  f5_stream stream) {
    if (!h || !temb || !x || Bp <= 0 || N <= 0 || D <= 0 || D % 4 || (temb_stride != 0 && temb_stride != D))
        return fail(F5_EINVAL, "f5k_unett_assemble: bad arguments (D %% 4 == 0, temb_stride 0 or D)");
    launch_unett_assemble((hipStream_t)stream, h, temb, temb_stride, x, Bp, N, D);
    return glue_done((hipStream_t)stream);
}
template <typename T> static int cat2_impl(const float* x, const float* skip, void* out, int rows, int D, int planar, hipStream_t s) {
    launch_cat2<T>(s, x, skip, static_cast<T*>(out), rows, D, planar);
    return glue_done(s);
}
extern "C" int f5k_cat2(int32_t prec, const float* x, const float* skip, void* out, int32_t rows, int32_t D, int32_t planar, f5_stream stream) {
    if (!x || !skip || !out || rows <= 0 || D <= 0 || D % 4 || !glue_prec_ok(prec) || !planar_ok(prec, planar, D))
        return fail(F5_EINVAL, "f5k_cat2: bad arguments (D %% 4 == 0; planar: an f32 output and D %% 32 == 0)");
    return F5K_BY_PREC(prec, cat2_impl, x, skip, out, rows, D, planar, (hipStream_t)stream);
}
extern "C" int f5k_strip_first_token(const float* in, float* out, int32_t Bp, int32_t N, int32_t C, f5_stream stream) {
    if (!in || !out || Bp <= 0 || N <= 0 || C <= 0 || C % 4) return fail(F5_EINVAL, "f5k_strip_first_token: bad arguments (C %% 4 == 0)");
    launch_strip_first_token((hipStream_t)stream, in, out, Bp, N, C);
    return glue_done((hipStream_t)stream);
}
