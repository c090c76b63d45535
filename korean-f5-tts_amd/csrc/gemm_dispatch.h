// launch_gemm(): C[M,N] = A[M,K] W[N,K]^T + epilogue.  It plans (plan_gemm: a pure host function of the problem's description) and
// then executes the plan (launch_gemm_tile: the one place that maps a tile id to a kernel instantiation).
//   ring (gemm2.h, LDS-DMA ring) whenever K is a whole number of 128-byte K-tiles (the engine pads its operands so that this
//   always holds on the hot path); ping-pong (gemm3.h, 256x256) for many-row problems that fill the chip with such tiles (the
//   utterance batches of C3 / C4); v1 (gemm.h, register-staged, any K % 16 bytes == 0) otherwise.
// Tile choice (measured on MI355X at M = 2048, tools/gemm2_sweep.py): the B=1 shapes are latency / L2-bandwidth
// bound, so the tile is the largest one that still yields >= ~1 workgroup per CU.
#pragma once
#include "gemm3.h"

namespace f5 {

enum GemmCfg { G2_128x128_8W = 2, G2_128x64_8W = 9, G2_64x64_4W = 8, G2_128x192_8W = 10, G2_256x128_8W = 13, G3_256x256_PP = 20,
               G1_128x128 = 128128, G1_128x64 = 128064, G1_64x64 = 64064 };
enum GemmFamily { GEMM_V1 = 1, GEMM_RING = 2, GEMM_PINGPONG = 3 };   // gemm.h, gemm2.h, gemm3.h

// THE tile table: every product tile, its kernel's template arguments, its family and its cost.  The cost search, the executor and
// "is this a product tile id" all read it; nothing else lists tiles (kapi_diag.hip adds diagnostic-only shapes under other ids).
// us: the time of one round of workgroups over the 256 CUs (K = 1024, measured with tools/gemm2_sweep.py on a full chip): the
// per-K-step time grows much more slowly than the tile area, so the largest tile that does not add a round wins; e.g. the QKV
// projection 2048 x 3072: 128x128 = 384 tiles = 2 rounds (25 us), 128x192 = 256 tiles = 1 round (20 us).  Listed largest first:
// ties keep the larger tile.  (The v1 tiles have no cost: pick_tile_v1 chooses among them.)
// (256x128: 865 TFLOP/s at M = 16384, N = 2048 against 722 for 128x128: the many-utterance batches C3 / C4)
// (256x256 ping-pong, gemm3.h: 16384 x {1024, 2048, 3072} x 1024 in 39 / 74 / 110 us = 37 us per round of 256 tiles against
//  42 us for two rounds of 256x128 tiles; 1.22 PFLOP/s in the K loop against 1.02)
// (Tried for the many-row block GEMMs and dropped, tools/block_gemm_time.py: 128x128 tiles with a 2-stage ring = 64 KB of LDS, two
//  workgroups per CU so that one's epilogue runs under the other's K loop -- 8 waves: 939 us per block of 32,768 rows against 794
//  for the tiles chosen below, QKV 420 against 284 us; 4 waves: 1,086 us.)
struct GemmTile { int id, bm, bn, wm, wn, ns; float us; GemmFamily family; };
constexpr GemmTile kGemmTiles[] = {
    {G3_256x256_PP, 256, 256, 0, 0, 0, 37.0f, GEMM_PINGPONG}, {G2_256x128_8W, 256, 128, 4, 2, 3, 21.0f, GEMM_RING},
    {G2_128x192_8W, 128, 192, 2, 4, 3, 19.3f, GEMM_RING},     {G2_128x128_8W, 128, 128, 2, 4, 4, 14.5f, GEMM_RING},
    {G2_128x64_8W, 128, 64, 4, 2, 4, 7.3f, GEMM_RING},        {G2_64x64_4W, 64, 64, 2, 2, 3, 4.0f, GEMM_RING},
    {G1_128x128, 128, 128, 0, 0, 0, 0.f, GEMM_V1},            {G1_128x64, 128, 64, 0, 0, 0, 0.f, GEMM_V1},
    {G1_64x64, 64, 64, 0, 0, 0, 0.f, GEMM_V1}};
inline const GemmTile* gemm_tile(int id) {   // null: not a product tile id
    for (const GemmTile& t : kGemmTiles) if (t.id == id) return &t;
    return nullptr;
}
// which (element size, operand form) have a ping-pong kernel: 16-bit operands, or f32 rows of pre-split planes
constexpr bool gemm_has_pingpong(int elem_size, GemmOperands ops) {
    return (elem_size == 2 && ops == GemmOperands::Plain) || (elem_size == 4 && ops == GemmOperands::AWSplit);
}

// e4m3 operands (element size 1, gemm8.h): the ring tiles instantiated for them -- one many-row tile, one for a few hundred rows, one
// small tile for few rows and the remainder launch.  No v1 and no ping-pong kernel: K is a whole number of 128-code K-tiles or refused.
constexpr bool gemm_tile_has_f8(int id) { return id == G2_256x128_8W || id == G2_128x128_8W || id == G2_64x64_4W; }

struct GemmProblem {   // what plan_gemm decides on
    int elem_size, M, N, K;
    bool has_m_limit;       // a device row count comes with the launch
    int m_hint;             // the row count the caller expects behind it (0: none) -- the tile is chosen for it, the grid covers M
    GemmOperands ops;
    bool conv, pp_epilogue; // implicit conv (GemmConv::tpt > 0); the epilogue admits the ping-pong tile (gemm3_epilogue_ok)
    int force_cfg;          // -1 auto, -2 the v1 kernel at its own tile, else a tile id of kGemmTiles
    int env_cfg, env_n;     // F5_GEMM_CFG (-1: unset; diagnostic: one ring / ping-pong tile for every GEMM) / F5_GEMM_CFG_N (only for this N)
};
struct GemmLaunch { int family, tile, row0, rows; };   // tile: a GemmCfg id
struct GemmPlan { bool ok = true; int n = 0; GemmLaunch l[2] = {}; };   // !ok: hipErrorInvalidValue; n == 0: nothing to do

// cost = rounds of workgroups over the 256 CUs x the time of one round of that tile
inline int pick_cfg_v2(int M, int N, bool allow_pp, int env_cfg, int env_n) {
    if (env_cfg >= 0 && (env_cfg != G3_256x256_PP || allow_pp) && (env_n == 0 || env_n == N)) {
        const GemmTile* t = gemm_tile(env_cfg);
        return t && t->family != GEMM_V1 ? env_cfg : G2_64x64_4W;   // (an id that names no such tile: the smallest one)
    }
    if (M <= 64) return G2_64x64_4W;  // skinny (time MLP, AdaLN stack over the NFE steps): weight-streaming, no row reuse to gain
    int best = G2_64x64_4W;
    float best_cost = 3.0e38f;
    for (const GemmTile& c : kGemmTiles) {
        if (c.family == GEMM_V1 || (c.family == GEMM_PINGPONG && !allow_pp)) continue;
        const long tiles = (long)((M + c.bm - 1) / c.bm) * ((N + c.bn - 1) / c.bn);
        const float cost = (float)((tiles + 255) / 256) * c.us;
        if (cost < best_cost) { best_cost = cost; best = c.id; }  // ties keep the larger tile (listed first)
    }
    return best;
}
inline int pick_tile_v1(int M, int N) {
    auto blocks = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    if (M > 64 && N > 64 && blocks(128, 128) >= 200) return G1_128x128;
    if (M > 64 && blocks(128, 64) >= 160) return G1_128x64;
    return G1_64x64;
}

// The plan for e4m3 operands: plain operands, no implicit conv, whole K-tiles; the cost search of pick_cfg_v2 over the f8 tiles (their
// times per round are taken as proportional to the 16-bit ones); the remainder split of the many-row tile as for the ping-pong kernel.
inline GemmPlan plan_gemm_f8(const GemmProblem& p) {
    GemmPlan r;
    const GemmPlan refused{false, 0, {}};
    if (p.ops != GemmOperands::Plain || p.conv || p.K <= 0 || p.K % GEMM_ROW_BYTES != 0 || p.force_cfg == -2) return refused;
    if (p.force_cfg >= 0 && !gemm_tile_has_f8(p.force_cfg)) return refused;
    auto pick = [&](int M) {
        if (p.env_cfg >= 0 && gemm_tile_has_f8(p.env_cfg) && (p.env_n == 0 || p.env_n == p.N)) return p.env_cfg;
        if (M <= 64) return (int)G2_64x64_4W;
        int best = G2_64x64_4W;
        float best_cost = 3.0e38f;
        for (const GemmTile& c : kGemmTiles) {
            if (!gemm_tile_has_f8(c.id)) continue;
            const long tiles = (long)((M + c.bm - 1) / c.bm) * ((p.N + c.bn - 1) / c.bn);
            const float cost = (float)((tiles + 255) / 256) * c.us;
            if (cost < best_cost) { best_cost = cost; best = c.id; }
        }
        return best;
    };
    r.n = 1;
    if (p.force_cfg == -1 && !p.has_m_limit) {
        const int rem = p.M % 256, main = p.M - rem;
        if (rem > 0 && rem <= 64 && main >= 4096 && pick(main) == G2_256x128_8W) {
            r.n = 2;
            r.l[0] = {GEMM_RING, G2_256x128_8W, 0, main};
            r.l[1] = {GEMM_RING, G2_64x64_4W, main, rem};
            return r;
        }
    }
    r.l[0] = {GEMM_RING, p.force_cfg >= 0 ? p.force_cfg : pick(p.m_hint > 0 ? p.m_hint : p.M), 0, p.M};
    return r;
}

// Every dispatch decision (no HIP call, no environment): launch_gemm() executes what this returns, f5k_gemm_plan() shows it to the
// tests without a GPU.
inline GemmPlan plan_gemm(const GemmProblem& p) {
    GemmPlan r;
    const GemmPlan refused{false, 0, {}};
    if (p.M <= 0 || p.N <= 0) return r;
    if (p.elem_size == 1) return plan_gemm_f8(p);
    const bool plain = p.ops == GemmOperands::Plain;
    const GemmTile* forced = p.force_cfg >= 0 ? gemm_tile(p.force_cfg) : nullptr;
    const bool forced_v1 = forced && forced->family == GEMM_V1;
    // v1: asked for, or K is no whole number of 128-byte K-tiles (a forced ring / ping-pong tile does not apply then)
    const bool v1 = p.force_cfg == -2 || forced_v1 || p.K % (GEMM_ROW_BYTES / p.elem_size) != 0;
    if (!plain && p.elem_size != 4) return refused;                 // the split forms are f32 rows
    if ((!plain || p.conv || p.has_m_limit) && v1) return refused;  // split operands, implicit conv, m_limit: ring / ping-pong only
    r.n = 1;
    if (v1) {
        r.l[0] = {GEMM_V1, forced_v1 ? forced->id : pick_tile_v1(p.M, p.N), 0, p.M};
        return r;
    }
    // A many-row problem whose row count is a few rows past a multiple of 256 (UNetT: 16 x 1025 = 16,400 rows) would pay
    // a whole extra round of 256-row tiles for the last 16 rows: the 256-row multiple goes to the ping-pong kernel and the
    // remainder to one row of 64x64 tiles (same K order per element: bit-identical to a single launch).
    // (Tried for the remainder launch and dropped: running it BESIDE the main launch on a second stream -- fork / join events, in the
    // captured graph a two-node parallel branch per GEMM -- C5 350.5 -> 356.0 ms: the cross-stream dependencies of 1,920 branches cost
    // more than the ~20 ms of remainder launches they hide.  Deeper LDS-DMA rings for its 64x64 tiles (6, 8 stages): 6.3 -> 6.5-6.8 us.)
    // (Round 2 sent the residual epilogue -- EpiGateRes reads and writes the f32 stream, 268 MB per launch at 32,768 rows -- to two
    // rounds of 256x128 tiles because the ping-pong kernel's fragment-order epilogue overlapped with nothing.  With the staged
    // row-major epilogue (gemm.h) the ping-pong tile wins there too: tools/block_gemm_time.py, 32,768 rows, out-proj / FF2.)
    const bool pp_ok = gemm_has_pingpong(p.elem_size, p.ops) && p.pp_epilogue && !p.conv;   // (no implicit-conv / row-offset mode there)
    if (p.force_cfg == -1 && !p.has_m_limit && pp_ok) {
        const int rem = p.M % 256, main = p.M - rem;
        const int cfg_main = (rem > 0 && rem <= 64 && main >= 4096) ? pick_cfg_v2(main, p.N, true, p.env_cfg, p.env_n) : -1;
        if (cfg_main == G3_256x256_PP || cfg_main == G2_256x128_8W) {
            r.n = 2;
            r.l[0] = {gemm_tile(cfg_main)->family, cfg_main, 0, main};
            r.l[1] = {GEMM_RING, G2_64x64_4W, main, rem};
            return r;
        }
    }
    int cfg = p.force_cfg;
    if (cfg >= 0) {
        if (!forced) cfg = G2_64x64_4W;                              // (an id that names no tile: the smallest one)
        else if (cfg == G3_256x256_PP && !pp_ok) return refused;     // a forced ping-pong tile where no such kernel exists
    } else {
        cfg = pick_cfg_v2(p.m_hint > 0 ? p.m_hint : p.M, p.N, pp_ok, p.env_cfg, p.env_n);
        // pre-split operands (F5_PREC_F16X3 block GEMMs): three MFMAs per fragment pair shift the balance towards the small tile
        // where both fit in two rounds (2048 x 1024 x {1024, 2048}: 64x64 16.2 / 28.7 us, 128x64 18.0 / 30.8 -- tools/probe/gemm_split_probe.hip)
        if (p.ops == GemmOperands::AWSplit && cfg == G2_128x64_8W && (long)((p.M + 63) / 64) * ((p.N + 63) / 64) <= 512) cfg = G2_64x64_4W;
    }
    r.l[0] = {gemm_tile(cfg)->family, cfg, 0, p.M};
    return r;
}

// One launch of a plan: walks kGemmTiles at compile time and instantiates, for this (T, operand form, Epi), only the kernels
// plan_gemm can return for it -- v1 for plain operands, ping-pong where gemm_has_pingpong says so.  (RING_ONLY: the tile sweeps of
// kapi_diag.hip, which reach the other two kernels under ids of their own.)
template <typename T, GemmOperands OPS, typename Epi, bool RING_ONLY = false, size_t I = 0>
inline hipError_t launch_gemm_tile(hipStream_t s, const T* A, int lda, const T* W, int ldw, int M, int N, int K, const Epi& epi, int tile,
                                   const int* ml, const GemmConv& cv) {
    if constexpr (I < sizeof(kGemmTiles) / sizeof(kGemmTiles[0])) {
        constexpr GemmTile t = kGemmTiles[I];
        if (t.id != tile) return launch_gemm_tile<T, OPS, Epi, RING_ONLY, I + 1>(s, A, lda, W, ldw, M, N, K, epi, tile, ml, cv);
        if constexpr (sizeof(T) == 1 && !(t.family == GEMM_RING && gemm_tile_has_f8(t.id))) return hipErrorInvalidValue;   // e4m3: its ring tiles only
        else if constexpr (t.family == GEMM_RING) return launch_gemm2<T, t.bm, t.bn, t.wm, t.wn, t.ns, Epi, OPS>(s, A, lda, W, ldw, M, N, K, epi, ml, cv);
        else if constexpr (RING_ONLY) return hipErrorInvalidValue;
        else if constexpr (t.family == GEMM_V1 && OPS == GemmOperands::Plain) return launch_gemm1<T, t.bm, t.bn, Epi>(s, A, lda, W, ldw, M, N, K, epi);
        else if constexpr (t.family == GEMM_PINGPONG && gemm_has_pingpong(sizeof(T), OPS)) return launch_gemm3<T, Epi, OPS>(s, A, lda, W, ldw, M, N, K, epi, ml);
    }
    return hipErrorInvalidValue;
}

// What a launch may say beyond the problem itself; every field has the everyday value as its default.
struct GemmOpts {
    GemmOperands ops = GemmOperands::Plain;
    int force_cfg = -1;              // -1 auto, -2 the v1 kernel, else a tile id (GemmCfg)
    const int* m_limit = nullptr;    // device int: rows actually present, <= M (ring / ping-pong only: the engine's operands always qualify)
    int m_hint = 0;                  // the row count the caller expects behind m_limit
    GemmConv conv = {};
    // e4m3 operands (T = e4m3_t, gemm8.h): one e8m0 scale byte per row of A and per row of W (w_scale 4-byte aligned)
    const unsigned char* a_scale = nullptr;
    const unsigned char* w_scale = nullptr;
};

template <typename T, typename Epi>
inline hipError_t launch_gemm(hipStream_t s, const T* A, int lda, const T* W, int ldw, int M, int N, int K, const Epi& epi,
                              const GemmOpts& o = GemmOpts{}) {
    static const int env_cfg = getenv("F5_GEMM_CFG") ? atoi(getenv("F5_GEMM_CFG")) : -1;
    static const int env_n = getenv("F5_GEMM_CFG_N") ? atoi(getenv("F5_GEMM_CFG_N")) : 0;
    const GemmPlan plan = plan_gemm({(int)sizeof(T), M, N, K, o.m_limit != nullptr, o.m_hint, o.ops, o.conv.tpt > 0, gemm3_epilogue_ok(epi),
                                     o.force_cfg, env_cfg, env_n});
    if (!plan.ok) return hipErrorInvalidValue;
    return with_static_act(epi, [&](const auto& e) {
        using E = std::decay_t<decltype(e)>;
        for (int i = 0; i < plan.n; ++i) {
            const GemmLaunch& l = plan.l[i];
            GemmConv c = o.conv;
            if (l.row0 > 0) c.m_base = l.row0;   // (the remainder launch: the epilogue addresses row m_base + m)
            hipError_t err = hipErrorInvalidValue;
            if constexpr (std::is_same_v<T, float>) {
                if (o.ops == GemmOperands::AWSplit) err = launch_gemm_tile<T, GemmOperands::AWSplit, E>(s, A + (size_t)l.row0 * lda, lda, W, ldw, l.rows, N, K, e, l.tile, o.m_limit, c);
                if (o.ops == GemmOperands::WSplit) err = launch_gemm_tile<T, GemmOperands::WSplit, E>(s, A + (size_t)l.row0 * lda, lda, W, ldw, l.rows, N, K, e, l.tile, o.m_limit, c);
            }
            if constexpr (sizeof(T) == 1) {   // the epilogue behind the operands' scales (row m of the epilogue = row m of a_scale)
                if (!o.a_scale || !o.w_scale) return hipErrorInvalidValue;
                err = launch_gemm_tile<T, GemmOperands::Plain, EpiScale8<E>>(s, A + (size_t)l.row0 * lda, lda, W, ldw, l.rows, N, K, EpiScale8<E>{e, o.a_scale, o.w_scale}, l.tile, o.m_limit, c);
            } else if (o.ops == GemmOperands::Plain) err = launch_gemm_tile<T, GemmOperands::Plain, E>(s, A + (size_t)l.row0 * lda, lda, W, ldw, l.rows, N, K, e, l.tile, o.m_limit, c);
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    });
}

}  // namespace f5
