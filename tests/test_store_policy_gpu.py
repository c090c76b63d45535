"""GPU: the store policy (F5_STORE_WT / f5x_set_store_policy, csrc/f5_common.h "store policy") changes HOW the block kernels store --
write-through, 16-bit outputs regrouped to 16 bytes per lane -- and nothing else: every case runs with mask 0 and with the full mask
into NaN-sentinel buffers between guard bands and demands the two raw buffers equal bit for bit.  That is equal output bits, intact
guard bands, and every in-buffer byte the plain kernel leaves alone (rows past M / m_limit / a span, V^T columns [Nseq, Npad), dropped
alignment rows) still holding its sentinel.  Each case also asserts that the plain run wrote something and left its own untouched
regions alone, so that "equal" cannot mean "both wrong in the same way" about the sentinels.

Shapes: the smallest at which a regrouped store can go wrong -- a row count that is no tile multiple (200), a last 16-row sub-tile that
is partly valid (37, 200), N below a tile (64), N = 192 (three 16-column sub-tiles per wave of the 128x192 tile: a pair and a single),
two batch rows inside one tile, packed rows whose alignment rows are dropped.  End to end: sample() of the small golden
configurations, F5_STORE_WT=0 against the default, graphs on and off, two calls each.

The QKV epilogue ships without a write-through form (it lost at C2, csrc/gemm.h EpiQKV): its cases hold the two policies to the same
bits all the same, so that a later form of it starts out checked."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded, k_attention_ex, k_gemm_epi, k_layernorm_mod_ex, k_xrmsnorm  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402

STORE, GATE_RES, QKV = _lib.F5K_EPI_STORE, _lib.F5K_EPI_GATE_RES, _lib.F5K_EPI_QKV
TDTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
FULL = 63
# the ring tiles the C2 dispatch picks (128x128, 128x64, 128x192), the 64x64 tile, and the dispatcher's own choice
CFGS = [2, 9, 10, 8, -1]
SHAPES = [(M, N) for M in (128, 200, 37) for N in (64, 192, 1024)]
K = 256


def set_policy(mask):
    fn = _lib.load().f5x_set_store_policy
    fn.restype, fn.argtypes = C.c_int32, [C.c_int32]
    assert fn(mask) == 0


@pytest.fixture(autouse=True)
def plain_after():
    yield
    set_policy(0)


def both(run):
    """run() -> list of Guarded, once per policy; the raw buffers (guard bands included) must agree bit for bit."""
    set_policy(0)
    plain = run()
    set_policy(FULL)
    wt = run()
    set_policy(0)
    for i, (a, b) in enumerate(zip(plain, wt)):
        assert a.guards_intact() and b.guards_intact(), i
        d = a.raw != b.raw
        assert not d.any(), (i, int(d.sum()), "first differing element", int(d.nonzero()[0]) - 64)
    return plain


def operands(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, K, generator=g).to(DEV), (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV))


# ====================================================================================================== GEMM epilogues
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("prec,sixteen", [("bf16", True), ("f16", True), ("f16", False), ("f32", False)])
def test_store_epilogue(prec, sixteen, cfg):
    for M, N in SHAPES:
        A, W, b = operands(M, N, seed=M + N)
        for m_limit in (-1, M - 5):
            def run():
                out = Guarded((M, N), TDTYPE[prec] if sixteen else torch.float32)
                k_gemm_epi(prec, A, W, b, STORE, [out], cfg=cfg, out16=sixteen, act=1 if sixteen else 0, m_limit=m_limit)
                return [out]
            out, = both(run)
            rows = M if m_limit < 0 else m_limit
            assert (out.bits[:rows] != out.sent).all() and (out.bits[rows:] == out.sent).all(), (M, N, m_limit)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("prec", ["f16", "bf16", "f32"])
def test_gate_res_epilogue_in_place(prec, cfg):
    rpb = 100   # two batch rows inside one 128-row tile
    for M, N in SHAPES:
        A, W, b = operands(M, N, seed=3 * M + N)
        nb = (M - 1) // rpb + 1
        g = torch.Generator().manual_seed(M * N)
        res, gate = torch.randn(M, N, generator=g).to(DEV), torch.randn(nb, N, generator=g).to(DEV)
        lens = [min(rpb, M) - 9, 61][:nb]

        def run():
            x = Guarded.like(res)
            k_gemm_epi(prec, A, W, b, GATE_RES, [x], cfg=cfg, res=x, gate=gate, gate_stride=N, rows_per_batch=rpb, lens=lens)
            return [x]
        x, = both(run)
        for bi, n in enumerate(lens):   # masked rows keep the residual bit for bit, the others moved
            lo, hi = bi * rpb, min((bi + 1) * rpb, M)
            assert torch.equal(x.value[lo + n:hi], res[lo + n:hi]), (M, N, bi)
            assert not torch.equal(x.value[lo:lo + n], res[lo:lo + n]), (M, N, bi)


def rotary(maxpos):
    f = torch.arange(maxpos)[:, None] * (1.0 / 10000 ** (torch.arange(32)[None, :] / 32.0))
    return f.cos().contiguous().to(DEV), f.sin().contiguous().to(DEV)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("pe", [1, 3])
def test_qkv_epilogue(prec, cfg, pe):
    Bp, H, Nseq, Npad = 2, 3, 100, 128
    A, W, b = operands(Bp * Nseq, 3 * H * 64, seed=17 + pe)
    cs, sn = rotary(Nseq + 3)
    lens = [100, 37]
    rs = [0, 100, 140]   # packed rows: utterances start at multiples of 4; rows 137 .. 139 are alignment rows (positions past the utterance)
    for row_start in (None, rs):
        def run():
            outs = [Guarded((Bp, H, Nseq, 64), TDTYPE[prec]), Guarded((Bp, H, Nseq, 64), TDTYPE[prec]), Guarded((Bp, H, 64, Npad), TDTYPE[prec])]
            k_gemm_epi(prec, A, W, b, QKV, outs, cfg=cfg, H=H, Nseq=Nseq, Npad=Npad, pe_heads=pe, q_scale=0.125, rope_cos=cs, rope_sin=sn,
                       row_start=row_start, Bp=Bp)
            return outs
        q, k, vt = both(run)
        assert (vt.bits[..., Nseq:] == vt.sent).all(), "V^T columns [Nseq, Npad) were written"
        for bi in range(Bp):
            n = Nseq if row_start is None else min(rs[bi + 1] - rs[bi], Nseq)
            for t in (q, k):
                assert (t.bits[bi, :, :n] != t.sent).all() and (t.bits[bi, :, n:] == t.sent).all(), (bi, row_start)
            assert (vt.bits[bi, :, :, :n] != vt.sent).all() and (vt.bits[bi, :, :, n:] == vt.sent).all(), (bi, row_start)


# ================================================================================================ LayerNorm / RMSNorm
@pytest.mark.parametrize("prec,planar", [("f16", 0), ("bf16", 0), ("f32", 0), ("f16x3", 1)])
@pytest.mark.parametrize("D", [256, 1024])
def test_layernorm(prec, planar, D):
    for R in (1, 5, 130):
        g = torch.Generator().manual_seed(R + D)
        x = (torch.randn(R, D, generator=g) * 3 + 1).to(DEV)
        rpb = 72
        nb = (R - 1) // rpb + 1
        sc, sh = torch.randn(nb, D, generator=g).to(DEV), torch.randn(nb, D, generator=g).to(DEV)
        for m_limit in (-1, R - 1):
            def run():
                out = Guarded((R, D), TDTYPE.get(prec, torch.float32))
                k_layernorm_mod_ex(prec, x, sc, sh, out, rpb, m_limit=m_limit, planar=planar)
                return [out]
            out, = both(run)
            rows = R if m_limit < 0 else m_limit
            assert (out.bits[:rows] != out.sent).all() and (out.bits[rows:] == out.sent).all(), (R, D, m_limit)


@pytest.mark.parametrize("prec,planar", [("f16", 0), ("bf16", 0), ("f32", 0), ("f16x3", 1)])
@pytest.mark.parametrize("D", [256, 1024])
def test_rmsnorm(prec, planar, D):
    for R in (1, 5, 130):
        g = torch.Generator().manual_seed(2 * R + D)
        x, gv = torch.randn(R, D, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV)

        def run():
            return [k_xrmsnorm(prec, x, gv, Guarded((R, D), TDTYPE.get(prec, torch.float32)), planar=planar)]
        out, = both(run)
        assert (out.bits != out.sent).all(), (R, D)


# ========================================================================================================== attention
@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("N,lens", [(37, [37, 20]), (200, [200, 70])])
def test_attention_output(prec, N, lens):
    Bp, H = 2, 2
    g = torch.Generator().manual_seed(N)
    qkv = [torch.randn(Bp, H, N, 64, generator=g).to(DEV) for _ in range(3)]
    for t in qkv:   # rows past a batch row's length: zeros, as the arena rule allows
        for bi in range(Bp):
            t[bi, :, lens[bi]:] = 0
    rs = [0]
    for n in lens:
        rs.append(rs[-1] + (n + 3) // 4 * 4)
    forms = [dict(), dict(kv_lens=lens, q_lens=lens), dict(kv_lens=lens, q_lens=lens, row_start=rs)]
    for tables in forms:
        rows = (rs[Bp] + 8) if "row_start" in tables else Bp * N

        def run():
            return [k_attention_ex(prec, *qkv, Guarded((rows, H * 64), TDTYPE[prec]), **tables)]
        out, = both(run)
        if "row_start" in tables:   # rows >= min(N, span) of every batch row, and everything past row_start[Bp], untouched
            keep = torch.ones(rows, dtype=torch.bool, device=DEV)
            for bi in range(Bp):
                span = min(N, rs[bi + 1] - rs[bi])
                keep[rs[bi]:rs[bi] + span] = False
                assert (out.bits[rs[bi]:rs[bi] + lens[bi]] != out.sent).all(), (N, bi)
            assert (out.bits[keep] == out.sent).all(), N
        elif not tables:
            assert (out.bits != out.sent).all(), N
    # the pre-split f32 output rows (F5_PREC_F16X3) keep their plain stores: still the same bits
    def run_planar():
        return [k_attention_ex("f16x3", *qkv, Guarded((Bp * N, H * 64), torch.float32), o_planar=1)]
    both(run_planar)


# ========================================================================================================= end to end
def _sample(monkeypatch, name, prec, wt, graphs):
    """out, traj of two sample() calls on a fresh engine under F5_STORE_WT=wt (None: the default) and F5_HIP_GRAPH=graphs."""
    from test_sample_gpu import build_cfm, run_case   # the golden configurations as that file builds them
    if wt is None:
        monkeypatch.delenv("F5_STORE_WT", raising=False)
    else:
        monkeypatch.setenv("F5_STORE_WT", str(wt))
    monkeypatch.setenv("F5_HIP_GRAPH", "1" if graphs else "0")
    meta, a = load_golden(name)
    model = build_cfm(meta, synthetic_weights(meta), prec)
    res = []
    for _ in range(2):   # (the second call of a signature is the captured graph's first replay)
        out, traj = run_case(meta, a, model)
        torch.cuda.synchronize()
        res.append((out.clone(), traj.clone()))
    return res


@pytest.mark.parametrize("name,prec", [("sample_b1_nfe16", "f32"), ("sample_b1_nfe16", "f16p"), ("sample_b1_nfe16", "bf16"),
                                       ("sample_b3_attnmask", "f16p"), ("sample_unett_b2", "f16x3")])
def test_sample_is_bit_equal_under_every_policy(monkeypatch, name, prec):
    ref = _sample(monkeypatch, name, prec, 0, True)
    assert torch.equal(ref[0][0], ref[1][0]) and torch.equal(ref[0][1], ref[1][1]), "eager first call vs graph replay"
    for wt, graphs in ((None, True), (None, False), (0, False)):
        got = _sample(monkeypatch, name, prec, wt, graphs)
        for call in range(2):
            assert torch.equal(got[call][0], ref[0][0]), (name, prec, wt, graphs, call, "out")
            assert torch.equal(got[call][1], ref[0][1]), (name, prec, wt, graphs, call, "traj")
