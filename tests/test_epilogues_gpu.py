"""GPU: the backbone GEMM epilogues (csrc/gemm.h EpiStore / EpiGateRes / EpiQKV, + qknorm_rope_kernel and the LayerNorm that
produces their A operands) through f5k_gemm_epi / f5k_layernorm_mod_ex, on every dispatch path: the fragment-order stores of
the v2 kernels and of the ping-pong kernel's edge tiles, the staged (LDS, row-major) stores of its interior tiles, the
remainder launch at GemmConv::m_base, the device-side row count with packed rows (rowmap), pre-split f16x3 operands and the
f16 QKV output of the f16x3 attention path.

Three kinds of check:
  * exact layouts: operands whose products and sums are exact in f32 and in the output type (A = a tiled identity, small
    integer / 8 W and bias, quarter-turn rotary tables, power-of-two gates): torch.equal against the float64 result;
  * random data against float64 on the operands as the kernel rounds them: rel_err < 2e-5 for f32 outputs; 16-bit outputs
    (operands on a coarse lattice, so that the f32 accumulation is exact) within 1 ulp of the float64 value rounded;
  * untouched memory: every output lives between guard bands of a NaN sentinel, and what the epilogue must not write
    (rows past m_limit, V^T columns [Nseq, Npad), positions past a packed utterance, the guard bands) is checked bit for bit;
    masked residual rows must equal res bit for bit.
Plus the bit identities the engine relies on (remainder split, pre-split A, planar store, staged vs fragment tile, packed vs
padded rows) and run-to-run determinism of the staged paths."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded, k_gemm_epi, k_layernorm_mod_ex, split_planar64  # noqa: E402

from f5_tts_amd import _lib  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

STORE, GATE_RES, QKV, QKNORM = _lib.F5K_EPI_STORE, _lib.F5K_EPI_GATE_RES, _lib.F5K_EPI_QKV, _lib.F5K_EPI_QKNORM
TDTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
CFGS = [-1, 2, 8, 9, 10, 13, 20]
# operand modes: name -> (precision, A pre-split, QKV output as f16 on f32 operands)
MODES = {"f32": ("f32", False, False), "f16x3": ("f16x3", False, False), "f16x3p": ("f16x3", True, False),
         "bf16": ("bf16", False, False), "f16": ("f16", False, False), "attn16": ("f16x3", True, True)}


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


def rnd(prec, x):
    """x as the MFMA operand type sees it (f16x3: hi + lo halves, 22 bits, treated as unchanged, as in test_kernels_gpu)."""
    return x if prec in ("f32", "f16x3") else x.to(TDTYPE[prec]).float()


def out_dtype(mode, sixteen):
    prec, _, o16 = MODES[mode]
    if not sixteen and not o16:
        return torch.float32
    return TDTYPE.get(prec, torch.float16)


def v3_ok(mode, H=None):
    """cfg 20 (ping-pong kernel) exists for 16-bit operands and pre-split f16x3 operands; QKV needs 2 H 64 % 256 == 0."""
    prec, pre, _ = MODES[mode]
    return (prec in ("bf16", "f16") or pre) and (H is None or H % 2 == 0)


def ulp_dist(out16, ref64, dt):
    """max distance in units in the last place of dt between a 16-bit result and the float64 reference rounded to dt."""
    def key(t):
        b = t.to(dt).view(torch.int16).to(torch.int32)
        return torch.where(b < 0, -(b & 0x7FFF), b)
    return (key(out16) - key(ref64)).abs().max().item()


# ---------------------------------------------------------------------------------------------------------- data
def lattice(g, shape, lo, hi, den):
    return (torch.randint(lo, hi + 1, shape, generator=g).float() / den).to(DEV)


def exact_operands(M, N, K, seed=0):
    """A: a tiled identity with a second, doubled marker per row (rows m and m + K differ); W, bias: asymmetric integers / 8.
    Every output value is a multiple of 1/8 below 4 in magnitude: exact in f32, bf16 and f16."""
    m = torch.arange(M)
    A = torch.zeros(M, K)
    A[m, m % K] += 1.0
    A[m, (37 * (m // K) + 11 + seed) % K] += 2.0
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    W = ((n * 7 + k * 13 + (n * k) % 5 + seed) % 15 - 7).float() / 8
    b = ((torch.arange(N) * 5 + seed) % 15 - 7).float() / 8
    return A.to(DEV), W.to(DEV), b.to(DEV)


def random_operands(M, N, K, seed, coarse):
    """coarse: lattice values (A in k/4, W in k/64, bias in k/64) whose f32 products and sums are exact, for the 1-ulp checks of
    16-bit outputs; else Gaussian."""
    g = torch.Generator().manual_seed(seed)
    if coarse:
        return lattice(g, (M, K), -4, 4, 4), lattice(g, (N, K), -8, 8, 64), lattice(g, (N,), -64, 64, 64)
    return (torch.randn(M, K, generator=g).to(DEV), (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV),
            torch.randn(N, generator=g).to(DEV))


def quarter_turn_tables(maxpos):
    """cos / sin in {0, +-1}: turn (3 pos + 5 pair + pos * pair) % 4, asymmetric in (pos, pair)."""
    p, j = torch.arange(maxpos)[:, None], torch.arange(32)[None, :]
    t = (3 * p + 5 * j + p * j) % 4
    cs = torch.tensor([1.0, 0.0, -1.0, 0.0])[t]
    sn = torch.tensor([0.0, 1.0, 0.0, -1.0])[t]
    return cs.to(DEV), sn.to(DEV)


def rotary_freqs(maxpos):
    return O.rotary_freqs(maxpos, 64)   # [maxpos, 64], interleaved pairs share a frequency


def rotary_tables(maxpos, coarse):
    f = rotary_freqs(maxpos)[:, ::2]
    cs, sn = f.cos(), f.sin()
    if coarse:   # multiples of 1/256: the rotary products of lattice values stay exact in f32
        cs, sn = (cs * 256).round() / 256, (sn * 256).round() / 256
    return cs.contiguous().to(DEV), sn.contiguous().to(DEV)


# ----------------------------------------------------------------------------------------------------- references
def gemm64(prec, A, W, b):
    return rnd(prec, A).double() @ rnd(prec, W).double().t() + b.double()


def gelu_tanh64(x):
    """torch's 0.5 x (1 + tanh(u)) written as x sigmoid(2 u): the tanh form cancels to 0 in float64 below x ~ -7, where bf16 still
    holds the (tiny) value."""
    return x * torch.sigmoid(2.0 * 0.7978845608028654 * (x + 0.044715 * x ** 3))


def rope64(x, cs, sn, Nseq):
    """interleaved pairs (2j, 2j + 1) of x [..., Nseq, 64] -> (a cos - b sin, b cos + a sin) with tables [maxpos, 32]."""
    c, s = cs[:Nseq].double(), sn[:Nseq].double()
    a, bb = x[..., 0::2], x[..., 1::2]
    return torch.stack((a * c - bb * s, bb * c + a * s), dim=-1).flatten(-2)


def qkv64(C, Bp, Nseq, H, pe_heads, q_scale, cs, sn):
    """C [Bp * Nseq, 3 H 64] -> q, k [Bp, H, Nseq, 64], vt [Bp, H, 64, Nseq] (modules.py:469-497 as EpiQKV computes it)."""
    C = C.view(Bp, Nseq, 3, H, 64)
    q, k = C[:, :, 0].permute(0, 2, 1, 3).clone(), C[:, :, 1].permute(0, 2, 1, 3).clone()
    vt = C[:, :, 2].permute(0, 2, 3, 1)
    if pe_heads:
        q[:, :pe_heads] = rope64(q[:, :pe_heads], cs, sn, Nseq)
        k[:, :pe_heads] = rope64(k[:, :pe_heads], cs, sn, Nseq)
    return q * q_scale, k, vt


# ------------------------------------------------------------------------------------------------------- runners
def run_store(mode, A, W, b, *, sixteen=False, act=0, planar=0, cfg=-1, m_limit=-1):
    prec, pre, _ = MODES[mode]
    M, N = A.shape[0], W.shape[0]
    out = Guarded((M, N), out_dtype(mode, sixteen))
    val, = k_gemm_epi(prec, A, W, b, STORE, [out], cfg=cfg, a_presplit=pre, m_limit=m_limit, out16=sixteen, act=act, planar=planar)
    assert out.guards_intact()
    if m_limit >= 0:
        assert (out.bits[m_limit:] == out.sent).all(), "rows at or past m_limit were written"
    return out, val


def run_gate_res(mode, A, W, b, res, gate, gate_stride, rpb, lens=None, *, alias=True, cfg=-1, m_limit=-1):
    prec, pre, _ = MODES[mode]
    M, N = A.shape[0], W.shape[0]
    x = Guarded.like(res) if alias else Guarded((M, N), torch.float32)
    r = x if alias else res
    val, = k_gemm_epi(prec, A, W, b, GATE_RES, [x], cfg=cfg, a_presplit=pre, m_limit=m_limit, res=r, gate=gate,
                      gate_stride=gate_stride, rows_per_batch=rpb, lens=lens)
    assert x.guards_intact()
    if m_limit >= 0:
        tail = x.bits[m_limit:]
        assert torch.equal(tail, res[m_limit:].view(torch.int32)) if alias else (tail == x.sent).all(), "rows past m_limit written"
    return x, val


def gate_res64(prec, A, W, b, res, gate, gate_stride, rpb, lens):
    C = gemm64(prec, A, W, b)
    M = C.shape[0]
    bi = torch.arange(M, device=DEV) // rpb
    g = gate.view(-1)[(bi * gate_stride)[:, None] + torch.arange(C.shape[1], device=DEV)[None, :]].double() if gate is not None else 1.0
    x = res.double() + g * C
    if lens is not None:
        keep = (torch.arange(M, device=DEV) - bi * rpb) < torch.tensor(lens, device=DEV)[bi]
        x = torch.where(keep[:, None], x, res.double())
    return x


def run_qkv(mode, A, W, b, Bp, Nseq, H, pe_heads, q_scale, cs, sn, *, cfg=-1, row_start=None, norm=False, gq=None, gk=None):
    prec, pre, o16 = MODES[mode]
    Npad = (Nseq + 63) // 64 * 64
    dt = out_dtype(mode, prec in ("bf16", "f16"))
    outs = [Guarded((Bp, H, Nseq, 64), dt), Guarded((Bp, H, Nseq, 64), dt), Guarded((Bp, H, 64, Npad), dt)]
    vals = k_gemm_epi(prec, A, W, b, QKNORM if norm else QKV, outs, cfg=cfg, a_presplit=pre, out16=o16, H=H, Nseq=Nseq, Npad=Npad,
                      pe_heads=pe_heads, q_scale=q_scale, rope_cos=cs, rope_sin=sn, row_start=row_start, Bp=Bp, gq=gq, gk=gk)
    for o in outs:
        assert o.guards_intact()
    assert (outs[2].bits[..., Nseq:] == outs[2].sent).all(), "V^T columns [Nseq, Npad) were written"
    return outs, [vals[0], vals[1], vals[2][..., :Nseq]]


def assert_same_bits(x, y, what):
    """torch.equal on the bit patterns of two Guarded buffers; on failure, where they differ."""
    d = x.bits != y.bits
    if d.any():
        idx = d.nonzero()
        j = tuple(idx[0].tolist())
        raise AssertionError(f"{what}: {len(idx)} elements differ, first at {j} ({x.value[j].item()} vs {y.value[j].item()}), "
                             f"dims {[idx[:, i].unique().tolist()[:8] for i in range(idx.shape[1])]}")


def check_random(vals, refs, dt, label):
    """f32 outputs: rel_err < 2e-5 against float64; 16-bit outputs: every element within 1 ulp of float64 rounded to dt."""
    for v, r in zip(vals, refs):
        assert torch.isfinite(v).all(), label
        if dt == torch.float32:
            e = rel_err(v, r)
            print(f"[{label}] rel_err {e:.2e}")
            assert e < 2e-5, label
        else:
            u = ulp_dist(v, r, dt)
            print(f"[{label}] max ulp {u}")
            assert u <= 1, label


# ================================================================================================ exact layouts: STORE
STORE_MODES = [("f32", False), ("f16x3", False), ("f16x3p", False), ("bf16", False), ("bf16", True), ("f16", True)]


@pytest.mark.parametrize("mode,sixteen,cfg", [(m, s, c) for m, s in STORE_MODES for c in CFGS if c != 20 or v3_ok(m)])
def test_store_exact_layout(mode, sixteen, cfg):
    """(cfg 20 only where the ping-pong kernel exists: test_cfg20_refused_where_it_does_not_exist)"""
    M, N, K = 600, 512, 256   # 600 = 2 x 256 + 88: interior and edge row tiles of every tile shape
    A, W, b = exact_operands(M, N, K)
    ref = gemm64(MODES[mode][0], A, W, b)
    out, val = run_store(mode, A, W, b, sixteen=sixteen, cfg=cfg)
    assert torch.equal(val, ref.float()), (mode, cfg)
    out, val = run_store(mode, A, W, b, sixteen=sixteen, cfg=cfg, m_limit=333)
    assert torch.equal(val[:333], ref[:333].float()), (mode, cfg)


def test_cfg20_refused_where_it_does_not_exist():
    A, W, b = exact_operands(64, 64, 64)
    for mode in ("f32", "f16x3"):
        with pytest.raises(_lib.F5Error):
            run_store(mode, A, W, b, cfg=20)
    cs, sn = quarter_turn_tables(64)
    A, W, b = exact_operands(64, 3 * 3 * 64, 64)
    with pytest.raises(_lib.F5Error):   # odd H: the V third starts inside a 256-column tile
        run_qkv("bf16", A, W, b, 1, 64, 3, 1, 0.125, cs, sn, cfg=20)


# ============================================================================================= exact layouts: GATE_RES
@pytest.mark.parametrize("mode,cfg", [(m, c) for m in ["f32", "f16x3", "f16x3p", "bf16", "f16"] for c in CFGS if c != 20 or v3_ok(m)])
@pytest.mark.parametrize("rpb,alias", [(72, False), (300, True), (48, True)])
def test_gate_res_exact_layout(mode, cfg, rpb, alias):
    """Power-of-two gates that differ per batch row and column; ragged lens (masked rows keep res bit for bit); rpb 72: 64-row
    halves straddle two batch rows; 48: the staged path is off."""
    M, N, K = 600, 512, 256
    A, W, b = exact_operands(M, N, K, seed=1)
    nb = (M - 1) // rpb + 1
    g = torch.Generator().manual_seed(rpb)
    res = lattice(g, (M, N), -40, 40, 8)
    gate = torch.exp2(((torch.arange(nb)[:, None] * 3 + torch.arange(N)[None, :]) % 5 - 2).float()).to(DEV)
    lens = [(rpb * (i + 1) * 5) // 7 % (rpb + 1) for i in range(nb)]
    lens[0] = rpb
    ref = gate_res64(MODES[mode][0], A, W, b, res, gate, N, rpb, lens)
    x, val = run_gate_res(mode, A, W, b, res, gate, N, rpb, lens, alias=alias, cfg=cfg)
    assert torch.equal(val, ref.float()), (mode, cfg)
    keep = (torch.arange(M, device=DEV) % rpb) < torch.tensor(lens, device=DEV)[torch.arange(M, device=DEV) // rpb]
    assert torch.equal(x.bits[~keep], res[~keep].view(torch.int32)), "a masked row does not keep res"
    x, val = run_gate_res(mode, A, W, b, res, gate, N, rpb, lens, alias=alias, cfg=cfg, m_limit=401)
    assert torch.equal(val[:401], ref[:401].float())


# ================================================================================================== exact layouts: QKV
@pytest.mark.parametrize("mode,cfg,Bp,Nseq,H,pe", [(m, c, *shape) for shape in [(2, 520, 4, 1), (3, 200, 3, 3)] for m in MODES
                                                    for c in CFGS if c != 20 or v3_ok(m, shape[2])])
def test_qkv_exact_layout(mode, cfg, Bp, Nseq, H, pe):
    """Head split, q / k layout, V^T layout with Npad, rotary pair map: bit for bit (quarter-turn tables, q_scale 1/8).
    (2, 520, 4): staged q / k / V^T in interior ping-pong tiles, fragment stores at the edges; (3, 200, 3): odd H, Nseq % 8 != 0."""
    K = 256
    A, W, b = exact_operands(Bp * Nseq, 3 * H * 64, K, seed=2)
    cs, sn = quarter_turn_tables(Nseq + 5)
    ref = qkv64(gemm64(MODES[mode][0], A, W, b), Bp, Nseq, H, pe, 0.125, cs, sn)
    _, vals = run_qkv(mode, A, W, b, Bp, Nseq, H, pe, 0.125, cs, sn, cfg=cfg)
    for name, v, r in zip("q k vt".split(), vals, ref):
        assert torch.equal(v, r.float()), (mode, cfg, name)


# =============================================================================================== random data, float64
@pytest.mark.parametrize("mode,sixteen", [("f32", False), ("f16x3", False), ("f16x3p", False), ("bf16", False), ("bf16", True),
                                          ("f16", True)])
@pytest.mark.parametrize("M,N,K,act", [(2048, 2048, 1024, 1), (1000, 1024, 1024, 0), (333, 256, 256, 1)])
def test_store_random_float64(mode, sixteen, M, N, K, act):
    """FF1 (K 1024 -> 2048, GELU-tanh), a row count that is not a multiple of 256, one small D."""
    prec = MODES[mode][0]
    dt = out_dtype(mode, sixteen)
    A, W, b = random_operands(M, N, K, seed=M + N, coarse=dt != torch.float32)
    ref = gemm64(prec, A, W, b)
    if act:
        ref = gelu_tanh64(ref)
    _, val = run_store(mode, A, W, b, sixteen=sixteen, act=act)
    check_random([val], [ref], dt, f"store {mode} {M}x{N}x{K} act {act}")


GATE_CASES = [  # rows, rpb, gate (1: one vector per batch row, 0: one vector for all, None: no gate = 1), lens pattern, alias
    (2048, 1024, 1, "ragged", True), (2050, 1025, 1, None, False), (2 * 1025, 1025, 0, "full", True), (720, 72, 1, "ragged", False),
    (480, 48, 1, "ragged", True), (16 * 1025, 1025, 1, "ragged", False),
    (2050, 1025, None, "ragged", False),   # UNetT out-projection: no gate, lens, x_in != x
    (720, 72, None, None, True)]           # UNetT FF2 / text encoder: no gate, no lens


def make_lens(pattern, nb, rpb):
    if pattern is None:
        return None
    if pattern == "full":
        return [rpb] * nb
    return [rpb if i == 0 else (0 if i == 1 else (rpb * (3 * i + 1)) // (3 * i + 4)) for i in range(nb)]


@pytest.mark.parametrize("mode", ["f32", "f16x3", "f16x3p", "bf16", "f16"])
@pytest.mark.parametrize("M,rpb,gs,lp,alias", GATE_CASES)
def test_gate_res_random_float64(mode, M, rpb, gs, lp, alias):
    prec = MODES[mode][0]
    N, K = 1024, 1024 if M >= 2048 else 256
    A, W, b = random_operands(M, N, K, seed=M + rpb, coarse=False)
    nb = (M - 1) // rpb + 1
    g = torch.Generator().manual_seed(rpb)
    res = torch.randn(M, N, generator=g).to(DEV)
    gate = None if gs is None else torch.randn(nb if gs else 1, N, generator=g).to(DEV)
    lens = make_lens(lp, nb, rpb)
    ref = gate_res64(prec, A, W, b, res, gate, N if gs else 0, rpb, lens)
    x, val = run_gate_res(mode, A, W, b, res, gate, N if gs else 0, rpb, lens, alias=alias)
    check_random([val], [ref], torch.float32, f"gate_res {mode} M={M} rpb={rpb}")
    if lens is not None:
        bi = torch.arange(M, device=DEV) // rpb
        keep = (torch.arange(M, device=DEV) - bi * rpb) < torch.tensor(lens, device=DEV)[bi]
        assert torch.equal(x.bits[~keep], res[~keep].view(torch.int32)), "a masked row does not keep res"


QKV_CASES = [  # Bp, Nseq, H, pe_heads, D
    (2, 1024, 16, 1, 1024),   # staged V^T fast path
    (2, 1025, 16, 16, 1024),  # Nseq % 8 != 0: staged V^T off
    (16, 1025, 16, 1, 1024),  # 16,400 rows: remainder split at m_base = 16,384
    (3, 200, 4, 0, 256),      # ragged M and N tiles
    (1, 7, 4, 4, 256),        # Nseq < 8
    (2, 264, 3, 1, 256),      # odd H: no ping-pong kernel
]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("Bp,Nseq,H,pe,D", QKV_CASES)
def test_qkv_random_float64(mode, Bp, Nseq, H, pe, D):
    prec, _, o16 = MODES[mode]
    dt = out_dtype(mode, prec in ("bf16", "f16"))
    coarse = dt != torch.float32
    A, W, b = random_operands(Bp * Nseq, 3 * H * 64, D, seed=Nseq + H, coarse=coarse)
    cs, sn = rotary_tables(Nseq + 3, coarse)
    q_scale = 0.125
    ref = qkv64(gemm64(prec, A, W, b), Bp, Nseq, H, pe, q_scale, cs, sn)
    _, vals = run_qkv(mode, A, W, b, Bp, Nseq, H, pe, q_scale, cs, sn)
    check_random(vals, ref, dt, f"qkv {mode} {Bp}x{Nseq} H={H} pe={pe}")


# QKNORM: max |out - ref| / max |ref| over q and k measured on MI355X (tests print it) -- f32 1.14e-6, f16x3 6.7e-7,
# bf16 4.8e-3, f16 6.9e-4 -- and tolerances at ~2x that
QKNORM_TOLS = {"f32": 2.5e-6, "f16x3": 1.5e-6, "f16x3p": 1.5e-6, "bf16": 1e-2, "f16": 1.4e-3}


@pytest.mark.parametrize("mode", list(QKNORM_TOLS))
@pytest.mark.parametrize("Bp,Nseq,H,pe", [(2, 1024, 16, 1), (3, 200, 4, 4)])
def test_qknorm_matches_oracle(mode, Bp, Nseq, H, pe):
    """qk_norm = "rms_norm": the QKV epilogue leaves q / k raw (no rotary, no scale), qknorm_rope_kernel applies RMSNorm, rotary,
    q scale in place -- through launch_qknorm_rope, the launcher the engine's qkv_project calls, in the own layout (layout length =
    Nseq, offset 0; the MMDiT's joint layout is the same kernel at another length and offset).  Reference: oracle RMSNorm (F.rms_norm) and rotary_apply on the float64 QKV result of the rounded operands.
    Under bf16 / f16 the raw q / k are rounded to 16 bit between the two launches and the result again at the end: two roundings
    of the operand type, so the tolerance there is a few of its ulps relative to the largest element."""
    prec = MODES[mode][0]
    D = 1024 if H == 16 else 256
    A, W, b = random_operands(Bp * Nseq, 3 * H * 64, D, seed=Nseq + 5, coarse=False)
    g = torch.Generator().manual_seed(7)
    gq, gk = (1.0 + 0.3 * torch.randn(64, generator=g)).to(DEV), (1.0 + 0.3 * torch.randn(64, generator=g)).to(DEV)
    freqs = rotary_freqs(Nseq + 2)
    cs, sn = freqs[:, ::2].cos().contiguous().to(DEV), freqs[:, ::2].sin().contiguous().to(DEV)
    q_scale = 0.125
    C = gemm64(prec, A, W, b).view(Bp, Nseq, 3, H, 64)
    f64 = freqs[:Nseq].double().to(DEV)
    refs = []
    for which, gain in ((0, gq), (1, gk)):
        x = F.rms_norm(C[:, :, which].permute(0, 2, 1, 3), (64,), weight=gain.double(), eps=1e-6)
        if pe:
            x = torch.cat((O.rotary_apply(x[:, :pe], f64), x[:, pe:]), dim=1)
        refs.append(x * (q_scale if which == 0 else 1.0))
    _, vals = run_qkv(mode, A, W, b, Bp, Nseq, H, pe, q_scale, cs, sn, norm=True, gq=gq, gk=gk)
    for name, v, r in zip("qk", vals, refs):
        assert torch.isfinite(v).all()
        e = rel_err(v, r)
        print(f"[qknorm {mode} {Bp}x{Nseq} H={H} pe={pe}] {name}: rel_err {e:.2e}")
        assert e < QKNORM_TOLS[mode], name
    C32 = C[:, :, 2].permute(0, 2, 3, 1)
    assert rel_err(vals[2], C32) < (2e-5 if prec in ("f32", "f16x3") else 8e-3)


# ============================================================================================= bit identities
@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3p", "attn16"])
def test_remainder_split_matches_one_64x64_launch(mode):
    """16 x 1025 rows: launch_gemm runs the first 16,384 rows on the ping-pong kernel and the last 16 at GemmConv::m_base = 16,384;
    every epilogue must equal one forced 64x64 launch (same K order per element) bit for bit."""
    prec, _, _ = MODES[mode]
    M, D = 16 * 1025, 1024
    sixteen = prec in ("bf16", "f16")
    A, W, b = random_operands(M, 1024, D, seed=3, coarse=False)
    if mode != "attn16":
        _, v0 = run_store(mode, A, W, b, sixteen=sixteen, act=1)
        _, v1 = run_store(mode, A, W, b, sixteen=sixteen, act=1, cfg=8)
        assert torch.equal(v0, v1), "store"
        g = torch.Generator().manual_seed(4)
        res, gate = torch.randn(M, 1024, generator=g).to(DEV), torch.randn(16, 1024, generator=g).to(DEV)
        lens = [1025 - 3 * i for i in range(16)]
        _, v0 = run_gate_res(mode, A, W, b, res, gate, 1024, 1025, lens, alias=False)
        _, v1 = run_gate_res(mode, A, W, b, res, gate, 1024, 1025, lens, alias=False, cfg=8)
        assert torch.equal(v0, v1), "gate_res"
    A, W, b = random_operands(M, 3 * 1024, D, seed=5, coarse=False)
    cs, sn = rotary_tables(1025, False)
    o0, _ = run_qkv(mode, A, W, b, 16, 1025, 16, 1, 0.125, cs, sn)
    o1, _ = run_qkv(mode, A, W, b, 16, 1025, 16, 1, 0.125, cs, sn, cfg=8)
    for x, y, name in zip(o0, o1, "q k vt".split()):
        assert_same_bits(x, y, name)


@pytest.mark.parametrize("cfg", [-1, 2, 8, 9, 10, 13])
def test_presplit_a_matches_in_register_split(cfg):
    """f16x3: an A operand stored pre-split (MODE 5 / DIAG 8) and one split in registers (MODE 3) give the same bits, every epilogue."""
    M, D = 1100, 256
    A, W, b = random_operands(M, 768, D, seed=8, coarse=False)
    _, v0 = run_store("f16x3", A, W, b, act=1, cfg=cfg)
    _, v1 = run_store("f16x3p", A, W, b, act=1, cfg=cfg)
    assert torch.equal(v0, v1), "store"
    g = torch.Generator().manual_seed(9)
    res, gate = torch.randn(M, 768, generator=g).to(DEV), torch.randn(11, 768, generator=g).to(DEV)
    lens = [100, 37, 0] + [100] * 8
    _, v0 = run_gate_res("f16x3", A, W, b, res, gate, 768, 100, lens, alias=False, cfg=cfg)
    _, v1 = run_gate_res("f16x3p", A, W, b, res, gate, 768, 100, lens, alias=False, cfg=cfg)
    assert torch.equal(v0, v1), "gate_res"
    cs, sn = rotary_tables(1100, False)
    o0, _ = run_qkv("f16x3", A, W, b, 2, 550, 4, 4, 0.125, cs, sn, cfg=cfg)
    o1, _ = run_qkv("f16x3p", A, W, b, 2, 550, 4, 4, 0.125, cs, sn, cfg=cfg)
    for x, y, name in zip(o0, o1, "q k vt".split()):
        assert torch.equal(x.bits, y.bits), name


@pytest.mark.parametrize("cfg", [-1, 2, 8, 13])
def test_planar_store_matches_split_of_plain_store(cfg):
    """EpiStore<float> planar (store4_planar: what FF1 / LayerNorm hand the next f16x3 GEMM) == split_planar_kernel(plain store)."""
    A, W, b = random_operands(700, 1024, 256, seed=10, coarse=False)
    p1, _ = run_store("f16x3p", A, W, b, act=1, planar=1, cfg=cfg)
    p2, plain = run_store("f16x3p", A, W, b, act=1, planar=2, cfg=cfg)
    assert torch.equal(p1.bits, p2.bits)
    assert torch.equal(p1.bits, split_planar64(run_store("f16x3p", A, W, b, act=1, cfg=cfg)[1]))
    _, v = run_store("f16x3p", A, W, b, act=1, planar=1, cfg=cfg, m_limit=450)
    assert torch.equal(p1.bits[:450], v.view(torch.int32)[:450])


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3p", "attn16"])
def test_staged_interior_rows_match_fragment_edge_rows(mode):
    """The ping-pong kernel stores interior tiles through LDS (staged) and edge tiles in fragment order: the same rows, computed
    once in an interior tile (M = 768) and once in an edge tile (M shortened to 712 / 456), must agree bit for bit."""
    prec = MODES[mode][0]
    sixteen = prec in ("bf16", "f16")
    A, W, b = random_operands(768, 1024, 512, seed=12, coarse=False)
    if mode != "attn16":
        _, full = run_store(mode, A, W, b, sixteen=sixteen, act=1, cfg=20)
        for m in (712, 456):
            _, part = run_store(mode, A[:m], W, b, sixteen=sixteen, act=1, cfg=20)
            assert torch.equal(part, full[:m]), ("store", m)
        g = torch.Generator().manual_seed(13)
        res, gate = torch.randn(768, 1024, generator=g).to(DEV), torch.randn(11, 1024, generator=g).to(DEV)
        lens = [72, 30, 64, 0, 72, 5, 72, 72, 71, 1, 72]
        _, full = run_gate_res(mode, A, W, b, res, gate, 1024, 72, lens, alias=False, cfg=20)
        for m in (712, 456):
            _, part = run_gate_res(mode, A[:m], W, b, res[:m], gate, 1024, 72, lens, alias=False, cfg=20)
            assert torch.equal(part, full[:m]), ("gate_res", m)
    A, W, b = random_operands(768, 3 * 512, 512, seed=14, coarse=False)
    cs, sn = rotary_tables(768, False)
    _, full = run_qkv(mode, A, W, b, 1, 768, 8, 2, 0.125, cs, sn, cfg=20)
    for m in (712, 456):
        _, part = run_qkv(mode, A[:m], W, b, 1, m, 8, 2, 0.125, cs, sn, cfg=20)
        for x, y, name in zip(part, full, "q k vt".split()):
            assert torch.equal(x, y[..., :m, :] if name != "vt" else y[..., :m]), (name, m)


def packed(lens, Nseq):
    rs = [0]
    for n in lens:
        rs.append(rs[-1] + (n + 3) // 4 * 4)
    return rs


@pytest.mark.parametrize("mode", ["f32", "f16x3p", "bf16", "f16", "attn16"])
@pytest.mark.parametrize("Nseq,lens,H", [(1024, [1024, 700], 16), (200, [200, 37, 129], 4), (1025, [1025, 3, 512], 4)])
def test_packed_rows_match_padded_rows(mode, Nseq, lens, H):
    """RowPack: utterance b occupies rows row_start[b] .. (multiples of 4), rowmap gives (b, pos), m_limit = row_start[Bp].  Its
    rows must equal the same positions of a padded launch bit for bit; positions past an utterance's rows stay untouched."""
    Bp, D = len(lens), 1024 if H == 16 else 256
    A, W, b = random_operands(Bp * Nseq, 3 * H * 64, D, seed=Nseq + len(lens), coarse=False)
    cs, sn = rotary_tables(Nseq + 3, False)
    pe = 1 if H == 16 else H
    padded, _ = run_qkv(mode, A, W, b, Bp, Nseq, H, pe, 0.125, cs, sn)
    rs = packed(lens, Nseq)
    Ap = torch.zeros_like(A)
    for i in range(Bp):
        cnt = rs[i + 1] - rs[i]
        n = min(cnt, Nseq)
        Ap[rs[i]:rs[i] + n] = A[i * Nseq:i * Nseq + n]
    pk, _ = run_qkv(mode, Ap, W, b, Bp, Nseq, H, pe, 0.125, cs, sn, row_start=rs)
    for i in range(Bp):
        cnt = min(rs[i + 1] - rs[i], Nseq)
        for name, x, y in zip("q k".split(), pk, padded):
            assert torch.equal(x.bits[i, :, :cnt], y.bits[i, :, :cnt]), (name, i)
            assert (x.bits[i, :, cnt:] == x.sent).all(), (name, i, "written past the utterance")
        assert torch.equal(pk[2].bits[i, ..., :cnt], padded[2].bits[i, ..., :cnt]), ("vt", i)
        assert (pk[2].bits[i, ..., cnt:] == pk[2].sent).all(), ("vt", i, "written past the utterance")


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3p", "attn16"])
def test_staged_paths_are_deterministic(mode):
    """Race detector for the staged epilogues (a wave's LDS slice, no barrier): 4 repeats, bit-equal."""
    prec = MODES[mode][0]
    sixteen = prec in ("bf16", "f16")
    A, W, b = random_operands(2048, 3072, 1024, seed=15, coarse=False)
    cs, sn = rotary_tables(1024, False)
    ref, _ = run_qkv(mode, A, W, b, 2, 1024, 16, 16, 0.125, cs, sn)
    for _ in range(4):
        again, _ = run_qkv(mode, A, W, b, 2, 1024, 16, 16, 0.125, cs, sn)
        assert all(torch.equal(x.bits, y.bits) for x, y in zip(ref, again))
    if mode == "attn16":
        return
    W2, b2 = W[:2048].contiguous(), b[:2048].contiguous()
    ref, _ = run_store(mode, A, W2, b2, sixteen=sixteen, act=1)
    g = torch.Generator().manual_seed(16)
    res, gate = torch.randn(2048, 1024, generator=g).to(DEV), torch.randn(2, 1024, generator=g).to(DEV)
    gref, _ = run_gate_res(mode, A, W[:1024].contiguous(), b[:1024].contiguous(), res, gate, 1024, 1024, [1024, 611], alias=False)
    for _ in range(4):
        assert torch.equal(run_store(mode, A, W2, b2, sixteen=sixteen, act=1)[0].bits, ref.bits)
        x, _ = run_gate_res(mode, A, W[:1024].contiguous(), b[:1024].contiguous(), res, gate, 1024, 1024, [1024, 611], alias=False)
        assert torch.equal(x.bits, gref.bits)


# ======================================================================================================= LayerNorm
@pytest.mark.parametrize("prec", ["f32", "f16x3", "bf16", "f16"])
@pytest.mark.parametrize("R,D,rpb", [(2050, 1024, 1025), (300, 256, 72)])
def test_layernorm_outputs_of_every_precision(prec, R, D, rpb):
    """layernorm_kernel<TO>: the f32 rows against float64; the 16-bit rows == the f32 rows rounded (same f32 arithmetic); the planar
    rows == split_planar_kernel(f32 rows); rows at or past m_limit untouched."""
    g = torch.Generator().manual_seed(R + D)
    x = (torch.randn(R, D, generator=g) * 3 + 1).to(DEV)
    nb = (R - 1) // rpb + 1
    sc, sh = torch.randn(nb, D, generator=g).to(DEV), torch.randn(nb, D, generator=g).to(DEV)
    f32 = Guarded((R, D), torch.float32)
    v32 = k_layernorm_mod_ex("f32", x, sc, sh, f32, rpb).clone()
    assert f32.guards_intact()
    if prec == "f32":   # (the other precisions are checked against these f32 rows)
        bi = torch.arange(R, device=DEV) // rpb
        ref = F.layer_norm(x.double(), (D,), eps=1e-6) * (1 + sc.double()[bi]) + sh.double()[bi]
        assert (v32 - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    if prec in ("bf16", "f16"):
        dt = TDTYPE[prec]
        out = Guarded((R, D), dt)
        v = k_layernorm_mod_ex(prec, x, sc, sh, out, rpb)
        assert out.guards_intact()
        assert torch.equal(out.value, v32.to(dt)) and torch.equal(v, v32.to(dt).float())
    else:
        out = Guarded((R, D), torch.float32)
        k_layernorm_mod_ex(prec, x, sc, sh, out, rpb, planar=1)
        ref_split = Guarded((R, D), torch.float32)
        k_layernorm_mod_ex(prec, x, sc, sh, ref_split, rpb, planar=2)
        assert out.guards_intact() and torch.equal(out.bits, ref_split.bits)
        assert torch.equal(out.bits, split_planar64(v32))
    ml = R - 77
    for planar in ((0, 1) if prec in ("f32", "f16x3") else (0,)):
        out = Guarded((R, D), torch.float32 if prec in ("f32", "f16x3") else TDTYPE[prec])
        k_layernorm_mod_ex(prec, x, sc, sh, out, rpb, m_limit=ml, planar=planar)
        assert out.guards_intact()
        assert (out.bits[ml:] == out.sent).all(), "rows at or past m_limit were written"
        assert (out.bits[:ml] != out.sent).all()
