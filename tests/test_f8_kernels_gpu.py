"""GPU: the kernels of the f8 precision (F5_PREC_F8) against the contract of include/f5_hip.h.

  G1  the e4m3 GEMM with exact integer operands: lane map, row / column orientation, scale application, every tile, a device row
      count, the remainder launch -- torch.equal against float64, outputs between NaN guard bands;
  G2  both quantisers (stand-alone rows, fused into the AdaLN LayerNorm) bit for bit against tests/f8_oracle.py;
  G3  random operands against float64 on the operands as the quantiser left them, through the three block epilogues.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded, _p, _s, k_gemm_epi, k_gemm_plan, k_layernorm_mod  # noqa: E402

import f8_oracle as Q  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from test_epilogues_gpu import (gate_res64, gelu_tanh64, packed, qkv64, random_operands, rel_err, rotary_tables,  # noqa: E402
                                ulp_dist)

STORE, GATE_RES, QKV = _lib.F5K_EPI_STORE, _lib.F5K_EPI_GATE_RES, _lib.F5K_EPI_QKV
F8_CFGS = [-1, 2, 8, 13]
SENT8 = 0xA5


# ------------------------------------------------------------------------------------------------------- entry points
def k_quant_rows(x, K=None, ldc=None, m_limit=-1):
    """f5k_quant_rows_e4m3 on x [R, ld] (f32 / f16 / bf16): (codes uint8 [R, ldc], scales uint8 [R]) inside sentinel-filled buffers,
    returned with their guard bands checked."""
    R, ld = x.shape
    K = ld if K is None else K
    ldc = K if ldc is None else ldc
    prec = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[x.dtype]
    codes = torch.full((R * ldc + 128,), SENT8, dtype=torch.uint8, device=DEV)
    scales = torch.full((R + 128,), SENT8, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().f5k_quant_rows_e4m3(_lib.PRECISIONS[prec], _p(x), ld, R, K, C.c_void_p(codes.data_ptr() + 64), ldc,
                                               C.c_void_p(scales.data_ptr() + 64), m_limit, _s()), "f5k_quant_rows_e4m3")
    for t, n in ((codes, R * ldc), (scales, R)):
        assert (t[:64] == SENT8).all() and (t[64 + n:] == SENT8).all(), "guard bytes were written"
    return codes[64:64 + R * ldc].view(R, ldc).cpu(), scales[64:64 + R].cpu()   # (compared on the CPU, where the restatement was checked)


def k_layernorm_q8(x, scale, shift, rows_per_batch, m_limit=-1, batch_of_row=None, eps=1e-6):
    R, D = x.shape
    codes = torch.full((R * D + 128,), SENT8, dtype=torch.uint8, device=DEV)
    scales = torch.full((R + 128,), SENT8, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().f5k_layernorm_q8(_p(x), _p(scale), _p(shift), C.c_void_p(codes.data_ptr() + 64), C.c_void_p(scales.data_ptr() + 64),
                                            R, D, rows_per_batch, eps, m_limit, _lib.int_array(batch_of_row), _s()), "f5k_layernorm_q8")
    for t, n in ((codes, R * D), (scales, R)):
        assert (t[:64] == SENT8).all() and (t[64 + n:] == SENT8).all(), "guard bytes were written"
    return codes[64:64 + R * D].view(R, D).cpu(), scales[64:64 + R].cpu()


# =========================================================================================================== G1
def integer_operands(M, N, K):
    """A: integers in -8 .. 8 with, in each 32-element K block of each row, a marker 8 at a position that depends on (row, block);
    W: the asymmetric (7 n + 13 k + n k mod 5) mod 15 - 7; row and channel scales cycle over 2^-4 .. 2^4 (different periods)."""
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    A = ((m * 3 + k * 5 + (m * k) % 7) % 17 - 8).float()
    blk = torch.arange(K // 32)[None, :]
    A[torch.arange(M)[:, None].expand(M, K // 32), blk * 32 + (torch.arange(M)[:, None] * 5 + blk * 11) % 32] = 8.0
    n = torch.arange(N)[:, None]
    W = ((n * 7 + k * 13 + (n * k) % 5) % 15 - 7).float()
    sa = torch.exp2(((torch.arange(M) * 2) % 9 - 4).float())
    sw = torch.exp2(((torch.arange(N) * 5 + 3) % 9 - 4).float())
    bias = ((torch.arange(N) * 5) % 15 - 7).float()
    return (A * sa[:, None]).to(DEV), (W * sw[:, None]).to(DEV), bias.to(DEV)


def run_store_f8(A, W, b, *, cfg=-1, m_limit=-1, sixteen=False, act=0):
    M, N = A.shape[0], W.shape[0]
    out = Guarded((M, N), torch.float16 if sixteen else torch.float32)
    val, = k_gemm_epi("f8", A, W, b, STORE, [out], cfg=cfg, m_limit=m_limit, out16=sixteen, act=act)
    assert out.guards_intact()
    if m_limit >= 0:
        assert (out.bits[m_limit:] == out.sent).all(), "rows at or past m_limit were written"
    return out, val


@pytest.mark.parametrize("K", [128, 256, 1024])
def test_g1_lane_and_scale_map_exact(K):
    """Integer codes times power-of-two scales: the quantiser represents them exactly, every partial sum is an integer below 2^24 times
    one power of two, so the f32 result IS the float64 result.  A row <-> column swap, a lane map that differs between the two
    operands, a wrong K block and a scale applied to the wrong row or channel each change it."""
    for M in (1, 17, 129, 257):
        for N in (64, 192, 1024):
            A, W, b = integer_operands(M, N, K)
            ref = (A.double() @ W.double().t() + b.double()).float()
            assert torch.equal(ref.double(), A.double() @ W.double().t() + b.double()), "the reference itself is exact in f32"
            for cfg in F8_CFGS:
                for ml in (-1, max(M - 3, 0)):
                    _, val = run_store_f8(A, W, b, cfg=cfg, m_limit=ml)
                    rows = M if ml < 0 else ml
                    assert torch.equal(val[:rows], ref[:rows]), (M, N, K, cfg, ml)


def test_g1_remainder_launch():
    """8192 + 16 rows: the plan sends the 256-row multiple to the many-row tile and the last 16 rows to a remainder launch whose
    epilogue (and row scales) are addressed from row 8192 on."""
    M, N, K = 8192 + 16, 1024, 256
    plan = k_gemm_plan(1, M, N, K)
    assert plan == [(2, 13, 0, 8192), (2, 8, 8192, 16)], plan
    A, W, b = integer_operands(M, N, K)
    ref = (A.double() @ W.double().t() + b.double()).float()
    _, val = run_store_f8(A, W, b)
    assert torch.equal(val, ref)
    _, one = run_store_f8(A, W, b, cfg=8)
    assert torch.equal(one, ref)


# =========================================================================================================== G2
def quantiser_rows(R, D, seed):
    """Row magnitudes spanning 2^-10 .. 2^10 row by row (a per-tensor or per-tile amax would pass any end-to-end test and fails here),
    a zero row, a row whose amax is exactly 2^k * 448, a row whose largest element sits in the last real column."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, D, generator=g) * torch.exp2(torch.linspace(-10, 10, R))[:, None]
    if R >= 5:
        x[1] = 0.0
        x[2] = torch.randn(D, generator=g).clamp(-1, 1)
        x[2, D // 3] = 448.0 / 64
        x[3] = torch.randn(D, generator=g).clamp(-2, 2)
        x[3, D - 1] = -7.5
    return x.to(DEV)


@pytest.mark.parametrize("D", [256, 1024])
@pytest.mark.parametrize("R", [1, 5, 130])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_g2_row_quantiser_bit_for_bit(D, R, dtype):
    x = quantiser_rows(R, D, seed=R + D)
    if dtype == torch.float16:
        x = (x.clamp(-6.0e4, 6.0e4)).half()
    ref_c, ref_b = Q.quantise_rows(x.float().cpu())
    codes, scales = k_quant_rows(x)
    assert torch.equal(scales, ref_b), "scale bytes"
    assert torch.equal(codes, ref_c), "codes"
    if R > 1:   # a device row count below the rows: the tail is neither read nor written
        ml = R - 2
        codes, scales = k_quant_rows(x, m_limit=ml)
        assert torch.equal(codes[:ml], ref_c[:ml]) and torch.equal(scales[:ml], ref_b[:ml])
        assert (codes[ml:] == SENT8).all() and (scales[ml:] == SENT8).all()
    # pad columns: K real elements of rows of ld, written into rows of ldc; what lies past K is neither read (NaN) nor counted
    K = D - 64
    xp = x.clone()
    xp[:, K:] = float("nan")
    ref_c, ref_b = Q.quantise_rows(x.float().cpu(), K)
    codes, scales = k_quant_rows(xp, K=K, ldc=D)
    assert torch.equal(scales, ref_b) and torch.equal(codes[:, :K], ref_c)
    assert (codes[:, K:] == SENT8).all(), "columns past K were written"


def quantise_with_bytes(y, b):
    s = Q.scale_values(b)[:, None]
    return (y / s).clamp(-Q.E4M3_MAX, Q.E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def check_ln_codes(codes, scales, y, rows):
    """The fused LayerNorm's f32 value is not observable: compare with the restatement applied to f5k_layernorm_mod's f32 output y;
    a code may differ by one step only where y is within 1 ulp of a rounding boundary (at most 0.1 % of the elements), a scale byte only
    where the row's amax is within 1 ulp of a power-of-two boundary."""
    y, codes, scales = y[:rows].cpu(), codes[:rows], scales[:rows]
    ref_b = Q.scale_bytes(y)
    amax = y.abs().amax(-1, keepdim=True)
    up, dn = torch.nextafter(amax, torch.full_like(amax, float("inf"))), torch.nextafter(amax, torch.zeros_like(amax))
    ok_b = (scales == ref_b) | (scales == Q.scale_bytes(up)) | (scales == Q.scale_bytes(dn))
    assert ok_b.all(), f"scale bytes differ in rows {(~ok_b).nonzero().flatten().tolist()[:8]}"
    ref_c = quantise_with_bytes(y, scales)
    diff = codes != ref_c
    inf = torch.full_like(y, float("inf"))
    near = (codes == quantise_with_bytes(torch.nextafter(y, inf), scales)) | (codes == quantise_with_bytes(torch.nextafter(y, -inf), scales))
    assert (near | ~diff).all(), f"{int((diff & ~near).sum())} codes differ away from a rounding boundary"
    share = diff.float().mean().item()
    print(f"[ln q8] {int(diff.sum())} of {diff.numel()} codes on a rounding boundary ({share:.2e}); scale bytes off-restatement: {int((scales != ref_b).sum())}")
    assert share <= 1e-3


@pytest.mark.parametrize("D", [256, 1024])
@pytest.mark.parametrize("R,rpb", [(1, 1), (5, 5), (130, 65)])
def test_g2_layernorm_quantiser(D, R, rpb):
    x = quantiser_rows(R, D, seed=3 * R + D) + 0.25
    g = torch.Generator().manual_seed(D)
    nb = R // rpb
    scale, shift = (torch.randn(nb, D, generator=g) * 0.3).to(DEV), (torch.randn(nb, D, generator=g) * 0.3).to(DEV)
    y = k_layernorm_mod(x, scale, shift, rpb)
    codes, scales = k_layernorm_q8(x, scale, shift, rpb)
    check_ln_codes(codes, scales, y, R)
    if R > 1:
        ml = R - 2
        c2, s2 = k_layernorm_q8(x, scale, shift, rpb, m_limit=ml)
        assert torch.equal(c2[:ml], codes[:ml]) and torch.equal(s2[:ml], scales[:ml])
        assert (c2[ml:] == SENT8).all() and (s2[ml:] == SENT8).all(), "rows at or past m_limit were written"
        # the packed form: a row's vectors are those of its batch row in the map (here a permutation of the padded assignment)
        bor = [(r * 7 + 1) % nb for r in range(R)]
        xs = x
        yp = torch.empty_like(y)
        for bi in range(nb):
            idx = torch.tensor([r for r in range(R) if bor[r] == bi], device=DEV, dtype=torch.long)
            if len(idx):
                yp[idx] = k_layernorm_mod(xs[idx].contiguous(), scale[bi:bi + 1].contiguous(), shift[bi:bi + 1].contiguous(), len(idx))
        c3, s3 = k_layernorm_q8(x, scale, shift, rpb, batch_of_row=bor)
        check_ln_codes(c3, s3, yp, R)


# =========================================================================================================== G3
def dequantised64(X):
    """X as the quantiser left it (read back through f5k_quant_rows_e4m3), float64."""
    c, b = k_quant_rows(X)
    return Q.dequantise(c, b).double().to(DEV)


def check(val, ref, dt, label):
    assert torch.isfinite(val).all(), label
    if dt == torch.float32:
        e = rel_err(val, ref)
        print(f"[{label}] rel_err {e:.2e}")
        assert e < 2e-5, label
    else:
        u = ulp_dist(val, ref, dt)
        print(f"[{label}] max ulp {u}")
        assert u <= 1, label


@pytest.mark.parametrize("M,N,K", [(130, 192, 256), (257, 1024, 1024)])
def test_g3_store_and_gate_res_float64(M, N, K):
    # FF1's epilogue: GELU-tanh, f32 output on Gaussian operands, f16 output on lattice operands
    for sixteen in (False, True):
        A, W, b = random_operands(M, N, K, seed=M + N + sixteen, coarse=sixteen)
        ref = gelu_tanh64(dequantised64(A) @ dequantised64(W).t() + b.double())
        out, val = run_store_f8(A, W, b, sixteen=sixteen, act=1)
        check(val, ref, torch.float16 if sixteen else torch.float32, f"f8 store {M}x{N}x{K} f16={sixteen}")
        again, _ = run_store_f8(A, W, b, sixteen=sixteen, act=1)
        assert torch.equal(out.bits, again.bits), "two launches differ"
    # the residual epilogue: gates per batch row, ragged lens
    A, W, b = random_operands(M, N, K, seed=M + 7, coarse=False)
    rpb = 65
    nb = (M - 1) // rpb + 1
    g = torch.Generator().manual_seed(rpb)
    res = torch.randn(M, N, generator=g).to(DEV)
    gate = torch.randn(nb, N, generator=g).to(DEV)
    lens = [rpb if i == 0 else (rpb * (3 * i + 1)) // (3 * i + 4) for i in range(nb)]
    # (gate_res64 rounds its operands as `prec` would: the dequantised operands go in under a precision it leaves alone)
    ref = gate_res64("f32", dequantised64(A).float(), dequantised64(W).float(), b, res, gate, N, rpb, lens)
    bits = []
    for _ in range(2):
        x = Guarded.like(res)
        val, = k_gemm_epi("f8", A, W, b, GATE_RES, [x], res=x, gate=gate, gate_stride=N, rows_per_batch=rpb, lens=lens)
        assert x.guards_intact()
        bits.append(x.bits.clone())
    check(val, ref, torch.float32, f"f8 gate_res {M}x{N}x{K}")
    assert torch.equal(bits[0], bits[1]), "two launches differ"


def test_g3_qkv_packed_rows_float64():
    """H = 4, Nseq = 65, Npad = 72, packed rows (row_start): q / k / v^T in f16 within 1 ulp of float64 on lattice operands, positions
    past an utterance untouched."""
    H, Nseq, Npad, D = 4, 65, 72, 256
    lens = [65, 37, 50]
    Bp = len(lens)
    A, W, b = random_operands(Bp * Nseq, 3 * H * 64, D, seed=11, coarse=True)
    cs, sn = rotary_tables(Nseq + 3, True)
    rs = packed(lens, Nseq)
    Ap = torch.zeros(rs[-1] + 8, D, device=DEV)
    for i in range(Bp):
        n = min(rs[i + 1] - rs[i], Nseq)
        Ap[rs[i]:rs[i] + n] = A[i * Nseq:i * Nseq + n]
    ref = qkv64(dequantised64(A) @ dequantised64(W).t() + b.double(), Bp, Nseq, H, 1, 0.125, cs, sn)
    runs = []
    for _ in range(2):
        outs = [Guarded((Bp, H, Nseq, 64), torch.float16), Guarded((Bp, H, Nseq, 64), torch.float16), Guarded((Bp, H, 64, Npad), torch.float16)]
        vals = k_gemm_epi("f8", Ap, W, b, QKV, outs, H=H, Nseq=Nseq, Npad=Npad, pe_heads=1, q_scale=0.125, rope_cos=cs, rope_sin=sn,
                          row_start=rs, Bp=Bp)
        for o in outs:
            assert o.guards_intact()
        runs.append([o.bits.clone() for o in outs])
    for i in range(Bp):
        cnt = min(rs[i + 1] - rs[i], Nseq)
        for name, v, r, o in zip("q k".split(), vals, ref, outs):
            check(v[i, :, :cnt], r[i, :, :cnt], torch.float16, f"f8 qkv {name} item {i}")
            assert (o.bits[i, :, cnt:] == o.sent).all(), (name, i, "written past the utterance")
        check(vals[2][i, ..., :cnt], ref[2][i, ..., :cnt], torch.float16, f"f8 qkv vt item {i}")
        assert (outs[2].bits[i, ..., cnt:] == outs[2].sent).all(), ("vt", i, "written past the utterance")
    assert all(torch.equal(x, y) for x, y in zip(*runs)), "two launches differ"
