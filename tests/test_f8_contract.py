"""CPU: the f8 precision (F5_PREC_F8, include/f5_hip.h) where no GPU is needed -- the torch restatement of its quantiser
(tests/f8_oracle.py), f5_create's refusals, launch_gemm's plan at element size 1 (f5k_gemm_plan) and the Python surface."""
import ctypes as C
import json
import os

import pytest
import torch

import f5_tts_amd as P
from f5_tts_amd import _lib
from gpu_util import k_gemm_plan

import f8_oracle as Q

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------ the quantiser restatement
def rows_spanning_magnitudes(R=64, K=192, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, K, generator=g) * torch.exp2(torch.linspace(-10, 10, R))[:, None]
    x[3] = 0.0                                  # a zero row
    x[5] = torch.randn(K, generator=g).clamp(-1, 1) * 0.5
    x[5, 17] = 448.0 * 2.0 ** -3                # amax exactly a power of two times 448
    x[7] = torch.randn(K, generator=g).clamp(-2, 2)
    x[7, K - 1] = -9.0                          # the largest element in the last real column
    return x


def test_scale_rule_and_half_step_error():
    x = rows_spanning_magnitudes()
    codes, b = Q.quantise_rows(x)
    s = Q.scale_values(b)
    amax = x.abs().amax(-1)
    nz = amax > 0
    r = amax[nz] / s[nz]
    assert (r > 224).all() and (r <= 448).all(), "amax / s lies in (224, 448]"
    assert b[3].item() == 127 and (codes[3] == 0).all(), "a zero row: byte 127, zero codes"
    assert (amax[5] / s[5]).item() == 448.0, "an amax of 2^k * 448 sits on the upper end of its scale"
    y = x / s[:, None]
    deq = Q.dequantise(codes, b)
    assert torch.isfinite(deq).all()
    err = (deq / s[:, None] - y).abs()
    assert (err <= Q.e4m3_step(y) / 2).all(), "dequantised codes are within half an e4m3 step of x"
    assert torch.equal(Q.fake_quant(deq), deq), "quantising is idempotent"


def test_row_scale_ignores_pad_columns():
    x = rows_spanning_magnitudes(R=16, K=128)
    padded = torch.cat((x, torch.full((16, 64), 1.0e6)), dim=1)
    c0, b0 = Q.quantise_rows(x)
    c1, b1 = Q.quantise_rows(padded, K=128)
    assert torch.equal(b0, b1) and torch.equal(c0, c1)
    assert not torch.equal(Q.scale_bytes(padded), b0)


def test_rounding_is_nearest_even_and_saturating():
    # e4m3 between 16 and 32 has step 2: 17 -> 16 (tie to even mantissa), 19 -> 20, 500 saturates at 448
    x = torch.tensor([[17.0, 19.0, 21.0, 448.0, 0.0, -17.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10]])
    c, b = Q.quantise_rows(x)
    assert b.item() == 127
    assert Q.dequantise(c, b)[0].tolist() == [16.0, 20.0, 20.0, 448.0, 0.0, -16.0, 2.0 ** -9, 0.0, 2.0 ** -8]
    y = torch.tensor([500.0, -1000.0]).clamp(-Q.E4M3_MAX, Q.E4M3_MAX).to(torch.float8_e4m3fn).float()
    assert y.tolist() == [448.0, -448.0]


# ------------------------------------------------------------------------------------------------ f5_create refusals
def f8_config(backbone=_lib.F5_BACKBONE_DIT, heads=4, ff_dim=512, options=0):
    cfg = _lib.f5_config()
    cfg.backbone, cfg.precision = backbone, _lib.F5_PREC_F8
    cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.ff_dim = 256, 2, heads, 64, ff_dim
    cfg.text_dim, cfg.conv_layers, cfg.pe_attn_head, cfg.text_num_embeds, cfg.mel_dim, cfg.max_pos = 64, 2, -1, 40, 100, 4096
    cfg.text_mask_padding = 1
    cfg.options = options
    return cfg


@pytest.mark.parametrize("kw,words", [
    (dict(backbone=_lib.F5_BACKBONE_UNETT), [b"F5_PREC_F8", b"DiT backbone", b"UNetT"]),
    (dict(backbone=_lib.F5_BACKBONE_MMDIT), [b"F5_PREC_F8", b"DiT backbone", b"MMDiT"]),
    (dict(options=_lib.F5_OPT_ADAPTERS), [b"F5_PREC_F8", b"F5_OPT_ADAPTERS"]),
    (dict(heads=3), [b"F5_PREC_F8", b"128", b"heads"]),
    (dict(ff_dim=576), [b"F5_PREC_F8", b"128", b"ff_dim"]),
])
def test_create_refuses_by_name(kw, words):
    lib = _lib.load()
    h = C.c_void_p()
    cfg = f8_config(**kw)
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == -1
    msg = lib.f5_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_create_accepts_the_plain_dit():
    lib = _lib.load()
    h = C.c_void_p()
    for opts in (0, _lib.F5_OPT_QK_RMSNORM | _lib.F5_OPT_LONG_SKIP):
        cfg = f8_config(options=opts)
        assert lib.f5_create(C.byref(cfg), C.byref(h)) == 0, lib.f5_last_error()
        assert lib.f5_destroy(h) == 0


# ------------------------------------------------------------------------------------------ the plan at element size 1
F8_TILES = {2: (128, 128), 8: (64, 64), 13: (256, 128)}


@pytest.mark.parametrize("M,N,K", [(2048, 3072, 1024), (32784, 1024, 2048), (1, 1024, 1024)])
@pytest.mark.parametrize("ml", [0, 1])
def test_plan_exists_at_element_size_one(M, N, K, ml):
    plan = k_gemm_plan(1, M, N, K, has_m_limit=ml, m_hint=M if ml else 0)
    assert plan, (M, N, K, ml)
    rows = 0
    for fam, tile, row0, cnt in plan:
        assert fam == 2 and tile in F8_TILES, "e4m3 operands run on their LDS-DMA ring tiles"
        assert row0 == rows
        rows += cnt
    assert rows == M
    if M == 32784 and not ml:
        assert plan == [(2, 13, 0, 32768), (2, 8, 32768, 16)], "the 16 rows past a multiple of 256 go to a remainder launch"
    if ml:
        assert len(plan) == 1, "no remainder split behind a device row count"
    if M == 1:
        assert plan == [(2, 8, 0, 1)]


def test_plan_refusals_at_element_size_one():
    assert k_gemm_plan(1, 256, 256, 192) is None, "K must be whole 128-code tiles"
    assert k_gemm_plan(1, 256, 256, 128), "a single K step is a plan"
    assert k_gemm_plan(1, 256, 256, 256, form=1) is None and k_gemm_plan(1, 256, 256, 256, form=2) is None
    assert k_gemm_plan(1, 256, 256, 256, conv=1) is None
    assert k_gemm_plan(1, 256, 256, 256, force_cfg=-2) is None, "no register-staged kernel"
    for cfg in (20, 9, 10, 128128):
        assert k_gemm_plan(1, 256, 256, 256, force_cfg=cfg) is None, cfg
    for cfg in F8_TILES:
        assert k_gemm_plan(1, 300, 256, 256, force_cfg=cfg) == [(2, cfg, 0, 300)]
    assert k_gemm_plan(1, 0, 256, 256) == []


def test_plans_of_sizes_two_and_four_unchanged():
    """A handful of the plans tests/test_gemm_plan.py pins (tests/golden/gemm_plan.json), asserted again."""
    with open(os.path.join(GOLDEN, "gemm_plan.json")) as fh:
        rows = json.load(fh)
    picked = rows[:: max(1, len(rows) // 40)]
    assert len(picked) >= 20 and {r[0] for r in picked} <= {2, 4}
    for r in picked:
        args, n, launches = r[:12], r[12], r[13:]
        plan = k_gemm_plan(*args)
        if n < 0:
            assert plan is None, r
        else:
            assert plan == [tuple(launches[4 * i:4 * i + 4]) for i in range(n)], r
    # and the shapes of the four block GEMMs at Base dims, stated
    assert k_gemm_plan(2, 2048, 3072, 1024) == [(2, 10, 0, 2048)]
    assert k_gemm_plan(2, 32768, 1024, 2048) == [(3, 20, 0, 32768)]
    assert k_gemm_plan(2, 16400, 1024, 1024) == [(3, 20, 0, 16384), (2, 8, 16384, 16)]
    assert k_gemm_plan(4, 2048, 1024, 1024, form=2) == [(2, 8, 0, 2048)]


# ---------------------------------------------------------------------------------------------------- Python surface
def test_python_surface():
    assert _lib.F5_PREC_F8 == 5 and _lib.PRECISIONS["f8"] == 5 and _lib.PRECISIONS["fp8"] == 5
    m = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100, precision="f8")
    assert m.precision == "f8"
    assert P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100, precision="fp8").precision == "f8"
    assert P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100).precision == "f16p", "the default stays f16p"
    e2 = dict(dim=256, depth=4, heads=4, dim_head=64, ff_mult=2, text_mask_padding=False, pe_attn_head=1)
    mm = dict(dim=256, depth=2, heads=4, dim_head=64, ff_mult=2)
    for cls, arch in ((P.UNetT, e2), (P.MMDiT, mm)):
        with pytest.raises(NotImplementedError, match="DiT"):
            cls(**arch, text_num_embeds=40, mel_dim=100, precision="f8")
    m.init_synthetic()
    with pytest.raises(NotImplementedError, match="f8"):
        m.add_adapter("a", {})
    with pytest.raises(ValueError):
        P.BigVGAN(precision="f8")
    loaded = P.infer.load_model(P.DiT, dict(P.config.F5TTS_TINY), None, device="cpu", precision="f8")
    assert loaded.transformer.precision == "f8"
    with pytest.raises(NotImplementedError, match="f8"):
        P.infer.load_adapter(loaded, os.path.join(GOLDEN, "no_such_adapter.pt"), "a")
