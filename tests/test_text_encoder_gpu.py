"""GPU: the text encoder -- text_embed_kernel, dwconv7_ln_kernel, grn_partial_kernel / grn_apply_kernel,
zero_filler_rows_kernel / zero_tail_rows_kernel, text_avg_upsample_kernel (csrc/elementwise.h) and the two float GEMMs of
run_text_embed with their GELU-erf and residual epilogues (csrc/engine_impl.h) -- through Engine.text_embed (f5_text_embed),
against the float64 reference of tests/text_oracle.py, on weights that make every term count (tests/text_cases.py).

Every case runs with drop_text False and True at precision "f32".  The bound is computed per run, not chosen: 8 x the
float32 CPU oracle's own L-inf error against float64 on the same inputs, floored at 4 ulp of float32 at the output's
largest magnitude (text_cases.bound).  Rows past a DiT sample's length, and the rows of a sample without a valid token
under average upsampling, must be exactly zero.  tests/test_text_encoder.py shows on the CPU that eleven deliberate errors
of the reference each leave these bounds by a factor of 20 or more.

Measured on the MI355X (L-inf against float64; `oracle32` is the float32 CPU oracle's error on the same inputs):

    case             drop_text   kernel      bound       oracle32    max|ref|
    d64_l2_nomask    0           3.363e-06   2.910e-05   3.637e-06   8.31
    d64_l2_nomask    1           3.927e-06   4.159e-05   5.198e-06   9.33
    d64_l2_mask      0           2.039e-06   1.732e-05   2.165e-06   6.89
    d64_l2_mask      1           2.225e-06   2.436e-05   3.045e-06   6.65
    d64_l4_fillers   0           4.405e-06   4.559e-05   5.698e-06   9.39
    d64_l4_fillers   1           5.663e-06   4.990e-05   6.238e-06   9.22
    d100_l1_trunc    0           4.109e-06   2.810e-05   3.513e-06   6.47
    d100_l1_trunc    1           3.810e-06   2.665e-05   3.331e-06   6.67
    d512_l4          0           1.656e-05   7.743e-05   9.679e-06   12.25
    d512_l4          1           1.807e-05   8.532e-05   1.067e-05   13.97
    d512_l4_up       0           1.379e-05   6.783e-05   8.478e-06   12.24
    d512_l4_up       1           1.807e-05   8.532e-05   1.067e-05   13.97
    d1024_l1         0           7.481e-06   2.017e-05   2.522e-06   6.38
    d1024_l1         1           1.214e-05   1.833e-05   2.291e-06   9.07
    d2048_l1         0           1.060e-05   1.729e-05   2.161e-06   7.18
    d2048_l1         1           1.506e-05   2.045e-05   2.556e-06   7.73
    d64_l0           0           0.000e+00   9.537e-07   0.000e+00   3.38
    d64_l0           1           0.000e+00   9.537e-07   0.000e+00   3.38
    up_ratios        0           2.688e-06   1.809e-05   2.261e-06   7.65
    up_ratios        1           4.000e-06   2.628e-05   3.284e-06   7.16
    up_rem2          0           2.980e-06   2.384e-05   2.980e-06   6.51
    up_rem2          1           2.001e-06   2.287e-05   2.858e-06   5.40
    up_all_filler    0           2.141e-06   1.622e-05   2.027e-06   6.70
    up_all_filler    1           2.289e-06   2.061e-05   2.577e-06   5.38
    u64_l2           0           2.372e-06   2.897e-05   3.622e-06   8.79
    u64_l2           1           2.225e-06   2.436e-05   3.045e-06   6.65
    u64_l1_clamp     0           1.690e-04   1.352e-03   1.690e-04   9.36
    u64_l1_clamp     1           1.685e-04   1.355e-03   1.694e-04   9.42

Reading the table.  The kernels are deterministic; `oracle32`, and with it the bound, moves by up to 50 % with the host's CPU
BLAS (its summation order).  At text_dim <= 512 the kernels are at 0.6 - 1.8 x the CPU oracle's own error.  At
text_dim 1024 and 2048 (GEMMs of K = 1024 .. 4096) they are at 3 - 6 x of it and use up to 0.74 of the bound: the float GEMM
adds K / 4 products into one accumulator in sequence, the CPU BLAS into many short ones -- sqrt(K)-ish growth, the
summation order the factor 8 is there for, not an error of the kernels.  u64_l1_clamp: both float32 paths share the
float32 position table, which is up to 1.5e-4 from float64's by row 4095; that is nearly the whole error there.  d64_l0 (no conv
layers) is a gather: exact.  No case was left out and no kernel bug was found.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import text_cases as T  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd.engine import Engine  # noqa: E402

DEV = "cuda:0"
F5_EINVAL = -1
_ENGINES: dict = {}


def engine_for(case, precision="f32", **kw):
    """One engine per (weights, precision), kept for the module (the text_dim = 2048 one is the heaviest)."""
    k = (case.key, precision, tuple(sorted(kw.items())))
    if k not in _ENGINES:
        e = Engine(case.arch, T.NV, backbone=case.backbone, precision=precision, device=DEV, **kw)
        e.load_state_dict(T.weights_for(case.key))
        _ENGINES[k] = e
    return _ENGINES[k]


def run(case, drop_text, precision="f32", lens="case", rows=None):
    text = T.text_for(case)
    lens = case.lens if lens == "case" else lens
    if rows is not None:
        text = text[rows]
        lens = None if lens is None else [lens[b] for b in rows]
    out = engine_for(case, precision).text_embed(text, case.N, lens=None if lens is None else list(lens), drop_text=drop_text)
    torch.cuda.synchronize()
    return out.cpu()


def past_length(case):
    """bool[B, N, 1]: rows the DiT leaves zero (n >= lens[b])."""
    lens = torch.tensor(case.lens if (case.lens is not None and case.backbone == "DiT") else [case.N] * case.B)
    return (torch.arange(case.N)[None, :] >= lens[:, None])[..., None]


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_text_embed_vs_float64(name):
    c = T.CASE[name]
    for drop in (False, True):
        out, ref = run(c, drop), T.reference(name, drop)
        bound, e32, top = T.bound(name, drop)
        err = (out.double() - ref).abs().max().item()
        print(f"[text f64] {name:15s} drop_text={int(drop)}  kernel {err:.3e}  bound {bound:.3e}  oracle32 {e32:.3e}  max|ref| {top:.2f}")
        assert torch.isfinite(out).all() and err <= bound
        assert not out[past_length(c).expand_as(out)].any(), "rows past a sample's length must be exactly zero"
        if c.upsample:
            text = T.text_for(c)
            for b in range(c.B):
                L = c.N if c.lens is None else c.lens[b]
                if not (text[b, :min(c.nt, L)] != -1).any():
                    assert not out[b].any(), "a sample without a valid token must come out as exact zeros"
        if c.mask_padding and c.layers and not c.upsample:
            filler = torch.ones(c.B, c.N, dtype=torch.bool)
            filler[:, :min(c.nt, c.N)] = T.text_for(c)[:, :c.N] == -1
            assert not out[filler].any(), "text_mask_padding: filler rows must be exactly zero (also under drop_text)"


def test_unett_clamps_the_position_row_at_4095():
    """Rows 4095 .. 4099 (all filler ids, rows not zeroed) against the reference with position row min(n, 4095); the same
    reference without the clamp is 1.96 away in rows 4096 .. 4099: three orders above the bound."""
    c = T.CASE["u64_l1_clamp"]
    for drop in (False, True):
        out, ref = run(c, drop), T.reference(c.name, drop)
        err = (out.double() - ref)[:, 4090:].abs().max().item()
        print(f"[text f64] {c.name} drop_text={int(drop)} rows 4090..4099: kernel {err:.3e}  bound {T.bound(c.name, drop)[0]:.3e}")
        assert err <= T.bound(c.name, drop)[0]
        unclamped = T.reference(c.name, drop, "unett_pos_not_clamped")
        assert (unclamped - ref)[:, 4096:].abs().max() > 100 * T.bound(c.name, drop)[0]


def test_unett_embeds_at_the_padded_length_whatever_lens_says():
    c = T.CASE["u64_l2"]
    for drop in (False, True):
        assert torch.equal(run(c, drop), run(c, drop, lens=None))


@pytest.mark.parametrize("name,precision", [("d64_l4_fillers", "f16p"), ("d512_l4_up", "bf16")])
def test_text_path_does_not_depend_on_the_backbone_precision(name, precision):
    c = T.CASE[name]
    for drop in (False, True):
        assert torch.equal(run(c, drop, precision), run(c, drop)), f"{precision} text embedding differs from the f32 engine's"


@pytest.mark.parametrize("name", ["d64_l4_fillers", "d512_l4_up", "d100_l1_trunc", "up_ratios", "u64_l2"])
def test_deterministic_and_per_sample(name):
    """Two calls are bit-equal, and batch row b alone gives row b of the batch call: the GRN reduces per sample and must
    not see its neighbours (nor may any GEMM tile choice that depends on the row count change a sum's order)."""
    c = T.CASE[name]
    for drop in (False, True):
        a = run(c, drop)
        assert torch.equal(a, run(c, drop))
        for b in range(c.B):
            assert torch.equal(run(c, drop, rows=[b])[0], a[b]), f"sample {b} alone differs from row {b} of the batch"


# ------------------------------------------------------------------------------------------------------- refusals
def test_refuses_n_past_the_text_position_table():
    """DiT with conv layers: N one above the rows of aux.text_pos (8192) is refused before anything is launched.  (The
    engine is made with a longer rotary table, so that the rotary check of every entry point does not answer first.)"""
    c = T.CASE["d64_l2_mask"]
    e = engine_for(c, max_pos=16384)
    host_text = T.text_for(c)[:1]
    text = host_text.to(DEV)
    N = 8192 + 1
    out = torch.full((1, N, 64), 7.0, device=DEV)
    args = (e._h, C.c_void_p(text.data_ptr()), 1, c.nt, None, N, 0, C.c_void_p(out.data_ptr()),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = e.lib.f5_text_embed(*args)
    msg = e.lib.f5_last_error().decode()
    assert rc == F5_EINVAL and msg == f"N={N} exceeds aux.text_pos rows", (rc, msg)
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call must not write its output"
    with pytest.raises(_lib.F5Error, match="exceeds aux.text_pos rows"):
        e.text_embed(host_text, N)
    ok = e.text_embed(host_text, 8192)          # the last length the table covers still runs
    assert torch.isfinite(ok).all()


def test_refuses_average_upsampling_without_mask_padding():
    arch = dict(T.CASE["up_rem2"].arch, text_mask_padding=False)
    with pytest.raises(AssertionError, match="requires text_mask_padding"):
        Engine(arch, T.NV, device=DEV)
    a = P.config.normalize_arch(arch)
    cfg = _lib.f5_config()
    cfg.backbone, cfg.precision = _lib.F5_BACKBONE_DIT, _lib.F5_PREC_F32
    cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.ff_dim = a["dim"], a["depth"], a["heads"], a["dim_head"], a["dim"] * a["ff_mult"]
    cfg.text_dim, cfg.conv_layers, cfg.pe_attn_head = a["text_dim"], a["conv_layers"], -1
    cfg.text_mask_padding, cfg.attn_mask_enabled = 0, 0
    cfg.text_num_embeds, cfg.mel_dim, cfg.max_pos = T.NV, 100, 8192
    cfg.options = _lib.F5_OPT_TEXT_AVG_UPSAMPLE
    lib, h = _lib.load(), C.c_void_p()
    rc = lib.f5_create(C.byref(cfg), C.byref(h))
    msg = lib.f5_last_error().decode()
    assert rc == F5_EINVAL and not h.value and msg.startswith("text_embedding_average_upsampling requires text_mask_padding to be True"), (rc, msg)
    cfg.text_mask_padding = 1                       # the same configuration with the mask on is accepted
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == 0 and h.value
    assert lib.f5_destroy(h) == 0
