"""CPU: the MMDiT backbone's host side -- state-dict layout, the float64 oracle (tests/mmdit_oracle.py) against the live reference
and the reference-generated fixtures (tools/make_mmdit_golden.py), the fixtures' text-sensitivity condition, constructor validation
and every refusal that needs no GPU (Python level, and f5_create at the C level)."""
import ctypes as C
import importlib

import pytest
import torch

import f5_tts_amd as P
import mmdit_oracle as MO
from conftest import load_golden
from mmdit_cases import SAMPLE_FIXTURES, mmdit_weights, sample_kwargs
from f5_tts_amd import _lib
from oracle import ref_harness as rh

ARCH = dict(dim=256, depth=3, heads=4, dim_head=64, ff_mult=2, text_mask_padding=True, qk_norm=None)
needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")


# ------------------------------------------------------------------------------------------------ state dict
@needs_reference
@pytest.mark.parametrize("arch", [ARCH, dict(ARCH, depth=2, qk_norm="rms_norm", text_mask_padding=False), dict(ARCH, depth=1, heads=8, ff_mult=4)])
def test_param_shapes_equal_the_live_reference_state_dict(arch):
    rh.load()
    ref = importlib.import_module("f5_tts.model.backbones.mmdit").MMDiT(**arch, text_num_embeds=40, mel_dim=100)
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = P.weights.mmdit_param_shapes(arch, 40)
    assert got == want and list(got) == list(want)
    assert not any("freqs_cis" in k for k in got)


# ---------------------------------------------------------------------------------------------------- oracle
@needs_reference
def test_oracle_matches_the_live_reference():
    """One cfg_infer forward and one ragged sample() of the reference's own module, on fresh inputs (bar of test_oracle_*: 5e-5)."""
    ref = rh.load()
    arch = dict(ARCH, qk_norm="rms_norm")
    sd = P.weights.synthetic_state_dict(P.weights.mmdit_param_shapes(arch, 40), seed=3, std=0.06)
    tr = importlib.import_module("f5_tts.model.backbones.mmdit").MMDiT(**arch, text_num_embeds=40, mel_dim=100)
    tr.load_state_dict(sd, strict=True)
    model = ref.CFM(transformer=tr, mel_spec_module=rh.InertMelSpec()).eval()
    g = torch.Generator().manual_seed(5)
    x, cond = torch.randn(2, 29, 100, generator=g), torch.randn(2, 29, 100, generator=g)
    text = torch.randint(0, 40, (2, 7), generator=g)
    text[1, 4:] = -1
    mask = torch.arange(29)[None] < torch.tensor([29, 18])[:, None]
    with torch.no_grad():
        want = tr(x=x, cond=cond, text=text, time=torch.tensor(0.41), mask=mask, cfg_infer=True, cache=False)
    got = MO.forward(sd, arch, x, cond, text, torch.tensor(0.41), mask, cfg_infer=True)
    e = (got - want).abs().max().item()
    print(f"[oracle vs live reference] forward Linf {e:.3e} (|out| <= {want.abs().max().item():.2f})")
    assert e <= 5e-5
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=11, lens=torch.tensor([12, 9]))
    w_out, w_traj = model.sample(cond[:, :12], text, torch.tensor([29, 18]), **kw)
    o_out, o_traj = MO.sample(sd, arch, cond[:, :12], text, torch.tensor([29, 18]), **kw)
    e = (o_traj - w_traj).abs().max().item()
    print(f"[oracle vs live reference] sample traj Linf {e:.3e}")
    assert e <= 5e-5 and (o_out - w_out).abs().max().item() <= 5e-5


@pytest.mark.parametrize("name", SAMPLE_FIXTURES)
def test_oracle_matches_the_sample_fixtures(name):
    meta, a = load_golden(name)
    sd = mmdit_weights(meta)
    dur, kw = sample_kwargs(meta, a)
    out, traj = MO.sample(sd, meta["arch"], a["cond"], a["text"], dur, **kw)
    e_out, e_traj = (out - a["out"]).abs().max().item(), (traj - a["traj"]).abs().max().item()
    print(f"[oracle vs fixture] {name}: out Linf {e_out:.3e} traj Linf {e_traj:.3e}")
    assert e_out <= 2e-5 and e_traj <= 2e-5


def test_oracle_matches_the_forward_taps():
    meta, a = load_golden("mmdit_forward_taps")
    for part in ("_x0", "_x1"):
        a.update(load_golden("mmdit_forward_taps" + part)[1])
    sd = mmdit_weights(meta)
    taps = {}
    out = MO.forward(sd, meta["arch"], a["x"], a["cond"], a["text"], a["time"], a["mask"], cfg_infer=True, taps=taps)
    assert (out - a["out"]).abs().max().item() <= 2e-5
    names = ["text_cond", "text_uncond", "audio_embed", "block0_c", "block0_x", "block1_c", "block1_x", "block2_x"]
    assert "block2_c" not in a and "block2_c" not in taps, "the last block is context_pre_only: its c is dropped"
    for k in names:
        e = (taps[k].float() - a[k]).abs().max().item()
        assert e <= 2e-5 * max(1.0, a[k].abs().max().item()), f"{k}: {e:.3e}"


# ----------------------------------------------------------------------------------- the sensitivity condition
@pytest.mark.parametrize("name", SAMPLE_FIXTURES)
def test_fixtures_hear_the_text_stream(name):
    """Replacing one token of item 0, and reversing item 0's valid tokens, each move the reference's `out` by at least 2e-2
    (20 x the parity bar): an engine that ignored the text stream, its order or its rotary positions could not pass the parity tests."""
    meta, a = load_golden(name)
    assert meta["sensitivity"] == 2e-2 and meta["std"] > 0.02
    assert not torch.equal(a["text_token"], a["text"]) and not torch.equal(a["text_order"], a["text"])
    assert (a["text_token"] != a["text"]).sum() == 1 and torch.equal(a["text_token"][1:], a["text"][1:])
    n0 = int((a["text"][0] != -1).sum())
    assert torch.equal(a["text_order"][0, :n0], a["text"][0, :n0].flip(0)) and torch.equal(a["text_order"][1:], a["text"][1:])
    d_tok, d_ord = (a["out_token"] - a["out"]).abs().max().item(), (a["out_order"] - a["out"]).abs().max().item()
    print(f"[sensitivity] {name}: one token {d_tok:.3e}, reversed order {d_ord:.3e}")
    assert d_tok >= 2e-2 and d_ord >= 2e-2


# ------------------------------------------------------------------------------- constructor and refusals (no GPU)
def test_constructor_takes_the_reference_keywords_and_validates():
    m = P.MMDiT(dim=256, depth=3, heads=4, dim_head=64, dropout=0.1, ff_mult=2, mel_dim=100, text_num_embeds=40,
                text_mask_padding=True, qk_norm=None)
    assert m.dim == 256 and m.depth == 3 and m.backbone_name == "MMDiT" and m.precision in ("f16p", "f16x3")
    assert m.param_shapes() == P.weights.mmdit_param_shapes(ARCH, 40)
    m.init_synthetic()
    assert set(m.state_dict()) == set(m.param_shapes()) and m.clear_cache() is None
    import f5_tts_amd
    assert f5_tts_amd.MMDiT is P.backbones.MMDiT and "MMDiT" in P.__all__
    with pytest.raises(ValueError, match="qk_norm"):
        P.MMDiT(dim=256, qk_norm="layer_norm")
    with pytest.raises(ValueError, match="dim_head"):
        P.MMDiT(dim=256, dim_head=32)
    with pytest.raises(RuntimeError, match="only runs on a GPU"):
        m.forward(torch.zeros(1, 8, 100), torch.zeros(1, 8, 100), torch.zeros(1, 3, dtype=torch.long), torch.tensor(0.5))


def test_packed_row_features_and_adapters_are_refused():
    m = P.MMDiT(**ARCH, text_num_embeds=40).init_synthetic()
    with pytest.raises(NotImplementedError, match="length buckets are built for the DiT backbone only"):
        m.set_length_buckets(64)
    with pytest.raises(NotImplementedError, match="isolated rows run on packed rows"):
        m.set_isolated_rows(True)
    with pytest.raises(NotImplementedError, match="length buckets are built for the DiT backbone only"):
        m.prepare_sample(1, 64, 128, 16, 4, 2.0)
    with pytest.raises(NotImplementedError, match="resident adapters are built for the DiT backbone only"):
        m.add_adapter("a", {})
    model = P.CFM(transformer=m, mel_spec_module=P.mel.MelSpec())
    cond, text = torch.zeros(1, 8, 100), torch.zeros(1, 3, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="MMDiT"):
        model.sample_items(cond, text, 20, steps=[4])
    with pytest.raises(NotImplementedError, match="MMDiT"):
        model.sample_span(cond, text, 20, steps=[4], start=[0], count=2)


def test_load_model_accepts_the_class():
    model = P.infer.load_model(P.MMDiT, dict(ARCH), None, device="cpu")
    assert isinstance(model.transformer, P.backbones.MMDiT) and model.transformer.text_num_embeds == 257


def _config(options=0):
    cfg = _lib.f5_config()
    cfg.backbone, cfg.precision = _lib.F5_BACKBONE_MMDIT, _lib.F5_PREC_F32
    cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.ff_dim = 256, 3, 4, 64, 512
    cfg.text_dim, cfg.mel_dim, cfg.text_num_embeds, cfg.text_mask_padding, cfg.max_pos = 256, 100, 40, 1, 4096
    cfg.pe_attn_head, cfg.options = -1, options
    return cfg


@pytest.mark.parametrize("option,reason", [(_lib.F5_OPT_LONG_SKIP, b"long skip"), (_lib.F5_OPT_TEXT_AVG_UPSAMPLE, b"stretch"),
                                           (_lib.F5_OPT_ADAPTERS, b"adapters")])
def test_f5_create_refuses_the_dit_only_options(option, reason):
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _config(option)
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == -1
    err = lib.f5_last_error()
    assert b"MMDiT" in err and reason in err


def test_f5_create_accepts_the_backbone_and_refuses_split_cfg(monkeypatch):
    lib = _lib.load()
    h = C.c_void_p()
    for options in (0, _lib.F5_OPT_QK_RMSNORM):
        cfg = _config(options)
        assert lib.f5_create(C.byref(cfg), C.byref(h)) == 0, lib.f5_last_error()
        # the packed-row switches are refused with the backbone's name; nothing was finalized, nothing is launched
        assert lib.f5_set_length_buckets(h, 64) == -1 and b"MMDiT" in lib.f5_last_error()
        assert lib.f5_set_length_buckets(h, 0) == 0
        assert lib.f5_set_isolated_rows(h, 1) == -1 and b"MMDiT" in lib.f5_last_error()
        assert lib.f5_set_isolated_rows(h, 0) == 0
        a = C.c_void_p()
        assert lib.f5_adapter_create(h, C.byref(a)) != 0 and b"MMDiT" in lib.f5_last_error()
        assert lib.f5_destroy(h) == 0
    monkeypatch.setenv("F5_SPLIT_CFG", "1")
    cfg = _config()
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == -1
    assert b"MMDiT" in lib.f5_last_error() and b"F5_SPLIT_CFG" in lib.f5_last_error()
