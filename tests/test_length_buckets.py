"""CPU: the plumbing of length-bucketed sample() graphs -- bucket arithmetic, the Python switches, the UNetT refusal and the
argument checks of the C entry points that need no GPU."""
import ctypes as C

import pytest

import f5_tts_amd as P
from f5_tts_amd import _lib, backbones, infer


def tiny_config(backbone=_lib.F5_BACKBONE_DIT):
    cfg = _lib.f5_config()
    cfg.backbone, cfg.precision = backbone, _lib.F5_PREC_F16P
    cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.ff_dim = 256, 2, 4, 64, 512
    cfg.text_dim, cfg.conv_layers, cfg.pe_attn_head, cfg.text_num_embeds, cfg.mel_dim, cfg.max_pos = 64, 2, -1, 40, 100, 4096
    return cfg


def test_bucket_arithmetic():
    assert [backbones.bucket_ceiling(n, 32) for n in (1, 32, 33, 63, 64, 65, 96)] == [32, 32, 64, 64, 64, 96, 96]
    assert backbones.bucket_ceiling(777, 0) == 777
    assert backbones.bucket_ceiling(1000, 64) == 1024 and backbones.bucket_ceiling(1024, 1024) == 1024
    for g in (0, 8, 32, 48, 64, 1024):
        assert backbones.valid_length_bucket(g)
    for g in (-8, 1, 4, 12, 100, 1032, 2048):
        assert not backbones.valid_length_bucket(g)


def test_engine_checks_the_granule_without_a_gpu():
    lib = _lib.load()
    h = C.c_void_p()
    cfg = tiny_config()
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == 0
    try:
        for g in (0, 8, 32, 1024, 0):
            assert lib.f5_set_length_buckets(h, g) == 0
        for g in (12, 2048, -8, 4):
            assert lib.f5_set_length_buckets(h, g) == -1 and str(g).encode() in lib.f5_last_error()       # F5_EINVAL
        assert lib.f5_set_length_buckets(None, 32) == -1
        # not finalized: F5_ESTATE, whatever the switch says
        assert lib.f5_prepare_sample(h, 1, 33, 96, 40, 3, 2.0, 0, 1, None) == -3 and b"f5_finalize" in lib.f5_last_error()
        out = (C.c_int32 * 4)(7, 7, 7, 7)
        assert lib.f5_graph_stats(h, out) == 0 and list(out) == [0, 0, 0, 0]
        assert lib.f5_graph_stats(h, None) == 0
    finally:
        lib.f5_destroy(h)


def test_environment_switch_is_read_and_checked_at_create(monkeypatch):
    lib = _lib.load()
    cfg = tiny_config()
    h = C.c_void_p()
    monkeypatch.setenv("F5_LEN_BUCKET", "12")
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == -1 and b"F5_LEN_BUCKET" in lib.f5_last_error()
    monkeypatch.setenv("F5_LEN_BUCKET", "64")
    assert lib.f5_create(C.byref(cfg), C.byref(h)) == 0
    lib.f5_destroy(h)


def test_backbone_keeps_the_switch_and_unett_refuses():
    m = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100)
    assert m.length_bucket == 0
    m.set_length_buckets(64)          # no engine yet: remembered, applied when the engine is built
    assert m.length_bucket == 64
    m.set_length_buckets(0)
    assert m.length_bucket == 0
    for bad in (12, 2048, -8):
        with pytest.raises(ValueError):
            m.set_length_buckets(bad)
    with pytest.raises(RuntimeError):   # no CPU path: preparing graphs needs the engine
        m.init_synthetic().prepare_sample(1, 33, 96, 40, 3, 2.0)
    u = P.UNetT(**P.config.E2TTS_TINY, text_num_embeds=40, mel_dim=100) if hasattr(P.config, "E2TTS_TINY") else None
    if u is None:
        u = P.UNetT(dim=256, depth=4, heads=4, ff_mult=2, text_num_embeds=40, mel_dim=100)
    with pytest.raises(NotImplementedError):
        u.set_length_buckets(64)
    with pytest.raises(NotImplementedError):
        u.prepare_sample(1, 33, 96, 40, 3, 2.0)


def test_load_model_passes_the_length_bucket():
    model = infer.load_model(P.DiT, dict(P.config.F5TTS_TINY), None, device="cpu", length_bucket=64)
    assert model.transformer.length_bucket == 64
    assert infer.load_model(P.DiT, dict(P.config.F5TTS_TINY), None, device="cpu").transformer.length_bucket == 0
    with pytest.raises(ValueError):
        infer.load_model(P.DiT, dict(P.config.F5TTS_TINY), None, device="cpu", length_bucket=12)
    with pytest.raises(NotImplementedError):
        infer.load_model(P.UNetT, dict(dim=256, depth=4, heads=4, ff_mult=2), None, device="cpu", length_bucket=64)
