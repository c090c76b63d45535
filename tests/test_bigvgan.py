"""BigVGAN v2 (BASELINE config 5's vocoder).  PARITY UNPINNED: the reference takes BigVGAN from an un-vendored
submodule and its weights from the hub, so the checker is the repository's own restatement of the published architecture
(oracle/bigvgan_oracle.py); the in-tree part -- the bigvgan mel variant, model/modules.py:33-75 -- is restated from the
reference's own lines, with librosa's filterbank from memory.

CPU: properties of the restated pieces that hold for the published design whatever the weights.
GPU: csrc/bigvgan.hip through the C ABI against the oracle on the same synthetic weights."""
import pytest
import torch

import f5_tts_amd as P
from oracle import bigvgan_oracle as BO


def test_kaiser_sinc_filter_and_alias_free_activation_properties():
    fu, fd = BO.aa_filters()
    assert fu.shape == (12,) and abs(float(fu.sum()) - 1.0) < 1e-6 and torch.allclose(fu, fu.flip(0), atol=1e-7)
    assert torch.equal(fu, P.bigvgan.kaiser_sinc_filter1d(0.25, 0.3, 12)), "the product uploads the oracle's filter"
    # a constant passes 2x upsampling and 2x low-pass downsampling unchanged (unit DC gain, replicate padding)
    x = torch.full((1, 3, 40), 0.7)
    up = BO.upsample1d(x, fu)
    assert up.shape == (1, 3, 80) and torch.allclose(up, torch.full_like(up, 0.7), atol=1e-5)
    dn = BO.downsample1d(up, fd)
    assert dn.shape == x.shape and torch.allclose(dn, x, atol=1e-5)
    # SnakeBeta with log-scale parameters 0 is x + sin(x)^2
    z = torch.randn(1, 3, 40)
    zero = torch.zeros(3)
    assert torch.allclose(BO.snake_beta(z, zero, zero), z + torch.sin(z) ** 2, atol=1e-6)


def test_generator_shapes_and_upsampling_factor():
    cfg = P.config.BIGVGAN_TINY
    V = P.weights.synthetic_state_dict(P.weights.bigvgan_param_shapes(cfg), seed=1)
    mel = torch.randn(2, 100, 9)
    wav = BO.bigvgan_forward(V, cfg, mel)
    assert wav.shape == (2, 1, 9 * 8) and torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0
    full = P.weights.bigvgan_param_shapes(P.config.BIGVGAN_V2_24K)
    n = sum(int(torch.tensor(s).prod()) for s in full.values())
    assert 100e6 < n < 125e6, f"bigvgan_v2_24khz_100band_256x has ~112 M parameters (restated layout gives {n / 1e6:.1f} M)"
    assert full["ups.0.0.weight"] == (1536, 768, 8) and full["resblocks.17.convs1.2.weight"] == (24, 24, 11)


def test_slaney_filterbank_and_bigvgan_mel_shape():
    fb = BO.librosa_slaney_mel_fb(24000, 1024, 100)
    assert fb.shape == (100, 513) and (fb >= 0).all()
    assert ((fb > 0).sum(1) >= 1).all(), "every band has support"
    peak = fb.argmax(1)
    assert (peak[1:] >= peak[:-1]).all(), "band centres increase"
    wav = torch.randn(2, 24000) * 0.1
    m = BO.mel_spectrogram_bigvgan(wav)
    assert m.shape == (2, 100, 24000 // 256) and torch.isfinite(m).all()      # center=False: floor(nw / hop) frames


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("cfg_name,T,B", [("BIGVGAN_TINY", 37, 2), ("BIGVGAN_TINY", 5, 1), ("BIGVGAN_MID", 24, 1), ("BIGVGAN_V2_24K", 8, 1)])
def test_bigvgan_hip_vs_oracle(cfg_name, T, B, prec):
    """(BIGVGAN_V2_24K, T = 8: the PRODUCTION width -- 1536 / 768 / 384 / 192 / 96 channels through the implicit-GEMM kernels with
    tpt = C / 32 up to 48 K-tiles per tap, and in f16x3 the pre-split MODE 5 operands + the hardware-sin activation -- on 8 frames,
    which the CPU restatement finishes in seconds.  Still PARITY UNPINNED: the checker is this repository's restatement.)"""
    cfg = getattr(P.config, cfg_name, None) or dict(P.config.BIGVGAN_V2_24K, upsample_initial_channel=256)   # MID: all 6 stages, 256 -> 4 channels
    V = P.weights.synthetic_state_dict(P.weights.bigvgan_param_shapes(cfg), seed=3)
    mel = torch.randn(B, T, 100, generator=torch.Generator().manual_seed(T)).permute(0, 2, 1)   # the callers' transposed view
    ref = BO.bigvgan_forward(V, cfg, mel.double(), dtype=torch.float64)
    voc = P.BigVGAN(cfg, precision=prec)
    voc.load_state_dict(V)
    voc.to("cuda:0")
    wav = voc(mel.to("cuda:0")).cpu()
    assert wav.shape == ref.shape
    e = (wav.double() - ref).abs().max().item()
    print(f"[bigvgan {prec}] {cfg_name} T={T}: wav Linf {e:.3e} vs float64 (peak {ref.abs().max().item():.3f}, clipped {(ref.abs() >= 1).float().mean().item():.3f})")
    assert e < {"f32": 1.5e-6, "f16x3": 3e-6}[prec] * max(1.0, ref.abs().max().item())   # measured 7.7e-7 / 1.4e-6


@pytest.mark.gpu
def test_bigvgan_full_size_runs_and_is_deterministic():
    """nvidia/bigvgan_v2_24khz_100band_256x dimensions (112 M parameters, 256x upsampling), 1 s of audio: shape, range,
    bit-determinism; the CPU restatement of this size takes minutes, so parity is asserted at the reduced widths above."""
    voc = P.BigVGAN(P.config.BIGVGAN_V2_24K).init_synthetic(seed=2).to("cuda:0")
    mel = torch.randn(1, 100, 94, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    w1 = voc(mel)
    w2 = voc(mel)
    assert w1.shape == (1, 1, 94 * 256) and torch.isfinite(w1).all() and float(w1.abs().max()) <= 1.0
    assert torch.equal(w1, w2)


@pytest.mark.gpu
def test_bigvgan_implicit_conv_equals_materialised_operand(monkeypatch):
    """The implicit-GEMM convolutions (GemmConv: K-tiles read shifted rows of the zero-haloed activation) accumulate the same
    products in the same order as the im2col GEMMs they replace: bit-identical waveforms (all kernel sizes and dilations)."""
    cfg = dict(P.config.BIGVGAN_V2_24K, upsample_initial_channel=256)
    voc = P.BigVGAN(cfg).init_synthetic(seed=5).to("cuda:0")
    mel = torch.randn(1, 100, 31, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    monkeypatch.setenv("F5_BIGVGAN_NARROW", "0")        # the narrow-stage MFMA kernel sums in another order: GEMM path for all stages here
    w_imp = voc(mel).clone()
    monkeypatch.setenv("F5_BIGVGAN_IMPLICIT", "0")
    w_mat = voc(mel)
    assert torch.equal(w_imp, w_mat)


@pytest.mark.gpu
def test_bigvgan_mel_variant_vs_oracle():
    """mel_spec_type="bigvgan" (model/modules.py:33-75) on the HIP front-end against the restatement of those lines."""
    g = torch.Generator().manual_seed(4)
    for nw in (24000, 12345):
        wav = torch.randn(2, nw, generator=g) * 0.1
        ref = BO.mel_spectrogram_bigvgan(wav)
        got = P.mel.MelSpec(mel_spec_type="bigvgan")(wav.to("cuda:0")).cpu()
        assert got.shape == ref.shape
        e = (got - ref).abs().max().item()
        print(f"[bigvgan mel] nw={nw}: frames {ref.shape[-1]}, log-mel Linf {e:.3e}")
        assert e < 2e-3
