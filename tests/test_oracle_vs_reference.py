"""CPU: the oracle against the reference itself, through what the reference computed on the same inputs
(tests/golden/ref_*.npz, written by oracle/make_golden.py, which imports the reference's own code)."""
import torch

import f5_tts_amd as P
from conftest import load_golden, synthetic_weights
from oracle import f5_oracle as O


def test_base_arch_cfg_forward_matches():
    """F5-TTS Base (configs/F5TTS_Base.yaml:24-36), one packed CFG forward at N=192."""
    meta, a = load_golden("ref_base_cfg_forward")
    arch = P.config.F5TTS_BASE
    nv = P.config.VOCAB_SIZE + 1  # load_model passes vocab_size + 1 (utils_infer.py:313-317)
    assert meta["arch"] == arch and meta["nvocab"] == nv
    sd = synthetic_weights(meta)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 192, 100, generator=g)
    cond = torch.randn(1, 192, 100, generator=g)
    cond[:, 60:] = 0
    text = torch.randint(0, nv - 1, (1, 40), generator=g)
    t = torch.tensor(0.25)
    assert torch.equal(x, a["x"]) and torch.equal(cond, a["cond"]) and torch.equal(text, a["text"]) and torch.equal(t, a["time"])
    r = a["out"]
    o = O.dit_forward(sd, arch, x, cond, text, t, cfg_infer=True)
    assert o.shape == r.shape
    assert (r - o).abs().max() < 5e-5
    assert r.abs().max() > 0.05


def test_tiny_sample_variants_match():
    meta, a = load_golden("ref_tiny_sample_attnmask")
    arch = dict(P.config.F5TTS_TINY, attn_mask_enabled=True)
    nv = 33
    assert meta["arch"] == arch and meta["nvocab"] == nv
    sd = synthetic_weights(meta)
    g = torch.Generator().manual_seed(9)
    cond = torch.randn(2, 28, 100, generator=g)
    text = torch.randint(0, nv, (2, 15), generator=g)
    text[1, 9:] = -1
    assert torch.equal(cond, a["cond"]) and torch.equal(text, a["text"])
    kw = dict(lens=torch.tensor([28, 19]), steps=10, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=11)
    r_out, r_traj = a["out"], a["traj"]
    o_out, o_traj = O.sample(sd, arch, cond, text, torch.tensor([60, 47]), **kw)
    assert o_traj.shape == r_traj.shape and o_out.shape == r_out.shape
    assert (r_traj - o_traj).abs().max() < 2e-5 and (r_out - o_out).abs().max() < 2e-5


def test_noise_draw_matches_reference_rule():
    """cfm.py:196-201: same seed for every sample -> identical noise prefixes across the batch."""
    y0 = O.draw_noise(torch.tensor([7, 4]), 100, seed=3)
    assert torch.equal(y0[0, :4], y0[1, :4]) and torch.all(y0[1, 4:] == 0)
