"""GPU: f8 at real size -- the C2 shape (F5-TTS Base, B = 1, 256 + 768 frames, NFE 16, cfg 2, sway -1, synthetic weights at std 0.02)
against the f32 ENGINE (never against f8 itself), beside f16p on the same call.  Synthetic weights cannot say whether f8 is good enough
for a checkpoint (infer.heldout_loss under f16p and f8 does); this is a regression guard: finite, and within 4x of the
error recorded in DESIGN.md section 3 (the factor covers seed-to-seed spread)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import f5_tts_amd as P  # noqa: E402
from test_configs_gpu import NV, _model  # noqa: E402

F8_C2_RECORDED = 2.2e-2   # max |f8 - f32 engine| over the trajectory, as measured for DESIGN.md section 3 (f16p on the same call: 1.7e-4)


def test_c2_size_f8_against_the_f32_engine():
    arch = P.config.F5TTS_BASE
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, NV))
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(1, 256, 100, generator=g)
    text = torch.randint(1, NV - 2, (1, round(0.15 * 1024)), generator=g)
    kw = dict(steps=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    _, ref = _model(P.DiT, arch, sd, "f32").sample(cond, text, 1024, **kw)
    errs = {}
    for prec in ("f16p", "f8"):
        _, traj = _model(P.DiT, arch, sd, prec).sample(cond, text, 1024, **kw)
        assert torch.isfinite(traj).all(), prec
        errs[prec] = (traj - ref).abs().max().item()
    print(f"[C2 size, N=1024 NFE=16] traj Linf against the f32 engine: f16p {errs['f16p']:.3e}, f8 {errs['f8']:.3e} "
          f"(state magnitude {ref.abs().max().item():.2f})")
    assert errs["f8"] <= 4 * F8_C2_RECORDED
