"""GPU: the DiT and the UNetT through the Python drop-in surface against the float64 reference of tests/backbone_cases.py, on weights
where every block counts (peaked softmax, AdaLN gates about 0.5).  tests/test_backbone_exposure.py shows on the CPU that one block
computed with the wrong rope table, pe_heads, q scale, key count, gate or AdaLN slice moves these outputs by MIN_SHIFT >= 4.5e-3
(DiT) and >= 6.6e-2 (UNetT): what this module holds to float64 is the composition inside the engine's block stages, which no
kernel test and no mode-against-mode test sees.  All errors are L-inf on valid frames.

MEASURED on an MI355X (L-inf against float64 on valid frames; `oracle32` is the float32 CPU oracle's error on the same inputs)

    forward, cfg_infer   f32       oracle32  f16x3     f16p      f16       bf16      f8
      dit_packed         1.08e-6   5.8e-7    4.86e-5   1.11e-4   7.08e-4   4.79e-3   1.28e-2
      dit_padded         8.09e-7   5.4e-7    6.83e-5   1.12e-4   5.47e-4   4.85e-3   1.17e-2
      dit_options        8.18e-7   5.9e-7    1.67e-5   5.62e-5   6.83e-4   5.34e-3   6.95e-3
      dit_b2             7.15e-7   5.5e-7    5.62e-5   1.01e-4   5.26e-4   4.53e-3   1.18e-2
      unett_masked       1.74e-6   1.6e-6    5.87e-4   1.35e-3   1.68e-3   1.22e-2   -
      unett_b2           1.84e-6   1.4e-6    5.45e-4   1.45e-3   1.44e-3   1.18e-2   -
    one Euler step, f32: dit_options in a length bucket of 32 1.64e-6, dit_b2 on isolated rows 1.72e-6 (both bit-equal to the exact form)
    sample(), NFE 4, cfg 2, sway -1, f32 (out / trajectory): DiT Euler 1.55e-6 / 1.55e-6, DiT midpoint 1.52e-6 / 1.52e-6,
                                                            UNetT Euler 3.76e-6 / 3.99e-6; eager, captured and replayed runs bit-equal

    GATES (twice the worst measured value, rounded up to one digit)  and  MIN_SHIFT / gate (smallest wrong-variant shift of any case)
               f32      f16x3    f16p     f16      bf16     f8
      DiT      4e-6     2e-4     3e-4     2e-3     2e-2     3e-2          1100     22       15       2.2      0.2      0.15
      UNetT    4e-6     1e-3     3e-3     4e-3     3e-2     -             16000    66       22       16       2.2      -

Reading the table.  The f32 engine is at 0.14 .. 0.23 of 8 x the CPU oracle's own float32 error (tests/text_cases.py's bound rule) on
every case, so the one f32 gate is 4e-6: 50 times under the project's per-forward gate of 2e-4 and more than 1000 times under the
smallest wrong-variant shift.  f16x3 on the UNetT would get 2e-3 by the rule; it is held to the 1e-3 parity bar instead (1.7 x the
measured 5.9e-4), so that it too detects every variant.  The DiT's f16p stays at 1.1e-4 on these weights, ten times under 1e-3:
DESIGN.md section 3's claim that AdaLN re-normalises each block's input holds where the gates are 0.5, and precision="parity" stays
f16p.  Reported only: bf16 and f8 on the DiT have gates above the smallest shifts (ratios 0.2 and 0.15), so they bound the error and
detect the large variants (gates, AdaLN slice, skipped block: >= 4.7e-2) but not a halved q scale in one block.  sample() is held to
the 1e-3 parity bar.  No case was left out and no defect of the engine was found.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import backbone_cases as BC  # noqa: E402

import f5_tts_amd as P  # noqa: E402

DEV = "cuda:0"
TOL_PARITY = 1e-3             # tests/test_sample_gpu.py: BASELINE.json north_star, "within 1e-3 mel L-inf"
GATE_F32 = 4e-6               # twice the worst measured f32 error (1.84e-6) rounded up to one digit; never above BC.GATE_F32
TOL = {"DiT": {"f16x3": 2e-4, "f16p": 3e-4, "f16": 2e-3, "bf16": 2e-2, "f8": 3e-2},
       "UNetT": {"f16x3": 1e-3, "f16p": 3e-3, "f16": 4e-3, "bf16": 3e-2}}
BUCKET = 32                   # dit_options (N = 65) is planned at 96 frames
T_GRID = [BC.TIME, 1.0]       # one Euler step from the forward cases' time: the engine forms that exist for sample() only
assert GATE_F32 <= BC.GATE_F32 and TOL["DiT"]["f16x3"] <= TOL_PARITY and TOL["UNetT"]["f16x3"] <= TOL_PARITY

_MODELS: dict = {}


def backbone(name, prec="f32", *, isolated=False, bucket=0):
    """The model of a case's weights; the f32 ones, which several tests share, are kept for the module."""
    c = BC.CASE[name]
    k = (c.key, prec, isolated, bucket)
    if k in _MODELS:
        return _MODELS[k]
    tr = (P.DiT if c.backbone == "DiT" else P.UNetT)(**c.arch, text_num_embeds=BC.NV, mel_dim=100, precision=prec)
    tr.load_state_dict(BC.weights_for(c.key))
    if isolated:
        tr.set_isolated_rows(True)
    if bucket:
        tr.set_length_buckets(bucket)
    tr.to(DEV)
    if prec == "f32":
        _MODELS[k] = tr
    return tr


def forward(name, prec="f32"):
    x, cond, text, time, mask = BC.inputs(name)
    out = backbone(name, prec)(x=x.to(DEV), cond=cond.to(DEV), text=text, time=time, mask=None if mask is None else mask.to(DEV),
                               cfg_infer=True)
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------ forward, f32
@pytest.mark.parametrize("name", BC.FORWARD_CASES)
def test_forward_f32_vs_float64(name):
    out, ref, v = forward(name), BC.reference(name), BC.valid(name)
    err, e32 = BC.linf(out, ref, v), BC.oracle32_error(name)
    print(f"[backbone f64] {name:13s} f32 {err:.3e}  oracle32 {e32:.3e}  f32 / (8 x oracle32) {err / (8 * e32):.2f}  "
          f"min shift / gate {BC.MIN_SHIFT[name] / GATE_F32:.0f}")
    assert out.shape == ref.shape and torch.isfinite(out[v.expand_as(out)]).all()
    assert err < GATE_F32


# ------------------------------------------------------------------------------------------------ other precisions
PREC_CASES = [(n, p) for n in BC.FORWARD_CASES for p in ("f16x3", "f16p", "f16", "bf16")] + \
             [(n, "f8") for n in BC.FORWARD_CASES if BC.CASE[n].backbone == "DiT"]


@pytest.mark.parametrize("name,prec", PREC_CASES)
def test_forward_other_precisions_vs_float64(name, prec):
    out, ref, v = forward(name, prec), BC.reference(name), BC.valid(name)
    err, gate = BC.linf(out, ref, v), TOL[BC.CASE[name].backbone][prec]
    print(f"[backbone f64] {name:13s} {prec:5s} {err:.3e}  gate {gate:.0e}  min shift / gate {BC.MIN_SHIFT[name] / gate:.2f}")
    assert torch.isfinite(out[v.expand_as(out)]).all()
    assert err < gate


# ------------------------------------------------------------------------------------------------ other engine forms
def one_step(ref, x):
    """float64: the state after one Euler step of T_GRID from x with the guided velocity of a cfg_infer forward `ref`."""
    B = x.shape[0]
    dt = (torch.tensor(T_GRID[1]) - torch.tensor(T_GRID[0])).double()     # the grid is float32, as sample() keeps it
    pred, null = ref[:B], ref[B:]
    return x.double() + dt * (pred + (pred - null) * BC.CFG)


def test_bucketed_step_is_the_exact_one_and_holds_the_f32_gate():
    """dit_options (B = 1, N = 65, qk_norm, long skip) as one Euler step of sample() from the forward case's x at its time: planned at
    96 frames under a length bucket of 32, it is the exact-shape step bit for bit, and both are the float64 step."""
    name = "dit_options"
    x, cond, text, _, _ = BC.inputs(name)
    cm = torch.ones(1, x.shape[1], dtype=torch.bool)
    got = {}
    for bucket in (0, BUCKET):
        eng = backbone(name, bucket=bucket).engine()
        _, traj = eng.sample(cond, cm, x, text, T_GRID, BC.CFG, want_traj=True)
        torch.cuda.synchronize()
        got[bucket] = traj.cpu()
    assert torch.equal(got[0][0], x)
    err = BC.linf(got[BUCKET][1], one_step(BC.reference(name), x))
    print(f"[backbone f64] {name} bucket {BUCKET}: one step vs float64 {err:.3e}")
    assert torch.equal(got[BUCKET], got[0]), "the bucketed step differs from the exact-shape one"
    assert err < GATE_F32


def test_isolated_rows_step_is_the_item_alone_and_holds_the_f32_gate():
    """dit_b2 ([65, 37], attn_mask_enabled) as one Euler step of sample_items() on isolated rows: every row is the same item through
    sample() at B = 1 on the exact path bit for bit, and the float64 step of the batch on valid frames."""
    name = "dit_b2"
    c = BC.CASE[name]
    x, cond, text, _, mask = BC.inputs(name)
    eng = backbone(name, isolated=True).engine()
    _, traj = eng.sample_items(cond, mask, x, text, [T_GRID] * c.B, [BC.CFG] * c.B, lens=list(c.lens), want_traj=True)
    torch.cuda.synchronize()
    traj = traj.cpu()
    v = BC.valid(name, halves=1)
    err = BC.linf(traj[1], one_step(BC.reference(name), x), v)
    print(f"[backbone f64] {name} isolated rows: one step vs float64 {err:.3e}")
    assert err < GATE_F32
    exact = backbone(name).engine()
    for b, n in enumerate(c.lens):
        nt = int((text[b] != -1).sum())
        _, alone = exact.sample(cond[b:b + 1, :n], torch.ones(1, n, dtype=torch.bool), x[b:b + 1, :n], text[b:b + 1, :nt], T_GRID, BC.CFG,
                                want_traj=True)
        assert torch.equal(traj[1, b, :n], alone.cpu()[1, 0]), f"item {b} on isolated rows differs from the item alone"


# ------------------------------------------------------------------------------------------------ sample()
@pytest.mark.parametrize("bb,method", [("DiT", "euler"), ("DiT", "midpoint"), ("UNetT", "euler")])
def test_sample_f32_vs_float64_forward_oracle(bb, method):
    cond, text, dur, lens = BC.sample_inputs(bb)
    o_out, o_traj = BC.sample64(bb, method)
    tr = backbone(BC.SAMPLE_CASES[bb])
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method=method)).to(DEV)
    tr.graph_stats(reset=True)
    runs = []
    for _ in range(3):          # eager, captured, replayed
        out, traj = model.sample(cond, text, dur, lens=lens, **BC.sample_kwargs())
        torch.cuda.synchronize()
        runs.append((out.cpu(), traj.cpu()))
    out, traj = runs[0]
    v = BC.sample_valid(bb)
    e_out, e_traj = BC.linf(out, o_out, v), BC.linf(traj, o_traj, v[None])
    print(f"[backbone f64] {bb} sample() {method}: out {e_out:.3e} traj {e_traj:.3e} (state magnitude {o_traj.abs().max().item():.2f})")
    assert traj.shape == o_traj.shape and e_out < TOL_PARITY and e_traj < TOL_PARITY
    for rep, (o, t) in enumerate(runs[1:], 1):
        assert torch.equal(o, out) and torch.equal(t, traj), f"run {rep} (captured, then replayed) differs from the eager one"
    st = tr.graph_stats()
    assert st["captures"] == 1 and st["replays"] >= 1, st
