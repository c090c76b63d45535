"""GPU: the MMDiT backbone (joint text-audio attention blocks) through the Python drop-in surface, against
  (1) the vectors produced by running the reference's MMDiT (tests/golden/mmdit_*.npz, tools/make_mmdit_golden.py), all frames --
      an MMDiT batch runs rectangular, padding rows computed --, and
  (2) the float64 restatement tests/mmdit_oracle.py (midpoint solver, which no fixture covers).
The fixtures' weights are N(0, 0.06) (three times the project's usual scale: the text stream must reach the output, see the
generator), so the gates are measured for this backbone, against the reference's vectors, on an MI355X:

    MEASURED (worst trajectory L-inf per fixture; state magnitude 5.8 .. 8.2)
                        f32       f16x3     f16p      f16       bf16
      mmdit_b1_nfe4     6.0e-6    2.1e-4    9.1e-4    4.0e-3    2.7e-2
      mmdit_b3_ragged   6.9e-6    2.2e-4    1.5e-3    4.0e-3    2.8e-2
      mmdit_b2_qknorm   5.2e-6    2.0e-4    9.0e-4    3.2e-3    2.6e-2
      mmdit_b1_nocfg    2.4e-6    8.3e-5    4.6e-4    1.7e-3    1.4e-2
    forward taps, f32: audio embedding 4.1e-6, c / x after every block <= 4.1e-6, output 4.1e-6; midpoint f32 vs float64 5.2e-6
    many-row f16 batch (ping-pong tile, staged joint epilogue) against its items alone: bit-identical at nt = 8 and nt = 13

Each gate is twice the worst measured value rounded up to one digit, and for f32 and f16x3 never above the project's 1e-3 mel L-inf
bar (TOL_PARITY).  f16p does not stay under 1e-3 at this weight scale (1.5e-3 on the ragged batch): it is held to f16's gate, as
test_sample_gpu.py holds it on the UNetT, and precision="parity" resolves to f16x3 for this backbone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import f5_tts_amd as P  # noqa: E402
import mmdit_oracle as MO  # noqa: E402
import ode_oracle as OO  # noqa: E402
from conftest import load_golden  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from gpu_util import k_gemm_plan  # noqa: E402
from mmdit_cases import SAMPLE_FIXTURES, mmdit_weights, sample_kwargs  # noqa: E402

DEV = "cuda:0"
TOL_PARITY = 1e-3
TOL = {"f32": 2e-5, "f16x3": 5e-4, "f16": 8e-3, "bf16": 6e-2}
TOL["f16p"] = TOL["f16"]


def build_cfm(meta, sd, precision, method="euler"):
    tr = P.MMDiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision=precision)
    tr.load_state_dict(sd)
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method=method)).to(DEV)


def run_case(meta, a, model):
    dur, kw = sample_kwargs(meta, a)
    out, traj = model.sample(a["cond"], a["text"], dur, **kw)
    return out.cpu(), traj.cpu()


_cases = {}


def case(name):
    if name not in _cases:
        meta, a = load_golden(name)
        _cases[name] = (meta, a, mmdit_weights(meta))
    return _cases[name]


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16p"])
@pytest.mark.parametrize("name", SAMPLE_FIXTURES)
def test_sample_parity_vs_reference_vectors(name, prec):
    meta, a, sd = case(name)
    out, traj = run_case(meta, a, build_cfm(meta, sd, prec))
    assert out.shape == a["out"].shape and traj.shape == a["traj"].shape
    assert torch.isfinite(traj).all(), "every frame is computed, padding rows included"
    e_out, e_traj = (out - a["out"]).abs().max().item(), (traj - a["traj"]).abs().max().item()
    print(f"[mmdit parity {prec}] {name}: out Linf {e_out:.3e} traj Linf {e_traj:.3e} (all frames)")
    assert prec == "f16p" or TOL[prec] <= TOL_PARITY
    assert e_traj < TOL[prec] and e_out < TOL[prec]


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", SAMPLE_FIXTURES)
def test_16bit_error_is_bounded_and_reported(name, prec):
    meta, a, sd = case(name)
    out, traj = run_case(meta, a, build_cfm(meta, sd, prec))
    e_out, e_traj = (out - a["out"]).abs().max().item(), (traj - a["traj"]).abs().max().item()
    print(f"[mmdit {prec}] {name}: out Linf {e_out:.3e} traj Linf {e_traj:.3e} (state magnitude {a['traj'].abs().max().item():.2f})")
    assert torch.isfinite(out).all() and torch.isfinite(traj).all()
    assert e_traj < TOL[prec] and e_out < TOL[prec]


def test_parity_precision_is_one_of_the_measured_ones():
    tr = P.MMDiT(dim=256, depth=2, heads=4, ff_mult=2, text_num_embeds=40)
    assert tr.precision == "f16x3"   # f16p misses 1e-3 on the ragged fixture (header); DESIGN.md section 10


# ----------------------------------------------------------------------------------------- forward taps, f32
def test_forward_taps_vs_reference():
    """One cfg_infer forward of the ragged case: text embedding and audio embedding < 1e-4; c and x after every block and the
    output < 2e-4 x max(1, tap abs-max) -- the bars the DiT taps are held to, scaled because these weights are larger."""
    meta, a = load_golden("mmdit_forward_taps")
    for part in ("_x0", "_x1"):
        a.update(load_golden("mmdit_forward_taps" + part)[1])
    sd = mmdit_weights(meta)
    tr = P.MMDiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    tr.to(DEV)
    eng = tr.engine()
    B, N = a["x"].shape[:2]
    nt, D, depth = a["text"].shape[1], meta["arch"]["dim"], meta["arch"]["depth"]
    tc = eng.text_embed(a["text"], N, drop_text=False).cpu()
    tu = eng.text_embed(a["text"], N, drop_text=True).cpu()
    assert tc.shape == a["text_cond"].shape
    assert (tc - a["text_cond"]).abs().max() < 1e-4 and (tu - a["text_uncond"]).abs().max() < 1e-4
    nx, nc = 2 * B * N * D, 2 * B * nt * D
    buf = torch.full((nx + (depth - 1) * (nc + nx) + nx,), float("nan"), device=DEV)
    eng.mmdit_taps(buf)
    out = tr(x=a["x"].to(DEV), cond=a["cond"].to(DEV), text=a["text"], time=a["time"], mask=a["mask"].to(DEV), cfg_infer=True).cpu()
    eng.mmdit_taps(None)
    taps, off = {}, 0

    def take(key, n, shape):
        nonlocal off
        taps[key] = buf[off:off + n].view(shape).cpu()
        off += n

    take("audio_embed", nx, (2 * B, N, D))
    for i in range(depth):
        if i < depth - 1:
            take(f"block{i}_c", nc, (2 * B, nt, D))
        take(f"block{i}_x", nx, (2 * B, N, D))
    assert off == buf.numel()
    e = (taps["audio_embed"] - a["audio_embed"]).abs().max().item()
    print(f"[mmdit taps f32] audio_embed Linf {e:.3e}")
    assert e < 1e-4
    for k in [k for k in taps if k.startswith("block")]:
        e, mag = (taps[k] - a[k]).abs().max().item(), a[k].abs().max().item()
        print(f"[mmdit taps f32] {k} Linf {e:.3e} (abs-max {mag:.2f})")
        assert e < 2e-4 * max(1.0, mag), k
    e, mag = (out - a["out"]).abs().max().item(), a["out"].abs().max().item()
    print(f"[mmdit taps f32] out Linf {e:.3e} (abs-max {mag:.2f})")
    assert e < 2e-4 * max(1.0, mag)


# ------------------------------------------------------------------------------------------------ midpoint
def test_midpoint_vs_float64_oracle():
    meta, a, sd = case("mmdit_b1_nfe4")
    dur, kw = sample_kwargs(meta, a)
    with OO.solver("midpoint"):
        o_out, o_traj = MO.sample(sd, meta["arch"], a["cond"], a["text"], dur, **kw)
    assert (o_traj - a["traj"]).abs().max() > 1e-2, "the midpoint solve is another trajectory than the Euler fixture"
    out, traj = run_case(meta, a, build_cfm(meta, sd, "f32", method="midpoint"))
    e_out, e_traj = (out - o_out).abs().max().item(), (traj - o_traj).abs().max().item()
    print(f"[mmdit midpoint f32] out Linf {e_out:.3e} traj Linf {e_traj:.3e}")
    assert traj.shape[0] == meta["steps"] + 1 and e_traj < TOL_PARITY and e_out < TOL_PARITY


# ------------------------------------------------------------------------------------------ engine invariances
def test_graph_capture_and_replay_are_bit_identical():
    meta, a, sd = case("mmdit_b3_ragged")
    model = build_cfm(meta, sd, "f16p")
    model.transformer.graph_stats(reset=True)
    runs = [run_case(meta, a, model) for _ in range(3)]   # eager, capture, replay
    for out, traj in runs[1:]:
        assert torch.equal(out, runs[0][0]) and torch.equal(traj, runs[0][1])
    st = model.transformer.graph_stats()
    assert st["captures"] == 1 and st["replays"] >= 1, st


def test_cfg_infer_equals_the_two_separate_forwards():
    meta, a = load_golden("mmdit_forward_taps")
    tr = P.MMDiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32")
    tr.load_state_dict(mmdit_weights(meta))
    tr.to(DEV)
    kw = dict(x=a["x"].to(DEV), cond=a["cond"].to(DEV), text=a["text"], time=a["time"], mask=a["mask"].to(DEV))
    both = tr(**kw, cfg_infer=True)
    cond_half = tr(**kw)
    uncond_half = tr(**kw, drop_audio_cond=True, drop_text=True)
    assert torch.equal(both, torch.cat((cond_half, uncond_half), dim=0))
    assert not torch.equal(cond_half, uncond_half)


def test_clear_cache_then_another_text_gives_that_texts_result():
    meta, a, sd = case("mmdit_b1_nfe4")
    model = build_cfm(meta, sd, "f32")
    dur, kw = sample_kwargs(meta, a)
    first, _ = model.sample(a["cond"], a["text"], dur, **kw)
    model.transformer.clear_cache()
    other, _ = model.sample(a["cond"], a["text_order"], dur, **kw)
    assert (first.cpu() - a["out"]).abs().max() < TOL_PARITY
    assert (other.cpu() - a["out_order"]).abs().max() < TOL_PARITY and (other.cpu() - a["out"]).abs().max() > 2e-2


def test_engine_refuses_per_item_solves_and_long_texts():
    meta, a, sd = case("mmdit_b1_nfe4")
    model = build_cfm(meta, sd, "f32")
    eng = model.transformer.engine()
    N = 50
    cm = torch.zeros(1, N, dtype=torch.bool)
    y0 = torch.zeros(1, N, 100)
    with pytest.raises(_lib.F5Error, match="MMDiT"):
        eng.sample_items(a["cond"], cm, y0, a["text"], [[0.0, 0.5, 1.0]], [2.0])
    with pytest.raises(_lib.F5Error, match="1024"):
        eng.sample(a["cond"], cm, y0, torch.zeros(1, 1025, dtype=torch.long), [0.0, 1.0], 2.0)
    with pytest.raises(_lib.F5Error, match="MMDiT"):
        eng.set_length_buckets(64)


# --------------------------------------------------------------------- many rows: the ping-pong GEMM's staged epilogue
@pytest.mark.parametrize("nt", [8, 13])
def test_many_row_batch_equals_its_items_alone(nt):
    """16,384 audio rows (B = 8 with cfg_infer, N = 1024) at dim 256: the QKV GEMM of the audio stream takes the 256 x 256 ping-pong
    tile, whose interior tiles store q / k / V^T through the STAGED form of the joint epilogue -- V^T staged at the aligned offset
    nt = 8, unstaged at nt = 13 (staged_ok) -- where one item alone (2,048 rows) takes a ring tile and the unstaged form.  Without a
    mask the items of a batch do not interact, so both must give the same f16 forward: the operands are rounded alike and only the
    f32 accumulation order of a tile may differ (a few ulp, far below 1e-4 of the output's magnitude; a misplaced store is O(1))."""
    arch = dict(dim=256, depth=2, heads=4, dim_head=64, ff_mult=2, text_mask_padding=True, qk_norm=None)
    tr = P.MMDiT(**arch, text_num_embeds=40, mel_dim=100, precision="f16")
    tr.load_state_dict(P.weights.synthetic_state_dict(P.weights.mmdit_param_shapes(arch, 40), seed=1, std=0.06))
    tr.to(DEV)
    B, N = 8, 1024
    assert tuple(k_gemm_plan(2, 2 * B * N, 3 * 256, 256)[0][:2]) == (3, 20), "the plan of this QKV GEMM is the ping-pong tile"
    assert k_gemm_plan(2, 2 * N, 3 * 256, 256)[0][0] == 2, "one item alone takes a ring tile"
    g = torch.Generator().manual_seed(9)
    x, cond = torch.randn(B, N, 100, generator=g).to(DEV), torch.randn(B, N, 100, generator=g).to(DEV)
    text = torch.randint(0, 40, (B, nt), generator=g)
    time = torch.tensor(0.37)
    batch = tr(x=x, cond=cond, text=text, time=time, cfg_infer=True).cpu()
    assert torch.isfinite(batch).all()
    worst = 0.0
    for b in range(B):
        alone = tr(x=x[b:b + 1], cond=cond[b:b + 1], text=text[b:b + 1], time=time, cfg_infer=True).cpu()
        worst = max(worst, (alone[0] - batch[b]).abs().max().item(), (alone[1] - batch[B + b]).abs().max().item())
    mag = batch.abs().max().item()
    print(f"[mmdit many rows f16] nt={nt}: batch vs items alone Linf {worst:.3e} (abs-max {mag:.2f})")
    assert worst <= 1e-4 * mag
