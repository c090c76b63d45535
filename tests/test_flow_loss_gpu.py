"""GPU: f5_flow_loss -- the glue kernels of csrc/flow.h against a NumPy restatement of their arithmetic contract, then CFM.flow_loss,
CFM.forward and infer.heldout_loss end to end against the fixtures tests/golden/flow_loss_*.npz (the reference's own CFM.forward,
tools/make_golden_flow.py) and the float64 oracle tests/flow_oracle.py.

Measured on an MI355X (pred Linf e against the reference; the loss error beside its bound flow_oracle.loss_tolerance(loss_ref, e, n)):
  f32    e 9.5e-7 .. 3.8e-6 over the six fixtures; loss error 0 .. 3.6e-11 (MMDiT 3.7e-9) under bounds of 9.7e-9 .. 3.8e-8 (6.3e-6)
  f16x3  e 3.4e-5 / 4.3e-5 (DiT B = 3 / attn_mask_enabled); loss error 9.8e-10 / 7.1e-10, bounds 2.7e-7 / 3.6e-7
  f16p   e 2.8e-4 / 3.3e-4; loss error 6.5e-9 / 2.6e-9, bounds 2.3e-6 / 2.7e-6
  bf16   e 5.8e-3 / 7.1e-3; loss error 2.3e-6 / 2.1e-6, bounds 7.8e-5 / 1.1e-4
  kernels: sq_sum within 1.9e-16 relative of a float64 fold; everything else bit-equal to the NumPy restatement
(DESIGN.md section 6p).  Every test prints its figures before it asserts.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import adapter_util as U
import f5_tts_amd as P
import flow_oracle as FO
import ode_oracle
from conftest import load_golden
from f5_tts_amd import _lib, adapters as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = ["flow_loss_dit_b3", "flow_loss_dit_b2_drop_audio", "flow_loss_dit_b2_drop_both", "flow_loss_dit_b3_attnmask",
            "flow_loss_unett_b2", "flow_loss_mmdit_b2"]
F32_BAR = 2e-4   # tests/test_sample_gpu.py and tests/test_mmdit_gpu.py: an f32 forward against the reference (x max(1, |pred|) for the MMDiT's larger weights)


# ------------------------------------------------------------------------------------------------ kernel wrappers
def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def k_flow_mix(x0, x1, t, span, want_cond=True):
    B, N, mel = x0.shape
    sp = torch.tensor(span, dtype=torch.int32, device=x0.device).contiguous()
    phi, cond = torch.empty_like(x0), (torch.empty_like(x0) if want_cond else None)
    _lib.check(_lib.load().f5k_flow_mix(_p(x0), _p(x1), _p(t), _p(sp), _lib.int_array([v for se in span for v in se]), _p(phi), _p(cond),
                                        B, N, mel, _s()), "f5k_flow_mix")
    return phi, cond


def k_flow_loss_reduce(pred, x0, x1, span, want_frame_err=True):
    B, N, mel = pred.shape
    sp = torch.tensor(span, dtype=torch.int32, device=pred.device).contiguous()
    part = torch.full((B * ((N + 63) // 64),), float("nan"), dtype=torch.float64, device=pred.device)
    sq, cnt = torch.empty(B, dtype=torch.float64, device=pred.device), torch.empty(B, dtype=torch.int32, device=pred.device)
    fe = torch.full((B, N), float("nan"), device=pred.device) if want_frame_err else None
    _lib.check(_lib.load().f5k_flow_loss_reduce(_p(pred), _p(x0), _p(x1), _p(sp), _lib.int_array([v for se in span for v in se]), _p(part),
                                                _p(sq), _p(cnt), _p(fe), B, N, mel, _s()), "f5k_flow_loss_reduce")
    return sq, cnt, fe


# ------------------------------------------------------------------------------------------------ the NumPy restatement (csrc/flow.h)
def _butterfly(v):
    """Six rounds v[l] += v[l ^ o], o = 32 .. 1, over the last axis (64 lanes); every lane ends with the same sum."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def np_flow_mix(x0, x1, t, span):
    B, N, _ = x0.shape
    tb = t.astype(np.float32)[:, None, None]
    om = np.float32(1.0) - tb
    phi = om * x0 + tb * x1   # float32 arrays: each product and the sum rounded to f32
    n = np.arange(N)[None, :]
    sp = np.asarray(span)
    in_span = (n >= sp[:, :1]) & (n < sp[:, 1:])
    return phi.astype(np.float32), np.where(in_span[..., None], np.float32(0.0), x1)


def np_flow_loss(pred, x0, x1, span):
    """sq_sum, count, frame_err in flow.h's order; frames outside the span are masked before any arithmetic touches them."""
    B, N, mel = pred.shape
    assert mel % 4 == 0 and mel // 4 <= 64
    n = np.arange(N)[None, :]
    sp = np.asarray(span)
    in_span = (n >= sp[:, :1]) & (n < sp[:, 1:])
    sel = in_span[..., None]
    p, a, z = (np.where(sel, v, np.float32(0.0)).astype(np.float32) for v in (pred, x0, x1))
    d = (p - (z - a)).astype(np.float32).astype(np.float64).reshape(B, N, mel // 4, 4)
    lane = np.zeros((B, N, 64))
    acc = np.zeros((B, N, mel // 4))
    for j in range(4):
        acc = acc + d[..., j] * d[..., j]
    lane[..., :mel // 4] = acc
    row = _butterfly(lane)                                    # [B, N]
    frame_err = np.where(in_span, (row / float(mel)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    nblk = (N + 63) // 64
    rows = np.zeros((B, nblk * 64))
    rows[:, :N] = np.where(in_span, row, 0.0)
    rows = rows.reshape(B, nblk, 16, 4)                        # frame 64 k + 4 j + w is [k, j, w]
    wave = np.zeros((B, nblk, 4))
    for j in range(16):
        wave = wave + rows[:, :, j, :]
    part = np.zeros((B, nblk))
    for w in range(4):
        part = part + wave[:, :, w]
    m = (nblk + 63) // 64
    parts = np.zeros((B, m * 64))
    parts[:, :nblk] = part
    parts = parts.reshape(B, m, 64)
    lanes = np.zeros((B, 64))
    for i in range(m):
        lanes = lanes + parts[:, i, :]
    return _butterfly(lanes), (sp[:, 1] - sp[:, 0]).astype(np.int32), frame_err


def _kernel_inputs(B, N, mel, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, mel, generator=g), torch.randn(B, N, mel, generator=g), torch.randn(B, N, mel, generator=g),
            torch.rand(B, generator=g))


def _poison(t, span):
    """NaN in every frame outside the item's span."""
    t = t.clone()
    for b, (s, e) in enumerate(span):
        t[b, :s] = float("nan")
        t[b, e:] = float("nan")
    return t


# B = 3, N = 37, mel = 100, lens 37 / 36 / 1: the empty span, the whole item, the last frame, an interior span
SPANS = {"empty_whole_one": [(0, 0), (0, 36), (0, 1)], "last_interior_empty": [(36, 37), (5, 20), (0, 0)],
         "whole_last_one": [(0, 37), (35, 36), (0, 1)]}


@pytest.mark.parametrize("which", list(SPANS))
def test_flow_mix_is_the_contract_bit_for_bit(which):
    span = SPANS[which]
    pred, x0, x1, t = _kernel_inputs(3, 37, 100, 1)
    phi, cond = k_flow_mix(x0.to(DEV), x1.to(DEV), t.to(DEV), span)
    want_phi, want_cond = np_flow_mix(x0.numpy(), x1.numpy(), t.numpy(), span)
    assert np.array_equal(phi.cpu().numpy().view(np.uint32), want_phi.view(np.uint32))
    assert np.array_equal(cond.cpu().numpy().view(np.uint32), want_cond.view(np.uint32))
    # ... which is torch's (1 - t) * x0 + t * x1, and torch.where(span, 0, x1)
    t3 = t[:, None, None]
    assert torch.equal(phi.cpu(), (1 - t3) * x0 + t3 * x1)
    phi_only, none = k_flow_mix(x0.to(DEV), x1.to(DEV), t.to(DEV), span, want_cond=False)
    assert none is None and torch.equal(phi_only, phi)


@pytest.mark.parametrize("which", list(SPANS))
def test_flow_loss_reduce_is_the_contract_and_never_reads_outside_the_span(which):
    span = SPANS[which]
    pred, x0, x1, _ = _kernel_inputs(3, 37, 100, 2)
    want_sq, want_cnt, want_fe = np_flow_loss(pred.numpy(), x0.numpy(), x1.numpy(), span)
    fold = np.array([((pred[b, s:e] - (x1[b, s:e] - x0[b, s:e])).double() ** 2).sum().item() for b, (s, e) in enumerate(span)])
    runs = []
    for poisoned in (False, True, True):
        args = [(_poison(v, span) if poisoned else v).to(DEV) for v in (pred, x0, x1)]
        sq, cnt, fe = k_flow_loss_reduce(*args, span)
        runs.append((sq.cpu().numpy(), cnt.cpu().numpy(), fe.cpu().numpy()))
    sq, cnt, fe = runs[0]
    for b, (s, e) in enumerate(span):
        rel = abs(sq[b] - fold[b]) / fold[b] if fold[b] else abs(sq[b])
        print(f"{which} item {b}: sq_sum {sq[b]:.17g}, float64 fold {fold[b]:.17g}, relative {rel:.2e} (bound {(e - s) * 100 * 2.0 ** -52:.2e})")
        assert rel <= (e - s) * 100 * 2.0 ** -52
    assert np.array_equal(cnt, want_cnt) and np.isfinite(sq).all() and np.isfinite(fe).all()
    assert np.array_equal(fe.view(np.uint32), want_fe.view(np.uint32))
    assert np.array_equal(sq.view(np.uint64), want_sq.view(np.uint64))       # the stated order, not only the bound
    for other in runs[1:]:                                                    # poisoned with NaN, twice: the same bits
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(other, runs[0]))
    sq2, cnt2, none = k_flow_loss_reduce(pred.to(DEV), x0.to(DEV), x1.to(DEV), span, want_frame_err=False)
    assert none is None and np.array_equal(sq2.cpu().numpy(), sq) and np.array_equal(cnt2.cpu().numpy(), cnt)


def test_flow_kernels_across_block_boundaries():
    """B = 2, N = 5,000: 79 blocks of 64 frames per item (the last one partial), more block sums than one wave has lanes."""
    span = [(3, 4990), (4031, 4097)]
    pred, x0, x1, t = _kernel_inputs(2, 5000, 100, 3)
    phi, cond = k_flow_mix(x0.to(DEV), x1.to(DEV), t.to(DEV), span)
    want_phi, want_cond = np_flow_mix(x0.numpy(), x1.numpy(), t.numpy(), span)
    assert np.array_equal(phi.cpu().numpy().view(np.uint32), want_phi.view(np.uint32))
    assert np.array_equal(cond.cpu().numpy().view(np.uint32), want_cond.view(np.uint32))
    want_sq, want_cnt, want_fe = np_flow_loss(pred.numpy(), x0.numpy(), x1.numpy(), span)
    outs = [k_flow_loss_reduce(*[_poison(v, span).to(DEV) for v in (pred, x0, x1)], span) for _ in range(2)]
    sq, cnt, fe = (v.cpu().numpy() for v in outs[0])
    for b, (s, e) in enumerate(span):
        fold = ((pred[b, s:e] - (x1[b, s:e] - x0[b, s:e])).double() ** 2).sum().item()
        print(f"item {b}: sq_sum {sq[b]:.17g}, float64 fold {fold:.17g}, relative {abs(sq[b] - fold) / fold:.2e}")
        assert abs(sq[b] - fold) / fold <= (e - s) * 100 * 2.0 ** -52
    assert np.array_equal(cnt, want_cnt) and np.array_equal(fe.view(np.uint32), want_fe.view(np.uint32))
    assert np.array_equal(sq.view(np.uint64), want_sq.view(np.uint64))
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))


# ------------------------------------------------------------------------------------------------ end to end
_models = {}


def build_model(meta, sd, prec):
    cls = {"DiT": P.DiT, "UNetT": P.UNetT, "MMDiT": P.MMDiT}[meta["backbone"]]
    arch = {k: v for k, v in meta["arch"].items()}
    tr = cls(**arch, text_num_embeds=meta["nvocab"], mel_dim=100, precision=prec)
    tr.load_state_dict(sd)
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)


def fixture_model(name, prec):
    if (name, prec) not in _models:
        meta, a = load_golden(name)
        _models[(name, prec)] = (meta, a, build_model(meta, FO.fixture_weights(meta), prec))
    return _models[(name, prec)]


def run_flow_loss(meta, a, model):
    return model.flow_loss(a["inp"], a["text"], torch.tensor(meta["lens"]), time=a["time"], span=meta["span"], x0=a["x0"],
                           drop_audio_cond=meta["drop_audio_cond"], drop_text=meta["drop_text"])


def check_against_fixture(tag, meta, a, loss, pred, bar):
    """Prints e and the loss error beside its bound, then holds e to `bar` (None: no bar of its own) and the loss to the bound."""
    e = (pred.cpu() - a["pred"]).abs().max().item()
    loss_ref = a["loss"].item()
    tol = FO.loss_tolerance(loss_ref, e, meta["n_selected"])
    d = abs(loss.item() - loss_ref)
    print(f"[{tag}] pred Linf e {e:.3e}; loss {loss.item():.9e} vs {loss_ref:.9e}: |d| {d:.3e}, bound {tol:.3e}")
    assert torch.isfinite(pred).all() and torch.isfinite(loss)
    if bar is not None:
        assert e < bar
    assert d <= tol
    return e


@pytest.mark.parametrize("name", FIXTURES)
def test_flow_loss_f32_vs_reference(name):
    meta, a, model = fixture_model(name, "f32")
    loss, per_item, pred, cond, frame_err = run_flow_loss(meta, a, model)
    bar = F32_BAR * (max(1.0, a["pred"].abs().max().item()) if meta["backbone"] == "MMDiT" else 1.0)
    check_against_fixture(f"f32 {name}", meta, a, loss, pred, bar)
    assert torch.equal(cond.cpu(), a["cond"])
    # per_item and frame_err are the same sums, cut another way
    count = torch.tensor([e - s for s, e in meta["span"]], dtype=torch.float64)
    assert (per_item.cpu().double() * count).sum().item() / count.sum().item() == pytest.approx(loss.item(), rel=1e-5)
    assert frame_err.cpu().double().sum(1).div(count).tolist() == pytest.approx(per_item.cpu().tolist(), rel=1e-5)
    seq = torch.arange(a["inp"].shape[1])
    outside = torch.stack([(seq < s) | (seq >= e) for s, e in meta["span"]])
    assert not frame_err.cpu()[outside].any()
    # the float64 oracle on the same inputs: frame by frame
    r = FO.flow_loss(meta["backbone"], FO.fixture_weights(meta), meta["arch"], a["inp"], a["x0"], a["text"], a["time"], meta["span"], meta["lens"],
                     meta["drop_audio_cond"], meta["drop_text"])
    e = (pred.cpu().double() - r["pred"]).abs().max().item()
    fe = (frame_err.cpu().double() - r["frame_err"]).abs().max().item()
    print(f"[f32 {name}] vs the float64 oracle: pred Linf {e:.3e}, frame_err Linf {fe:.3e} (largest frame_err {r['frame_err'].max().item():.3e})")
    fmax = r["frame_err"].max().item()
    assert fe <= 2 * fmax ** 0.5 * e + e * e + fmax * 2.0 ** -22   # (as loss_tolerance, per frame; the last term: the f64 -> f32 rounding)


@pytest.mark.parametrize("prec", ["f16p", "f16x3", "bf16"])
def test_flow_loss_16bit_precisions_stay_inside_the_inequality(prec):
    """No bar of their own: each precision's measured e is printed (DESIGN.md section 6p records it) and the loss must lie inside the
    same inequality with that e."""
    for name in ("flow_loss_dit_b3", "flow_loss_dit_b3_attnmask"):
        meta, a, model = fixture_model(name, prec)
        loss, per_item, pred, cond, frame_err = run_flow_loss(meta, a, model)
        check_against_fixture(f"{prec} {name}", meta, a, loss, pred, None)
        assert torch.equal(cond.cpu(), a["cond"])


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_with_the_fixtures_seeds(name):
    """CFM.forward draws on the CPU in the reference's order: the fixture's seeds give the fixture's span, noise, time and flags, so
    `cond` is the fixture's bit for bit and the loss lies inside the inequality."""
    meta, a, model = fixture_model(name, "f32")
    model.audio_drop_prob, model.cond_drop_prob = meta["audio_drop_prob"], meta["cond_drop_prob"]
    assert model.noise_device == "cpu"
    torch.manual_seed(meta["seed"])
    random.seed(meta["seed"])
    loss, cond, pred = model(a["inp"], a["text"], lens=torch.tensor(meta["lens"]))
    assert loss.dtype == torch.float32 and loss.device.type == "cuda" and torch.equal(cond.cpu(), a["cond"])
    bar = F32_BAR * (max(1.0, a["pred"].abs().max().item()) if meta["backbone"] == "MMDiT" else 1.0)
    check_against_fixture(f"forward {name}", meta, a, loss, pred, bar)


def test_forward_raises_on_bad_spans_before_anything_runs():
    meta, a, model = fixture_model("flow_loss_dit_b3", "f32")
    with pytest.raises(_lib.F5Error, match=r"f5_flow_loss: item 1: span = \[3, 34\)"):
        model.flow_loss(a["inp"], a["text"], torch.tensor(meta["lens"]), time=a["time"], span=[(1, 30), (3, 34), (0, 20)], x0=a["x0"])
    loss, per_item, *_ = model.flow_loss(a["inp"], a["text"], torch.tensor(meta["lens"]), time=a["time"], span=[(1, 30), (5, 5), (0, 20)],
                                         x0=a["x0"])
    assert torch.isnan(per_item[1]) and torch.isfinite(per_item[[0, 2]]).all() and torch.isfinite(loss)   # an empty span: NaN for that item alone


# ------------------------------------------------------------------------------------------------ batch composition
def test_an_item_is_bit_equal_alone_and_in_a_batch_with_attn_mask_enabled():
    """With attn_mask_enabled=True the keys, the conv position embedding and the text of an item stop at its own length, so its sq_sum
    does not depend on the items beside it.  With the shipped setting (attn_mask_enabled=False) no such claim is made: rows attend
    over the padding of the batch, as they do in the reference, so an item's loss depends on the batch's N."""
    meta, a, model = fixture_model("flow_loss_dit_b3_attnmask", "f32")
    eng = model.transformer.engine()
    sq, cnt, pred, _, fe = eng.flow_loss(a["inp"], a["x0"], a["text"], a["time"].tolist(), meta["span"], lens=meta["lens"])
    for b, n in enumerate(meta["lens"]):
        one = eng.flow_loss(a["inp"][b:b + 1, :n], a["x0"][b:b + 1, :n], a["text"][b:b + 1], a["time"][b:b + 1].tolist(), [meta["span"][b]],
                            lens=[n])
        print(f"item {b} (len {n}): in the batch {sq[b].item():.17g}, alone {one[0][0].item():.17g}")
        assert torch.equal(one[0][0], sq[b]) and torch.equal(one[4][0], fe[b, :n]) and torch.equal(one[2][0], pred[b, :n])


# ------------------------------------------------------------------------------------------------ adapters
ADAPTERS = {"a": (dict(seed=1), U.RECIPE), "b": (dict(seed=2, ranks=8, in_rank=0, blocks=[1], mods=("to_q", "to_v"), scale=2.0, text=True),
                                                  dict(lora_alpha=32, lora_r=16))}


def _heldout_set():
    g = torch.Generator().manual_seed(12)
    mels = [torch.randn(n, 100, generator=g) for n in (33, 21, 40)]
    texts = [torch.randint(0, 40, (6 + 2 * i,), generator=g) for i in range(3)]
    return mels, texts


def _tiny(sd=None, prec="f16p", attn_mask=False):
    arch = dict(P.config.F5TTS_TINY, attn_mask_enabled=attn_mask)
    meta = dict(backbone="DiT", arch=arch, nvocab=40)
    if sd is None:
        sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, 40), seed=0)
        sd = ode_oracle.scaled_time_mlp(sd, 8.0)
    return meta, sd, build_model(meta, sd, prec)


def test_heldout_loss_under_set_adapter_equals_a_fresh_engine_on_merged_weights():
    mels, texts = _heldout_set()
    meta, sd, model = _tiny()
    tensors = {}
    for name, (kw, scales) in ADAPTERS.items():
        tensors[name] = U.synth_adapter(sd, meta["arch"]["depth"], **kw)
        model.transformer.add_adapter(name, tensors[name], **scales)
    model.transformer.set_adapter("b")
    got = P.infer.heldout_loss(model, mels, texts, adapters=(None, "a", "b"), times=2, seed=1, batch_frames=80)
    assert model.transformer.active_adapter == "b"
    for name in (None, "a", "b"):
        merged = sd if name is None else A.merge_adapter(sd, tensors[name], rule="contract", **ADAPTERS[name][1])
        want = P.infer.heldout_loss(_tiny(merged)[2], mels, texts, times=2, seed=1, batch_frames=80)[None]
        print(f"adapter {name}: resident {got[name]['loss']:.9e}, fresh engine on merged weights {want['loss']:.9e}")
        assert got[name]["per_item"] == want["per_item"] and got[name]["per_time"] == want["per_time"] and got[name]["loss"] == want["loss"]
    assert got["a"]["per_item"] != got[None]["per_item"] and got["b"]["per_item"] != got[None]["per_item"], "an adapter changes nothing"


def test_heldout_ranking_matches_the_float64_oracle():
    """Three fine-tunes of one base -- two synthetic adapters, and the base with noise added to every to_q (in the form an adapter
    carries it: a rank-8 pair whose product has std 0.05) -- ranked by heldout_loss on one resident f32 engine and by the float64
    oracle over the same rows, batches and draws.  A ranking is only asked for where it means something: the oracle's smallest gap
    must be 20 x the largest distance between the engine's loss and the oracle's."""
    mels, texts = _heldout_set()
    meta, sd, model = _tiny(prec="f32")
    depth = meta["arch"]["depth"]
    tensors = {name: U.synth_adapter(sd, depth, **kw) for name, (kw, _) in ADAPTERS.items()}
    scales = {name: s for name, (_, s) in ADAPTERS.items()}
    tensors["noisy_q"] = U.synth_adapter(sd, depth, seed=5, ranks=8, in_rank=0, mods=("to_q",), scale=2.0, text=False, delta_std=0.05)
    scales["noisy_q"] = dict(lora_alpha=32, lora_r=16)
    for name, t in tensors.items():
        model.transformer.add_adapter(name, t, **scales[name])
    names = list(tensors)
    got = P.infer.heldout_loss(model, mels, texts, adapters=names, times=2, seed=1, batch_frames=80)
    lens = [m.shape[0] for m in mels]
    spans, noises = P.infer.heldout_draws(lens, 100, seed=1)
    pad = torch.nn.utils.rnn.pad_sequence
    want = {}
    for name in names:
        W = A.merge_adapter(sd, tensors[name], rule="contract", **scales[name])
        sq = cnt = 0.0
        for rows in P.infer.heldout_rows(lens, 2, 80):
            us = [u for u, _ in rows]
            r = FO.flow_loss("DiT", W, meta["arch"], pad([mels[u] for u in us], batch_first=True), pad([noises[u] for u in us], batch_first=True),
                             pad([texts[u] for u in us], padding_value=-1, batch_first=True), torch.tensor([(k + 0.5) / 2 for _, k in rows]),
                             [spans[u] for u in us], [lens[u] for u in us])
            sq, cnt = sq + r["sq_sum"].sum().item(), cnt + r["count"].sum().item() * 100
        want[name] = sq / cnt
        print(f"{name}: heldout_loss {got[name]['loss']:.9e}, float64 oracle {want[name]:.9e}")
    order = sorted(names, key=lambda n: want[n])
    gaps = [want[b] - want[a] for a, b in zip(order, order[1:])]
    worst = max(abs(got[n]["loss"] - want[n]) for n in names)
    print(f"oracle order {order}, gaps {gaps}, largest |engine - oracle| {worst:.3e}")
    assert min(gaps) > 20 * worst, "the fine-tunes are too close for a ranking to mean anything"
    assert sorted(names, key=lambda n: got[n]["loss"]) == order
