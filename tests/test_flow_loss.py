"""CPU: CFM.forward / CFM.flow_loss / infer.heldout_loss above the engine call (f5_flow_loss), without a GPU.

  * the host part of CFM.forward -- the draws, the span, the flags -- against the reference's CFM.forward imported live, on stub
    backbones that record what they are handed;
  * tests/flow_oracle.py (float64) against the fixtures tests/golden/flow_loss_*.npz, which tools/make_golden_flow.py made by running
    the reference; and the fixtures' power to tell the oracle's deliberately wrong variants from the right glue;
  * f5_flow_loss's argument rules on a null handle, the ABI symbols;
  * heldout_loss's draws, batching, result and adapter handling on a stub engine.
"""
import ctypes as C
import random

import pytest
import torch

from conftest import load_golden

import f5_tts_amd as P
import flow_oracle as FO
from f5_tts_amd import _lib
from oracle import ref_harness as rh

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")

FIXTURES = ["flow_loss_dit_b3", "flow_loss_dit_b2_drop_audio", "flow_loss_dit_b2_drop_both", "flow_loss_dit_b3_attnmask",
            "flow_loss_unett_b2", "flow_loss_mmdit_b2"]
ORACLE_TOL = 2e-5    # float64 oracle vs the reference's f32 CPU run: the bar of tests/test_oracle_golden.py
GPU_F32_BAR = 2e-4   # the bar tests/test_sample_gpu.py holds an f32 forward to against the reference (the GPU tests' e is below it)


# ------------------------------------------------------------------------------------------------ stubs
class StubEngine:
    """Stands where Engine stands: records every flow_loss call, returns host tensors of the right shapes."""

    def __init__(self, owner=None):
        self.calls, self.owner = [], owner

    def flow_loss(self, x1, x0, text, time, span, lens=None, drop_audio_cond=False, drop_text=False, want_pred=True, want_cond=True,
                  want_frame_err=True):
        B, N, mel = x1.shape
        self.calls.append(dict(x1=x1.clone(), x0=x0.clone(), text=text.clone(), time=list(time), span=[tuple(s) for s in span], lens=lens,
                               drop_audio_cond=drop_audio_cond, drop_text=drop_text,
                               adapter=None if self.owner is None else self.owner.active_adapter))
        if self.owner is not None and self.owner.fail_on == self.owner.active_adapter and self.owner.fail_on is not None:
            raise RuntimeError("stub failure")
        # a sum that depends on the row's own data, time and adapter only: the mean over the span of (x1 + x0)^2, scaled by the time
        sq = torch.stack([((x1[b, s:e] + x0[b, s:e]).double() ** 2).sum() * (1 + time[b]) for b, (s, e) in enumerate(span)])
        if self.owner is not None and self.owner.active_adapter is not None:
            sq = sq * 2
        cnt = torch.tensor([e - s for s, e in span], dtype=torch.int32)
        z = torch.zeros(B, N, mel)
        return sq, cnt, z if want_pred else None, z.clone() if want_cond else None, torch.zeros(B, N) if want_frame_err else None


class StubBackbone(torch.nn.Module):
    def __init__(self, adapters=()):
        super().__init__()
        self.dim, self._names, self.active_adapter, self.fail_on = 8, list(adapters), None, None
        self._anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)
        self.eng = StubEngine(self)
        self.switches = []

    @property
    def device(self):
        return self._anchor.device

    def engine(self):
        return self.eng

    def set_adapter(self, name):
        assert name is None or name in self._names
        self.active_adapter = name
        self.switches.append(name)


class RefRecorder(torch.nn.Module):
    """The reference CFM's transformer: records its keyword arguments, predicts zero."""

    def __init__(self):
        super().__init__()
        self.dim, self.seen = 8, {}
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, **kw):
        self.seen = kw
        return torch.zeros_like(kw["x"])


def stub_cfm(adapters=()):
    return P.CFM(StubBackbone(adapters), mel_spec_module=rh.InertMelSpec())


# ------------------------------------------------------------------------------------------------ CFM.forward, host part
def test_forward_returns_loss_cond_pred_from_one_engine_call():
    model = stub_cfm()
    inp, text = torch.randn(2, 12, 100), torch.randint(0, 30, (2, 5))
    torch.manual_seed(3)
    random.seed(3)
    loss, cond, pred = model(inp, text, lens=torch.tensor([12, 9]))
    (call,) = model.transformer.eng.calls
    assert loss.dtype == torch.float32 and loss.ndim == 0 and cond.shape == pred.shape == inp.shape
    assert call["lens"] == [12, 9] and len(call["time"]) == 2 and call["x0"].shape == inp.shape
    for (s, e), n in zip(call["span"], (12, 9)):
        assert 0 <= s <= e <= n and e - s >= int(0.7 * n)
    want = sum(((inp[b, s:e] + call["x0"][b, s:e]).double() ** 2).sum() * (1 + call["time"][b]) for b, (s, e) in enumerate(call["span"]))
    assert loss.item() == pytest.approx(float(want) / (sum(e - s for s, e in call["span"]) * 100), rel=1e-6)
    with pytest.raises(TypeError):
        model(inp, text, torch.tensor([12, 9]))   # lens is keyword-only, as in the reference


def test_forward_over_an_empty_selection_is_nan():
    model = stub_cfm()
    model.frac_lengths_mask = (0.0, 0.0)
    loss, _, _ = model(torch.randn(1, 6, 100), torch.zeros(1, 3, dtype=torch.long))
    assert model.transformer.eng.calls[0]["span"][0][0] == model.transformer.eng.calls[0]["span"][0][1] and torch.isnan(loss)


@needs_reference
@pytest.mark.parametrize("seed", [0, 1, 2, 5, 11, 23])
@pytest.mark.parametrize("lens", [None, [30, 30, 30], [30, 17, 1], [30, 29, 8]])
def test_forward_draws_and_spans_are_the_references(seed, lens):
    """Same torch.manual_seed and random.seed: the reference's CFM.forward (imported live) hands its transformer x, cond, time and the
    flags; ours hands the engine x0, time, span and the flags.  They must be the same draws, bit for bit."""
    ref = rh.load()
    theirs = ref.CFM(transformer=RefRecorder(), mel_spec_module=rh.InertMelSpec())
    ours = stub_cfm()
    B, N = 3, 30
    g = torch.Generator().manual_seed(100 + seed)
    inp, text = torch.randn(B, N, 100, generator=g), torch.randint(0, 30, (B, 7), generator=g)
    lens_t = None if lens is None else torch.tensor(lens)
    for m in (theirs, ours):
        torch.manual_seed(seed)
        random.seed(seed)
        with torch.no_grad():
            m(inp, text, lens=lens_t)
    seen, (call,) = theirs.transformer.seen, ours.transformer.eng.calls
    assert call["time"] == seen["time"].tolist() and torch.equal(torch.tensor(call["time"], dtype=torch.float32), seen["time"])
    assert (call["drop_audio_cond"], call["drop_text"]) == (seen["drop_audio_cond"], seen["drop_text"])
    assert call["lens"] == (lens or [N] * B) and torch.equal(seen["mask"], P.utils.lens_to_mask(torch.tensor(call["lens"]), N))
    seq = torch.arange(N)
    in_span = torch.stack([(seq >= s) & (seq < e) for s, e in call["span"]])
    assert torch.equal(seen["cond"], torch.where(in_span[..., None], torch.zeros_like(inp), inp))
    t = seen["time"][:, None, None]
    assert torch.equal(seen["x"], (1 - t) * call["x0"] + t * inp)
    assert torch.equal(call["x1"], inp) and torch.equal(call["text"], text)


@needs_reference
def test_span_arithmetic_is_the_references():
    ref = rh.load()
    lens = torch.tensor([40, 33, 21, 1, 7])
    for seed in range(8):
        frac = torch.zeros(5).uniform_(0.0 if seed % 2 else 0.7, 1.0, generator=torch.Generator().manual_seed(seed))
        torch.manual_seed(seed)
        theirs = ref.utils.mask_from_frac_lengths(lens, frac)
        torch.manual_seed(seed)
        ours = P.utils.mask_from_frac_lengths(lens, frac)
        torch.manual_seed(seed)
        start, end = P.utils.span_from_frac_lengths(lens, frac)
        assert torch.equal(theirs, ours) and torch.equal(ours, P.utils.mask_from_start_end_indices(lens, start, end))
        assert torch.equal(ref.utils.mask_from_start_end_indices(lens, start, end), ours)
        assert (start >= 0).all() and (end <= lens).all() and (start <= end).all()


# ------------------------------------------------------------------------------------------------ the oracle and the fixtures
@pytest.fixture(scope="module")
def oracle_runs():
    """Every fixture through the float64 oracle, once: the right glue and each wrong variant."""
    runs = {}
    for name in FIXTURES:
        meta, a = load_golden(name)
        W = FO.fixture_weights(meta)
        args = (meta["backbone"], W, meta["arch"], a["inp"], a["x0"], a["text"], a["time"], meta["span"], meta["lens"],
                meta["drop_audio_cond"], meta["drop_text"])
        runs[name] = (meta, a, FO.flow_loss(*args), {v: FO.flow_loss(*args, variant=v) for v in FO.VARIANTS})
    return runs


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_fixture(oracle_runs, name):
    meta, a, r, _ = oracle_runs[name]
    e = (r["pred"] - a["pred"]).abs().max().item()
    loss_ref = a["loss"].item()
    tol = FO.loss_tolerance(loss_ref, e, meta["n_selected"])
    print(f"{name}: oracle pred Linf {e:.3e}; loss {r['loss'].item():.9e} vs {loss_ref:.9e} (|d| {abs(r['loss'].item() - loss_ref):.3e}, bound {tol:.3e})")
    assert e <= ORACLE_TOL
    assert torch.equal(r["cond"].float(), a["cond"]) and int(r["count"].sum()) * 100 == meta["n_selected"]
    assert abs(r["loss"].item() - loss_ref) <= tol


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_tells_every_wrong_variant_apart(oracle_runs, name):
    """Each wrong variant misses the fixture's loss by at least 100 x the GPU tests' tolerance (flow_oracle.loss_tolerance at the f32 bar:
    the GPU tests use their measured e, which is smaller).  "ignore_drops" is a variant only where the fixture sets a drop flag."""
    meta, a, _, wrong = oracle_runs[name]
    loss_ref = a["loss"].item()
    tol = FO.loss_tolerance(loss_ref, GPU_F32_BAR, meta["n_selected"])
    for v, r in wrong.items():
        ratio = abs(r["loss"].item() - loss_ref) / tol
        print(f"{name}: variant {v}: loss {r['loss'].item():.6e} vs {loss_ref:.6e}: {ratio:.1f} x the tolerance {tol:.3e}")
        if v == "ignore_drops" and not (meta["drop_audio_cond"] or meta["drop_text"]):
            continue
        assert ratio >= 100.0, (name, v, ratio)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_symbols_are_exported():
    lib = _lib.load()
    for name in ("f5_flow_loss", "f5k_flow_mix", "f5k_flow_loss_reduce"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def _flow_loss_rc(time, lens, span, B, N, handle=None, nt=4):
    lib = _lib.load()
    one = C.c_void_p(8)   # never dereferenced: the rules are checked first
    rc = lib.f5_flow_loss(handle, one, one, one, nt, _lib.float_array(time), _lib.int_array(lens), _lib.int_array(span), B, N, 0, 0,
                          one, one, None, None, None, None)
    return rc, lib.f5_last_error().decode()


def test_argument_rules_are_checked_before_the_engine():
    rc, msg = _flow_loss_rc([0.5, 0.5], [10, 8], [0, 10, 2, 8], 2, 10)
    assert rc != 0 and msg == "f5_flow_loss: null engine"           # well-formed tables: the engine is the first thing missing
    for time, lens, span, B, N, what in [
        ([0.5, float("nan")], [10, 8], [0, 10, 2, 8], 2, 10, "item 1: time is not finite"),
        ([0.5, 0.5], [10, 11], [0, 10, 2, 8], 2, 10, "lens[1]=11 out of (0, N]"),
        ([0.5, 0.5], [10, 0], [0, 10, 0, 0], 2, 10, "lens[1]=0 out of (0, N]"),
        ([0.5, 0.5], [10, 8], [0, 10, 2, 9], 2, 10, "item 1: span = [2, 9) outside 0 <= start <= end <= 8 frames"),
        ([0.5, 0.5], [10, 8], [-1, 10, 2, 8], 2, 10, "item 0: span = [-1, 10)"),
        ([0.5, 0.5], [10, 8], [0, 10, 5, 4], 2, 10, "item 1: span = [5, 4)"),
        ([0.5], None, [0, 11], 1, 10, "item 0: span = [0, 11) outside 0 <= start <= end <= 10 frames"),
        ([0.5], None, [0, 0], 0, 10, "bad arguments"),
    ]:
        rc, msg = _flow_loss_rc(time, lens, span, B, N)
        assert rc == -1 and msg.startswith("f5_flow_loss: ") and what in msg, (msg, what)
    lib = _lib.load()
    assert lib.f5k_flow_mix(None, None, None, None, None, None, None, 1, 4, 100, None) == -1 and lib.f5_last_error().startswith(b"f5k_flow_mix:")
    one = C.c_void_p(8)
    assert lib.f5k_flow_mix(one, one, one, one, _lib.int_array([0, 5]), one, None, 1, 4, 100, None) == -1
    assert b"f5k_flow_mix: item 0: span = [0, 5)" in lib.f5_last_error()
    assert lib.f5k_flow_loss_reduce(one, one, one, one, _lib.int_array([0, 4]), one, one, one, None, 1, 4, 98, None) == -1
    assert lib.f5_last_error().startswith(b"f5k_flow_loss_reduce:")


# ------------------------------------------------------------------------------------------------ heldout_loss
def _heldout_inputs():
    g = torch.Generator().manual_seed(9)
    mels = [torch.randn(n, 100, generator=g) for n in (30, 17, 44, 8, 25)]
    texts = [torch.randint(0, 30, (5 + i,), generator=g) for i in range(5)]
    return mels, texts


def _rows(calls, adapter):
    """{(utterance length, time): (span, x0, x1)} of every row the stub saw under `adapter`."""
    rows = {}
    for c in calls:
        if c["adapter"] != adapter:
            continue
        for b, n in enumerate(c["lens"]):
            key = (n, round(c["time"][b], 9))
            assert key not in rows
            rows[key] = (c["span"][b], c["x0"][b, :n].clone(), c["x1"][b, :n].clone())
            assert not c["x0"][b, n:].any() and not c["x1"][b, n:].any() and not c["drop_audio_cond"] and not c["drop_text"]
    return rows


def test_heldout_draws_do_not_depend_on_the_adapter_or_the_batching():
    mels, texts = _heldout_inputs()
    seen, results = [], []
    for batch_frames in (38400, 60, 1):
        model = stub_cfm(adapters=("a", "b"))
        results.append(P.infer.heldout_loss(model, mels, texts, adapters=(None, "a", "b"), times=4, seed=3, batch_frames=batch_frames))
        calls = model.transformer.eng.calls
        per = [_rows(calls, a) for a in (None, "a", "b")]
        assert len(per[0]) == 5 * 4 and {t for _, t in per[0]} == {0.125, 0.375, 0.625, 0.875}
        for other in per[1:]:
            assert other.keys() == per[0].keys()
            for k, (span, x0, x1) in per[0].items():
                assert other[k][0] == span and torch.equal(other[k][1], x0) and torch.equal(other[k][2], x1)
        seen.append(per[0])
        assert model.transformer.active_adapter is None
    for other in seen[1:]:
        assert other.keys() == seen[0].keys()
        for k, (span, x0, x1) in seen[0].items():
            assert other[k][0] == span and torch.equal(other[k][1], x0)
    # one span and one noise per utterance, whatever the time; the spans follow the span rule
    spans, noises = P.infer.heldout_draws([m.shape[0] for m in mels], 100, seed=3)
    for (n, t), (span, x0, _) in seen[0].items():
        u = [m.shape[0] for m in mels].index(n)
        assert span == spans[u] and torch.equal(x0, noises[u]) and 0 <= span[0] <= span[1] <= n and span[1] - span[0] == int(
            (torch.empty(1).uniform_(0.7, 1.0, generator=torch.Generator().manual_seed((3 << 32) + u)) * n).long())
    # the result does not depend on the batching either, and is what the stub's sums make it
    for r in results[1:]:
        for a in (None, "a", "b"):
            assert r[a]["loss"] == pytest.approx(results[0][a]["loss"], rel=1e-12)
            assert r[a]["per_item"] == pytest.approx(results[0][a]["per_item"], rel=1e-12)
            assert r[a]["per_time"] == pytest.approx(results[0][a]["per_time"], rel=1e-12)
    r = results[0]
    assert r["a"]["loss"] == pytest.approx(2 * r[None]["loss"]) and len(r[None]["per_item"]) == 5 and len(r[None]["per_time"]) == 4
    want = 0.0
    for (n, t), (span, x0, x1) in seen[0].items():
        want += float(((x1[span[0]:span[1]] + x0[span[0]:span[1]]).double() ** 2).sum() * (1 + t))
    assert r[None]["loss"] == pytest.approx(want / (4 * 100 * sum(s[1] - s[0] for s in spans)), rel=1e-9)


def test_heldout_batches_respect_the_frame_budget():
    lens = [30, 17, 44, 8, 25]
    rows = P.infer.heldout_rows(lens, 3, 60)
    assert sorted(r for b in rows for r in b) == [(u, k) for u in range(5) for k in range(3)]
    assert len(rows) > 1 and len(P.infer.heldout_rows(lens, 3, 10 ** 6)) <= len(rows)


def test_heldout_texts_per_adapter_and_previous_adapter_restored():
    mels, texts = _heldout_inputs()
    model = stub_cfm(adapters=("a", "b"))
    other = [t + 1 for t in texts]
    model.transformer.set_adapter("b")
    P.infer.heldout_loss(model, mels, {None: texts, "a": other}, adapters=(None, "a"), times=2)
    assert model.transformer.active_adapter == "b"
    for c in model.transformer.eng.calls:
        first = c["text"][0]
        want = (other if c["adapter"] == "a" else texts)
        assert any(torch.equal(first[:len(w)], w) for w in want)
    with pytest.raises(ValueError, match="one text per utterance"):
        P.infer.heldout_loss(model, mels, {None: texts}, adapters=(None, "a"))
    # an exception inside the walk: the adapter that was active before is active again
    model.transformer.fail_on = "a"
    with pytest.raises(RuntimeError, match="stub failure"):
        P.infer.heldout_loss(model, mels, texts, adapters=(None, "a"), times=2)
    assert model.transformer.active_adapter == "b"
