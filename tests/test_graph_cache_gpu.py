"""GPU: the sample() graph cache through eviction, resize and invalidation, held to the header's contract.

Every call of an engine with graphs on is compared, bit for bit (torch.equal on `out` and on the trajectory), with the same call on a
second engine built under F5_HIP_GRAPH=0, and after every call f5_graph_stats must read what tests/graph_cache_oracle.py (the header's
rules, in plain Python) says -- which also fixes the path of every call: eager, capture or replay.  One signature per precision anchors
the eager engine to oracle.f5_oracle.sample, so that "eager" is not its own witness.  Signatures that share a shape differ in
cfg_strength (2.0, 2.25, 2.5, ...), and their eager references are asserted pairwise unequal: a lookup that returned another
signature's graph could not go unseen.  A captured graph holds raw arena pointers, so a graph that survives a clear, or a key that
resolves to the wrong exec, shows as a wrong mel, not as an error.

F5TTS_TINY DiT, synthetic weights at std 0.02, f16p and f32, NFE 2, B in {1, 2, 3}, N in {32, 48, 96} (the prepare case needs one
length per bucket: 17 buckets of 8 frames from 32 to 160, which hold 32, 48 and 96), texts of 9 to 40 tokens.  Every test prints its
counters before it asserts."""
import contextlib
import itertools
import os
from dataclasses import dataclass, replace

import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_cache_oracle as G  # noqa: E402
import f5_tts_amd as P  # noqa: E402
from graph_cache_oracle import GraphCacheModel, ItemSig, Sig  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

DEV = "cuda:0"
NV = 40
ARCH = P.config.F5TTS_TINY
TOL_PARITY = 1e-3            # tests/test_sample_gpu.py: BASELINE.json north_star, "within 1e-3 mel L-inf"
COND_FRAMES = 24
PRECISIONS = ("f16p", "f32")
_cache = {}


@dataclass(frozen=True)
class Call:
    """One sampler call.  lens: None, "ragged" (N, N - 7, N - 13) or "equal" (N, N, N); items: through sample_items, one setting for all."""
    B: int
    N: int
    cfg: float = 2.0
    nt: int = 12
    steps: int = 2
    lens: str | None = None
    items: bool = False

    def durations(self):
        return None if self.lens is None else [self.N - (0, 7, 13)[b] * (self.lens == "ragged") for b in range(self.B)]

    def sig(self):
        if self.items:   # (Euler, one grid for every item: one time row per step)
            return ItemSig(B=self.B, N=self.N, nt=self.nt, steps=self.steps, U=self.steps, guided=self.cfg >= 1e-5, lens=self.lens)
        return Sig(B=self.B, N=self.N, nt=self.nt, steps=self.steps, cfg=self.cfg, lens=self.lens)


def st(captures, replays, eager, evictions):
    return dict(captures=captures, replays=replays, eager=eager, evictions=evictions)


@contextlib.contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def weights():
    if "sd" not in _cache:
        _cache["sd"] = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(ARCH, NV), seed=0, std=0.02)
    return _cache["sd"]


def make(prec, *, graphs=True):
    """A DiT whose engine is built now: the switches are read when the engine is created."""
    tr = P.DiT(**ARCH, text_num_embeds=NV, mel_dim=100, precision=prec)
    tr.load_state_dict(weights())
    tr.to(DEV)
    with environ(F5_HIP_GRAPH=None if graphs else "0", F5_LEN_BUCKET=None, F5_SPLIT_CFG=None):
        tr.engine()
    return tr


def inputs(c: Call):
    """Deterministic inputs of a call's shape (the guidance is not part of them): 24 prompt frames, noise that is zero past an item's own
    length (as CFM.sample draws it), texts padded with -1 behind nt, nt - 2, nt - 3 tokens."""
    key = ("in", c.B, c.N, c.nt, c.steps, c.lens)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * c.B + 10 * c.N + c.nt)
        cond = torch.randn(c.B, COND_FRAMES, 100, generator=g)
        y0 = torch.randn(c.B, c.N, 100, generator=g)
        text = torch.randint(0, NV - 1, (c.B, c.nt), generator=g)
        for b, d in enumerate(c.durations() or []):
            y0[b, d:] = 0
            text[b, c.nt - (0, 2, 3)[b]:] = -1
        mask = torch.zeros(c.B, c.N, dtype=torch.bool)
        mask[:, :COND_FRAMES] = True
        _cache[key] = (cond, mask, y0, text, O.time_grid(c.steps, -1.0).tolist())
    return _cache[key]


def launch(eng, c: Call):
    """The call, enqueued: (out, traj) on the device, nothing waited for."""
    cond, mask, y0, text, t = inputs(c)
    if c.items:
        return eng.sample_items(cond, mask, y0, text, [t] * c.B, [c.cfg] * c.B, lens=c.durations())
    return eng.sample(cond, mask, y0, text, t, c.cfg, lens=c.durations())


def reference(prec, c: Call):
    """(out, traj) of the call on the engine built under F5_HIP_GRAPH=0.  Computed once per (precision, call), never modified."""
    if ("eager", prec) not in _cache:
        _cache["eager", prec] = make(prec, graphs=False).engine()
    if ("ref", prec, c) not in _cache:
        eng = _cache["eager", prec]
        out, traj = launch(eng, c)
        _cache["ref", prec, c] = (out.cpu(), traj.cpu())
        s = eng.graph_stats()
        assert s["captures"] == s["replays"] == s["evictions"] == 0, f"the reference engine is not eager: {s}"
    return _cache["ref", prec, c]


def assert_references_distinct(prec, calls):
    """The vacuity guard: calls that differ in nothing but cfg_strength have pairwise different eager results."""
    calls = list(dict.fromkeys(calls))
    smallest = None
    for a, b in itertools.combinations(calls, 2):
        if replace(a, cfg=0.0) != replace(b, cfg=0.0):
            continue
        d = (reference(prec, a)[0] - reference(prec, b)[0]).abs().max().item()
        smallest = d if smallest is None else min(smallest, d)
        assert d > 0, f"{a} and {b} have the same eager result: the comparison could not tell their graphs apart"
    print(f"[graph cache {prec}] smallest pairwise L-inf between the eager references of signatures of one shape: {smallest}")
    return smallest


class Rig:
    """An engine with graphs on beside the model: every event goes to both, the counters must agree after each, and every output
    must equal the eager reference -- at once (a .cpu() per call) or, sync=False, after one synchronisation at the end, which is
    how a server calls: sample() returns without waiting and the next call follows."""

    def __init__(self, prec, *, sync=True, tag=""):
        self.prec, self.sync, self.tag = prec, sync, tag
        self.tr = make(prec)
        self.eng = self.tr.engine()
        self.model = GraphCacheModel(uc_arch=G.uc_arch(ARCH, "DiT"))
        self.pending, self.paths = [], []
        assert self.eng.graph_stats() == st(0, 0, 0, 0)

    def event(self, name, *args, on=None):
        """reserve / set_length_buckets / set_graph_capacity / prepare (the engine's prepare_sample) on both."""
        getattr(on or self.eng, {"prepare": "prepare_sample"}.get(name, name))(*args)
        _, want = getattr(self.model, name)(*args)
        got = self.eng.graph_stats()
        print(f"[graph cache {self.prec}{self.tag}] {name}{args}: {got}")
        assert got == want, f"after {name}{args}: the engine counts {got}, the header's rules give {want}"

    def call(self, c: Call, expect=None):
        before = self.eng.graph_stats()
        out, traj = launch(self.eng, c)
        got = self.eng.graph_stats()   # (four host integers: no device work)
        path, want = (self.model.sample_items if c.items else self.model.sample)(c.sig())
        took = [k for k in ("eager", "captures", "replays") if got[k] != before[k]]
        print(f"[graph cache {self.prec}{self.tag}] call {len(self.paths)} {c}: engine {took}, model {path}, {got}")
        assert got == want, f"call {len(self.paths)} {c}: the engine counts {got}, the header's rules give {want} ({path})"
        assert expect is None or path == expect, f"call {len(self.paths)} {c}: the model says {path}, the test expected {expect}"
        self.paths.append(path)
        self.pending.append((len(self.paths) - 1, c, path, out, traj))
        if self.sync:
            self.compare()
        return path

    def compare(self):
        for i, c, path, out, traj in self.pending:
            r_out, r_traj = reference(self.prec, c)
            d = (traj.cpu() - r_traj).abs().max().item()
            assert torch.equal(traj.cpu(), r_traj), f"call {i} {c} ({path}): the trajectory differs from the eager engine's by {d:.3e}"
            assert torch.equal(out.cpu(), r_out), f"call {i} {c} ({path}): out differs from the eager engine's"
        self.pending = []

    def finish(self, want=None):
        torch.cuda.synchronize()
        self.compare()
        got = self.eng.graph_stats()
        print(f"[graph cache {self.prec}{self.tag}] final counters {got}; paths {self.paths}")
        assert got["captures"] + got["replays"] > 0, "no call was captured or replayed: the graph cache is off"
        assert want is None or got == want
        return got


def batch(i, **kw):
    """Signature i of a family that shares its shape: B = 2 with lengths, guidance 2.0, 2.25, 2.5, ..."""
    return Call(B=2, N=48, cfg=2.0 + 0.25 * i, lens="ragged", **kw)


# ================================================================================================ the yardstick's own anchor
@pytest.mark.parametrize("prec", PRECISIONS)
def test_the_eager_reference_is_anchored_to_the_oracle(prec):
    for c in (Call(B=1, N=48), batch(0)):
        cond, mask, y0, text, t = inputs(c)
        durs = torch.tensor(c.durations() or [c.N])
        o_out, o_traj = O.sample(weights(), ARCH, cond, text, durs if c.B > 1 else c.N, lens=torch.full((c.B,), COND_FRAMES), steps=c.steps,
                                 cfg_strength=c.cfg, sway_sampling_coef=-1.0, y0=y0)
        out, traj = reference(prec, c)
        assert traj.shape == o_traj.shape and out.shape == o_out.shape
        valid = (torch.arange(c.N)[None, :] < durs[:, None])[..., None]   # (frames past an item's own length are nobody's)
        e_traj, e_out = ((traj - o_traj) * valid).abs().max().item(), ((out - o_out) * valid).abs().max().item()
        print(f"[graph cache {prec}] eager engine vs oracle, {c}: traj Linf {e_traj:.3e} out Linf {e_out:.3e}")
        assert e_traj < TOL_PARITY and e_out < TOL_PARITY


# ================================================================================================ FIFO eviction at capacity 16
@pytest.mark.parametrize("sync", [True, False], ids=["cpu_after_every_call", "one_final_sync"])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_fifo_eviction_at_capacity_16(prec, sync):
    """17 signatures, each twice, fill the cache and push the first out; then the first (captured again, pushes out the second), the
    third (resident: replays), the second (captured again, pushes out the third although it has just replayed: FIFO, not LRU) and the
    third once more (captured again).  With sync=False no call is waited for: graphs are destroyed while the stream is still busy,
    which the engine's event behind every launch makes safe."""
    sigs = [batch(i) for i in range(17)]
    assert_references_distinct(prec, sigs)
    rig = Rig(prec, sync=sync, tag="" if sync else " no-sync")
    rig.event("reserve", 2, 48, 2)
    for i, c in enumerate(sigs):
        rig.call(c, "eager")
        rig.call(c, "capture")
        assert rig.eng.graph_stats() == st(i + 1, 0, i + 1, 1 if i == 16 else 0)
    rig.call(sigs[0], "capture")
    rig.call(sigs[2], "replay")
    rig.call(sigs[1], "capture")
    rig.call(sigs[2], "capture")
    rig.call(sigs[16], "replay")
    rig.finish(st(20, 2, 17, 4))


# ================================================================================================ capacity
@pytest.mark.parametrize("prec", PRECISIONS)
def test_capacity_raised_to_20_then_shrunk_to_16(prec):
    sigs = [batch(i) for i in range(20)]
    assert_references_distinct(prec, sigs)
    rig = Rig(prec)
    rig.event("reserve", 2, 48, 2)
    rig.event("set_graph_capacity", 20)
    for c in sigs:
        rig.call(c, "eager")
        rig.call(c, "capture")
    assert rig.eng.graph_stats() == st(20, 0, 20, 0)
    rig.event("set_graph_capacity", 16)
    assert rig.eng.graph_stats() == st(20, 0, 20, 4)
    # the oldest four are gone, the other sixteen are resident: newest first, so that the residents replay before anything is pushed out
    for c in reversed(sigs):
        rig.call(c, "capture" if c in sigs[:4] else "replay")
    for c in sigs[4:8]:   # ... and 3, 2, 1, 0 pushed out 4 .. 7, which now push out 8 .. 11
        rig.call(c, "capture")
    rig.call(sigs[12], "replay")
    rig.finish(st(28, 17, 20, 12))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_wrapper_capacity_survives_set_length_buckets(prec):
    """DiT.set_graph_capacity(32), then DiT.set_length_buckets(32) -- the engine's setter puts the cache back to 16, the wrapper
    applies the 32 again -- and 20 signatures of one bucket are all held."""
    sigs = [Call(B=2, N=48, cfg=2.0 + 0.25 * i, lens="equal") for i in range(20)]
    assert_references_distinct(prec, sigs)
    rig = Rig(prec)
    rig.event("set_graph_capacity", 32, on=rig.tr)
    rig.event("set_length_buckets", 32, on=rig.tr)
    rig.model.set_graph_capacity(32)   # (what the wrapper does behind the engine's setter)
    assert rig.tr.graph_capacity == 32 and rig.tr.length_bucket == 32
    for c in sigs:
        rig.call(c, "eager")
        rig.call(c, "capture")
    for c in sigs:
        rig.call(c, "replay")
    assert rig.finish(st(20, 20, 20, 0))["evictions"] == 0


# ================================================================================================ invalidation without reserve()
BASE = Call(B=1, N=48)
GROWS = {
    "N_48_to_96": Call(B=1, N=96),
    "B_1_to_3": Call(B=3, N=48, lens="ragged"),
    "steps_2_to_6": Call(B=1, N=48, steps=6),
    "text_12_to_40": Call(B=1, N=48, nt=40),
    "first_sample_items": Call(B=1, N=48, items=True),
    "set_length_buckets": None,
}


@pytest.mark.parametrize("what", list(GROWS))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_invalidation_without_reserve(prec, what):
    """A warm, captured, replayed signature; then something grows (or the buckets are switched); then the same signature three more
    times: eager, capture and replay again, each bit-equal to the eager engine -- a graph that survived the clear would read the
    arena as it was laid out before."""
    rig = Rig(prec)
    for path in ("eager", "capture", "replay"):
        rig.call(BASE, path)
    if GROWS[what] is None:
        rig.event("set_length_buckets", 32)
    else:
        rig.call(GROWS[what], "eager")
    for path in ("eager", "capture", "replay"):
        rig.call(BASE, path)
    rig.finish(st(2, 2, 2 if GROWS[what] is None else 3, 0))


# ================================================================================================ the |uc key under eviction
@pytest.mark.parametrize("prec", PRECISIONS)
def test_uncond_embedding_graph_is_evicted_and_comes_back(prec):
    # the preconditions of the kept unconditional embedding: the DiT, an embedding that does not depend on the text, B = 1, guidance on, no lens
    assert not (ARCH["text_mask_padding"] and ARCH["conv_layers"] > 0) and not ARCH.get("text_embedding_average_upsampling")
    assert G.uc_arch(ARCH, "DiT")
    one, long = Call(B=1, N=48), Call(B=1, N=96)
    assert one.B == 1 and one.cfg >= 1e-5 and one.lens is None
    others = [batch(i) for i in range(16)]
    assert_references_distinct(prec, others)
    rig = Rig(prec)
    rig.event("reserve", 2, 96, 2)
    rig.call(one, "eager")      # stores the embedding of N = 48
    rig.call(one, "capture")    # "|uc"
    for c in others:
        rig.call(c, "eager")
        rig.call(c, "capture")
    assert rig.eng.graph_stats() == st(17, 0, 17, 1)   # the 16th pushed "|uc" out
    rig.call(long, "eager")     # stores N = 96
    rig.call(one, "eager")      # must store N = 48 again
    rig.call(one, "capture")    # "|uc" again, pushing out the oldest of the others
    rig.call(one, "replay")
    rig.call(others[0], "capture")
    rig.call(one, "replay")
    rig.finish(st(19, 2, 19, 3))


# ================================================================================================ prepare_sample over 17 buckets
@pytest.mark.parametrize("prec", PRECISIONS)
def test_prepare_over_17_buckets(prec):
    g, n_min, n_max = 8, 32, 160
    ceilings = list(range(n_min, n_max + g, g))
    assert len(ceilings) == 17 and {32, 48, 96} <= set(ceilings)
    rig = Rig(prec)
    rig.event("set_length_buckets", g)
    rig.event("prepare", 1, n_min, n_max, 40, 2, 2.0)
    assert rig.eng.graph_stats() == st(17, 0, 0, 0)
    for k, nc in enumerate(ceilings):   # the ceiling itself, one and two frames below it
        rig.call(Call(B=1, N=nc - k % 3), "replay")
    assert rig.eng.graph_stats() == st(17, 17, 0, 0)   # capacity 17: nothing was pushed out
    stranger = Call(B=1, N=48, cfg=2.25)
    assert_references_distinct(prec, [stranger, Call(B=1, N=48)])
    rig.call(stranger, "eager")
    rig.call(stranger, "capture")                       # pushes out exactly the oldest prepared bucket
    assert rig.eng.graph_stats() == st(18, 17, 1, 1)
    for nc in ceilings[1:4]:
        rig.call(Call(B=1, N=nc), "replay")
    rig.call(Call(B=1, N=30), "capture")                # bucket 32: prepared counts as seen, so it is captured again at once
    rig.call(Call(B=1, N=32), "replay")
    rig.finish(st(19, 21, 1, 2))
