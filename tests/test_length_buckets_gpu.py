"""GPU: length-bucketed sample() graphs (f5_set_length_buckets / f5_prepare_sample / f5_graph_stats).

A bucketed call is planned at its length rounded up to the granule and runs the packed (RowPack) body with the true length in the
device tables.  It must give, BIT FOR BIT, what today's eager exact-shape path gives -- torch.equal, no tolerance: the same
kernels compute the same rows with the same reduction order, only the launch geometry around them differs -- and the graph of a
bucket must really be shared by its lengths (f5_graph_stats).  Tiny architectures of the committed fixtures, 3 steps."""
import contextlib
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import f5_tts_amd as P  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402

DEV = "cuda:0"
TOL_PARITY = 1e-3            # tests/test_sample_gpu.py: BASELINE.json north_star, "within 1e-3 mel L-inf"
GRANULE = 32
STEPS = 3
COND_FRAMES = 24
# not a multiple of 4 (RowPack rounds rows up to 4); the bucket ceiling and ceiling + 1; below one 64-key attention tile and across it
LENGTHS = (33, 47, 60, 61, 63, 64, 65, 95, 96)
# descending lengths inside a bucket (stale rows of a longer call sit behind a shorter one); every replay at an N other than the captured one
STREAM = (33, 47, 63, 61, 60, 64, 96, 65, 95, 33)
NT_LONG, NT_SHORT = 40, 14   # text longer than N (N = 33) and shorter; the longest comes first, so the staging capacity never moves
PRECISIONS = ("f32", "f16x3", "f16p", "f16", "bf16")


@contextlib.contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_engine(fixture, prec, *, graphs=True, granule=0):
    """The engine of a fixture's architecture with its synthetic weights; the switches are read when the engine is created."""
    meta, _ = load_golden(fixture)
    cls = P.UNetT if meta.get("backbone", "DiT") == "UNetT" else P.DiT
    tr = cls(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision=prec)
    tr.load_state_dict(synthetic_weights(meta))
    tr.to(DEV)
    with environ(F5_HIP_GRAPH=None if graphs else "0", F5_LEN_BUCKET=None):
        eng = tr.engine()
    if granule:
        tr.set_length_buckets(granule)
    return tr, eng


def inputs(n, batch=1, nvocab=40):
    """Deterministic inputs of one call at length n: 24 prompt frames, noise, a text longer than n at n = 33 and shorter elsewhere
    (the second utterance of a batch is padded with -1)."""
    g = torch.Generator().manual_seed(1000 + n)
    cond = torch.randn(batch, COND_FRAMES, 100, generator=g)
    y0 = torch.randn(batch, n, 100, generator=g)
    nt = NT_LONG if n == 33 else NT_SHORT
    text = torch.randint(0, nvocab - 1, (batch, nt), generator=g)
    if batch > 1:
        text[1, nt - 5:] = -1
    mask = torch.zeros(batch, n, dtype=torch.bool)
    mask[:, :COND_FRAMES] = True
    t = torch.linspace(0, 1, STEPS + 1, dtype=torch.float32)
    t = t + -1.0 * (torch.cos(torch.pi / 2 * t) - 1 + t)
    return cond, mask, y0, text, t.tolist()


def run(eng, n, cfg, method, batch=1):
    cond, mask, y0, text, t = inputs(n, batch)
    out, traj = eng.sample(cond, mask, y0, text, t, cfg, lens=[n] * batch if batch > 1 else None, want_traj=True, method=method)
    torch.cuda.synchronize()
    return out.cpu(), traj.cpu()


@functools.lru_cache(maxsize=None)
def reference(prec, method, cfg, fixture="sample_b1_nfe16", batch=1, lengths=LENGTHS):
    """ref[n] = (out, traj) of today's eager exact-shape path: F5_HIP_GRAPH=0, buckets off.  Computed once, never modified."""
    _, eng = make_engine(fixture, prec, graphs=False)
    ref = {n: run(eng, n, cfg, method, batch) for n in lengths}
    assert eng.graph_stats() == dict(captures=0, replays=0, eager=len(lengths), evictions=0)
    return ref


@functools.lru_cache(maxsize=None)
def bucketed_stream(prec, method, cfg):
    """The stream of test 1 on an engine with granule 32 and graphs on: per call (n, out, traj, stats after the call)."""
    _, eng = make_engine("sample_b1_nfe16", prec, granule=GRANULE)
    eng.reserve(1, max(LENGTHS), STEPS)   # as a server does: an arena that grows mid-stream drops every captured graph
    calls = []
    for n in STREAM:
        out, traj = run(eng, n, cfg, method)
        calls.append((n, out, traj, eng.graph_stats()))
    return calls


COMBOS = [(p, m, c) for p in PRECISIONS for m in ("euler", "midpoint") for c in (2.0, 0.0)]


@pytest.mark.parametrize("prec,method,cfg", COMBOS)
def test_bucketed_stream_is_bit_exact_against_the_eager_exact_path(prec, method, cfg):
    ref = reference(prec, method, cfg)
    for i, (n, out, traj, _) in enumerate(bucketed_stream(prec, method, cfg)):
        assert traj.shape == ref[n][1].shape and out.shape == ref[n][0].shape
        d = (traj - ref[n][1]).abs().max().item()
        print(f"[bucket {prec} {method} cfg {cfg}] call {i} N={n}: traj Linf vs eager exact path {d:.3e}")
        assert torch.equal(traj, ref[n][1]), f"call {i} (N={n}): trajectory differs from the exact path by {d:.3e}"
        assert torch.equal(out, ref[n][0]), f"call {i} (N={n}): out differs from the exact path"


@pytest.mark.parametrize("prec,method,cfg", [("f16p", "euler", 2.0), ("f32", "midpoint", 0.0)])
def test_one_graph_per_bucket_is_shared_by_its_lengths(prec, method, cfg):
    calls = bucketed_stream(prec, method, cfg)
    seen = {}
    want = dict(captures=0, replays=0, eager=0, evictions=0)
    for n, _, _, stats in calls:
        bucket = -(-n // GRANULE) * GRANULE
        seen[bucket] = seen.get(bucket, 0) + 1
        # first sighting of a bucket: eager; second: capture (the capturing call launches its graph); every later one: replay
        want["eager" if seen[bucket] == 1 else "captures" if seen[bucket] == 2 else "replays"] += 1
        assert stats == want, f"after N={n} (sighting {seen[bucket]} of bucket {bucket})"
    assert sorted(seen) == [64, 96]
    assert calls[-1][3] == dict(captures=2, replays=6, eager=2, evictions=0)


@pytest.mark.parametrize("prec", ["f32", "f16p"])
def test_batch_of_equal_lengths_and_v1_arch_take_the_bucket(prec):
    """B = 2 with lens == [N, N] on the v1 architecture (text_mask_padding, rotary on every head): eligible, bit-exact, one graph."""
    lengths = (33, 47, 61)   # (the longest text first: the staging capacity never moves)
    ref = reference(prec, "euler", 2.0, "sample_b2_v1arch", 2, lengths)
    _, eng = make_engine("sample_b2_v1arch", prec, granule=GRANULE)
    for n in lengths:
        out, traj = run(eng, n, 2.0, "euler", batch=2)
        assert torch.equal(traj, ref[n][1]) and torch.equal(out, ref[n][0]), f"N={n}"
    assert eng.graph_stats() == dict(captures=1, replays=1, eager=1, evictions=0)


def test_prepared_graphs_replay_on_the_first_call():
    prec, method, cfg = "f16p", "euler", 2.0
    ref = reference(prec, method, cfg)
    tr, eng = make_engine("sample_b1_nfe16", prec, granule=GRANULE)
    tr.prepare_sample(1, 33, 96, NT_LONG, STEPS, cfg, method=method)
    assert eng.graph_stats() == dict(captures=2, replays=0, eager=0, evictions=0)
    for i, n in enumerate((47, 96)):
        out, traj = run(eng, n, cfg, method)
        assert eng.graph_stats() == dict(captures=2, replays=i + 1, eager=0, evictions=0), f"the first call at N={n} must replay"
        assert torch.equal(traj, ref[n][1]) and torch.equal(out, ref[n][0]), f"N={n}"
    tr.prepare_sample(1, 33, 96, NT_LONG, STEPS, cfg, method=method)   # already there: nothing is captured twice
    assert eng.graph_stats(reset=True)["captures"] == 2
    assert eng.graph_stats() == dict(captures=0, replays=0, eager=0, evictions=0)


def fixture_call(name, model, extra=0):
    """The fixture's own CFM.sample call (tests/test_sample_gpu.py run_case), optionally `extra` frames longer."""
    meta, a = load_golden(name)
    dur = meta["duration"]
    dur = dur + extra if isinstance(dur, int) else torch.tensor(dur) + extra
    kw = dict(steps=meta["steps"], cfg_strength=meta["cfg_strength"], sway_sampling_coef=meta["sway"], seed=meta["seed"],
              use_epss=meta["use_epss"], no_ref_audio=meta["no_ref_audio"])
    if meta["lens"] is not None:
        kw["lens"] = torch.tensor(meta["lens"])
    out, traj = model.sample(a["cond"], a["text"], dur, **kw)
    torch.cuda.synchronize()
    return out.cpu(), traj.cpu()


@pytest.mark.parametrize("name", ["sample_b3_attnmask", "sample_b3_masked", "sample_unett_b2"])
def test_ineligible_calls_keep_their_path_and_their_exact_key(name):
    """Ragged batches and the UNetT under granule 32: bit-equal to the same engine with buckets off, keyed per exact shape."""
    tr, eng = make_engine(name, "f16p")
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    base = fixture_call(name, model)
    base_longer = fixture_call(name, model, extra=1)
    eng.set_length_buckets(GRANULE)   # (the engine's own switch: UNetT.set_length_buckets refuses, the engine ignores the UNetT silently)
    eng.graph_stats(reset=True)
    for sighting, want in enumerate((dict(captures=0, replays=0, eager=1, evictions=0), dict(captures=1, replays=0, eager=1, evictions=0),
                                     dict(captures=1, replays=1, eager=1, evictions=0))):
        out, traj = fixture_call(name, model)
        assert torch.equal(out, base[0]) and torch.equal(traj, base[1]), f"sighting {sighting}"
        assert eng.graph_stats() == want
    # one frame more lies in the same bucket of 32 but is another exact shape: its own eager first sighting, no shared graph
    out, traj = fixture_call(name, model, extra=1)
    assert torch.equal(out, base_longer[0]) and torch.equal(traj, base_longer[1])
    assert eng.graph_stats() == dict(captures=1, replays=1, eager=2, evictions=0)


def test_granule_zero_is_the_exact_path():
    """Buckets switched on and off again: exact-shape keys (N = 64 and N = 60 share nothing) and the results of an engine that never had them."""
    ref = reference("f16p", "euler", 2.0)
    _, eng = make_engine("sample_b1_nfe16", "f16p", granule=GRANULE)
    eng.set_length_buckets(0)
    for n in (64, 60, 64, 60):
        out, traj = run(eng, n, 2.0, "euler")
        assert torch.equal(traj, ref[n][1]) and torch.equal(out, ref[n][0]), f"N={n}"
    # (a single-utterance CFG call that finds the cached unconditional text embedding made for another N runs eagerly and stores
    #  its own: alternating lengths never reach a capture on the exact path, which is the behaviour buckets are there to end)
    assert eng.graph_stats() == dict(captures=0, replays=0, eager=4, evictions=0)


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16p"])
def test_fixture_parity_with_a_bucket_wider_than_the_utterance(prec):
    """sample_b1_nfe16 (N = 64) under granule 48 is planned at 96 frames: inside the parity bar of the reference's own vectors."""
    meta, a = load_golden("sample_b1_nfe16")
    tr, eng = make_engine("sample_b1_nfe16", prec, granule=48)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    out, traj = fixture_call("sample_b1_nfe16", model)
    e_out, e_traj = (out - a["out"]).abs().max().item(), (traj - a["traj"]).abs().max().item()
    print(f"[bucket 48, {prec}] sample_b1_nfe16 planned at 96: out Linf {e_out:.3e} traj Linf {e_traj:.3e}")
    assert e_traj < TOL_PARITY and e_out < TOL_PARITY


def test_errors_carry_a_code_and_a_message():
    tr, eng = make_engine("sample_b1_nfe16", "f16p")
    lib = eng.lib

    def err():
        return lib.f5_last_error().decode()

    assert lib.f5_set_length_buckets(eng._h, 12) == -1 and "12" in err()          # F5_EINVAL: not a multiple of 8
    assert lib.f5_set_length_buckets(eng._h, 2048) == -1 and "2048" in err()      # F5_EINVAL: above 1024
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.f5_prepare_sample(eng._h, 1, 33, 96, NT_LONG, STEPS, 2.0, 0, 1, stream) == -3 and "f5_set_length_buckets" in err()   # F5_ESTATE
    with pytest.raises(_lib.F5Error, match="f5_set_length_buckets"):
        tr.prepare_sample(1, 33, 96, NT_LONG, STEPS, 2.0)
    with pytest.raises(ValueError):
        tr.set_length_buckets(12)
    tr.set_length_buckets(GRANULE)
    assert lib.f5_prepare_sample(eng._h, 1, 33, eng.max_pos + 1, NT_LONG, STEPS, 2.0, 0, 1, stream) == -1 and "rotary" in err()      # F5_EINVAL
    tr.set_length_buckets(8)
    assert lib.f5_prepare_sample(eng._h, 1, 8, 8 * 65, NT_LONG, STEPS, 2.0, 0, 1, stream) == -1 and "at most 64" in err()            # 65 buckets
    assert eng.graph_stats() == dict(captures=0, replays=0, eager=0, evictions=0)
