"""CPU: per-item sampler settings as far as they go without a device -- the time rows of a call (f5k_item_time_rows) against a
restatement and a hand-written table, CFM.sample_items' grids and noise against the oracle's per item, the refusals of
f5_sample_items that are decided before the engine is looked at, and the pool's choice between sample() and sample_items()."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import items_oracle as IO
from oracle import f5_oracle as O

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I

F5_EINVAL = -1
EULER, MIDPOINT = _lib.F5_ODE_EULER, _lib.F5_ODE_MIDPOINT


def grid(steps, sway=None):
    return O.time_grid(steps, sway, True).tolist()


# ------------------------------------------------------------------------------------------------ time rows
@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_time_rows_equal_the_restatement(method):
    lib = _lib.load()
    steps = [3, 1, 2]
    grids = [grid(3, -1.0), grid(1, None), grid(3, -1.0)[:3]]        # items 0 and 2 share a grid as far as item 2 goes
    rc, times, idx = IO.k_item_time_rows(lib, grids, steps, _lib.ODE_METHODS[method])
    assert rc == 0, lib.f5_last_error()
    want_t, want_i = IO.item_time_rows(grids, steps, method)
    assert times.tobytes() == want_t.tobytes() and np.array_equal(idx, want_i)
    evals = 2 if method == "midpoint" else 1
    assert np.array_equal(idx[:evals * 2, 0], idx[:evals * 2, 2]), "items on one grid share their rows"
    assert len(times) < evals * sum(steps), "the shared times are stored once"
    assert (idx[evals:, 1] == 0).all() and (idx[2 * evals:, 2] == 0).all(), "a finished item points at row 0"


def test_time_rows_hand_written():
    lib = _lib.load()
    # exact binary fractions: item 0 steps over 0, .25, .5, 1; item 1 over 0, 1; item 2 over 0, .25, .5
    grids, steps = [[0.0, 0.25, 0.5, 1.0], [0.0, 1.0], [0.0, 0.25, 0.5]], [3, 1, 2]
    rc, times, idx = IO.k_item_time_rows(lib, grids, steps, EULER)
    assert rc == 0 and times.tolist() == [0.0, 0.25, 0.5]
    assert idx.tolist() == [[0, 0, 0], [1, 0, 1], [2, 0, 0]]
    rc, times, idx = IO.k_item_time_rows(lib, grids, steps, MIDPOINT)
    # evaluation-major, item-major: ev 0: 0 (all); ev 1: .125 (item 0), .5 (item 1), .125; ev 2: .25; ev 3: .375; ev 4: .5 (seen); ev 5: .75
    assert rc == 0 and times.tolist() == [0.0, 0.125, 0.5, 0.25, 0.375, 0.75]
    assert idx.tolist() == [[0, 0, 0], [1, 2, 1], [3, 0, 3], [4, 0, 4], [2, 0, 0], [5, 0, 0]]


@pytest.mark.parametrize("method", ["euler", "midpoint"])
def test_uniform_time_rows_are_the_time_table(method):
    lib = _lib.load()
    t = grid(5, -1.0)
    rc, times, idx = IO.k_item_time_rows(lib, [t] * 3, [5] * 3, _lib.ODE_METHODS[method])
    assert rc == 0
    f = np.array(t, np.float32)
    if method == "euler":
        want = f[:5]                                                   # the grid's head
    else:
        want = np.stack([f[:5], f[:5] + np.float32(0.5) * (f[1:] - f[:5])], 1).reshape(-1)   # t[i], t[i] + dt/2 interleaved
    assert times.tobytes() == want.astype(np.float32).tobytes()
    assert np.array_equal(idx, np.repeat(np.arange(len(want), dtype=np.int32)[:, None], 3, 1)), "every item maps to the same row"


def test_refusals_name_the_item():
    """The table rules are decided before the engine is looked at (a null handle, as test_ode_midpoint's refusal uses)."""
    lib = _lib.load()

    def call(t, steps, smax, cfg, method=EULER, B=None):
        B = len(steps) if B is None else B
        return lib.f5_sample_items(None, None, 0, None, None, None, 1, (C.c_float * len(t))(*t), _lib.int_array(steps), smax,
                                   (C.c_float * len(cfg))(*cfg), None, B, 8, None, None, None, method)

    ok_t = [0.0, 0.5, 1.0, 0.0, 1.0, 0.0]
    assert call(ok_t, [2, 1], 2, [2.0, 0.0], method=7) == F5_EINVAL and b"unknown ODE method 7" in lib.f5_last_error()
    assert call(ok_t, [2, 0], 2, [2.0, 0.0]) == F5_EINVAL and b"item 1" in lib.f5_last_error()
    assert call(ok_t, [3, 1], 2, [2.0, 0.0]) == F5_EINVAL and b"item 0" in lib.f5_last_error()
    assert call(ok_t, [1, 1], 2, [2.0, 0.0]) == F5_EINVAL and b"steps_max" in lib.f5_last_error()
    assert call([0.0, 0.5, 1.0, 0.0, math.nan, 0.0], [2, 1], 2, [2.0, 0.0]) == F5_EINVAL and b"item 1" in lib.f5_last_error()
    assert call([0.0, math.inf, 1.0, 0.0, 1.0, 0.0], [2, 1], 2, [2.0, 0.0]) == F5_EINVAL and b"item 0" in lib.f5_last_error()
    assert call(ok_t, [2, 1], 2, [2.0, math.nan]) == F5_EINVAL and b"item 1" in lib.f5_last_error()
    # what follows an item's own grid is ignored: the NaN behind item 1's single step is not read; the call gets as far as the engine
    assert call([0.0, 0.5, 1.0, 0.0, 1.0, math.nan], [2, 1], 2, [2.0, 0.0]) == F5_EINVAL and b"null engine" in lib.f5_last_error()
    rc, _, _ = IO.k_item_time_rows(lib, [[0.0, math.nan]], [1], EULER)
    assert rc == F5_EINVAL


# ------------------------------------------------------------------------------------------------ CFM.sample_items on the host
class _Engine:
    def __init__(self):
        self.calls = []

    def sample_items(self, cond, cond_mask, y0, text, t_grids, cfgs, lens=None, want_traj=True, method="euler"):
        self.calls.append(dict(cond=cond, cond_mask=cond_mask, y0=y0, text=text, t_grids=t_grids, cfgs=cfgs, lens=lens, method=method))
        return y0, y0[None]


def host_model():
    m = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))
    eng = _Engine()
    m.transformer.engine = lambda: eng
    m.transformer.clear_cache = lambda: None
    return m, eng


def batch():
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(3, 12, 100, generator=g)
    text = torch.randint(0, 200, (3, 9), generator=g)
    return cond, text, torch.tensor([40, 21, 33]), torch.tensor([12, 7, 9])


def test_grids_and_noise_are_the_oracles_per_item():
    m, eng = host_model()
    cond, text, dur, lens = batch()
    steps, cfgs, sways, seeds = [4, 2, 3], [2.0, 0.0, 0.5], [-1.0, None, -0.5], [3, None, 7]
    m.sample_items(cond, text, dur, lens=lens, steps=steps, cfg_strength=cfgs, sway_sampling_coef=sways, seed=seeds)
    call = eng.calls[0]
    assert call["cfgs"] == cfgs and call["lens"] == dur.tolist() and call["method"] == "euler"
    for b in range(3):
        want = O.time_grid(steps[b], sways[b], True)
        assert torch.tensor(call["t_grids"][b], dtype=torch.float32).numpy().tobytes() == want.numpy().tobytes(), f"grid of item {b}"
    # the oracle's draw, item by item in order, on one generator: an item without a seed goes on from the state the item before it left
    rows = []
    for b in range(3):
        rows.append(O.draw_noise(dur[b:b + 1], 100, seeds[b])[0])
    want = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)
    assert torch.equal(call["y0"], want)
    assert call["cond_mask"].shape == (3, 40) and call["cond_mask"].sum(1).tolist() == lens.tolist()


def test_scalars_broadcast_and_wrong_lengths_are_refused():
    m, eng = host_model()
    cond, text, dur, lens = batch()
    m.sample_items(cond, text, dur, lens=lens, steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    call = eng.calls[0]
    assert call["cfgs"] == [2.0] * 3 and call["t_grids"] == [O.time_grid(3, -1.0, True).tolist()] * 3
    assert torch.equal(call["y0"], O.draw_noise(dur, 100, 3)), "a scalar seed is sample()'s draw"
    m.sample_items(cond, text, dur, lens=lens, steps=[3, 2, 1], cfg_strength=2.0, use_epss=False)
    assert [len(g) - 1 for g in eng.calls[1]["t_grids"]] == [3, 2, 1]
    assert eng.calls[1]["t_grids"][1] == torch.linspace(0, 1, 3).tolist()
    for bad in (dict(steps=[3, 2]), dict(cfg_strength=[1.0] * 4), dict(sway_sampling_coef=[None]), dict(seed=[1, 2])):
        with pytest.raises(ValueError, match="sample_items"):
            m.sample_items(cond, text, dur, lens=lens, **bad)
    with pytest.raises(ValueError, match="steps"):
        m.sample_items(cond, text, dur, lens=lens, steps=[3, 0, 1])
    with pytest.raises(TypeError):
        m.sample_items(cond, text, dur, lens=lens, duplicate_test=True)


# ------------------------------------------------------------------------------------------------ the pool on the host
REF = "Some call me nature, others call me mother nature."
SENT = "The quick brown fox jumps over the lazy dog."


class _Bank:
    names, ref_texts, seconds, samples, frames, speeds, target_rms = ["v", "w"], [REF, REF], [3.0, 10.0], [72000, 240000], [282, 938], [None, 2.0], 0.1
    mel = torch.zeros(2, 938, 100)
    rms = torch.zeros(2)


class _Vocoder:
    def decode_ragged(self, *a, **k):
        raise AssertionError("not reached on the CPU")


class _Stop(Exception):
    pass


def recording_model():
    """A model whose two sampler entry points record their call and end the tick there (the rest of a tick needs the device; the
    tests call pool._enqueue, the tick that step() runs inside the device's context)."""
    m = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))
    calls = []

    def record(name):
        def call(*a, **kw):
            calls.append((name, kw))
            raise _Stop()
        return call

    m.sample, m.sample_items = record("sample"), record("sample_items")
    return m, calls


POOL_KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)


def test_default_clients_run_sample_with_the_pools_settings():
    m, calls = recording_model()
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=20000, first_alone=False, **POOL_KW)
    keys = set(pool.stats())
    for voice in ("v", "w"):
        pool.connect(voice).submit(SENT)
    with pytest.raises(_Stop):
        pool._enqueue()
    (name, kw), = calls
    assert name == "sample" and len(pool.log[0]) == 2
    assert {k: kw[k] for k in ("steps", "cfg_strength", "sway_sampling_coef", "seed")} == dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    # a client that states the pool's own values is a default client
    m, calls = recording_model()
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=20000, first_alone=False, **POOL_KW)
    pool.connect("v", nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3).submit(SENT)
    with pytest.raises(_Stop):
        pool._enqueue()
    assert calls[0][0] == "sample" and set(pool.stats()) == keys


def test_a_client_with_its_own_settings_makes_the_tick_a_sample_items_call():
    m, calls = recording_model()
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=20000, first_alone=False, **POOL_KW)
    keys = set(pool.stats())
    a, b, c = pool.connect("v"), pool.connect("w", nfe_step=2, cfg_strength=0.5), pool.connect("v", sway_sampling_coef=None, seed=None)
    reqs = [a.submit(SENT), b.submit(SENT), c.submit(SENT)]
    with pytest.raises(_Stop):
        pool._enqueue()
    (name, kw), = calls
    assert name == "sample_items"
    own = {reqs[0].id: (4, 2.0, -1.0, 3), reqs[1].id: (2, 0.5, -1.0, 3), reqs[2].id: (4, 2.0, None, None)}
    rows = [own[rid] for rid, _ in pool.log[0]]
    assert len(rows) == 3, "the three first chunks share the tick"
    assert (kw["steps"], kw["cfg_strength"], kw["sway_sampling_coef"], kw["seed"]) == tuple(list(col) for col in zip(*rows))
    assert kw["lens"].tolist() == [_Bank.frames[pool._requests[i].voice] for i in range(3)] and len(kw["text"]) == 3
    assert set(pool.stats()) == keys == {"ticks", "sample_calls", "decode_calls", "emit_launches", "copies", "packets", "prompt_passes"}


def test_connect_refuses_bad_settings():
    m, _ = recording_model()
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=None, **POOL_KW)
    for bad in (dict(nfe_step=0), dict(nfe_step=-3), dict(cfg_strength=math.nan), dict(cfg_strength=math.inf), dict(sway_sampling_coef=math.nan)):
        with pytest.raises(ValueError, match="connect"):
            pool.connect("v", **bad)
    c = pool.connect("v", cfg_strength=0.0, seed=None)
    assert c.sample_kw == dict(steps=4, cfg_strength=0.0, sway_sampling_coef=-1.0, seed=None) and pool.sample_kw["seed"] == 3


def test_batch_drivers_route_sequences_to_sample_items():
    m, calls = recording_model()
    cond, text, dur, lens = batch()

    class _V:
        decode_ragged = None

    with pytest.raises(_Stop):
        I.synthesize_batch(m, _V(), cond, text, dur, lens=lens, steps=4, cfg_strength=2.0)
    with pytest.raises(_Stop):
        I.synthesize_batch(m, _V(), cond, text, dur, lens=lens, steps=[4, 2, 3], cfg_strength=2.0)
    assert [c[0] for c in calls] == ["sample", "sample_items"] and calls[1][1]["steps"] == [4, 2, 3] and calls[0][1]["steps"] == 4
