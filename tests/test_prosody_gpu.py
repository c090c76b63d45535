"""GPU: f5_mel_align (csrc/dtw.hip) and f5_pitch_track (csrc/pitch.hip) against the float64 restatements of their contracts in
prosody_oracle.py and pitch_oracle.py, then infer.heldout_prosody on a tiny synthetic DiT.

Paths are compared exactly.  That rests on D being bit-equal to the oracle's, as measured for f5_mel_distance; test_prosody.py holds,
on these same fixtures, that no competing candidate is within 2^-39 (relative) of the best one, so that even a last-bit difference
could not flip a choice -- at n_cep 13 and 1, but for 2,049 x 2,100 at n_cep = 1 (prosody_oracle.GAP_EXCEPTIONS), where no fixture
without an exact-arithmetic tie was found; at n_cep = 1 the value itself is asserted bit-equal to the oracle's here, on every case.
The all-tie cases (every frame the same constant, every sum equal) test the tie rule alone.
Pitch tracks are compared bit for bit: every operation of the contract is a correctly rounded f64 add, multiply, divide or compare
in a fixed order.  Every case prints its measured maximum difference."""
import ctypes as C

import numpy as np
import pytest
import torch

import adapter_util as U
import dtw_oracle as O
import pitch_oracle as Y
import prosody_oracle as R
import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_device(pairs):
    return [torch.from_numpy(a).to(DEV) for a, _ in pairs], [torch.from_numpy(b).to(DEV) for _, b in pairs]


def bits(t):
    return t.cpu().view(torch.int64).tolist()


def device_paths(a, b, n_cep=13):
    """mel_alignment, read back: (dist bits, [path as a list of (i, j)] per pair, the raw outputs)."""
    dist, path, start, plen = M.mel_alignment(a, b, n_cep=n_cep)
    host, lens = path.cpu().tolist(), plen.cpu().tolist()
    return bits(dist), [[tuple(c) for c in host[s:s + n]] for s, n in zip(start, lens)], (dist, path, start, plen)


# ---------------------------------------------------------------------------------------------------- f5_mel_align
@pytest.mark.parametrize("n_cep", [13, 1])
@pytest.mark.parametrize("group", list(R.ALIGN_CASES))
def test_paths_equal_the_oracle(group, n_cep):
    pairs = R.case_pairs(group)
    a, b = on_device(pairs)
    dist, paths, _ = device_paths(a, b, n_cep)
    assert dist == bits(M.mel_distance(a, b, n_cep=n_cep))
    for (n, m), (x, y), got, d in zip(R.ALIGN_CASES[group], pairs, paths, dist):
        value, want = R.alignment(x, y, n_cep)
        same = np.float64(value).view(np.int64) == d
        print(f"{group} ({n}, {m}) n_cep {n_cep}: {len(want)} cells, value bit-equal to the oracle: {bool(same)}")
        assert n_cep != 1 or same
        assert got == want, (group, n, m)


def test_all_tie_inputs_follow_the_rule():
    a = [torch.full((n, 100), -3.25, device=DEV) for n, _ in R.ALL_TIE]
    b = [torch.full((m, 100), -3.25, device=DEV) for _, m in R.ALL_TIE]
    for n_cep in (13, 1):
        dist, paths, _ = device_paths(a, b, n_cep)
        assert dist == [0] * len(a) == bits(M.mel_distance(a, b, n_cep=n_cep))
        for (n, m), got in zip(R.ALL_TIE, paths):
            d = np.zeros((n, m))
            assert got == R.path_of(O.accumulate(d, full=True), d), (n, m)


NINE = [(40, 55), (1, 9), (300, 257), (64, 64), (520, 513), (7, 1), (90, 700), (33, 32), (128, 127)]


def nine(seed0):
    return [O.pair(seed0 + 31 * k + n + m, n, m, 100) for k, (n, m) in enumerate(NINE)]


def test_ragged_batch_equals_each_pair_alone(monkeypatch):
    a, b = on_device(nine(5))
    dist, paths, _ = device_paths(a, b)
    for k, (x, y) in enumerate(zip(a, b)):
        d1, p1, _ = device_paths([x], [y])
        assert d1[0] == dist[k] and p1[0] == paths[k], k
    assert [len(p) for p in paths] == [len(R.alignment(x, y)[1]) for x, y in nine(5)]
    # a batch over the cap on back-pointers goes down in several calls: the same outputs (here with the cap at 8 KiB: seven calls)
    monkeypatch.setattr(M, "MAX_TRACE_BYTES", 8192)
    d2, p2, _ = device_paths(a, b)
    assert d2 == dist and p2 == paths


def test_a_nan_in_one_pair_gives_it_no_path_and_leaves_the_others():
    a, b = on_device(nine(8))
    dist, paths, _ = device_paths(a, b)
    for side, k, row in (("a", 4, 300), ("b", 2, 0), ("a", 6, 89)):
        a2, b2 = [t.clone() for t in a], [t.clone() for t in b]
        (a2 if side == "a" else b2)[k][row, 50] = float("nan")
        d2, p2, raw = device_paths(a2, b2)
        assert raw[3].cpu().tolist()[k] == 0 and p2[k] == [] and not np.isfinite(raw[0].cpu()[k].item())
        assert [v for i, v in enumerate(d2) if i != k] == [v for i, v in enumerate(dist) if i != k]
        assert [v for i, v in enumerate(p2) if i != k] == [v for i, v in enumerate(paths) if i != k]


def test_reads_in_place_from_a_strided_view():
    pairs = nine(7)[:4]
    a, b = on_device(pairs)
    dist, paths, _ = device_paths(a, b)
    big = torch.full((4, 320, 128), float("nan"), device=DEV)    # [B, N, mel] of a wider buffer: row stride 128, NaN all around
    view = big[:, :, 14:114]
    starts = [3, 0, 17, 250]
    for k, x in enumerate(a):
        view[k, starts[k]:starts[k] + x.shape[0]] = x
    views = [(view, k, starts[k], x.shape[0]) for k, x in enumerate(a)]
    d2, p2, _ = device_paths(views, b)
    assert d2 == dist and p2 == paths
    d3, p3, _ = device_paths(b, views)                           # the roles swapped: the same value, the mirrored rule
    assert d3 == dist
    for (x, y), got in zip(pairs, p3):
        assert got == R.alignment(y, x)[1]


def raw_align(a, b, dist_ptr, len_ptr, path_ptr, n_cep=13, a_frames=None, b_frames=None):
    base_a, base_b = min(t.data_ptr() for t in a), min(t.data_ptr() for t in b)
    i64 = lambda ts, base: (C.c_int64 * len(ts))(*[(t.data_ptr() - base) // 4 for t in ts])   # noqa: E731
    return _lib.load().f5_mel_align(C.c_void_p(base_a), C.c_void_p(base_b), len(a), i64(a, base_a),
                                    _lib.int_array(a_frames or [t.shape[0] for t in a]), 100, i64(b, base_b),
                                    _lib.int_array(b_frames or [t.shape[0] for t in b]), 100, 100, n_cep, C.c_void_p(dist_ptr), C.c_void_p(len_ptr),
                                    C.c_void_p(path_ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_guard_words_stay_intact_and_refused_calls_write_nothing():
    a, b = on_device(nine(9))
    dist, paths, _ = device_paths(a, b)
    slots = sum(n + m - 1 for n, m in NINE)
    s64, s32 = 0x7FF8A5A5A5A5A5A5, 0x5A5A5A5A
    gd = torch.full((8 + len(a) + 8,), s64, dtype=torch.int64, device=DEV)
    gl = torch.full((8 + len(a) + 8,), s32, dtype=torch.int32, device=DEV)
    gp = torch.full((8 + 2 * slots + 8,), s32, dtype=torch.int32, device=DEV)
    err = lambda: _lib.load().f5_last_error().decode()          # noqa: E731
    with torch.cuda.device(DEV):
        assert raw_align(a, b, gd.data_ptr() + 64, gl.data_ptr() + 32, gp.data_ptr() + 32) == 0
        torch.cuda.synchronize()
        hd, hl, hp = gd.cpu().tolist(), gl.cpu().tolist(), gp.cpu().tolist()
        assert hd[:8] == [s64] * 8 and hd[-8:] == [s64] * 8 and hd[8:-8] == dist
        assert hl[:8] == [s32] * 8 and hl[-8:] == [s32] * 8 and hl[8:-8] == [len(p) for p in paths]
        assert hp[:8] == [s32] * 8 and hp[-8:] == [s32] * 8
        at = 8
        for (n, m), p in zip(NINE, paths):
            assert hp[at:at + 2 * len(p)] == [v for c in p for v in c]
            at += 2 * (n + m - 1)
        for t in (gd, gl, gp):
            t.fill_(s64 if t is gd else s32)
        args = (gd.data_ptr() + 64, gl.data_ptr() + 32, gp.data_ptr() + 32)
        assert raw_align(a, b, *args, n_cep=0) == -1 and "n_cep" in err()
        assert raw_align(a, b, *args, n_cep=100) == -1
        assert raw_align(a, b, *args, a_frames=[40, 0] + [t.shape[0] for t in a[2:]]) == -1 and "pair 1 has a_frames = 0" in err()
        assert raw_align(a, b, args[0], 0, args[2]) == -1 and "path_len" in err()
        assert raw_align(a, b, args[0], args[1], 0) == -1 and "null path" in err()
        assert raw_align(a, b, 0, args[1], args[2]) == -1 and "null out" in err()
        # 17 pairs of 4096 x 4096 frames are 68 MiB of back-pointers, over the 2^26 bytes of one call: refused before the tensors
        # (far smaller than that) are ever read
        big = [4096] * 17
        assert raw_align(a[:1] * 17, b[:1] * 17, *args, a_frames=big, b_frames=big) == -1 and "back-pointers" in err() and "pair 16" in err()
        torch.cuda.synchronize()
    assert gd.cpu().tolist() == [s64] * gd.numel() and gl.cpu().tolist() == [s32] * gl.numel() and gp.cpu().tolist() == [s32] * gp.numel()


# ---------------------------------------------------------------------------------------------------- f5_pitch_track
HOP = 256
TONE = Y.harmonic(220, seed=220)


def signals():
    """name -> f32 wave: the edge lengths (1, hop - 1, hop, hop + 1, one shorter than L = 1,425), the tones, noise, silence (the
    S = 0 branch), a DC offset, a +-1 square wave (exact ties in d')."""
    out = {f"len_{n}": TONE[:n].copy() for n in (1, HOP - 1, HOP, HOP + 1, 1000)}
    out.update({f"tone_{f}": Y.harmonic(f, seed=f) for f in Y.TONES})
    out.update(noise=Y.noise(), zeros=np.zeros(12000, np.float32), dc=np.full(3000, 0.5, np.float32), square=Y.square())
    return out


def as_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def compare_tracks(waves, **kw):
    """One device call for the ragged batch against the oracle item by item; returns the largest |difference| seen."""
    centre, W = kw.get("first_centre", 0), kw.get("window", 1024)
    lo, hi = M.pitch_lags(24000, kw.get("fmin", 60.0), kw.get("fmax", 600.0))
    frames = [max(1, len(x) // HOP + (1 if centre == 0 else 0)) for x in waves.values()]
    f0, ap, got_frames = M.pitch_track([torch.from_numpy(x).to(DEV) for x in waves.values()], frames=frames, **kw)
    assert got_frames == frames
    f0, ap = f0.cpu().numpy(), ap.cpu().numpy()
    worst, at = 0.0, 0
    for (name, x), n in zip(waves.items(), frames):
        w0, wp = Y.track(x, first_centre=centre, frames=n, window=W, tau_min=lo, tau_max=hi, threshold=kw.get("threshold", 0.15))
        g0, gp = f0[at:at + n], ap[at:at + n]
        at += n
        diff = max(np.abs(g0 - w0).max(), np.abs(gp - wp).max())
        worst = max(worst, diff)
        print(f"{name}: {n} frames, {(w0 > 0).sum()} voiced, largest |device - oracle| {diff:.3e}")
        assert np.array_equal(as_bits(g0), as_bits(w0)) and np.array_equal(as_bits(gp), as_bits(wp)), name
    return worst


@pytest.mark.parametrize("first_centre", [0, 128])
def test_tracks_equal_the_oracle_bit_for_bit(first_centre):
    worst = compare_tracks(signals(), first_centre=first_centre)
    print(f"first_centre {first_centre}: measured maximum difference {worst:.3e}")


@pytest.mark.parametrize("window, fmin, fmax", [(64, 1500.0, 12000.0), (2048, 24000 / 1024, 12000.0)])
def test_the_smallest_and_the_largest_window_and_lag_range(window, fmin, fmax):
    assert M.pitch_lags(24000, fmin, fmax) == ((2, 16) if window == 64 else (2, 1024))
    s = signals()
    waves = {k: s[k][:6000] for k in ("len_1", "len_257", "len_1000", "tone_110", "tone_440", "noise", "zeros", "square")}
    waves["high"] = Y.harmonic(3000, seconds=0.1, seed=1, harmonics=2)
    worst = compare_tracks(waves, window=window, fmin=fmin, fmax=fmax)
    print(f"window {window}: measured maximum difference {worst:.3e}")


def test_ragged_batch_of_five_equals_each_item_alone_in_any_order():
    s = signals()
    five = [torch.from_numpy(s[k]).to(DEV) for k in ("tone_155", "len_257", "noise", "square", "tone_523")]
    f0, ap, frames = M.pitch_track(five)
    assert frames == [len(x) // HOP + 1 for x in five]
    pieces = list(zip(f0.cpu().view(torch.int64).split(frames), ap.cpu().view(torch.int64).split(frames)))
    for x, (p0, pa) in zip(five, pieces):
        a0, aa, _ = M.pitch_track([x])
        assert torch.equal(a0.cpu().view(torch.int64), p0) and torch.equal(aa.cpu().view(torch.int64), pa)
    perm = [3, 0, 4, 2, 1]
    g0, ga, gf = M.pitch_track([five[i] for i in perm])
    again = list(zip(g0.cpu().view(torch.int64).split(gf), ga.cpu().view(torch.int64).split(gf)))
    for k, i in enumerate(perm):
        assert torch.equal(again[k][0], pieces[i][0]) and torch.equal(again[k][1], pieces[i][1])
    # rows of a [B, L_max] tensor with lens, as decode_ragged returns them: read in place
    L = max(x.numel() for x in five)
    wav = torch.full((5, L), float("nan"), device=DEV)
    for k, x in enumerate(five):
        wav[k, :x.numel()] = x
    r0, ra, rf = M.pitch_track(wav, [x.numel() for x in five])
    assert rf == frames and torch.equal(r0.cpu().view(torch.int64), f0.cpu().view(torch.int64)) and torch.equal(ra.cpu().view(torch.int64), ap.cpu().view(torch.int64))


def test_a_nan_sample_stays_inside_its_item_and_guard_words_stay_intact():
    s = signals()
    three = [torch.from_numpy(s[k]).to(DEV) for k in ("tone_155", "tone_311", "len_257")]
    f0, ap, frames = M.pitch_track(three)
    bad = [t.clone() for t in three]
    bad[1][5000] = float("nan")
    g0, ga, _ = M.pitch_track(bad)
    keep = torch.ones(sum(frames), dtype=torch.bool)
    keep[frames[0]:frames[0] + frames[1]] = False
    assert torch.equal(g0.cpu().view(torch.int64)[keep], f0.cpu().view(torch.int64)[keep])
    assert torch.equal(ga.cpu().view(torch.int64)[keep], ap.cpu().view(torch.int64)[keep])
    mid = g0.cpu()[frames[0]:frames[0] + frames[1]]
    assert (~torch.isfinite(mid) | (mid == 0)).sum() >= 4         # frames 19 .. 22 hold the sample inside their window: unvoiced
    # the raw call between guard words; a refused call writes nothing
    total, s64 = sum(frames), 0x7FF8A5A5A5A5A5A5
    g = [torch.full((8 + total + 8,), s64, dtype=torch.int64, device=DEV) for _ in range(2)]
    base = min(t.data_ptr() for t in three)

    def raw(window=1024):
        return _lib.load().f5_pitch_track(C.c_void_p(base), 3, (C.c_int64 * 3)(*[(t.data_ptr() - base) // 4 for t in three]),
                                          _lib.int_array([t.numel() for t in three]), 24000, HOP, 0, _lib.int_array(frames), window, 40, 400,
                                          0.15, C.c_void_p(g[0].data_ptr() + 64), C.c_void_p(g[1].data_ptr() + 64),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    with torch.cuda.device(DEV):
        assert raw() == 0
        torch.cuda.synchronize()
        for t, want in zip(g, (f0, ap)):
            h = t.cpu().tolist()
            assert h[:8] == [s64] * 8 and h[-8:] == [s64] * 8 and h[8:-8] == want.cpu().view(torch.int64).tolist()
            t.fill_(s64)
        assert raw(window=4096) == -1 and "window" in _lib.load().f5_last_error().decode()
        torch.cuda.synchronize()
    assert all(t.cpu().tolist() == [s64] * t.numel() for t in g)


# ---------------------------------------------------------------------------------------------------- the driver
ADAPTERS = {"a": (dict(seed=1), U.RECIPE), "b": (dict(seed=2, ranks=8, in_rank=0, blocks=[1], mods=("to_q", "to_v"), scale=2.0, text=True),
                                                  dict(lora_alpha=32, lora_r=16))}
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
PROMPT, TARGET = (20, 24, 18), (38, 42, 56)     # totals 58, 66, 74: one bucket of bucket_prompts, so ONE ragged batch of B = 3


def tiny(prec="f16p", adapters=True):
    arch = dict(P.config.F5TTS_TINY)
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, 40), seed=0)
    tr = P.DiT(**arch, text_num_embeds=40, mel_dim=100, precision=prec)
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    if adapters:
        for name, (kw, scales) in ADAPTERS.items():
            tr.add_adapter(name, U.synth_adapter(sd, arch["depth"], **kw), **scales)
    return model


def vibrato(n, f, depth, rate, seed):
    """n samples of three harmonics around f Hz, the pitch swinging by +-depth at `rate` Hz."""
    g = np.random.default_rng(seed)
    inst = f * (1.0 + depth * np.sin(2 * np.pi * rate * np.arange(n) / 24000.0))
    phase = 2 * np.pi * np.cumsum(inst) / 24000.0
    return (0.3 * sum(np.sin(h * phase + g.uniform(0, 2 * np.pi)) / h for h in (1, 2, 3))).astype(np.float32)


def heldout_items():
    """(prompt_mel, prompt tokens, target_wave, target tokens): the targets are voiced tones with vibrato, a stretch of noise in the
    middle of the second one, so that some cells are voiced on one side only."""
    g = torch.Generator().manual_seed(21)
    items = []
    for k, (p, t) in enumerate(zip(PROMPT, TARGET)):
        n = (t - 1) * HOP + 17 * (k + 1)                          # t frames of the vocos front-end
        wave = vibrato(n, 140.0 + 40 * k, 0.06, 5.0 + k, seed=60 + k)
        if k == 1:
            wave[3000:6000] = Y.noise(seed=9)[:3000]
        items.append((torch.from_numpy(O.random_walk_mel(40 + k, p)), torch.randint(0, 40, (5 + k,), generator=g), torch.from_numpy(wave),
                      torch.randint(0, 40, (7 + 2 * k,), generator=g)))
    return items


class ToneVocoder:
    """decode_ragged's interface, returning prepared tones of the right lengths (a synthetic Vocos only makes noise): item b of call
    c is a tone with vibrato near the targets' pitch, unvoiced at its start."""
    def __init__(self):
        self.calls, self.waves = 0, []

    def decode_ragged(self, mel, ends, starts=None, gain=None):
        lens = [(int(e) - int(s) - 1) * HOP for e, s in zip(ends, starts)]
        host = [vibrato(n, 150.0 + 35 * b + 7 * self.calls, 0.05, 4.0 + b, seed=80 + 10 * self.calls + b) for b, n in enumerate(lens)]
        for w in host:
            w[:1500] = 0.0
        wav = torch.zeros(len(lens), max(lens))
        for b, w in enumerate(host):
            wav[b, :len(w)] = torch.from_numpy(w)
        self.calls += 1
        self.waves.append(host)
        return wav.to(mel.device), lens


def sample_alone(model, items, adapter):
    pad = torch.nn.utils.rnn.pad_sequence
    cond = pad([it[0] for it in items], batch_first=True).to(DEV)
    text = pad([torch.cat([it[1], it[3]]) for it in items], padding_value=-1, batch_first=True)
    lens = torch.tensor([it[0].shape[0] for it in items])
    total = torch.tensor([it[0].shape[0] + t for it, t in zip(items, TARGET)])
    model.transformer.set_adapter(adapter)
    out, _ = model.sample(cond, text, total, lens=lens, steps=KW["nfe_step"], cfg_strength=KW["cfg_strength"],
                          sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
    return out.cpu(), P.cfm.clamp_durations(text, lens, total).tolist()


def target_mels(model, items):
    return [model.mel_spec.forward(it[2][None].to(DEV))[0].transpose(0, 1).contiguous().cpu() for it in items]


def test_heldout_prosody_equals_the_oracle_chain():
    model, items, voc = tiny(), heldout_items(), ToneVocoder()
    tmels = target_mels(model, items)
    assert [t.shape[0] for t in tmels] == list(TARGET)
    model.transformer.set_adapter("b")
    got = P.infer.heldout_prosody(model, voc, items, adapters=(None, "a", "b"), **KW)
    assert model.transformer.active_adapter == "b" and voc.calls == 3          # restored; ONE decode per adapter
    mel_items = [(it[0], it[1], t, it[3]) for it, t in zip(items, tmels)]
    dist = P.infer.heldout_distance(model, mel_items, adapters=(None, "a", "b"), **KW)
    t_tracks = [Y.track(it[2].numpy(), frames=t)[0] for it, t in zip(items, TARGET)]
    for c, name in enumerate((None, "a", "b")):
        assert got[name]["mcd"] == dist[name]["mcd"] and [r["mcd"] for r in got[name]["per_item"]] == dist[name]["per_item"]
        out, ends = sample_alone(model, items, name)
        pooled = dict(cells=0, both_voiced=0, vuv_mismatch=0, **{k: 0.0 for k in R.SUMS})
        for u, it in enumerate(items):
            p = it[0].shape[0]
            g_track = Y.track(voc.waves[c][u], frames=ends[u] - p)[0]
            _, path = R.alignment(out[u, p:ends[u]].numpy(), tmels[u].numpy())
            want, have = R.fold(g_track, t_tracks[u], path), got[name]["per_item"][u]
            for k in ("cells", "both_voiced", "vuv_mismatch"):
                assert have[k] == want[k], (name, u, k, have[k], want[k])
            # N terms of magnitude at most T = log2(600)^2 < 86; each term carries the few-ulp log2 of the device (taken as 4 ulp per
            # logarithm, 16 ulp on a product of two with its own rounding), and N additions in any order add N ulp of the running sum
            N = want["both_voiced"]
            bound = N * 86.0 * (N + 16) * 2.0 ** -53
            for k in R.SUMS:
                assert abs(have[k] - want[k]) <= bound, (name, u, k, have[k], want[k], bound)
                pooled[k] += want[k]
            for k in ("cells", "both_voiced", "vuv_mismatch"):
                pooled[k] += want[k]
            print(f"adapter {name} item {u}: {want['cells']} cells, {N} voiced on both sides, {want['vuv_mismatch']} on one")
            assert N > 10 and want["vuv_mismatch"] > 0
        ref = P.infer.prosody_numbers(pooled)
        for k in ("f0_rmse_cents", "f0_corr", "vuv_error"):
            print(f"adapter {name}: {k} {got[name][k]!r} (oracle chain {ref[k]!r})")
            assert np.isfinite(got[name][k]) and abs(got[name][k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k]))
        assert got[name]["f0_rmse_cents"] == 1200.0 * np.sqrt(sum(r["diff2"] for r in got[name]["per_item"]) /
                                                              sum(r["both_voiced"] for r in got[name]["per_item"]))
    model.transformer.set_adapter("b")
    with pytest.raises(Exception):
        P.infer.heldout_prosody(model, ToneVocoder(), items, adapters=("a", "no such adapter"), **KW)
    assert model.transformer.active_adapter == "b"


def test_heldout_prosody_adds_no_eager_bodies_and_runs_with_the_real_tiny_vocos():
    model, items = tiny(adapters=False), heldout_items()
    voc = P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV)
    first = P.infer.heldout_prosody(model, voc, items, **KW)[None]             # (captures whatever sample() captures)
    tr = model.transformer
    tr.graph_stats(reset=True)
    sample_alone(model, items, None)
    alone = tr.graph_stats(reset=True)
    again = P.infer.heldout_prosody(model, voc, items, **KW)[None]
    scored = tr.graph_stats(reset=True)
    print(f"real tiny Vocos: mcd {again['mcd']:.6f} dB, rmse {again['f0_rmse_cents']}, corr {again['f0_corr']}, v/uv {again['vuv_error']}; "
          f"sample() alone {alone}, under heldout_prosody {scored}")
    assert scored["eager"] <= alone["eager"] and sum(scored.values()) == sum(alone.values())
    assert np.isfinite(again["mcd"]) and again["mcd"] > 0 and again["mcd"] == first["mcd"]
    voiced = sum(r["both_voiced"] for r in again["per_item"])
    assert (voiced > 0) == bool(np.isfinite(again["f0_rmse_cents"]))          # NaN, not an error, where nothing is voiced on both sides
    assert 0.0 <= again["vuv_error"] <= 1.0 and len(again["per_item"]) == 3
