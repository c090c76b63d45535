"""GPU: silence clipping on the device (f5_silence_analyse, f5_wave_gather, infer.clip_prompts / remove_silence and the
`clip_silence` switch) against silence_oracle.py, the literal restatement of pydub on top of audioop.rms.  Everything here is
exact: flags are compared byte for byte, waveforms bit for bit.

The items of the C-level calls are views into one flat buffer whose gaps hold full-scale samples (1.0) in front of, between and
behind them: a read outside an item would add 32767^2 to an energy and flip flags that the oracle, which only ever sees the item,
calls silent.  (NaN would not show: the contract reads NaN as 0; one item carries NaN inside to pin exactly that.)  The gather's
output is over-allocated and NaN-prefilled: a write outside an item's planned range shows in the NaN that is gone."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import silence_oracle as O  # noqa: E402
from gpu_util import DEV  # noqa: E402
from test_silence import LOUD, QUIET, build, four_squares, materialise  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd import silence as S  # noqa: E402

# every window rule the drivers use, plus a detect_silence query whose last start is off the step
QUERIES = ((1000, 10, 103, 0), (100, 10, 327, 0), (10, 10, 260, 1), (1, 1, 260, 1), (300, 7, 103, 0))
GAPS = (17, 3, 10, 1, 6, 5, 4, 9, 2)

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def constant(frames, value, special=None):
    q = np.full((1, frames), value, dtype=np.int16)
    if special is not None:
        q[0, :4] = special
    return q


def make_items():
    """(rate, int16 [C, F] the oracle sees, f32 [C, F_stored] the device sees) per item."""
    T = 103
    rng = np.random.default_rng(11)
    items = []
    # 0: 600 ms at exactly T, then T + 1: rms == T + 1 is not silent, anything below it is
    q = np.concatenate([constant(14400, T), constant(25600, T + 1)], axis=1)
    items.append((24000, q))
    # 1, 2: every sample T + 1 but four, so that the first 1000 ms window sums to cnt * (T + 1)^2 - 1 (silent) / that value (not)
    items.append((24000, constant(36000, T + 1, four_squares(4 * (T + 1) ** 2 - 1))))
    items.append((24000, constant(36000, T + 1)))
    # 3: 44100 Hz (44.1 frames per ms), speech and room noise
    items.append((44100, build(44100, 1, [(120, "q"), (380, "S"), (250, "0"), (157, "S")], seed=3)))
    # 4: stereo 48000 Hz
    items.append((48000, build(48000, 2, [(205, "0"), (200, "S"), (215, "q")], seed=4)))
    # 5: L rounds up (F = 24 L - 11): frames [F, pos(L)) read as zeros
    items.append((24000, build(24000, 1, [(1400, "q")], seed=5)[:, :24 * 1400 - 11]))
    # 6: L rounds down (F = 24 L + 11): the last 11 frames are never read -- they are full scale on the device and in the oracle alike
    q = build(24000, 1, [(1300, "q")], seed=6)
    items.append((24000, np.concatenate([q, np.full((1, 11), 32767, dtype=np.int16)], axis=1)))
    # 7: one frame (L = 0: no flag at all)
    items.append((24000, np.full((1, 1), 20000, dtype=np.int16)))
    # 8: 11025 Hz, odd length
    items.append((11025, build(11025, 1, [(333, "q"), (700, "S"), (777, "q")], seed=8)[:, :-3]))
    out = []
    for k, (rate, q) in enumerate(items):
        x = q.astype(np.float32) / np.float32(32768.0)
        if k == 3:   # NaN reads as 0: the oracle sees zeros there
            q = q.copy()
            q[0, 5000:5100] = 0
            x[0, 5000:5100] = np.nan
        out.append((rate, q, x))
    assert S.ms_len(items[5][1].shape[1], 24000) == 1400 and S.ms_len(items[6][1].shape[1], 24000) == 1300
    assert all(1 <= q.shape[1] <= 40000 for _, q in items)
    return out


def items():
    return cached("items", make_items)


def oracle_flags(q, rate, queries=QUERIES):
    def one(W, s, T, kind):
        seg = O.Segment.from_array(q, rate)
        if kind == 0:
            return O.silence_flags(seg, W, {103: -50, 327: -40}[T], s)
        assert T == 260 and W == s
        return O.leading_flags(seg, -42, W) if W == 10 else O.trailing_flags(seg, -42)
    return cached(("oracle", q.tobytes(), q.shape, rate, queries), lambda: [np.array(one(*qq), dtype=np.uint8) for qq in queries])


def place(arrays, gaps=GAPS, fill=1.0):
    """The f32 arrays as views into one device buffer with `fill` in the gaps; returns (views, the buffer)."""
    sizes = [a.size for a in arrays]
    total = sum(sizes) + sum(gaps[k % len(gaps)] for k in range(len(arrays) + 1))
    host = torch.full((total,), fill, dtype=torch.float32)
    offs, at = [], 0
    for k, a in enumerate(arrays):
        at += gaps[k % len(gaps)]
        host[at:at + a.size] = torch.from_numpy(a.reshape(-1))
        offs.append(at)
        at += a.size
    dev = host.to(DEV)
    return [dev[o:o + n] for o, n in zip(offs, sizes)], dev


def device_flags(specs, queries=QUERIES, qscale=32768.0, tables=None, lens=None, gaps=GAPS):
    views, _keep = place([x for _, _, x in specs], gaps)
    shapes = [x.shape for _, _, x in specs]
    rates = [r for r, _, _ in specs]
    lens = lens if lens is not None else [S.ms_len(f, r) for (_, f), r in zip(shapes, rates)]
    out = I.silence_flags(views, shapes, rates, lens, queries, qscale, tables)
    torch.cuda.synchronize()
    return out


def batch_flags():
    return cached("batch", lambda: device_flags(items()))


@pytest.mark.parametrize("k", range(9))
def test_flags_are_the_oracles(k):
    rate, q, _x = items()[k]
    want = oracle_flags(q, rate)
    got = batch_flags()[k]
    for qi in range(len(QUERIES)):
        assert got[qi].dtype == np.uint8 and got[qi].shape == want[qi].shape, (k, qi)
        assert np.array_equal(got[qi], want[qi]), (k, QUERIES[qi], np.flatnonzero(got[qi] != want[qi])[:8])


def test_the_items_sit_on_the_edges_they_are_named_for():
    f = [oracle_flags(q, r) for r, q, _ in items()]
    assert f[0][0][0] == 1 and f[0][0][60] == 0                   # rms == T is silent; a window of T + 1 alone is not ...
    assert f[0][0][-1] == 1 and f[0][1][0] == 1                   # ... until the zero extension takes 8 of its frames
    assert f[1][0][0] == 1 and f[2][0][0] == 0                    # cnt * (T + 1)^2 - 1 against the value itself
    assert len(f[3][0]) == 0 and len(f[7][3]) == 0                # L < W; one frame
    assert len(f[0][4]) == len(S.query_starts(1667, 300, 7)) and (1667 - 300) % 7 != 0
    assert f[5][3][-1] == 1 and f[6][3][-1] == 1                  # the zero extension; the full-scale frames behind pos(L) are not read


def test_each_item_alone_gives_the_batchs_flags():
    for k, spec in enumerate(items()):
        alone = device_flags([spec], gaps=(k % 4,))[0]             # another alignment than in the batch
        for qi in range(len(QUERIES)):
            assert np.array_equal(alone[qi], batch_flags()[k][qi]), (k, qi)


def test_vector_and_element_loads_agree():
    q = build(24000, 2, [(300, "q"), (400, "S"), (100, "0"), (700, "q")], seed=21)
    assert q.shape[1] % 4 == 0
    x = q.astype(np.float32) / np.float32(32768.0)
    want = oracle_flags(q, 24000)
    for gap in (0, 4, 1, 3):                                       # 16-byte aligned rows twice, then not
        got = device_flags([(24000, q, x)], gaps=(gap,))[0]
        for qi in range(len(QUERIES)):
            assert np.array_equal(got[qi], want[qi]), (gap, qi)


def test_generated_wave_scale_32767():
    x = (np.random.default_rng(9).standard_normal((1, 30000)) * 0.004).astype(np.float32)
    x[0, 7000:9000] *= 40
    x[0, 100] = 3.0                                                # clamps to 32767
    x[0, 101] = -3.0
    q = O.quantise(x, 32767.0)
    assert q[0, 100] == 32767 and q[0, 101] == -32768
    got = device_flags([(24000, q, x)], qscale=32767.0)[0]
    for qi, want in enumerate(oracle_flags(q, 24000)):
        assert np.array_equal(got[qi], want), qi


def test_analysis_through_a_segment_table_equals_the_materialised_signal():
    rate = 24000
    q = build(rate, 2, [(200, "S"), (300, "q"), (500, "S"), (250, "0")], seed=31)
    F = q.shape[1]
    pieces = [(5000, 7000), (100, 3000), (-1, 50), (F - 10, 100), (12000, 9000)]      # a gap of silence; a piece that runs past F
    table = S.segment_table(pieces)
    assert len(table) == 4 and table[2] == (10050, F - 10, 100)
    sig = materialise(pieces, q)
    L = S.ms_len(sig.shape[1], rate)
    want = oracle_flags(sig, rate)
    x = q.astype(np.float32) / np.float32(32768.0)
    through = device_flags([(rate, q, x)], tables=[table], lens=[L])[0]
    plain = device_flags([(rate, sig, sig.astype(np.float32) / np.float32(32768.0))])[0]
    for qi in range(len(QUERIES)):
        assert np.array_equal(through[qi], plain[qi]) and np.array_equal(through[qi], want[qi]), qi


# ---------------------------------------------------------------------------------------------------- gather
def c_gather(specs, tables, out_frames, out_starts, capacity, qscale):
    views, _keep = place([x for _, _, x in specs])
    B = len(specs)
    base = min(v.data_ptr() for v in views)
    out = torch.full((capacity + 64,), float("nan"), device=DEV, dtype=torch.float32)
    counts = (C.c_int32 * B)(*[len(t) for t in tables])
    flat = [int(v) for t in tables for seg in t for v in seg]
    _lib.check(_lib.load().f5_wave_gather(C.c_void_p(base), B, (C.c_int64 * B)(*[(v.data_ptr() - base) // 4 for v in views]),
                                          _lib.int_array([x.shape[0] for _, _, x in specs]), _lib.int_array([x.shape[1] for _, _, x in specs]),
                                          float(qscale), counts, (C.c_int32 * max(len(flat), 1))(*flat), _lib.int_array(out_frames),
                                          (C.c_int64 * B)(*out_starts), C.c_void_p(out.data_ptr()), capacity,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "f5_wave_gather")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("qscale", [32768.0, 32767.0])
def test_wave_gather_bits_zeros_and_bounds(qscale):
    rng = np.random.default_rng(41)
    xs = [(rng.standard_normal((c, f)) * 0.3).astype(np.float32) for c, f in ((1, 9000), (2, 5003), (1, 1), (2, 4096))]
    xs[0][0, 10] = np.nan
    xs[0][0, 11] = 5.0
    specs = [(24000, None, x) for x in xs]
    tables = [[(0, 0, 4096), (4100, 8990, 100), (4300, 7, 1900)],          # a hole, and a segment that runs 90 frames past F
              [(3, 5000, 3), (10, 0, 2500)],                               # uncovered head; odd F_out: row 1 starts off 16 bytes
              [],                                                          # nothing covered: all +0.0
              [(0, 0, 4096)]]                                              # a plain aligned copy
    out_frames = [6200, 2511, 5, 4096]
    out_starts = [0, 6200, 6200 + 2 * 2511 + 1, 11232]                     # item 2 starts off 16 bytes
    capacity = 11232 + 2 * 4096
    got = c_gather(specs, tables, out_frames, out_starts, capacity, qscale)
    want = np.full(capacity + 64, np.nan, dtype=np.float32)
    for x, table, n, o in zip(xs, tables, out_frames, out_starts):
        q = O.quantise(x, qscale)
        pieces, at = [], 0
        for dst, src, fr in table:
            pieces += [(-1, dst - at), (src, fr)]
            at = dst + fr
        pieces.append((-1, n - at))
        item = materialise([p for p in pieces if p[1] > 0], q).astype(np.float32) / np.float32(32768.0)
        assert item.shape == (x.shape[0], n)
        want[o:o + item.size] = item.reshape(-1)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))         # bit for bit: +0.0 where nothing is, NaN where nothing was written
    assert np.isnan(got[6200 + 2 * 2511]) and np.isnan(got[capacity:]).all()


# ---------------------------------------------------------------------------------------------------- end to end
DRIVER_PROMPTS = {}   # (filled in further down)
PROMPTS = {
    "rule1": (24000, 1, [(3500, "S"), (1200, "q"), (3500, "S"), (1200, "0"), (4000, "S")]),
    "rule2": (44100, 2, [(1400, "S"), (300, "q")] * 3 + [(1400, "S"), (900, "q")] + [(1400, "S"), (100, "0")] * 3 + [(1400, "S")]),
    "rule3": (24000, 2, [(150, "q"), (12850, "S")]),
    "edges": (11025, 1, [(215, "q"), (2600, "S"), (187, "0")]),
    "silent": (48000, 1, [(1500, "q")]),
}


def prompt(name):
    rate, ch, parts = PROMPTS[name] if name in PROMPTS else DRIVER_PROMPTS[name]
    q = cached(("prompt", name), lambda: build(rate, ch, parts, seed=len(name)))
    return rate, q, torch.from_numpy(q.astype(np.float32) / np.float32(32768.0))


def oracle_clip(name):
    rate, q, _ = prompt(name)

    def run():
        seg, rule = O.clip_prompt(O.Segment.from_array(q, rate))
        if name == "silent":
            seg = O.Segment.silent(50).set_frame_rate(rate).set_channels(q.shape[0])
        return seg.array(), rule
    return cached(("clip", name), run)


def test_clip_prompts_against_the_oracles_pipeline():
    names = list(PROMPTS)
    assert [oracle_clip(n)[1] for n in names] == [1, 2, 3, 0, 0]
    assert all(prompt(n)[1].shape[1] <= 14 * prompt(n)[0] for n in names)
    clipped, frames = I.clip_prompts([prompt(n)[2] for n in names], [prompt(n)[0] for n in names], device=DEV)
    for n, got, f in zip(names, clipped, frames):
        want = oracle_clip(n)[0]
        assert tuple(got.shape) == want.shape and f == want.shape[1], n
        assert np.array_equal(got.cpu().numpy().view(np.int32), (want.astype(np.float32) / np.float32(32768.0)).view(np.int32)), n
    # alone, from the device, in another order: the same bits
    for n in ("edges", "rule2"):
        alone, f = I.clip_prompts([prompt(n)[2].to(DEV)], [prompt(n)[0]])
        assert torch.equal(alone[0], clipped[names.index(n)])
    with pytest.raises(ValueError, match="11025"):
        I.clip_prompts([torch.zeros(1, 8000)], [8000], device=DEV)


def test_prompt_batch_clip_silence_uses_the_clipped_prompts():
    names = ["rule1", "edges", "rule3"]
    ms = P.mel.MelSpec()
    raw = [(prompt(n)[2], prompt(n)[0], "Some reference text.") for n in names]
    pre = [(torch.from_numpy(oracle_clip(n)[0].astype(np.float32) / np.float32(32768.0)), prompt(n)[0], "Some reference text.") for n in names]
    texts = ["The text to speak, item %d." % k for k in range(len(names))]
    got = I.prompt_batch(raw, texts, mel_spec=ms, device=DEV, prompt_on_device=True, clip_silence=True)
    want = I.prompt_batch(pre, texts, mel_spec=ms, device=DEV, prompt_on_device=True)
    unclipped = I.prompt_batch(raw, texts, mel_spec=ms, device=DEV, prompt_on_device=True)
    assert got["lens"] == want["lens"] and got["durations"] == want["durations"] and got["texts"] == want["texts"]
    assert torch.equal(got["cond"], want["cond"]) and torch.equal(got["rms"], want["rms"])
    assert got["lens"][0] < unclipped["lens"][0] and got["durations"][2] < unclipped["durations"][2]
    for k, n in enumerate(names):
        nw = M_resampled(oracle_clip(n)[0].shape[1], prompt(n)[0])
        assert got["lens"][k] == nw // 256 + 1
    with pytest.raises(ValueError, match="prompt_on_device"):
        I.prompt_batch(raw, texts, mel_spec=ms, device=DEV, clip_silence=True)


def M_resampled(n, rate):
    return P.mel.resampled_length(n, rate, 24000)


def test_remove_silence_on_generated_waves():
    rng = np.random.default_rng(51)
    parts = [(1200, 0.1), (1200, 0.0004), (1200, 0.1), (1200, 0.0), (1200, 0.1)]
    x = np.concatenate([(rng.standard_normal(int(24 * ms)) * a).astype(np.float32) for ms, a in parts])
    quiet = (rng.standard_normal(30001) * 0.0003).astype(np.float32)
    assert x.shape[0] == 6 * 24000

    def want_of(w):
        seg = O.remove_silence_for_generated_wav(O.Segment.from_array(O.quantise(w[None], 32767.0), 24000))
        return seg.array()[0].astype(np.float32) / np.float32(32768.0) if seg.frame_count() else np.zeros(0, dtype=np.float32)

    want = [want_of(x), want_of(quiet)]
    assert 0 < want[0].shape[0] < x.shape[0] - 2 * 150 * 24 and want[1].shape[0] == 0
    waves, lens = I.remove_silence([torch.from_numpy(x).to(DEV), torch.from_numpy(quiet).to(DEV)])
    assert lens == [w.shape[0] for w in want]
    for g, w in zip(waves, want):
        assert np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32))
    packed = torch.full((2, x.shape[0] + 7), float("nan"), device=DEV)
    packed[0, :x.shape[0]] = torch.from_numpy(x)
    packed[1, :quiet.shape[0]] = torch.from_numpy(quiet)
    waves2, lens2 = I.remove_silence(packed, [x.shape[0], quiet.shape[0]])
    assert lens2 == lens and torch.equal(waves2[0], waves[0])


# ---------------------------------------------------------------------------------------------------- the drivers
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
DRIVER_PROMPTS = {"short": (24000, 2, [(100, "0"), (1500, "S"), (1200, "q"), (800, "S"), (300, "q")])}


def tiny_model():
    def make():
        tr = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
        return P.CFM(transformer=tr).to(DEV)                               # no vocab map: utf-8 byte tokens
    return cached("model", make)


def tiny_vocoder():
    return cached("voc", lambda: P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV))


def oracle_audio(name):
    return torch.from_numpy(oracle_clip(name)[0].astype(np.float32) / np.float32(32768.0))


def test_synthesize_prompts_with_the_switches():
    names, texts = ["edges", "short"], ["I am the wind.", "Yes, indeed."]
    model, voc = tiny_model(), tiny_vocoder()
    raw = [(prompt(n)[2], prompt(n)[0], "Some call me nature.") for n in names]
    pre = [(oracle_audio(n), prompt(n)[0], "Some call me nature.") for n in names]
    want = I.synthesize_prompts(model, voc, pre, texts, prompt_on_device=True, **KW)
    got = I.synthesize_prompts(model, voc, raw, texts, prompt_on_device=True, clip_silence=True, **KW)
    plain = I.synthesize_prompts(model, voc, raw, texts, prompt_on_device=True, **KW)
    for i in range(2):
        assert torch.equal(got[0][i].view(torch.int32), want[0][i].view(torch.int32)) and torch.equal(got[2][i], want[2][i]), i
    assert got[0][0].shape != plain[0][0].shape                            # the clipped prompt is shorter: another duration
    cut = I.synthesize_prompts(model, voc, raw, texts, prompt_on_device=True, clip_silence=True, remove_silence=True, **KW)
    again, lens = I.remove_silence(want[0])
    for i in range(2):
        assert cut[0][i].shape[0] == lens[i] and torch.equal(cut[0][i].view(torch.int32), again[i].view(torch.int32)), i
        assert torch.equal(cut[2][i], want[2][i])
    with pytest.raises(ValueError, match="prompt_on_device"):
        I.synthesize_prompts(model, voc, raw, texts, clip_silence=True, **KW)


def test_batched_infer_process_with_the_switches():
    model, voc = tiny_model(), tiny_vocoder()
    rate, _q, audio = prompt("short")
    text = "I am the wind. Yes, indeed it is so."
    kw = dict(show_info=None, batched=True, prompt_on_device=True, nfe_step=4, seed=3)
    want = I.infer_process((oracle_audio("short"), rate), "Some call me nature.", text, model, voc, **kw)
    got = I.infer_process((audio, rate), "Some call me nature.", text, model, voc, clip_silence=True, **kw)
    assert got[1] == want[1] and np.array_equal(got[0].view(np.int32), want[0].view(np.int32)) and np.array_equal(got[2], want[2])
    cut = I.infer_process((audio, rate), "Some call me nature.", text, model, voc, clip_silence=True, remove_silence=True, **kw)
    again = I.remove_silence([torch.from_numpy(want[0]).to(DEV)])[0][0].cpu().numpy()
    assert np.array_equal(cut[0].view(np.int32), again.view(np.int32)) and np.array_equal(cut[2], want[2])
    long = I.synthesize_long((audio, rate), "Some call me nature.", ["I am the wind."], model, voc, prompt_on_device=True,
                             clip_silence=True, nfe_step=4, seed=3)
    ref = I.synthesize_long((oracle_audio("short"), rate), "Some call me nature.", ["I am the wind."], model, voc, prompt_on_device=True,
                            nfe_step=4, seed=3)
    assert torch.equal(long[0].view(torch.int32), ref[0].view(torch.int32))
