"""GPU: f5_wave_emit against the composition of the two committed yardsticks (emit_oracle: the float64 fold over the join plan, cut
to `settled`, then the delivery fold) bit for bit -- one mixed call of every rate, both formats, final and growing streams, into a
Guarded byte buffer from pieces that lie between NaN --, against the device chain wave_deliver(wave_join(...)), across block
boundaries, tick by tick against at once, alone against in a batch; and infer.open_pool: one client against a session, three
clients replayed from pool.log with the existing parts, the late first chunks, the per-tick counters, cancel and early close."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import deliver_oracle as O  # noqa: E402
import emit_oracle as E  # noqa: E402
from test_long_form_gpu import cached, tiny_model, tiny_vocoder  # noqa: E402
from test_stream_deliver_gpu import CHUNKS, KW, REF_TEXT, SHORT, SPEED, TEXT, lengths, place, signal  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

RATES = (24000, 16000, 8000, 22050, 44100, 48000)
FMT_ID = {"f32": 0, "s16": 1}
NP_TYPE = {"f32": np.float32, "s16": np.int16}


def mel_spec(rates=RATES):
    """One MelSpec for the kernel tests, with the banks of `rates` in its handle."""
    ms = cached("emit mel", lambda: P.mel.MelSpec().to(DEV))
    for rate in rates:
        I.wave_deliver(ms, [torch.zeros(1, device=DEV)], out_rate=rate)          # (uploads the bank on its first use)
    return ms, ms._handle(torch.device(DEV))


# name -> (piece lengths, the fade each piece asks for)
SHAPES = {
    "one": ([4097], [0]),
    "two": ([700, 900], [0, 1]),
    # the 40-sample piece is all fade (n = 40, off = 460) and the next one fades over 100: it starts at 400, in front of it, so pieces
    # 0, 1 and 2 cover [460, 500); the 1-sample piece opens a run and the last piece fades over min(2, R = 1) = 1 sample
    "five": ([500, 40, 600, 1, 300], [0, 100, 100, 0, 2]),
    "tiny": ([8, 3, 3, 3, 20], [0, 6, 6, 6, 6]),
}


def mixed_case():
    """The streams of the mixed call, computed once: dicts with the host pieces (`host`), the device views (`pieces`, filled by
    placed()), and what wave_emit takes."""
    def make():
        specs = []

        def add(shape, rate, fmt, settled, final, rng=None):
            lens, fades = SHAPES[shape]
            total = I.join_plan(lens, fades)[2]
            settled = total + settled if settled <= 0 else settled           # 0: all of it; -k: k samples short of it
            if settled > total:
                return
            ready = O.plan(rate, settled, final)[1]
            o0, o1 = (0, ready) if rng is None else (min(rng[0], ready), max(min(rng[0], ready), ready - rng[1]))
            specs.append(dict(shape=shape, fades=fades, settled=settled, final=final, range=(o0, o1), out_rate=rate, sample_format=fmt,
                              host=[signal(n, seed=1000 * len(specs) + i) for i, n in enumerate(lens)]))

        assert O.geometry(44100)[1] == 147 and O.geometry(16000)[1] == 2
        add("one", 24000, "f32", 0, True)
        add("two", 16000, "s16", -1, False, (3, 0))                           # o0 = 3 is inside a frame of new = 2
        add("five", 22050, "s16", 481, False)
        add("five", 44100, "f32", 0, True, (150, 3))                          # 150 is inside a frame of new = 147
        add("two", 48000, "s16", 8, False)                                    # width + orig samples: the first frame, 2 outputs
        add("one", 8000, "f32", 2500, True, (1, 0))
        add("five", 16000, "f32", 0, True, (5, 10**9))                        # an empty range: (5, 5)
        add("five", 24000, "s16", -100, False, (1, 0))                        # at the stream's rate, growing, three pieces over one sample
        add("tiny", 8000, "s16", 0, True)
        add("tiny", 24000, "f32", 0, True)
        add("one", 44100, "s16", 86, False)                                   # width + orig - 1: nothing is ready, an empty range
        k = 0
        for rate in RATES:                                                    # the lengths at which the window logic changes
            for n in lengths(rate):
                for shape in ("five", "one"):
                    k += 1
                    add(shape, rate, ("f32", "s16")[k % 2], n, k % 3 == 0)
        assert specs[6]["range"] == (5, 5) and specs[10]["range"] == (0, 0)
        assert {s["out_rate"] for s in specs} == set(RATES) and {s["final"] for s in specs} == {True, False}
        assert any(s["range"][0] % O.geometry(s["out_rate"])[1] for s in specs)
        views = iter(place([x for s in specs for x in s["host"]]))
        for s in specs:
            s["pieces"] = [next(views) for _ in s["host"]]
            s["want"] = E.emit(s["host"], s["fades"], s["settled"], s["final"], s["range"], s["out_rate"], s["sample_format"])
            assert s["want"].dtype == NP_TYPE[s["sample_format"]] and len(s["want"]) == s["range"][1] - s["range"][0]
        return specs
    return cached("emit mixed case", make)


def arguments(streams):
    return [{k: s[k] for k in ("pieces", "fades", "settled", "final", "range", "out_rate", "sample_format")} for s in streams]


def emit_call(h, streams, out, cap=None):
    """f5_wave_emit into the Guarded `out` (16-bit words); returns (code, the streams' byte offsets)."""
    S = len(streams)
    pieces = [p for s in streams for p in s["pieces"]]
    first = min(p.data_ptr() for p in pieces)
    i64 = lambda vals: (C.c_int64 * len(vals))(*vals)   # noqa: E731
    at = (C.c_int64 * S)()
    rc = _lib.load().f5_wave_emit(h, C.c_void_p(first), S, _lib.int_array([len(s["pieces"]) for s in streams]),
                                  i64([(p.data_ptr() - first) // 4 for p in pieces]), _lib.int_array([p.shape[0] for p in pieces]),
                                  _lib.int_array([f for s in streams for f in s["fades"]]), i64([s["settled"] for s in streams]),
                                  _lib.int_array([int(s["final"]) for s in streams]), i64([s["range"][0] for s in streams]),
                                  i64([s["range"][1] for s in streams]), _lib.int_array([s["out_rate"] for s in streams]),
                                  _lib.int_array([FMT_ID[s["sample_format"]] for s in streams]), C.c_void_p(out.ptr()),
                                  2 * out.n if cap is None else cap, at, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, list(at)


def test_one_mixed_call_equals_the_oracle_and_touches_nothing_else():
    _, h = mel_spec()
    streams = mixed_case()
    starts, total = E.placement([s["range"] for s in streams], [s["sample_format"] for s in streams])
    assert total % 2 == 0 and any(a > b + E.WIDTH[s["sample_format"]] * len(s["want"]) for a, b, s in zip(starts[1:], starts, streams)), "no gap"
    out = Guarded((total // 2 + 9,), torch.int16)
    rc, at = emit_call(h, streams, out, cap=total)
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().f5_last_error().decode()
    assert at == starts and all(a % 16 == 0 for a in at)
    assert out.guards_intact(), "a guard band was overwritten"
    words = out.bits.cpu().numpy()
    got, untouched = words.view(np.uint8), np.ones(out.n, bool)
    for s, (a, st) in enumerate(zip(at, streams)):
        want = E.as_bytes(st["want"])
        have = got[a:a + len(want)]
        assert np.array_equal(have, want), (f"stream {s} ({st['shape']}, {st['out_rate']} Hz {st['sample_format']}, settled {st['settled']}, "
                                            f"final {st['final']}, range {st['range']}): {int((have != want).sum())} of {len(want)} bytes differ "
                                            f"(first at {int(np.argmax(have != want))})")
        untouched[a // 2:(a + len(want)) // 2] = False
    assert (words[untouched] == np.int16(out.sent)).all(), "a byte outside the streams' ranges was written"


def test_the_mixed_call_equals_the_device_chain():
    ms, _ = mel_spec()
    streams = mixed_case()
    views, buf = I.wave_emit(ms, arguments(streams))
    assert buf.dtype == torch.uint8 and len(views) == len(streams)
    for s, (view, st) in enumerate(zip(views, streams)):
        assert view.dtype == (torch.float32 if st["sample_format"] == "f32" else torch.int16) and view.shape[0] == len(st["want"])
        assert np.array_equal(E.as_bytes(view.cpu().numpy()), E.as_bytes(st["want"])), f"stream {s}: the wrapper's view"
        joined = I.wave_join(st["pieces"], st["fades"])
        chain = I.wave_deliver(ms, [joined[:st["settled"]]], out_rate=st["out_rate"], sample_format=st["sample_format"], ranges=[st["range"]],
                               final=st["final"])[0]
        assert torch.equal(view.view(torch.uint8), chain.view(torch.uint8)), f"stream {s} differs from wave_deliver(wave_join(...)[:settled])"


def test_each_stream_alone_equals_the_same_stream_in_the_mixed_call():
    ms, _ = mel_spec()
    streams = mixed_case()
    views, _ = I.wave_emit(ms, arguments(streams))
    for s, st in enumerate(streams):
        (alone,), buf = I.wave_emit(ms, arguments([st]))
        assert torch.equal(alone, views[s]), f"stream {s} alone differs from the batch"
        assert buf.numel() == max(alone.numel() * alone.element_size(), 1)


@pytest.mark.parametrize("rate, lens, boundary", [
    # at the stream's rate a block is 1024 outputs: the fade [974, 1074) lies across 1024
    (24000, [1074, 2200], 1024),
    # 44.1 kHz: 6 frames of 80 samples a block, its window from 7 samples in front: the fade [420, 520) lies across 480 - 7 = 473
    (44100, [520, 1500], 473),
])
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_a_fade_across_a_block_boundary(rate, lens, boundary, fmt):
    ms, _ = mel_spec((rate,))
    fades = [0, 100]
    offs, ns, total = I.join_plan(lens, fades)
    assert offs[1] < boundary < offs[1] + ns[1], "the fade does not lie across the boundary: the case lost its point"
    host = [signal(n, seed=rate + i) for i, n in enumerate(lens)]
    ready = O.plan(rate, total, True)[1]
    orig, new, _, _ = O.geometry(rate)
    per_block = 1024 if new == 1 else min(max(1, 1024 // new), (8192 - O.geometry(rate)[3]) // orig + 1) * new
    assert ready > 3 * per_block, "fewer than three blocks"
    pieces = place(host)
    for rng in ((0, ready), (per_block // 2 + 1, ready - 5)):                  # the second moves every block's window
        want = E.emit(host, fades, total, True, rng, rate, fmt)
        (got,), _ = I.wave_emit(ms, [dict(pieces=pieces, fades=fades, settled=total, final=True, range=rng, out_rate=rate, sample_format=fmt)])
        assert np.array_equal(E.as_bytes(got.cpu().numpy()), E.as_bytes(want)), (rate, fmt, rng)


@pytest.mark.parametrize("rate, fmt", [(16000, "s16"), (16000, "f32"), (44100, "s16"), (44100, "f32")])
def test_a_stream_emitted_tick_by_tick_equals_the_finished_stream_emitted_once(rate, fmt):
    ms, _ = mel_spec((rate,))
    fade, lens = 100, [1300, 700, 40, 2100]                                    # the 40-sample piece is shorter than the fade
    host = [signal(n, seed=rate + 7 * i) for i, n in enumerate(lens)]
    pieces = place(host)
    fades = [0] + [fade] * (len(lens) - 1)
    total = I.join_plan(lens, fades)[2]
    whole_range = (0, O.plan(rate, total, True)[1])
    (whole,), _ = I.wave_emit(ms, [dict(pieces=pieces, fades=fades, settled=total, final=True, range=whole_range, out_rate=rate, sample_format=fmt)])
    assert np.array_equal(E.as_bytes(whole.cpu().numpy()), E.as_bytes(E.emit(host, fades, total, True, whole_range, rate, fmt)))
    sent, got = 0, []
    for k in range(1, len(lens) + 1):
        last = k == len(lens)
        so_far = I.join_plan(lens[:k], fades[:k])[2]
        settled = so_far if last else so_far - fade
        ready = I.deliver_plan(rate, settled, last)[1]
        assert ready >= sent
        (part,), _ = I.wave_emit(ms, [dict(pieces=pieces[:k], fades=fades[:k], settled=settled, final=last, range=(sent, ready), out_rate=rate,
                                           sample_format=fmt)])
        got.append(part)
        sent = ready
    assert sent == whole.shape[0] and torch.equal(torch.cat(got), whole), "a stream emitted as it grew differs from one call"


# ------------------------------------------------------------------------------------------------ the pool
def voices():
    """Three voices of different length, RMS 0.05 < target_rms: the rescale runs, and a batch holds prompts of unequal length."""
    def noise(n, seed):
        return torch.randn(1, n, generator=torch.Generator().manual_seed(seed)) * 0.05
    return {"main": dict(ref_audio=(noise(24000, 5), 24000), ref_text=REF_TEXT), "b": dict(ref_audio=(noise(19200, 6), 24000), ref_text=REF_TEXT),
            "c": dict(ref_audio=(noise(30000, 7), 24000), ref_text=REF_TEXT)}


def bank_of(model, masked):
    return cached(("pool bank", masked), lambda: I.prepare_voices(model, voices()))


def same_packets(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(E.as_bytes(a), E.as_bytes(b)), f"packet {k}"


@pytest.mark.parametrize("budget, fade, rate, fmt", [(False, 0.0, 24000, "f32"), (False, 0.15, 16000, "s16"), (True, 0.0, 44100, "s16"),
                                                     (True, 0.15, 22050, "f32")])
def test_one_client_is_a_session(budget, fade, rate, fmt):
    model, voc = tiny_model(False), tiny_vocoder()
    bank = bank_of(model, False)
    probe = I.open_stream(model, voc, (bank, "main"), speed=SPEED, **KW)
    ends = probe.plan(TEXT)["ends"]
    batch_frames = 3 * max(ends[1:4]) if budget else None
    kw = dict(out_rate=rate, sample_format=fmt, chunk_size=1000, cross_fade_duration=fade, speed=SPEED)
    session = I.open_stream(model, voc, (bank, "main"), batch_frames=batch_frames, **kw, **KW)
    want = [[p for p, _ in session.stream(TEXT)] for _ in range(2)]             # a first package, then the same client again
    pool = I.open_pool(model, voc, bank, batch_frames=batch_frames, **KW)
    client = pool.connect("main", **kw)
    for text_round in range(2):
        req = client.submit(TEXT)
        got = []
        for r, packet, out_rate in pool.run():
            assert r is req and out_rate == rate
            got.append(packet)
        assert req.done and pool.idle()
        same_packets(got, want[text_round])
    if budget:
        assert [[k for _, k in tick] for tick in pool.log[:3]] == [[0], [1, 2, 3], [4]], "the ticks of one client are a session's groups"
    else:
        assert all(len(tick) == 1 for tick in pool.log)


TEXTS = {"main": TEXT, "b": " ".join(CHUNKS[:3]), "c": SHORT + " " + CHUNKS[0]}
CLIENTS = {"main": dict(out_rate=16000, sample_format="s16"), "b": dict(out_rate=24000, sample_format="f32", cross_fade_duration=0.15),
           "c": dict(out_rate=44100, sample_format="s16", chunk_size=700)}


def pool_run(masked):
    """Three clients of three voices; the second and third submit after the first tick.  Returns what the tests read, computed once."""
    def make():
        model, voc = tiny_model(masked), tiny_vocoder()
        bank = bank_of(model, masked)
        counts = dict(sample=0, decode=0, emit=0, join=0, deliver=0)
        mels, per_tick = [], []
        real_sample, real_decode, real_emit, real_join, real_deliver = model.sample, voc.decode_ragged, I.wave_emit, I.wave_join, I.wave_deliver

        def sample(*a, **k):
            counts["sample"] += 1
            out = real_sample(*a, **k)
            mels.append(out[0])
            return out

        def counting(name, fn):
            def call(*a, **k):
                counts[name] += 1
                return fn(*a, **k)
            return call

        model.sample, voc.decode_ragged = sample, counting("decode", real_decode)
        I.wave_emit, I.wave_join, I.wave_deliver = counting("emit", real_emit), counting("join", real_join), counting("deliver", real_deliver)
        try:
            pool = I.open_pool(model, voc, bank, batch_frames=1500, **KW)
            clients = {name: pool.connect(name, speed=SPEED, **kw) for name, kw in CLIENTS.items()}
            reqs, packets = {"main": clients["main"].submit(TEXTS["main"])}, {}
            while not pool.idle():
                before, stats = dict(counts), pool.stats()
                out = pool.step()
                per_tick.append(({k: counts[k] - before[k] for k in counts}, {k: pool.stats()[k] - stats[k] for k in stats}))
                for r, pk in out:
                    packets.setdefault(r.id, []).extend(pk)
                if len(per_tick) == 1:
                    reqs["b"], reqs["c"] = clients["b"].submit(TEXTS["b"]), clients["c"].submit(TEXTS["c"])
        finally:
            del model.sample, voc.decode_ragged
            I.wave_emit, I.wave_join, I.wave_deliver = real_emit, real_join, real_deliver
        return dict(pool=pool, reqs=reqs, packets=packets, mels=mels, per_tick=per_tick, bank=bank)
    return cached(("pool run", masked), make)


def test_three_clients_replayed_from_the_log_with_the_existing_parts():
    model, voc = tiny_model(False), tiny_vocoder()
    run = pool_run(False)
    pool, reqs, bank = run["pool"], run["reqs"], run["bank"]
    by_id = {r.id: r for r in reqs.values()}
    chunk_counts = {name: len(r.plan["chunks"]) for name, r in reqs.items()}
    assert len(set(chunk_counts.values())) == 3, chunk_counts
    assert len(set(bank.frames)) == 3 and all(r.done for r in reqs.values()) and pool.idle()
    # the late first chunks ran in the tick after their submission, ahead of the first client's remaining chunks
    assert pool.log[0] == [(reqs["main"].id, 0)] and pool.log[1] == [(reqs["b"].id, 0), (reqs["c"].id, 0)]
    assert any(len(tick) > 1 and len({rid for rid, _ in tick}) > 1 for tick in pool.log[2:]), "no tick mixes clients: the case lost its point"
    assert sorted(it for tick in pool.log for it in tick) == sorted((r.id, k) for r in reqs.values() for k in range(len(r.plan["chunks"])))
    # the recomputation: model.sample on the logged batch, decode_ragged, rescale_to_prompt, wave_join, wave_deliver(final=True)
    pieces = {rid: [] for rid in by_id}
    with torch.inference_mode():
        for tick in pool.log:
            items = [(by_id[rid], k) for rid, k in tick]
            glens = [bank.frames[r.voice] for r, _ in items]
            rows = torch.tensor([r.voice for r, _ in items], device=DEV)
            generated, _ = model.sample(cond=bank.mel[:, :max(glens)].index_select(0, rows), text=[r.plan["texts"][k] for r, k in items],
                                        duration=torch.tensor([r.plan["durations"][k] for r, k in items]), lens=torch.tensor(glens),
                                        steps=KW["nfe_step"], cfg_strength=KW["cfg_strength"], sway_sampling_coef=KW["sway_sampling_coef"],
                                        seed=KW["seed"])
            wave, wave_lens = voc.decode_ragged(generated.to(torch.float32).permute(0, 2, 1), ends=[r.plan["ends"][k] for r, k in items],
                                                starts=[bank.samples[r.voice] // 256 for r, _ in items])
            wave = I.rescale_to_prompt(wave, bank.rms.index_select(0, rows)[:, None], bank.target_rms)
            for b, (r, _) in enumerate(items):
                pieces[r.id].append(wave[b, :wave_lens[b]])
        for name, r in reqs.items():
            c = r.client
            joined = I.wave_join(pieces[r.id], [0] + [c.fade] * (len(pieces[r.id]) - 1))
            want = I.wave_deliver(model.mel_spec, [joined], out_rate=c.out_rate, sample_format=c.sample_format, final=True)[0].cpu().numpy()
            got = np.concatenate(run["packets"][r.id])
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(E.as_bytes(got), E.as_bytes(want)), name
            assert all(len(p) <= c.chunk_size for p in run["packets"][r.id])
    assert reqs["b"].client.fade == 3600 and CLIENTS["c"]["chunk_size"] == 700


def test_per_tick_there_is_one_sample_one_decode_one_emit_and_at_most_one_copy():
    run = pool_run(False)
    assert len(run["per_tick"]) == len(run["pool"].log) >= 4
    for calls, stats in run["per_tick"]:
        assert calls == dict(sample=1, decode=1, emit=1, join=0, deliver=0), calls
        assert (stats["ticks"], stats["sample_calls"], stats["decode_calls"], stats["emit_launches"]) == (1, 1, 1, 1) and stats["copies"] <= 1
    stats = run["pool"].stats()
    assert stats["packets"] == sum(len(p) for p in run["packets"].values()) and stats["prompt_passes"] == 0
    assert stats["ticks"] == len(run["pool"].log)


def test_a_requests_mel_rows_equal_the_chunks_run_alone_under_masked_attention():
    model = tiny_model(True)
    run = pool_run(True)
    pool, bank = run["pool"], run["bank"]
    by_id = {r.id: r for r in run["reqs"].values()}
    assert any(len(tick) > 1 for tick in pool.log)
    with torch.inference_mode():
        for tick, generated in zip(pool.log, run["mels"]):
            for b, (rid, k) in enumerate(tick):
                r = by_id[rid]
                frames = bank.frames[r.voice]
                alone, _ = model.sample(cond=bank.mel[:, :frames].index_select(0, torch.tensor([r.voice], device=DEV)), text=[r.plan["texts"][k]],
                                        duration=torch.tensor([r.plan["durations"][k]]), lens=torch.tensor([frames]), steps=KW["nfe_step"],
                                        cfg_strength=KW["cfg_strength"], sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
                end = r.plan["ends"][k]
                assert torch.equal(generated[b, :end], alone[0, :end]), f"request {rid} chunk {k} in a tick of {len(tick)} rows"


def test_cancel_and_an_early_close_leave_the_pool_usable():
    model, voc = tiny_model(False), tiny_vocoder()
    bank = bank_of(model, False)
    kw = dict(out_rate=16000, sample_format="s16", chunk_size=1000, speed=SPEED)
    want = [p for p, _ in I.open_stream(model, voc, (bank, "main"), **kw, **KW).stream(TEXT)]
    pool = I.open_pool(model, voc, bank, batch_frames=None, **KW)
    # an early close: what was not handed out is kept, and the next run() goes on from there
    req = pool.connect("main", **kw).submit(TEXT)
    gen = pool.run()
    got = [next(gen)[1]]
    gen.close()
    assert not req.done
    got += [p for _, p, _ in pool.run()]
    same_packets(got, want)
    assert req.done and pool.idle()
    # cancel: the chunks that have not started are dropped, the pool goes idle, what came is a prefix of the stream
    req = pool.connect("main", **kw).submit(TEXT)
    first = [p for r, pk in pool.step() for p in pk]
    req.cancel()
    rest = [p for _, p, _ in pool.run()]
    assert req.done and pool.idle() and rest == [] and pool.step() == []
    whole = np.concatenate(want)
    part = np.concatenate(first)
    assert 0 < len(part) < len(whole) and np.array_equal(part, whole[:len(part)])
    assert len(pool.log) == 5 + 1
    # and the pool still serves: a new client's request is the session's
    req = pool.connect("main", **kw).submit(TEXT)
    same_packets([p for _, p, _ in pool.run()], want)
    assert req.done
