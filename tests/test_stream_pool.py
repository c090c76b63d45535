"""CPU: the stream pool as far as it goes without a device -- pool_tick's rule as properties over seeded random queues and a few
hand-computed ticks, every refusal of f5_wave_emit decided before the first HIP call, the argument errors of open_pool and
connect, a client's first-package state through submit() and reset(), and the placement arithmetic of emit_plan."""
import copy
import ctypes as C
import random

import pytest
import torch

import emit_oracle as E

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd import stream as S

F5_EINVAL, F5_ESTATE = -1, -3


# ------------------------------------------------------------------------------------------------ pool_tick
def test_pool_tick_hand_computed():
    # three requests past their first chunk, 100-frame chunks, 4 rows of 100 fit: one chunk each, then request 3's second one
    waiting = [(3, 1, [100, 100]), (5, 2, [100]), (9, 1, [100, 100, 100])]
    assert S.pool_tick(waiting, 400, 64, True, 0) == ([(3, 1), (5, 2), (9, 1), (3, 2)], 9)      # (9, 2) did not fit: the cursor is 9
    assert S.pool_tick(waiting, 400, 64, True, 9) == ([(9, 1), (3, 1), (5, 2), (9, 2)], 3)
    assert S.pool_tick(waiting, 400, 64, True, 6) == ([(9, 1), (3, 1), (5, 2), (9, 2)], 3)      # the first id >= 6 is 9
    assert S.pool_tick(waiting, 400, 64, True, 10) == ([(3, 1), (5, 2), (9, 1), (3, 2)], 9)     # past the last id: wraps around
    assert S.pool_tick(waiting, None, 64, True, 0) == ([(3, 1), (5, 2), (9, 1), (3, 2), (9, 2), (9, 3)], 0)   # everything: the cursor stays
    assert S.pool_tick(waiting, None, 2, True, 0) == ([(3, 1), (5, 2)], 9)
    # rows x longest row: 150 joins 100 only while 2 x 150 <= budget
    assert S.pool_tick([(0, 1, [100]), (1, 1, [150])], 299, 64, True, 0) == ([(0, 1)], 1)
    assert S.pool_tick([(0, 1, [100]), (1, 1, [150])], 300, 64, True, 0) == ([(0, 1), (1, 1)], 0)
    # an item over the budget runs alone; nothing overtakes the item that did not fit
    assert S.pool_tick([(0, 1, [900, 10]), (1, 1, [10])], 400, 64, True, 0) == ([(0, 1)], 1)
    assert S.pool_tick([(0, 1, [100]), (1, 1, [900]), (2, 1, [100])], 400, 64, True, 0) == ([(0, 1)], 1)
    # a waiting first chunk keeps later chunks out: first chunks only, in submission order, the cursor untouched
    waiting = [(3, 1, [100, 100]), (5, 0, [50, 100]), (9, 0, [60])]
    assert S.pool_tick(waiting, 400, 64, True, 3) == ([(5, 0), (9, 0)], 3)
    assert S.pool_tick(waiting, 100, 64, True, 3) == ([(5, 0)], 3)
    assert S.pool_tick(waiting, 400, 64, False, 3) == ([(3, 1), (5, 0), (9, 0), (3, 2)], 5)
    assert S.pool_tick([], 400, 64, True, 7) == ([], 7) and S.pool_tick([(1, 2, [])], 400, 64, True, 7) == ([], 7)


def random_queue(rng, first_id=0):
    rid, queue = first_id, []
    for _ in range(rng.randint(1, 7)):
        rid += rng.randint(1, 3)
        queue.append((rid, rng.choice([0, 0, 1, 2, 5]), [rng.choice([40, 90, 100, 250, 700]) for _ in range(rng.randint(1, 6))]))
    return queue


@pytest.mark.parametrize("seed", range(40))
def test_pool_tick_properties_over_random_queues(seed):
    rng = random.Random(seed)
    queue = random_queue(rng)
    batch_frames, max_items = rng.choice([None, 100, 300, 600, 2000]), rng.choice([1, 2, 3, 8, 64])
    first_alone, cursor = rng.random() < 0.7, rng.randint(0, 12)
    previous, ticks, left = None, 0, sum(len(w[2]) for w in queue)
    while queue:
        before = copy.deepcopy(queue)
        items, new_cursor = S.pool_tick(queue, batch_frames, max_items, first_alone, cursor)
        assert queue == before, "pool_tick changed its input"
        assert (items, new_cursor) == S.pool_tick(copy.deepcopy(queue), batch_frames, max_items, first_alone, cursor), "not deterministic"
        frames_of = {(rid, k + j): f for rid, k, fr in queue for j, f in enumerate(fr)}
        assert items and len(set(items)) == len(items) and all(it in frames_of for it in items), "no progress, or an item that does not wait"
        # both budgets; the oversize item alone
        rows, longest = len(items), max(frames_of[it] for it in items)
        assert rows <= max_items
        assert rows == 1 or batch_frames is None or rows * longest <= batch_frames, (items, batch_frames)
        # order inside a request: its chunks from its first waiting one on, without a gap, ascending in row order
        for rid, k, _ in queue:
            own = [c for r, c in items if r == rid]
            assert own == list(range(k, k + len(own))), (rid, k, own)
        # first chunks first
        firsts = [rid for rid, k, _ in queue if k == 0]
        round_robin = not (first_alone and firsts)
        if not round_robin:
            assert all(k == 0 for _, k in items) and [r for r, _ in items] == firsts[:rows] and new_cursor == cursor
        # the fairness bound: of two requests that wait through two round-robin ticks in a row, one never gets rows in both while
        # the other gets none
        served = {r for r, _ in items}
        waited = {rid for rid, _, _ in queue}
        if round_robin and previous is not None:
            for x in (previous["waited"] & waited) - previous["served"] - served:
                assert not (previous["served"] & served), f"request {x} was passed over twice in a row for {previous['served'] & served}"
        previous = dict(served=served, waited=waited) if round_robin else None
        # the tick is applied; now and then a new request arrives
        queue = [(rid, k + sum(1 for r, _ in items if r == rid), fr[sum(1 for r, _ in items if r == rid):]) for rid, k, fr in queue]
        queue = [w for w in queue if w[2]]
        cursor, ticks, left = new_cursor, ticks + 1, left - rows
        if rng.random() < 0.25 and ticks < 30:
            more = random_queue(rng, first_id=max([w[0] for w in queue], default=cursor) + 1)[:2]
            queue, left = queue + more, left + sum(len(w[2]) for w in more)
    assert left == 0


# ------------------------------------------------------------------------------------------------ f5_wave_emit's refusals
@pytest.fixture(scope="module")
def unloaded_handle():
    h = C.c_void_p()
    assert _lib.load().f5_mel_create(1024, 256, 100, C.byref(h)) == 0       # host bookkeeping only: no table, no bank
    return h


def test_emit_refusals_without_a_device(unloaded_handle):
    """Every refusal is decided before the first HIP call; the pointers are never dereferenced on the way."""
    lib = _lib.load()
    h = unloaded_handle
    buf = (C.c_float * 4)()
    ptr = C.cast(buf, C.c_void_p)
    at = (C.c_int64 * 2)(-9, -9)
    # stream 0: pieces of 100 and 50 samples, the second fading over 10: total 140, final, 16 kHz s16: ceil(280 / 3) = 94 samples,
    # 188 bytes.  stream 1: one piece of 13 samples, growing, 16 kHz f32: 2 samples ready, 8 bytes at 192.  200 bytes in all.
    def call(m=h, base=ptr, S=2, counts=(2, 1), starts=(0, 100, 150), lens=(100, 50, 13), fades=(0, 10, 0), settled=(140, 13), fin=(1, 0),
             o0=(0, 0), o1=(94, 2), rates=(16000, 16000), fmts=(1, 0), out=ptr, cap=200, at_out=at):
        i64 = lambda v: None if v is None else (C.c_int64 * len(v))(*v)   # noqa: E731
        i32 = lambda v: None if v is None else _lib.int_array(v)          # noqa: E731
        return lib.f5_wave_emit(m, base, S, i32(counts), i64(starts), i32(lens), i32(fades), i64(settled), i32(fin), i64(o0), i64(o1),
                                i32(rates), i32(fmts), out, cap, at_out, None)

    def refused(rc, *words):
        msg = lib.f5_last_error()
        assert rc == F5_EINVAL, (rc, msg)
        assert msg.startswith(b"f5_wave_emit:") and all(w in msg for w in words), msg

    refused(call(m=None), b"m")
    refused(call(base=None), b"base")
    refused(call(counts=None), b"piece_count_host")
    refused(call(starts=None), b"start_host")
    refused(call(lens=None), b"lens_host")
    refused(call(fades=None), b"fade_host")
    refused(call(settled=None), b"settled_host")
    refused(call(fin=None), b"final_host")
    refused(call(o0=None), b"o0_host")
    refused(call(o1=None), b"o1_host")
    refused(call(rates=None), b"rate_host")
    refused(call(fmts=None), b"format_host")
    refused(call(out=None), b"out")
    refused(call(at_out=None), b"out_start_bytes_out")
    refused(call(S=0), b"S")
    refused(call(S=-1), b"S")
    refused(call(S=65536), b"S")
    refused(call(counts=(2, 0)), b"stream 1", b"piece_count = 0")
    refused(call(counts=(-1, 1)), b"stream 0", b"piece_count = -1")
    refused(call(counts=(65535, 1)), b"65535 pieces", b"stream 1")
    # what f5_wave_join refuses, with the stream and the piece
    refused(call(lens=(100, 0, 13)), b"stream 0 piece 1", b"lens_host[1] = 0")
    refused(call(lens=(100, 50, -3)), b"stream 1 piece 0", b"lens_host[2] = -3")
    refused(call(fades=(0, -1, 0)), b"stream 0 piece 1", b"fade_host[1] = -1")
    refused(call(starts=(0, 100, -5)), b"stream 1 piece 0", b"start_host[2] = -5")
    # settled outside [0, total]: the second piece fades over 10 samples, so 140, not 150
    refused(call(settled=(141, 13)), b"stream 0", b"settled = 141", b"total = 140")
    refused(call(settled=(140, -1)), b"stream 1", b"settled = -1")
    refused(call(settled=(140, 14)), b"stream 1", b"total = 13")
    # what f5_wave_deliver refuses, with the stream
    refused(call(rates=(16000, 7999)), b"stream 1", b"out_rate")
    refused(call(rates=(192001, 16000)), b"stream 0", b"out_rate")
    refused(call(rates=(16000, 8001)), b"stream 1", b"8001", b"2^20")
    refused(call(fmts=(2, 0)), b"stream 0", b"format")
    refused(call(fmts=(1, -1)), b"stream 1", b"format")
    refused(call(o1=(95, 2)), b"stream 0", b"ready = 94")               # past the end of a final stream
    refused(call(o1=(94, 3)), b"stream 1", b"ready = 2")                # a sample whose taps are not all there yet
    refused(call(settled=(139, 13)), b"stream 0", b"ready = 93")        # ceil(278 / 3) = 93: the range follows `settled`, not the total
    refused(call(o0=(0, 3)), b"stream 1")                               # o0 > o1
    refused(call(o0=(-1, 0)), b"stream 0")
    refused(call(cap=199), b"out_capacity_bytes", b"200")
    refused(call(fmts=(0, 0), cap=391), b"out_capacity_bytes", b"392")  # f32: 376 bytes | pad to 384 | 8
    assert list(at) == [-9, -9], "a refused call wrote out_start_bytes_out"
    # valid arguments: the only thing missing is the bank, and it is stream 0 that says so
    assert call() == F5_ESTATE and lib.f5_last_error().startswith(b"f5_wave_emit:") and b"f5_mel_resample_bank" in lib.f5_last_error()
    assert b"stream 0" in lib.f5_last_error() and list(at) == [-9, -9]
    assert call(rates=(24000, 16000), o1=(140, 2), cap=296) == F5_ESTATE and b"stream 1" in lib.f5_last_error()
    count = C.c_int32(-1)
    assert lib.f5_mel_resample_bank_count(h, C.byref(count)) == 0 and count.value == 0
    # empty ranges at the stream's own rate need no bank and launch nothing
    assert call(rates=(24000, 24000), o1=(0, 0), cap=0) == 0, lib.f5_last_error()
    assert list(at) == [0, 0]
    assert call(rates=(24000, 24000), o0=(7, 1), o1=(7, 1), cap=0) == 0 and list(at) == [0, 0]


def test_emit_plan_and_the_python_wrapper_without_a_gpu():
    streams = [dict(range=(0, 94), sample_format="s16"), dict(range=(5, 5), sample_format="f32"), dict(range=(0, 2), sample_format="f32"),
               dict(range=(3, 10), sample_format="s16")]
    want = E.placement([st["range"] for st in streams], [st["sample_format"] for st in streams])
    assert want == ([0, 192, 192, 208], 222) and I.emit_plan(streams) == want
    ms = P.mel.MelSpec()
    x = torch.zeros(100)
    ok = dict(pieces=[x], fades=[0], settled=100, final=True, range=(0, 10), out_rate=16000, sample_format="f32")
    with pytest.raises(RuntimeError, match="GPU"):
        I.wave_emit(ms, [ok])
    with pytest.raises(ValueError, match="no stream"):
        I.wave_emit(ms, [])
    with pytest.raises(ValueError, match="sample_format"):
        I.wave_emit(ms, [dict(ok, sample_format="u8")])
    with pytest.raises(ValueError, match="stream 1.*one fade per piece"):
        I.wave_emit(ms, [ok, dict(ok, fades=[0, 3])])
    with pytest.raises(ValueError, match="at least one piece"):
        I.wave_emit(ms, [dict(ok, pieces=[], fades=[])])
    with pytest.raises(ValueError, match="1-D f32"):
        I.wave_emit(ms, [dict(ok, pieces=[x[::2]])])
    assert "u8" not in _lib.PCM_FORMATS


# ------------------------------------------------------------------------------------------------ the pool on the host
REF = "Some call me nature, others call me mother nature."    # 50 bytes
SENT = "The quick brown fox jumps over the lazy dog."           # 44 bytes


class _Bank:
    """What a pool reads of a VoiceBank on the host."""
    names, ref_texts, seconds, samples, frames, speeds, target_rms = ["v", "w"], [REF, REF], [3.0, 10.0], [72000, 240000], [282, 938], [None, 2.0], 0.1
    mel = torch.zeros(2, 938, 100)
    rms = torch.zeros(2)


class _Vocoder:
    def decode_ragged(self, *a, **k):
        raise AssertionError("not reached on the CPU")


def model():
    return P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100))


def test_open_pool_and_connect_argument_errors():
    m = model()
    for bad in (dict(batch_frames=0), dict(batch_frames=-5), dict(batch_frames=100, max_items=0), dict(batch_frames=100, lookahead=-1)):
        with pytest.raises(ValueError, match="open_pool"):
            I.open_pool(m, _Vocoder(), _Bank, **bad)
    with pytest.raises(TypeError):
        I.open_pool(m, _Vocoder(), _Bank)                               # batch_frames has no default
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        I.open_pool(m, object(), _Bank, batch_frames=None)
    kor = model()
    kor._tokenizer_type = "kor_g2p"
    with pytest.raises(NotImplementedError, match="text_tokenizer"):
        I.open_pool(kor, _Vocoder(), _Bank, batch_frames=None)
    with pytest.raises(ValueError, match="no voice"):
        I.open_pool(m, _Vocoder(), {}, batch_frames=None)              # (prepare_voices' refusal: the dict is prepared here)
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=1000, nfe_step=2)
    assert isinstance(pool, I.StreamPool) and pool.step() == [] and list(pool.run()) == [] and pool.log == []
    assert pool.stats() == dict(ticks=0, sample_calls=0, decode_calls=0, emit_launches=0, copies=0, packets=0, prompt_passes=0)
    with pytest.raises(ValueError, match="no voice"):
        pool.connect("x")
    for bad in (dict(sample_format="u8"), dict(chunk_size=0)):
        with pytest.raises(ValueError, match="connect"):
            pool.connect("v", **bad)
    with pytest.raises(_lib.F5Error, match="out_rate"):
        pool.connect("v", out_rate=4000)
    c = pool.connect("w", out_rate=16000, sample_format="s16", chunk_size=500, cross_fade_duration=0.15)
    assert (c.out_rate, c.sample_format, c.chunk_size, c.fade, c.voice) == (16000, "s16", 500, 3600, 1)
    assert pool.connect("v").fade == 0 and pool.connect("v", cross_fade_duration=-1.0).fade == 0


def test_a_clients_plan_is_a_sessions_and_its_first_package_state():
    m = model()
    text = " ".join([SENT] * 4)
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=2000, nfe_step=2)
    session = I.open_stream(m, _Vocoder(), (_Bank, "v"), batch_frames=2000, nfe_step=2)
    c = pool.connect("v")
    first = c.submit(text)
    want = session.plan(text)
    assert first.plan == {k: want[k] for k in ("chunks", "texts", "durations", "ends")}
    assert first.plan["chunks"] == [SENT + " " + SENT] * 2 and not first.done and (first.id, first.voice, first.client) == (0, 0, c)
    again = c.submit(text)                                     # the same client's second request: one chunk
    assert again.plan["chunks"] == [text] and again.plan == {k: v for k, v in session.plan(text).items() if k != "groups"} and again.id == 1
    c.reset()                                                  # the client left
    assert c.submit(text).plan["chunks"] == first.plan["chunks"]
    assert c.submit(text).plan["chunks"] == [text]
    c.update_reference("v")                                    # a new reference re-arms the first package
    assert c.submit(text).plan["chunks"] == first.plan["chunks"]
    other = pool.connect("v")                                  # the state is the client's, not the pool's
    assert other.submit(text).plan["chunks"] == first.plan["chunks"]
    empty = c.submit("")
    assert empty.done and empty.plan["chunks"] == [] and empty.id == 6
    # a voice's own speed goes first; without one the client's, else 1.0 (text_numerics on the prompt's samples)
    w = pool.connect("w", speed=4.0)
    assert w.submit(SENT).plan["durations"][0] == I.text_numerics(240000, REF, SENT, 2.0, None)[2]
    assert pool.connect("v", speed=4.0).submit(SENT).plan["durations"][0] == I.text_numerics(72000, REF, SENT, 4.0, None)[2]
    assert pool.connect("v").submit(SENT).plan["durations"][0] == I.text_numerics(72000, REF, SENT, 1.0, None)[2]
    w.update_reference("v")
    assert w.voice == 0 and w.submit(SENT).plan["durations"][0] == I.text_numerics(72000, REF, SENT, 4.0, None)[2]
    # cancel drops what has not started: the request leaves the queue and the pool goes idle without a device
    pool = I.open_pool(m, _Vocoder(), _Bank, batch_frames=2000, nfe_step=2)
    r = pool.connect("v").submit(text)
    assert not pool.idle() and not r.done
    r.cancel()
    assert r.done and pool.idle() and pool.step() == [] and pool.stats()["ticks"] == 0
