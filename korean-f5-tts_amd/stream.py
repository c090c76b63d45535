"""Streaming sessions (the reference's serving mode, socket_server.py: TTSStreamingProcessor): a voice prepared once, each request's
text split so that its first chunk is short, and the audio sent packet by packet while later chunks are still being generated.
`stream_chunks` is the host text plan of generate_stream (socket_server.py:112-143); `StreamSession` (infer.open_stream) runs the
chunks on the device path -- the voice from a VoiceBank, ragged sample(), decode_ragged, f5_wave_join, f5_wave_deliver -- and
yields packets at the client's rate and sample format.  `StreamPool` (infer.open_pool) serves many clients at once, which the
reference's server does not: `pool_tick` puts waiting chunks of different clients into one ragged batch per tick, and one
f5_wave_emit joins and delivers every touched request's new audio; with `slice_steps` a tick is a few steps of the solve
(CFM.sample_span) and `pool_slice` re-forms the batch between ticks: finished rows leave, waiting chunks join.  The TCP shell and
the sound-card code of the server are not here."""
from __future__ import annotations

import torch

from .config import HOP_LENGTH, SAMPLE_RATE


def stream_limits(ref_text: str, ref_seconds: float) -> tuple[int, int, int]:
    """(max_chars, few_chars, min_chars) of update_reference (socket_server.py:112-121): the prompt's bytes per second times the
    25 s the server budgets minus the prompt, then half and a quarter of it, each truncated by int on its own."""
    rate = len(ref_text.encode("utf-8")) / ref_seconds * (25 - ref_seconds)
    return int(rate), int(rate / 2), int(rate / 4)


def stream_chunks(text: str, ref_text: str, ref_seconds: float, first_package: bool) -> list[str]:
    """The text chunks of one request (generate_stream, socket_server.py:137-143): chunk_text at max_chars; on a client's first
    package the first chunk is chunked again at few_chars, and the new first chunk again at min_chars, so that the first audio
    comes early.  A text without chunks gives [] (the server would fail on it)."""
    from .infer import chunk_text

    max_chars, few_chars, min_chars = stream_limits(ref_text, ref_seconds)
    chunks = chunk_text(text, max_chars=max_chars)
    if chunks and first_package:
        chunks = chunk_text(chunks[0], max_chars=few_chars) + chunks[1:]
        chunks = chunk_text(chunks[0], max_chars=min_chars) + chunks[1:]
    return chunks


def packet_sizes(count: int, chunk_size: int) -> list[int]:
    """The sizes `for j in range(0, count, chunk_size): wave[j:j + chunk_size]` gives: full packets, then one short one."""
    return [min(chunk_size, count - j) for j in range(0, count, chunk_size)]


def request_plan(model, bank, v: int, text: str, first_package: bool, speed, fix_duration, text_tokenizer, stacklevel: int = 4) -> dict:
    """The host plan of one request spoken with voice v of the bank (what a session and a pool's client both run): the chunks
    (stream_chunks), the text and the total frames sample() runs each at (text_numerics, clamp_durations: as synthesize_script
    plans a chunk).  Returns dict(chunks, texts, durations, ends); a text without chunks gives empty lists."""
    from . import infer as I

    chunks = stream_chunks(text, bank.ref_texts[v], bank.seconds[v], first_package)
    texts, durations = [], []
    for chunk in chunks:
        rtext, _ref_len, duration = I.text_numerics(bank.samples[v], bank.ref_texts[v], chunk, speed, fix_duration)
        texts.append(rtext + chunk)
        durations.append(duration)
    if not chunks:
        return dict(chunks=[], texts=[], durations=[], ends=[])
    texts, idx = I._tokenise(model, texts, text_tokenizer, stacklevel=stacklevel)
    ends = I.clamp_durations(idx.to("cpu", torch.long), torch.tensor([bank.frames[v]] * len(chunks)), torch.tensor(durations)).tolist()
    return dict(chunks=chunks, texts=texts, durations=durations, ends=ends)


class StreamSession:
    """One client's stream (infer.open_stream builds it).  `stream(text)` is a generator of (packet, out_rate): numpy views of
    `chunk_size` samples (the last of an emission shorter) at the session's rate and format.  Concatenated, a request's packets
    are bit for bit `wave_deliver(wave_join(pieces, fades), final=True)` -- the request's finished waveform at the client's rate --
    where the pieces are the chunks' waveforms as synthesize_script makes them and a piece inside the request fades over
    int(cross_fade_duration * 24000) samples.

    Per group of chunks: ONE model.sample, ONE decode_ragged, the rescale to the prompt's level, ONE wave_join of the request's
    pieces so far, ONE wave_deliver of the samples that have become settled, ONE asynchronous copy into a pinned buffer.  Behind a
    group the joined waveform is settled up to its length minus the fade (a later piece fades over at most that many samples and
    never reaches further back), and of that prefix the resampler has settled what deliver_plan calls ready; after the last group
    everything is.  `lookahead = k`: the work of groups g + 1 .. g + k is enqueued before the host waits for group g's copy."""

    def __init__(self, model, vocoder, voice, *, out_rate, sample_format, chunk_size, cross_fade_duration, batch_frames, lookahead,
                 nfe_step, cfg_strength, sway_sampling_coef, speed, fix_duration, seed, text_tokenizer, clip_silence):
        from . import infer as I

        I._require_text_tokenizer(model, text_tokenizer)
        I._require_ragged_vocoder(vocoder, "open_stream", "stream through infer_batch_process(streaming=True)")
        if sample_format not in ("f32", "s16"):
            raise ValueError(f"open_stream: sample_format {sample_format!r} (expected 'f32' or 's16')")
        if int(chunk_size) < 1:
            raise ValueError(f"open_stream: chunk_size = {chunk_size} (need at least 1 sample per packet)")
        if int(lookahead) < 0:
            raise ValueError(f"open_stream: lookahead = {lookahead} (need 0 or more groups)")
        if batch_frames is not None and int(batch_frames) < 1:
            raise ValueError(f"open_stream: batch_frames = {batch_frames} (need None or a positive budget)")
        I.deliver_plan(out_rate, 0)                                          # refuses a rate the device stage does not take
        self.model, self.vocoder = model, vocoder
        self.out_rate, self.sample_format, self.chunk_size = int(out_rate), sample_format, int(chunk_size)
        self.fade = int(cross_fade_duration * SAMPLE_RATE) if cross_fade_duration > 0 else 0
        self.batch_frames, self.lookahead = batch_frames, int(lookahead)
        self.sample_kw = dict(steps=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
        self.speed, self.fix_duration, self.text_tokenizer, self.clip_silence = speed, fix_duration, text_tokenizer, clip_silence
        self._stats = dict(prompt_passes=0, groups_enqueued=0, groups_emitted=0, packets=0)
        self.update_reference(voice)

    # ---- the voice ---------------------------------------------------------------------------------------------------------
    def update_reference(self, voice):
        """A new voice for the session: a (VoiceBank, name) pair -- nothing is prepared, the bank has it -- or the dict
        prepare_voices takes with one voice, whose prompt is prepared here, once.  Re-arms the first package."""
        from . import infer as I

        if isinstance(voice, tuple):
            bank, name = voice
            if name not in bank.names:
                raise ValueError(f"open_stream: the bank has no voice {name!r} (it has {bank.names})")
        else:
            if len(voice) != 1:
                raise ValueError(f"open_stream: a session speaks with one voice; the dict names {len(voice)}")
            bank = I.prepare_voices(self.model, voice, clip_silence=self.clip_silence)
            name = bank.names[0]
            self._stats["prompt_passes"] += 1
        v = bank.names.index(name)
        self.bank, self.voice = bank, v
        own = bank.speeds[v]
        self._speed = self.speed if own is None else own
        self._row = torch.tensor([v], device=bank.mel.device)
        self._first = True

    def reset(self):
        """The client left (socket_server.py:160-162): the next request is a first package again."""
        self._first = True

    def warm_up(self, text: str = "Warm-up text for the model.", max_seconds: float = 25.0):
        """The server's _warm_up: with length buckets on, captures the graphs of every bucket a B = 1 request can touch (from the
        prompt's frames to `max_seconds` in all, the server's budget); then runs one request through to its last packet, which
        also builds everything the first request would otherwise pay for (the rate's filter bank, the workspaces)."""
        tr = self.model.transformer
        if getattr(tr, "length_bucket", 0):
            frames = self.bank.frames[self.voice]
            n_max = max(frames + 2, int(max_seconds * SAMPLE_RATE / HOP_LENGTH))
            tr.prepare_sample(1, frames + 1, n_max, n_max, self.sample_kw["steps"], self.sample_kw["cfg_strength"],
                              method=self.model.odeint_kwargs.get("method", "euler"))
        first = self._first
        for _ in self.stream(text):
            pass
        self._first = first

    def stats(self) -> dict:
        """prompt_passes: prompts this session prepared; groups_enqueued / groups_emitted: groups whose device work was issued /
        whose copy the host has waited for; packets: packets yielded."""
        return dict(self._stats)

    # ---- a request ---------------------------------------------------------------------------------------------------------
    def plan(self, text: str) -> dict:
        """The host plan of one request, consuming the first package: chunks, the text and the total frames sample() runs each
        at (text_numerics, clamp_durations: as synthesize_script plans a chunk), the groups as ranges of chunks."""
        from . import infer as I

        plan = request_plan(self.model, self.bank, self.voice, text, self._first, self._speed, self.fix_duration, self.text_tokenizer,
                            stacklevel=5)
        self._first = False
        ends = plan["ends"]
        if not ends:
            groups = []
        elif self.batch_frames is None:
            groups = [range(i, i + 1) for i in range(len(ends))]
        else:                                                               # the first chunk alone: its audio is what the client waits for
            groups = [range(0, 1)] + [range(r.start + 1, r.stop + 1) for r in I.group_chunks(ends[1:], self.batch_frames)]
        return dict(plan, groups=groups)

    def _enqueue(self, plan, g, pieces, state):
        """The device work of group g, all of it asynchronous: returns (pinned host tensor or None, event)."""
        from . import infer as I

        bank, v, run = self.bank, self.voice, plan["groups"][g]
        frames, start = bank.frames[v], bank.samples[v] // HOP_LENGTH
        rows = self._row.expand(len(run))
        generated, _ = self.model.sample(cond=bank.mel[:, :frames].index_select(0, rows), text=[plan["texts"][k] for k in run],
                                         duration=torch.tensor([plan["durations"][k] for k in run]),
                                         lens=torch.tensor([frames] * len(run)), **self.sample_kw)
        wave, wave_lens = self.vocoder.decode_ragged(generated.to(torch.float32).permute(0, 2, 1), ends=[plan["ends"][k] for k in run],
                                                     starts=[start] * len(run))
        wave = I.rescale_to_prompt(wave, bank.rms.index_select(0, rows)[:, None], bank.target_rms)
        pieces.extend(wave[b, :wave_lens[b]] for b in range(len(run)))
        last = g == len(plan["groups"]) - 1
        fades = [0] + [self.fade] * (len(pieces) - 1)
        total = I.join_plan([int(p.shape[0]) for p in pieces], fades)[2]
        settled = total if last else max(total - self.fade, 0)
        ready = I.deliver_plan(self.out_rate, settled, last)[1]
        host = None
        if ready > state["sent"]:
            joined = I.wave_join(pieces, fades)
            out = I.wave_deliver(self.model.mel_spec, [joined[:settled]], out_rate=self.out_rate, sample_format=self.sample_format,
                                 ranges=[(state["sent"], ready)], final=last)[0]
            host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
            host.copy_(out, non_blocking=True)
            state["sent"] = ready
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(bank.mel.device))
        self._stats["groups_enqueued"] += 1
        return host, event

    def stream(self, text: str):
        """(packet, out_rate) pairs of one request.  Closing the generator early abandons the rest of the request; the session
        stays usable (work already enqueued runs to its end on the stream, and nothing waits for it)."""
        plan = self.plan(text)
        groups = plan["groups"]
        if not groups:
            return
        pieces, state, pending, nxt = [], dict(sent=0), [], 0
        with torch.inference_mode(), torch.cuda.device(self.bank.mel.device):
            for g in range(len(groups)):
                while nxt < len(groups) and nxt <= g + self.lookahead:
                    pending.append(self._enqueue(plan, nxt, pieces, state))
                    nxt += 1
                host, event = pending.pop(0)
                event.synchronize()
                self._stats["groups_emitted"] += 1
                if host is None:
                    continue
                samples = host.numpy()                                      # (a view: the packets keep the pinned buffer alive)
                for j in range(0, samples.shape[0], self.chunk_size):
                    self._stats["packets"] += 1
                    yield samples[j:j + self.chunk_size], self.out_rate


def open_stream(model, vocoder, voice, *, out_rate=SAMPLE_RATE, sample_format="f32", chunk_size=2048, cross_fade_duration=0.0,
                batch_frames=None, lookahead=1, nfe_step=32, cfg_strength=2.0, sway_sampling_coef=-1.0, speed=1.0, fix_duration=None,
                seed=None, text_tokenizer=None, clip_silence=False) -> StreamSession:
    """A streaming session for one client (the reference's TTSStreamingProcessor without its TCP shell): voice is a
    (VoiceBank, name) pair or the dict prepare_voices takes (one voice; prepared once, here or by update_reference).
    out_rate in [8000, 192000] and sample_format "f32" / "s16": what the client receives (f5_wave_deliver); chunk_size: samples per
    packet at out_rate; cross_fade_duration: seconds the chunks of a request fade into each other (0, the server's behaviour:
    plain concatenation); batch_frames: None runs every chunk as its own B = 1 sample(), each as if alone; an int runs the first
    chunk alone and the rest as ragged batches of at most that many rows x longest row (group_chunks; with
    `attn_mask_enabled=False` a chunk in a batch sees the batch's padding, as in every batch driver); lookahead: groups enqueued
    ahead of the one the host waits for (DESIGN.md 6k has the measurement behind the default).  The other keywords are
    synthesize_script's.  See StreamSession."""
    return StreamSession(model, vocoder, voice, out_rate=out_rate, sample_format=sample_format, chunk_size=chunk_size,
                         cross_fade_duration=cross_fade_duration, batch_frames=batch_frames, lookahead=lookahead, nfe_step=nfe_step,
                         cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration,
                         seed=seed, text_tokenizer=text_tokenizer, clip_silence=clip_silence)


# ---------------------------------------------------------------------------------------------------------------- the pool
def tick_cost(frames, packed):
    """What a tick of rows of these frame counts costs against batch_frames: rows x longest row, or (packed: the rows run on packed
    rows, as an isolated pool's do) the sum of the rows' frames, each rounded up to 4 as the packed layout rounds them."""
    if packed:
        return sum(-(-f // 4) * 4 for f in frames)
    return len(frames) * max(frames) if frames else 0


def pool_tick(waiting, batch_frames, max_items, first_alone, cursor, packed=False):
    """Which chunks run in the next tick of a StreamPool: a pure function of the queue.  `waiting` lists the requests that have
    chunks waiting, in submission order, as (request id, index of its first waiting chunk, [frames sample() runs each waiting chunk
    at, in the request's order]); ids are integers that ascend with submission.  Returns (items, cursor): the tick's rows as
    (request id, chunk index) in row order, and the cursor for the tick after it.

    The budget is that of group_chunks: a tick costs its row count times its longest row, so an item joins while
    (rows + 1) * max(longest, its frames) <= batch_frames (None: no such limit) and rows + 1 <= max_items.  The first item of a tick
    is always taken: a chunk over the budget runs alone.  The tick ends at the first item that does not fit -- nothing behind it is
    tried, so nobody overtakes it.  A request's chunks are only ever taken in their own order.
      * While a request whose first chunk (index 0) waits is in the queue and `first_alone` is set, the tick holds first chunks
        only, in submission order (a client's first audio is what it waits for); the cursor stays.
      * Otherwise round-robin: the requests in ascending id from the first id >= cursor, wrapping around, give one chunk each;
        when all have given and the budget is not spent they give their next one, and so on.  The tick ends where an item does
        not fit, and that request's id is the new cursor: the requests the tick did not reach are first in the next one, ahead of
        every request it served.  So of two requests that wait through two round-robin ticks in a row, one never gets rows in both
        while the other gets none -- no request is passed over twice in a row.  When everything waiting was taken the cursor stays.

    packed=True (a pool with isolate=True, whose ticks run on packed rows): a tick costs the sum of its rows' frames, each rounded up
    to 4 (tick_cost), so an item joins while that sum with its own frames stays <= batch_frames; everything else is as above."""
    items, longest, taken = [], 0, []

    def fits(frames):
        rows = len(items)
        if packed:
            return rows == 0 or (rows < max_items and (batch_frames is None or tick_cost(taken + [frames], True) <= batch_frames))
        return rows == 0 or (rows < max_items and (batch_frames is None or (rows + 1) * max(longest, frames) <= batch_frames))

    live = [w for w in waiting if w[2]]
    firsts = [w for w in live if w[1] == 0]
    if first_alone and firsts:
        for rid, _, frames in firsts:
            if not fits(frames[0]):
                break
            items.append((rid, 0))
            taken.append(frames[0])
            longest = max(longest, frames[0])
        return items, cursor
    if not live:
        return [], cursor
    start = next((i for i, w in enumerate(live) if w[0] >= cursor), 0)
    order = live[start:] + live[:start]
    for depth in range(max(len(w[2]) for w in order)):
        for rid, k, frames in order:
            if depth >= len(frames):
                continue
            if not fits(frames[depth]):
                return items, rid
            items.append((rid, k + depth))
            taken.append(frames[depth])
            longest = max(longest, frames[depth])
    return items, cursor


def pool_slice(under_way, waiting, batch_frames, max_items, first_alone, cursor, packed=False):
    """Which rows run in the next tick of a StreamPool that solves in slices (open_pool(slice_steps=...)): a pure function of the
    rows under way and the queue.  `under_way` lists the chunks whose solve has begun and not ended, in the order they joined, as
    (request id, chunk index, frames); `waiting` is pool_tick's list.  Returns (items, cursor): the tick's rows as (request id,
    chunk index) in row order -- rows under way first, then the chunks that join -- and the cursor for the tick after it.

    The budget is pool_tick's, over both kinds of row alike: an item is taken while (rows + 1) * max(longest, its frames) <=
    batch_frames (None: no such limit) and rows + 1 <= max_items.  The first item of a tick is always taken.  The tick ends at the
    first item that does not fit -- nothing behind it is tried, so nobody overtakes it: a row under way that does not fit keeps
    every later row and every waiting chunk out.
      * While a first chunk (index 0) waits or is under way and `first_alone` is set, the tick holds first chunks only: those under
        way in the order they joined, then the waiting ones in submission order; the cursor stays.  Every other row under way is
        parked: it is not in the tick, keeps its state and its position, and is taken again once no first chunk is left.
      * Otherwise every row under way in the order it joined, and then the waiting chunks by pool_tick's round-robin: the requests
        in ascending id from the first id >= cursor, wrapping around, give one chunk each, then their next one, and so on.  Where
        a waiting item does not fit the tick ends and that request's id is the new cursor, so pool_tick's property holds: of two
        requests that wait through two round-robin ticks in a row, one never gets rows in both while the other gets none.  When
        everything waiting was taken, or a row under way did not fit, the cursor stays.

    packed=True: pool_tick's packed budget -- the sum of the rows' frames, each rounded up to 4 -- over both kinds of row alike."""
    items, longest, taken = [], 0, []

    def fits(frames):
        rows = len(items)
        if packed:
            return rows == 0 or (rows < max_items and (batch_frames is None or tick_cost(taken + [frames], True) <= batch_frames))
        return rows == 0 or (rows < max_items and (batch_frames is None or (rows + 1) * max(longest, frames) <= batch_frames))

    live = [w for w in waiting if w[2]]
    firsts = [w for w in live if w[1] == 0]
    if first_alone and (firsts or any(k == 0 for _, k, _ in under_way)):
        for rid, k, frames in [(rid, k, f) for rid, k, f in under_way if k == 0] + [(rid, 0, f[0]) for rid, _, f in firsts]:
            if not fits(frames):
                break
            items.append((rid, k))
            taken.append(frames)
            longest = max(longest, frames)
        return items, cursor
    for rid, k, frames in under_way:
        if not fits(frames):
            return items, cursor
        items.append((rid, k))
        taken.append(frames)
        longest = max(longest, frames)
    if not live:
        return items, cursor
    start = next((i for i, w in enumerate(live) if w[0] >= cursor), 0)
    order = live[start:] + live[:start]
    for depth in range(max(len(w[2]) for w in order)):
        for rid, k, frames in order:
            if depth >= len(frames):
                continue
            if not fits(frames[depth]):
                return items, rid
            items.append((rid, k + depth))
            taken.append(frames[depth])
            longest = max(longest, frames[depth])
    return items, cursor


def span_prev(sources):
    """The `prev` of a model.sample_span call whose rows come from these places: per row (state tensor, row in it), or (None, -1)
    for a row that begins.  Returns (state, rows) -- None for the state when every row begins.  Rows that continue from one tensor
    use it as it is; rows from several tensors (a parked row resumes beside rows of a later tick) are gathered into one, each at
    the longest tensor's frame count, zero padded: what the engine's staging does with frames a previous state did not have."""
    tensors = []
    for t, _ in sources:
        if t is not None and not any(t is u for u in tensors):
            tensors.append(t)
    if len(tensors) <= 1:
        return (tensors[0] if tensors else None), [row for _, row in sources]
    frames = max(t.shape[1] for t in tensors)
    kept = [(t, row) for t, row in sources if t is not None]
    state = torch.zeros(len(kept), frames, tensors[0].shape[2], device=tensors[0].device, dtype=tensors[0].dtype)
    for j, (t, row) in enumerate(kept):
        state[j, :t.shape[1]] = t[row]
    at = iter(range(len(kept)))
    return state, [-1 if t is None else next(at) for t, _ in sources]


class SliceRow:
    """A chunk whose solve is under way in a pool that solves in slices: its request and chunk index, the state tensor that holds
    its row and the row, the steps it has made, and the sampler settings it joined with."""

    def __init__(self, req, k):
        self.req, self.k, self.state, self.row, self.made, self.kw = req, k, None, -1, 0, dict(req.client.sample_kw)


class PoolRequest:
    """One submitted text of a client (client.submit): `id` ascends with submission, `plan` is request_plan's dict, `voice` the
    bank's row it is spoken with, `done` whether its last packet has been handed out (or it was cancelled with nothing under way)."""

    def __init__(self, rid, client, voice, plan):
        self.id, self.client, self.voice, self.plan = rid, client, voice, plan
        self.next = 0                       # the first chunk that has not been put into a tick
        self.stop = len(plan["ends"])       # chunks that run at all (cancel lowers it)
        self.flying = 0                     # ticks enqueued whose bytes the host has not cut into packets yet
        self.under_way = 0                  # chunks whose solve has begun and not ended (a pool that solves in slices)
        self.pieces, self.sent = [], 0      # the chunks' waveforms so far, on the device; samples delivered at the client's rate
        self.done = self.stop == 0

    def cancel(self):
        """Drops the chunks that have not started.  What is under way still arrives; the stream is not finalised, so the last
        `fade` samples of what ran (and the resampler's last taps) are never sent."""
        self.stop = self.next
        if self.flying == 0 and self.under_way == 0:
            self.done = True


UNSET = object()   # connect(sway_sampling_coef=..., seed=...): "the pool's own value" (None is a value of both)


class PoolClient:
    """One client of a StreamPool (pool.connect): its voice, rate, format, packet size, cross-fade and first-package state, and the
    sampler settings its chunks run with (`sample_kw`: the pool's, unless connect gave the client its own)."""

    def __init__(self, pool, voice, out_rate, sample_format, chunk_size, cross_fade_duration, speed, fix_duration, nfe_step=None,
                 cfg_strength=None, sway_sampling_coef=UNSET, seed=UNSET):
        import math

        from . import infer as I

        kw = dict(pool.sample_kw)
        if nfe_step is not None:
            if int(nfe_step) < 1:
                raise ValueError(f"connect: nfe_step = {nfe_step} (need at least 1 step)")
            kw["steps"] = int(nfe_step)
        if cfg_strength is not None:
            if not math.isfinite(float(cfg_strength)):
                raise ValueError(f"connect: cfg_strength = {cfg_strength} (need a finite number)")
            kw["cfg_strength"] = float(cfg_strength)
        if sway_sampling_coef is not UNSET:
            if sway_sampling_coef is not None and not math.isfinite(float(sway_sampling_coef)):
                raise ValueError(f"connect: sway_sampling_coef = {sway_sampling_coef} (need None or a finite number)")
            kw["sway_sampling_coef"] = sway_sampling_coef
        if seed is not UNSET:
            kw["seed"] = seed
        self.sample_kw = kw

        if sample_format not in ("f32", "s16"):
            raise ValueError(f"connect: sample_format {sample_format!r} (expected 'f32' or 's16')")
        if int(chunk_size) < 1:
            raise ValueError(f"connect: chunk_size = {chunk_size} (need at least 1 sample per packet)")
        I.deliver_plan(out_rate, 0)                                          # refuses a rate the device stage does not take
        self.pool, self.out_rate, self.sample_format, self.chunk_size = pool, int(out_rate), sample_format, int(chunk_size)
        self.fade = int(cross_fade_duration * SAMPLE_RATE) if cross_fade_duration > 0 else 0
        self.speed, self.fix_duration = speed, fix_duration
        self.update_reference(voice)

    def update_reference(self, name):
        """Another voice of the pool's bank for this client.  Re-arms the first package."""
        bank = self.pool.bank
        if name not in bank.names:
            raise ValueError(f"connect: the bank has no voice {name!r} (it has {bank.names})")
        self.voice = bank.names.index(name)
        own = bank.speeds[self.voice]
        base = 1.0 if self.speed is None else self.speed
        self._speed = base if own is None else own
        self._first = True

    def reset(self):
        """The client left: its next request is a first package again."""
        self._first = True

    def submit(self, text: str) -> PoolRequest:
        """Plans the request (request_plan: exactly a session's plan, consuming the first package) and queues its chunks."""
        pool = self.pool
        plan = request_plan(pool.model, pool.bank, self.voice, text, self._first, self._speed, self.fix_duration, pool.text_tokenizer)
        self._first = False
        req = PoolRequest(pool._next_id, self, self.voice, plan)
        pool._next_id += 1
        if not req.done:
            pool._requests.append(req)
        return req


class StreamPool:
    """Many clients on one model (infer.open_pool builds it): the chunks of different clients' requests share ragged batches.  One
    tick is, all asynchronous on the stream: ONE model.sample (model.sample_items when its rows differ in sampler settings) over the tick's items (pool_tick chooses them) with each item's own
    voice row and prompt frames, as synthesize_script runs a group; ONE decode_ragged; the rescale to each prompt's level; ONE
    wave_emit over every request the tick touched -- its pieces so far joined and the samples that have become settled delivered at
    its client's rate and format, read where the pieces lie; ONE copy of the emitted bytes into a pinned buffer.  The host then
    cuts each request's bytes into packets of its client's chunk_size.  Behind a tick a request is settled up to its joined length
    minus its fade, and wholly after its last chunk, as in a StreamSession; concatenated, a request's packets are bit for bit
    wave_deliver(wave_join(pieces, fades), final=True) at its client's rate.

    `step()` runs one tick and returns [(request, [packets])] for the requests it touched ([] when nothing waits); `run()` yields
    (request, packet, out_rate) until nothing waits.  Requests may be submitted between any two ticks.  `log` holds the batches as
    run: per tick the (request id, chunk index) items in row order.

    slice_steps = k (None: everything above, call for call): a tick is ONE model.sample_span of at most k steps over the rows
    pool_slice chooses -- the rows under way, whose state stays on the device between ticks, and the waiting chunks that join.
    The rows whose last step a tick ran, and only these, are decoded, rescaled, emitted and copied as above; a tick that ends no
    row emits nothing and step() returns [] for it.  While a first chunk waits or is under way (first_alone) the other rows are
    parked.  `spans` holds, beside `log`, per tick the (first step, steps run) of each row.  stats(): ticks and sample_calls
    count every slice; decode_calls, emit_launches and copies only the ticks that ended a row."""

    def __init__(self, model, vocoder, voices, *, batch_frames, max_items, first_alone, lookahead, nfe_step, cfg_strength,
                 sway_sampling_coef, seed, text_tokenizer, clip_silence, slice_steps=None, isolate=False):
        from . import infer as I

        I._require_text_tokenizer(model, text_tokenizer)
        I._require_ragged_vocoder(vocoder, "open_pool", "stream through infer_batch_process(streaming=True)")
        if int(lookahead) < 0:
            raise ValueError(f"open_pool: lookahead = {lookahead} (need 0 or more ticks)")
        if batch_frames is not None and int(batch_frames) < 1:
            raise ValueError(f"open_pool: batch_frames = {batch_frames} (need None or a positive budget)")
        if int(max_items) < 1:
            raise ValueError(f"open_pool: max_items = {max_items} (need at least 1 row per tick)")
        if slice_steps is not None and (isinstance(slice_steps, bool) or int(slice_steps) != slice_steps or int(slice_steps) < 1):
            raise ValueError(f"open_pool: slice_steps = {slice_steps} (need None or a whole number of steps, at least 1)")
        self.slice_steps = None if slice_steps is None else int(slice_steps)
        self.isolate = bool(isolate)
        if self.isolate:   # every row as if alone in its tick: the model's switch (raises for a backbone without packed rows), and room for the ticks' graphs
            tr = getattr(model, "transformer", model)
            tr.set_isolated_rows(True)
            tr.set_graph_capacity(64)
        self.spans, self._rows = [], []     # slice_steps: per tick the (start, steps run) of each row; the rows under way
        self.model, self.vocoder, self.text_tokenizer = model, vocoder, text_tokenizer
        self.batch_frames, self.max_items = batch_frames, int(max_items)
        self.first_alone, self.lookahead = bool(first_alone), int(lookahead)
        self.sample_kw = dict(steps=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
        self._stats = dict(ticks=0, sample_calls=0, decode_calls=0, emit_launches=0, copies=0, packets=0, prompt_passes=0)
        if isinstance(voices, dict):
            self.bank = I.prepare_voices(model, voices, clip_silence=clip_silence)
            self._stats["prompt_passes"] += 1
        else:
            self.bank = voices
        self.log, self._requests, self._pending, self._outbox, self._cursor, self._next_id = [], [], [], [], 0, 0

    def connect(self, voice, *, out_rate=SAMPLE_RATE, sample_format="f32", chunk_size=2048, cross_fade_duration=0.0, speed=None,
                fix_duration=None, nfe_step=None, cfg_strength=None, sway_sampling_coef=UNSET, seed=UNSET) -> PoolClient:
        """A client that speaks with `voice` of the pool's bank and receives packets of chunk_size samples at out_rate in
        sample_format; cross_fade_duration: seconds the chunks of one of its requests fade into each other; speed: None is 1.0 (a
        voice's own speed goes first, as in a session).  nfe_step / cfg_strength / sway_sampling_coef / seed: the client's own
        sampler settings; left out, the pool's.  Clients of different settings still share ticks (model.sample_items)."""
        return PoolClient(self, voice, out_rate, sample_format, chunk_size, cross_fade_duration, speed, fix_duration, nfe_step,
                          cfg_strength, sway_sampling_coef, seed)

    def stats(self) -> dict:
        """ticks run; sample_calls / decode_calls / emit_launches: model.sample, decode_ragged and wave_emit calls; copies: device
        to host copies; packets handed out; prompt_passes: prompt preparations this pool ran; isolated: True, for a pool opened
        with isolate=True (any other pool's dict is the one it always was: read it with .get("isolated", False), or pool.isolate)."""
        return dict(self._stats, isolated=True) if self.isolate else dict(self._stats)

    def idle(self) -> bool:
        return not self._pending and not self._rows and not any(r.next < r.stop for r in self._requests)

    # ---- a tick ------------------------------------------------------------------------------------------------------------
    def _batch_of(self, run):
        """The rows `run` ([(request, chunk)]) as the sampler's cond, text, duration and lens keywords, and the rows' voices."""
        bank = self.bank
        glens = [bank.frames[r.voice] for r, _ in run]
        rows = torch.tensor([r.voice for r, _ in run], device=bank.mel.device)
        return dict(cond=bank.mel[:, :max(glens)].index_select(0, rows), text=[r.plan["texts"][k] for r, k in run],
                    duration=torch.tensor([r.plan["durations"][k] for r, k in run]), lens=torch.tensor(glens)), rows

    def _enqueue(self):
        """The device work of the next tick, all of it asynchronous: None when nothing waits, else (touched requests with their
        byte spans, pinned host tensor or None, event)."""
        self._requests = [r for r in self._requests if r.next < r.stop or r.flying]
        waiting = [(r.id, r.next, r.plan["ends"][r.next:r.stop]) for r in self._requests if r.next < r.stop]
        # batch_frames=None is a session's: every chunk as its own B = 1 sample()
        items, self._cursor = pool_tick(waiting, self.batch_frames, self.max_items if self.batch_frames is not None else 1,
                                        self.first_alone, self._cursor, packed=self.isolate)
        if not items:
            return None
        by_id = {r.id: r for r in self._requests}
        run = [(by_id[rid], k) for rid, k in items]
        self.log.append(list(items))
        batch, rows = self._batch_of(run)
        # a tick whose rows all carry the pool's settings is one sample(); any other is one sample_items() with the rows' own
        row_kw = [r.client.sample_kw for r, _ in run]
        # (an isolated pool always takes sample_items: the model's switch is about the per-item calls)
        if not self.isolate and all(kw == self.sample_kw for kw in row_kw):
            sample, kw = self.model.sample, self.sample_kw
        else:
            sample, kw = self.model.sample_items, {name: [rk[name] for rk in row_kw] for name in self.sample_kw}
        generated, _ = sample(**batch, **kw)
        for r, k in run:
            assert k == r.next, "a request's chunks run in order"
            r.next += 1
        for key in ("ticks", "sample_calls"):
            self._stats[key] += 1
        return self._deliver(run, generated, rows)

    def _enqueue_slice(self):
        """_enqueue for a pool that solves in slices: one model.sample_span of at most slice_steps steps over the rows pool_slice
        chooses; the rows whose last step it ran, and only these, are delivered.  A tick that ends no row gives ([], None, event)."""
        self._requests = [r for r in self._requests if r.next < r.stop or r.flying or r.under_way]
        waiting = [(r.id, r.next, r.plan["ends"][r.next:r.stop]) for r in self._requests if r.next < r.stop]
        under_way = [(row.req.id, row.k, row.req.plan["ends"][row.k]) for row in self._rows]
        items, self._cursor = pool_slice(under_way, waiting, self.batch_frames, self.max_items if self.batch_frames is not None else 1,
                                         self.first_alone, self._cursor, packed=self.isolate)
        if not items:
            return None
        by_id, known = {r.id: r for r in self._requests}, {(row.req.id, row.k): row for row in self._rows}
        chosen = []
        for rid, k in items:
            row = known.get((rid, k))
            if row is None:                                                 # a waiting chunk joins
                r = by_id[rid]
                assert k == r.next, "a request's chunks run in order"
                r.next += 1
                r.under_way += 1
                row = SliceRow(r, k)
                self._rows.append(row)
            chosen.append(row)
        bank, run = self.bank, [(row.req, row.k) for row in chosen]
        self.log.append(list(items))
        batch, rows = self._batch_of(run)
        state, prev_rows = span_prev([(row.state, row.row) for row in chosen])
        start = [row.made for row in chosen]
        res = self.model.sample_span(**batch, start=start, count=self.slice_steps, prev=None if state is None else (state, prev_rows),
                                     **{name: [row.kw[name] for row in chosen] for name in self.sample_kw})
        self.spans.append([(a, min(self.slice_steps, int(row.kw["steps"]) - a)) for a, row in zip(start, chosen)])
        for key in ("ticks", "sample_calls"):
            self._stats[key] += 1
        ended = []
        for b, (row, (_, made)) in enumerate(zip(chosen, self.spans[-1])):
            row.state, row.row, row.made = res.state, b, row.made + made
            if res.done[b]:
                ended.append(b)
                row.req.under_way -= 1
                self._rows.remove(row)
        if not ended:
            return [], None, self._mark()
        if len(ended) == len(chosen):
            return self._deliver(run, res.out, rows)
        pick = torch.tensor(ended, device=bank.mel.device)
        return self._deliver([run[b] for b in ended], res.out.index_select(0, pick), rows.index_select(0, pick))

    def _deliver(self, run, generated, rows):
        """The rest of a tick for the rows `run` whose solve has ended, generated[b] the mel of run[b] and rows[b] its voice:
        decode_ragged, the rescale, wave_emit and the copy.  Returns what _enqueue returns."""
        from . import infer as I

        bank = self.bank
        wave, wave_lens = self.vocoder.decode_ragged(generated.to(torch.float32).permute(0, 2, 1), ends=[r.plan["ends"][k] for r, k in run],
                                                     starts=[bank.samples[r.voice] // HOP_LENGTH for r, _ in run])
        wave = I.rescale_to_prompt(wave, bank.rms.index_select(0, rows)[:, None], bank.target_rms)
        touched = []
        for b, (r, k) in enumerate(run):
            assert k == len(r.pieces), "a request's chunks end in order"
            r.pieces.append(wave[b, :wave_lens[b]])
            if r not in touched:
                touched.append(r)
        streams = []
        for r in touched:
            c, last = r.client, len(r.pieces) >= len(r.plan["ends"])      # (len(r.pieces) is r.next unless a later chunk is under way)
            fades = [0] + [c.fade] * (len(r.pieces) - 1)
            total = I.join_plan([int(p.shape[0]) for p in r.pieces], fades)[2]
            settled = total if last else max(total - c.fade, 0)
            ready = I.deliver_plan(c.out_rate, settled, last)[1]
            streams.append(dict(pieces=r.pieces, fades=fades, settled=settled, final=last, range=(r.sent, max(ready, r.sent)),
                                out_rate=c.out_rate, sample_format=c.sample_format))
            r.sent = max(ready, r.sent)
            r.flying += 1
        _views, buf = I.wave_emit(self.model.mel_spec, streams)
        starts, total = I.emit_plan(streams)
        host = None
        if total:
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            host.copy_(buf[:total], non_blocking=True)
            self._stats["copies"] += 1
        event = self._mark()
        for key in ("decode_calls", "emit_launches"):
            self._stats[key] += 1
        spans = [(r, a, st["range"][1] - st["range"][0]) for r, a, st in zip(touched, starts, streams)]
        return spans, host, event

    def _mark(self):
        """An event behind everything the tick has put on the stream."""
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self.bank.mel.device))
        return event

    def step(self):
        """One tick: enqueues the device work of up to 1 + lookahead ticks, waits for the oldest one's copy and returns
        [(request, [packets])] for the requests it touched; [] when nothing waits and nothing is under way."""
        import numpy as np

        if self.idle():
            return []
        with torch.inference_mode(), torch.cuda.device(self.bank.mel.device):
            while len(self._pending) <= self.lookahead:
                tick = self._enqueue() if self.slice_steps is None else self._enqueue_slice()
                if tick is None:
                    break
                self._pending.append(tick)
        if not self._pending:
            return []
        spans, host, event = self._pending.pop(0)
        event.synchronize()
        raw = host.numpy() if host is not None else None                    # (a view: the packets keep the pinned buffer alive)
        out = []
        for r, a, count in spans:
            c = r.client
            width, dtype = (4, np.float32) if c.sample_format == "f32" else (2, np.int16)
            samples = raw[a:a + count * width].view(dtype) if count else np.empty(0, dtype)
            packets = [samples[j:j + c.chunk_size] for j in range(0, count, c.chunk_size)]
            self._stats["packets"] += len(packets)
            r.flying -= 1
            if r.flying == 0 and r.under_way == 0 and r.next >= r.stop:
                r.done = True
            out.append((r, packets))
        return out

    def run(self):
        """(request, packet, out_rate) until nothing waits.  Closing the generator early leaves the pool usable: what is queued
        stays queued and the packets of the current tick that were not handed out are kept; the next run() goes on from there."""
        while self._outbox or not self.idle():
            if not self._outbox:
                self._outbox = [(r, packet) for r, packets in self.step() for packet in packets]
                continue
            r, packet = self._outbox.pop(0)
            yield r, packet, r.client.out_rate


def open_pool(model, vocoder, voices, *, batch_frames, max_items=64, first_alone=True, lookahead=0, nfe_step=32, cfg_strength=2.0,
              sway_sampling_coef=-1.0, seed=None, text_tokenizer=None, clip_silence=False, slice_steps=None, isolate=False) -> StreamPool:
    """A pool that serves many streaming clients from one model: voices is a VoiceBank or the dict prepare_voices takes (prepared
    once, here).  batch_frames: the budget of a tick, rows x longest row (None: every chunk as its own B = 1 sample(), as in
    open_stream; the ticks then share only the emit); max_items: rows of a tick at most; first_alone: a waiting first chunk keeps
    later chunks out of its tick (pool_tick has the rule); lookahead: ticks enqueued ahead of the one the host waits for;
    slice_steps: None, or the steps a tick runs at most -- the pool then solves in slices and re-forms the batch between them
    (StreamPool has the rules); isolate: every row of a tick is computed as if it were alone in it -- a client's audio does not depend on
    who shares its tick, and equals a session's (batch_frames=None) bit for bit, also with `attn_mask_enabled=False`.  It turns on the
    model's isolated rows (DiT.set_isolated_rows; DiT only) and a graph cache of 64, every tick runs as model.sample_items /
    model.sample_span on packed rows, and batch_frames budgets a tick by the sum of its rows' frames, each rounded up to 4 (what a
    packed tick costs), not rows x longest row.  The
    sampler settings are the pool's defaults: pool.connect may give a client its own.  Refuses what open_stream refuses.  See StreamPool, and pool.connect for a client's side."""
    return StreamPool(model, vocoder, voices, batch_frames=batch_frames, max_items=max_items, first_alone=first_alone,
                      lookahead=lookahead, nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                      seed=seed, text_tokenizer=text_tokenizer, clip_silence=clip_silence, slice_steps=slice_steps, isolate=isolate)
