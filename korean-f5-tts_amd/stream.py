"""Streaming sessions (the reference's serving mode, socket_server.py: TTSStreamingProcessor): a voice prepared once, each request's
text split so that its first chunk is short, and the audio sent packet by packet while later chunks are still being generated.
`stream_chunks` is the host text plan of generate_stream (socket_server.py:112-143); `StreamSession` (infer.open_stream) runs the
chunks on the device path -- the voice from a VoiceBank, ragged sample(), decode_ragged, f5_wave_join, f5_wave_deliver -- and
yields packets at the client's rate and sample format.  The TCP shell and the sound-card code of the server are not here."""
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

        bank, v = self.bank, self.voice
        chunks = stream_chunks(text, bank.ref_texts[v], bank.seconds[v], self._first)
        self._first = False
        texts, durations = [], []
        for chunk in chunks:
            rtext, _ref_len, duration = I.text_numerics(bank.samples[v], bank.ref_texts[v], chunk, self._speed, self.fix_duration)
            texts.append(rtext + chunk)
            durations.append(duration)
        if not chunks:
            return dict(chunks=[], texts=[], durations=[], ends=[], groups=[])
        texts, idx = I._tokenise(self.model, texts, self.text_tokenizer, stacklevel=4)
        ends = I.clamp_durations(idx.to("cpu", torch.long), torch.tensor([bank.frames[v]] * len(chunks)), torch.tensor(durations)).tolist()
        if self.batch_frames is None:
            groups = [range(i, i + 1) for i in range(len(chunks))]
        else:                                                               # the first chunk alone: its audio is what the client waits for
            groups = [range(0, 1)] + [range(r.start + 1, r.stop + 1) for r in I.group_chunks(ends[1:], self.batch_frames)]
        return dict(chunks=chunks, texts=texts, durations=durations, ends=ends, groups=groups)

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
