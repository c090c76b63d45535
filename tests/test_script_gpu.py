"""GPU: the multi-voice script -- f5_wave_join / infer.wave_join against the host join it replaces (cross_fade_concat per run,
concatenated, cast to f32; script_oracle.host_join) bit for bit, and infer.synthesize_script / prepare_voices against
synthesize_long per stretch (masked attention) and against the composition of the existing public parts on the same groups
(unmasked).  Every piece lies between NaN and outputs go to gpu_util.Guarded buffers, so a read outside a piece or a write
outside [0, total) shows."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import script_oracle as O  # noqa: E402
from test_long_form_gpu import assert_same_bits, cached, tiny_model, tiny_vocoder  # noqa: E402

from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd.cfm import clamp_durations  # noqa: E402
from f5_tts_amd.utils import list_str_to_tensor  # noqa: E402

SR = 24000
EXTRA = 5    # elements of out_cap past total
F5_EINVAL = -1


def _short_runs():
    g = np.random.default_rng(11)
    lens = g.integers(1, 8, size=1000).tolist()
    return [lens[:400], lens[400:401], lens[401:751], lens[751:]]


KERNEL_CASES = dict(O.JOIN_CASES)
KERNEL_CASES["thousand_short_pieces"] = (_short_runs(), 4)                       # the lookup; many pieces over one sample
KERNEL_CASES["tile_boundaries"] = ([[1023, 1025, 2048], [2048, 1023], [1025]], 100)
KERNEL_CASES["real_fade"] = ([[4096, 4100, 300], [9000, 5000]], 3600)            # several blocks; a piece shorter than the fade


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def place(pieces, memory_order=None, tensors=1):
    """The pieces as views of `tensors` device buffers, laid down in memory_order (default: as given) with one to three NaN
    in front of, between and behind them (so most pieces start off a 16-byte multiple).  Returns the views in piece order."""
    memory_order = list(range(len(pieces))) if memory_order is None else list(memory_order)
    views = [None] * len(pieces)
    for t in range(tensors):
        mine, at, spans = memory_order[t::tensors], 1 + t, []
        for i in mine:
            spans.append((i, at))
            at += len(pieces[i]) + 1 + i % 3
        host = torch.full((at,), float("nan"))
        for i, a in spans:
            host[a:a + len(pieces[i])] = torch.from_numpy(pieces[i])
        dev = host.to(DEV)
        for i, a in spans:
            views[i] = dev[a:a + len(pieces[i])]
    return views


def join_call(views, fades, out, n, B=None, starts=None, lens=None, base=None, out_ptr=None, cap=None):
    first = min(v.data_ptr() for v in views)
    starts = [(v.data_ptr() - first) // 4 for v in views] if starts is None else starts
    lens = [v.shape[0] for v in views] if lens is None else lens
    return _lib.load().f5_wave_join(C.c_void_p(first) if base is None else base, len(views) if B is None else B,
                                    (C.c_int64 * len(starts))(*starts), _lib.int_array(lens), _lib.int_array(fades),
                                    C.c_void_p(out.ptr()) if out_ptr is None else out_ptr, out.n if cap is None else cap, C.byref(n),
                                    _stream())


def check_join(out, n, want, what, shift=0):
    """out: a Guarded that received the result `shift` elements in."""
    total = len(want)
    assert n.value == total, f"{what}: out_len_host {n.value}, expected {total}"
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    assert (out.bits[:shift] == out.sent).all(), f"{what}: an element in front of out was written"
    assert (out.bits[shift + total:] == out.sent).all(), f"{what}: an element at or past total was written"
    assert torch.isfinite(out.value[shift:shift + total]).all(), f"{what}: an element outside a piece was read, or a sample was not written"
    got = out.bits[shift:shift + total].cpu()
    ref = torch.from_numpy(want.view(np.int32))
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {total} samples differ from the host join"


@pytest.mark.parametrize("shuffled", [False, True], ids=["in_order", "shuffled_in_two_tensors"])
@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_equals_the_host_join_bit_for_bit(name, shuffled):
    runs, fade = KERNEL_CASES[name]
    pieces, fades = O.flat(O.pieces_of(runs, seed=len(runs) + fade), fade)
    want = O.host_join(O.pieces_of(runs, seed=len(runs) + fade), fade)
    if shuffled:
        views = place(pieces, np.random.default_rng(3).permutation(len(pieces)).tolist(), tensors=2)
    else:
        views = place(pieces)
    for shift in (0, 1):                                    # the output on a 16-byte multiple, and one element off it
        out = Guarded((shift + len(want) + EXTRA,), torch.float32)
        n = C.c_int64(-1)
        rc = join_call(views, fades, out, n, out_ptr=C.c_void_p(out.ptr() + 4 * shift), cap=out.n - shift)
        torch.cuda.synchronize()
        assert rc == 0, _lib.load().f5_last_error().decode()
        check_join(out, n, want, f"{name}, out {shift} elements off a 16-byte multiple", shift)
    # the Python wrapper: the same bits in a tensor of exactly `total` samples
    got = I.wave_join(views, fades)
    assert got.shape == (len(want),) and torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(want.view(np.int32)))


def test_a_single_run_is_wave_crossfade():
    lens, cf = [4096, 4100, 300, 777], 3600
    g = torch.Generator().manual_seed(8)
    wav = torch.full((len(lens), max(lens) + 37), float("nan"))
    for i, ln in enumerate(lens):
        wav[i, :ln] = torch.randn(ln, generator=g)
    wav = wav.to(DEV)
    want = I.wave_crossfade(wav, lens, cf)
    got = I.wave_join([wav[i, :ln] for i, ln in enumerate(lens)], [0] + [cf] * (len(lens) - 1))
    assert torch.equal(got, want) and torch.isfinite(got).all()


def test_documented_refusals_leave_the_output_untouched():
    pieces = [p for run in O.pieces_of([[10, 20, 15]]) for p in run]
    views = place(pieces)
    fades = [0, 4, 0]                                       # total = 10 + 20 - 4 + 15 = 41
    out = Guarded((41 + EXTRA,), torch.float32)
    n = C.c_int64(-7)

    def refused(word, **kw):
        assert join_call(views, kw.pop("fades", fades), out, n, **kw) == F5_EINVAL
        msg = _lib.load().f5_last_error()
        assert msg.startswith(b"f5_wave_join:") and word in msg, msg
        assert n.value == -7, "a refused call wrote out_len_host"

    refused(b"B", B=0)
    refused(b"B", B=65536)
    refused(b"base", base=C.c_void_p(0))
    refused(b"out", out_ptr=C.c_void_p(0))
    refused(b"lens_host[1]", lens=[10, 0, 15])
    refused(b"fade_host[2]", fades=[0, 4, -1])
    refused(b"start_host[0]", starts=[-1, 11, 33])
    refused(b"out_cap", cap=40)
    lib = _lib.load()
    for missing in (2, 3, 4):                               # start_host, lens_host, fade_host
        args = [C.c_void_p(views[0].data_ptr()), 3, (C.c_int64 * 3)(0, 11, 33), _lib.int_array([10, 20, 15]), _lib.int_array(fades),
                C.c_void_p(out.ptr()), out.n, C.byref(n), _stream()]
        args[missing] = None
        assert lib.f5_wave_join(*args) == F5_EINVAL and lib.f5_last_error().startswith(b"f5_wave_join:")
    torch.cuda.synchronize()
    assert (out.raw == out.sent).all(), "a refused call wrote to the output"
    # and the same arguments, unspoiled, are accepted
    assert join_call(views, fades, out, n) == 0, lib.f5_last_error().decode()
    torch.cuda.synchronize()
    check_join(out, n, O.host_join([pieces[:2], pieces[2:]], 4), "accepted")


# ------------------------------------------------------------------------------------------------ end to end
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
TARGET_RMS = 0.1
BOLD = "General Kenobi, you are a bold one."
FIX = 0.6                                                    # int(0.6 * 24000 / 256) = 56 frames; longer texts run at their length + 1


def voices():
    """ann: 0.3 s of 24 kHz mono noise, RMS 0.05 < target_rms (the rescale runs), 3 bytes of text: max_chars = int(3 / 0.3 * 21.7)
    = 217.  bob: 0.5 s of 16 kHz stereo, RMS about 0.2 (no rescale).  cy: never spoken."""
    def make():
        g = torch.Generator().manual_seed(5)
        return {
            "ann": dict(ref_audio=(torch.randn(1, 7200, generator=g) * 0.05, 24000), ref_text="Oh."),
            "bob": dict(ref_audio=(torch.randn(2, 8000, generator=g) * 0.28, 16000), ref_text="Yes."),
            "cy": dict(ref_audio=(torch.randn(1, 9000, generator=g) * 0.1, 22050), ref_text="hello there."),
        }
    return cached("script voices", make)


# stretches ann (7 sentences, 251 bytes: two chunks, a cross-fade), bob, ann; text in front of the first tag goes to the default
SCRIPT = " ".join([BOLD] * 7) + " [bob] So uncivilised, this is. [ann] " + BOLD


def per_stretch(model, voc, vs, script, default, **kw):
    """The reference's route with today's public parts: parse, then one synthesize_long per stretch with that voice's prompt and
    speed, chunked as infer_process chunks.  Returns (waves, mels, stretches)."""
    stretches = O.reference_parse(script, vs, default)
    waves, mels = [], []
    for voice, text in stretches:
        audio, sr = vs[voice]["ref_audio"]
        speed = vs[voice].get("speed", kw.get("speed", 1.0))
        ref_text = vs[voice]["ref_text"]
        max_chars = int(len(ref_text.encode("utf-8")) / (audio.shape[-1] / sr) * (22 - audio.shape[-1] / sr) * speed)
        wave, _, mel = I.synthesize_long((audio, sr), ref_text, I.chunk_text(text, max_chars=max_chars), model, voc,
                                         prompt_on_device=True, **dict(kw, speed=speed), **KW)
        waves.append(wave)
        mels.append(mel)
    return waves, mels, stretches


def same_device_bits(got, want, what):
    assert got.device.type == "cuda" and got.dtype == torch.float32
    assert_same_bits(got.cpu().numpy(), want.cpu().numpy() if torch.is_tensor(want) else want, what)


def check_segments(segments, stretches, waves):
    at = 0
    assert len(segments) == len(stretches)
    for seg, (voice, text), wave in zip(segments, stretches, waves):
        assert seg == (voice, text, at, at + wave.shape[0])
        at += wave.shape[0]


def test_one_voice_without_a_tag_is_synthesize_long():
    model, voc = tiny_model(False), tiny_vocoder()
    vs = {"main": voices()["ann"]}
    text = BOLD + " Yes."                                    # one chunk at this prompt's bytes per second, natural durations
    wave, sr, mel, segments = I.synthesize_script(model, voc, vs, text, **KW)
    (want,), (want_mel,), stretches = per_stretch(model, voc, vs, text, "main")
    assert sr == SR and stretches == [("main", text)]
    same_device_bits(wave, want, "one voice: waveform against synthesize_long")
    same_device_bits(mel, want_mel, "one voice: mel against synthesize_long")
    assert segments == [("main", text, 0, wave.shape[0])]


@pytest.mark.parametrize("split", [False, True], ids=["one_group", "two_groups"])
def test_masked_attention_every_stretch_is_synthesize_long_alone(split):
    """attn_mask_enabled=True: the backbone runs the valid rows only, so an item does not see its neighbours or their prompts."""
    model, voc, vs = tiny_model(True), tiny_vocoder(), voices()
    waves, mels, stretches = cached("masked per stretch", lambda: per_stretch(model, voc, vs, SCRIPT, "ann", fix_duration=FIX))
    assert [v for v, _ in stretches] == ["ann", "bob", "ann"]
    batch_frames = None
    if split:
        batch_frames = 2 * (3 + 1 + 215 + 1)                 # the two chunks of stretch 0 ("Oh. " + 215 bytes, + 1) fill a group
    wave, sr, mel, segments = I.synthesize_script(model, voc, vs, SCRIPT, fix_duration=FIX, batch_frames=batch_frames,
                                                  default="ann", **KW)
    assert sr == SR
    same_device_bits(wave, torch.cat(waves), f"masked, split={split}: waveform against synthesize_long per stretch")
    same_device_bits(mel, torch.cat(mels, dim=1), f"masked, split={split}: mel")
    check_segments(segments, stretches, waves)
    # stretch 0: chunks of 220 and 56 frames behind ann's 28, cross-faded over 3600 samples
    assert waves[0].shape[0] == (220 - 28 - 1 + 56 - 28 - 1) * 256 - 3600, "stretch 0 was not cross-faded: the case lost its point"


def composed(model, voc, bank, plan, stretches, groups, cross_fade_duration):
    """The expected value from existing public parts: per group one model.sample on the bank's mel rows, then per item
    vocoder.decode of its frames behind its own prompt, the rescale with that voice's rms, cross_fade_concat per stretch and
    np.concatenate."""
    items = plan["items"]
    lens = [bank.frames[it[0]] for it in items]
    starts = [bank.samples[it[0]] // 256 for it in items]
    ends = clamp_durations(list_str_to_tensor([it[2] for it in items]), torch.tensor(lens), torch.tensor([it[3] for it in items])).tolist()
    waves, specs = [[] for _ in stretches], []
    for run in groups:
        glens = [lens[k] for k in run]
        cond = torch.stack([bank.mel[items[k][0], :max(glens)] for k in run])
        out, _ = model.sample(cond=cond, text=[items[k][2] for k in run], duration=torch.tensor([items[k][3] for k in run]),
                              lens=torch.tensor(glens), steps=KW["nfe_step"], cfg_strength=KW["cfg_strength"],
                              sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
        for b, k in enumerate(run):
            gen = out[b:b + 1, starts[k]:ends[k]].permute(0, 2, 1)
            wave = I.rescale_to_prompt(voc.decode(gen), bank.rms[items[k][0]], TARGET_RMS)
            waves[items[k][1]].append(wave.squeeze().cpu().numpy())
            specs.append(gen[0].cpu().numpy())
    joined = np.concatenate([I.cross_fade_concat(w, cross_fade_duration) for w in waves]).astype(np.float32)
    return joined, np.concatenate(specs, axis=1), ends


@pytest.mark.parametrize("split", [False, True], ids=["one_group", "two_groups"])
def test_unmasked_attention_equals_the_composition_of_existing_parts(split):
    model, voc, vs = tiny_model(False), tiny_vocoder(), voices()
    bank = cached("bank", lambda: I.prepare_voices(model, vs, target_rms=TARGET_RMS))
    stretches = I.parse_script(SCRIPT, bank.names, "ann")
    plan = I.script_plan(stretches, bank.prompts(), fix_duration=FIX, cross_fade_duration=I.cross_fade_duration)
    assert [it[:2] for it in plan["items"]] == [(0, 0), (0, 0), (1, 1), (0, 2)] and plan["fades"] == [0, 3600, 0, 0]
    batch_frames, groups = None, [range(4)]
    if split:
        batch_frames, groups = 2 * 220, [range(0, 2), range(2, 4)]
    want_wave, want_mel, ends = composed(model, voc, bank, plan, stretches, groups, I.cross_fade_duration)
    assert [list(r) for r in I.group_chunks(ends, batch_frames)] == [list(r) for r in groups], (ends, batch_frames)
    wave, _, mel, segments = I.synthesize_script(model, voc, bank, SCRIPT, fix_duration=FIX, batch_frames=batch_frames, default="ann", **KW)
    same_device_bits(wave, want_wave, f"unmasked, split={split}: waveform against the composition")
    same_device_bits(mel, want_mel, f"unmasked, split={split}: mel")
    assert [s[:2] for s in segments] == stretches and segments[0][2] == 0 and segments[-1][3] == len(want_wave)
    assert all(a[3] == b[2] for a, b in zip(segments, segments[1:]))


def test_a_bank_is_prepared_once_and_reused():
    model, voc, vs = tiny_model(False), tiny_vocoder(), voices()
    ms, calls = model.mel_spec, []
    real = {name: getattr(ms, name) for name in ("prepare_ragged", "forward_ragged")}

    def counting(name):
        def call(items, *a, **k):
            calls.append((name, len(items)))
            return real[name](items, *a, **k)
        return call

    try:
        for name in real:
            setattr(ms, name, counting(name))
        direct = I.synthesize_script(model, voc, vs, SCRIPT, fix_duration=FIX, default="ann", **KW)
        assert calls == [("prepare_ragged", 2), ("forward_ragged", 2)], "one pass each, over the two voices the script uses"
        del calls[:]
        bank = I.prepare_voices(model, vs, target_rms=TARGET_RMS)
        assert calls == [("prepare_ragged", 3), ("forward_ragged", 3)]
        assert bank.mel.device.type == "cuda" and bank.mel.shape[0] == 3 and bank.mel.shape[2] == 100 and bank.rms.shape == (3,)
        assert bank.rms.device.type == "cuda" and bank.names == ["ann", "bob", "cy"] and bank.samples[:2] == [7200, 12000]
        del calls[:]
        first = I.synthesize_script(model, voc, bank, SCRIPT, fix_duration=FIX, default="ann", **KW)
        second = I.synthesize_script(model, voc, bank, SCRIPT, fix_duration=FIX, default="ann", **KW)
        assert calls == [], "a call with a bank prepared a prompt again"
    finally:
        for name in real:
            delattr(ms, name)
    for other, what in ((second, "second call with the bank"), (direct, "voices as a dict")):
        assert torch.equal(first[0].view(torch.int32), other[0].view(torch.int32)), what
        assert torch.equal(first[2].view(torch.int32), other[2].view(torch.int32)) and first[3] == other[3], what


def test_a_voices_speed_changes_only_that_voices_durations():
    model, voc = tiny_model(False), tiny_vocoder()
    vs = {k: dict(v) for k, v in voices().items()}
    script = BOLD + " [bob] " + BOLD + " [ann] Yes, a bold one indeed."
    plain = I.synthesize_script(model, voc, vs, script, default="ann", **KW)[3]
    vs["bob"]["speed"] = 2.0
    fast = I.synthesize_script(model, voc, vs, script, default="ann", **KW)[3]
    length = lambda seg: seg[3] - seg[2]                     # noqa: E731
    assert [length(s) for s in plain[::2]] == [length(s) for s in fast[::2]]
    # bob: 12000 samples at 24 kHz, 46 frames, "Yes. " = 5 bytes; the generated frames are int(46 / 5 * 35 / speed), less one, times the hop
    assert length(plain[1]) == (int(46 / 5 * 35 / 1.0) - 1) * 256 and length(fast[1]) == (int(46 / 5 * 35 / 2.0) - 1) * 256
