"""GPU: the batched long-form path -- f5_wave_crossfade against the host fold it replaces (infer.cross_fade_concat cast to f32,
bit for bit), and infer.synthesize_long / infer_batch_process(batched=True) against the composition of the existing public
pieces (model.sample on the same batch, vocoder.decode per item, the RMS rescale, cross_fade_concat), bit for bit; with
attention masking, against today's sequential B = 1 path.  Every input element past a piece's length is NaN and outputs go to
gpu_util.Guarded buffers, so a read or a write outside a piece or outside [0, total) shows."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd.cfm import clamp_durations  # noqa: E402

SR = 24000
PAD = 37     # elements of wav_stride past the longest piece
EXTRA = 5    # elements of out_cap past total

# (piece lengths, cross-fade samples)
KERNEL_CASES = {
    "two_per_sample": ([256, 256, 512], 100),
    "short_pieces": ([30, 10, 5, 40], 16),           # a later piece starts before an earlier one: up to four pieces over a sample
    "shorter_than_fade": ([8, 3, 3, 3, 20], 6),
    "one_sample_pieces": ([1, 1, 1], 4),             # n = 1: fo = 1, fi = 0
    "no_fade": ([50, 60], 0),
    "fade_longer_than_a_piece": ([2048, 256, 1024], 3600),
    "single_piece": ([777], 100),
    "max_pieces": (list(range(3, 67)), 7),           # B = 64
    "real_fade": ([4096, 4100, 300], 3600),          # 0.15 s at 24 kHz, more than one block, the last piece shorter than the fade
}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_pieces(lens, seed):
    g = np.random.default_rng(seed)
    return [g.standard_normal(n).astype(np.float32) for n in lens]


def packed_rows(pieces):
    """[B, longest + PAD] on the device, NaN behind every piece."""
    wav = torch.full((len(pieces), max(len(p) for p in pieces) + PAD), float("nan"))
    for i, p in enumerate(pieces):
        wav[i, :len(p)] = torch.from_numpy(p)
    return wav.to(DEV)


def crossfade_call(wav, lens, cf, out, n):
    return _lib.load().f5_wave_crossfade(C.c_void_p(wav.data_ptr()), len(lens), wav.stride(0), _lib.int_array(lens), cf,
                                         C.c_void_p(out.ptr()), out.n, C.byref(n), _stream())


def check_crossfade(out, n, want, what):
    total = len(want)
    assert n.value == total, f"{what}: out_len_host {n.value}, expected {total}"
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    assert (out.bits[total:] == out.sent).all(), f"{what}: an element at or past total was written"
    assert torch.isfinite(out.value[:total]).all(), f"{what}: an element past a piece's length was read, or a sample was not written"
    got = out.bits[:total].cpu()
    ref = torch.from_numpy(want.view(np.int32))
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {total} samples differ from the host fold"


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_equals_the_host_fold_bit_for_bit(name):
    lens, cf = KERNEL_CASES[name]
    assert int(cf / SR * SR) == cf
    pieces = make_pieces(lens, seed=len(lens) + cf)
    want = I.cross_fade_concat(pieces, cf / SR).astype(np.float32)
    wav = packed_rows(pieces)
    out = Guarded((len(want) + EXTRA,), torch.float32)
    n = C.c_int64(-1)
    rc = crossfade_call(wav, lens, cf, out, n)
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_crossfade(out, n, want, name)
    # the Python wrapper: the same bits in a tensor of exactly `total` samples
    got = I.wave_crossfade(wav, lens, cf)
    assert got.shape == (len(want),) and torch.equal(got.view(torch.int32), out.bits[:len(want)])


def test_kernel_call_is_capturable_and_replays_the_same_result():
    """Captured into a graph, the call launches nothing, allocates nothing and synchronises nothing (either would end the
    capture with an error); the replay writes the same bits."""
    lens, cf = KERNEL_CASES["real_fade"]
    pieces = make_pieces(lens, seed=21)
    want = I.cross_fade_concat(pieces, cf / SR).astype(np.float32)
    wav = packed_rows(pieces)
    out = Guarded((len(want) + EXTRA,), torch.float32)
    n = C.c_int64(-1)
    assert crossfade_call(wav, lens, cf, out, n) == 0        # eager once: the kernel's code object is loaded before the capture
    torch.cuda.synchronize()
    out.raw.fill_(out.sent)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = crossfade_call(wav, lens, cf, out, n)
    assert rc == 0, _lib.load().f5_last_error().decode()
    torch.cuda.synchronize()
    assert (out.bits == out.sent).all(), "the captured call ran during the capture"
    graph.replay()
    torch.cuda.synchronize()
    check_crossfade(out, n, want, "replay")
    out.raw.fill_(out.sent)
    graph.replay()
    torch.cuda.synchronize()
    check_crossfade(out, n, want, "second replay")


# ------------------------------------------------------------------------------------------------ end to end
REF_TEXT = "hello there."
CHUNKS = ["General Kenobi, you are a bold one.", "Yes.", "So uncivilised, this is."]   # "Yes." < 10 bytes: local_speed 0.3
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
TARGET_RMS = 0.1
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def tiny_model(attn_mask):
    def make():
        arch = dict(P.config.F5TTS_TINY, attn_mask_enabled=attn_mask)      # dim 256, depth 2, heads 4
        tr = P.DiT(**arch, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
        return P.CFM(transformer=tr).to(DEV)                               # no vocab map: utf-8 byte tokens
    return cached(("model", attn_mask), make)


def tiny_vocoder():
    return cached("voc", lambda: P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV))


def prompt():
    """0.3 s of noise with RMS 0.05 < target_rms: the rescale runs."""
    return cached("prompt", lambda: torch.randn(1, 7200, generator=torch.Generator().manual_seed(5)) * 0.05)


def composed(model, voc, groups, cross_fade_duration):
    """The expected value from existing public pieces only: per group one model.sample on the batch, then per item
    vocoder.decode of its [ref_len, duration_i) slice, * rms / target_rms, and the host cross-fade cast to f32."""
    waves, specs = [], []
    for run in groups:
        nums = [I.prompt_numerics(prompt(), SR, REF_TEXT, CHUNKS[k]) for k in run]
        a, rms, rtext, ref_len, _ = nums[0]
        texts = [rtext + CHUNKS[k] for k in run]
        cond = model.mel_spec(a.to(DEV)).permute(0, 2, 1).expand(len(run), -1, -1)
        lens = torch.full((len(run),), cond.shape[1], dtype=torch.long)
        duration = torch.tensor([x[4] for x in nums])
        ends = clamp_durations(P.utils.list_str_to_tensor(texts), lens, duration).tolist()
        out, _ = model.sample(cond=cond, text=texts, duration=duration, lens=lens, steps=KW["nfe_step"],
                              cfg_strength=KW["cfg_strength"], sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
        assert rms < TARGET_RMS
        for b in range(len(run)):
            gen = out[b:b + 1, ref_len:ends[b]].permute(0, 2, 1)
            wave = voc.decode(gen) * rms / TARGET_RMS
            waves.append(wave.squeeze().cpu().numpy())
            specs.append(gen[0].cpu().numpy())
    return I.cross_fade_concat(waves, cross_fade_duration).astype(np.float32), np.concatenate(specs, axis=1)


def assert_same_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.shape}"
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print(f"[long form] {what}: {got.shape}, Linf {diff:.3e} (peak {np.abs(want).max():.3e})")
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{what}: Linf {diff:.3e}"


@pytest.mark.parametrize("case", ["one_group", "no_cross_fade", "two_groups"])
def test_batched_equals_the_composition_of_existing_parts(case):
    model, voc = tiny_model(False), tiny_vocoder()
    cfd = 0.0 if case == "no_cross_fade" else I.cross_fade_duration
    groups, batch_frames = [range(3)], None
    if case == "two_groups":
        nums = [I.prompt_numerics(prompt(), SR, REF_TEXT, c) for c in CHUNKS]
        texts = P.utils.list_str_to_tensor([nums[0][2] + c for c in CHUNKS])
        ends = clamp_durations(texts, torch.full((3,), nums[0][3] + 1), torch.tensor([x[4] for x in nums])).tolist()
        batch_frames = 2 * max(ends[:2])                      # the first two chunks fit, the third does not
        groups = I.group_chunks(ends, batch_frames)
        assert [list(r) for r in groups] == [[0, 1], [2]], (ends, batch_frames)
    want_wave, want_spec = composed(model, voc, groups, cfd)
    items = list(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, voc, cross_fade_duration=cfd, batched=True,
                                       batch_frames=batch_frames, **KW))
    assert len(items) == 1
    wave, sr, spec = items[0]
    assert sr == SR and np.isfinite(wave).all()
    assert_same_bits(wave, want_wave, f"{case}: waveform")
    assert_same_bits(spec, want_spec, f"{case}: combined mel")
    # the device-resident form, and infer_process's switch over the same chunks
    dw, dsr, dspec = I.synthesize_long((prompt(), SR), REF_TEXT, CHUNKS, model, voc, cross_fade_duration=cfd,
                                       batch_frames=batch_frames, **KW)
    assert dw.device.type == "cuda" and dspec.device.type == "cuda" and dsr == SR
    assert np.array_equal(dw.cpu().numpy().view(np.int32), wave.view(np.int32)) and np.array_equal(dspec.cpu().numpy(), spec)


def test_chunks_are_independent_where_attention_is_masked():
    """attn_mask_enabled=True: the batch runs valid rows only (RowPack), so every chunk is computed as if alone and the batched
    waveform is today's sequential one (the unchanged B = 1 path), rounded to f32: bit equality, as DESIGN section 2's "a row's
    result does not depend on which tile or batch computed it" predicts."""
    model, voc = tiny_model(True), tiny_vocoder()
    seq_wave, _, seq_spec = next(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, voc, **KW))
    assert seq_wave.dtype == np.float64                      # numpy promoted in the cross-fade
    wave, _, spec = next(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, voc, batched=True, **KW))
    assert_same_bits(spec, seq_spec, "masked attention: combined mel against the sequential path")
    assert_same_bits(wave, seq_wave.astype(np.float32), "masked attention: waveform against the sequential path")


def test_infer_process_switch_and_documented_errors():
    model, voc = tiny_model(False), tiny_vocoder()
    text = " ".join(CHUNKS)
    wave, sr, spec = I.infer_process((prompt(), SR), REF_TEXT, text, model, voc, show_info=None, batched=True, **KW)
    assert wave.dtype == np.float32 and wave.ndim == 1 and sr == SR and spec.shape[0] == 100
    assert wave.shape[0] == (spec.shape[1] - 1) * 256        # one chunk at this prompt's bytes-per-second: no cross-fade
    with pytest.raises(ValueError, match="64"):
        next(I.infer_batch_process((prompt(), SR), REF_TEXT, ["Yes."] * 65, model, voc, batched=True, **KW))
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        next(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, P.BigVGAN(P.config.BIGVGAN_TINY), batched=True, **KW))
    with pytest.raises(ValueError, match="streaming"):
        next(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, voc, batched=True, streaming=True, **KW))
