"""GPU: the ragged prompt mel front-end (f5_mel_forward_ragged, MelSpec.forward_ragged, infer.synthesize_prompts) -- prompts of
unequal length in one pass over packed rows.  The yardstick is the rectangular front-end it stands beside: every item must be
BIT-identical to f5_mel_forward_ex on that item alone with B = 1 (both GEMMs take the v2 kernels, whose K order per element does
not depend on the row count; the magnitude and the log epilogue are element-wise), for lengths whose frame counts put the item
boundaries inside and across 64- / 128-row GEMM tiles, down to the shortest legal prompt.  The items sit in ONE buffer with NaN
between and around them, so a read outside an item shows up in the output; outputs go to gpu_util.Guarded buffers with a NaN
stride gap behind every item's T_out rows: guards and gaps intact, padding rows +0.0 by bit pattern."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd.batching import prompt_text_and_frames  # noqa: E402
from f5_tts_amd.cfm import clamp_durations  # noqa: E402

N_FFT, HOP, N_MELS = 1024, 256, 100
MEL_VARIANTS = {"vocos": (512, 0.0), "bigvgan": (384, 1e-9)}   # (reflect padding, magnitude epsilon)
# vocos: T = 3, 4, 4, 5, 5 (513 is the shortest legal prompt) and 20, 3, 130, 64, 131 (R = 27 + 7 + 134 + 68 + 134 rows: item
# boundaries inside the first 64- / 128-row tile and across tile rounds); bigvgan: 385 is the shortest, a one-frame item
LENGTH_SETS = {
    "vocos": [(513, 768, 1023, 1024, 1025), (5000, 513, 33111, 16383, 33280)],
    "bigvgan": [(385, 640, 1024), (385, 16500, 33111)],
}
CASES = [(v, i) for v, sets in LENGTH_SETS.items() for i in range(len(sets))]
GAPS = (17, 3, 10, 1, 6, 5)   # NaN elements in front of item 0, between the items, behind the last: items start off 16-byte multiples


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def handle(variant):
    return cached(("h", variant), lambda: P.mel.MelSpec(mel_spec_type=variant)._handle(torch.device(DEV)))


def frames_of(variant, nw):
    return (nw + 2 * MEL_VARIANTS[variant][0] - N_FFT) // HOP + 1


def signal(nw):
    return cached(("sig", nw), lambda: torch.randn(nw, generator=torch.Generator().manual_seed(nw)) * 0.1)


def rect_run(h, variant, wav_dev):
    """The existing rectangular front-end on f32 [B, nw] -> Guarded [B, T, n_mels]."""
    pad, eps = MEL_VARIANTS[variant]
    B, nw = wav_dev.shape
    out = Guarded((B, frames_of(variant, nw), N_MELS), torch.float32)
    rc = _lib.load().f5_mel_forward_ex(h, _ptr(wav_dev), B, nw, pad, eps, C.c_void_p(out.ptr()), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().f5_last_error().decode()
    assert out.guards_intact() and not torch.isnan(out.value).any()
    return out


def alone(variant, nw):
    """Item `nw` through f5_mel_forward_ex with B = 1: int32 bits [T, n_mels] on the device (computed once, never modified)."""
    return cached(("ref", variant, nw), lambda: rect_run(handle(variant), variant, signal(nw)[None].to(DEV).contiguous()).bits[0].clone())


def packed_items(nws):
    """(one device buffer, element offset per item): the items in order, NaN in front, between and behind."""
    parts, starts, off = [], [], 0
    for i, nw in enumerate(nws):
        gap = GAPS[i % len(GAPS)]
        parts += [torch.full((gap,), float("nan")), signal(nw)]
        starts.append(off + gap)
        off += gap + nw
    parts.append(torch.full((GAPS[len(nws) % len(GAPS)],), float("nan")))
    return torch.cat(parts).to(DEV), starts


def ragged_run(h, variant, nws, T_extra=0, gap=0):
    """f5_mel_forward_ragged -> (rc, Guarded [B, T_out * n_mels + gap], T_out)."""
    pad, eps = MEL_VARIANTS[variant]
    wav, starts = packed_items(nws)
    T_out = max(frames_of(variant, nw) for nw in nws) + T_extra
    out = Guarded((len(nws), T_out * N_MELS + gap), torch.float32)
    rc = _lib.load().f5_mel_forward_ragged(h, _ptr(wav), len(nws), (C.c_int64 * len(nws))(*starts), _lib.int_array(nws), pad, eps,
                                           C.c_void_p(out.ptr()), T_out * N_MELS + gap, T_out, _stream())
    torch.cuda.synchronize()
    return rc, out, T_out


def check_ragged(out, T_out, variant, nws, what):
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    rows = out.bits[:, :T_out * N_MELS].view(len(nws), T_out, N_MELS)
    assert (out.bits[:, T_out * N_MELS:] == out.sent).all(), f"{what}: the stride gap behind T_out rows was written"
    assert not (rows == out.sent).any(), f"{what}: {int((rows == out.sent).sum())} output elements never written"
    assert torch.isfinite(out.value[:, :T_out * N_MELS]).all(), f"{what}: something outside an item's samples was read"
    for b, nw in enumerate(nws):
        T = frames_of(variant, nw)
        ref = alone(variant, nw)
        assert torch.equal(rows[b, :T], ref), \
            f"{what}: item {b} (nw = {nw}, T = {T}) differs from the rectangular front-end on it alone in {int((rows[b, :T] != ref).sum())} of {T * N_MELS} values"
        assert not rows[b, T:].any(), f"{what}: item {b}: the rows behind its {T} frames are not all +0.0"


@pytest.mark.parametrize("variant,k", CASES)
def test_ragged_items_bit_equal_the_rectangular_front_end(variant, k):
    """Per item bit-identity, padding rows, guard bands and stride gaps; T_out = the maximum and the maximum + 5; the item order
    and its reverse."""
    h = handle(variant)
    nws = LENGTH_SETS[variant][k]
    for order, T_extra, gap in ((nws, 0, 0), (nws, 5, 36), (nws[::-1], 0, 7)):   # gap 7: out_stride_b off 16 bytes (scalar stores)
        rc, out, T_out = ragged_run(h, variant, order, T_extra, gap)
        assert rc == 0, _lib.load().f5_last_error().decode()
        check_ragged(out, T_out, variant, order, f"{variant} {order} T_out +{T_extra} gap {gap}")


@pytest.mark.parametrize("variant", list(MEL_VARIANTS))
def test_one_item_equals_the_rectangular_call(variant):
    h = handle(variant)
    rc, out, T_out = ragged_run(h, variant, (5000,))
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_ragged(out, T_out, variant, (5000,), "B = 1")
    want = rect_run(h, variant, signal(5000)[None].to(DEV).contiguous())
    assert torch.equal(out.bits.view(1, T_out, N_MELS), want.bits)


def test_workspace_reuse_across_ragged_and_rectangular_calls():
    """One fresh handle: a large ragged call, a rectangular call, a small ragged call, the large one again (the workspace only
    grows and is never cleared; the ragged calls' device tables live in it): every result equals the first-run result."""
    variant = "vocos"
    h = P.mel.MelSpec(mel_spec_type=variant)._handle(torch.device(DEV))
    small, large = LENGTH_SETS[variant]
    rect_in = torch.stack([signal(7000), signal(7000).flip(0)]).to(DEV).contiguous()
    want_rect = rect_run(handle(variant), variant, rect_in).bits.clone()
    first = {}
    for step in ("large", "rect", "small", "large", "rect"):
        if step == "rect":
            got = rect_run(h, variant, rect_in).bits.clone()
            assert torch.equal(got, want_rect), "the rectangular call behind a ragged one differs from a first run"
            continue
        nws = large if step == "large" else small
        rc, out, T_out = ragged_run(h, variant, nws, 2, 12)
        assert rc == 0, _lib.load().f5_last_error().decode()
        check_ragged(out, T_out, variant, nws, f"reuse: {step}")
        if step in first:
            assert torch.equal(out.bits, first[step]), f"{step}: a repeated call differs"
        first[step] = out.bits.clone()


@pytest.mark.parametrize("variant", list(MEL_VARIANTS))
def test_forward_ragged_input_forms(variant):
    ms = P.mel.MelSpec(mel_spec_type=variant)
    nws = LENGTH_SETS[variant][1]
    host = [signal(nw) for nw in nws]
    mel, frames = ms.forward_ragged(host, device=DEV)
    T = max(frames)
    assert frames == [frames_of(variant, nw) for nw in nws]
    assert mel.shape == (len(nws), N_MELS, T) and mel.stride() == (T * N_MELS, 1, N_MELS) and mel.device.type == "cuda"
    for b, w in enumerate(host):
        one = ms(w[None].to(DEV))                                          # [1, n_mels, T_b]
        assert torch.equal(mel[b, :, :frames[b]].view(torch.int32), one[0].view(torch.int32)), f"item {b} differs from forward() on it alone"
        assert not mel[b, :, frames[b]:].view(torch.int32).any()
    bits = mel.view(torch.int32)
    on_dev = [w.to(DEV) for w in host]
    forms = {
        "device tensors": on_dev,
        "[1, nw] host tensors": [w[None] for w in host],
        "[1, nw] device tensors": [w[None] for w in on_dev],
        "host and device mixed": [w if i % 2 else d for i, (w, d) in enumerate(zip(host, on_dev))],
    }
    for name, wavs in forms.items():
        got, fr = ms.forward_ragged(wavs) if "host tensors" not in name else ms.forward_ragged(wavs, device=DEV)
        assert fr == frames and torch.equal(got.view(torch.int32), bits), f"{name}: the input form changed the result"


# ---- infer.synthesize_prompts against the per-item sequence it replaces
SR = 24000
TARGET_RMS = 0.1
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)


def tiny_model():
    def make():
        tr = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
        return P.CFM(transformer=tr).to(DEV)                               # no vocab map: utf-8 byte tokens
    return cached("model", make)


def tiny_vocoder():
    return cached("voc", lambda: P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV))


def prompts():
    """Four speakers: different lengths, one at 44.1 kHz (stereo), one louder than target_rms (no rescale for that row)."""
    def make():
        g = torch.Generator().manual_seed(5)
        return [
            (torch.randn(1, 7200, generator=g) * 0.05, SR, "Some call me nature."),
            (torch.randn(2, 11025, generator=g) * 0.05, 44100, "안녕하세요"),              # -> 6000 samples at 24 kHz
            (torch.randn(1, 9001, generator=g) * 0.3, SR, "Others call me mother nature!"),
            (torch.randn(1, 5555, generator=g) * 0.02, SR, "Good morning"),
        ]
    return cached("prompts", make)


GEN_TEXTS = ["I am the wind.", "반갑습니다.", "The quick brown fox jumps over the lazy dog.", "Yes, indeed."]


def sequence(model, voc, run):
    """The reference's sequence for the items of one group, from existing public pieces only: normalise_prompt and MelSpec.forward
    per item, zero-pad and stack (padded_mel_batch), model.sample on the batch, vocoder.decode per item, the rescale."""
    items = [prompts()[k] for k in run]
    norm = [I.normalise_prompt(a, sr, TARGET_RMS) for a, sr, _ in items]
    mels = [model.mel_spec(a.to(DEV)).permute(0, 2, 1)[0] for a, _ in norm]          # [T_i, 100]
    lens = [m.shape[0] for m in mels]
    cond = torch.zeros(len(items), max(lens), 100, device=DEV)
    for i, m in enumerate(mels):
        cond[i, :lens[i]] = m
    pairs = [prompt_text_and_frames(n, rt, GEN_TEXTS[k], 1.0) for n, (_, _, rt), k in zip(lens, items, run)]
    texts, durs = [p[0] for p in pairs], torch.tensor([p[1] for p in pairs])
    out, _ = model.sample(cond, texts, durs, lens=torch.tensor(lens), steps=KW["nfe_step"], cfg_strength=KW["cfg_strength"],
                          sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
    ends = clamp_durations(P.utils.list_str_to_tensor(texts), torch.tensor(lens), durs).tolist()
    waves, specs = [], []
    for i, (_, rms) in enumerate(norm):
        gen = out[i:i + 1, lens[i]:ends[i]].permute(0, 2, 1).to(torch.float32)
        wave = voc.decode(gen)
        if rms < TARGET_RMS:
            wave = wave * rms / TARGET_RMS
        waves.append(wave[0])
        specs.append(gen[0])
    return waves, specs, ends


@pytest.mark.parametrize("case", ["one_group", "two_groups"])
def test_synthesize_prompts_equals_the_per_item_sequence(case):
    model, voc = tiny_model(), tiny_vocoder()
    rms = [I.normalise_prompt(a, sr, TARGET_RMS)[1] for a, sr, _ in prompts()]
    assert [r < TARGET_RMS for r in rms] == [True, True, False, True]
    groups, batch_frames = [range(4)], None
    if case == "two_groups":
        ends = sequence(model, voc, range(4))[2]
        batch_frames = 2 * max(ends)
        groups = I.group_chunks(ends, batch_frames)
        assert [list(r) for r in groups] == [[0, 1], [2, 3]], (ends, batch_frames)
    want_waves, want_specs = [], []
    for run in groups:                        # per group: an unmasked batch sees its own padding
        w, s, _ = sequence(model, voc, run)
        want_waves += w
        want_specs += s
    waves, sr, specs = I.synthesize_prompts(model, voc, prompts(), GEN_TEXTS, target_rms=TARGET_RMS, batch_frames=batch_frames, **KW)
    assert sr == SR and len(waves) == len(specs) == 4
    for i in range(4):
        assert waves[i].dim() == 1 and waves[i].device.type == "cuda" and torch.isfinite(waves[i]).all()
        assert waves[i].shape == want_waves[i].shape and specs[i].shape == want_specs[i].shape
        assert torch.equal(specs[i].view(torch.int32), want_specs[i].view(torch.int32)), f"{case}: item {i}: generated mel differs"
        assert torch.equal(waves[i].view(torch.int32), want_waves[i].view(torch.int32)), f"{case}: item {i}: waveform differs"
