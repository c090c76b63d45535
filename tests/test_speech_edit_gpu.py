"""GPU: speech editing -- f5_edit_assemble / MelSpec.edit_assemble against the per-frame host construction and the torch.cat
chain, f5_wave_splice / infer.wave_splice against the float64 per-sample fold (tests/edit_oracle.py), both bit for bit, and
infer.speech_edit against the composition of the existing public pieces (MelSpec.forward, torch.cat, model.sample(edit_mask=...),
vocoder.decode, rescale_to_prompt), bit for bit.  Inputs carry -0.0 in every case and NaN wherever nothing may be read (behind T_i
in the packed mels, behind L in the decoded rows, between the originals); outputs of the C-level calls go to gpu_util.Guarded
buffers.  Bits are compared as int32, which is torch.equal made strict about the sign of zero.
Not checked here: that the prompt_on_device route runs no torch.cuda.synchronize / .item() between the preparation and the returned
tensors -- test_prompt_prepare_gpu.py has no such check for its drivers that this one could follow."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import edit_oracle as O  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402

SR, HOP, NM = 24000, 256, 100
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, f"{what}: {got.shape} {got.dtype} against {want.shape}"
    diff = int((bits(got) != bits(want)).sum())
    assert diff == 0, f"{what}: {diff} of {got.numel()} elements differ in their bits"


def fake_mel(T, seed, row=NM):
    """[T, row] of noise with -0.0 sprinkled in."""
    m = torch.randn(T, row, generator=torch.Generator().manual_seed(seed))
    m.view(-1)[::7] = -0.0
    return m


# ------------------------------------------------------------------------------------------------ assembly
@pytest.mark.parametrize("name", list(O.PLAN_CASES))
def test_assemble_one_recording(name):
    n_frames, parts, fix = O.PLAN_CASES[name]
    mel = fake_mel(n_frames, seed=n_frames + len(parts))
    plan = I.edit_plan(n_frames, parts, fix)
    view = mel[None].to(DEV).permute(0, 2, 1)                       # [1, 100, T], as MelSpec.forward returns it
    cond, mask, D = P.mel.MelSpec().edit_assemble(view, [n_frames], [plan])
    want = O.assemble([mel], [O.frame_map(n_frames, parts, fix)])
    cat_cond, cat_mask = O.cat_construction(mel[None], parts, fix)
    assert D == [want.shape[1]] and cond.device.type == "cuda" and mask.device.type == "cpu"
    same_bits(cond, want, name)
    same_bits(cond, cat_cond, f"{name}: against the torch.cat chain")
    assert torch.equal(cond.cpu(), cat_cond) and torch.equal(mask, cat_mask)


BATCH = [(5, [(0.02, 0.04)], [0.5]),                                 # frames [2, 4) become 47: D = 50
         (37,) + O.PLAN_CASES["no_parts"][1:],                        # D = 37
         O.PLAN_CASES["two_parts_fixed"]]                             # T = 64


def packed_batch():
    """(storage [3, 64, 100] on the host with NaN behind every T_i, mels, maps)."""
    mels = [fake_mel(T, seed=10 + T) for T, _, _ in BATCH]
    store = torch.full((len(BATCH), 64, NM), float("nan"))
    for b, m in enumerate(mels):
        store[b, :m.shape[0]] = m
    return store, mels, [O.frame_map(*c) for c in BATCH]


def test_assemble_three_recordings_of_unequal_length():
    store, mels, maps = packed_batch()
    frames = [c[0] for c in BATCH]
    assert frames == [5, 37, 64]
    plans = [I.edit_plan(*c) for c in BATCH]
    cond, mask, D = P.mel.MelSpec().edit_assemble(store.to(DEV).permute(0, 2, 1), frames, plans)
    want = O.assemble(mels, maps)
    assert D == [len(m) for m in maps] and len(set(D)) == 3 and cond.shape == want.shape
    assert torch.isfinite(cond).all(), "something behind an item's frames was read"
    same_bits(cond, want, "B = 3")
    for b, d in enumerate(D):
        assert (bits(cond[b, d:]) == 0).all(), f"item {b}: the frames behind D are not +0.0"
        cat_cond, cat_mask = O.cat_construction(mels[b][None], *BATCH[b][1:])
        same_bits(cond[b:b + 1, :d], cat_cond, f"item {b} against the torch.cat chain")
        assert torch.equal(mask[b, :d], cat_mask[0]) and mask[b, d:].all()
    # every EDIT frame is +0.0 too (sign bit included)
    for b, fm in enumerate(maps):
        edit = torch.tensor([s < 0 for s in fm])
        assert (bits(cond[b, :len(fm)].cpu())[edit] == 0).all()


@pytest.mark.parametrize("row, shift", [(100, 0), (100, 1), (7, 0), (6, 2)])
def test_assemble_c_level_vector_and_element_paths(row, shift):
    """The 16-byte path (row 100, aligned bases) and the element path (a base 4 bytes off, rows of 7 and 6 elements): the same
    bits, nothing written outside cond, nothing read outside the items' frames."""
    frames = [c[0] for c in BATCH]
    mels = [fake_mel(T, seed=20 + T, row=row) for T in frames]
    maps = [O.frame_map(*c) for c in BATCH]
    plans = [I.edit_plan(*c) for c in BATCH]
    T_max, D = 64, [len(m) for m in maps]
    flat = torch.full((shift + 3 * T_max * row,), float("nan"))
    for b, m in enumerate(mels):
        flat[shift + b * T_max * row: shift + b * T_max * row + m.numel()] = m.reshape(-1)
    flat = flat.to(DEV)
    out = Guarded((shift + 3 * max(D) * row,), torch.float32)
    counts, segs = P.edit.segment_table(plans)
    rc = _lib.load().f5_edit_assemble(C.c_void_p(flat.data_ptr() + 4 * shift), 3, T_max * row, row, _lib.int_array(frames),
                                      _lib.int_array(counts), _lib.int_array(segs), _lib.int_array(D),
                                      C.c_void_p(out.ptr() + 4 * shift), max(D), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().f5_last_error().decode()
    assert out.guards_intact() and (out.bits[:shift] == out.sent).all(), "something outside cond was written"
    same_bits(out.value[shift:].view(3, max(D), row), O.assemble(mels, maps), f"row {row}, base shifted by {shift} elements")


# ------------------------------------------------------------------------------------------------ splice
# name -> (cross_fade_samples, [(L, n, KEEP segments (dst, src, frames))]); hop 256
SPLICE_CASES = {
    "no_fade": (0, [(1280, 1380, [(0, 0, 2), (3, 3, 2)])]),
    "fade_240": (240, [(1536, 1800, [(0, 0, 2), (3, 4, 2)])]),                  # the second KEEP is shifted, as after a fix_duration
    "fade_clamped_to_half_a_frame": (240, [(1280, 1280, [(2, 2, 1)])]),          # m = 128
    "two_samples_left": (240, [(1280, 514, [(2, 2, 3)])]),                       # p1 - p0 = 2: m = 1
    "keeps_at_both_ends": (240, [(1280, 1280, [(0, 0, 1), (4, 4, 1)])]),         # no outer fade
    "original_shorter_than_its_frames": (240, [(1280, 1081, [(0, 0, 2), (3, 3, 2)])]),   # [1081, 1280) falls to the generated samples
    "odd_length_unaligned_row": (240, [(1023, 1100, [(0, 0, 2), (3, 3, 1)])]),
    "three_items": (240, [(1280, 1380, [(0, 0, 2), (3, 3, 2)]), (515, 600, [(1, 1, 1)]), (2051, 2100, [(0, 0, 3), (5, 4, 4)])]),
    "signed_zeros_only": (100, [(1280, 1380, [(0, 0, 2), (3, 3, 2)])]),
    "source_behind_the_original": (240, [(1280, 700, [(0, 0, 2), (3, 3, 2)])]),  # 3 * 256 >= 700: the second KEEP is dropped
}


def splice_inputs(name):
    cf, items = SPLICE_CASES[name]
    rng = np.random.default_rng(len(name))
    gs, as_ = [], []
    for L, n, _ in items:
        g, a = rng.standard_normal(L).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        if name == "signed_zeros_only":
            g, a = np.copysign(np.float32(0), g), np.copysign(np.float32(0), a)
        g[::7] = -0.0
        a[::5] = -0.0
        gs.append(g)
        as_.append(a)
    return cf, items, gs, as_


def run_splice(name, W, shift):
    """f5_wave_splice with rows of W samples, the output `shift` elements into a Guarded buffer -> (out rows on the host, wants)."""
    cf, items, gs, as_ = splice_inputs(name)
    B = len(items)
    gen = torch.full((B, W + 3), float("nan"))
    for b, g in enumerate(gs):
        gen[b, :len(g)] = torch.from_numpy(g)
    parts, starts, off = [], [], 0
    for b, a in enumerate(as_):
        gap = (3, 1, 6)[b % 3]
        parts += [torch.full((gap,), float("nan")), torch.from_numpy(a)]
        starts.append(off + gap)
        off += gap + len(a)
    parts.append(torch.full((5,), float("nan")))
    gen, flat = gen.to(DEV), torch.cat(parts).to(DEV)
    out = Guarded((shift + B * W,), torch.float32)
    counts = [len(it[2]) for it in items]
    segs = [v for it in items for s in it[2] for v in s]
    rc = _lib.load().f5_wave_splice(C.c_void_p(gen.data_ptr()), B, gen.stride(0), _lib.int_array([it[0] for it in items]),
                                    C.c_void_p(flat.data_ptr()), (C.c_int64 * B)(*starts), _lib.int_array([it[1] for it in items]),
                                    _lib.int_array(counts), _lib.int_array(segs), HOP, cf, C.c_void_p(out.ptr() + 4 * shift), W, _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().f5_last_error().decode()
    assert out.guards_intact() and (out.bits[:shift] == out.sent).all(), f"{name}: something outside the output rows was written"
    wants = [O.splice_fold(g, a, it[2], HOP, cf, width=W) for g, a, it in zip(gs, as_, items)]
    return out.value[shift:].view(B, W).cpu(), wants, (gen, flat, starts)


@pytest.mark.parametrize("name", list(SPLICE_CASES))
def test_splice_equals_the_per_sample_fold_bit_for_bit(name):
    cf, items, gs, as_ = splice_inputs(name)
    Lmax = max(it[0] for it in items)
    unaligned = name == "odd_length_unaligned_row"
    W, shift = (Lmax, 1) if unaligned else (Lmax + 9, 0)            # 1023-sample rows one element off a 16-byte boundary
    got, wants, (gen, flat, starts) = run_splice(name, W, shift)
    assert torch.isfinite(got).all(), f"{name}: something outside [0, L) of g or [0, n) of a was read"
    for b, want in enumerate(wants):
        L = items[b][0]
        same_bits(got[b], torch.from_numpy(want), f"{name} item {b}")
        assert (bits(got[b, L:]) == 0).all(), f"{name} item {b}: the samples behind L are not +0.0"
    if name == "original_shorter_than_its_frames":
        same_bits(got[0, 1081:1280], torch.from_numpy(gs[0][1081:]), "the tail behind the original")
    if name == "source_behind_the_original":
        same_bits(got[0, 512:1280], torch.from_numpy(gs[0][512:]), "a KEEP whose source lies behind the original")
    # the Python wrapper, with the EDIT segments of a whole plan in the table: the same bits
    plans = []
    for L, n, keeps in items:
        segs, at = [], 0
        for dst, src, frames in keeps:
            if dst > at:
                segs.append((at, -1, dst - at))
            segs.append((dst, src, frames))
            at = dst + frames
        plans.append((segs, at))
    wav = gen[:, :W]                                                 # rows W + 3 apart: a strided view
    originals = [flat[s:s + it[1]] for s, it in zip(starts, items)]
    py = I.wave_splice(wav, [it[0] for it in items], originals, plans, cf)
    assert py.shape == wav.shape
    same_bits(py, got, f"{name}: infer.wave_splice")


# ------------------------------------------------------------------------------------------------ driver
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
SKW = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
TARGET_RMS = 0.1
# (samples at 24 kHz, amplitude, target text, parts to edit, fix_duration): 32, 20 and 43 frames; rms below and above target_rms
RECORDINGS = [(8000, 0.05, "I am the wind.", [(0.1, 0.2)], None),
              (5000, 0.3, "Yes, indeed.", [(0.05, 0.1)], [0.12]),
              (11000, 0.05, "Some call me nature, others not.", [(0.1, 0.15), (0.3, 0.4)], [0.1, 0.05])]


def tiny_model(attn_mask):
    def make():
        arch = dict(P.config.F5TTS_TINY, attn_mask_enabled=attn_mask)
        tr = P.DiT(**arch, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
        return P.CFM(transformer=tr).to(DEV)                               # no vocab map: utf-8 byte tokens
    return cached(("model", attn_mask), make)


def tiny_vocoder():
    return cached("voc", lambda: P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV))


def tiny_bigvgan():
    def make():
        cfg = P.config.BIGVGAN_TINY
        voc = P.BigVGAN(cfg, precision="f32")
        voc.load_state_dict(P.weights.synthetic_state_dict(P.weights.bigvgan_param_shapes(cfg), seed=3))
        return voc.to(DEV)
    return cached("bigvgan", make)


def item(k, sr=SR, channels=1):
    n, amp, text, parts, fix = RECORDINGS[k]
    audio = cached(("audio", k, channels), lambda: torch.randn(channels, n, generator=torch.Generator().manual_seed(40 + k)) * amp)
    return (audio, sr, text, parts, fix)


def composed(model, voc, a, rms, text, parts, fix):
    """One recording from existing public pieces: a f32 [1, nw] prepared audio on the device -> (mel [1, N, 100], pre-rescale
    wave, rescaled wave, original mel [1, T, 100], mask)."""
    orig = model.mel_spec(a).permute(0, 2, 1)
    cond, mask = O.cat_construction(orig, parts, fix)
    mel, _ = model.sample(cond, [text], cond.shape[1], edit_mask=mask, **SKW)
    raw = voc.decode(mel.permute(0, 2, 1))[0]
    return mel, raw, I.rescale_to_prompt(raw, rms, TARGET_RMS), orig, mask


def test_one_recording_equals_the_composition_of_existing_parts():
    model, voc = tiny_model(False), tiny_vocoder()
    for k in (0, 1):                                                        # rms below target_rms (rescaled) and above
        audio, sr, text, parts, fix = item(k)
        a, rms = I.normalise_prompt(audio, sr, TARGET_RMS)
        assert (rms < TARGET_RMS) == (k == 0)
        want_mel, _, want_wave, orig, _ = composed(model, voc, a.to(DEV), rms, text, parts, fix)
        waves, rate, mels = I.speech_edit(model, voc, [item(k)], **KW)
        assert rate == SR and len(waves) == len(mels) == 1 and waves[0].dim() == 1 and waves[0].device.type == "cuda"
        D = len(O.frame_map(orig.shape[1], parts, fix))
        assert mels[0].shape == (NM, D + 1) == (NM, want_mel.shape[1])      # one generated frame behind the recording
        same_bits(mels[0], want_mel[0].permute(1, 0), f"recording {k}: mel")
        same_bits(waves[0], want_wave, f"recording {k}: waveform")
        assert torch.isfinite(waves[0]).all() and waves[0].shape == (D * HOP,)
        for d, src in enumerate(O.frame_map(orig.shape[1], parts, fix)):    # KEEP frames are the original's frames
            if src >= 0:
                assert torch.equal(bits(mels[0][:, d]), bits(orig[0, src])), f"recording {k}: frame {d} is not original frame {src}"


def alone(model, voc, ks, **kw):
    return [I.speech_edit(model, voc, [item(k)], **KW, **kw) for k in ks]


def check_items_equal_alone(model, voc, batch_frames, what):
    waves, _, mels = I.speech_edit(model, voc, [item(k) for k in range(3)], batch_frames=batch_frames, **KW)
    singles = cached(("alone", what.split(":")[0]), lambda: alone(model, voc, range(3)))
    assert len({m.shape[1] for m in mels}) == 3                             # unequal lengths
    for k in range(3):
        same_bits(mels[k], singles[k][2][0], f"{what}: item {k} mel against the item alone")
        same_bits(waves[k], singles[k][0][0], f"{what}: item {k} waveform against the item alone")


def ends_of_the_batch(model):
    frames = [RECORDINGS[k][0] // HOP + 1 for k in range(3)]
    D = [len(O.frame_map(frames[k], RECORDINGS[k][3], RECORDINGS[k][4])) for k in range(3)]
    return [max(len(RECORDINGS[k][2].encode()), D[k]) + 1 for k in range(3)]


def test_three_recordings_each_equal_the_recording_alone_where_attention_is_masked():
    """attn_mask_enabled=True: the batch runs valid rows only, so every item is computed as if alone -- bit equality, the
    criterion of test_long_form_gpu.py::test_chunks_are_independent_where_attention_is_masked."""
    check_items_equal_alone(tiny_model(True), tiny_vocoder(), None, "vocos: one group")


def two_group_budget(model):
    ends = ends_of_the_batch(model)
    budget = 2 * max(ends[:2])
    assert [list(r) for r in I.group_chunks(ends, budget)] == [[0, 1], [2]], (ends, budget)
    return budget


def test_two_groups_equal_one_group_per_item():
    model = tiny_model(True)
    check_items_equal_alone(model, tiny_vocoder(), two_group_budget(model), "vocos: two groups")


def test_two_groups_through_the_ragged_bigvgan():
    model = tiny_model(True)
    check_items_equal_alone(model, tiny_bigvgan().ragged(), two_group_budget(model), "bigvgan: two groups")


def test_splice_in_the_driver():
    model, voc = tiny_model(False), tiny_vocoder()
    k, cf = 2, 240                                                          # two parts, rms below target_rms: the rescale runs
    audio, sr, text, parts, fix = item(k)
    a, rms = I.normalise_prompt(audio, sr, TARGET_RMS)
    assert rms < TARGET_RMS
    _, raw, _, orig, _ = composed(model, voc, a.to(DEV), rms, text, parts, fix)
    fm = O.frame_map(orig.shape[1], parts, fix)
    keeps, d = [], 0                                                        # runs of consecutive source frames
    while d < len(fm):
        e = d + 1
        while e < len(fm) and fm[d] >= 0 and fm[e] == fm[e - 1] + 1:
            e += 1
        if fm[d] >= 0:
            keeps.append((d, fm[d], e - d))
        d = e
    assert len(keeps) == 3
    plain, _, mels0 = I.speech_edit(model, voc, [item(k)], **KW)
    waves, _, mels = I.speech_edit(model, voc, [item(k)], splice=True, **KW)                # splice_cross_fade = 0.01 s = 240
    same_bits(mels[0], mels0[0], "the splice does not touch the mel")
    fold = O.splice_fold(raw.cpu().numpy(), a[0].numpy(), keeps, HOP, cf)
    want = I.rescale_to_prompt(torch.from_numpy(fold).to(DEV), rms, TARGET_RMS)
    same_bits(waves[0], want, "spliced waveform")
    assert not torch.equal(waves[0], plain[0])
    level = I.rescale_to_prompt(a[0].to(DEV), rms, TARGET_RMS)
    L, n, inner = raw.shape[0], a.shape[1], 0
    for dst, src, frames in keeps:
        p0, p1 = dst * HOP, min((dst + frames) * HOP, L, dst * HOP + n - src * HOP)
        lo, hi = p0 + cf, p1 - cf
        assert hi > lo, "a KEEP range shorter than two fades: choose other spans"
        same_bits(waves[0][lo:hi], level[src * HOP + cf: src * HOP + cf + hi - lo], f"KEEP range [{p0}, {p1}): its inner samples")
        inner += hi - lo
    assert inner > 0.4 * L


def test_prompt_on_device_equals_the_composition_from_the_prepared_audio():
    model, voc = tiny_model(False), tiny_vocoder()
    n, amp, text, parts, fix = RECORDINGS[0]
    audio = torch.randn(2, 5334, generator=torch.Generator().manual_seed(9)) * amp     # 16 kHz stereo: 8001 samples at 24 kHz
    wavs, rms = model.mel_spec.prepare_ragged([audio], [16000], TARGET_RMS, device=DEV)
    assert wavs[0].shape == (8001,) and float(rms[0]) < TARGET_RMS
    want_mel, raw, want_wave, _, _ = composed(model, voc, wavs[0][None], rms[0], text, parts, fix)
    for splice in (False, True):
        waves, rate, mels = I.speech_edit(model, voc, [(audio, 16000, text, parts, fix)], prompt_on_device=True, splice=splice, **KW)
        same_bits(mels[0], want_mel[0].permute(1, 0), "prompt on device: mel")
        if not splice:
            same_bits(waves[0], want_wave, "prompt on device: waveform")
        else:
            plan = I.edit_plan(8001 // HOP + 1, parts, fix)
            fold = O.splice_fold(raw.cpu().numpy(), wavs[0].cpu().numpy(), O.keeps_of(plan), HOP, 240)
            same_bits(waves[0], I.rescale_to_prompt(torch.from_numpy(fold).to(DEV), rms[0], TARGET_RMS), "prompt on device: spliced")


def test_refusals():
    model = tiny_model(False)
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        I.speech_edit(model, P.BigVGAN(P.config.BIGVGAN_TINY), [item(0)], **KW)

    class Kor:
        _tokenizer_type = "kor_jamo"
        vocab_char_map = None
    with pytest.raises(NotImplementedError, match="text_tokenizer"):
        I.speech_edit(Kor(), tiny_vocoder(), [item(0)], **KW)
    with pytest.raises(ValueError):
        I.speech_edit(model, tiny_vocoder(), [], **KW)
    with pytest.raises(ValueError, match="time order"):
        I.speech_edit(model, tiny_vocoder(), [item(0)[:3] + ([(0.2, 0.1)], None)], **KW)
