"""GPU: the ragged BigVGAN pass (f5_bigvgan_forward_ragged, BigVGAN.forward_ragged, BigVGAN.ragged() in the batch drivers) -- a
batch of windows of unequal length through the generator in one pass over a packed time axis.  The yardstick is the per-item path
it replaces: every item must be BIT-identical to f5_bigvgan_forward on its own slice with B = 1, in both precisions, for item ends
inside the activation kernel's 8-step tiles, the narrow kernel's 128-row tiles and the 64- / 128-row GEMM tiles, across a tile
round, and for one-frame items shorter than the convolutions' reach and the 12-tap filters.  Every mel frame outside an item's
window is NaN, so a read of a prompt frame, of a frame past the end or of a neighbour shows up in the output.  Outputs go to
gpu_util.Guarded buffers: guards intact, every element written, the tail behind each waveform exactly +0.0."""
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
from oracle import bigvgan_oracle as BO  # noqa: E402

F5_EINVAL, F5_ESTATE = -1, -3
TAIL = 37          # samples of wav_stride past the longest waveform: every item has a tail to zero
ORACLE_TOL = {"f32": 1.5e-6, "f16x3": 3e-6}     # x max(1, peak): the bound of tests/test_bigvgan.py::test_bigvgan_hip_vs_oracle
CFGS = {"BIGVGAN_TINY": P.config.BIGVGAN_TINY, "BIGVGAN_MID": dict(P.config.BIGVGAN_V2_24K, upsample_initial_channel=256),
        "BIGVGAN_V2_24K": P.config.BIGVGAN_V2_24K}
# (config, frames per item).  TINY (4, 2): rows per frame 4 and 8; MID / V2_24K: 4 .. 256.
#  (1, 2, 37, 5): one- and two-frame items (4 / 8 rows: less than the 25-row reach, less than a 12-tap filter), ends inside 8-step
#                 activation tiles (37 * 4 = 148 = 18.5 tiles) and inside the first 64- / 128-row tile;
#  (33, 1, 130, 64): 264 packed frames = 1,056 / 2,112 rows: several 128-row tiles, ends off every tile multiple, a one-frame item
#                 between two long ones; (24, 3) and (8, 3): every stage of the six-stage generators, wide and narrow kernels.
CASES = [("BIGVGAN_TINY", (1, 2, 37, 5)), ("BIGVGAN_TINY", (33, 1, 130, 64)), ("BIGVGAN_MID", (24, 3)), ("BIGVGAN_V2_24K", (8, 3))]
STARTS = (3, 0, 5, 2)
IDS = [f"{n}-{'_'.join(map(str, f))}" for n, f in CASES]

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def weights(cfg_name, seed=3):
    return cached(("V", cfg_name, seed), lambda: P.weights.synthetic_state_dict(P.weights.bigvgan_param_shapes(CFGS[cfg_name]), seed=seed))


def vocoder(cfg_name, prec, fresh=False):
    def make():
        voc = P.BigVGAN(CFGS[cfg_name], precision=prec)
        voc.load_state_dict(weights(cfg_name))
        return voc.to(DEV)
    return make() if fresh else cached(("voc", cfg_name, prec), make)


def batch(frames, layout="bct"):
    """(mel view [B, 100, T] on the device, starts, ends): NaN in every frame outside the windows.  layout "btc": sample()'s
    [B, T, C] output permuted, as the drivers pass it."""
    def make():
        B = len(frames)
        starts = list(STARTS[:B])
        ends = [s + f for s, f in zip(starts, frames)]
        T = max(ends) + 4
        g = torch.Generator().manual_seed(sum(frames))
        mel = torch.full((B, 100, T), float("nan"))
        for b in range(B):
            mel[b, :, starts[b]:ends[b]] = torch.randn(100, frames[b], generator=g)
        return mel, starts, ends
    mel, starts, ends = cached(("mel", frames), make)
    dev = cached(("mel_dev", frames, layout), lambda: mel.to(DEV) if layout == "bct" else mel.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1))
    return dev, starts, ends


def alone(cfg_name, prec, frames):
    """The reference, computed once and left unchanged: forward() of every item's slice alone, [L_b] each."""
    def make():
        voc = vocoder(cfg_name, prec)
        mel, starts, ends = batch(frames)
        return [voc(mel[b:b + 1, :, s:e])[0, 0].clone() for b, (s, e) in enumerate(zip(starts, ends))]
    return cached(("alone", cfg_name, prec, frames), make)


def ragged_call(voc, mel, starts, ends, gain=None, stride=None):
    """f5_bigvgan_forward_ragged into a Guarded [B, stride] buffer; returns (code, buffer)."""
    B = mel.shape[0]
    stride = max(e - s for s, e in zip(starts, ends)) * voc.total_up + TAIL if stride is None else stride
    out = Guarded((B, stride), torch.float32)
    sb, sc, st = mel.stride()
    rc = _lib.load().f5_bigvgan_forward_ragged(voc._handle(), _ptr(mel), B, sb, sc, st, _lib.int_array(starts), _lib.int_array(ends),
                                               None if gain is None else _lib.float_array(gain), C.c_void_p(out.ptr()), stride, _stream())
    torch.cuda.synchronize()
    return rc, out


def check_items(out, want, what):
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    for b, w in enumerate(want):
        n = w.shape[0]
        assert torch.isfinite(out.value[b, :n]).all(), f"{what}: item {b}: a frame outside the window was read, or a sample was not written"
        got = out.bits[b, :n]
        assert torch.equal(got, w.view(torch.int32)), f"{what}: item {b}: {int((got != w.view(torch.int32)).sum())} of {n} samples differ"
        assert (out.bits[b, n:] == 0).all(), f"{what}: item {b}: the tail is not +0.0"


@pytest.mark.parametrize("layout", ["bct", "btc"])
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("cfg_name,frames", CASES, ids=IDS)
def test_items_bit_equal_forward_alone(cfg_name, frames, prec, layout):
    voc = vocoder(cfg_name, prec)
    want = alone(cfg_name, prec, frames)
    mel, starts, ends = batch(frames, layout)
    rc, out = ragged_call(voc, mel, starts, ends)
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_items(out, want, f"{cfg_name} {frames} {prec} {layout}")
    # the Python surface: the same bits in a [B, L_max] tensor
    wav, lens = voc.forward_ragged(mel, ends, starts=starts)
    assert lens == [f * voc.total_up for f in frames] and wav.shape == (len(frames), max(lens))
    assert torch.equal(wav.view(torch.int32), out.bits[:, :max(lens)])
    view_wav, view_lens = voc.ragged().decode_ragged(mel, ends, starts=starts)
    assert view_lens == lens and torch.equal(view_wav.view(torch.int32), wav.view(torch.int32))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_one_item_and_no_starts(prec):
    """B = 1 is the rectangular call; starts = NULL reads every row from frame 0."""
    voc = vocoder("BIGVGAN_TINY", prec)
    mel = torch.randn(2, 100, 21, generator=torch.Generator().manual_seed(9)).to(DEV)
    mel[1, :, 6:] = float("nan")
    want = [voc(mel[0:1])[0, 0].clone(), voc(mel[1:2, :, :6])[0, 0].clone()]
    wav, lens = voc.forward_ragged(mel, [21, 6])
    assert lens == [168, 48]
    assert torch.equal(wav[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(wav[1, :48].view(torch.int32), want[1].view(torch.int32)) and (wav[1, 48:].view(torch.int32) == 0).all()
    one, _ = voc.forward_ragged(mel[0:1], [21])
    assert torch.equal(one[0].view(torch.int32), want[0].view(torch.int32))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_gains_are_a_separate_multiply(prec):
    cfg_name, frames = CASES[0]
    voc = vocoder(cfg_name, prec)
    gain = [0.37, 1.0, 2.5, 0.0625]
    want = [w * g for w, g in zip(alone(cfg_name, prec, frames), gain)]
    mel, starts, ends = batch(frames)
    rc, out = ragged_call(voc, mel, starts, ends, gain=gain)
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_items(out, want, f"gains {prec}")


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_workspace_reuse_leaves_no_stale_gap_rows(prec):
    """ragged, another ragged layout, a rectangular forward, the first layout again -- on ONE handle, whose arena then holds the
    earlier calls' rows (and NaN is easy to come by: the rectangular call below decodes a NaN mel first)."""
    voc = vocoder("BIGVGAN_TINY", prec, fresh=True)
    (_, fa), (_, fb) = CASES[0], CASES[1]
    mel_a, sa, ea = batch(fa)
    mel_b, sb_, eb = batch(fb)
    first, _ = voc.forward_ragged(mel_a, ea, starts=sa)
    other, _ = voc.forward_ragged(mel_b, eb, starts=sb_)
    rect_mel = torch.randn(2, 100, 37, generator=torch.Generator().manual_seed(2)).to(DEV)
    voc(torch.full((1, 100, 150), float("nan"), device=DEV))     # fills the arena with NaN
    rect = voc(rect_mel)
    again, _ = voc.forward_ragged(mel_a, ea, starts=sa)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    assert torch.isfinite(again).all()
    assert torch.equal(rect.view(torch.int32), vocoder("BIGVGAN_TINY", prec, fresh=True)(rect_mel).view(torch.int32))
    for b, w in enumerate(alone("BIGVGAN_TINY", prec, fb)):
        assert torch.equal(other[b, :w.shape[0]].view(torch.int32), w.view(torch.int32))


def test_max_frames_groups_give_the_same_bits():
    cfg_name, frames = CASES[1]
    voc = vocoder(cfg_name, "f32")
    mel, starts, ends = batch(frames)
    one, lens = voc.forward_ragged(mel, ends, starts=starts)
    assert len(voc._ragged_groups(list(frames), 100)) > 1
    for max_frames in (100, 1):
        grouped, glens = voc.forward_ragged(mel, ends, starts=starts, max_frames=max_frames)
        assert glens == lens and torch.equal(grouped.view(torch.int32), one.view(torch.int32)), f"max_frames = {max_frames}"


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("cfg_name,frames", CASES, ids=IDS)
def test_items_against_the_float64_restatement(cfg_name, frames, prec):
    voc = vocoder(cfg_name, prec)
    mel, starts, ends = batch(frames)
    wav, lens = voc.forward_ragged(mel, ends, starts=starts)
    cpu = cached(("mel", frames), None)[0]
    for b, (s, e) in enumerate(zip(starts, ends)):
        ref = cached(("oracle", cfg_name, frames, b),
                     lambda: BO.bigvgan_forward(weights(cfg_name), CFGS[cfg_name], cpu[b:b + 1, :, s:e].double(), dtype=torch.float64))[0, 0]
        err = (wav[b, :lens[b]].cpu().double() - ref).abs().max().item()
        print(f"[bigvgan ragged {prec}] {cfg_name} item {b} ({frames[b]} frames): Linf {err:.3e} vs float64 (peak {ref.abs().max().item():.3f})")
        assert err < ORACLE_TOL[prec] * max(1.0, ref.abs().max().item())


def test_implicit_conv_equals_materialised_operand_on_the_packed_axis(monkeypatch):
    """The relation test_bigvgan_implicit_conv_equals_materialised_operand asserts for the rectangular call: with the GEMM path in
    every stage, implicit and im2col convolutions give the same bits -- here over the packed axis (im2col reads the zero gap rows)."""
    cfg_name, frames = CASES[2]
    voc = vocoder(cfg_name, "f32")
    mel, starts, ends = batch(frames)
    monkeypatch.setenv("F5_BIGVGAN_NARROW", "0")
    w_imp, lens = voc.forward_ragged(mel, ends, starts=starts)
    w_imp = w_imp.clone()
    alone_imp = [voc(mel[b:b + 1, :, s:e])[0, 0].clone() for b, (s, e) in enumerate(zip(starts, ends))]
    monkeypatch.setenv("F5_BIGVGAN_IMPLICIT", "0")
    w_mat, _ = voc.forward_ragged(mel, ends, starts=starts)
    assert torch.isfinite(w_mat).all() and torch.equal(w_imp.view(torch.int32), w_mat.view(torch.int32))
    for b, w in enumerate(alone_imp):
        assert torch.equal(w_mat[b, :lens[b]].view(torch.int32), w.view(torch.int32)), f"item {b} differs from forward() alone"


def test_refusals_launch_nothing():
    lib = _lib.load()
    voc = vocoder("BIGVGAN_TINY", "f32")
    h = voc._handle()
    mel = torch.randn(2, 100, 12, generator=torch.Generator().manual_seed(1)).to(DEV)
    sb, sc, st = mel.stride()
    out = Guarded((2, 96 + TAIL), torch.float32)

    def call(handle=h, melp=_ptr(mel), B=2, starts=(0, 2), ends=(12, 9), wavp=C.c_void_p(out.ptr()), stride=96 + TAIL):
        rc = lib.f5_bigvgan_forward_ragged(handle, melp, B, sb, sc, st, _lib.int_array(starts), None if ends is None else _lib.int_array(ends),
                                           None, wavp, stride, _stream())
        return rc, lib.f5_last_error().decode()

    for kw, word in ((dict(starts=(0, 9), ends=(12, 9)), "item 1"), (dict(starts=(0, 9), ends=(12, 5)), "item 1"),   # T_b = 0, < 0
                     (dict(starts=(-1, 2)), "item 0"), (dict(stride=95), "wav_stride"), (dict(B=0), "B = 0"), (dict(B=-3), "B = -3"),
                     (dict(B=65536), "B = 65536"), (dict(melp=None), "null"), (dict(ends=None), "null"), (dict(wavp=None), "null"),
                     (dict(handle=None), "null"),
                     # 2^24 rows at the last stage = 2,097,152 frames of this 8x generator
                     (dict(starts=(0, 0), ends=(1_500_000, 1_000_000), stride=12_000_000), "2^24")):
        rc, msg = call(**kw)
        assert rc == F5_EINVAL and word in msg and "f5_bigvgan" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (out.bits == out.sent).all() and out.guards_intact(), "a refused call wrote to wav"
    # before finalize
    raw = C.c_void_p()
    assert lib.f5_bigvgan_create(C.byref(voc._config()), C.byref(raw)) == 0
    try:
        rc, msg = call(handle=raw)
        assert rc == F5_ESTATE and "finalize" in msg
    finally:
        lib.f5_bigvgan_destroy(raw)
    assert (out.bits == out.sent).all()
    rc, _ = call()
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(out.value[0, :96]).all()
    with pytest.raises(ValueError, match="item 1"):
        voc.forward_ragged(mel, [12, 13])


# ------------------------------------------------------------------------------------------------ the drivers
SR = 24000
REF_TEXT = "hello there."
CHUNKS = ["General Kenobi, you are a bold one.", "Yes."]
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)


def tiny_model(attn_mask):
    def make():
        arch = dict(P.config.F5TTS_TINY, attn_mask_enabled=attn_mask)
        tr = P.DiT(**arch, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
        return P.CFM(transformer=tr, mel_spec_kwargs=dict(mel_spec_type="bigvgan")).to(DEV)      # center=False: nw // 256 frames
    return cached(("model", attn_mask), make)


def driver_vocoder():
    """All six stages at 256 -> 4 channels: the shipped 256x upsampling at a width a test can afford."""
    return cached("driver_voc", lambda: P.BigVGAN(CFGS["BIGVGAN_MID"]).init_synthetic(seed=4).to(DEV))


def prompt():
    return cached("prompt", lambda: torch.randn(1, 7200, generator=torch.Generator().manual_seed(5)) * 0.05)


def test_synthesize_batch_equals_sample_and_per_item_forward():
    model, bv = tiny_model(False), driver_vocoder()
    g = torch.Generator().manual_seed(6)
    audio = [torch.randn(1, 7200, generator=g) * 0.1, torch.randn(1, 5000, generator=g) * 0.1]
    mels = [model.mel_spec(a.to(DEV)).permute(0, 2, 1)[0] for a in audio]
    lens = [m.shape[0] for m in mels]
    assert lens == [7200 // 256, 5000 // 256]
    cond = torch.zeros(2, max(lens), 100, device=DEV)
    for i, m in enumerate(mels):
        cond[i, :lens[i]] = m
    texts, durs = ["I am the wind.", "Yes, indeed it is so."], torch.tensor([45, 52])
    skw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    wav, wav_lens, mel = I.synthesize_batch(model, bv.ragged(), cond, texts, durs, lens=lens, gain=[0.5, 1.0], **skw)
    out, _ = model.sample(cond, texts, durs, lens=torch.tensor(lens), **skw)
    assert torch.equal(mel, out)
    ends = clamp_durations(P.utils.list_str_to_tensor(texts), torch.tensor(lens), durs).tolist()
    assert wav_lens == [(e - l) * 256 for e, l in zip(ends, lens)] and wav.shape == (2, max(wav_lens))
    for b, gain in enumerate((0.5, 1.0)):
        want = bv(out[b:b + 1, lens[b]:ends[b]].to(torch.float32).permute(0, 2, 1))[0, 0] * gain
        assert torch.equal(wav[b, :wav_lens[b]].view(torch.int32), want.view(torch.int32)), f"item {b}"
        assert (wav[b, wav_lens[b]:].view(torch.int32) == 0).all()


def test_infer_process_batched_through_the_view():
    model, bv = tiny_model(False), driver_vocoder()
    wave, sr, spec = I.infer_process((prompt(), SR), REF_TEXT, " ".join(CHUNKS), model, bv.ragged(), mel_spec_type="bigvgan",
                                     show_info=None, batched=True, **KW)
    assert wave.dtype == np.float32 and wave.ndim == 1 and sr == SR and spec.shape[0] == 100 and np.isfinite(wave).all()
    assert wave.shape[0] == spec.shape[1] * 256        # one chunk at this prompt's bytes-per-second: no cross-fade; no (T - 1) here


def test_batched_chunks_equal_the_sequential_path_where_attention_is_masked():
    model, bv = tiny_model(True), driver_vocoder()
    seq_wave, _, seq_spec = next(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, bv, mel_spec_type="bigvgan", **KW))
    wave, _, spec = next(I.infer_batch_process((prompt(), SR), REF_TEXT, CHUNKS, model, bv.ragged(), mel_spec_type="bigvgan",
                                               batched=True, **KW))
    assert np.array_equal(spec.view(np.int32), seq_spec.view(np.int32))
    want = seq_wave.astype(np.float32)
    assert wave.dtype == np.float32 and wave.shape == want.shape and np.array_equal(wave.view(np.int32), want.view(np.int32))


def test_synthesize_prompts_items_equal_the_single_item_results():
    model, bv = tiny_model(True), driver_vocoder()
    g = torch.Generator().manual_seed(7)
    prompts = [(torch.randn(1, 7200, generator=g) * 0.05, SR, "Some call me nature."),
               (torch.randn(1, 5555, generator=g) * 0.3, SR, "Good morning")]
    texts = ["I am the wind.", "Yes, indeed."]
    waves, sr, specs = I.synthesize_prompts(model, bv.ragged(), prompts, texts, **KW)
    assert sr == SR and len(waves) == len(specs) == 2
    for i in range(2):
        (w1,), _, (s1,) = I.synthesize_prompts(model, bv.ragged(), prompts[i:i + 1], texts[i:i + 1], **KW)
        assert waves[i].dim() == 1 and waves[i].shape[0] == specs[i].shape[1] * bv.total_up and torch.isfinite(waves[i]).all()
        assert torch.equal(specs[i].view(torch.int32), s1.view(torch.int32)), f"item {i}: generated mel differs"
        assert torch.equal(waves[i].view(torch.int32), w1.view(torch.int32)), f"item {i}: waveform differs"
