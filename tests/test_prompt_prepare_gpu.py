"""GPU: the prompt preparation stage (f5_mel_prepare_ragged, MelSpec.prepare_ragged, the `prompt_on_device` route of the infer
drivers) -- mono mix, RMS, level and resample for a ragged batch in one pass.  Three yardsticks, all computed on the host:
  contract order   a restatement of include/f5_hip.h's contract in torch f32 operations (mono, the two-operation gain, then
                   acc = acc + bank[:, k] * x[i * orig + k] for ascending k), given the device's own rms: BIT-equal per item;
  rms              sqrt(mean(mono.double() ** 2)).float(), or the f32 value next to it;
  error bound      the same pipeline in float64 with the f32 bank: every output sample within (K + 1) * 2^-24 * sum_k |bank[p][k] *
                   v[i * orig + k]|, K = 2 width + orig taps -- the forward error bound of an f32 recursive sum, computed per
                   sample in float64 (the f32 mono mix and gain add at most three more roundings per sample; measured on the
                   host, both the contract order and sinc_resample's conv1d stay within 0.3 x the bound, so there is room).
The items of the C-level calls are views into one flat buffer with NaN in front of, between and behind them, the packed output
is over-allocated and NaN-prefilled: a read outside an item shows in the result, a write outside an item's planned range in the
NaN that is gone."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from f5_tts_amd import mel as M  # noqa: E402

TARGET, TARGET_RMS, HOP = 24000, 0.1, 256
# (rate, n, channels, amplitude): rms well below target_rms (x 0.02) or well above (x 0.5)
ITEMS = [(48000, 1, 1, 0.02), (48000, 5003, 2, 0.5), (44100, 146, 1, 0.02), (44100, 148, 2, 0.5), (22050, 5003, 3, 0.02),
         (16000, 7, 1, 0.5), (8000, 2048, 2, 0.02), (24000, 1001, 2, 0.02)]
# the other code paths of the resample kernel: 32000 and 11025 Hz (new = 320: fewer than four frames per block); 192 kHz; a
# window that only fits the LDS a few frames at a time (6 MHz: orig 250, K 3282, 20 frames per block, two blocks); one that does
# not fit at all and is read from global memory (24 MHz: orig 1000, K 13122); and 24 kHz above target_rms: a plain copy
ODD_ITEMS = [(32000, 5003, 2, 0.02), (11025, 5003, 1, 0.5), (192000, 6000, 1, 0.02), (6_000_000, 6000, 1, 0.5),
             (24_000_000, 6000, 2, 0.02), (24000, 4099, 1, 0.5)]
GAPS = (17, 3, 10, 1, 6, 5)   # NaN elements in front of item 0, between the items, behind the last: items start off 16-byte multiples

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def audio(item):
    sr, n, ch, amp = item
    return cached(("audio", item), lambda: torch.randn(ch, n, generator=torch.Generator().manual_seed(sr + 7 * n + ch)) * amp)


def mono32(a):
    if a.shape[0] == 1:
        return a[0]
    s = a[0]
    for c in range(1, a.shape[0]):
        s = s + a[c]
    return s / float(a.shape[0])


def bank_of(sr):
    k, orig, new, width = M.resample_kernel(sr, TARGET)
    return k[:, 0].to(torch.float32), orig, new, width


def polyphase(v, sr, dtype):
    """y[i * new + p] = sum_k bank[p][k] * vpad[i * orig + k], k ascending from zero, in `dtype`; also sum_k |.| in that dtype."""
    bank, orig, new, width = bank_of(sr)
    bank = bank.to(dtype)
    n = v.shape[0]
    L = -(-new * n // orig)
    frames = -(-L // new)
    K = 2 * width + orig
    x = torch.zeros(width + frames * orig + K, dtype=dtype)
    x[width:width + n] = v.to(dtype)
    acc = torch.zeros(frames, new, dtype=dtype)
    mag = torch.zeros(frames, new, dtype=dtype)
    for k in range(K):
        term = bank[:, k][None, :] * x[k:k + frames * orig:orig][:, None]
        acc = acc + term
        mag = mag + term.abs()
    return acc.reshape(-1)[:L], mag.reshape(-1)[:L], K


def contract(a, sr, rms, dtype=torch.float32):
    """The contract on the host for one item [C, n], given its rms (a 0-dim f32 tensor): (y, sum of |terms|, taps)."""
    if dtype == torch.float32:
        v = mono32(a)
        if rms < TARGET_RMS:
            v = v * TARGET_RMS / rms
    else:
        v = a.double().mean(dim=0)
        if rms < TARGET_RMS:
            v = v * TARGET_RMS / rms.double()
    if sr == TARGET:
        return v, v.abs(), 0
    return polyphase(v, sr, dtype)


def check_item(what, item, got, rms):
    """got, rms: the device's item and rms on the host."""
    sr, n, ch, amp = item
    a = audio(item)
    assert got.shape == (M.resampled_length(n, sr, TARGET),), what
    assert torch.isfinite(got).all() and torch.isfinite(rms), f"{what}: something outside the item's samples was read"
    true = a.double().mean(dim=0).square().mean().sqrt()
    assert abs(float(true) / TARGET_RMS - 1) > 0.01, f"{what}: the item lies within 1 % of the threshold"
    want_rms = true.float()
    near = (want_rms, torch.nextafter(want_rms, torch.tensor(0.0)), torch.nextafter(want_rms, torch.tensor(1.0)))
    print(f"{what}: rms {float(rms):.9g} want {float(want_rms):.9g}")
    assert any(torch.equal(rms, w) for w in near), f"{what}: rms {float(rms):.9g} is not {float(want_rms):.9g} or its neighbour"
    y32, _, _ = contract(a, sr, rms)
    diff = int((got.view(torch.int32) != y32.view(torch.int32)).sum())
    y64, mag, K = contract(a, sr, rms, torch.float64)
    bound = (K + 1) * 2.0 ** -24 * mag
    err = (got.double() - y64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: {diff} of {got.numel()} samples differ from the contract order; worst error / bound = {worst:.4f} (K = {K})")
    assert diff == 0, f"{what}: {diff} of {got.numel()} samples differ from the contract order"
    if sr != TARGET:
        assert (err <= bound).all(), f"{what}: worst error / bound = {worst:.3f}"
    else:                                    # nothing is summed: the item is the levelled mono audio itself
        lev = mono32(a) * TARGET_RMS / rms if rms < TARGET_RMS else mono32(a)
        assert torch.equal(got.view(torch.int32), lev.view(torch.int32)), f"{what}: not the levelled mono audio"


def plan(items):
    B = len(items)
    lens, starts, total = (C.c_int64 * B)(), (C.c_int64 * B)(), C.c_int64()
    _lib.check(_lib.load().f5_mel_prepare_plan(B, _lib.int_array([i[1] for i in items]), _lib.int_array([i[0] for i in items]), TARGET, lens,
                                               starts, C.byref(total)), "f5_mel_prepare_plan")
    return list(lens), list(starts), total.value


def mel_spec():
    return cached("ms", lambda: P.mel.MelSpec())


def c_level_run(ms, items, slack=64):
    """f5_mel_prepare_ragged on items inside one NaN-separated buffer -> (out on the host with `slack` elements behind the plan's
    total, rms on the host, lens, starts, total)."""
    parts, in_starts, off = [], [], 0
    for i, it in enumerate(items):
        gap = GAPS[i % len(GAPS)]
        parts += [torch.full((gap,), float("nan")), audio(it).reshape(-1)]
        in_starts.append(off + gap)
        off += gap + it[1] * it[2]
    parts.append(torch.full((GAPS[len(items) % len(GAPS)],), float("nan")))
    flat = torch.cat(parts).to(DEV)
    lens, starts, total = plan(items)
    B = len(items)
    out = torch.full((total + slack,), float("nan"), device=DEV)
    rms = torch.full((B + 4,), float("nan"), device=DEV)
    h = ms._handle(torch.device(DEV))
    lib = _lib.load()
    ms._resample_banks(lib, h, torch.device(DEV), [it[0] for it in items])
    rc = lib.f5_mel_prepare_ragged(h, C.c_void_p(flat.data_ptr()), B, (C.c_int64 * B)(*in_starts), _lib.int_array([it[2] for it in items]),
                                   _lib.int_array([it[1] for it in items]), _lib.int_array([it[0] for it in items]), TARGET, TARGET_RMS,
                                   C.c_void_p(out.data_ptr()), total, C.c_void_p(rms.data_ptr()),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, lib.f5_last_error().decode()
    return out.cpu(), rms.cpu(), lens, starts, total


def check_c_level(what, ms, items):
    out, rms, lens, starts, total = c_level_run(ms, items)
    written = torch.zeros(out.numel(), dtype=torch.bool)
    for (ln, st) in zip(lens, starts):
        written[st:st + ln] = True
    assert torch.isnan(out[~written]).all(), f"{what}: something outside the planned item ranges was written"
    assert torch.isnan(out[total:]).all() and out.numel() - total == 64, f"{what}: the guard behind the plan's total was written"
    assert torch.isnan(rms[len(items):]).all(), f"{what}: rms_out was written past B"
    for b, it in enumerate(items):
        check_item(f"{what} item {b} {it}", it, out[starts[b]:starts[b] + lens[b]], rms[b])
    return out, rms, lens, starts


def batch_bits():
    """The eight items in one call (computed once): (out, rms, lens, starts) on the host."""
    return cached("batch", lambda: c_level_run(mel_spec(), ITEMS)[:4])


def test_items_contract_order_and_error_bound():
    ms = mel_spec()
    out, rms, lens, starts = check_c_level("forward order", ms, ITEMS)
    _CACHE.setdefault("batch", (out, rms, lens, starts))
    rout, rrms, rlens, rstarts = check_c_level("reverse order", ms, ITEMS[::-1])
    B = len(ITEMS)
    for b in range(B):                       # other offsets, other neighbours: the same bits
        r = B - 1 - b
        assert torch.equal(out[starts[b]:starts[b] + lens[b]].view(torch.int32), rout[rstarts[r]:rstarts[r] + rlens[r]].view(torch.int32))
        assert torch.equal(rms[b].view(torch.int32), rrms[r].view(torch.int32))


def test_the_other_kernel_paths():
    check_c_level("odd rates", mel_spec(), ODD_ITEMS)


def test_one_item_alone_equals_the_item_in_a_batch():
    ms = mel_spec()
    out, rms, lens, starts = batch_bits()
    for b, it in enumerate(ITEMS):
        wavs, r = ms.prepare_ragged([audio(it).to(DEV)], [it[0]], TARGET_RMS)
        assert torch.equal(wavs[0].cpu().view(torch.int32), out[starts[b]:starts[b] + lens[b]].view(torch.int32)), f"item {b} {it}"
        assert torch.equal(r.cpu().view(torch.int32), rms[b:b + 1].view(torch.int32)), f"item {b} {it}: rms"


def bank_count(ms):
    n = C.c_int32(-1)
    _lib.check(_lib.load().f5_mel_resample_bank_count(ms._handle(torch.device(DEV)), C.byref(n)), "f5_mel_resample_bank_count")
    return n.value


def test_reuse_of_workspace_and_banks():
    ms = P.mel.MelSpec()                     # a fresh handle: its workspace grows here and nowhere else
    want = batch_bits()[0]
    first = c_level_run(ms, ITEMS)[0]
    assert torch.equal(first.view(torch.int32), want.view(torch.int32))
    pairs = len({it[0] for it in ITEMS} - {TARGET})
    assert bank_count(ms) == pairs == 5
    again = c_level_run(ms, ITEMS)[0]
    assert torch.equal(again.view(torch.int32), first.view(torch.int32)) and bank_count(ms) == pairs
    larger = ITEMS + ODD_ITEMS[:2] + ITEMS[::-1]
    check_c_level("larger", ms, larger)
    assert bank_count(ms) == pairs + 2       # 32000 and 11025 Hz are new, nothing else is
    assert torch.equal(c_level_run(ms, ITEMS)[0].view(torch.int32), first.view(torch.int32))
    check_c_level("smaller", ms, ITEMS[2:4])
    assert torch.equal(c_level_run(ms, ITEMS)[0].view(torch.int32), first.view(torch.int32))
    assert bank_count(ms) == pairs + 2
    # the python layer asks for no bank it has handed over before
    ms.prepare_ragged([audio(it) for it in ITEMS], [it[0] for it in ITEMS], TARGET_RMS, device=DEV)
    assert bank_count(ms) == pairs + 2


def test_prepare_ragged_input_forms():
    ms = mel_spec()
    out, rms, lens, starts = batch_bits()
    host = [audio(it) for it in ITEMS]
    rates = [it[0] for it in ITEMS]
    wavs, r = ms.prepare_ragged(host, rates, TARGET_RMS, device=DEV)
    assert r.device.type == "cuda" and r.shape == (len(ITEMS),) and r.dtype == torch.float32
    assert torch.equal(r.cpu().view(torch.int32), rms[:len(ITEMS)].view(torch.int32))
    for b, w in enumerate(wavs):
        assert w.dim() == 1 and w.device.type == "cuda" and w.data_ptr() % 16 == 0
        assert w.data_ptr() - wavs[0].data_ptr() == 4 * starts[b]                                     # views into ONE packed buffer
        assert torch.equal(w.cpu().view(torch.int32), out[starts[b]:starts[b] + lens[b]].view(torch.int32)), f"item {b}"
    want = [w.cpu().view(torch.int32) for w in wavs]
    on_dev = [a.to(DEV) for a in host]
    wide = [torch.randn(a.shape[1], 2 * a.shape[0], generator=torch.Generator().manual_seed(3)) for a in host]
    for w, a in zip(wide, host):
        w[:, ::2] = a.t()
    forms = {
        "device tensors": on_dev,
        "host and device mixed": [a if i % 2 else d for i, (a, d) in enumerate(zip(host, on_dev))],
        "[n] for the mono items": [a[0] if a.shape[0] == 1 else a for a in host],
        "[n] on the device": [d[0] if d.shape[0] == 1 else d for d in on_dev],
        "non-contiguous host tensors": [w[:, ::2].t() for w in wide],
        "non-contiguous device tensors": [w.to(DEV)[:, ::2].t() for w in wide],
    }
    assert not any(f.is_contiguous() for f, a in zip(forms["non-contiguous host tensors"], host) if a.numel() > 1)
    for name, audios in forms.items():
        got, r2 = ms.prepare_ragged(audios, rates, TARGET_RMS, device=DEV)
        assert torch.equal(r2.view(torch.int32), r.view(torch.int32)), f"{name}: the input form changed the rms"
        for b in range(len(ITEMS)):
            assert torch.equal(got[b].cpu().view(torch.int32), want[b]), f"{name}: the input form changed item {b}"


# ---- composition with the mel front-end and the batch driver
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
GEN_TEXTS = ["I am the wind.", "반갑습니다.", "Yes, indeed."]


def tiny_model():
    def make():
        tr = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
        return P.CFM(transformer=tr).to(DEV)                               # no vocab map: utf-8 byte tokens
    return cached("model", make)


def tiny_vocoder():
    return cached("voc", lambda: P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV))


def test_forward_ragged_reads_the_prepared_waveforms_in_place():
    ms = mel_spec()
    items = [(44100, 5003, 2, 0.02), (48000, 5000, 1, 0.5), (24000, 3000, 2, 0.02)]       # 2723, 2500 and 3000 samples at 24 kHz
    wavs, _ = ms.prepare_ragged([audio(it) for it in items], [it[0] for it in items], TARGET_RMS, device=DEV)
    clones = [w.clone() for w in wavs]
    mel, frames = ms.forward_ragged(wavs)
    mel2, frames2 = ms.forward_ragged(clones)
    assert frames == frames2 == [w.shape[0] // HOP + 1 for w in wavs]
    assert torch.isfinite(mel).all() and torch.equal(mel.view(torch.int32), mel2.view(torch.int32))
    for w, c in zip(wavs, clones):
        assert torch.equal(w.view(torch.int32), c.view(torch.int32))                       # and they are still what they were


def test_synthesize_prompts_routes_agree_exactly_where_nothing_is_levelled_or_resampled():
    g = torch.Generator().manual_seed(11)
    prompts = [(torch.randn(1, 5200, generator=g) * 0.3, TARGET, "Some call me nature."),
               (torch.randn(1, 3900, generator=g) * 0.5, TARGET, "안녕하세요"),
               (torch.randn(1, 4444, generator=g) * 0.2, TARGET, "Good morning")]
    assert all(I.normalise_prompt(a, sr, TARGET_RMS)[1] > 1.5 * TARGET_RMS for a, sr, _ in prompts)
    model, voc = tiny_model(), tiny_vocoder()
    off = I.synthesize_prompts(model, voc, prompts, GEN_TEXTS, target_rms=TARGET_RMS, **KW)
    on = I.synthesize_prompts(model, voc, prompts, GEN_TEXTS, target_rms=TARGET_RMS, prompt_on_device=True, **KW)
    assert off[1] == on[1] == TARGET and len(on[0]) == len(on[2]) == 3
    for i in range(3):
        assert on[0][i].dim() == 1 and on[0][i].device.type == "cuda" and torch.isfinite(on[0][i]).all()
        assert on[0][i].shape == off[0][i].shape and on[2][i].shape == off[2][i].shape
        assert torch.equal(on[2][i].view(torch.int32), off[2][i].view(torch.int32)), f"item {i}: generated mel differs"
        assert torch.equal(on[0][i].view(torch.int32), off[0][i].view(torch.int32)), f"item {i}: waveform differs"


def test_synthesize_prompts_with_stereo_44k1_prompts():
    items = [(44100, 5003, 2, 0.02), (44100, 5999, 2, 0.5), (44100, 4100, 2, 0.02)]
    prompts = [(audio(it), it[0], t) for it, t in zip(items, ("Some call me nature.", "안녕하세요", "Good morning"))]
    model, voc = tiny_model(), tiny_vocoder()
    ms = model.mel_spec
    # the prepared audio against the host route's, under the bound of the first test
    wavs, rms = ms.prepare_ragged([p[0] for p in prompts], [p[1] for p in prompts], TARGET_RMS, device=DEV)
    for b, it in enumerate(items):
        check_item(f"stereo 44.1 kHz item {b}", it, wavs[b].cpu(), rms[b].cpu())
        host_audio, host_rms = I.normalise_prompt(audio(it), it[0], TARGET_RMS)
        assert wavs[b].shape == host_audio.shape[1:]
        assert abs(float(rms[b]) - host_rms) <= 1e-6 * host_rms               # (the host sums the squares in f32)
    pb_off = I.prompt_batch(prompts, GEN_TEXTS, target_rms=TARGET_RMS, mel_spec=ms, device=DEV)
    pb_on = I.prompt_batch(prompts, GEN_TEXTS, target_rms=TARGET_RMS, mel_spec=ms, device=DEV, prompt_on_device=True)
    assert isinstance(pb_on["rms"], torch.Tensor) and pb_on["rms"].device.type == "cuda"
    for key in ("lens", "durations", "texts"):
        assert pb_on[key] == pb_off[key], key
    off = I.synthesize_prompts(model, voc, prompts, GEN_TEXTS, target_rms=TARGET_RMS, **KW)
    on = I.synthesize_prompts(model, voc, prompts, GEN_TEXTS, target_rms=TARGET_RMS, prompt_on_device=True, **KW)
    for i in range(3):
        assert torch.isfinite(on[0][i]).all() and torch.isfinite(on[2][i]).all()
        assert on[0][i].shape == off[0][i].shape and on[2][i].shape == off[2][i].shape     # the same frame counts and durations


def test_synthesize_long_on_device_prompt():
    it = (44100, 5999, 2, 0.02)
    model, voc = tiny_model(), tiny_vocoder()
    chunks = ["I am the wind.", "Yes, indeed it is so."]
    off = I.synthesize_long((audio(it), it[0]), "Some call me nature.", chunks, model, voc, target_rms=TARGET_RMS, **KW)
    on = I.synthesize_long((audio(it), it[0]), "Some call me nature.", chunks, model, voc, target_rms=TARGET_RMS, prompt_on_device=True, **KW)
    assert on[1] == off[1] == TARGET and on[0].device.type == "cuda"
    assert on[0].shape == off[0].shape and on[2].shape == off[2].shape and torch.isfinite(on[0]).all()
