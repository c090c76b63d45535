"""GPU: the ragged Vocos decode (f5_vocos_decode_ragged, Vocos.decode_ragged, infer.synthesize_batch) -- a batch of windows
of unequal length decoded in one pass over packed rows.  The yardstick is the per-item path it replaces: every item must
be BIT-identical to f5_vocos_decode_strided on its own slice with B = 1 (the GEMMs' K order per element does not depend on
the row count, the conv / overlap-add kernels share their bodies with the rectangular ones), for windows whose boundaries
fall inside 64- and 128-row GEMM tiles and off every tile multiple.  Every mel frame outside an item's window is NaN, so a
read of a prompt frame, of a frame past the end or of a neighbour's row shows up in the output.  Outputs go to
gpu_util.Guarded buffers: guards intact, every element written, the tail behind each waveform exactly zero."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

F64 = torch.float64
F5_EINVAL = -1
HOP = 256
VOCOS_TOL = 4e-6   # max |wav - wav_64| / max |wav_64|: the bound of test_audio_kernels_gpu.test_vocos_decode_vs_float64_all_layouts
TAIL = 37          # samples of wav_stride past the longest waveform: every item has a tail to zero

# (start, end) per batch row of a [B, 100, T_max] mel
CASES = {
    # T_b = 2, 3, 37, 130: R = 172 packed rows, item boundaries at rows 2, 5, 42 -- inside the first 64- / 128-row tile
    "tiles": dict(T_max=200, windows=((0, 2), (5, 8), (1, 38), (64, 194))),
    # T_b = 130, 131, 2, 257: R = 520, boundaries at rows 130, 261, 263 -- more than one round of tiles, off every multiple
    "rounds": dict(T_max=270, windows=((0, 130), (3, 134), (0, 2), (7, 264))),
}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def vocos_weights(seed=3):
    return P.weights.synthetic_state_dict(P.weights.vocos_param_shapes(P.config.VOCOS_24K), seed=seed)


def vocos_handle(V):
    voc = P.Vocos(P.config.VOCOS_24K)
    voc.load_state_dict(V)
    voc.to(DEV)
    return voc, voc._handle()


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def shared_vocoder():
    def make():
        V = vocos_weights()
        return (V, *vocos_handle(V))
    return cached("voc", make)


def case_mel(name):
    """[B, 100, T_max] on the host: N(0, 1) inside each item's window, NaN everywhere else."""
    def make():
        c = CASES[name]
        B = len(c["windows"])
        mel = torch.full((B, 100, c["T_max"]), float("nan"))
        for b, (s, e) in enumerate(c["windows"]):
            mel[b, :, s:e] = torch.randn(100, e - s, generator=torch.Generator().manual_seed(100 * b + e))
        return mel
    return cached(("mel", name), make)


def layouts(mel):
    contig = mel.to(DEV).contiguous()
    perm = mel.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)    # sample()'s [B, T, C] output as decode sees it
    assert perm.stride() == (mel.shape[2] * 100, 1, 100)
    return {"contiguous": contig, "permuted": perm}


def strided_run(h, mel_view):
    """The existing rectangular decode of a [B, C, T] view -> (rc, Guarded [B, (T - 1) hop])."""
    B, _, T = mel_view.shape
    out = Guarded((B, (T - 1) * HOP), torch.float32)
    sb, sc, st = mel_view.stride()
    rc = _lib.load().f5_vocos_decode_strided(h, _ptr(mel_view), B, T, sb, sc, st, C.c_void_p(out.ptr()), _stream())
    torch.cuda.synchronize()
    return rc, out


def ragged_run(h, mel_view, windows, gain=None, wav_stride=None, use_starts=True, B=None):
    """f5_vocos_decode_ragged -> (rc, Guarded [B, wav_stride])."""
    starts, ends = [w[0] for w in windows], [w[1] for w in windows]
    if wav_stride is None:
        wav_stride = max((e - s - 1) * HOP for s, e in windows) + TAIL
    out = Guarded((len(windows), wav_stride), torch.float32)
    sb, sc, st = mel_view.stride()
    rc = _lib.load().f5_vocos_decode_ragged(h, _ptr(mel_view), len(windows) if B is None else B, sb, sc, st,
                                            _lib.int_array(starts) if use_starts else None, _lib.int_array(ends),
                                            None if gain is None else _lib.float_array(gain), C.c_void_p(out.ptr()), wav_stride,
                                            _stream())
    torch.cuda.synchronize()
    return rc, out


def per_item_reference(name):
    """Each item's slice decoded alone with B = 1 by the existing entry point: a list of int32 bit tensors on the device."""
    def make():
        _V, _voc, h = shared_vocoder()
        mel = case_mel(name).to(DEV)
        refs = []
        for b, (s, e) in enumerate(CASES[name]["windows"]):
            rc, out = strided_run(h, mel[b:b + 1, :, s:e])
            assert rc == 0 and out.guards_intact() and not torch.isnan(out.value).any()
            refs.append(out.bits[0].clone())
        return refs
    return cached(("ref", name), make)


def check_ragged(out, windows, refs, what):
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    assert not (out.bits == out.sent).any(), f"{what}: {int((out.bits == out.sent).sum())} output elements never written"
    assert not torch.isnan(out.value).any(), f"{what}: a frame outside an item's window was read"
    for b, (s, e) in enumerate(windows):
        L = (e - s - 1) * HOP
        assert torch.equal(out.bits[b, :L], refs[b]), \
            f"{what}: item {b} (T_b = {e - s}) differs from its own B = 1 decode in {int((out.bits[b, :L] != refs[b]).sum())} of {L} samples"
        assert not out.bits[b, L:].any(), f"{what}: item {b}: the tail behind the waveform is not all +0.0"


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_items_bit_equal_their_own_decode(name):
    """Tests 1 and 2 of the feature: bit-identity per item, nothing outside the windows read, both mel layouts."""
    _V, _voc, h = shared_vocoder()
    windows = CASES[name]["windows"]
    refs = per_item_reference(name)
    bits = {}
    for lay, view in layouts(case_mel(name)).items():
        rc, out = ragged_run(h, view, windows)
        assert rc == 0, _lib.load().f5_last_error().decode()
        check_ragged(out, windows, refs, f"{name} {lay}")
        bits[lay] = out.bits.clone()
    assert torch.equal(bits["contiguous"], bits["permuted"]), "the input layout changed the waveforms"


def test_degenerate_batches_equal_the_rectangular_decode():
    _V, _voc, h = shared_vocoder()
    T = 37
    mel = torch.randn(3, 100, T, generator=torch.Generator().manual_seed(11)).to(DEV)
    L = (T - 1) * HOP
    # one item, the whole row
    rc, want = strided_run(h, mel[:1])
    assert rc == 0
    rc, got = ragged_run(h, mel[:1], [(0, T)])
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_ragged(got, [(0, T)], [want.bits[0]], "B = 1")
    # equal lengths, starts = NULL: the rectangular batch
    rc, want = strided_run(h, mel)
    assert rc == 0
    rc, got = ragged_run(h, mel, [(0, T)] * 3, use_starts=False, wav_stride=L)
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_ragged(got, [(0, T)] * 3, list(want.bits), "equal lengths")
    assert torch.equal(got.bits, want.bits)


def test_ragged_items_vs_float64():
    """Bit-identity with the per-item path already implies the per-item path's accuracy; this catches a mistake both share."""
    V, _voc, h = shared_vocoder()
    windows = CASES["tiles"]["windows"]
    mel = case_mel("tiles")
    rc, out = ragged_run(h, layouts(mel)["permuted"], windows)
    assert rc == 0, _lib.load().f5_last_error().decode()
    got = out.value.cpu()
    for b, (s, e) in enumerate(windows):
        ref = O.vocos_decode(V, mel[b:b + 1, :, s:e].to(F64), dtype=F64)
        L = (e - s - 1) * HOP
        assert ref.shape == (1, L)
        err = ((got[b:b + 1, :L].to(F64) - ref).abs().max() / ref.abs().max()).item()
        print(f"[vocos ragged f32] item {b} T_b={e - s}: rel err {err:.3e} (peak {ref.abs().max().item():.3f}, bound {VOCOS_TOL:.1e})")
        assert err < VOCOS_TOL


def test_gain_is_one_f32_multiply_per_sample():
    _V, _voc, h = shared_vocoder()
    windows = CASES["tiles"]["windows"]
    gain = (0.5, 1.0, 0.037, 2.0)
    refs = per_item_reference("tiles")
    scaled = [(r.view(torch.float32) * torch.tensor(g, dtype=torch.float32, device=DEV)).view(torch.int32) for r, g in zip(refs, gain)]
    rc, out = ragged_run(h, layouts(case_mel("tiles"))["permuted"], windows, gain=gain)
    assert rc == 0, _lib.load().f5_last_error().decode()
    check_ragged(out, windows, scaled, "gain")


def test_arena_reuse_and_determinism():
    """One handle: ragged R = 520, ragged R = 172, a rectangular decode, R = 520 again (the workspace only grows and is never
    cleared; the device tables of the ragged calls live in it): each result equals a fresh handle's; a repeated call is
    bit-identical."""
    V = vocos_weights(seed=5)
    _voc, h = vocos_handle(V)
    rect = torch.randn(3, 100, 130, generator=torch.Generator().manual_seed(130)).to(DEV)
    views = {n: layouts(case_mel(n))["permuted"] for n in CASES}

    def run(handle, step):
        rc, out = strided_run(handle, rect) if step == "rect" else ragged_run(handle, views[step], CASES[step]["windows"])
        assert rc == 0, _lib.load().f5_last_error().decode()
        assert out.guards_intact() and not (out.bits == out.sent).any()
        return out.bits.clone()

    fresh = {}
    for step in ("rounds", "tiles", "rect", "rounds"):
        got = run(h, step)
        assert torch.equal(got, run(h, step)), f"{step}: two identical calls differ"
        if step not in fresh:
            _voc2, h2 = vocos_handle(V)
            fresh[step] = run(h2, step)
            del _voc2
        assert torch.equal(got, fresh[step]), f"{step}: the reused workspace differs from a fresh handle"


def test_refusals_launch_nothing():
    _V, _voc, h = shared_vocoder()
    lib = _lib.load()
    mel = layouts(case_mel("tiles"))["contiguous"]
    windows = list(CASES["tiles"]["windows"])
    Lmax = 129 * HOP

    def refused(out, what):
        assert out.guards_intact() and (out.bits == out.sent).all(), f"{what}: a refused call wrote to the output"

    one = windows[:2] + [(9, 10)] + windows[3:]
    rc, out = ragged_run(h, mel, one)
    assert rc == F5_EINVAL and b"item 2" in lib.f5_last_error(), lib.f5_last_error()
    refused(out, "T_b = 1")
    rc, out = ragged_run(h, mel, windows, wav_stride=Lmax - 1)
    assert rc == F5_EINVAL
    refused(out, "wav_stride too small")
    rc, out = ragged_run(h, mel, [(-1, 2)] + windows[1:])
    assert rc == F5_EINVAL
    refused(out, "negative start")
    rc, out = ragged_run(h, mel, windows, B=0)
    assert rc == F5_EINVAL
    refused(out, "B = 0")


def test_synthesize_batch_equals_sample_then_per_item_decode():
    from f5_tts_amd import infer as I

    g = torch.Generator().manual_seed(9)
    tr = P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100, precision="f32").init_synthetic(seed=2)
    model = P.CFM(transformer=tr).to(DEV)
    voc = P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV)
    lens = [20, 33, 27]
    cond = torch.zeros(3, max(lens), 100)
    for i, n in enumerate(lens):
        cond[i, :n] = torch.randn(n, 100, generator=g)
    nts = [9, 14, 40]                       # item 2: 40 text tokens > its 27 prompt frames and its requested 30 -> runs at 41
    text = torch.full((3, max(nts)), -1, dtype=torch.long)
    for i, n in enumerate(nts):
        text[i, :n] = torch.randint(1, 39, (n,), generator=g)
    duration = torch.tensor([70, 95, 30])
    durs = [70, 95, 41]
    kw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    wav, wav_lens, mel = I.synthesize_batch(model, voc, cond, text, duration, lens=lens, **kw)
    want_mel, _ = model.sample(cond, text, duration, lens=torch.tensor(lens), **kw)
    assert mel.shape == (3, 95, 100) and torch.equal(mel, want_mel)
    assert wav_lens == [(d - n - 1) * HOP for d, n in zip(durs, lens)] and wav.shape == (3, max(wav_lens))
    assert not torch.isnan(wav).any()
    for i in range(3):
        one = voc.decode(mel[i:i + 1, lens[i]:durs[i]].permute(0, 2, 1))
        assert torch.equal(wav[i, :wav_lens[i]].view(torch.int32), one[0].view(torch.int32)), f"item {i} differs from its own decode"
        assert not wav[i, wav_lens[i]:].view(torch.int32).any()
