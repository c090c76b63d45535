"""GPU: both ends of the audio path -- the mel front-end (csrc/mel.hip, both variants), the Vocos decoder (csrc/vocos.hip with
the im2col / depthwise-conv / ISTFT kernels of csrc/elementwise.h) and the BigVGAN generator (csrc/bigvgan.hip) -- through
their C entry points, against a float64 evaluation of the same operation on the same weights (the oracle restatements run
with dtype=torch.float64; the mel reference uses the product's own filterbank tables).

Every call writes into a gpu_util.Guarded buffer: the NaN guard bands around the output must be intact afterwards and no
sentinel may remain inside it (every output element written, none outside).  Edge shapes (the shortest inputs each entry
point accepts, T = 2 / 3 frames, lengths at and just past a multiple of hop), strided input views, arena reuse across sizes,
refusals, the clip and range reduction of the ISTFT head and snake arguments in the hundreds are covered here; the tolerances
are about twice the worst error measured on the MI355X (printed by each test)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from oracle import bigvgan_oracle as BO  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

F64 = torch.float64
F5_EINVAL = -1
N_FFT, HOP, N_MELS, NF = 1024, 256, 100, 513


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def check_layout(out: Guarded, what):
    """Guard bands intact and every element written (no sentinel left inside)."""
    assert out.guards_intact(), f"{what}: a guard band was overwritten"
    assert not (out.bits == out.sent).any(), f"{what}: {int((out.bits == out.sent).sum())} output elements never written"


# -------------------------------------------------------------------------------------------------- mel front-end
MEL_VARIANTS = {"vocos": (N_FFT // 2, 0.0), "bigvgan": ((N_FFT - HOP) // 2, 1e-9)}   # (reflect pad, magnitude eps), mel.py
MEL_MIN_NW = {"vocos": 513, "bigvgan": 385}       # the shortest input each variant accepts: 3 frames / 1 frame
MEL_FLOOR = 1e-2        # bands with at least this fraction of their frame's largest mel energy: held to MEL_TOL (log domain)
# measured worst: noise 4.0e-6, square 8.3e-6, sine 2.1e-6, DC 6.4e-7, silence (bigvgan variant) 6.4e-7
MEL_TOL = {"noise": 8e-6, "square": 2e-5, "sine": 5e-6, "dc": 2e-6, "silence": 2e-6}
MEL_LIN_TOL = 4e-6      # every band: |mel - mel_64| / (the frame's largest mel energy); measured worst 1.8e-6


def product_fb(variant):
    """The filterbank mel.py uploads, [n_mels, n_freqs] f32."""
    make = P.mel.htk_mel_filterbank if variant == "vocos" else P.mel.slaney_mel_filterbank
    return make(NF, N_MELS, 24000)


def mel_ref64(variant, wav):
    """float64 log-mel [B, T, n_mels] of the same operation on the product's filterbank."""
    fb = product_fb(variant).to(F64)
    if variant == "vocos":
        r = O.mel_spectrogram_vocos(wav.to(F64), dtype=F64, fb=fb.t())
    else:
        r = BO.mel_spectrogram_bigvgan(wav.to(F64), dtype=F64, fb=fb)
    return r.permute(0, 2, 1)


def mel_frames(variant, nw):
    pad = MEL_VARIANTS[variant][0]
    return (nw + 2 * pad - N_FFT) // HOP + 1


def mel_run(h, variant, wav_dev, pad=None, eps=None):
    """f5_mel_forward_ex into a Guarded [B, T, n_mels]; returns (rc, guarded buffer)."""
    p0, e0 = MEL_VARIANTS[variant]
    pad = p0 if pad is None else pad
    eps = e0 if eps is None else eps
    B, nw = wav_dev.shape
    T = max(1, (nw + 2 * pad - N_FFT) // HOP + 1)
    out = Guarded((B, T, N_MELS), torch.float32)
    rc = _lib.load().f5_mel_forward_ex(h, _ptr(wav_dev), B, nw, pad, eps, C.c_void_p(out.ptr()), _stream())
    torch.cuda.synchronize()
    return rc, out


def mel_handle(variant):
    return P.mel.MelSpec(mel_spec_type=variant)._handle(torch.device(DEV))


def mel_signal(kind, B, nw):
    n = torch.arange(nw, dtype=F64)
    rows = []
    for b in range(B):
        if kind == "noise":
            x = torch.randn(nw, generator=torch.Generator().manual_seed(100 * b + nw), dtype=F64) * 0.1
        elif kind == "square":      # full scale: +-1 exactly, half period 24 + 4 b samples
            x = torch.where((n // (24 + 4 * b)) % 2 == 0, 1.0, -1.0).to(F64)
        elif kind == "sine":        # on the centre of DFT bin 40 + 17 b
            x = 0.5 * torch.sin(2 * math.pi * (40 + 17 * b) * n / N_FFT)
        elif kind == "dc":
            x = torch.full((nw,), 0.5 - 0.125 * (b % 5), dtype=F64)
        else:                       # digital silence
            x = torch.zeros(nw, dtype=F64)
        rows.append(x)
    return torch.stack(rows).to(torch.float32)


MEL_SIGNALS = ["noise", "square", "sine", "dc", "silence"]

@pytest.mark.parametrize("variant", list(MEL_VARIANTS))
@pytest.mark.parametrize("kind", MEL_SIGNALS)
def test_mel_frontend_vs_float64(variant, kind):
    """Log-mel against float64 with an absolute bound on every band that holds at least MEL_FLOOR of its frame's largest
    mel energy (for white noise: almost all of them); on every band, the linear-domain error relative to that largest
    energy.  Why not one absolute log bound everywhere: an f32 DFT of a frame has an absolute rounding floor of about
    1e-6 of the frame's peak, so bands that hold (nearly) no energy in float64 -- below the lowest harmonic of the
    full-scale square wave, away from the bin of the sine or of DC -- come out at ~1e-5 instead of ~0, and the log turns
    that into an error of O(0.1) at the 1e-5 clamp.  The f32 CPU restatement (torch.stft) shows the same (0.08 for the
    square wave, 0.2 for the sine): it is inherent to the f32 arithmetic the path is specified to use."""
    h = mel_handle(variant)
    e_log = e_lin = 0.0
    covered = []
    for B in (1, 3, 8):
        for nw in (MEL_MIN_NW[variant], 96 * HOP, 96 * HOP + 1, 240000):
            wav = mel_signal(kind, B, nw)
            rc, out = mel_run(h, variant, wav.to(DEV))
            assert rc == 0, _lib.load().f5_last_error().decode()
            T = mel_frames(variant, nw)
            assert out.shape == (B, T, N_MELS)
            check_layout(out, f"mel {variant} B={B} nw={nw}")
            got = out.value.cpu()
            if variant == "vocos" and kind == "silence":
                # |S| = 0 everywhere: every output is the clamp, logf(1e-5f) within 1 ulp of torch's f32 log
                want = torch.tensor(1e-5, dtype=torch.float32).log()
                ulp = torch.nextafter(want, torch.tensor(0.0)) - want
                assert ((got - want).abs() <= ulp.abs()).all(), f"silence: {got.min().item()} .. {got.max().item()} vs {want.item()}"
                continue
            ref = mel_ref64(variant, wav)
            assert ref.shape == got.shape
            err = (got.to(F64) - ref).abs()
            lin_g, lin_r = got.to(F64).exp(), ref.exp()
            peak = lin_r.amax(-1, keepdim=True)
            big = lin_r >= MEL_FLOOR * peak
            covered.append(big.double().mean().item())
            e_log = max(e_log, err[big].max().item())
            e_lin = max(e_lin, ((lin_g - lin_r).abs() / peak).max().item())
    covered = min(covered, default=1.0)
    print(f"[mel {variant}] {kind}: log-mel abs err {e_log:.3e} on {covered:.2f}+ of the bands (bound {MEL_TOL[kind]:.1e}), "
          f"linear err / frame peak {e_lin:.3e} (bound {MEL_LIN_TOL:.1e})")
    if kind == "noise":
        assert covered > 0.9
    assert e_log < MEL_TOL[kind] and e_lin < MEL_LIN_TOL


@pytest.mark.parametrize("variant", list(MEL_VARIANTS))
def test_mel_frontend_refuses_too_short_inputs(variant):
    h = mel_handle(variant)
    pad = MEL_VARIANTS[variant][0]
    for nw, p in ((pad, pad), (800, 100)):       # nw <= pad;  nw + 2 pad < n_fft
        wav = torch.zeros(2, nw, device=DEV)
        rc, out = mel_run(h, variant, wav, pad=p)
        assert rc == F5_EINVAL, f"nw={nw} pad={p}: rc {rc}"
        assert out.guards_intact() and (out.bits == out.sent).all(), "a refused call launched nothing"


@pytest.mark.parametrize("variant", list(MEL_VARIANTS))
def test_mel_frontend_arena_reuse_is_bit_exact(variant):
    """One handle runs 240000 -> 513 -> 24000 samples (the arena only grows, and is zeroed only then): each result equals
    that of a fresh handle bit for bit."""
    h = mel_handle(variant)
    for nw in (240000, 513, 24000):
        wav = mel_signal("noise", 3, nw).to(DEV)
        rc, out = mel_run(h, variant, wav)
        assert rc == 0
        check_layout(out, f"reused handle nw={nw}")
        rc, fresh = mel_run(mel_handle(variant), variant, wav)
        assert rc == 0
        assert torch.equal(out.bits, fresh.bits), f"nw={nw}: reused arena differs from a fresh handle"


# -------------------------------------------------------------------------------------------------- Vocos
VOCOS_TOL = 4e-6          # max |wav - wav_64| / max |wav_64|; measured worst 2.0e-6 (T = 938, B = 3)
VOCOS_HEAD_TOL = 3e-5     # measured worst 1.5e-5: phases of |p| ~ 100 carry an f32 rounding of ~1e-5 into cos / sin


def vocos_weights(seed=3, head_edge=False):
    V = P.weights.synthetic_state_dict(P.weights.vocos_param_shapes(P.config.VOCOS_24K), seed=seed)
    if head_edge:
        # log-magnitudes ~ N(3, 1.8^2): about a third above ln 100 (the clip); phases ~ N(0, 25^2): |p| up to ~100
        w, b = V["head.out.weight"].clone(), V["head.out.bias"].clone()
        w[:NF] *= 4.0
        b[:NF] += 3.0
        w[NF:] *= 20.0
        V["head.out.weight"], V["head.out.bias"] = w, b
    return V


def vocos_handle(V):
    voc = P.Vocos(P.config.VOCOS_24K)
    voc.load_state_dict(V)
    voc.to(DEV)
    return voc, voc._handle()


def vocos_run(h, mel_view):
    """f5_vocos_decode_strided on any [B, C, T] view into a Guarded [B, (T-1) hop]; returns (rc, guarded buffer)."""
    B, Cc, T = mel_view.shape
    out = Guarded((B, max(T - 1, 1) * HOP), torch.float32)
    sb, sc, st = mel_view.stride()
    rc = _lib.load().f5_vocos_decode_strided(h, _ptr(mel_view), B, T, sb, sc, st, C.c_void_p(out.ptr()), _stream())
    torch.cuda.synchronize()
    return rc, out


def mel_layouts(mel):
    """The same [B, C, T] values as: contiguous; sample()'s [B, T, C] output permuted; a view at an element offset into a
    NaN-filled buffer with stride_b > C T."""
    B, Cc, T = mel.shape
    contig = mel.to(DEV).contiguous()
    perm = mel.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
    sb, off = Cc * T + 53, 11
    base = torch.full((off + B * sb,), float("nan"), device=DEV)
    off_view = base.as_strided((B, Cc, T), (sb, T, 1), off)
    off_view.copy_(contig)
    assert perm.stride() == (T * Cc, 1, Cc) and off_view.stride()[0] > Cc * T and off_view.storage_offset() == off
    return {"contiguous": contig, "permuted": perm, "offset": off_view}


def rel_err(got, ref):
    return ((got.to(F64) - ref).abs().max() / ref.abs().max()).item()


_VOC = {}


def vocos_cached(head_edge=False):
    if head_edge not in _VOC:
        V = vocos_weights(head_edge=head_edge)
        _VOC[head_edge] = (V, *vocos_handle(V))
    return _VOC[head_edge]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [2, 3, 4, 37, 130, 938])
def test_vocos_decode_vs_float64_all_layouts(T, B):
    V, _voc, h = vocos_cached()
    mel = torch.randn(B, 100, T, generator=torch.Generator().manual_seed(7 * T + B))
    ref = O.vocos_decode(V, mel.to(F64), dtype=F64)
    assert ref.shape == (B, (T - 1) * HOP)
    wavs = {}
    for name, view in mel_layouts(mel).items():
        rc, out = vocos_run(h, view)
        assert rc == 0, _lib.load().f5_last_error().decode()
        check_layout(out, f"vocos T={T} B={B} {name}")
        wavs[name] = out.bits.clone()
    assert torch.equal(wavs["contiguous"], wavs["permuted"]) and torch.equal(wavs["contiguous"], wavs["offset"]), \
        "the input layout changed the waveform"
    e = rel_err(wavs["contiguous"].view(torch.float32).cpu(), ref)
    print(f"[vocos f32] T={T} B={B}: rel err {e:.3e} (peak {ref.abs().max().item():.3f}, bound {VOCOS_TOL:.1e})")
    assert e < VOCOS_TOL


def test_vocos_head_clip_and_large_phases_vs_float64():
    """Head outputs past the exp clip (|S| = 100) and phases of |p| ~ 50 .. 100 through cosf / sinf."""
    V, _voc, h = vocos_cached(head_edge=True)
    for T, B in ((3, 1), (130, 3)):
        mel = torch.randn(B, 100, T, generator=torch.Generator().manual_seed(T))
        x = O.linear(O.vocos_backbone(V, mel.to(F64), dtype=F64), O.weights_as(V, F64), "head.out")
        logmag, phase = x[..., :NF], x[..., NF:]
        clipped = (logmag > math.log(100.0)).double().mean().item()
        pmax = phase.abs().max().item()
        assert clipped > 0.05, f"the clip must trigger (fraction {clipped:.3f})"
        assert 50 < pmax < 200, pmax
        ref = O.vocos_decode(V, mel.to(F64), dtype=F64)
        rc, out = vocos_run(h, mel_layouts(mel)["permuted"])
        assert rc == 0
        check_layout(out, f"vocos head edge T={T}")
        e = rel_err(out.value.cpu(), ref)
        print(f"[vocos f32 head edge] T={T} B={B}: rel err {e:.3e} (clipped {clipped:.3f}, max |phase| {pmax:.1f}, "
              f"bound {VOCOS_HEAD_TOL:.1e})")
        assert e < VOCOS_HEAD_TOL


def test_vocos_refuses_one_frame():
    _V, _voc, h = vocos_cached()
    mel = torch.randn(2, 100, 1, device=DEV)
    rc, out = vocos_run(h, mel)
    assert rc == F5_EINVAL
    assert out.guards_intact() and (out.bits == out.sent).all(), "a refused call launched nothing"


def test_vocos_arena_reuse_and_determinism():
    """One handle decodes T = 938 -> 2 -> 130 (the arena is never cleared on reuse): bit-equal to fresh handles; two decodes
    of the same input are bit-identical."""
    V = vocos_weights(seed=5)
    _voc, h = vocos_handle(V)
    for T in (938, 2, 130):
        mel = torch.randn(3, 100, T, generator=torch.Generator().manual_seed(T)).to(DEV)
        rc, out = vocos_run(h, mel)
        assert rc == 0
        check_layout(out, f"reused handle T={T}")
        rc, again = vocos_run(h, mel)
        assert rc == 0 and torch.equal(out.bits, again.bits), f"T={T}: two decodes differ"
        _voc2, h2 = vocos_handle(V)
        rc, fresh = vocos_run(h2, mel)
        assert rc == 0 and torch.equal(out.bits, fresh.bits), f"T={T}: reused arena differs from a fresh handle"
        del _voc2


# -------------------------------------------------------------------------------------------------- BigVGAN
BIGVGAN_MID = dict(P.config.BIGVGAN_V2_24K, upsample_initial_channel=256)    # all 6 stages, 256 -> 4 channels (test_bigvgan.py)
BV_CFGS = {"BIGVGAN_TINY": P.config.BIGVGAN_TINY, "BIGVGAN_MID": BIGVGAN_MID}
# max |wav - wav_64| / max(1, peak); measured worst (BIGVGAN_MID): f32 7.7e-7, f16x3 1.2e-6; large snake f32 5.0e-6, f16x3 8.8e-6
BV_TOL = {"f32": 1.5e-6, "f16x3": 2.5e-6}
BV_SNAKE_TOL = {"f32": 1e-5, "f16x3": 2e-5}


def bigvgan_weights(cfg, seed, large_snake=False):
    V = P.weights.synthetic_state_dict(P.weights.bigvgan_param_shapes(cfg), seed=seed)
    if large_snake:
        # alpha = exp(log alpha) ~ 30 (x e^{+-0.9}), 1 / beta ~ 0.14: snake arguments |alpha x| of 100 .. 200 while the
        # sin^2 term keeps the signal bounded
        for k in V:
            if k.endswith(".act.alpha"):
                V[k] = V[k] + 3.4
            elif k.endswith(".act.beta"):
                V[k] = V[k] + 2.0
    return V


def bigvgan_handle(cfg, V, prec):
    voc = P.BigVGAN(cfg, precision=prec)
    voc.load_state_dict(V)
    voc.to(DEV)
    return voc, voc._handle()


def bigvgan_run(voc, h, mel_view):
    B, Cc, T = mel_view.shape
    out = Guarded((B, 1, T * voc.total_up), torch.float32)
    sb, sc, st = mel_view.stride()
    rc = _lib.load().f5_bigvgan_forward(h, _ptr(mel_view), B, T, sb, sc, st, C.c_void_p(out.ptr()), _stream())
    torch.cuda.synchronize()
    return rc, out


_BV_REF = {}


def bigvgan_ref64_cached(key, V, cfg, mel, record=None):
    """bigvgan_ref64, computed once per case for both precisions."""
    if key not in _BV_REF:
        args = []
        _BV_REF[key] = (bigvgan_ref64(V, cfg, mel, record=args), args)
    ref, args = _BV_REF[key]
    if record is not None:
        record.extend(args)
    return ref


def bigvgan_ref64(V, cfg, mel, record=None):
    """float64 generator; record: a list that receives max |alpha x| of every snake evaluation."""
    if record is None:
        return BO.bigvgan_forward(V, cfg, mel.to(F64), dtype=F64)
    snake = BO.snake_beta

    def spy(x, log_alpha, log_beta):
        record.append((x * torch.exp(log_alpha)[None, :, None]).abs().max().item())
        return snake(x, log_alpha, log_beta)

    BO.snake_beta = spy
    try:
        return BO.bigvgan_forward(V, cfg, mel.to(F64), dtype=F64)
    finally:
        BO.snake_beta = snake


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("cfg_name,T,B", [("BIGVGAN_TINY", 1, 2), ("BIGVGAN_TINY", 2, 1), ("BIGVGAN_TINY", 37, 2),
                                          ("BIGVGAN_MID", 24, 1)])
def test_bigvgan_vs_float64_layouts_and_edges(cfg_name, T, B, prec):
    """Contiguous and permuted inputs give bit-identical waveforms; T = 1 and 2 are the shortest inputs (every edge clamp of
    the activation and convolution kernels at once); guard bands around B * T * prod(upsample_rates) samples."""
    cfg = BV_CFGS[cfg_name]
    V = bigvgan_weights(cfg, seed=3)
    voc, h = bigvgan_handle(cfg, V, prec)
    mel = torch.randn(B, T, 100, generator=torch.Generator().manual_seed(T)).permute(0, 2, 1)
    ref = bigvgan_ref64_cached((cfg_name, T, B), V, cfg, mel)
    lay = mel_layouts(mel)
    wavs = {}
    for name in ("contiguous", "permuted"):
        rc, out = bigvgan_run(voc, h, lay[name])
        assert rc == 0, _lib.load().f5_last_error().decode()
        check_layout(out, f"bigvgan {cfg_name} T={T} {name}")
        wavs[name] = out.bits.clone()
    assert torch.equal(wavs["contiguous"], wavs["permuted"]), "the input layout changed the waveform"
    got = wavs["contiguous"].view(torch.float32).cpu()
    assert got.shape == ref.shape
    e = (got.to(F64) - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"[bigvgan {prec}] {cfg_name} T={T} B={B}: err {e:.3e} (peak {ref.abs().max().item():.3f}, bound {BV_TOL[prec]:.1e})")
    assert e < BV_TOL[prec]


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("cfg_name,T", [("BIGVGAN_TINY", 37), ("BIGVGAN_MID", 24)])
def test_bigvgan_large_snake_arguments_vs_float64(cfg_name, T, prec):
    """Snake arguments |alpha x| of 100 .. 200: the range reductions of bv_sin (f32) and bv_sin_hw (f16x3).  The error grows
    over the normal case (7.7e-7 -> 5.0e-6 on BIGVGAN_MID) because an f32 argument of ~150 is itself rounded by ~1e-5 and
    the residual branches carry that on; the f32 CPU restatement with libm's sinf misses float64 by the same amount
    (5.2e-6), so bv_sin stays in the error class of a correctly rounded f32 sine.  Measured: f32 5.0e-6, f16x3 8.8e-6."""
    cfg = BV_CFGS[cfg_name]
    V = bigvgan_weights(cfg, seed=4, large_snake=True)
    voc, h = bigvgan_handle(cfg, V, prec)
    mel = torch.randn(1, T, 100, generator=torch.Generator().manual_seed(T)).permute(0, 2, 1)
    args = []
    ref = bigvgan_ref64_cached((cfg_name, T, "snake"), V, cfg, mel, record=args)
    assert max(args) > 100, f"max |alpha x| {max(args):.1f}"
    rc, out = bigvgan_run(voc, h, mel.to(DEV))
    assert rc == 0
    check_layout(out, f"bigvgan large snake {cfg_name}")
    e = (out.value.cpu().to(F64) - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"[bigvgan {prec} large snake] {cfg_name} T={T}: err {e:.3e} (max |alpha x| {max(args):.1f}, "
          f"clipped {(ref.abs() >= 1).double().mean().item():.3f}, bound {BV_SNAKE_TOL[prec]:.1e})")
    assert e < BV_SNAKE_TOL[prec]
