"""GPU: the host machinery the audio stages share (csrc/internal.h: Arena::reserve, WeightStore, DevPool, Staging::upload) and
the Python owner of their handles (native.NativeModule), through MelSpec, Vocos and BigVGAN at tiny shapes.  Everything is
compared bit for bit: a handle that was dropped and rebuilt, reloaded and finalized again, or whose workspace grew between two
calls must give what a fresh one gives."""
import ctypes as C
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV, Guarded  # noqa: E402

import f5_tts_amd as P  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402

F5_EINVAL, F5_ESTATE = -1, -3
MEL_VARIANTS = ("vocos", "bigvgan")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def err():
    return _lib.load().f5_last_error().decode()


def bits(t):
    return t.contiguous().view(torch.int32)


def noise(*shape, seed):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.1).to(DEV)


# ------------------------------------------------------------------------------------------------ MelSpec lifecycle
@pytest.mark.parametrize("variant", MEL_VARIANTS)
def test_melspec_drops_rebuilds_and_destroys_its_handle(variant):
    """forward, _drop_handle, forward again: bit-equal.  A second instance is collected (f5_mel_destroy from __del__); a third
    one still works and agrees."""
    wav = noise(2, 1500, seed=1)
    ms = P.mel.MelSpec(mel_spec_type=variant)
    first = bits(ms(wav)).clone()
    assert ms._h is not None and ms._h_dev == wav.device
    ms._drop_handle()
    assert ms._h is None and ms._h_dev is None
    assert torch.equal(bits(ms(wav)), first), "a rebuilt handle differs from the first one"
    ms2 = P.mel.MelSpec(mel_spec_type=variant)
    assert torch.equal(bits(ms2(wav)), first)
    del ms2
    gc.collect()
    ms3 = P.mel.MelSpec(mel_spec_type=variant)
    assert torch.equal(bits(ms3(wav)), first), "an instance made after another was collected differs"
    assert torch.equal(bits(ms(wav)), first), "collecting one instance disturbed another"


# ------------------------------------------------------------------------------------------------ reload after finalize
# (module, config, frames, entry-point prefix, decode entry point, what finalize calls the weights, a tensor that gets new
#  values, a tensor that is first loaded with a wrong shape)
VOCODERS = {
    "vocos": dict(make=lambda: P.Vocos(P.config.VOCOS_TINY), T=3, prefix="f5_vocos", decode="f5_vocos_decode_strided",
                  changed="backbone.norm.weight", misshapen="backbone.norm.bias",
                  samples=lambda voc, T: (T - 1) * voc.cfg["hop_length"]),
    "bigvgan": dict(make=lambda: P.BigVGAN(P.config.BIGVGAN_TINY), T=2, prefix="f5_bigvgan", decode="f5_bigvgan_forward",
                    changed="activation_post.act.alpha", misshapen="activation_post.act.beta",
                    samples=lambda voc, T: T * voc.total_up),
}


def vocoder_run(kind, voc, h, mel):
    """The rectangular decode of mel f32[B, C, T] through the C entry point -> (rc, Guarded [B, samples])."""
    v = VOCODERS[kind]
    B, _, T = mel.shape
    out = Guarded((B, v["samples"](voc, T)), torch.float32)
    sb, sc, st = mel.stride()
    rc = getattr(_lib.load(), v["decode"])(h, _ptr(mel), B, T, sb, sc, st, C.c_void_p(out.ptr()), _stream())
    torch.cuda.synchronize()
    return rc, out


def load_tensor(kind, h, name, t):
    d = t.to(DEV, torch.float32).contiguous()
    rc = getattr(_lib.load(), VOCODERS[kind]["prefix"] + "_load_weight")(h, name.encode(), _ptr(d), _lib.shape_array(d.shape), d.dim(),
                                                                       _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kind", list(VOCODERS))
def test_reload_on_a_live_handle_needs_finalize_and_equals_a_fresh_handle(kind):
    """f5_*_load_weight on a finalized handle: decode refuses (F5_ESTATE) until f5_*_finalize has run again.  finalize releases
    the raw store, so the reload brings every tensor; one with a wrong shape fails finalize (F5_EINVAL, the tensor named) and
    loading it again with the right shape repairs it.  The reloaded handle then equals a fresh one on the same weights."""
    v = VOCODERS[kind]
    lib = _lib.load()
    finalize = getattr(lib, v["prefix"] + "_finalize")
    voc = v["make"]().init_synthetic(seed=2).to(DEV)
    h = voc._handle()
    mel = noise(2, 100, v["T"], seed=3) * 10
    rc, before = vocoder_run(kind, voc, h, mel)
    assert rc == 0, err()

    sd = voc.state_dict()
    sd[v["changed"]] = sd[v["changed"]] + 0.25
    fresh = v["make"]()
    fresh.load_state_dict(sd)
    fresh.to(DEV)
    tensors = dict(fresh._tensors())

    def refused(what):
        rc, out = vocoder_run(kind, voc, h, mel)
        assert rc == F5_ESTATE and f"{v['prefix']}_finalize has not been called" in err(), f"{what}: rc {rc}, {err()}"
        assert out.guards_intact() and (out.bits == out.sent).all(), f"{what}: a refused call launched something"

    assert load_tensor(kind, h, v["changed"], tensors[v["changed"]]) == 0, err()
    refused("one tensor reloaded")
    assert finalize(h, _stream()) == F5_ESTATE and f"missing {kind} weight" in err()     # the raw store was released by the first finalize
    refused("finalize without the other tensors")
    for name, t in tensors.items():
        wrong = name == v["misshapen"]
        assert load_tensor(kind, h, name, torch.cat([t, t]) if wrong else t) == 0, err()
    assert finalize(h, _stream()) == F5_EINVAL
    assert err() == f"{kind} weight '{v['misshapen']}' has the wrong shape"
    refused("finalize failed on a shape")
    assert load_tensor(kind, h, v["misshapen"], tensors[v["misshapen"]]) == 0, err()
    assert finalize(h, _stream()) == 0, err()
    rc, after = vocoder_run(kind, voc, h, mel)
    assert rc == 0, err()
    rc, want = vocoder_run(kind, fresh, fresh._handle(), mel)
    assert rc == 0, err()
    assert after.guards_intact() and not (after.bits == after.sent).any()
    assert torch.equal(after.bits, want.bits), "the reloaded handle differs from a fresh one on the same weights"
    assert not torch.equal(after.bits, before.bits), "the new values did not reach the packed weights"


# ------------------------------------------------------------------------------------------------ growth keeps results
@pytest.mark.parametrize("kind", list(VOCODERS))
def test_vocoder_workspace_growth_keeps_results(kind):
    """T = 2 (the block is made), T = 40 (it is replaced), T = 2 again (it stays): the two small results are bit-equal."""
    voc = VOCODERS[kind]["make"]().init_synthetic(seed=5).to(DEV)
    h = voc._handle()
    small, large = noise(2, 100, 2, seed=6) * 10, noise(2, 100, 40, seed=7) * 10
    got = []
    for mel in (small, large, small):
        rc, out = vocoder_run(kind, voc, h, mel)
        assert rc == 0, err()
        assert out.guards_intact() and not (out.bits == out.sent).any()
        got.append(out.bits.clone())
    assert torch.equal(got[0], got[2]), "the small decode changed after the workspace grew"


@pytest.mark.parametrize("ragged", [False, True])
def test_mel_workspace_growth_keeps_results(ragged):
    """nw = 1100, then 9000 (the block is replaced), then 1100 again, through f5_mel_forward_ex and f5_mel_forward_ragged."""
    ms = P.mel.MelSpec()
    small, large = noise(2, 1100, seed=8), noise(2, 9000, seed=9)
    run = (lambda w: ms.forward_ragged(list(w))[0]) if ragged else ms
    first = bits(run(small)).clone()
    assert torch.isfinite(run(large)).all()
    assert torch.equal(bits(run(small)), first), "the small call changed after the workspace grew"
    assert torch.equal(first, bits(P.mel.MelSpec()(small))), "... or differs from a fresh handle"


# ------------------------------------------------------------------------------------------------ Staging::upload ring
def test_ragged_tables_survive_the_staging_ring_wrapping():
    """Nine ragged calls in a row on one handle, nothing synchronised in between (the ring has 8 pinned slots): every call
    equals the first."""
    voc = P.Vocos(P.config.VOCOS_TINY).init_synthetic(seed=4).to(DEV)
    mel = noise(3, 100, 5, seed=10) * 10
    waves = [voc.decode_ragged(mel, ends=[2, 5, 3])[0] for _ in range(9)]
    ms = P.mel.MelSpec()
    prompts = [noise(n, seed=n) for n in (1100, 1500, 2049)]
    mels = [ms.forward_ragged(prompts)[0] for _ in range(9)]
    torch.cuda.synchronize()
    for i in range(1, 9):
        assert torch.equal(bits(waves[i]), bits(waves[0])), f"decode_ragged call {i} differs from call 0"
        assert torch.equal(bits(mels[i]), bits(mels[0])), f"forward_ragged call {i} differs from call 0"
    assert torch.isfinite(waves[0]).all() and torch.isfinite(mels[0]).all()
