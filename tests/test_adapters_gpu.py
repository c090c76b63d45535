"""GPU: resident LoRA adapters (F5_OPT_ADAPTERS, f5_set_adapter).  An engine switched to an adapter must compute, bit for
bit, what a fresh engine computes on the state dict merged on the host by the ABI's rule (product rounded, then added, in
ascending rank; adapters.merge_adapter(rule="contract")); switching must leave nothing behind; and the result must agree
with the reference's semantics (torch's `B @ A` merge through convert_peft_state_dict_to_plain, run by the CPU oracle)
inside the parity gates of tests/test_sample_gpu.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import adapter_util as U  # noqa: E402
import f5_tts_amd as P  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from f5_tts_amd import _lib, adapters as A  # noqa: E402
from f5_tts_amd import infer as I  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402
from test_sample_gpu import TOL_16, TOL_PARITY, build_cfm, run_case, valid_frames  # noqa: E402

PRECS = ["f32", "bf16", "f16", "f16x3", "f16p"]
FIXTURES = ["sample_b1_nfe16", "sample_b3_attnmask"]   # B = 1; B = 3 with attn_mask_enabled (packed rows)
# a: the recipe (rank 16 on the attention linears of every block, rank 64 on input_embed.proj, scale 2, text encoder replaced)
# b: block 0 only, ranks 1 / 8 / 24 / 128, scale 0.75 (not a power of two), no text encoder    -- overlaps a
# c: block 1 only, to_q / to_v at rank 8 and the text encoder                                    -- disjoint from b's pairs
ADAPTERS = {
    "a": (dict(seed=1), U.RECIPE),
    "b": (dict(seed=2, ranks={"to_q": 1, "to_k": 8, "to_v": 24, "to_out.0": 128}, in_rank=0, blocks=[0], scale=0.75, text=False),
          dict(lora_alpha=12, lora_r=16)),
    "c": (dict(seed=3, ranks=8, in_rank=0, blocks=[1], mods=("to_q", "to_v"), scale=2.0, text=True), dict(lora_alpha=32, lora_r=16)),
}
_cache = {}


def fixture(name):
    if name not in _cache:
        meta, a = load_golden(name)
        _cache[name] = (meta, a, synthetic_weights(meta))
    return _cache[name]


def adapter(name, which):
    meta, _, sd = fixture(name)
    kw, scales = ADAPTERS[which]
    return U.synth_adapter(sd, meta["arch"]["depth"], **kw), scales


def fresh(name, prec, which):
    """(out, traj) of a model without the option whose state dict was merged on the host by the contract's rule."""
    key = ("fresh", name, prec, which)
    if key not in _cache:
        meta, a, sd = fixture(name)
        if which is not None:
            t, scales = adapter(name, which)
            sd = A.merge_adapter(sd, t, rule="contract", **scales)
        out, traj = run_case(meta, a, build_cfm(meta, sd, prec))
        _cache[key] = (out.cpu(), traj.cpu())
    return _cache[key]


def resident(name, prec, which=("a", "b", "c")):
    meta, a, sd = fixture(name)
    model = build_cfm(meta, sd, prec)
    for w in which:
        t, scales = adapter(name, w)
        model.transformer.add_adapter(w, t, **scales)
    return meta, a, model


def same(got, want):
    return torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("which", ["a", "b"])
def test_switch_is_bit_exact_with_a_fresh_engine_on_the_host_merged_weights(name, prec, which):
    meta, a, model = resident(name, prec, which=(which,))
    model.transformer.set_adapter(which)
    want = fresh(name, prec, which)
    assert not same(want, fresh(name, prec, None)), "the adapter changes nothing: the test would be vacuous"
    for call in ("eager", "graph capture", "graph replay"):      # the same signature three times
        assert same(run_case(meta, a, model), want), f"{call}: differs from the fresh engine"
    assert model.transformer.engine().adapters


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("seq", [("a", "b"), ("b", "c")], ids=["overlapping", "disjoint"])
def test_switching_leaves_nothing_behind(name, prec, seq):
    x, y = seq
    meta, a, model = resident(name, prec)
    tr = model.transformer
    eng = None
    for step in (None, x, y, None, x):
        tr.set_adapter(step)
        got = run_case(meta, a, model)
        assert same(got, fresh(name, prec, step)), f"after switching to {step!r} in {(None, x, y, None, x)}"
        eng = eng or tr.engine()
        assert tr.engine() is eng, "a switch rebuilt the engine"
    # adding to a live engine and deleting do not rebuild it either
    t, scales = adapter(name, "b")
    tr.add_adapter("late", t, **scales)
    tr.set_adapter("late")
    assert same(run_case(meta, a, model), fresh(name, prec, "b")) and tr.engine() is eng
    tr.set_adapter(None)
    tr.delete_adapter("late")
    assert same(run_case(meta, a, model), fresh(name, prec, None)) and tr.engine() is eng


def test_first_adapter_on_a_live_engine_rebuilds_it_once():
    meta, a, sd = fixture("sample_b1_nfe16")
    model = build_cfm(meta, sd, "f16p")
    base = run_case(meta, a, model)
    e0 = model.transformer.engine()
    assert not e0.adapters and same(base, fresh("sample_b1_nfe16", "f16p", None))
    t, scales = adapter("sample_b1_nfe16", "a")
    model.transformer.add_adapter("a", t, **scales)
    model.transformer.set_adapter("a")
    assert same(run_case(meta, a, model), fresh("sample_b1_nfe16", "f16p", "a"))
    e1 = model.transformer.engine()
    assert e1 is not e0 and e1.adapters


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_reference_merge(name, prec, tmp_path):
    """The reference merges with torch's matmul and then runs (utils_infer.py:198-239): the oracle on
    convert_peft_state_dict_to_plain of the PEFT checkpoint, against load_adapter + set_adapter on the resident engine."""
    meta, a, sd = fixture(name)
    t, scales = adapter(name, "a")
    ck = U.peft_checkpoint(sd, t)
    plain = P.weights.strip_prefixes(I.convert_peft_state_dict_to_plain({k.replace("ema_model.", ""): v for k, v in ck.items()}))
    dur = meta["duration"]
    kw = dict(steps=meta["steps"], cfg_strength=meta["cfg_strength"], sway_sampling_coef=meta["sway"], seed=meta["seed"],
              use_epss=meta["use_epss"], no_ref_audio=meta["no_ref_audio"])
    if meta["lens"] is not None:
        kw["lens"] = torch.tensor(meta["lens"])
    key = ("oracle", name)
    if key not in _cache:
        dur = dur if isinstance(dur, int) else torch.tensor(dur)
        _cache[key] = (O.sample(plain, meta["arch"], a["cond"], a["text"], dur, **kw), O.sample(sd, meta["arch"], a["cond"], a["text"], dur, **kw))
    (o_out, o_traj), (_, base_traj) = _cache[key]
    tol = TOL_PARITY if prec in ("f32", "f16x3", "f16p") else TOL_16[prec]
    packed = bool(meta["arch"].get("attn_mask_enabled")) and o_traj.shape[1] > 1
    v = valid_frames(meta, a) if packed else torch.ones_like(o_traj[0, :, :, :1], dtype=torch.bool)   # (packed rows: test_sample_gpu.py)
    moved = ((o_traj - base_traj) * v).abs().max().item()      # the oracle with against without the adapter
    assert moved >= 10 * tol, f"the adapter moves the oracle's trajectory by {moved:.3e} only: parity would hide a failure"
    path = str(tmp_path / "ft.pt")
    torch.save({"ema_model_state_dict": ck}, path)
    model = build_cfm(meta, sd, prec)
    I.load_adapter(model, path, "ft", **scales)
    model.transformer.set_adapter("ft")
    out, traj = run_case(meta, a, model)
    e_out = ((out.cpu() - o_out) * v).abs().max().item()
    e_traj = ((traj.cpu() - o_traj) * v).abs().max().item()
    print(f"[adapter parity {prec}] {name}: out Linf {e_out:.3e} traj Linf {e_traj:.3e} (adapter moved the trajectory by {moved:.3e})")
    assert e_traj < tol and e_out < tol


# ------------------------------------------------------------------------------------------------ errors
def _arr(shape):
    return _lib.shape_array(shape), len(shape)


def test_errors_name_the_tensor_and_leave_the_engine_usable():
    meta, a, sd = fixture("sample_b1_nfe16")
    lib = _lib.load()
    err = lambda: lib.f5_last_error().decode()  # noqa: E731
    # an engine without the option bit
    plain = build_cfm(meta, sd, "f32")
    e0 = plain.transformer.engine()
    h = C.c_void_p()
    assert lib.f5_adapter_create(e0._h, C.byref(h)) == -3 and "F5_OPT_ADAPTERS" in err()
    assert lib.f5_set_adapter(e0._h, None, None) == -3 and "F5_OPT_ADAPTERS" in err()
    # an engine with it
    meta, a, model = resident("sample_b1_nfe16", "f32", which=("a",))
    tr = model.transformer
    eng = tr.engine()
    assert lib.f5_adapter_create(eng._h, C.byref(h)) == 0
    dev = eng.device
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    D, kin = 256, 264
    q = b"transformer_blocks.1.attn.to_q.weight"

    def put_lora(name, A_, B_, scale=1.0, a_shape=None, b_shape=None):
        return lib.f5_adapter_put_lora(h, name, C.c_void_p(A_.data_ptr()), *_arr(a_shape or A_.shape), C.c_void_p(B_.data_ptr()),
                                       *_arr(b_shape or B_.shape), scale, None)

    def put_tensor(name, t):
        return lib.f5_adapter_put_tensor(h, name, C.c_void_p(t.data_ptr()), *_arr(t.shape), None)

    assert put_lora(b"transformer_blocks.0.ff.ff.2.weight", z(4, 512), z(D, 4)) == -1 and "transformer_blocks.0.ff.ff.2.weight" in err()
    assert put_lora(b"transformer_blocks.9.attn.to_q.weight", z(4, D), z(D, 4)) == -1 and "transformer_blocks.9" in err()
    assert put_lora(b"text_embed.text_embed.weight", z(4, 64), z(41, 4)) == -1 and "text_embed.text_embed.weight" in err()
    assert put_lora(q, z(4, D + 4), z(D, 4)) == -1 and q.decode() in err()                   # A: wrong `in`
    assert put_lora(q, z(4, D), z(D + 1, 4)) == -1 and q.decode() in err()                   # B: wrong `out`
    assert put_lora(q, z(4, D), z(D, 5)) == -1 and q.decode() in err()                       # ranks disagree
    assert put_lora(q, z(4, D), z(D, 4), a_shape=(0, D), b_shape=(D, 0)) == -1 and "rank 0" in err() and q.decode() in err()
    assert put_lora(q, z(129, D), z(D, 129)) == -1 and "rank 129" in err() and q.decode() in err()
    assert put_lora(b"input_embed.proj.weight", z(128, kin), z(D, 128)) == 0                # the largest rank is fine
    assert put_tensor(b"proj_out.weight", z(100, D)) == -1 and "proj_out.weight" in err()
    assert put_tensor(q, z(D, D)) == -1 and q.decode() in err()                              # a LoRA target is not replaceable in full
    assert put_tensor(b"text_embed.text_embed.weight", z(40, 64)) == -1 and "text_embed.text_embed.weight" in err() and "41" in err()
    assert put_tensor(b"text_embed.text_blocks.0.dwconv.weight", z(64, 7)) == -1 and "dwconv.weight" in err()
    # destroying / changing the active adapter
    assert lib.f5_set_adapter(eng._h, h, None) == 0
    assert lib.f5_adapter_destroy(h) == -3 and "active" in err()
    assert put_lora(q, z(4, D), z(D, 4)) == -3 and "active" in err()
    assert lib.f5_set_adapter(eng._h, None, None) == 0
    assert lib.f5_adapter_destroy(h) == 0
    # ... and the engine still samples correctly: base, then a registered adapter
    assert same(run_case(meta, a, model), fresh("sample_b1_nfe16", "f32", None))
    tr.set_adapter("a")
    assert same(run_case(meta, a, model), fresh("sample_b1_nfe16", "f32", "a"))
    with pytest.raises(RuntimeError):
        tr.delete_adapter("a")
