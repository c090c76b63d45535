"""GPU: CFM.sample with the midpoint ODE solver (odeint_kwargs=dict(method="midpoint")) against the reference-generated
midpoint fixtures (tools/make_golden_ode.py) and the in-repo oracle run with the test-side midpoint solver
(tests/ode_oracle.py), plus the engine invariances (graph replay, chunking, split CFG, method switches on one engine)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import f5_tts_amd as P  # noqa: E402
import ode_oracle as OO  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from f5_tts_amd import _lib  # noqa: E402
from f5_tts_amd.engine import _h2d_async, _ptr, _stream_ptr  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

DEV = "cuda:0"
TOL_PARITY = 1e-3
# 16-bit operands: ~2x the largest trajectory L-inf measured on these fixtures (MI355X): bf16 1.4e-2, f16 1.9e-3
TOL_16 = {"bf16": 3e-2, "f16": 4e-3}
FIXTURES = ["sample_b1_midpoint", "sample_b3_midpoint_attnmask", "sample_b1_midpoint_nocfg", "sample_unett_b2_midpoint"]


def fixture(name):
    meta, a = load_golden(name)
    assert meta["method"] == "midpoint"
    return meta, a, OO.scaled_time_mlp(synthetic_weights(meta), meta["time_mlp_scale"])


def build_cfm(meta, sd, precision, method="midpoint"):
    cls = P.UNetT if meta.get("backbone", "DiT") == "UNetT" else P.DiT
    tr = cls(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision=precision)
    tr.load_state_dict(sd)
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method=method)).to(DEV)


def run_case(meta, a, model):
    dur = meta["duration"]
    dur = dur if isinstance(dur, int) else torch.tensor(dur)
    kw = dict(steps=meta["steps"], cfg_strength=meta["cfg_strength"], sway_sampling_coef=meta["sway"], seed=meta["seed"],
              use_epss=meta["use_epss"], no_ref_audio=meta["no_ref_audio"])
    if meta["lens"] is not None:
        kw["lens"] = torch.tensor(meta["lens"])
    if meta.get("duplicate_test"):
        kw.update(duplicate_test=True, t_inter=meta["t_inter"])
    out, traj = model.sample(a["cond"], a["text"], dur, **kw)
    return out.cpu(), traj.cpu()


def valid_frames(meta, a):
    """[B, N, 1] frames inside each sample's own duration (the rule of test_sample_gpu.py)."""
    dur = meta["duration"]
    N = a["traj"].shape[2]
    if isinstance(dur, int):
        return torch.ones(a["traj"].shape[1], N, 1, dtype=torch.bool)
    text_len = (a["text"] != -1).sum(-1)
    lens = torch.tensor(meta["lens"]) if meta["lens"] is not None else torch.full_like(text_len, a["cond"].shape[1])
    d = torch.maximum(torch.maximum(text_len, lens) + 1, torch.tensor(dur))
    return (torch.arange(N)[None, :] < d[:, None])[..., None]


def packed(meta, a):
    return bool(meta["arch"].get("attn_mask_enabled")) and a["traj"].shape[1] > 1


def errors(meta, a, out, traj):
    v = valid_frames(meta, a) if packed(meta, a) else True
    return ((out - a["out"]) * v).abs().max().item(), ((traj - a["traj"]) * v).abs().max().item()


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16p"])
@pytest.mark.parametrize("name", FIXTURES)
def test_midpoint_parity_vs_reference_vectors(name, prec):
    meta, a, sd = fixture(name)
    out, traj = run_case(meta, a, build_cfm(meta, sd, prec))
    assert out.shape == a["out"].shape and traj.shape == a["traj"].shape
    e_out, e_traj = errors(meta, a, out, traj)
    print(f"[midpoint {prec}] {name}: out Linf {e_out:.3e} traj Linf {e_traj:.3e}" + (" (valid frames)" if packed(meta, a) else ""))
    # (as in test_sample_gpu.py: f16p is the DiT's parity precision; on UNetT it is held to f16's bound)
    tol = TOL_16["f16"] if (prec == "f16p" and meta.get("backbone") == "UNetT") else TOL_PARITY
    assert e_traj < tol and e_out < tol
    if packed(meta, a):
        pad = ~valid_frames(meta, a).expand_as(traj[0])
        assert pad.any()
        for k in range(1, traj.shape[0]):
            assert torch.equal(traj[k][pad], traj[0][pad]), "frames past a sample's length keep their initial value"


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_midpoint_16bit_error_is_bounded_and_reported(name, prec):
    meta, a, sd = fixture(name)
    out, traj = run_case(meta, a, build_cfm(meta, sd, prec))
    e_out, e_traj = errors(meta, a, out, traj)
    print(f"[midpoint {prec}] {name}: traj Linf {e_traj:.3e} (state magnitude {a['traj'].abs().max().item():.2f})")
    assert torch.isfinite(out).all() and e_traj < TOL_16[prec]


def test_midpoint_attn_mask_batch_unpacked_matches_reference_in_full(monkeypatch):
    """F5_PACK_ROWS=0: the padded-row path reproduces the reference's whole trajectory, frames past each length included."""
    monkeypatch.setenv("F5_PACK_ROWS", "0")
    meta, a, sd = fixture("sample_b3_midpoint_attnmask")
    out, traj = run_case(meta, a, build_cfm(meta, sd, "f32"))
    e = (traj - a["traj"]).abs().max().item()
    print(f"[midpoint f32, unpacked] sample_b3_midpoint_attnmask: traj Linf {e:.3e}")
    assert e < TOL_PARITY and (out - a["out"]).abs().max() < TOL_PARITY


def test_midpoint_base_arch_vs_oracle_mid_size():
    """F5-TTS Base dims, N=160, 4 midpoint steps (8 evaluations): HIP f32 vs the CPU oracle with the midpoint solver."""
    arch = P.config.F5TTS_BASE
    nv = P.config.VOCAB_SIZE + 1
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv))
    g = torch.Generator().manual_seed(21)
    cond = torch.randn(1, 48, 100, generator=g)
    text = torch.randint(0, nv - 1, (1, 30), generator=g)
    kw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=5)
    with OO.solver("midpoint"):
        o_out, o_traj = O.sample(sd, arch, cond, text, 160, **kw)
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method="midpoint")).to(DEV)
    out, traj = model.sample(cond, text, 160, **kw)
    e = (traj.cpu() - o_traj).abs().max().item()
    print(f"[midpoint f32 base] traj Linf {e:.3e}")
    assert traj.shape[0] == 5 and e < TOL_PARITY


# ------------------------------------------------------------------------------------------------ engine invariances (f32)
def test_midpoint_graph_replay_is_bit_equal_to_eager(monkeypatch):
    meta, a, sd = fixture("sample_b3_midpoint_attnmask")
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    eager = run_case(meta, a, build_cfm(meta, sd, "f32"))
    monkeypatch.setenv("F5_HIP_GRAPH", "1")
    model = build_cfm(meta, sd, "f32")
    runs = [run_case(meta, a, model) for _ in range(3)]   # eager, capture + launch, replay
    for k, (out, traj) in enumerate(runs):
        assert torch.equal(traj, eager[1]) and torch.equal(out, eager[0]), f"call {k + 1} differs from F5_HIP_GRAPH=0"


def test_midpoint_chunked_batch_matches_reference_vectors(monkeypatch):
    monkeypatch.setenv("F5_CHUNK_ROWS", "1")   # one utterance per chunk
    for name in ("sample_b3_midpoint_attnmask", "sample_unett_b2_midpoint"):
        meta, a, sd = fixture(name)
        out, traj = run_case(meta, a, build_cfm(meta, sd, "f32"))
        e_out, e_traj = errors(meta, a, out, traj)
        print(f"[midpoint f32, chunked] {name}: traj Linf {e_traj:.3e}")
        assert e_traj < TOL_PARITY and e_out < TOL_PARITY


def split_cfg_is_bit_equal(monkeypatch, prec):
    for name in ("sample_b1_midpoint", "sample_b3_midpoint_attnmask"):
        meta, a, sd = fixture(name)
        monkeypatch.setenv("F5_PACK_ROWS", "0")   # (split CFG steps padded rows; compare like with like)
        monkeypatch.setenv("F5_SPLIT_CFG", "0")
        base = run_case(meta, a, build_cfm(meta, sd, prec))
        monkeypatch.setenv("F5_SPLIT_CFG", "1")
        split = build_cfm(meta, sd, prec)
        for _ in range(3):
            out, traj = run_case(meta, a, split)
            assert torch.equal(traj, base[1]) and torch.equal(out, base[0]), f"{name} {prec}: F5_SPLIT_CFG=1 differs"


def test_midpoint_split_cfg_is_bit_equal(monkeypatch):
    split_cfg_is_bit_equal(monkeypatch, "f32")


def test_midpoint_split_cfg_is_bit_equal_f16p(monkeypatch):
    """f16p packs its input rows as f32: the side chain's half of that buffer starts behind the main chain's f32 rows."""
    split_cfg_is_bit_equal(monkeypatch, "f16p")


def test_one_engine_alternating_methods_keeps_euler_bit_identical():
    """Euler -> midpoint -> Euler ... on one engine at one shape: the graph key and the arena plan keep the methods apart."""
    meta, a, sd = fixture("sample_b1_midpoint")
    model = build_cfm(meta, sd, "f32", method="euler")
    res = {"euler": [], "midpoint": []}
    for method in ("euler", "midpoint") * 3:
        model.odeint_kwargs = dict(method=method)
        res[method].append(run_case(meta, a, model))
    for method, runs in res.items():
        for out, traj in runs[1:]:
            assert torch.equal(traj, runs[0][1]) and torch.equal(out, runs[0][0]), method
    assert not torch.equal(res["euler"][0][1], res["midpoint"][0][1])
    assert (res["midpoint"][0][1] - a["traj"]).abs().max() < TOL_PARITY


def test_f5_sample_equals_f5_sample_ode_euler(monkeypatch):
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    meta, a, sd = fixture("sample_b3_midpoint_attnmask")
    model = build_cfm(meta, sd, "f32", method="euler")
    eng = model.transformer.engine()
    B, N = a["out"].shape[:2]
    g = torch.Generator().manual_seed(8)
    y0 = torch.randn(B, N, 100, generator=g)
    lens = [44, 27, 35]
    cond_mask = torch.arange(N)[None, :] < torch.tensor(meta["lens"])[:, None]
    t = O.time_grid(5, -1.0, True).tolist()
    out_ode, traj_ode = eng.sample(a["cond"], cond_mask, y0, a["text"], t, 2.0, lens=lens, method="euler")
    # the same call through the original entry point
    dev = eng.device
    cond = _h2d_async(a["cond"], dev, torch.float32)
    y0d = _h2d_async(y0, dev, torch.float32)
    cm = _h2d_async(cond_mask, dev, torch.uint8)
    text = _h2d_async(a["text"], dev, torch.long)
    out = torch.empty(B, N, 100, device=dev)
    traj = torch.empty(len(t), B, N, 100, device=dev)
    with torch.cuda.device(dev):
        _lib.check(eng.lib.f5_sample(eng._h, _ptr(cond), cond.shape[1], _ptr(cm), _ptr(y0d), _ptr(text), text.shape[1],
                                     _lib.float_array(t), len(t) - 1, C.c_float(2.0), _lib.int_array(lens), B, N, _ptr(out),
                                     _ptr(traj), _stream_ptr(dev)), "f5_sample")
    assert torch.equal(out.cpu(), out_ode.cpu()) and torch.equal(traj.cpu(), traj_ode.cpu())
    with pytest.raises(ValueError):
        eng.sample(a["cond"], cond_mask, y0, a["text"], t, 2.0, lens=lens, method="rk4")


def test_load_model_and_dp_sample_with_midpoint():
    """infer.load_model(ode_method="midpoint") and dist.dp_sample need no change of their own: a world-1 job over a
    ragged pair matches the oracle's midpoint solve of the same batch."""
    from f5_tts_amd import dist as D
    from f5_tts_amd import infer as I
    arch = P.config.F5TTS_TINY
    model = I.load_model(P.DiT, arch, None, ode_method="midpoint", device=DEV, precision="f32")
    nv = model.transformer.text_num_embeds
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv), seed=3)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(12)
    conds = [torch.randn(20, 100, generator=g), torch.randn(14, 100, generator=g)]
    texts = [torch.randint(0, nv - 1, (11,), generator=g), torch.randint(0, nv - 1, (8,), generator=g)]
    durs = [48, 37]
    kw = dict(steps=6, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=4)
    mels, lens = D.dp_sample(model, conds, texts, durs, **kw)
    cond = torch.nn.utils.rnn.pad_sequence(conds, batch_first=True)
    text = torch.nn.utils.rnn.pad_sequence(texts, batch_first=True, padding_value=-1)
    with OO.solver("midpoint"):
        o_out, _ = O.sample(sd, arch, cond, text, torch.tensor(durs), lens=torch.tensor([20, 14]), **kw)
    v = (torch.arange(48)[None, :] < torch.tensor(durs)[:, None])[..., None]
    e = ((mels.cpu() - o_out) * v).abs().max().item()
    print(f"[midpoint f32, dp_sample world 1] out Linf {e:.3e}")
    assert lens == durs and e < TOL_PARITY
