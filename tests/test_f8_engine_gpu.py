"""GPU: the engine under precision "f8" (F5_PREC_F8).

  G4  the bit identities the engine advertises, which per-row and per-channel dynamic scales keep: graph replay == eager, a
      length-bucketed call == the exact call, isolated rows (an item in a batch == the item alone), sample_items uniform == sample(),
      a chain of sample_span slices == the unsliced solve; and f8 differs from f16p (the path is on);
  G5  the engine against its contract: tests/f8_oracle.py's emulation of the header's rounding points, within a quarter of the
      emulation's own distance from the f32 oracle;
  G6  f5_flow_loss under f8 against the same emulation, and infer.heldout_loss.
F5TTS_TINY, synthetic weights at std 0.02, NFE 4.  Every test prints its figures before it asserts.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import f8_oracle as Q  # noqa: E402
import flow_oracle as FO  # noqa: E402
import f5_tts_amd as P  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

DEV = "cuda:0"
NV = 40
ARCH = P.config.F5TTS_TINY
KW = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
_cache = {}


def weights():
    if "sd" not in _cache:
        _cache["sd"] = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(ARCH, NV), seed=0, std=0.02)
    return _cache["sd"]


def model(prec="f8", *, bucket=0, isolated=False, arch=None):
    tr = P.DiT(**dict(ARCH, **(arch or {})), text_num_embeds=NV, mel_dim=100, precision=prec)
    tr.load_state_dict(weights())
    if bucket:
        tr.set_length_buckets(bucket)
    if isolated:
        tr.set_isolated_rows(True)
    return P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)


def inputs(refs, nts, seed=5):
    g = torch.Generator().manual_seed(seed)
    cond = torch.zeros(len(refs), max(refs), 100)
    text = torch.full((len(refs), max(nts)), -1, dtype=torch.long)
    for i, (r, n) in enumerate(zip(refs, nts)):
        cond[i, :r] = torch.randn(r, 100, generator=g)
        text[i, :n] = torch.randint(1, NV - 2, (n,), generator=g)
    return cond, text


# =========================================================================================================== G4
def test_g4_replay_equals_eager_and_f8_is_on(monkeypatch):
    cond, text = inputs([24], [11])
    m = model()
    first = m.sample(cond, text, 70, **KW)
    again = m.sample(cond, text, 70, **KW)          # the captured graph, replayed
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    eager = model().sample(cond, text, 70, **KW)
    monkeypatch.delenv("F5_HIP_GRAPH")
    for a, b, c in zip(first, again, eager):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b) and torch.equal(a, c)
    p16 = model("f16p").sample(cond, text, 70, **KW)
    d = (p16[1] - first[1]).abs().max().item()
    print(f"[f8 vs f16p, tiny] traj Linf {d:.3e}")
    assert d > 0, "f8 computes what f16p computes: the e4m3 path is not on"


def test_g4_bucketed_call_equals_exact_call():
    cond, text = inputs([24, 20], [11, 9])
    durs, lens = torch.tensor([70, 45]), torch.tensor([24, 20])
    exact = model().sample(cond, text, durs, lens=lens, **KW)
    bucketed = model(bucket=32).sample(cond, text, durs, lens=lens, **KW)
    for b, n in enumerate(durs.tolist()):
        assert torch.equal(exact[0][b, :n], bucketed[0][b, :n]) and torch.equal(exact[1][:, b, :n], bucketed[1][:, b, :n])
    one = model().sample(cond[:1], text[:1], 70, **KW)
    one_b = model(bucket=32).sample(cond[:1], text[:1], 70, **KW)
    assert torch.equal(one[0], one_b[0]) and torch.equal(one[1], one_b[1])


def test_g4_isolated_rows_items_and_spans():
    refs, nts, durs = [24, 20], [11, 9], [70, 45]
    cond, text = inputs(refs, nts)
    iso = model(isolated=True)
    alone = []
    for b in range(2):
        alone.append(iso.sample_items(cond[b:b + 1, :refs[b]], text[b:b + 1, :nts[b]], durs[b], **KW))
    for order in ([0, 1], [1, 0]):
        c, t = inputs([refs[i] for i in order], [nts[i] for i in order])
        for j, i in enumerate(order):       # the same items, in this row order
            c[j], t[j] = 0, -1
            c[j, :refs[i]], t[j, :nts[i]] = cond[i, :refs[i]], text[i, :nts[i]]
        out, traj = iso.sample_items(c, t, torch.tensor([durs[i] for i in order]), lens=torch.tensor([refs[i] for i in order]), **KW)
        for j, i in enumerate(order):
            n = durs[i]
            assert torch.equal(out[j, :n], alone[i][0][0, :n]), (order, i)
            assert torch.equal(traj[:, j, :n], alone[i][1][:, 0, :n]), (order, i)
    # sample_items with one setting for every item == sample()
    plain = model()
    d, ln = torch.tensor(durs), torch.tensor(refs)
    s_out, s_traj = plain.sample(cond, text, d, lens=ln, **KW)
    i_out, i_traj = plain.sample_items(cond, text, d, lens=ln, **KW)
    for b, n in enumerate(durs):
        assert torch.equal(s_out[b, :n], i_out[b, :n]) and torch.equal(s_traj[:, b, :n], i_traj[:, b, :n])
    # a chain of two slices == the unsliced solve
    r1 = plain.sample_span(cond, text, d, lens=ln, start=[0, 0], count=2, **KW)
    r2 = plain.sample_span(cond, text, d, lens=ln, start=[2, 2], count=2, prev=(r1.state, [0, 1]), **KW)
    assert all(r2.done)
    for b, n in enumerate(durs):
        assert torch.equal(r2.out[b, :n], i_out[b, :n]), b


def test_g4_options_run_under_f8():
    """midpoint, qk_norm, long_skip and cfg < 1e-5 take the same four GEMMs: finite, and replay == first call."""
    cond, text = inputs([24], [11])
    sd = dict(weights())
    arch = dict(ARCH, qk_norm="rms_norm", long_skip_connection=True)
    sd.update(P.weights.synthetic_state_dict({k: v for k, v in P.weights.dit_param_shapes(arch, NV).items() if k not in sd}, seed=0, std=0.02))
    tr = P.DiT(**arch, text_num_embeds=NV, mel_dim=100, precision="f8")
    tr.load_state_dict(sd)
    m = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec(), odeint_kwargs=dict(method="midpoint")).to(DEV)
    a = m.sample(cond, text, 70, **KW)
    b = m.sample(cond, text, 70, **KW)
    assert torch.isfinite(a[1]).all() and torch.equal(a[1], b[1])
    c = m.sample(cond, text, 70, **dict(KW, cfg_strength=0.0))
    assert torch.isfinite(c[1]).all() and not torch.equal(a[1], c[1])


# =========================================================================================================== G5
def test_g5_engine_against_its_contract():
    """D_e = max |emulation - f32 oracle| on the CPU; the engine must stay within 0.25 D_e of the emulation (measured on the CPU when
    the bound was set: roundings of f16 size move the emulation by 0.04 D_e, leaving out every f16 rounding before the quantisers
    by 0.15 D_e, another scale rule by 1.1 D_e)."""
    refs, nts = [40, 31], [14, 11]
    cond, text = inputs(refs, nts, seed=9)
    durs, lens = torch.tensor([96, 77]), torch.tensor(refs)
    with torch.no_grad():
        _, o_traj = O.sample(weights(), ARCH, cond, text, durs, lens=lens, **KW)
        with Q.f8_blocks():
            _, e_traj = O.sample(weights(), ARCH, cond, text, durs, lens=lens, **KW)
    valid = O.lens_to_mask(durs, 96)[None, ..., None]
    D_e = ((e_traj - o_traj) * valid).abs().max().item()
    _, traj = model().sample(cond, text, durs, lens=lens, **KW)
    assert torch.isfinite(traj).all()
    d = ((traj.cpu() - e_traj) * valid).abs().max().item()
    d16 = ((model("f16p").sample(cond, text, durs, lens=lens, **KW)[1].cpu() - o_traj) * valid).abs().max().item()
    print(f"[G5] D_e = {D_e:.3e}; engine f8 - emulation = {d:.3e} = {d / D_e:.3f} D_e; engine f8 - f32 oracle = "
          f"{((traj.cpu() - o_traj) * valid).abs().max().item():.3e}; engine f16p - f32 oracle = {d16:.3e}")
    assert d <= 0.25 * D_e


# =========================================================================================================== G6
def flow_case():
    g = torch.Generator().manual_seed(21)
    lens = [64, 51]
    mel = torch.zeros(2, 64, 100)
    for b, n in enumerate(lens):
        mel[b, :n] = torch.randn(n, 100, generator=g)
    x0 = torch.randn(2, 64, 100, generator=g)
    text = torch.full((2, 12), -1, dtype=torch.long)
    text[0, :12] = torch.randint(1, NV - 2, (12,), generator=g)
    text[1, :9] = torch.randint(1, NV - 2, (9,), generator=g)
    return mel, x0, text, lens, [0.35, 0.8], [(10, 50), (5, 44)]


def test_g6_flow_loss_against_the_emulation():
    mel, x0, text, lens, time, span = flow_case()
    with torch.no_grad():
        ref = FO.flow_loss("DiT", weights(), ARCH, mel, x0, text, time, span, lens)
        with Q.f8_blocks():
            emu = FO.flow_loss("DiT", weights(), ARCH, mel, x0, text, time, span, lens)
    m = model()
    loss, per_item, pred, _, _ = m.flow_loss(mel.to(DEV), text, torch.tensor(lens), time=time, span=span, x0=x0.to(DEV))
    assert torch.isfinite(pred).all() and torch.isfinite(per_item).all()
    valid = O.lens_to_mask(torch.tensor(lens), 64)[..., None]
    D_p = ((emu["pred"] - ref["pred"]) * valid).abs().max().item()
    d_p = ((pred.cpu().double() - emu["pred"]) * valid).abs().max().item()
    D_l = (emu["per_item"] - ref["per_item"]).abs().max().item()
    d_l = (per_item.cpu().double() - emu["per_item"]).abs().max().item()
    print(f"[G6] pred: D = {D_p:.3e}, engine - emulation = {d_p:.3e} = {d_p / D_p:.3f} D; per-item loss: D = {D_l:.3e}, engine - emulation = "
          f"{d_l:.3e} = {d_l / D_l:.3f} D (loss {loss.item():.6f}, emulation {emu['loss'].item():.6f}, f32 oracle {ref['loss'].item():.6f})")
    assert d_p <= 0.25 * D_p
    assert d_l <= 0.25 * D_l


def test_g6_heldout_loss_runs():
    g = torch.Generator().manual_seed(3)
    mels = [torch.randn(n, 100, generator=g) for n in (48, 37, 60)]
    texts = [torch.randint(1, NV - 2, (n,), generator=g).tolist() for n in (9, 7, 11)]
    r8 = P.infer.heldout_loss(model(), mels, texts, times=2)[None]
    r16 = P.infer.heldout_loss(model("f16p"), mels, texts, times=2)[None]
    print(f"[heldout] f8 {r8['loss']:.6f}, f16p {r16['loss']:.6f}")
    assert all(torch.isfinite(torch.tensor(r8[k])).all() for k in ("loss", "per_item", "per_time"))
