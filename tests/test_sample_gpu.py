"""GPU parity proper: the HIP engine (through the Python drop-in surface -> ctypes -> libf5hip) against
  (1) the golden vectors produced by running the reference (tests/golden, oracle/make_golden.py), and
  (2) the CPU oracle on the same seeded inputs at mid sizes.
Tolerance: north_star's 1e-3 mel L-inf, asserted for the exact-f32 ("parity") precision; the 16-bit-operand speed
precisions (bf16, f16) are asserted at about twice their measured error (so that a 2x accuracy regression fails) and
the measured error is printed.  tests/test_configs_gpu.py repeats this at the sizes of BASELINE's configs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import f5_tts_amd as P  # noqa: E402
from conftest import load_golden, synthetic_weights  # noqa: E402
from oracle import f5_oracle as O  # noqa: E402

DEV = "cuda:0"
TOL_PARITY = 1e-3   # BASELINE.json north_star: "within 1e-3 mel L-inf"
# 16-bit MFMA operands through depth x NFE compounding, ~2x the measured trajectory L-inf (state magnitude ~5):
#   tiny fixtures: bf16 0.9e-2 .. 1.5e-2, f16 1.1e-3 .. 1.9e-3;   Base dims N=160 NFE=4: bf16 2.5e-2, f16 3e-3
TOL_16 = {"bf16": 3e-2, "f16": 4e-3}
TOL_16_BASE = {"bf16": 5e-2, "f16": 7e-3}
TOL_BF16 = TOL_16["bf16"]

CASES = ["sample_b1_nfe16", "sample_b3_masked", "sample_b3_attnmask", "sample_b1_editmask", "sample_b1_norefaudio",
         "sample_b2_v1arch", "sample_b1_nocfg_linspace", "sample_b1_textclamp", "sample_b1_duplicate", "sample_unett_b2",
         # qk_norm="rms_norm" + long_skip_connection + text_embedding_average_upsampling (dit.py:160-166), all heads / head 0 rotary
         "sample_b2_options", "sample_b1_options_pe1"]


def build_cfm(meta, sd, precision):
    cls = P.UNetT if meta.get("backbone", "DiT") == "UNetT" else P.DiT
    tr = cls(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision=precision)
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    return model


def run_case(meta, a, model):
    dur = meta["duration"]
    dur = dur if isinstance(dur, int) else torch.tensor(dur)
    kw = dict(steps=meta["steps"], cfg_strength=meta["cfg_strength"], sway_sampling_coef=meta["sway"], seed=meta["seed"],
              use_epss=meta["use_epss"], no_ref_audio=meta["no_ref_audio"])
    if meta["lens"] is not None:
        kw["lens"] = torch.tensor(meta["lens"])
    if "edit_mask" in a:
        kw["edit_mask"] = a["edit_mask"]
    if meta.get("duplicate_test"):
        kw.update(duplicate_test=True, t_inter=meta["t_inter"])
    return model.sample(a["cond"], a["text"], dur, **kw)


def valid_frames(meta, a):
    """[B, N, 1] mask of the frames inside each sample's own duration (all ones for a single utterance)."""
    dur = meta["duration"]
    N = a["traj"].shape[2]
    if isinstance(dur, int):
        return torch.ones(a["traj"].shape[1], N, 1, dtype=torch.bool)
    text_len = (a["text"] != -1).sum(-1)
    lens = torch.tensor(meta["lens"]) if meta["lens"] is not None else torch.full_like(text_len, a["cond"].shape[1])
    d = torch.maximum(torch.maximum(text_len, lens) + 1, torch.tensor(dur))      # cfm.py:125-131
    return (torch.arange(N)[None, :] < d[:, None])[..., None]


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16p"])     # the precisions held to the 1e-3 parity bar (f16x3: split-f16 products; f16p: f16 blocks + split-f16 I/O layers)
@pytest.mark.parametrize("name", CASES)
def test_sample_parity_f32_vs_reference_vectors(name, prec):
    meta, a = load_golden(name)
    sd = synthetic_weights(meta)
    model = build_cfm(meta, sd, prec)
    out, traj = run_case(meta, a, model)
    assert out.shape == a["out"].shape and traj.shape == a["traj"].shape
    packed = bool(meta["arch"].get("attn_mask_enabled")) and traj.shape[1] > 1
    # attn_mask_enabled batches run on the valid rows only (RowPack, csrc/engine_types.h): the frames past a sample's own
    # length -- which influence nothing in that configuration and which no caller reads -- keep their initial value
    # instead of the reference's drifted one; everything else is compared in full
    v = valid_frames(meta, a) if packed else torch.ones_like(a["traj"][0, :, :, :1], dtype=torch.bool)
    e_out = ((out.cpu() - a["out"]) * v).abs().max().item()
    e_traj = ((traj.cpu() - a["traj"]) * v).abs().max().item()
    print(f"[parity {prec}] {name}: out Linf {e_out:.3e} traj Linf {e_traj:.3e}" + (" (valid frames; packed rows)" if packed else ""))
    # f16p is the DiT's parity precision (AdaLN re-normalises every block's input); on UNetT the 4 .. 24 blocks' own f16 products
    # dominate and its parity precision is f16x3: f16p is held to f16's bound there (measured 1.1e-3)
    tol = TOL_16["f16"] if (prec == "f16p" and meta.get("backbone") == "UNetT") else TOL_PARITY
    assert e_traj < tol and e_out < tol
    if packed:
        pad = ~v.expand_as(traj[0].cpu())
        assert torch.equal(traj.cpu()[-1][pad], traj.cpu()[0][pad]), "frames past a sample's length keep their initial value"


def test_attn_mask_batch_unpacked_matches_reference_in_full(monkeypatch):
    """F5_PACK_ROWS=0: the attn_mask_enabled batch on padded rows reproduces the reference's trajectory everywhere,
    including the frames past each sample's length."""
    monkeypatch.setenv("F5_PACK_ROWS", "0")
    meta, a = load_golden("sample_b3_attnmask")
    sd = synthetic_weights(meta)
    out, traj = run_case(meta, a, build_cfm(meta, sd, "f32"))
    e = (traj.cpu() - a["traj"]).abs().max().item()
    print(f"[parity f32, unpacked] sample_b3_attnmask: traj Linf {e:.3e}")
    assert e < TOL_PARITY and (out.cpu() - a["out"]).abs().max() < TOL_PARITY


# F5_SPLIT_CFG=1 runs the two CFG halves as two concurrent stream chains, each in its own half of every work buffer
# (second_half, csrc/engine_impl.h; tests/test_work_plan.py holds the halves disjoint without a GPU).  f16p packs its input rows
# (acat) as f32 and long_skip_connection concatenates into cat2: the two buffers whose halves once overlapped.
@pytest.mark.parametrize("name,prec", [("sample_b1_nfe16", "f32"), ("sample_b1_nfe16", "f16p"), ("sample_b3_attnmask", "f16p"),
                                       ("sample_b2_options", "f32"), ("sample_b2_options", "f16p")])
def test_split_cfg_is_bit_equal(monkeypatch, name, prec):
    meta, a = load_golden(name)
    sd = synthetic_weights(meta)
    monkeypatch.setenv("F5_PACK_ROWS", "0")   # (split CFG steps padded rows; compare like with like)
    monkeypatch.setenv("F5_SPLIT_CFG", "0")
    base_out, base_traj = (t.cpu() for t in run_case(meta, a, build_cfm(meta, sd, prec)))
    monkeypatch.setenv("F5_SPLIT_CFG", "1")
    split = build_cfm(meta, sd, prec)
    for rep in range(3):   # eager, then captured, then replayed
        out, traj = (t.cpu() for t in run_case(meta, a, split))
        assert torch.equal(traj, base_traj) and torch.equal(out, base_out), f"{name} {prec}: F5_SPLIT_CFG=1 differs (run {rep})"


@pytest.mark.parametrize("prec", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["sample_b1_nfe16", "sample_b3_masked", "sample_b3_attnmask", "sample_unett_b2", "sample_b2_options"])
def test_sample_16bit_error_is_bounded_and_reported(name, prec):
    meta, a = load_golden(name)
    sd = synthetic_weights(meta)
    model = build_cfm(meta, sd, prec)
    out, traj = run_case(meta, a, model)
    v = valid_frames(meta, a) if meta["arch"].get("attn_mask_enabled") else True     # (packed rows: see the f32 test)
    e = ((traj.cpu() - a["traj"]) * v).abs().max().item()
    print(f"[{prec}] {name}: traj Linf {e:.3e} (state magnitude {a['traj'].abs().max().item():.2f})")
    assert torch.isfinite(out).all() and e < TOL_16[prec]


@pytest.mark.parametrize("name", ["dit_forward_taps", "dit_forward_taps_masked"])
def test_text_embed_and_forward_vs_reference_taps(name):
    meta, a = load_golden(name)
    sd = synthetic_weights(meta)
    tr = P.DiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    tr.to(DEV)
    eng = tr.engine()
    B, N = a["x"].shape[:2]
    mask = a.get("mask")
    lens = mask.sum(1).tolist() if mask is not None else None
    tc = eng.text_embed(a["text"], N, lens=lens, drop_text=False).cpu()
    tu = eng.text_embed(a["text"], N, lens=lens, drop_text=True).cpu()
    assert (tc - a["text_cond"]).abs().max() < 1e-4
    assert (tu - a["text_uncond"]).abs().max() < 1e-4
    out = tr(x=a["x"].to(DEV), cond=a["cond"].to(DEV), text=a["text"], time=a["time"],
             mask=None if mask is None else mask.to(DEV), cfg_infer=True).cpu()
    e = (out - a["out"]).abs().max().item()
    print(f"[forward f32] {name}: Linf {e:.3e}")
    assert e < 2e-4


def test_base_arch_sample_vs_oracle_mid_size():
    """F5-TTS Base dims, N=160, NFE=4: HIP f32 vs the CPU oracle on the same weights / noise (oracle finishes in seconds)."""
    arch = P.config.F5TTS_BASE
    nv = P.config.VOCAB_SIZE + 1
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, nv))
    g = torch.Generator().manual_seed(21)
    cond = torch.randn(1, 48, 100, generator=g)
    text = torch.randint(0, nv - 1, (1, 30), generator=g)
    kw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=5)
    o_out, o_traj = O.sample(sd, arch, cond, text, 160, **kw)
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    out, traj = model.sample(cond, text, 160, **kw)
    e = (traj.cpu() - o_traj).abs().max().item()
    print(f"[parity f32 base] traj Linf {e:.3e}")
    assert e < TOL_PARITY
    for prec in ("bf16", "f16"):
        tr16 = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision=prec)
        tr16.load_state_dict(sd)
        m16 = P.CFM(transformer=tr16, mel_spec_module=P.mel.MelSpec()).to(DEV)
        out16, traj16 = m16.sample(cond, text, 160, **kw)
        e16 = (traj16.cpu() - o_traj).abs().max().item()
        print(f"[{prec} base] traj Linf {e16:.3e}")
        assert e16 < TOL_16_BASE[prec]


@pytest.mark.parametrize("B,durs,refs,nts", [
    (1, [1], [1], [1]),            # degenerate: one frame (duration is raised to max(text, prompt) + 1 = 2)
    (1, [7], [3], [2]),            # shorter than the conv halo (15) and than one MFMA tile
    (1, [33], [9], [40]),          # text longer than the audio -> duration raised to 41 (cfm.py:125-131)
    (1, [65], [64], [5]),          # one frame past a 64-key attention tile; almost everything is prompt
    (2, [129, 17], [40, 16], [11, 3]),    # ragged batch across a 128-row GEMM tile edge, short item nearly all prompt
    (3, [200, 96, 1], [50, 95, 1], [20, 30, 1]),   # three lengths, one item degenerate
])
def test_ragged_and_edge_sizes_vs_oracle(B, durs, refs, nts):
    """Edge sizes the golden fixtures do not hold (the reference has no unit tests for these; the oracle, pinned on the
    fixtures, is the checker): tiny / odd N, N straddling kernel tile edges, text longer than audio, ragged batches."""
    meta, _ = load_golden("sample_b1_nfe16")
    arch, nv = meta["arch"], meta["nvocab"]
    sd = synthetic_weights(meta)
    g = torch.Generator().manual_seed(sum(durs) + 7 * B)
    rmax, tmax = max(refs), max(nts)
    cond = torch.zeros(B, rmax, 100)
    text = torch.full((B, tmax), -1, dtype=torch.long)
    for i in range(B):
        cond[i, :refs[i]] = torch.randn(refs[i], 100, generator=g)
        text[i, :nts[i]] = torch.randint(0, nv - 1, (nts[i],), generator=g)
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3, lens=torch.tensor(refs))
    dur = torch.tensor(durs)
    o_out, o_traj = O.sample(sd, arch, cond, text, dur, **kw)
    model = build_cfm(meta, sd, "f32")
    out, traj = model.sample(cond, text, dur, **kw)
    assert out.shape == o_out.shape and traj.shape == o_traj.shape
    e = (traj.cpu() - o_traj).abs().max().item()
    print(f"[edge sizes f32] B={B} durs={durs}: traj Linf {e:.3e}")
    assert e < TOL_PARITY and (out.cpu() - o_out).abs().max() < TOL_PARITY
    for prec in ("bf16", "f16"):
        m16 = build_cfm(meta, sd, prec)
        out16, traj16 = m16.sample(cond, text, dur, **kw)
        assert torch.isfinite(traj16).all() and (traj16.cpu() - o_traj).abs().max() < TOL_16[prec]


def test_chunked_batch_matches_reference_vectors(monkeypatch):
    """sample() steps large batches in utterance chunks (engine.hip::chunk_utts).  F5_CHUNK_ROWS forces one utterance
    per chunk on the three-utterance ragged fixture: the chunk-major length table, the per-chunk CFG halves and the
    per-chunk Euler update must reproduce the reference exactly as the unchunked path does."""
    monkeypatch.setenv("F5_CHUNK_ROWS", "150")   # 2 x 72 rows per utterance -> chunks of one
    for name in ("sample_b3_masked", "sample_b3_attnmask", "sample_b2_v1arch", "sample_unett_b2"):
        meta, a = load_golden(name)
        sd = synthetic_weights(meta)
        out, traj = run_case(meta, a, build_cfm(meta, sd, "f32"))
        v = valid_frames(meta, a) if meta["arch"].get("attn_mask_enabled") else True     # (packed rows: see the f32 test)
        e = ((traj.cpu() - a["traj"]) * v).abs().max().item()
        print(f"[chunked f32] {name}: traj Linf {e:.3e}")
        assert e < TOL_PARITY and ((out.cpu() - a["out"]) * v).abs().max() < TOL_PARITY


def test_uncond_text_cache_is_not_used_when_it_depends_on_the_text():
    """text_mask_padding=True (F5TTS_v1): the unconditional text embedding zeroes the rows whose ORIGINAL token is the
    filler (dit.py:90-91,104-108), so it depends on the call's text and must not be cached across sample() calls of equal N.
    Two B=1 calls at the same N with texts of different length: the second must match the oracle (it did not when the
    engine cached the first call's embedding)."""
    meta, _ = load_golden("sample_b2_v1arch")
    arch, nv = meta["arch"], meta["nvocab"]
    assert arch["text_mask_padding"]
    sd = synthetic_weights(meta)
    model = build_cfm(meta, sd, "f32")
    g = torch.Generator().manual_seed(77)
    cond = torch.randn(1, 20, 100, generator=g)
    kw = dict(steps=3, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=4)
    for nt in (30, 9, 30):
        text = torch.randint(0, nv - 1, (1, nt), generator=g)
        o_out, o_traj = O.sample(sd, arch, cond, text, 64, **kw)
        out, traj = model.sample(cond, text, 64, **kw)
        e = (traj.cpu() - o_traj).abs().max().item()
        print(f"[uncond cache, v1 arch] nt={nt}: traj Linf {e:.3e}")
        assert e < TOL_PARITY


def test_uncond_text_cache_and_graphs_survive_changes_of_length(monkeypatch):
    """The cached unconditional embedding lives in the arena next to every other pointer a captured sample() graph
    holds.  reserve() up front (as bench.py and a server do), then N = a, a, b (> a), a, a: the last call replays the
    first graph after the cache has been refilled for another N; it must equal an eager (F5_HIP_GRAPH=0) run bit for bit."""
    meta, a = load_golden("sample_b1_nfe16")
    arch, nv = meta["arch"], meta["nvocab"]
    sd = synthetic_weights(meta)
    kw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=2)
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(1, 24, 100, generator=g)
    text = torch.randint(0, nv - 1, (1, 12), generator=g)
    monkeypatch.setenv("F5_HIP_GRAPH", "0")
    eager = build_cfm(meta, sd, "f32")
    ref = {n: eager.sample(cond, text, n, **kw)[1].clone() for n in (64, 128)}
    monkeypatch.setenv("F5_HIP_GRAPH", "1")
    model = build_cfm(meta, sd, "f32")
    model.transformer.engine().reserve(1, 256, 8)
    for n in (64, 64, 128, 64, 64, 128, 128):
        traj = model.sample(cond, text, n, **kw)[1]
        assert torch.equal(traj, ref[n]), f"N={n}: graph / cache path differs from the eager run"


def test_full_size_properties():
    """BASELINE config C2 size (N=1024, NFE=16): size-independent properties instead of an oracle run."""
    arch = P.config.F5TTS_BASE
    nv = P.config.VOCAB_SIZE + 1
    tr = P.DiT(**arch, text_num_embeds=nv, mel_dim=100, precision="bf16").init_synthetic()
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    g = torch.Generator().manual_seed(1)
    cond = torch.randn(1, 256, 100, generator=g)
    text = torch.randint(0, nv - 1, (1, 150), generator=g)
    kw = dict(steps=16, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=0)
    out, traj = model.sample(cond, text, 1024, **kw)
    out2, traj2 = model.sample(cond, text, 1024, **kw)
    assert out.shape == (1, 1024, 100) and traj.shape == (17, 1, 1024, 100)
    assert torch.isfinite(traj).all()
    assert torch.equal(traj, traj2), "same seed -> bit-identical trajectory (deterministic kernels)"
    assert torch.equal(out[:, :256].cpu(), cond), "prompt frames are returned verbatim (cfm.py:221-223)"
    assert torch.equal(out[:, 256:], traj[-1][:, 256:])
    y0 = O.draw_noise(torch.tensor([1024]), 100, 0)
    assert torch.equal(traj[0].cpu(), y0), "trajectory starts at the reference's noise draw"
    # cfg_strength = 0 path runs one forward per step and differs from the guided result
    out0, _ = model.sample(cond, text, 1024, **dict(kw, cfg_strength=0.0))
    assert (out0 - out).abs().max() > 1e-3


def test_vocos_decode_vs_oracle():
    for cfg, T, B in ((P.config.VOCOS_TINY, 37, 2), (P.config.VOCOS_24K, 130, 1)):
        V = P.weights.synthetic_state_dict(P.weights.vocos_param_shapes(cfg), seed=3)
        mel = torch.randn(B, 100, T, generator=torch.Generator().manual_seed(T))
        ref = O.vocos_decode(V, mel)
        voc = P.Vocos(cfg)
        voc.load_state_dict(V)
        voc.to(DEV)
        wav = voc.decode(mel.to(DEV)).cpu()
        assert wav.shape == ref.shape
        e = (wav - ref).abs().max().item()
        print(f"[vocos f32] T={T}: wav Linf {e:.3e} (peak {ref.abs().max().item():.3f})")
        assert e < 2e-6 * max(1.0, ref.abs().max().item())      # measured 8.0e-7 (T = 130)


def test_mel_frontend_vs_oracle_and_wav_prompt():
    """wav -> log-mel (modules.py:78-146) on the HIP path vs the torch.stft restatement; then sample() with a raw-wave
    prompt (cfm.py:106-109) equals sample() with that mel."""
    g = torch.Generator().manual_seed(11)
    for nw in (24000, 12345):
        wav = torch.randn(2, nw, generator=g) * 0.1
        ref = O.mel_spectrogram_vocos(wav)
        ms = P.mel.MelSpec()
        got = ms(wav.to(DEV)).cpu()
        assert got.shape == ref.shape == (2, 100, nw // 256 + 1)
        e = (got - ref).abs().max().item()
        print(f"[mel front-end] nw={nw}: log-mel Linf {e:.3e}")
        assert e < 2e-3
    meta, a = load_golden("sample_b1_nfe16")
    sd = synthetic_weights(meta)
    tr = P.DiT(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100, precision="f32")
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr).to(DEV)
    wav = (torch.randn(1, 24 * 256 - 1, generator=g) * 0.1).to(DEV)   # -> 24 mel frames
    mel = model.mel_spec(wav).permute(0, 2, 1)
    kw = dict(steps=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=1)
    o1, _ = model.sample(wav, a["text"], 64, **kw)
    o2, _ = model.sample(mel, a["text"], 64, **kw)
    assert torch.equal(o1, o2)


def test_infer_process_end_to_end_vs_oracle():
    """wav prompt + text -> wav through the harness (infer.py) on the HIP path (mel front-end, sample(), Vocos) against
    the same pipeline assembled from oracle pieces on the CPU."""
    from f5_tts_amd import infer as I

    arch = P.config.F5TTS_TINY
    g = torch.Generator().manual_seed(5)
    tr = P.DiT(**arch, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
    model = P.CFM(transformer=tr).to(DEV)          # no vocab map -> utf-8 byte tokens (cfm.py:119-123)
    vsd = P.weights.synthetic_state_dict(P.weights.vocos_param_shapes(P.config.VOCOS_TINY), seed=4)
    voc = P.Vocos(P.config.VOCOS_TINY)
    voc.load_state_dict(vsd)
    voc.to(DEV)
    audio = torch.randn(1, 9000, generator=g) * 0.05
    ref_text, gen_text = "hello there.", "General Kenobi, you are a bold one."
    kw = dict(nfe_step=6, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    wave, sr, spec = next(I.infer_batch_process((audio, 24000), ref_text, [gen_text], model, voc, **kw))
    # oracle pipeline
    a, rms, rtext, ref_len, dur = I.prompt_numerics(audio, 24000, ref_text, gen_text)
    cond = O.mel_spectrogram_vocos(a).permute(0, 2, 1)
    text = P.utils.list_str_to_tensor([rtext + gen_text])
    out, _ = O.sample(tr.state_dict(), arch, cond, text, dur, steps=6, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    wref = O.vocos_decode(vsd, out[:, ref_len:].permute(0, 2, 1)) * (rms / 0.1 if rms < 0.1 else 1.0)
    assert sr == 24000 and wave.shape == (wref.shape[-1],)
    e_mel = float((torch.from_numpy(spec) - out[0, ref_len:].t()).abs().max())
    e_wav = float((torch.from_numpy(wave) - wref[0]).abs().max())
    print(f"[harness e2e f32] mel Linf {e_mel:.3e}, wav Linf {e_wav:.3e}")
    assert e_mel < 1e-3 and e_wav < 1e-3


def _real_prompt():
    """2 s (0.5 s .. 2.5 s) of the reference's bundled example prompt src/f5_tts/infer/examples/basic/basic_ref_en.wav
    (24 kHz mono PCM16; its transcript is in basic.toml), stored as tests/golden/prompt_basic_ref_en_2s.wav: real speech
    instead of white noise for the mel front-end (peaky spectrum, silence, 1e-5 clamp) and the harness numerics."""
    import os
    import wave

    import numpy as np
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_basic_ref_en_2s.wav")
    with wave.open(path) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16)
    return torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None]


def test_real_speech_prompt_mel_and_harness():
    from f5_tts_amd import infer as I

    audio = _real_prompt()
    ref = O.mel_spectrogram_vocos(audio)
    got = P.mel.MelSpec()(audio.to(DEV)).cpu()
    e = (got - ref).abs().max().item()
    print(f"[mel front-end, real speech] frames {ref.shape[-1]}, log-mel range [{ref.min():.2f}, {ref.max():.2f}], Linf {e:.3e}")
    assert got.shape == ref.shape and e < 2e-3
    # the example's texts (basic.toml), through the harness: duration formula, byte tokens, prompt slicing, RMS handling
    ref_text = "Some call me nature,"
    gen_text = "I don't really care what you call me."
    arch = P.config.F5TTS_TINY
    tr = P.DiT(**arch, text_num_embeds=257, mel_dim=100, precision="f32").init_synthetic(seed=2)
    model = P.CFM(transformer=tr).to(DEV)
    vsd = P.weights.synthetic_state_dict(P.weights.vocos_param_shapes(P.config.VOCOS_TINY), seed=4)
    voc = P.Vocos(P.config.VOCOS_TINY)
    voc.load_state_dict(vsd)
    voc.to(DEV)
    kw = dict(nfe_step=5, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    wave_out, sr, spec = next(I.infer_batch_process((audio, 24000), ref_text, [gen_text], model, voc, **kw))
    a, rms, rtext, ref_len, dur = I.prompt_numerics(audio, 24000, ref_text, gen_text)
    cond = O.mel_spectrogram_vocos(a).permute(0, 2, 1)
    text = P.utils.list_str_to_tensor([rtext + gen_text])
    out, _ = O.sample(tr.state_dict(), arch, cond, text, dur, steps=5, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
    wref = O.vocos_decode(vsd, out[:, ref_len:].permute(0, 2, 1)) * (rms / 0.1 if rms < 0.1 else 1.0)
    e_mel = float((torch.from_numpy(spec) - out[0, ref_len:].t()).abs().max())
    e_wav = float((torch.from_numpy(wave_out) - wref[0]).abs().max())
    print(f"[harness e2e f32, real prompt] rms {rms:.4f}, prompt {ref_len} frames, total {dur}; mel Linf {e_mel:.3e}, wav Linf {e_wav:.3e}")
    assert wave_out.shape == (wref.shape[-1],) and e_mel < 1e-3 and e_wav < 1e-3


@pytest.mark.parametrize("name,expect", [("sample_b1_nfe16", "f16p"), ("sample_unett_b2", "f16x3")])
def test_default_precision_is_parity_grade_for_the_backbone(name, expect):
    """A backbone built WITHOUT a precision argument ("parity") must land inside the 1e-3 bar of the reference vectors: DiT resolves
    to f16p, the E2-TTS UNetT (no AdaLN gates; every GEMM class costs ~1e-3 in plain fp16) to f16x3."""
    meta, a = load_golden(name)
    sd = synthetic_weights(meta)
    cls = P.UNetT if meta.get("backbone", "DiT") == "UNetT" else P.DiT
    tr = cls(**meta["arch"], text_num_embeds=meta["nvocab"], mel_dim=100)
    assert tr.precision == expect
    tr.load_state_dict(sd)
    out, traj = run_case(meta, a, P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV))
    e = (traj.cpu() - a["traj"]).abs().max().item()
    print(f"[default precision] {name}: {tr.precision}, traj Linf {e:.3e}")
    assert e < TOL_PARITY
