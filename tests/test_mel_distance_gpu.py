"""GPU: f5_mel_distance (csrc/dtw.hip) against the float64 restatement of its contract in dtw_oracle.py, then infer.heldout_distance
on a tiny synthetic DiT.

The gate is relative 2^-39: D is at most n + m - 1 < 2^13 f64 additions along the optimal path, each within 2^-53 relative, which
gives 2^-40; the gate doubles that to allow one ulp on each d should the device's f64 sqrt not be correctly rounded.  Bit equality
with the oracle is what is expected; every case prints its measured maximum (on an MI355X: 0 on all 54 pairs).  The shapes go around every size at which the kernel
takes another path: the wave (64), the workgroup's column count (metrics.DTW_THREADS: the strip goes from 1 to 2 columns), every
further strip width up to DTW_THREADS * DTW_MAX_STRIP = 4096 columns (the largest pair there is: one past it is refused, which the
CPU test holds), the row blocks of the streamed side (DTW_ROW_BLOCK) and its ring wrapping around, cepstra that do and do not fit
the workgroup's LDS (n_cep = 64 with 256 active threads; 1,500 columns at n_cep = 13), n >> m and m >> n."""
import ctypes as C

import numpy as np
import pytest
import torch

import adapter_util as U
import dtw_oracle as O
import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 2.0 ** -39
T, S, RB = M.DTW_THREADS, M.DTW_MAX_STRIP, M.DTW_ROW_BLOCK

# (n, m) per group; every group is ONE device call, (n_cep, n_mels) apart
GROUPS = {
    "edges": (13, 100, [(1, 1), (1, 7), (7, 1), (1, 4096), (4096, 1), (63, 63), (63, 64), (64, 64), (65, 64), (64, 65), (65, 65),
                        (2, 2), (3, 129)]),
    "workgroup_columns": (13, 100, [(300, T - 1), (300, T), (300, T + 1), (T + 1, 300), (T, T), (T + 1, T + 1), (T - 1, T + 1)]),
    "strips": (13, 100, [(2 * T, 2 * T + 9), (2 * T + 1, 2 * T + 1), (4 * T, 4 * T + 3), (4 * T + 1, 4 * T + 2), (8 * T, 8 * T + 1),
                         (8 * T + 1, 8 * T + 1)]),
    "largest_strip": (1, 100, [(S * T, S * T), (S * T - 1, S * T)]),
    "row_blocks": (13, 100, [(RB - 1, 5), (RB, 5), (RB + 1, 5), (2 * RB - 1, 9), (2 * RB, 9), (2 * RB + 1, 9), (3 * RB + 1, 20),
                             (700, 90), (90 + 2 * RB, 90), (90 + 2 * RB + 1, 90)]),
    "lopsided": (13, 100, [(3000, 40), (40, 3000), (4096, 1500)]),
    "one_coefficient": (1, 100, [(50, 70), (257, 256), (1, 1)]),
    "all_coefficients": (64, 100, [(300, T), (200, 100), (65, 64), (1, 5), (600, 300)]),
    "eighty_mels": (13, 80, [(50, 70), (257, 258), (7, 1)]),
    "eighty_mels_64": (64, 80, [(65, 64), (120, 300)]),
}


def fixture_pairs(shapes, n_mels, seed0=0):
    return [O.pair(seed0 + 31 * k + n + m, n, m, n_mels) for k, (n, m) in enumerate(shapes)]


def on_device(pairs):
    return [torch.from_numpy(a).to(DEV) for a, _ in pairs], [torch.from_numpy(b).to(DEV) for _, b in pairs]


def bits(t):
    return t.cpu().view(torch.int64).tolist()


@pytest.mark.parametrize("group", list(GROUPS))
def test_kernel_matches_the_oracle(group):
    n_cep, n_mels, shapes = GROUPS[group]
    pairs = fixture_pairs(shapes, n_mels)
    a, b = on_device(pairs)
    got = M.mel_distance(a, b, n_cep=n_cep).cpu().tolist()
    worst = 0.0
    for (n, m), (x, y), g in zip(shapes, pairs, got):
        want = O.value(x, y, n_cep)
        rel = abs(g - want) / want if want else abs(g)
        worst = max(worst, rel)
        print(f"{group}: ({n}, {m}) n_cep {n_cep} mels {n_mels}: device {g!r}, oracle {want!r}, relative {rel:.3e}")
        assert np.isfinite(g) and rel <= GATE, (group, n, m, g, want)
    print(f"{group}: measured maximum relative error {worst:.3e} (gate {GATE:.3e})")


NINE = [(40, 55), (1, 9), (300, 257), (64, 64), (520, 513), (7, 1), (90, 700), (33, 32), (128, 127)]


def test_ragged_batch_equals_each_pair_alone_in_any_order():
    a, b = on_device(fixture_pairs(NINE, 100, seed0=5))
    batch = bits(M.mel_distance(a, b))
    alone = [bits(M.mel_distance([x], [y]))[0] for x, y in zip(a, b)]
    assert batch == alone
    perm = [4, 8, 0, 6, 2, 7, 1, 5, 3]
    shuffled = bits(M.mel_distance([a[i] for i in perm], [b[i] for i in perm]))
    assert shuffled == [batch[i] for i in perm]


def test_value_is_bit_symmetric():
    a, b = on_device(fixture_pairs(NINE, 100, seed0=6))
    assert bits(M.mel_distance(a, b)) == bits(M.mel_distance(b, a))
    assert bits(M.mel_distance(a, a)) == [0] * len(a)            # +0.0 exactly


def test_reads_in_place_from_a_strided_tensor_with_nan_outside_the_ranges():
    pairs = fixture_pairs(NINE[:4], 100, seed0=7)
    a, b = on_device(pairs)
    want = bits(M.mel_distance(a, b))
    big = torch.full((4, 320, 128), float("nan"), device=DEV)    # [B, N, mel] of a wider buffer: row stride 128, NaN all around
    view = big[:, :, 14:114]
    starts = [3, 0, 17, 250]
    for k, x in enumerate(a):
        view[k, starts[k]:starts[k] + x.shape[0]] = x
    got = M.mel_distance([(view, k, starts[k], x.shape[0]) for k, x in enumerate(a)], b)
    assert torch.isfinite(got).all() and bits(got) == want
    # both sides from ONE buffer, the roles swapped
    got2 = M.mel_distance(b, [(view, k, starts[k], x.shape[0]) for k, x in enumerate(a)])
    assert bits(got2) == want


def test_a_nan_inside_one_pair_leaves_the_eight_others_alone():
    pairs = fixture_pairs(NINE, 100, seed0=8)
    a, b = on_device(pairs)
    clean = bits(M.mel_distance(a, b))
    for side, k, row in (("a", 4, 300), ("b", 2, 0), ("a", 6, 89)):
        a2, b2 = [t.clone() for t in a], [t.clone() for t in b]
        (a2 if side == "a" else b2)[k][row, 50] = float("nan")
        got = M.mel_distance(a2, b2).cpu()
        assert not np.isfinite(got[k].item())
        rest = bits(got)
        assert [v for i, v in enumerate(rest) if i != k] == [v for i, v in enumerate(clean) if i != k]
    a2 = [t.clone() for t in a]
    a2[1][0, 3] = float("inf")
    got = M.mel_distance(a2, b).cpu()
    assert not np.isfinite(got[1].item()) and [v for i, v in enumerate(bits(got)) if i != 1] == [v for i, v in enumerate(clean) if i != 1]


def raw_call(a, b, out_ptr, n_cep=13, n_mels=100, a_frames=None):
    """f5_mel_distance itself on contiguous device tensors, `out` wherever the test says (a_frames: other lengths than the tensors')."""
    base_a, base_b = min(t.data_ptr() for t in a), min(t.data_ptr() for t in b)
    i64 = lambda ts, base: (C.c_int64 * len(ts))(*[(t.data_ptr() - base) // 4 for t in ts])   # noqa: E731
    return _lib.load().f5_mel_distance(C.c_void_p(base_a), C.c_void_p(base_b), len(a), i64(a, base_a), _lib.int_array(a_frames or [t.shape[0] for t in a]),
                                       n_mels, i64(b, base_b), _lib.int_array([t.shape[0] for t in b]), n_mels, n_mels, n_cep,
                                       C.c_void_p(out_ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_guard_words_stay_intact_and_refused_calls_write_nothing():
    a, b = on_device(fixture_pairs(NINE, 100, seed0=9))
    want = bits(M.mel_distance(a, b))
    sentinel = 0x7FF8A5A5A5A5A5A5                                 # a NaN with a payload
    raw = torch.full((8 + len(a) + 8,), sentinel, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        assert raw_call(a, b, raw.data_ptr() + 64) == 0
        torch.cuda.synchronize()
        host = raw.cpu().tolist()
        assert host[:8] == [sentinel] * 8 and host[-8:] == [sentinel] * 8 and host[8:-8] == want
        raw.fill_(sentinel)
        assert raw_call(a, b, raw.data_ptr() + 64, n_cep=0) == -1 and "n_cep" in _lib.load().f5_last_error().decode()
        assert raw_call(a, b, raw.data_ptr() + 64, n_cep=100) == -1
        assert raw_call(a, b, raw.data_ptr() + 64, a_frames=[40, 0] + [t.shape[0] for t in a[2:]]) == -1 and "pair 1 has a_frames = 0" in _lib.load().f5_last_error().decode()
        torch.cuda.synchronize()
    assert raw.cpu().tolist() == [sentinel] * raw.numel()


# ---------------------------------------------------------------------------------------------------- the driver
ADAPTERS = {"a": (dict(seed=1), U.RECIPE), "b": (dict(seed=2, ranks=8, in_rank=0, blocks=[1], mods=("to_q", "to_v"), scale=2.0, text=True),
                                                  dict(lora_alpha=32, lora_r=16))}
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
PROMPT, TARGET = (20, 24, 18), (38, 42, 56)     # totals 58, 66, 74: one bucket of bucket_prompts, so ONE ragged batch of B = 3


def tiny(prec="f16p", adapters=True):
    arch = dict(P.config.F5TTS_TINY)
    sd = P.weights.synthetic_state_dict(P.weights.dit_param_shapes(arch, 40), seed=0)
    tr = P.DiT(**arch, text_num_embeds=40, mel_dim=100, precision=prec)
    tr.load_state_dict(sd)
    model = P.CFM(transformer=tr, mel_spec_module=P.mel.MelSpec()).to(DEV)
    if adapters:
        for name, (kw, scales) in ADAPTERS.items():
            tr.add_adapter(name, U.synth_adapter(sd, arch["depth"], **kw), **scales)
    return model


def heldout_items():
    g = torch.Generator().manual_seed(21)
    items = []
    for k, (p, t) in enumerate(zip(PROMPT, TARGET)):
        whole = torch.from_numpy(O.random_walk_mel(40 + k, p + t))
        items.append((whole[:p].clone(), torch.randint(0, 40, (5 + k,), generator=g), whole[p:].clone(),
                      torch.randint(0, 40, (7 + 2 * k,), generator=g)))
    return items


def sample_alone(model, items, adapter):
    """What heldout_distance asks of sample() for the one batch of `items`, done by hand: (out on the host, ends)."""
    pad = torch.nn.utils.rnn.pad_sequence
    cond = pad([it[0] for it in items], batch_first=True).to(DEV)
    text = pad([torch.cat([it[1], it[3]]) for it in items], padding_value=-1, batch_first=True)
    lens = torch.tensor([it[0].shape[0] for it in items])
    total = torch.tensor([it[0].shape[0] + it[2].shape[0] for it in items])
    model.transformer.set_adapter(adapter)
    out, _ = model.sample(cond, text, total, lens=lens, steps=KW["nfe_step"], cfg_strength=KW["cfg_strength"],
                          sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
    return out.cpu(), P.cfm.clamp_durations(text, lens, total).tolist()


def test_heldout_distance_scores_what_sample_generates():
    model, items = tiny(), heldout_items()
    assert P.infer.heldout_distance_plan(items)[3] == [[0, 1, 2]]
    model.transformer.set_adapter("b")
    got = P.infer.heldout_distance(model, items, adapters=(None, "a", "b"), **KW)
    assert model.transformer.active_adapter == "b"             # restored
    for name in (None, "a", "b"):
        out, ends = sample_alone(model, items, name)
        num = den = 0.0
        for u, (it, end) in enumerate(zip(items, ends)):
            p, g = it[0].shape[0], it[2].shape[0]
            want = O.value(out[u, p:end].numpy(), it[2].numpy())
            have = got[name]["per_item"][u]
            print(f"adapter {name} item {u}: heldout_distance {have!r}, oracle on sample()'s output {want!r}")
            assert want > 0 and abs(have - want) <= GATE * want
            num, den = num + have * (end - p + g), den + (end - p + g)
        assert abs(got[name]["mcd"] - num / den) <= 1e-12 * num / den
    model.transformer.set_adapter("b")
    assert got["a"]["per_item"] != got[None]["per_item"] and got["b"]["per_item"] != got[None]["per_item"]
    assert got["a"]["mcd"] != got["b"]["mcd"], "two fine-tunes, one number"
    # the restore holds on an exception too
    with pytest.raises(Exception):
        P.infer.heldout_distance(model, items, adapters=("a", "no such adapter"), **KW)
    assert model.transformer.active_adapter == "b"


def test_the_models_own_output_as_target_scores_exactly_zero():
    model, items = tiny(adapters=False), heldout_items()
    out, ends = sample_alone(model, items, None)
    own = [(it[0], it[1], out[u, it[0].shape[0]:ends[u]].clone(), it[3]) for u, it in enumerate(items)]
    assert [o[2].shape[0] for o in own] == list(TARGET)
    got = P.infer.heldout_distance(model, own, **KW)[None]
    assert got["per_item"] == [0.0, 0.0, 0.0] and got["mcd"] == 0.0


@pytest.mark.parametrize("prec", ["f16p", "f8"])
def test_heldout_distance_runs_at_both_precisions_without_extra_eager_bodies(prec):
    model, items = tiny(prec, adapters=False), heldout_items()
    first = P.infer.heldout_distance(model, items, **KW)[None]      # (captures whatever sample() captures)
    tr = model.transformer
    tr.graph_stats(reset=True)
    sample_alone(model, items, None)
    alone = tr.graph_stats(reset=True)
    again = P.infer.heldout_distance(model, items, **KW)[None]
    scored = tr.graph_stats(reset=True)
    print(f"{prec}: mcd {again['mcd']:.6f} dB, sample() alone {alone}, under heldout_distance {scored}")
    assert np.isfinite(again["mcd"]) and again["mcd"] > 0 and again == first
    assert scored["eager"] <= alone["eager"] and sum(scored.values()) == sum(alone.values())


def test_isolated_rows_make_a_score_independent_of_the_batch():
    model, items = tiny(adapters=False), heldout_items()
    model.transformer.set_isolated_rows(True)
    together = P.infer.heldout_distance(model, items, **KW)[None]["per_item"]
    alone = [P.infer.heldout_distance(model, [it], **KW)[None]["per_item"][0] for it in items]
    assert together == alone
