"""GPU: f5_cep_moments and f5_gauss_divergence (csrc/speaker.hip) against the ordered float64 oracle of their contract in
speaker_oracle.py, then infer.heldout_speaker on a tiny synthetic DiT.

Bit equality with the ordered oracle is what is asserted: every sum the contract orders is summed by one thread in that order,
everything else is single IEEE f64 operations (the device's f64 division and square root are correctly rounded), and the DCT table is
built on the host by the expression the contract states.  Every case prints how many values it compared (on an MI355X: every
value of every case equal, measured maximum difference 0).  The shapes go around every
size at which the kernels take another path: one frame, fewer frames than the delta window (every clamp case at 1, 2 and 5 frames),
one chunk less one, one chunk, one chunk and one, two chunks and one (metrics.MOM_CHUNK), the smallest and a usual mel count, one
coefficient, the usual 13 and the most (32; with deltas C = 64, the largest record there is)."""
import math

import numpy as np
import pytest
import torch

import adapter_util as U
import speaker_oracle as O
import f5_tts_amd as P
from f5_tts_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = M.MOM_CHUNK
FRAMES = (1, 2, 5, K - 1, K, K + 1, 2 * K + 1)


def mel(seed, frames, n_mels=100):
    rng = np.random.default_rng(seed)
    if n_mels != 100:
        return (rng.normal(size=(frames, n_mels)) * 2.0 - 5.0).astype(np.float32)
    return O.synthetic_utterance(rng, O.synthetic_speaker(rng), frames)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_bits(got, want):
    """Bit equality of two f64 arrays; NaN matches NaN (whatever its payload)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def check_records(tag, got: M.Moments, want):
    count, mean, scatter = got.count.cpu().tolist(), got.mean.cpu().numpy(), got.scatter.cpu().numpy()
    compared = 0
    for s, (n, m, sc) in enumerate(want):
        assert count[s] == n, (tag, s, count[s], n)
        assert same_bits(mean[s], m), (tag, s, "mean", np.abs(mean[s] - m).max())
        assert same_bits(scatter[s], sc), (tag, s, "scatter", np.abs(scatter[s] - sc).max())
        compared += len(m) + len(sc)
    print(f"{tag}: {len(want)} records, {compared} values bit-equal to the ordered oracle")


# ---------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("n_mels,n_cep,deltas", [(100, 1, False), (100, 1, True), (100, 13, False), (100, 13, True), (100, 32, False),
                                                 (100, 32, True), (2, 1, False), (2, 1, True)])
def test_moments_match_the_ordered_oracle(n_mels, n_cep, deltas):
    """Every frame count of FRAMES as the segments of ONE call.  (n_mels = 2 admits n_cep = 1 alone: n_cep <= n_mels - 1.)"""
    xs = [mel(100 * n_cep + f, f, n_mels) for f in FRAMES]
    got = M.cepstral_moments([torch.from_numpy(x).to(DEV) for x in xs], n_cep=n_cep, deltas=deltas)
    assert got.dim == n_cep * (2 if deltas else 1) and len(got) == len(FRAMES)
    check_records(f"mels {n_mels} n_cep {n_cep} deltas {deltas}", got, [O.moments(x, n_cep, deltas) for x in xs])


def test_moments_read_the_segments_where_they_lie():
    """A row stride above n_mels with non-zero starts; in-place entries of a [B, N, mel] tensor; host tensors (packed once)."""
    wide = torch.from_numpy(np.random.default_rng(1).normal(size=(300, 120)).astype(np.float32) - 4.0).to(DEV)
    cuts = [(7, 70), (100, 101), (150, 290)]
    views = [wide[a:b, 11:111] for a, b in cuts]
    assert views[0].stride(0) == 120 and views[0].storage_offset() > 0
    want = [O.moments(v.cpu().numpy(), 13, True) for v in views]
    check_records("stride 120", M.cepstral_moments(views, n_cep=13, deltas=True), want)
    check_records("host tensors", M.cepstral_moments([v.cpu() for v in views], n_cep=13, deltas=True), want)
    cube = torch.from_numpy(np.random.default_rng(2).normal(size=(3, 150, 100)).astype(np.float32) - 4.0).to(DEV)
    entries = [(cube, 2, 10, 131), (cube, 0, 0, 150), (cube, 1, 149, 1)]
    want = [O.moments(cube[b, s:s + f].cpu().numpy(), 13, False) for _, b, s, f in entries]
    check_records("in place", M.cepstral_moments(entries, n_cep=13), want)


@pytest.mark.parametrize("S", [1, 70])
def test_a_record_does_not_depend_on_its_batch(S):
    frames = [1 + (37 * s) % 90 for s in range(S)]
    xs = [mel(500 + s, f) for s, f in enumerate(frames)]
    got = M.cepstral_moments([torch.from_numpy(x).to(DEV) for x in xs], n_cep=13, deltas=True)
    check_records(f"S = {S}", got, [O.moments(x, 13, True) for x in xs])


def test_selection_by_mask_and_gate():
    """Masks: none, all, alternating, a chunk with nothing selected between two that have frames, nothing at all; the gate alone and
    with a mask; the mask is one entry per frame of the call, segment after segment."""
    F = 3 * K
    x = mel(9, F)
    hole = np.ones(F, dtype=bool)
    hole[K:2 * K] = False
    masks = [np.ones(F, dtype=bool), np.arange(F) % 2 == 0, hole, np.zeros(F, dtype=bool)]
    dev = [torch.from_numpy(x).to(DEV)] * len(masks)
    got = M.cepstral_moments(dev, n_cep=13, deltas=True, select=torch.from_numpy(np.concatenate(masks)))
    want = [O.moments(x, 13, True, mask=m) for m in masks]
    assert [w[0] for w in want] == [F, F // 2, 2 * K, 0]
    check_records("masks", got, want)
    none = M.cepstral_moments(dev[:1], n_cep=13, deltas=True)
    assert torch.equal(none.scatter[0], got.scatter[0]) and torch.equal(none.mean[0], got.mean[0])    # all == none
    assert got.count[3].item() == 0 and not got.mean[3].any() and not got.scatter[3].any()           # nothing selected: zeros
    both = torch.from_numpy(np.concatenate([masks[0], masks[1]]))
    y = mel(10, 2 * K + 7)
    pair = [dev[0], torch.from_numpy(y).to(DEV)]
    for gate_db in (0.0, 1.5, 6.0, 200.0):
        gs = M.gate_sum_of(gate_db, 100)
        for deltas in (False, True):
            # the gate alone: no mask at all (what a caller who only sets gate_db runs), two segments with their own loudest frames
            alone = M.cepstral_moments(pair, n_cep=13, deltas=deltas, gate_db=gate_db)
            want = [O.moments(x, 13, deltas, gate_sum=gs), O.moments(y, 13, deltas, gate_sum=gs)]
            print(f"gate {gate_db} dB alone, deltas {deltas}: {want[0][0]} of {F} and {want[1][0]} of {y.shape[0]} frames pass")
            check_records(f"gate {gate_db} dB alone, deltas {deltas}", alone, want)
            # the gate together with a mask
            got = M.cepstral_moments(dev[:2], n_cep=13, deltas=deltas, select=both, gate_db=gate_db)
            want = [O.moments(x, 13, deltas, mask=masks[0], gate_sum=gs), O.moments(x, 13, deltas, mask=masks[1], gate_sum=gs)]
            print(f"gate {gate_db} dB with masks, deltas {deltas}: {want[0][0]} of {F} frames pass, {want[1][0]} with the alternating mask")
            check_records(f"gate {gate_db} dB with masks, deltas {deltas}", got, want)
    counts = [M.cepstral_moments(pair[:1], n_cep=13, gate_db=g).count.item() for g in (0.0, 1.5, 6.0, 200.0)]
    assert 1 <= counts[0] <= counts[1] <= counts[2] <= counts[3] == F and counts[0] < F, counts   # the gate bites, on the device
    on_device = M.cepstral_moments(pair, n_cep=13, select=torch.ones(F + y.shape[0], dtype=torch.uint8, device=DEV), gate_db=6.0)
    alone = M.cepstral_moments(pair, n_cep=13, gate_db=6.0)
    assert torch.equal(on_device.count, alone.count) and torch.equal(on_device.scatter, alone.scatter)   # a device mask, in place


def test_the_cepstra_are_mel_distances():
    """c_k is f5_mel_distance's cepstrum: the same table and the same sum order, restated in speaker.hip.  Tied together on the
    device: a one-frame segment's mean is its cepstral vector exactly (0 + c, divided by 1), and a one-frame pair against a frame
    of zeros (whose cepstra are exactly 0) has the distance D(0, 0) / 2 = d(0, 0) = (10 / ln 10) sqrt(2 sum_k c_k^2), k ascending --
    so the moments' cepstra, put through that expression on the host, must give mel_distance's bits, for every n_cep (each one
    adds one coefficient to the sum) and for 80 mel bins as well as 100."""
    scale = 4.3429448190325175
    for n_mels in (100, 80):
        rng = np.random.default_rng(n_mels)
        frames = [torch.from_numpy((rng.normal(size=(1, n_mels)) * 2.0 - 5.0).astype(np.float32)).to(DEV) for _ in range(6)]
        zeros = [torch.zeros(1, n_mels, device=DEV)] * len(frames)
        for n_cep in (1, 2, 3, 5, 13, 32):
            c = M.cepstral_moments(frames, n_cep=n_cep).mean.cpu().numpy()
            dist = M.mel_distance(frames, zeros, n_cep=n_cep).cpu().numpy()
            want = []
            for row in c:
                acc = 0.0
                for k in range(n_cep):
                    diff = row[k] - 0.0
                    acc = acc + diff * diff
                want.append(scale * math.sqrt(2.0 * acc))
            assert same_bits(dist, np.array(want)), (n_mels, n_cep, dist.tolist(), want)
    print("6 frames x 6 coefficient counts x 2 mel counts: the moments' cepstra reproduce mel_distance's bits")


def test_a_non_finite_frame_reaches_its_own_segment_alone():
    xs = [mel(60 + s, f) for s, f in enumerate((70, 130, 5, 66))]
    clean = M.cepstral_moments([torch.from_numpy(x).to(DEV) for x in xs], n_cep=13, deltas=True)
    for value, seg, t in ((np.nan, 1, 64), (np.inf, 1, 0), (-np.inf, 2, 4), (np.nan, 0, 69)):
        dirty = [x.copy() for x in xs]
        dirty[seg][t, 17] = value
        got = M.cepstral_moments([torch.from_numpy(x).to(DEV) for x in dirty], n_cep=13, deltas=True)
        assert got.count.cpu().tolist() == [-1 if s == seg else xs[s].shape[0] for s in range(4)]
        assert torch.isnan(got.mean[seg]).all() and torch.isnan(got.scatter[seg]).all()
        for s in range(4):
            if s != seg:
                assert torch.equal(got.mean[s], clean.mean[s]) and torch.equal(got.scatter[s], clean.scatter[s])
    check_records("non-finite", got, [O.moments(x, 13, True) for x in dirty])


# ---------------------------------------------------------------------------------------------------- divergence
def to_device(records, n_cep, deltas):
    return M.Moments(torch.tensor([r[0] for r in records], dtype=torch.int32, device=DEV),
                     torch.tensor(np.stack([r[1] for r in records]), device=DEV),
                     torch.tensor(np.stack([r[2] for r in records]), device=DEV), n_cep, deltas)


@pytest.mark.parametrize("n_cep,deltas", [(1, False), (1, True), (13, False), (13, True), (32, True)])
def test_divergence_matches_the_ordered_oracle(n_cep, deltas):
    """C in {1, 2, 13, 26, 64}.  Records 0 .. 2 are sound; 3 has count == C (too few frames); 4 has a duplicated feature (a
    covariance that is exactly singular: its second pivot is 0 or negative); the singular pairs sit between sound ones."""
    Cd = n_cep * (2 if deltas else 1)
    recs = [O.moments(mel(700 + k, 150 + 40 * k), n_cep, deltas) for k in range(3)]
    few = O.moments(mel(710, Cd), n_cep, deltas)
    assert few[0] == Cd
    n, m, sc = recs[0]
    S = O.unpack(sc, Cd)
    if Cd > 1:                                      # feature 1 := feature 0, with a variance of exactly 4 (its root and the quotient
        S[:, 1], S[1, :] = S[:, 0].copy(), S[0, :].copy()   # 4 / 2 are exact), so that the second pivot is exactly 0
        S[:2, :2] = 4.0 * n
    else:
        S[0, 0] = 0.0
    dup = (n, m, S[O.triu(Cd)])
    recs += [few, dup]
    pairs = [(0, 1), (0, 3), (1, 0), (4, 2), (2, 2), (3, 3), (1, 2), (2, 4), (0, 0)]
    rec = to_device(recs, n_cep, deltas)
    terms, status = M.gaussian_divergence(rec, rec, pairs)
    terms, status = terms.cpu().numpy(), status.cpu().tolist()
    want = [O.divergence(recs[i], recs[j]) for i, j in pairs]
    assert status == [w[1] for w in want] == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    for p, (w, _) in enumerate(want):
        assert same_bits(terms[p], w), (Cd, pairs[p], terms[p].tolist(), w)
    assert terms[4].tolist() == [Cd, Cd, 0.0, 0.0] and terms[8].tolist() == [Cd, Cd, 0.0, 0.0]      # (a, a)
    assert same_bits(terms[0], terms[2][[1, 0, 3, 2]])                                             # (a, b) and (b, a), swapped
    kl = M.speaker_numbers(terms, Cd)
    assert kl["kl"][4] == 0.0 and kl["sphericity"][4] == 0.0 and kl["kl"][0] == kl["kl"][2] and kl["kl"][0] > 0
    assert math.isnan(kl["kl"][1]) and math.isnan(kl["sphericity"][3])
    print(f"C = {Cd}: {4 * len(pairs)} terms bit-equal to the ordered oracle; kl(0, 1) = {kl['kl'][0]!r}")
    # pairs = None is record s against record s; two different sets of records
    other = to_device(recs[1:4], n_cep, deltas)
    terms2, status2 = M.gaussian_divergence(to_device(recs[:3], n_cep, deltas), other)
    assert status2.cpu().tolist() == [0, 0, 1] and same_bits(terms2[0].cpu().numpy(), want[0][0])


def test_device_moments_feed_the_divergence():
    """The two stages chained on the device: moments of two speakers' utterances, pooled, then compared."""
    rng = np.random.default_rng(5)
    A, B = O.synthetic_speaker(rng), O.synthetic_speaker(rng)
    xs = [O.synthetic_utterance(rng, s, f) for s, f in ((A, 90), (A, 150), (B, 120), (A, 200))]
    rec = M.cepstral_moments([torch.from_numpy(x).to(DEV) for x in xs], n_cep=13)
    pooled, labels = M.merge_moments(rec, ["a", "a", "b", "a2"])
    assert labels == ["a", "b", "a2"] and pooled.count.cpu().tolist() == [240, 120, 200]
    terms, status = M.gaussian_divergence(pooled, pooled, [(0, 2), (0, 1)])
    assert status.cpu().tolist() == [0, 0]
    nums = M.speaker_numbers(terms.cpu(), 13)
    assert 0 < nums["kl"][0] < nums["kl"][1] and 0 < nums["sphericity"][0] < nums["sphericity"][1]
    whole = O.moments(np.concatenate(xs[:2]), 13)
    assert np.allclose(pooled.scatter[0].cpu().numpy(), whole[2], rtol=1e-11, atol=1e-11 * np.abs(whole[2]).max())


# ---------------------------------------------------------------------------------------------------- the driver
ADAPTERS = {"a": (dict(seed=1), U.RECIPE), "b": (dict(seed=2, ranks=8, in_rank=0, blocks=[1], mods=("to_q", "to_v"), scale=2.0, text=True),
                                                  dict(lora_alpha=32, lora_r=16))}
KW = dict(nfe_step=4, cfg_strength=2.0, sway_sampling_coef=-1.0, seed=3)
SPK = dict(n_cep=5, deltas=True)
PROMPT, TARGET = (20, 24, 18), (38, 42, 56)     # totals 58, 66, 74: one bucket under the default budget, so ONE ragged batch of B = 3
SPEAKERS = ["x", "y", "x"]


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
        whole = torch.from_numpy(mel(40 + k, p + t))
        items.append((whole[:p].clone(), torch.randint(0, 40, (5 + k,), generator=g), whole[p:].clone(),
                      torch.randint(0, 40, (7 + 2 * k,), generator=g)))
    return items


def by_hand(model, items, adapter):
    """heldout_speaker's three metrics calls for the one batch of `items`, composed by hand."""
    pad = torch.nn.utils.rnn.pad_sequence
    cond = pad([it[0] for it in items], batch_first=True).to(DEV)
    text = pad([torch.cat([it[1], it[3]]) for it in items], padding_value=-1, batch_first=True)
    lens = torch.tensor([it[0].shape[0] for it in items])
    total = torch.tensor([it[0].shape[0] + it[2].shape[0] for it in items])
    model.transformer.set_adapter(adapter)
    out, _ = model.sample(cond, text, total, lens=lens, steps=KW["nfe_step"], cfg_strength=KW["cfg_strength"],
                          sway_sampling_coef=KW["sway_sampling_coef"], seed=KW["seed"])
    ends = P.cfm.clamp_durations(text, lens, total).tolist()
    B = len(items)
    ref = M.cepstral_moments([it[0].to(DEV) for it in items] + [it[2].to(DEV) for it in items], **SPK)
    gen = M.cepstral_moments([out[b, it[0].shape[0]:ends[b]].contiguous() for b, it in enumerate(items)], **SPK)
    item_terms, item_status = M.gaussian_divergence(gen, ref, [(b, b) for b in range(B)] + [(b, B + b) for b in range(B)])
    pg, labels = M.merge_moments(gen, SPEAKERS)
    pooled = {}
    for part, side in enumerate(("to_prompt", "to_target")):
        half = M.Moments(ref.count[part * B:(part + 1) * B], ref.mean[part * B:(part + 1) * B], ref.scatter[part * B:(part + 1) * B],
                         ref.n_cep, ref.deltas)
        pooled[side] = M.gaussian_divergence(pg, M.merge_moments(half, SPEAKERS)[0])
    return item_terms.cpu(), item_status.cpu().tolist(), pooled, labels


def test_heldout_speaker_is_the_hand_composition_bit_for_bit():
    model, items = tiny(), heldout_items()
    Cd = 10
    model.transformer.set_adapter("b")
    before = P.infer.heldout_distance(model, items, adapters=(None, "a"), **KW)
    got = P.infer.heldout_speaker(model, items, adapters=(None, "a", "b"), speakers=SPEAKERS, **SPK, **KW)
    assert model.transformer.active_adapter == "b"             # restored
    for name in (None, "a", "b"):
        terms, status, pooled, labels = by_hand(model, items, name)
        assert labels == ["x", "y"] and status == [0] * 6 and got[name]["singular"] == 0
        nums = M.speaker_numbers(terms, Cd)
        for u in range(3):
            for k, side in enumerate(("to_prompt", "to_target")):
                want = dict(kl=nums["kl"][3 * k + u], sphericity=nums["sphericity"][3 * k + u])
                print(f"adapter {name} item {u} {side}: {got[name]['per_item'][u][side]} (by hand {want})")
                assert got[name]["per_item"][u][side] == want and want["kl"] > 0
        for side in ("to_prompt", "to_target"):
            pn = M.speaker_numbers(pooled[side][0].cpu(), Cd)
            for k, label in enumerate(labels):
                assert got[name]["per_speaker"][label][side] == dict(kl=pn["kl"][k], sphericity=pn["sphericity"][k])
            assert got[name][side] == {key: math.fsum(pn[key]) / 2 for key in ("kl", "sphericity")}
    model.transformer.set_adapter("b")
    assert got["a"]["per_item"] != got[None]["per_item"] and got["a"]["to_prompt"] != got["b"]["to_prompt"]
    only = P.infer.heldout_speaker(model, items, adapters=("a",), speakers=SPEAKERS, against=("target",), **SPK, **KW)["a"]
    assert "to_prompt" not in only and only["to_target"] == got["a"]["to_target"]
    # the restore holds on an exception too, and the sibling's numbers on the same items have not moved
    with pytest.raises(KeyError, match="no adapter 'no such adapter'"):
        P.infer.heldout_speaker(model, items, adapters=("a", "no such adapter"), **SPK, **KW)
    assert model.transformer.active_adapter == "b"
    assert P.infer.heldout_distance(model, items, adapters=(None, "a"), **KW) == before


def test_isolated_rows_make_per_item_independent_of_batch_frames_and_singular_items_are_counted():
    model, items = tiny(adapters=False), heldout_items()
    model.transformer.set_isolated_rows(True)
    frames_per_batch = 50                           # below every item's total: every item closes a batch of its own
    assert len(P.infer.heldout_distance_plan(items)[3]) == 1
    assert len(P.infer.heldout_distance_plan(items, batch_frames=frames_per_batch)[3]) == 3
    together = P.infer.heldout_speaker(model, items, speakers=SPEAKERS, **SPK, **KW)[None]
    apart = P.infer.heldout_speaker(model, items, speakers=SPEAKERS, batch_frames=frames_per_batch, **SPK, **KW)[None]
    assert together["per_item"] == apart["per_item"] and together["singular"] == 0
    assert all(np.isfinite(v) for it in together["per_item"] for side in it.values() for v in side.values())
    # at C = 26 the 18 to 24 prompt frames are too few for a covariance: to_prompt is NaN for every item and speaker "y" (24 frames),
    # while speaker "x" pools 38 prompt frames and stands
    wide = P.infer.heldout_speaker(model, items, speakers=SPEAKERS, n_cep=13, deltas=True, **KW)[None]
    assert wide["singular"] == 3 and all(math.isnan(it["to_prompt"]["kl"]) for it in wide["per_item"])
    assert all(np.isfinite(it["to_target"]["kl"]) for it in wide["per_item"])
    assert math.isnan(wide["per_speaker"]["y"]["to_prompt"]["kl"]) and np.isfinite(wide["per_speaker"]["x"]["to_prompt"]["kl"])
    assert wide["to_prompt"]["kl"] == wide["per_speaker"]["x"]["to_prompt"]["kl"]
