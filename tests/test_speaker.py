"""CPU: the Gaussian cepstral divergence (include/f5_hip.h "speaker similarity", csrc/speaker.hip, metrics.py) without a GPU -- the
entry points are declared, exported and bound; every refusal names its argument and happens before anything is launched; the plan
arithmetic; the ordered oracle (speaker_oracle.py, loops in the contract's order) against the plain one (np.cov, np.linalg) within
a gate derived from the condition number of the covariances; merge_moments over a split against the moments of the concatenation;
the identities of the measure in the oracle; and a discrimination property on synthetic log-mels (a sanity condition on the measure,
not a claim about real voices)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import speaker_oracle as O
from conftest import ROOT

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import metrics as M

FAKE = C.c_void_p(0x1000)                   # a device pointer that no refusal may dereference
EPS = 2.0 ** -52


def i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def err():
    return _lib.load().f5_last_error().decode()


# ---------------------------------------------------------------------------------------------------- ABI
def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    for name in ("f5_cep_moments_plan", "f5_cep_moments", "f5_gauss_divergence"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("Moments", "cepstral_moments", "merge_moments", "gaussian_divergence", "speaker_numbers"):
        assert hasattr(M, name), name
    assert callable(P.infer.heldout_speaker)


def test_the_chunk_is_named_once_everywhere():
    header = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    src = open(os.path.join(ROOT, "korean-f5-tts_amd", "csrc", "speaker.hip")).read()
    assert re.search(rf"#define F5_MOM_CHUNK {M.MOM_CHUNK}\b", header)
    assert re.search(rf"constexpr int kMomChunk = {M.MOM_CHUNK};", src) and "kMomChunk == F5_MOM_CHUNK" in src
    assert re.search(rf"constexpr int kMaxDim = {M.MOM_MAX_DIM};", src)
    assert O.MOM_CHUNK == M.MOM_CHUNK == 64 and M.MOM_MAX_DIM == 2 * M.MOM_MAX_CEP
    # the contract comes before the kernels: the header states the order of every sum
    for phrase in ("chunk ascending", "t ascending", "Centred sums, never raw second moments", "k = c .. r - 1 ascending"):
        assert phrase in header, phrase


# ---------------------------------------------------------------------------------------------------- refusals
def moments_call(S=2, base=FAKE, start=(0, 700), frames=(7, 5), stride=100, n_mels=100, n_cep=13, deltas=0, mask=None, gate=-1.0,
                 count=FAKE, mean=FAKE, scatter=FAKE):
    arr = lambda v, f: None if v is None else f(list(v))   # noqa: E731
    return _lib.load().f5_cep_moments(base, S, arr(start, i64), arr(frames, _lib.int_array), stride, n_mels, n_cep, deltas, mask,
                                      gate, count, mean, scatter, None)


MOMENT_REFUSALS = [
    (dict(base=None), "null base"), (dict(start=None), "start_host"), (dict(frames=None), "frames_host"),
    (dict(count=None), "null count"), (dict(mean=None), "null mean"), (dict(scatter=None), "null scatter"),
    (dict(S=0), "S = 0"), (dict(S=65536), "S = 65536"), (dict(S=-1), "S = -1"),
    (dict(frames=(0, 5)), "segment 0 has frames = 0"), (dict(frames=(7, 4097)), "segment 1 has frames = 4097"),
    (dict(frames=(-3, 5)), "segment 0 has frames = -3"),
    (dict(n_mels=1, n_cep=1), "n_mels = 1"), (dict(n_mels=257, stride=300), "n_mels = 257"),
    (dict(n_cep=0), "n_cep = 0"), (dict(n_cep=33), "n_cep = 33"), (dict(n_cep=13, n_mels=13), "n_cep = 13"),
    (dict(deltas=2), "deltas = 2"), (dict(deltas=-1), "deltas = -1"),
    (dict(stride=99), "row_stride = 99"), (dict(start=(0, -1)), "segment 1 has start = -1"),
    (dict(gate=float("nan")), "gate_sum"),
]


@pytest.mark.parametrize("kw,needle", MOMENT_REFUSALS, ids=[n for _, n in MOMENT_REFUSALS])
def test_every_moments_refusal_names_its_argument(kw, needle):
    assert moments_call(**kw) == -1, needle
    assert "f5_cep_moments" in err() and needle in err(), err()


def divergence_call(a=(FAKE, FAKE, FAKE), a_records=3, b=(FAKE, FAKE, FAKE), b_records=2, C_=13, P_=2, i=(0, 2), j=(1, 0), terms=FAKE,
                    status=FAKE):
    arr = lambda v: None if v is None else _lib.int_array(list(v))   # noqa: E731
    return _lib.load().f5_gauss_divergence(*a, a_records, *b, b_records, C_, P_, arr(i), arr(j), terms, status, None)


DIVERGENCE_REFUSALS = [
    (dict(a=(None, FAKE, FAKE)), "a_count"), (dict(a=(FAKE, None, FAKE)), "a_mean"), (dict(a=(FAKE, FAKE, None)), "a_scatter"),
    (dict(b=(None, FAKE, FAKE)), "b_count"), (dict(b=(FAKE, None, FAKE)), "b_mean"), (dict(b=(FAKE, FAKE, None)), "b_scatter"),
    (dict(i=None), "i_host"), (dict(j=None), "j_host"), (dict(terms=None), "null terms"), (dict(status=None), "null status"),
    (dict(C_=0), "C = 0"), (dict(C_=65), "C = 65"), (dict(P_=0), "P = 0"), (dict(P_=65536), "P = 65536"),
    (dict(a_records=0), "a_records = 0"), (dict(b_records=0), "b_records = 0"),
    (dict(i=(0, 3)), "pair 1 has i = 3"), (dict(i=(-1, 0)), "pair 0 has i = -1"), (dict(j=(2, 0)), "pair 0 has j = 2"),
]


@pytest.mark.parametrize("kw,needle", DIVERGENCE_REFUSALS, ids=[n for _, n in DIVERGENCE_REFUSALS])
def test_every_divergence_refusal_names_its_argument(kw, needle):
    assert divergence_call(**kw) == -1, needle
    assert "f5_gauss_divergence" in err() and needle in err(), err()


def test_wrappers_refuse_off_gpu_and_bad_arguments():
    a = [torch.zeros(5, 100)]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=r"cepstral_moments only runs on a GPU \(there is no CPU path\)"):
            M.cepstral_moments(a)
        rec = M.Moments(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 13, dtype=torch.float64),
                        torch.zeros(1, 91, dtype=torch.float64), 13, False)
        with pytest.raises(RuntimeError, match=r"gaussian_divergence only runs on a GPU \(there is no CPU path\)"):
            M.gaussian_divergence(rec, rec)
        m = P.CFM(transformer=P.DiT(**P.config.F5TTS_TINY, text_num_embeds=40, mel_dim=100).init_synthetic())
        with pytest.raises(RuntimeError, match=r"heldout_speaker only runs on a GPU \(there is no CPU path\)"):
            P.infer.heldout_speaker(m, [(torch.zeros(20, 100), [1, 2, 3], torch.zeros(30, 100), [4, 5])])
    with pytest.raises(ValueError, match="at least one"):
        M.cepstral_moments([])
    with pytest.raises(ValueError, match="gate_db"):
        M.gate_sum_of(-1.0, 100)
    assert M.gate_sum_of(None, 100) == -1.0
    assert M.gate_sum_of(40.0, 100) == 40.0 * math.log(10.0) / 20.0 * 100


# ---------------------------------------------------------------------------------------------------- plan
def expected_workspace(frames, n_cep, deltas):
    """The contract's list: (n_cep + 1) doubles and a byte per frame, C + C (C + 1) / 2 doubles and an int per chunk, an int per
    segment, the tables (a DCT table for 256 bins and 24 bytes per segment); every block starts on a multiple of 256 bytes, and the
    whole is rounded up to 256 plus one more 256."""
    Cd = n_cep * (1 + deltas)
    rows, chunks, S = sum(frames), sum(-(-f // M.MOM_CHUNK) for f in frames), len(frames)
    off = 0
    for size in (rows * n_cep * 8, rows * 8, chunks * Cd * 8, chunks * (Cd * (Cd + 1) // 2) * 8, chunks * 4, S * 4, rows,
                 256 * n_cep * 8 + S * 24):
        off = -(-off // 256) * 256 + size
    return -(-off // 256) * 256 + 256


@pytest.mark.parametrize("frames,n_cep,deltas", [([1], 1, 0), ([63, 64, 65, 129], 13, 1), ([4096] * 3, 32, 1), ([700, 5], 13, 0)])
def test_plan_arithmetic(frames, n_cep, deltas):
    assert M.cepstral_moments_plan(frames, n_cep=n_cep, deltas=bool(deltas)) == expected_workspace(frames, n_cep, deltas)


def test_plan_refusals_and_the_call_total():
    lib = _lib.load()
    need = C.c_int64()
    for args, needle in (((0, _lib.int_array([1]), 13, 0, C.byref(need)), "S = 0"), ((1, None, 13, 0, C.byref(need)), "frames_host"),
                         ((1, _lib.int_array([4097]), 13, 0, C.byref(need)), "segment 0 has frames = 4097"),
                         ((1, _lib.int_array([5]), 33, 0, C.byref(need)), "n_cep = 33"),
                         ((1, _lib.int_array([5]), 13, 3, C.byref(need)), "deltas = 3"), ((1, _lib.int_array([5]), 13, 0, None), "workspace_bytes_out")):
        assert lib.f5_cep_moments_plan(*args) == -1 and "f5_cep_moments_plan" in err() and needle in err(), err()
    # 4096 frames at C = 64: the chunk partials are 64 chunks of 64 + 2080 doubles a segment, 2^28 / (64 * 2144) = 1956.3 segments
    # fit (the cepstra, 33 values a frame, would allow 1985); without deltas at n_cep = 1 the 2 values a frame bind: 2^28 / 8192
    big = [4096] * 65535
    assert lib.f5_cep_moments_plan(65535, _lib.int_array(big), 32, 1, C.byref(need)) == -1
    assert "split the batch" in err() and "segment 1956" in err(), err()
    assert lib.f5_cep_moments_plan(32768, _lib.int_array(big[:32768]), 1, 0, C.byref(need)) == 0
    assert lib.f5_cep_moments_plan(32769, _lib.int_array(big[:32769]), 1, 0, C.byref(need)) == -1 and "segment 32768" in err(), err()


# ---------------------------------------------------------------------------------------------------- the oracles
def fixture_pair(seed, frames, n_mels=100):
    rng = np.random.default_rng(seed)
    A, B = O.synthetic_speaker(rng, n_mels), O.synthetic_speaker(rng, n_mels)
    return O.synthetic_utterance(rng, A, frames), O.synthetic_utterance(rng, B, frames + 17)


@pytest.mark.parametrize("n_cep,deltas,frames", [(13, False, 150), (13, True, 300), (5, True, 70), (1, False, 9)])
def test_ordered_oracle_against_the_plain_one(n_cep, deltas, frames):
    """The gate.  Both oracles compute the same quantities from the same f32 inputs in different orders.  Features differ by at
    most n_mels eps relative (a dot product of n_mels terms), means and covariances by a further F eps (sums of F terms, centred),
    and a Cholesky solve with a matrix of condition number kappa returns a perturbation of the data amplified by kappa, with its
    own backward error below 4 C^2 eps (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.4); the terms are
    quadratic in the solves, which doubles it.  Hence rel <= 2 kappa eps (4 C^2 + 2 F + 2 n_mels), kappa the larger condition number
    of the two covariances, measured here."""
    x, y = fixture_pair(11, frames)
    Cd = n_cep * (2 if deltas else 1)
    ri, rj = O.moments(x, n_cep, deltas), O.moments(y, n_cep, deltas)
    (ni, mi, ci), (nj, mj, cj) = O.plain_moments(x, n_cep, deltas), O.plain_moments(y, n_cep, deltas)
    assert (ri[0], rj[0]) == (ni, nj) == (frames, frames + 17)
    kappa = max(np.linalg.cond(ci), np.linalg.cond(cj))
    gate = 2 * kappa * EPS * (4 * Cd * Cd + 2 * (frames + 17) + 2 * 100)
    assert gate < 1e-6, (kappa, gate)           # the fixtures are well enough conditioned for the comparison to mean something
    scale = np.sqrt(np.outer(np.diag(ci), np.diag(ci)))
    assert np.all(np.abs(O.unpack(ri[2], Cd) / ni - ci) <= gate * scale)
    assert np.all(np.abs(ri[1] - mi) <= gate * (np.abs(mi) + np.sqrt(np.diag(ci))))
    terms, status = O.divergence(ri, rj)
    assert status == 0
    plain = O.plain_terms(mi, ci, mj, cj)
    for got, want in zip(terms, plain):
        assert abs(got - want) <= gate * abs(want), (got, want, gate)
    kl, sph = O.numbers(terms, Cd)
    assert kl > 0 and (sph > 0 if Cd > 1 else sph == 0.0)    # (one dimension: two variances are always proportional)


def test_oracle_identities_are_exact():
    """kl(a, a) == 0.0 exactly; (a, b) and (b, a) are the same bits, swapped; a singular side is NaN with status 1."""
    x, y = fixture_pair(3, 120)
    for n_cep, deltas in ((13, False), (13, True), (1, False)):
        Cd = n_cep * (2 if deltas else 1)
        a, b = O.moments(x, n_cep, deltas), O.moments(y, n_cep, deltas)
        same, status = O.divergence(a, a)
        assert status == 0 and same == (float(Cd), float(Cd), 0.0, 0.0)
        assert O.numbers(same, Cd) == (0.0, 0.0)
        ab, ba = O.divergence(a, b)[0], O.divergence(b, a)[0]
        assert ab == (ba[1], ba[0], ba[3], ba[2])
        assert O.numbers(ab, Cd)[0] == O.numbers(ba, Cd)[0] and O.numbers(ab, Cd)[1] == O.numbers(ba, Cd)[1]
        assert M.speaker_numbers(ab, Cd) == dict(kl=O.numbers(ab, Cd)[0], sphericity=O.numbers(ab, Cd)[1])
    few = O.moments(x[:13], 13, False)           # count == C: singular by the rule
    terms, status = O.divergence(few, b := O.moments(y, 13, False))
    assert status == 1 and all(math.isnan(v) for v in terms)
    n, mean, sc = O.moments(x, 13, False)        # feature 1 := feature 0 with a variance of exactly 4 (its root and 4 / 2 are exact):
    S = O.unpack(sc, 13)                         # the second pivot is exactly 0
    S[:, 1], S[1, :] = S[:, 0].copy(), S[0, :].copy()
    S[:2, :2] = 4.0 * n
    assert O.divergence((n, mean, S[O.triu(13)]), b)[1] == 1 and O.divergence(b, (n, mean, S[O.triu(13)]))[1] == 1
    out = M.speaker_numbers([list(terms), [13.0, 13.0, 0.0, 0.0]], 13)
    assert math.isnan(out["kl"][0]) and math.isnan(out["sphericity"][0]) and out["kl"][1] == 0.0 and out["sphericity"][1] == 0.0


def test_the_table_is_the_distance_oracles_table():
    """One DCT table for both measures: speaker_oracle's (the contract's expression with the C library's cosine, as the host code
    builds it) against dtw_oracle's (np.cos), transposed; two correctly rounded cosines of one argument differ by an ulp at most."""
    import dtw_oracle
    for n_mels, n_cep in ((100, 32), (80, 13), (2, 1)):
        ours, theirs = O.dct_table(n_mels, n_cep), dtw_oracle.dct_table(n_mels, n_cep).T
        assert ours.shape == theirs.shape and np.all(np.abs(ours - theirs) <= 2.0 ** -52 * np.abs(theirs))
    x, _ = fixture_pair(2, 40)
    assert np.allclose(O.features(x, 13, False), dtw_oracle.cepstra(x, 13), rtol=0, atol=100 * 2.0 ** -52 * np.abs(x).sum(axis=1).max())


def test_selection_in_the_oracle():
    x, _ = fixture_pair(5, 90)
    e = O.energies(x)
    gate = M.gate_sum_of(3.0, 100)
    sel, finite = O.selection(x, None, gate)
    assert finite and 0 < sel.sum() < 90 and np.array_equal(sel, e >= e.max() - gate)
    n, mean, sc = O.moments(x, 13, True, gate_sum=gate)
    pn, pm, pc = O.plain_moments(x, 13, True, sel)      # deltas over the segment's own frames, whatever the selection
    assert n == pn == sel.sum() and np.allclose(mean, pm, rtol=1e-10, atol=1e-12) and np.allclose(O.unpack(sc, 26) / n, pc, rtol=1e-9, atol=1e-13)
    assert O.moments(x, 13, False, mask=np.zeros(90))[0] == 0
    bad = x.copy()
    bad[40, 7] = np.inf
    n, mean, sc = O.moments(bad, 13, False)
    assert n == -1 and np.all(np.isnan(mean)) and np.all(np.isnan(sc))


# ---------------------------------------------------------------------------------------------------- merge_moments
def as_moments(records, n_cep, deltas):
    return M.Moments(torch.tensor([r[0] for r in records], dtype=torch.int32), torch.tensor(np.stack([r[1] for r in records])),
                     torch.tensor(np.stack([r[2] for r in records])), n_cep, deltas)


def test_merge_over_a_split_is_the_moments_of_the_concatenation():
    """The bound.  A scatter entry is a sum of F products whose absolute values add up to at most sqrt(S_pp S_qq) (Cauchy-Schwarz),
    so either way of summing it carries at most F eps of that; the pairwise update adds three such terms and a handful of
    operations: |dS_pq| <= 4 (F + 8) eps sqrt(S_pp S_qq).  A mean is a sum of F values: |dmean_p| <= 4 F eps max_t |v_tp|."""
    x, _ = fixture_pair(7, 333)
    n_cep, Cd = 13, 13
    cuts = [0, 1, 65, 200, 333]
    parts = [O.moments(x[a:b], n_cep) for a, b in zip(cuts[:-1], cuts[1:])]
    parts.insert(2, O.moments(x[:4], n_cep, mask=np.zeros(4)))       # an empty record adds nothing
    whole = O.moments(x, n_cep)
    other = O.moments(x[100:180], n_cep)
    rec = as_moments(parts + [other], n_cep, False)
    merged, labels = M.merge_moments(rec, ["a"] * 5 + ["b"])
    assert labels == ["a", "b"] and merged.count.tolist() == [333, 80]
    assert torch.equal(merged.mean[1], rec.mean[5]) and torch.equal(merged.scatter[1], rec.scatter[5])   # alone: unchanged
    v = O.features(x, n_cep, False)
    S = O.unpack(whole[2], Cd)
    p, q = O.triu(Cd)
    tol_s = 4 * (333 + 8) * EPS * np.sqrt(np.diag(S)[p] * np.diag(S)[q])
    tol_m = 4 * 333 * EPS * np.abs(v).max(axis=0)
    assert np.all(np.abs(merged.scatter[0].numpy() - whole[2]) <= tol_s)
    assert np.all(np.abs(merged.mean[0].numpy() - whole[1]) <= tol_m)
    # the torch fold is the oracle's pairwise update, folded in item order
    acc = parts[0]
    for r in parts[1:]:
        acc = O.merge(acc, r) if r[0] > 0 else acc
    assert np.allclose(merged.scatter[0].numpy(), acc[2], rtol=1e-13, atol=0) and np.allclose(merged.mean[0].numpy(), acc[1], rtol=1e-14)
    # a record with a non-finite frame poisons its own label alone
    bad = (-1, np.full(Cd, np.nan), np.full(len(p), np.nan))
    merged, labels = M.merge_moments(as_moments([parts[0], bad, other], n_cep, False), [0, 0, 1])
    assert merged.count.tolist() == [-1, 80] and torch.isnan(merged.mean[0]).all() and torch.isnan(merged.scatter[0]).all()
    assert torch.equal(merged.scatter[1], rec.scatter[5])
    with pytest.raises(ValueError, match="labels"):
        M.merge_moments(rec, ["a"])


# ---------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("frames", [60, 200, 800])
def test_same_speaker_is_closer_than_another_speaker(frames):
    """A sanity condition on the measure, not a claim about real voices: 100 mel bins, 13 cepstra, 50 seeds.  Two utterances of one
    synthetic speaker (speaker_oracle.synthetic_speaker: a smooth envelope and a speaker's own mixing of a shared AR(1) content
    process) are closer than utterances of two speakers, for both numbers, on every seed."""
    for seed in range(50):
        rng = np.random.default_rng(seed)
        A, B = O.synthetic_speaker(rng), O.synthetic_speaker(rng)
        a1, a2, b1 = (O.moments(O.synthetic_utterance(rng, s, frames), 13) for s in (A, A, B))
        same = O.numbers(O.divergence(a1, a2)[0], 13)
        other = O.numbers(O.divergence(a1, b1)[0], 13)
        assert 0 < same[0] < other[0], (seed, "kl", same, other)
        assert 0 < same[1] < other[1], (seed, "sphericity", same, other)
