"""CPU: the DTW-aligned mel-cepstral distance (include/f5_hip.h, csrc/dtw.hip, metrics.py) without a GPU -- the two entry points are
declared, exported and bound; every refusal names its argument and happens before anything is launched (null handles and pointers
that are never dereferenced); the plan against hand-computed orders and the workspace bound (never an n x m matrix); the oracle
(dtw_oracle.py) pinned three ways -- its cepstra against scipy's orthonormal DCT-II, its D against the exhaustive enumeration of
every monotone path for all n, m <= 4, and the identities of the measure -- and every named wrong variant at least 1e-3 (relative)
away from the true value on the fixtures, so that the GPU gate of 2^-39 cannot hide a wrong recurrence; heldout_distance's host plan
against the reference's get_inference_prompt arithmetic (eval/utils_eval.py:109-148), restated."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import dtw_oracle as O
from conftest import ROOT

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import metrics as M

FAKE = C.c_void_p(0x1000)                   # a device pointer that no refusal may dereference


def i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def err():
    return _lib.load().f5_last_error().decode()


# ---------------------------------------------------------------------------------------------------- ABI
def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    for name in ("f5_mel_distance_plan", "f5_mel_distance"):
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/f5_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "metrics" in P.__all__ and P.metrics is M
    assert callable(P.infer.heldout_distance)


def test_named_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "korean-f5-tts_amd", "csrc", "dtw.hip")).read()
    for name, val in (("kDtwThreads", M.DTW_THREADS), ("kDtwMaxStrip", M.DTW_MAX_STRIP), ("kDtwRowBlock", M.DTW_ROW_BLOCK)):
        assert re.search(rf"constexpr int {name} = {val};", src), name
    assert M.DTW_THREADS * M.DTW_MAX_STRIP == M.MAX_FRAMES == 4096
    assert [M.strip_width(c) for c in (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert re.search(r"4\.3429448190325175", src) and float.fromhex("0x1.15f2ced384f28p+2") == O.SCALE


# ---------------------------------------------------------------------------------------------------- refusals
def call(P_=2, a_base=FAKE, b_base=FAKE, a_start=(0, 700), a_frames=(7, 5), a_stride=100, b_start=(0, 900), b_frames=(9, 3),
         b_stride=100, n_mels=100, n_cep=13, out=FAKE):
    arr = lambda v, f: None if v is None else f(list(v))   # noqa: E731
    return _lib.load().f5_mel_distance(a_base, b_base, P_, arr(a_start, i64), arr(a_frames, _lib.int_array), a_stride,
                                       arr(b_start, i64), arr(b_frames, _lib.int_array), b_stride, n_mels, n_cep, out, None)


REFUSALS = [
    (dict(a_base=None), "a_base"), (dict(b_base=None), "b_base"), (dict(out=None), "out"),
    (dict(a_start=None), "a_start_host"), (dict(b_start=None), "b_start_host"),
    (dict(a_frames=None), "a_frames_host"), (dict(b_frames=None), "b_frames_host"),
    (dict(P_=0), "P = 0"), (dict(P_=65536), "P = 65536"), (dict(P_=-1), "P = -1"),
    (dict(a_frames=(0, 5)), "pair 0 has a_frames = 0"), (dict(a_frames=(7, 4097)), "pair 1 has a_frames = 4097"),
    (dict(b_frames=(9, 0)), "pair 1 has b_frames = 0"), (dict(b_frames=(4097, 3)), "pair 0 has b_frames = 4097"),
    (dict(b_frames=(-3, 3)), "pair 0 has b_frames = -3"),
    (dict(n_cep=0), "n_cep = 0"), (dict(n_cep=65, n_mels=128, a_stride=128, b_stride=128), "n_cep = 65"), (dict(n_cep=13, n_mels=13), "n_cep = 13"),
    (dict(n_cep=100), "n_cep = 100"),
    (dict(n_mels=1, n_cep=1), "n_mels = 1"), (dict(n_mels=257, a_stride=300, b_stride=300), "n_mels = 257"),
    (dict(a_stride=99), "a_row_stride = 99"), (dict(b_stride=0), "b_row_stride = 0"),
    (dict(a_start=(0, -1)), "pair 1 has a_start = -1"), (dict(b_start=(-5, 0)), "pair 0 has b_start = -5"),
]


@pytest.mark.parametrize("kw,needle", REFUSALS, ids=[n for _, n in REFUSALS])
def test_every_refusal_names_its_argument(kw, needle):
    assert call(**kw) == -1, needle
    assert "f5_mel_distance" in err() and needle in err(), err()


def test_the_limits_themselves_pass_the_plan():
    lib = _lib.load()
    order, need = (C.c_int32 * 2)(), C.c_int64()
    assert lib.f5_mel_distance_plan(2, _lib.int_array([4096, 1]), _lib.int_array([1, 4096]), 64, order, C.byref(need)) == 0
    for kw, needle in ((dict(P=0), "P = 0"), (dict(a=[4097, 1]), "pair 0 has a_frames"), (dict(b=[1, 0]), "pair 1 has b_frames"),
                       (dict(n_cep=65), "n_cep = 65"), (dict(n_cep=0), "n_cep = 0"), (dict(order=None), "order_out"),
                       (dict(need=None), "workspace_bytes_out"), (dict(a=None), "a_frames_host"), (dict(b=None), "b_frames_host")):
        args = dict(P=2, a=[3, 4], b=[5, 6], n_cep=13, order=order, need=C.byref(need))
        args.update(kw)
        rc = lib.f5_mel_distance_plan(args["P"], _lib.int_array(args["a"]), _lib.int_array(args["b"]), args["n_cep"], args["order"],
                                      args["need"])
        assert rc == -1 and "f5_mel_distance_plan" in err() and needle in err(), err()
    # the total of one call: 65535 pairs of 4096 + 4096 frames at n_cep = 64 is far past 2^28 cepstral values
    big = [4096] * 65535
    rc = lib.f5_mel_distance_plan(65535, _lib.int_array(big), _lib.int_array(big), 64, (C.c_int32 * 65535)(), C.byref(need))
    assert rc == -1 and "split the batch" in err() and "pair 512" in err(), err()   # 2^28 / (64 * 8192) = 512 pairs fit


def test_wrapper_refuses_off_gpu_and_bad_arguments():
    a = [torch.zeros(5, 100)]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=r"mel_distance only runs on a GPU \(there is no CPU path\)"):
            M.mel_distance(a, a)
    with pytest.raises(ValueError, match="one pair each"):
        M.mel_distance(a, a + a)
    with pytest.raises(ValueError, match="one pair each"):
        M.mel_distance([], [])
    with pytest.raises(ValueError, match="view"):
        M.mel_distance([(torch.zeros(2, 9, 100), 0, 5, 5)], a)
    with pytest.raises(ValueError, match="one pair each"):
        M.mel_distance_plan([1, 2], [3])


# ---------------------------------------------------------------------------------------------------- plan
def test_plan_orders_by_area_and_never_holds_a_matrix():
    # areas 12, 12, 35, 1, 35, 4096: largest first, ties by index
    order, need = M.mel_distance_plan([3, 6, 5, 1, 7, 4096], [4, 2, 7, 1, 5, 1])
    assert order == [5, 2, 4, 0, 1, 3]
    assert M.mel_distance_plan([9], [9])[0] == [0]
    assert M.mel_distance_plan([2, 2, 2], [2, 2, 2])[0] == [0, 1, 2]
    assert M.mel_distance_plan([1, 4096, 64], [4096, 4096, 65])[0] == [1, 2, 0]
    # one 4096 x 4096 pair at n_cep = 13: the cepstra (8192 * 13 * 8 bytes) and the tables, under 2 MiB; the matrix would be 128 MiB
    need = M.mel_distance_plan([4096], [4096], n_cep=13)[1]
    assert 8192 * 13 * 8 <= need < 2 * 1024 * 1024
    # the workspace grows with sum n + sum m, not with n * m
    n1 = M.mel_distance_plan([100] * 10, [200] * 10)[1]
    n2 = M.mel_distance_plan([100] * 20, [200] * 20)[1]
    assert 0 < n2 - n1 <= 10 * (300 * 13 * 8 + 256) + 512


# ---------------------------------------------------------------------------------------------------- the oracle, pinned
@pytest.mark.parametrize("n_mels,n_cep", [(100, 13), (80, 13), (100, 1), (100, 64), (17, 16)])
def test_oracle_cepstra_are_the_orthonormal_dct(n_mels, n_cep):
    dct = pytest.importorskip("scipy.fft").dct
    x = O.random_walk_mel(3, 37, n_mels)
    ref = dct(x.astype(np.float64), type=2, norm="ortho", axis=1)[:, 1:n_cep + 1]
    got = O.cepstra(x, n_cep)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12
    with0 = O.cepstra(x, n_cep, first=0)
    assert np.abs(with0 - dct(x.astype(np.float64), type=2, norm="ortho", axis=1)[:, :n_cep]).max() <= 1e-12


def all_paths(n, m):
    """Every monotone path (0, 0) -> (n - 1, m - 1) over the steps (1, 0), (1, 1), (0, 1), as lists of (i, j, weight)."""
    def walk(i, j):
        if (i, j) == (n - 1, m - 1):
            yield []
            return
        for di, dj, w in ((1, 0, 1.0), (1, 1, 2.0), (0, 1, 1.0)):
            if i + di < n and j + dj < m:
                for rest in walk(i + di, j + dj):
                    yield [(i + di, j + dj, w)] + rest
    return walk(0, 0)


@pytest.mark.parametrize("n,m", list(itertools.product(range(1, 5), repeat=2)))
def test_oracle_D_is_the_minimum_over_all_monotone_paths(n, m):
    g = np.random.default_rng(10 * n + m)
    d = g.uniform(0.1, 5.0, size=(n, m))
    best, count = math.inf, 0
    for path in all_paths(n, m):
        total, weight = 2.0 * d[0, 0], 2.0
        for i, j, w in path:                 # summed in path order, as the recurrence does
            total = total + w * d[i, j]
            weight += w
        assert weight == n + m               # every path has total weight n + m
        best, count = min(best, total), count + 1
    assert count >= 1 and O.accumulate(d) == best
    assert O.accumulate(d, full=True)[-1, -1] == best


def test_oracle_identities():
    a = O.random_walk_mel(1, 41)
    b = O.warped(a, 2, 57)
    assert O.value(a, a) == 0.0
    assert O.value(a, np.repeat(a, 2, axis=0)) == 0.0          # a perfect warp costs nothing
    assert O.value(a, b) == O.value(b, a) > 0.0                # bit symmetry
    assert np.array_equal(O.frame_distances(O.cepstra(a, 13), O.cepstra(b, 13)), O.frame_distances(O.cepstra(b, 13), O.cepstra(a, 13)).T)
    x = a.copy()
    x[5, 7] = np.nan
    assert not np.isfinite(O.value(x, b)) and not np.isfinite(O.value(b, x))


FIXTURES = [(11, 60, 75), (12, 90, 64), (13, 33, 130)]


@pytest.mark.parametrize("variant", O.VARIANTS)
def test_every_wrong_variant_misses_the_true_value(variant):
    for seed, n, m in FIXTURES:
        a, b = O.pair(seed, n, m)
        true, wrong = O.value(a, b), O.value(a, b, variant=variant)
        rel = abs(wrong - true) / true
        print(f"{variant}: seed {seed} ({n} x {m}): true {true:.6f} dB, variant {wrong:.6f}, relative {rel:.3e}")
        assert true > 0.0 and rel >= 1e-3, (variant, seed, true, wrong)


# ---------------------------------------------------------------------------------------------------- heldout_distance's host plan
def reference_prompt(p, prompt_text, g, target_text, speed, use_truth_duration):
    """get_inference_prompt's text and duration arithmetic (eval/utils_eval.py:120-148) for one utterance whose prompt mel has p
    frames and whose target has g frames (gt_audio.shape[-1] / hop_length), restated."""
    if len(prompt_text[-1].encode("utf-8")) == 1:
        prompt_text = prompt_text + " "
    text = prompt_text + target_text
    if use_truth_duration:
        total = p + int(g / speed)
    else:
        total = p + int(p / len(prompt_text.encode("utf-8")) * len(target_text.encode("utf-8")) / speed)
    return text, total


ITEMS = [(310, "안녕하세요.", 421, "오늘 날씨가 참 좋네요"), (95, "반갑습니다", 777, "이 문장은 조금 더 길게 이어지는 문장입니다."),
         (288, "Some text", 150, "and a short one."), (1200, "긴 프롬프트입니다!", 2100, "그리고 긴 목표 문장이 여기에 옵니다, 정말로요.")]


@pytest.mark.parametrize("duration", ["truth", "text"])
@pytest.mark.parametrize("speed", [1.0, 0.8, 1.3])
def test_heldout_plan_is_the_references_arithmetic(duration, speed):
    items = [(torch.zeros(p, 100), pt, torch.zeros(g, 100), tt) for p, pt, g, tt in ITEMS]
    texts, lens, totals, groups = P.infer.heldout_distance_plan(items, duration=duration, speed=speed, batch_frames=2000)
    for u, (p, pt, g, tt) in enumerate(ITEMS):
        text, total = reference_prompt(p, pt, g, tt, speed, duration == "truth")
        assert texts[u] == text and lens[u] == p and totals[u] == total
    assert texts[0].startswith("안녕하세요. ") and texts[1].startswith("반갑습니다이")      # one-byte last character: a space; else none
    # the reference's bucketing (no duration window, no shuffle): every item once, batches under the frame budget rule
    assert sorted(u for g_ in groups for u in g_) == list(range(len(ITEMS)))
    assert groups == P.batching.bucket_prompts(totals, infer_batch_size=2000, min_secs=0,
                                               max_secs=max(40, max(totals) * 256 // 24000 + 1), shuffle_seed=None)


def test_heldout_plan_tokens_and_refusals():
    z = torch.zeros
    items = [(z(10, 100), [1, 2, 3], z(20, 100), [4, 5]), (z(7, 100), torch.tensor([9]), z(31, 100), torch.tensor([8, 7]))]
    texts, lens, totals, groups = P.infer.heldout_distance_plan(items, speed=2.0)
    assert texts == [[1, 2, 3, 4, 5], [9, 8, 7]] and lens == [10, 7] and totals == [20, 22]
    with pytest.raises(ValueError, match="duration='text'.*item 0.*strings"):
        P.infer.heldout_distance_plan(items, duration="text")
    with pytest.raises(ValueError, match="duration = 'frames'"):
        P.infer.heldout_distance_plan(items, duration="frames")
    with pytest.raises(ValueError, match="item 0: prompt_text and target_text"):
        P.infer.heldout_distance_plan([(z(10, 100), "ab", z(20, 100), [4, 5])])
    with pytest.raises(ValueError, match="item 0.*at least one frame"):
        P.infer.heldout_distance_plan([(z(0, 100), "ab", z(20, 100), "cd")])
