"""CPU: the host side of speech editing -- infer.edit_plan against a per-frame restatement (tests/edit_oracle.py), the documented
errors, the host edit mask against the torch.cat construction, and the argument validation of f5_edit_assemble / f5_wave_splice,
which runs before anything touches a GPU."""
import ctypes as C

import pytest
import torch

import edit_oracle as O

import f5_tts_amd as P
from f5_tts_amd import _lib
from f5_tts_amd import infer as I


@pytest.mark.parametrize("name", list(O.PLAN_CASES))
def test_edit_plan_equals_the_per_frame_restatement(name):
    n_frames, parts, fix = O.PLAN_CASES[name]
    plan = I.edit_plan(n_frames, parts, fix)
    segments, D = plan
    want = O.frame_map(n_frames, parts, fix)
    assert O.expand(plan) == want and D == len(want)
    assert all(isinstance(v, int) for s in segments for v in s)
    # neighbours of one kind are allowed (an empty KEEP between two parts leaves two EDIT segments); empty segments are not
    assert all(frames > 0 for _, _, frames in segments)


def test_plan_cases_are_what_their_names_say():
    seg = lambda name: I.edit_plan(*O.PLAN_CASES[name])  # noqa: E731
    assert seg("no_parts") == ([(0, 0, 37)], 37)
    assert seg("part_from_frame_0") == ([(0, -1, 19), (19, 19, 45)], 64)
    assert seg("part_to_the_last_frame") == ([(0, 0, 38), (38, -1, 27)], 65)           # 37.5 -> 38, 0.283 s -> 26.53 -> 27; no KEEP behind
    assert seg("adjacent_parts") == ([(0, 0, 9), (9, -1, 19), (28, -1, 19), (47, 47, 17)], 64)
    assert seg("fix_duration_longer") == ([(0, 0, 19), (19, -1, 47), (66, 38, 26)], 92)
    assert seg("fix_duration_shorter") == ([(0, 0, 19), (19, -1, 5), (24, 38, 26)], 50)
    assert seg("fix_duration_of_0_frames") == ([(0, 0, 19), (19, 38, 26)], 45)


def test_ties_round_to_even():
    """The starts 2.0 s and 6.0 s land exactly on k + 0.5 in double, k = 187 (odd: up to 188) and k = 562 (even: stays)."""
    assert 2.0 * 24000 / 256 == 187.5 and 6.0 * 24000 / 256 == 562.5
    assert round(187.5) == 188 and round(562.5) == 562
    segments, D = I.edit_plan(*O.PLAN_CASES["ties_to_even"])
    assert segments == [(0, 0, 188), (188, -1, 94), (282, 281, 281), (563, -1, 94), (657, 656, 44)] and D == 701


@pytest.mark.parametrize("args, match", [
    ((64, [(0.3, 0.5), (0.1, 0.2)], None), "time order"),                 # out of order
    ((64, [(0.1, 0.3), (0.25, 0.5)], None), "time order"),                # overlapping
    ((64, [(0.5, 0.3)], None), "time order"),                             # ends before it starts
    ((64, [(0.2, 0.8)], None), "inside the recording"),                   # 75 > 64 frames
    ((64, [(-0.1, 0.2)], None), "time order"),                            # starts before the recording
    ((64, [(0.1, 0.2)], [0.1, 0.1]), "fix_duration"),
    ((64, [(0.1, 0.2)], []), "fix_duration"),
    ((64, [(0.1, 0.2)], [-0.1]), "frames"),
    ((700, [(0.1 * k, 0.1 * k + 0.05) for k in range(17)], None), "at most 16"),
    ((1, [], None), "at least 2"),
    ((20, [(0.0, 0.2)], [0.004]), "at least 2"),                          # 19 of 20 frames cut out, nothing put in
])
def test_edit_plan_errors(args, match):
    with pytest.raises(ValueError, match=match):
        I.edit_plan(*args)


def test_sixteen_parts_are_accepted():
    parts = [(0.1 * (k + 1), 0.1 * (k + 1) + 0.05) for k in range(16)]
    plan = I.edit_plan(700, parts, None)
    assert len(plan[0]) == 33 and O.expand(plan) == O.frame_map(700, parts)


@pytest.mark.parametrize("name", list(O.PLAN_CASES))
def test_host_mask_and_frames_equal_the_cat_construction(name):
    n_frames, parts, fix = O.PLAN_CASES[name]
    mel = torch.randn(1, n_frames, 4, generator=torch.Generator().manual_seed(n_frames))
    want_cond, want_mask = O.cat_construction(mel, parts, fix)
    plan = I.edit_plan(n_frames, parts, fix)
    mask = I.edit_mask([plan])
    assert mask.dtype == torch.bool and mask.device.type == "cpu" and torch.equal(mask, want_mask)
    assert torch.equal(O.assemble([mel[0]], [O.expand(plan)]), want_cond)     # the two yardsticks agree with each other


def test_host_mask_of_a_batch_is_padded_with_true():
    names = ["fix_duration_longer", "no_parts", "fix_duration_of_0_frames"]
    plans = [I.edit_plan(*O.PLAN_CASES[n]) for n in names]
    mask = I.edit_mask(plans)
    assert mask.shape == (3, 92)
    for b, n in enumerate(names):
        n_frames, parts, fix = O.PLAN_CASES[n]
        want = O.cat_construction(torch.zeros(1, n_frames, 1), parts, fix)[1][0]
        assert torch.equal(mask[b, :len(want)], want) and mask[b, len(want):].all()


# ------------------------------------------------------------------------------------ argument validation, no GPU
FAKE = C.c_void_p(0x1000)        # a non-null "device pointer": validation never dereferences device memory


def assemble_args(**over):
    a = dict(mel=FAKE, B=1, mel_stride=8 * 100, row=100, frames=_lib.int_array([8]), counts=_lib.int_array([2]),
             segs=_lib.int_array([0, 0, 3, 3, -1, 2]), dur=_lib.int_array([5]), cond=FAKE, D_max=5, stream=None)
    a.update(over)
    return [a[k] for k in ("mel", "B", "mel_stride", "row", "frames", "counts", "segs", "dur", "cond", "D_max", "stream")]


def splice_args(**over):
    a = dict(gen=FAKE, B=1, gen_stride=1024, lens=_lib.int_array([1024]), a_base=FAKE, a_start=(C.c_int64 * 1)(0),
             a_len=_lib.int_array([2048]), counts=_lib.int_array([1]), segs=_lib.int_array([0, 0, 2]), hop=256, cf=240, out=FAKE,
             out_stride=1024, stream=None)
    a.update(over)
    return [a[k] for k in ("gen", "B", "gen_stride", "lens", "a_base", "a_start", "a_len", "counts", "segs", "hop", "cf", "out",
                           "out_stride", "stream")]


def rejected(fn, args, name):
    lib = _lib.load()
    rc = getattr(lib, fn)(*args)
    msg = lib.f5_last_error().decode()
    assert rc == -1, f"{fn} with a bad {name}: rc {rc} ({msg})"
    assert msg.startswith(fn + ":"), msg
    return msg


C_NAMES = dict(frames="frames_host", counts="seg_count_host", segs="segs_host", dur="dur_host", lens="len_host",
               a_start="a_start_host", a_len="a_len_host")     # the argument's name in include/f5_hip.h, which the message gives


@pytest.mark.parametrize("name", ["mel", "frames", "counts", "segs", "dur", "cond"])
def test_assemble_rejects_null_pointers(name):
    assert C_NAMES.get(name, name) + " is null" in rejected("f5_edit_assemble", assemble_args(**{name: None}), name)


@pytest.mark.parametrize("name", ["gen", "lens", "a_base", "a_start", "a_len", "counts", "segs", "out"])
def test_splice_rejects_null_pointers(name):
    assert C_NAMES.get(name, name) + " is null" in rejected("f5_wave_splice", splice_args(**{name: None}), name)


@pytest.mark.parametrize("B", [0, 65, -1])
def test_item_count_out_of_range(B):
    assert "B" in rejected("f5_edit_assemble", assemble_args(B=B), "B")
    assert "B" in rejected("f5_wave_splice", splice_args(B=B), "B")


@pytest.mark.parametrize("segs, what", [
    ([0, 6, 3, 3, -1, 2], "source range [6, 9) of 8 frames"),
    ([0, -2, 3, 3, -1, 2], "source frame -2"),
    ([0, 0, 3, 3, -1, 3], "destination [3, 6) of 5 frames"),
    ([-1, 0, 3, 3, -1, 2], "destination from frame -1"),
    ([0, 0, 3, 2, -1, 2], "overlapping destinations"),
    ([0, 0, 0, 3, -1, 2], "an empty segment"),
])
def test_assemble_rejects_segments_out_of_range(segs, what):
    assert "segment" in rejected("f5_edit_assemble", assemble_args(segs=_lib.int_array(segs)), what)


def test_assemble_rejects_the_rest():
    rejected("f5_edit_assemble", assemble_args(dur=_lib.int_array([6])), "D_b above D_max")
    rejected("f5_edit_assemble", assemble_args(counts=_lib.int_array([34])), "segment count")
    rejected("f5_edit_assemble", assemble_args(mel_stride=7 * 100), "stride below T rows")
    rejected("f5_edit_assemble", assemble_args(row=0), "row")


@pytest.mark.parametrize("segs, what", [
    ([0, -1, 2], "an EDIT segment"),
    ([-1, 0, 2], "destination from frame -1"),
    ([0, 0, 0], "an empty segment"),
])
def test_splice_rejects_segments_out_of_range(segs, what):
    assert "segment" in rejected("f5_wave_splice", splice_args(segs=_lib.int_array(segs)), what)


def test_splice_rejects_the_rest():
    rejected("f5_wave_splice", splice_args(counts=_lib.int_array([2]), segs=_lib.int_array([2, 0, 2, 3, 0, 1])), "overlapping destinations")
    rejected("f5_wave_splice", splice_args(lens=_lib.int_array([1025])), "L above the strides")
    rejected("f5_wave_splice", splice_args(hop=0), "hop")
    rejected("f5_wave_splice", splice_args(cf=-1), "cross_fade_samples")
    rejected("f5_wave_splice", splice_args(a_len=_lib.int_array([-1])), "a_len")
    rejected("f5_wave_splice", splice_args(counts=_lib.int_array([34])), "segment count")


def test_python_wrappers_refuse_to_run_off_the_gpu():
    ms = P.mel.MelSpec()
    with pytest.raises(RuntimeError, match="GPU"):
        ms.edit_assemble(torch.zeros(1, 100, 8), [8], [I.edit_plan(8, [], None)])
    with pytest.raises(RuntimeError, match="GPU"):
        I.wave_splice(torch.zeros(1, 1792), [1792], [torch.zeros(2048)], [I.edit_plan(8, [], None)], 240)


class StubModel:
    vocab_char_map = None
    device = "cpu"
    mel_spec = None


class StubVocoder:
    def decode_ragged(self, *a, **k):
        raise AssertionError("not reached")


def test_speech_edit_argument_errors():
    rec = [(torch.full((1, 24000), 0.2), 24000, "Hello there.", [(0.1, 0.2)], None)]
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        I.speech_edit(StubModel(), P.BigVGAN(P.config.BIGVGAN_TINY), rec)
    kor = StubModel()
    kor._tokenizer_type = "kor_jamo"
    with pytest.raises(NotImplementedError, match="text_tokenizer"):
        I.speech_edit(kor, StubVocoder(), rec)
    with pytest.raises(ValueError):
        I.speech_edit(StubModel(), StubVocoder(), [])
    with pytest.raises(TypeError, match="edit_mask"):
        I.speech_edit(StubModel(), StubVocoder(), rec, edit_mask=None)
