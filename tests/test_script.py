"""CPU: the host side of the multi-voice script (infer.synthesize_script) -- parse_script against the reference's loop restated
(script_oracle.reference_parse), script_plan against hand-computed cases, join_plan plus the fold of include/f5_hip.h against
cross_fade_concat per run, and f5_wave_join's declaration, binding and argument checks (they precede every HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import script_oracle as O

from f5_tts_amd import _lib
from f5_tts_amd import infer as I
from f5_tts_amd import script as S

F5_EINVAL = -1
NAME = "f5_wave_join"
VOICES = {"main": {}, "town": {}, "나레이터": {}}

SCRIPTS = {
    "text_before_the_first_tag": "Hello there. [town] General Kenobi! [main] You are a bold one.",
    "adjacent_tags": "[town][main] Two tags, each a stretch of its own. [town] [main] And two more here.",
    "unknown_name": "[nobody] spoken by the default voice. [town] and by town.",
    "tag_at_the_end": "[town] some words [main]",
    "bracketed_non_word": "[town] this [a b] is no tag, nor is [] or [a-b]. [main]back.",
    "whitespace_only_stretches": "  \n [town]   \t\n[main]   [town] words at last  \n ",
    "hangul_names": "[나레이터] 안녕하세요. [town] hello [나레이터]다시.",
    "no_tag_at_all": "Only the default voice speaks here.",
}


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_parse_script_is_the_reference_loop(name):
    want = O.reference_parse(SCRIPTS[name], VOICES)
    assert want, "the case is empty"
    assert S.parse_script(SCRIPTS[name], VOICES) == want
    assert I.parse_script is S.parse_script


def test_parse_script_cases_say_what_their_names_say():
    parse = lambda name: S.parse_script(SCRIPTS[name], VOICES)   # noqa: E731
    assert parse("text_before_the_first_tag")[0] == ("main", "Hello there.")
    assert parse("adjacent_tags") == [("town", ""), ("main", "Two tags, each a stretch of its own."), ("town", ""),
                                      ("main", "And two more here.")]
    assert parse("unknown_name")[0] == ("main", "spoken by the default voice.")
    assert parse("tag_at_the_end") == [("town", "some words"), ("main", "")]
    assert parse("bracketed_non_word") == [("town", "this [a b] is no tag, nor is [] or [a-b]."), ("main", "back.")]
    assert parse("whitespace_only_stretches") == [("town", ""), ("main", ""), ("town", "words at last")]
    assert parse("hangul_names") == [("나레이터", "안녕하세요."), ("town", "hello"), ("나레이터", "다시.")]
    assert S.parse_script("[town] x", VOICES, default="나레이터") == [("town", "x")]
    assert S.parse_script("[gone] x", VOICES, default="나레이터") == [("나레이터", "x")]
    for empty in ("", "  \n\t "):
        assert O.reference_parse(empty, VOICES) == []
        with pytest.raises(ValueError, match="parse_script"):
            S.parse_script(empty, VOICES)


# 2 s prompts at 24 kHz: 48000 samples, ref_audio_len = 48000 // 256 = 187 frames
PROMPTS = {
    "main": dict(seconds=2.0, samples=48000, ref_text="hello there."),            # 12 bytes, 13 with the trailing space
    "slow": dict(seconds=2.0, samples=48000, ref_text="hello there.", speed=0.5),
    "terse": dict(seconds=2.0, samples=48000, ref_text="hi.", speed=None),         # 3 bytes: max_chars = int(3 / 2 * 20) = 30
    "한": dict(seconds=2.0, samples=48000, ref_text="안녕하세요"),                    # 15 bytes, the last of 3: no space is added
}
BOLD = "General Kenobi, you are a bold one."                                       # 35 bytes
LONG = "General Kenobi, you are a bold one. So uncivilised, this is."


def test_script_plan_hand_computed():
    stretches = [("main", BOLD), ("slow", BOLD), ("main", "Yes."), ("terse", LONG), ("slow", ""), ("한", BOLD)]
    plan = S.script_plan(stretches, PROMPTS, speed=1.0, cross_fade_duration=0.15)
    assert plan["items"] == [
        (0, 0, "hello there. " + BOLD, 187 + 503),                # int(187 / 13 * 35 / 1.0) = int(503.46)
        (1, 1, "hello there. " + BOLD, 187 + 1006),               # the voice's speed 0.5: int(187 / 13 * 35 / 0.5) = int(1006.92)
        (0, 2, "hello there. Yes.", 187 + 191),                   # 4 bytes < 10: local_speed 0.3, int(187 / 13 * 4 / 0.3) = int(191.79)
        (2, 3, "hi. General Kenobi,", 187 + 701),                 # max_chars 30: 16 + 19 > 30, 20 + 15 > 30, 16 + 8 <= 30
        (2, 3, "hi. you are a bold one.", 187 + 888),             # int(187 / 4 * 19) = int(888.25)
        (2, 3, "hi. So uncivilised, this is.", 187 + 1122),       # int(187 / 4 * 24) = 1122
        (3, 5, "안녕하세요" + BOLD, 187 + 436),                    # int(187 / 15 * 35) = int(436.33); stretch 4 has no text
    ]
    assert plan["fades"] == [0, 0, 0, 0, 3600, 3600, 0]
    assert I.script_plan is S.script_plan


def test_script_plan_speed_fix_duration_and_no_cross_fade():
    stretches = [("main", BOLD), ("slow", BOLD), ("terse", LONG)]
    plan = S.script_plan(stretches, PROMPTS, speed=2.0, fix_duration=3.0, cross_fade_duration=0.0)
    # fix_duration: int(3.0 * 24000 / 256) = int(281.25) for every chunk; terse at the call's speed 2.0: max_chars 60 holds LONG whole
    assert [(v, s, d) for v, s, _, d in plan["items"]] == [(0, 0, 281), (1, 1, 281), (2, 2, 281)]
    assert plan["items"][2][2] == "hi. " + LONG and plan["fades"] == [0, 0, 0]
    # the call's speed reaches the voices without one of their own, and only those
    fast = S.script_plan(stretches[:2], PROMPTS, speed=2.0)
    assert [d for *_, d in fast["items"]] == [187 + 251, 187 + 1006]          # int(187 / 13 * 35 / 2.0) = int(251.73)
    with pytest.raises(ValueError, match="nobody"):
        S.script_plan([("nobody", "x")], PROMPTS)


@pytest.mark.parametrize("name", list(O.JOIN_CASES))
def test_join_plan_and_the_header_fold_are_the_host_join_bit_for_bit(name):
    runs, fade = O.JOIN_CASES[name]
    pieces, fades = O.flat(O.pieces_of(runs, seed=1), fade)
    want = O.host_join(O.pieces_of(runs, seed=1), fade)
    offs, ns, total = I.join_plan([len(x) for x in pieces], fades)
    assert total == len(want) and len(offs) == len(ns) == len(pieces)
    got = O.contract_fold(pieces, offs, ns, total)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_join_plan_restarts_its_running_length_with_every_run():
    offs, ns, total = I.join_plan([256, 256, 512, 5, 40], [0, 16, 16, 0, 16])
    assert ns == [0, 16, 16, 0, 5] and offs == [0, 240, 480, 992, 992] and total == 1032
    offs, ns, total = I.join_plan([30, 10, 5, 40], [0, 16, 16, 16])
    assert ns == [0, 10, 5, 16] and offs == [0, 20, 25, 14] and total == 54       # piece 3 starts before pieces 1 and 2
    # one run is cross_fade_plan
    assert I.join_plan([8, 3, 3, 3, 20], [0, 6, 6, 6, 6]) == I.cross_fade_plan([8, 3, 3, 3, 20], 6)
    # a fade on piece 0 has nothing in front of it
    assert I.join_plan([9, 9], [4, 4]) == ([0, 5], [0, 4], 14)
    with pytest.raises(ValueError):
        I.join_plan([1, 2], [0])


def test_wave_join_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "f5_hip.h")).read()
    assert "f5_wave_join <- infer_cli.py:363-415" in src, "the header's list of replaced reference interfaces lacks the entry"
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src), f"{NAME} is not declared in include/f5_hip.h"
    assert hasattr(_lib.load(), NAME), f"{NAME} is not exported by libf5hip.so"
    res, args = _lib.SIGNATURES[NAME]
    # (base, B, start_host, lens_host, fade_host, out, out_cap, out_len_host, stream)
    assert res is C.c_int32 and len(args) == 9 and args[6] is C.c_int64
    assert args[2] == C.POINTER(C.c_int64) and args[3] == args[4] == C.POINTER(C.c_int32) and args[7] == C.POINTER(C.c_int64)


def test_argument_checks_need_no_device():
    lib = _lib.load()
    base, out = C.c_void_p(4096), C.c_void_p(8192)         # never dereferenced: every call below is refused before a launch
    i64 = lambda v: (C.c_int64 * len(v))(*v)               # noqa: E731
    starts, lens, fades = i64([0, 10, 30]), _lib.int_array([10, 20, 15]), _lib.int_array([0, 4, 0])
    n = C.c_int64(-7)

    def refused(word, *args):
        assert lib.f5_wave_join(*args, C.byref(n), None) == F5_EINVAL
        msg = lib.f5_last_error()
        assert msg.startswith(b"f5_wave_join:") and word in msg, msg
        assert n.value == -7, "a refused call wrote out_len_host"

    for B in (0, -1, 65536):
        refused(b"B", base, B, starts, lens, fades, out, 100)
    refused(b"base", None, 3, starts, lens, fades, out, 100)
    refused(b"start_host", base, 3, None, lens, fades, out, 100)
    refused(b"lens_host", base, 3, starts, None, fades, out, 100)
    refused(b"fade_host", base, 3, starts, lens, None, out, 100)
    refused(b"out", base, 3, starts, lens, fades, None, 100)
    refused(b"lens_host[1]", base, 3, starts, _lib.int_array([10, 0, 15]), fades, out, 100)
    refused(b"fade_host[2]", base, 3, starts, lens, _lib.int_array([0, 4, -1]), out, 100)
    refused(b"start_host[0]", base, 3, i64([-1, 10, 30]), lens, fades, out, 100)
    refused(b"out_cap", base, 3, starts, lens, fades, out, 40)             # total = 10 + 20 - 4 + 15 = 41


def test_driver_refusals_come_before_a_device_is_touched():
    import f5_tts_amd as P

    class Model:
        _tokenizer_type = "kor_allophone"

    voices = {"main": dict(ref_audio=(None, 24000), ref_text="hello there.")}
    with pytest.raises(NotImplementedError, match="text_tokenizer"):
        I.synthesize_script(Model(), P.Vocos(P.config.VOCOS_TINY), voices, "words")
    Model._tokenizer_type = "custom"
    with pytest.raises(NotImplementedError, match="decode_ragged"):
        I.synthesize_script(Model(), P.BigVGAN(P.config.BIGVGAN_TINY), voices, "words")
    with pytest.raises(ValueError, match="default voice"):
        I.synthesize_script(Model(), P.Vocos(P.config.VOCOS_TINY), {"a": voices["main"]}, "words")
    with pytest.raises(ValueError, match="parse_script"):
        I.synthesize_script(Model(), P.Vocos(P.config.VOCOS_TINY), voices, "  ")
    with pytest.raises(RuntimeError, match="GPU"):
        import torch
        I.wave_join([torch.zeros(4)], [0])
