"""Host arithmetic of the multi-voice script (the reference's infer/infer_cli.py:363-415, the "Multi-Speech" tab of
infer_gradio.py): from a text with [voice] tags to tagged stretches, and from there to the flat list of items that run as ragged
batches and the fade each item's waveform asks of f5_wave_join.  Pure Python: the prompts are infer.prepare_voices', the
sampling and the join infer.synthesize_script's."""
from __future__ import annotations

import re

from .config import SAMPLE_RATE

_SPLIT = re.compile(r"(?=\[\w+\])")     # before every [word]: \w is Unicode's, so a Hangul name is a tag and "[a b]" is not
_TAG = re.compile(r"\[(\w+)\]")


def parse_script(text: str, voices, default: str = "main") -> list[tuple[str, str]]:
    """The grammar of infer_cli.py:363-383: the text is split before every `[\\w+]` tag and blank stretches are dropped; a
    stretch's leading tag names its voice -- no tag, or a name that is not in `voices`, means `default` -- then every tag is
    removed from the stretch and the text stripped (a stretch that was a tag alone keeps its place with an empty text, as in
    the reference's loop).  Returns [(voice, text)] in script order; ValueError when nothing is left."""
    out = []
    for stretch in _SPLIT.split(text):
        if not stretch.strip():
            continue
        match = _TAG.match(stretch)
        voice = match[1] if match else default
        if voice not in voices:
            voice = default
        out.append((voice, _TAG.sub("", stretch).strip()))
    if not out:
        raise ValueError("parse_script: the script has no text")
    return out


def script_plan(stretches, prompts, *, speed: float = 1.0, fix_duration=None, cross_fade_duration: float = 0.15) -> dict:
    """What infer_process and infer_batch_process compute on the host for every stretch, for the whole script at once.
    stretches: parse_script's return; prompts: {voice: dict(seconds=, samples=, ref_text=, speed=optional)} -- the prompt's
    length in seconds as infer_process sees it (frames / rate of the raw or clipped audio), its sample count at 24 kHz, its text,
    and the voice's own speed, which stands in for `speed` where given (infer_cli.py:382).  Per stretch: max_chars as
    infer_process writes it, chunk_text, then text_numerics per chunk (local_speed, the duration formula, the trailing-space
    rule).  Returns dict(items, fades): items is the flat list in script order of (voice index into list(prompts), stretch index,
    text = prompt text + chunk, duration in mel frames); fades[i] is 0 for a stretch's first chunk and
    int(cross_fade_duration * 24000) for its others, 0 everywhere when cross_fade_duration <= 0."""
    from .infer import chunk_text, text_numerics   # (infer re-exports this module's functions)

    order = {name: i for i, name in enumerate(prompts)}
    fade = int(cross_fade_duration * SAMPLE_RATE) if cross_fade_duration > 0 else 0
    items, fades = [], []
    for s, (voice, text) in enumerate(stretches):
        if voice not in order:
            raise ValueError(f"script_plan: stretch {s} is spoken by {voice!r}, which has no prompt")
        p = prompts[voice]
        own = p.get("speed")
        own = speed if own is None else own
        max_chars = int(len(p["ref_text"].encode("utf-8")) / p["seconds"] * (22 - p["seconds"]) * own)
        for c, chunk in enumerate(chunk_text(text, max_chars=max_chars)):
            rtext, _ref_len, duration = text_numerics(p["samples"], p["ref_text"], chunk, own, fix_duration)
            items.append((order[voice], s, rtext + chunk, duration))
            fades.append(fade if c > 0 else 0)
    return dict(items=items, fades=fades)
