"""Yardsticks of the multi-voice script tests (test_script.py, test_script_gpu.py), none of which uses the code under test:
the reference's tag loop restated literally (infer/infer_cli.py:363-383), the per-piece fold that include/f5_hip.h documents for
f5_wave_join in float64 numpy, the host form of a join (cross_fade_concat per run, concatenated) and the cases both files run."""
import re

import numpy as np

from f5_tts_amd import infer as I

SR = 24000


def reference_parse(gen_text, voices, main="main"):
    """infer_cli.py:363-383 up to the infer_process call: (voice, gen_text_) per stretch the loop does not skip."""
    out = []
    reg1 = r"(?=\[\w+\])"
    chunks = re.split(reg1, gen_text)
    reg2 = r"\[(\w+)\]"
    for text in chunks:
        if not text.strip():
            continue
        match = re.match(reg2, text)
        if match:
            voice = match[1]
        else:
            voice = main
        if voice not in voices:
            voice = main
        text = re.sub(reg2, "", text)
        out.append((voice, text.strip()))
    return out


# name -> (runs: the piece lengths of every run, fade in samples asked by every piece that is not the first of its run)
JOIN_CASES = {
    "later_run_shorter_than_the_fade": ([[256, 256, 512], [5, 40]], 16),   # run-local R: n = 5; a global running length gives 16
    "piece_starts_before_the_one_in_front": ([[30, 10, 5, 40]], 16),
    "one_sample_pieces": ([[1, 1, 1], [1], [1, 1]], 4),
    "fade_zero_everywhere": ([[50], [60], [7]], 0),
    "single_piece": ([[777]], 100),
    "three_voices": ([[300, 200], [40], [8, 3, 3, 3, 20], [100, 100]], 6),
}


def pieces_of(runs, seed=0):
    g = np.random.default_rng(seed)
    return [[g.standard_normal(n).astype(np.float32) for n in run] for run in runs]


def flat(runs, fade):
    """(pieces in order, the fade each asks for): 0 opens a run."""
    return [x for run in runs for x in run], [fade if k > 0 else 0 for run in runs for k in range(len(run))]


def host_join(runs, fade):
    """What the reference computes: cross_fade_concat of every run alone, concatenated (np.concatenate promotes), cast to f32."""
    assert int(fade / SR * SR) == fade, "fade / 24000 does not survive cross_fade_concat's int(duration * 24000)"
    return np.concatenate([I.cross_fade_concat(run, fade / SR) for run in runs]).astype(np.float32)


def contract_fold(pieces, offs, ns, total):
    """include/f5_hip.h's fold for f5_wave_join given a plan: per output sample over the covering pieces in ascending i, in
    double, rounded to f32 once.  Pieces are taken in ascending order over whole arrays, which is that order for every sample;
    numpy multiplies and adds separately.  The weights are written out (no np.linspace)."""
    v = np.zeros(total, np.float64)
    for x, off, n in zip(pieces, offs, ns):
        x = x.astype(np.float64)
        if n > 0:
            j = np.arange(n, dtype=np.float64)
            step = 1.0 / (n - 1) if n > 1 else 0.0
            fi, fo = j * step + 0.0, j * (-step) + 1.0
            if n == 1:
                fi[0], fo[0] = 0.0, 1.0
            else:
                fi[n - 1], fo[n - 1] = 1.0, 0.0
            v[off:off + n] = v[off:off + n] * fo + x[:n] * fi
        v[off + n:off + len(x)] = x[n:]
    return v.astype(np.float32)
