"""The contract of f5_wave_emit (include/f5_hip.h) for the tests, as the composition of the two committed yardsticks and nothing
else: script_oracle.contract_fold on the join plan of a stream's pieces, cut to `settled`, then deliver_oracle.deliver -- plus
the byte placement of a call (the running byte total rounded up to 16) restated in plain integers."""
import numpy as np

import deliver_oracle as D
import script_oracle as J

from f5_tts_amd import infer as I

WIDTH = {"f32": 4, "s16": 2}


def joined(pieces, fades):
    """J_s: the float64 fold of the pieces (f32 numpy arrays) over join_plan, rounded to f32 once."""
    offs, ns, total = I.join_plan([len(x) for x in pieces], list(fades))
    return J.contract_fold(pieces, offs, ns, total)


def emit(pieces, fades, settled, final, rng, out_rate, sample_format):
    """The samples [o0, o1) stream s must receive: f32 or int16 numpy."""
    whole = joined(pieces, fades)
    assert 0 <= settled <= len(whole)
    return D.deliver(whole[:settled], out_rate, sample_format, final, rng[0], rng[1])


def placement(ranges, formats):
    """(byte offset per stream, bytes in all)."""
    starts, run = [], 0
    for (o0, o1), fmt in zip(ranges, formats):
        run = (run + 15) // 16 * 16
        starts.append(run)
        run += (o1 - o0) * WIDTH[fmt]
    return starts, run


def as_bytes(samples):
    return np.ascontiguousarray(samples).view(np.uint8)
