"""Host restatements that the speech-editing tests compare against, written from the feature's description and sharing no code
with the product (korean-f5-tts_amd/edit.py, csrc/edit.hip):
  frame_map            the edited timeline frame by frame: for every output frame its source frame, or -1 for an EDIT frame;
  expand               a plan's segments as such a per-frame list (so that the two can be compared);
  cat_construction     the torch.cat chain of the editing script, on any [1, T, C] mel: a second, independent construction of
                       the conditioning and the mask;
  assemble             cond [B, D_max, C] frame by frame from per-frame maps;
  splice_fold          the waveform splice sample by sample in float64.
Plain loops on purpose: nothing here is fast, and the cases are small."""
import numpy as np
import torch

SR, HOP = 24000, 256


def frame_map(n_frames, parts, fix_duration=None, sample_rate=SR, hop=HOP):
    out, offset = [], 0
    for k, (start, end) in enumerate(parts):
        dur = (end - start) if fix_duration is None else fix_duration[k]
        start_frame = round(start * sample_rate / hop)
        end_frame = round(end * sample_rate / hop)
        part_frames = round(dur * sample_rate / hop)
        for f in range(offset, start_frame):
            out.append(f)
        for _ in range(part_frames):
            out.append(-1)
        offset = end_frame
    for f in range(offset, n_frames):
        out.append(f)
    return out


def expand(plan):
    """A plan (segments, D) frame by frame; also checks that the segments tile [0, D) in order with no empty one."""
    segments, D = plan
    out = []
    for dst, src, frames in segments:
        assert frames > 0, f"zero-length segment {(dst, src, frames)}"
        assert dst == len(out), f"segment {(dst, src, frames)} does not start where the previous one ends ({len(out)})"
        assert src >= -1
        for j in range(frames):
            out.append(-1 if src < 0 else src + j)
    assert len(out) == D, f"the segments cover {len(out)} frames, D = {D}"
    return out


def cat_construction(original_mel, parts, fix_duration=None, sample_rate=SR, hop=HOP):
    """original_mel [1, T, C] -> (mel_cond [1, D, C], edit_mask bool [1, D]) by concatenation, part by part."""
    C = original_mel.shape[2]
    kw = dict(device=original_mel.device)
    mel_cond = torch.zeros(1, 0, C, **kw)
    mask = torch.zeros(1, 0, dtype=torch.bool)
    fix = list(fix_duration) if fix_duration is not None else None
    offset = 0
    for start, end in parts:
        dur = end - start if fix is None else fix.pop(0)
        sf, ef = round(start * sample_rate / hop), round(end * sample_rate / hop)
        pf = round(dur * sample_rate / hop)
        mel_cond = torch.cat((mel_cond, original_mel[:, offset:sf, :], torch.zeros(1, pf, C, **kw)), dim=1)
        mask = torch.cat((mask, torch.ones(1, sf - offset, dtype=torch.bool), torch.zeros(1, pf, dtype=torch.bool)), dim=-1)
        offset = ef
    mel_cond = torch.cat((mel_cond, original_mel[:, offset:, :]), dim=1)
    mask = torch.nn.functional.pad(mask, (0, mel_cond.shape[1] - mask.shape[-1]), value=True)
    return mel_cond, mask


def assemble(mels, maps):
    """mels: list of [T_i, C] host tensors; maps: per-frame source lists -> [B, D_max, C], +0.0 wherever nothing is copied."""
    D_max = max(len(m) for m in maps)
    out = torch.zeros(len(mels), D_max, mels[0].shape[1])
    for b, (mel, fm) in enumerate(zip(mels, maps)):
        for d, src in enumerate(fm):
            if src >= 0:
                out[b, d] = mel[src]
    return out


def linspace_weights(j, m):
    """(fi, fo) = (linspace(0, 1, m)[j], linspace(1, 0, m)[j]) as numpy computes them, in float64."""
    if m == 1:
        return np.float64(0.0), np.float64(1.0)
    if j == m - 1:
        return np.float64(1.0), np.float64(0.0)
    step = np.float64(1.0) / np.float64(m - 1)
    return np.float64(j) * step + np.float64(0.0), np.float64(j) * (-step) + np.float64(1.0)


def splice_fold(g, a, keeps, hop, cf, width=None):
    """g: f32 numpy [L] (decoded), a: f32 numpy [n] (original), keeps: (dst, src, frames) of the KEEP segments -> f32 [width]
    (default L), sample by sample."""
    L, n = len(g), len(a)
    width = L if width is None else width
    out = np.zeros(width, dtype=np.float32)
    out[:L] = g
    for dst, src, frames in keeps:
        p0 = dst * hop
        p1 = min((dst + frames) * hop, L, p0 + n - src * hop)
        if p1 <= p0:
            continue
        m = min(cf, (p1 - p0) // 2)
        for p in range(p0, p1):
            q = src * hop + (p - p0)
            j = None
            if p0 > 0 and p - p0 < m:
                j = p - p0
            elif p1 < L and p1 - 1 - p < m:
                j = p1 - 1 - p
            if j is None:
                out[p] = a[q]
            else:
                fi, fo = linspace_weights(j, m)
                out[p] = np.float32(np.float64(g[p]) * fo + np.float64(a[q]) * fi)
    return out


def keeps_of(plan):
    return [s for s in plan[0] if s[1] >= 0]


# name -> (n_frames, parts_to_edit, fix_duration): the plan cases the CPU and the GPU tests share.  93.75 frames per second.
PLAN_CASES = {
    "no_parts": (37, [], None),
    "part_from_frame_0": (64, [(0.0, 0.2)], None),                      # frames [0, 19)
    "part_to_the_last_frame": (64, [(0.4, 0.683)], None),               # round(64.03) = 64 = n_frames
    "adjacent_parts": (64, [(0.1, 0.3), (0.3, 0.5)], None),             # [9, 28) and [28, 47): an empty KEEP between them
    "fix_duration_longer": (64, [(0.2, 0.4)], [0.5]),
    "fix_duration_shorter": (64, [(0.2, 0.4)], [0.05]),
    "fix_duration_of_0_frames": (64, [(0.2, 0.4)], [0.004]),            # round(0.375) = 0: the span is cut out
    "ties_to_even": (700, [(2.0, 3.0), (6.0, 7.0)], None),              # starts at 187.5 -> 188 (odd k: up) and 562.5 -> 562 (even k: stays)
    "two_parts_fixed": (64, [(0.1, 0.2), (0.35, 0.6)], [0.15, 0.1]),
}
