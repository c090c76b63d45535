"""Host-side helpers of the sampler with the reference's names and behaviour (model/utils.py:32-37,53-58,92-106,
538-551).  Pure Python / torch-CPU bookkeeping; no model arithmetic happens here."""
from __future__ import annotations

import torch
from torch.nn.utils.rnn import pad_sequence


def exists(v):
    return v is not None


def default(v, d):
    return v if exists(v) else d


def lens_to_mask(t: torch.Tensor, length: int | None = None) -> torch.Tensor:
    if not exists(length):
        length = int(t.amax())
    seq = torch.arange(length, device=t.device)
    return seq[None, :] < t[:, None]


def mask_from_start_end_indices(seq_len: torch.Tensor, start: torch.Tensor, end: torch.Tensor) -> torch.Tensor:
    """bool [B, max(seq_len)]: frame n of item b is inside [start[b], end[b])   (utils.py:61-66)."""
    seq = torch.arange(int(seq_len.max()), device=start.device).long()
    return (seq[None, :] >= start[:, None]) & (seq[None, :] < end[:, None])


def span_from_frac_lengths(seq_len: torch.Tensor, frac_lengths: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The random training span of utils.py:69-75 as (start, end), long [B]: lengths = (frac * seq_len).long(), start =
    (max_start * rand_like(frac)).long().clamp(min=0), end = start + lengths.  Draws `rand_like` where frac_lengths lives, as
    the reference does.  end <= seq_len, so the reference's `rand_span_mask & mask` is this one interval."""
    lengths = (frac_lengths * seq_len).long()
    max_start = seq_len - lengths
    rand = torch.rand_like(frac_lengths)
    start = (max_start * rand).long().clamp(min=0)
    return start, start + lengths


def mask_from_frac_lengths(seq_len: torch.Tensor, frac_lengths: torch.Tensor) -> torch.Tensor:
    """utils.py:69-77."""
    start, end = span_from_frac_lengths(seq_len, frac_lengths)
    return mask_from_start_end_indices(seq_len, start, end)


def list_str_to_tensor(text: list[str], padding_value=-1) -> torch.Tensor:
    tensors = [torch.tensor([*bytes(t, "UTF-8")]) for t in text]
    return pad_sequence(tensors, padding_value=padding_value, batch_first=True)


def list_str_to_idx(text, vocab_char_map: dict[str, int], padding_value=-1) -> torch.Tensor:
    tensors = [torch.tensor([vocab_char_map.get(c, 0) for c in t]) for t in text]
    return pad_sequence(tensors, padding_value=padding_value, batch_first=True)


_EPSS_TABLE = {
    5: [0, 2, 4, 8, 16, 32],
    6: [0, 2, 4, 6, 8, 16, 32],
    7: [0, 2, 4, 6, 8, 16, 24, 32],
    10: [0, 2, 4, 6, 8, 12, 16, 20, 24, 28, 32],
    12: [0, 2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32],
    16: [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32],
}


def get_epss_timesteps(n, device="cpu", dtype=torch.float32):
    t = _EPSS_TABLE.get(n, [])
    if not t:
        return torch.linspace(0, 1, n + 1, device=device, dtype=dtype)
    return (1 / 32) * torch.tensor(t, device=device, dtype=dtype)


def load_vocab(path: str) -> tuple[dict[str, int], int]:
    """vocab.txt -> ({char: idx}, vocab_size) exactly as get_tokenizer's custom/pinyin branch (utils.py:112-149)."""
    with open(path, "r", encoding="utf-8") as f:
        m = {}
        for i, ch in enumerate(f):
            m[ch[:-1]] = i
    return m, len(m)


def configure_host_threads(n: int = 1) -> None:
    """The engine's host side is a handful of tiny CPU tensor ops per call (seeded noise draw, pads, masks).  torch's default
    intra-op pool has one thread per logical CPU of the HOST, not of the job's share, so on a shared or multi-rank node
    those ops wake an oversubscribed OpenMP team and its spinning workers starve the HIP runtime's submission thread:
    occasional 100-200 ms utterances instead of 34 ms (tools/stall_probe.py).  Serving loops should call this once."""
    import torch

    torch.set_num_threads(n)

