"""Drop-in for the reference's `CFM` inference surface (model/cfm.py:34-229): same constructor keywords, same
`sample()` signature and return value, same attributes read by callers (`.transformer`, `.mel_spec`,
`.vocab_char_map`, `.device`, `.dim`, `.num_channels`).  Argument handling (cfm.py:103-158, 196-216, 219-229) is
host-side Python; the ODE solve itself (cfm.py:160-191, 218) is ONE call into the HIP engine (f5_sample_ode), with
odeint_kwargs["method"] "euler" or "midpoint" (torchdiffeq's fixed-grid solvers; midpoint makes 2 evaluations per step).
Training (`forward`, cfm.py:231-302) is out of scope.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pad_sequence

from .utils import default, exists, get_epss_timesteps, lens_to_mask, list_str_to_idx, list_str_to_tensor


def clamp_durations(text: torch.Tensor, lens: torch.Tensor, duration, max_duration=65536) -> torch.Tensor:
    """The per-item total lengths sample() runs at (cfm.py:125-141): at least one frame past the longer of the text and the
    prompt, at most max_duration.  text: CPU long [B, nt] padded with -1; lens: CPU long [B]; duration: int or long [B]."""
    if isinstance(duration, int):
        duration = torch.full((lens.shape[0],), duration, dtype=torch.long)
    duration = duration.to("cpu", torch.long)
    duration = torch.maximum(torch.maximum((text != -1).sum(dim=-1), lens) + 1, duration)
    return duration.clamp(max=max_duration)


def per_item(name: str, value, batch: int) -> list:
    """A sampler setting as a list of `batch` entries: a scalar (or None) is every item's value, a sequence is one value per item."""
    if isinstance(value, (list, tuple)) or (isinstance(value, torch.Tensor) and value.ndim > 0):
        vals = [v.item() if isinstance(v, torch.Tensor) else v for v in value]
        if len(vals) != batch:
            raise ValueError(f"sample_items: {name} has {len(vals)} entries for a batch of {batch}")
        return vals
    return [value.item() if isinstance(value, torch.Tensor) else value] * batch


def is_per_item(*values) -> bool:
    """Whether any of the sampler settings is given per item (a sequence) rather than once for the batch."""
    return any(isinstance(v, (list, tuple)) or (isinstance(v, torch.Tensor) and v.ndim > 0) for v in values)


def item_time_grids(steps: list, sway: list, use_epss=True) -> list[torch.Tensor]:
    """One time grid per item: sample()'s own host arithmetic (cfm.py:211-216) with the item's step count and sway coefficient."""
    grids = []
    for n, sw in zip(steps, sway):
        n = int(n)
        if n < 1:
            raise ValueError(f"sample_items: steps must be at least 1 (got {n})")
        t = get_epss_timesteps(n, device="cpu", dtype=torch.float32) if use_epss else torch.linspace(0, 1, n + 1, dtype=torch.float32)
        if sw is not None:
            t = t + sw * (torch.cos(torch.pi / 2 * t) - 1 + t)
        grids.append(t)
    return grids


def item_noise(durations: list, seeds: list, mel: int, device="cpu") -> torch.Tensor:
    """y0 of a batch whose items carry their own seeds (cfm.py:196-201 per item): drawn in item order, each at its own length after
    `manual_seed(seed)` when it has one, zero padded."""
    y0 = []
    for dur, seed in zip(durations, seeds):
        if exists(seed):
            torch.manual_seed(int(seed))
        y0.append(torch.randn(int(dur), mel, device=device, dtype=torch.float32))
    return pad_sequence(y0, padding_value=0, batch_first=True)


class CFM(nn.Module):
    def __init__(self, transformer: nn.Module, sigma=0.0, odeint_kwargs: dict = dict(method="euler"),
                 audio_drop_prob=0.3, cond_drop_prob=0.2, num_channels=None, mel_spec_module: nn.Module | None = None,
                 mel_spec_kwargs: dict = dict(), frac_lengths_mask=(0.7, 1.0), vocab_char_map=None):
        super().__init__()
        if odeint_kwargs.get("method", "euler") not in ("euler", "midpoint"):
            raise NotImplementedError(f"ODE method {odeint_kwargs.get('method')!r}: only the fixed-grid solvers "
                                      "'euler' (every shipped config) and 'midpoint' are built")
        self.frac_lengths_mask = frac_lengths_mask
        if mel_spec_module is None:
            from .mel import MelSpec
            mel_spec_module = MelSpec(**mel_spec_kwargs)
        self.mel_spec = mel_spec_module
        self.num_channels = default(num_channels, getattr(self.mel_spec, "n_mel_channels", 100))
        self.audio_drop_prob, self.cond_drop_prob = audio_drop_prob, cond_drop_prob
        self.transformer = transformer
        self.dim = transformer.dim
        self.sigma = sigma
        self.odeint_kwargs = odeint_kwargs
        self.vocab_char_map = vocab_char_map
        # The reference draws y0 with the generator of the model's device (cfm.py:196-201).  "cpu" reproduces the
        # reference's CPU path bit for bit (the parity target); "cuda" draws on the GPU generator instead.
        self.noise_device = "cpu"

    @property
    def device(self):
        return self.transformer.device

    def forward(self, *a, **k):
        raise NotImplementedError("training (cfm.py:231-302) is outside the inference hot path")

    def load_state_dict(self, sd, strict=True, assign=False):
        """Accepts the reference's CFM state dict (`transformer.*` keys, optional `mel_spec.*` buffers): the backbone
        keeps the weights; everything else in a CFM is parameter-free."""
        return self.transformer.load_state_dict(sd, strict=strict)

    def state_dict(self, *a, **k):
        return {"transformer." + n: t for n, t in self.transformer.state_dict().items()}

    @torch.no_grad()
    def sample(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None,
               seed: int | None = None, max_duration=65536, vocoder=None, use_epss=True, no_ref_audio=False,
               duplicate_test=False, t_inter=0.1, edit_mask=None):
        self.eval()
        device = self.device
        if cond.ndim == 2:  # raw wave -> mel (cfm.py:106-109)
            cond = self.mel_spec(cond.to(device))
            cond = cond.permute(0, 2, 1)
            assert cond.shape[-1] == self.num_channels
        cond = cond.to(device=device, dtype=torch.float32)
        batch, cond_seq_len = cond.shape[:2]
        if not exists(lens):
            lens = torch.full((batch,), cond_seq_len, dtype=torch.long)
        lens = lens.to("cpu", torch.long)

        if isinstance(text, list):
            text = list_str_to_idx(text, self.vocab_char_map) if exists(self.vocab_char_map) else list_str_to_tensor(text)
            assert text.shape[0] == batch
        text_cpu = text.to("cpu", torch.long)

        cond_mask = lens_to_mask(lens)
        if edit_mask is not None:
            cond_mask = cond_mask & edit_mask.to("cpu")
        duration = clamp_durations(text_cpu, lens, duration, max_duration)
        N = int(duration.amax())

        if duplicate_test:
            test_cond = F.pad(cond, (0, 0, cond_seq_len, N - 2 * cond_seq_len), value=0.0)
        # cond = F.pad(cond, (0, 0, 0, N - cond_seq_len)) (cfm.py:145) happens inside the engine: the prompt goes down
        # unpadded with its frame count; no_ref_audio (cfm.py:146-147: an all-zero cond) is "zero prompt frames"
        cond_mask = F.pad(cond_mask, (0, N - cond_mask.shape[-1]), value=False)   # (host tensor)

        # noise (cfm.py:196-201): same seed for every sample, drawn per sample at its own length, zero padded
        y0 = []
        for dur in duration.tolist():
            if exists(seed):
                torch.manual_seed(seed)
            y0.append(torch.randn(dur, self.num_channels, device=self.noise_device if self.noise_device == "cpu" else device,
                                  dtype=torch.float32))
        y0 = pad_sequence(y0, padding_value=0, batch_first=True)   # stays where it was drawn; Engine.sample copies it asynchronously

        t_start = 0
        if duplicate_test:
            t_start = t_inter
            y0 = (1 - t_start) * y0.to(device) + t_start * test_cond
            steps = int(steps * (1 - t_start))
        if t_start == 0 and use_epss:
            t = get_epss_timesteps(steps, device="cpu", dtype=torch.float32)
        else:
            t = torch.linspace(t_start, 1, steps + 1, dtype=torch.float32)
        if sway_sampling_coef is not None:
            t = t + sway_sampling_coef * (torch.cos(torch.pi / 2 * t) - 1 + t)

        eng = self.transformer.engine()
        out, trajectory = eng.sample(None if no_ref_audio else cond, cond_mask, y0, text_cpu, t.tolist(), cfg_strength,
                                     lens=duration.tolist() if batch > 1 else None, want_traj=True,
                                     method=self.odeint_kwargs.get("method", "euler"))
        self.transformer.clear_cache()
        if exists(vocoder):
            out = vocoder(out.permute(0, 2, 1))
        return out, trajectory

    @torch.no_grad()
    def sample_items(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None, seed=None,
                     use_epss=True, max_duration=65536, vocoder=None, no_ref_audio=False, edit_mask=None):
        """sample() with per-item settings: `steps`, `cfg_strength`, `sway_sampling_coef` and `seed` each take one value for the batch or
        a sequence of one value per item (entries of the last two may be None).  One engine call (f5_sample_items) runs the batch for
        max(steps) steps; an item with fewer steps keeps its final state from then on.  Returns (out, trajectory[max(steps) + 1, B, N, mel])."""
        self.eval()
        device = self.device
        if cond.ndim == 2:
            cond = self.mel_spec(cond.to(device))
            cond = cond.permute(0, 2, 1)
            assert cond.shape[-1] == self.num_channels
        cond = cond.to(device=device, dtype=torch.float32)
        batch, cond_seq_len = cond.shape[:2]
        steps_i = [int(v) for v in per_item("steps", steps, batch)]
        cfg_i = [float(v) for v in per_item("cfg_strength", cfg_strength, batch)]
        sway_i = per_item("sway_sampling_coef", sway_sampling_coef, batch)
        seed_i = per_item("seed", seed, batch)
        if not exists(lens):
            lens = torch.full((batch,), cond_seq_len, dtype=torch.long)
        lens = lens.to("cpu", torch.long)

        if isinstance(text, list):
            text = list_str_to_idx(text, self.vocab_char_map) if exists(self.vocab_char_map) else list_str_to_tensor(text)
            assert text.shape[0] == batch
        text_cpu = text.to("cpu", torch.long)

        cond_mask = lens_to_mask(lens)
        if edit_mask is not None:
            cond_mask = cond_mask & edit_mask.to("cpu")
        duration = clamp_durations(text_cpu, lens, duration, max_duration)
        N = int(duration.amax())
        cond_mask = F.pad(cond_mask, (0, N - cond_mask.shape[-1]), value=False)

        y0 = item_noise(duration.tolist(), seed_i, self.num_channels, self.noise_device if self.noise_device == "cpu" else device)
        grids = item_time_grids(steps_i, sway_i, use_epss)

        eng = self.transformer.engine()
        out, trajectory = eng.sample_items(None if no_ref_audio else cond, cond_mask, y0, text_cpu, [t.tolist() for t in grids], cfg_i,
                                           lens=duration.tolist() if batch > 1 else None, want_traj=True,
                                           method=self.odeint_kwargs.get("method", "euler"))
        self.transformer.clear_cache()
        if exists(vocoder):
            out = vocoder(out.permute(0, 2, 1))
        return out, trajectory
