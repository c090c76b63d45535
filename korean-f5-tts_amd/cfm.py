"""Drop-in for the reference's `CFM` (model/cfm.py:34-302) in inference mode: same constructor keywords, same
`sample()` and `forward()` signatures and return values, same attributes read by callers (`.transformer`, `.mel_spec`,
`.vocab_char_map`, `.device`, `.dim`, `.num_channels`).  Argument handling (cfm.py:103-158, 196-216, 219-229) is
host-side Python; the ODE solve itself (cfm.py:160-191, 218) is ONE call into the HIP engine (f5_sample_ode), with
odeint_kwargs["method"] "euler" or "midpoint" (torchdiffeq's fixed-grid solvers; midpoint makes 2 evaluations per step).
`forward` (cfm.py:231-302) is the teacher-forced flow-matching loss, one call into the engine too (f5_flow_loss), under no_grad:
a held-out loss for model selection.  Training -- gradients, an optimizer, a trainer -- is out of scope.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pad_sequence

from .utils import default, exists, get_epss_timesteps, lens_to_mask, list_str_to_idx, list_str_to_tensor, span_from_frac_lengths


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


def item_settings(steps, cfg_strength, sway_sampling_coef, seed, batch: int) -> tuple[list, list, list, list]:
    """The four sampler settings of sample_items() / sample_span(), each as a list of `batch` entries."""
    return ([int(v) for v in per_item("steps", steps, batch)], [float(v) for v in per_item("cfg_strength", cfg_strength, batch)],
            per_item("sway_sampling_coef", sway_sampling_coef, batch), per_item("seed", seed, batch))


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


class SampleInputs(NamedTuple):
    """What CFM's three sampler methods make of their shared arguments before anything differs between them."""
    cond: torch.Tensor        # f32 [B, cond_seq_len, mel] on the model's device
    text_cpu: torch.Tensor    # long [B, nt], -1 padded
    cond_mask: torch.Tensor   # bool [B, N] on the host: the prompt frames that are kept (lens, less the edit_mask's spans)
    duration: torch.Tensor    # long [B] on the host (clamp_durations)
    N: int
    batch: int
    cond_seq_len: int


class SpanResult:
    """What CFM.sample_span returns: `out` [B, N, mel] (an item's result once it is done), `state` [B, N, mel] (the raw ODE state:
    the next call's prev[0]) and `done`, a list of B bools, true where the item's last step was run."""

    def __init__(self, out, state, done):
        self.out, self.state, self.done = out, state, done


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

    def _flow_inputs(self, inp, text, lens):
        """The argument handling forward() and flow_loss() share (cfm.py:239-258): (mel as given or computed, text long [B, nt] on
        the host, lens long [B] on the host)."""
        self.eval()
        if inp.ndim == 2:  # raw wave -> mel (cfm.py:240-243)
            inp = self.mel_spec(inp.to(self.device))
            inp = inp.permute(0, 2, 1)
            assert inp.shape[-1] == self.num_channels
        batch, seq_len = inp.shape[:2]
        if isinstance(text, list):
            text = list_str_to_idx(text, self.vocab_char_map) if exists(self.vocab_char_map) else list_str_to_tensor(text)
            assert text.shape[0] == batch
        if not exists(lens):
            lens = torch.full((batch,), seq_len, dtype=torch.long)
        return inp, text.to("cpu", torch.long), torch.as_tensor(lens).to("cpu", torch.long)

    @staticmethod
    def _loss_of(sq_sum, count, mel: int):
        """cfm.py:299-302 from the engine's per-item sums: the mean over the selected elements of the whole batch, f32; NaN when
        nothing is selected, as the reference's mean over nothing is.  Device ops only."""
        return (sq_sum.sum() / (count.sum().to(torch.float64) * mel)).to(torch.float32)

    @torch.no_grad()
    def forward(self, inp, text, *, lens=None, noise_scheduler: str | None = None):
        """The reference's CFM.forward (cfm.py:231-302) in inference mode: one teacher-forced backbone evaluation at a random time
        with a random span of the conditioning zeroed, and the mean squared error against the flow x1 - x0 over that span.
        Returns (loss, cond, pred) as the reference does; no gradient is recorded.  The draws are made where `noise_device` says,
        in the reference's order (frac_lengths.uniform_, rand_like, randn_like, rand, random() twice): with noise_device="cpu" the
        same torch.manual_seed / random.seed give the reference's CPU draws.  One engine call (f5_flow_loss)."""
        from random import random
        inp, text_cpu, lens = self._flow_inputs(inp, text, lens)
        batch, seq_len = inp.shape[:2]
        nd = self._noise_device
        lens_d = lens.to(nd)
        frac_lengths = torch.zeros((batch,), device=nd).float().uniform_(*self.frac_lengths_mask)
        start, end = span_from_frac_lengths(lens_d, frac_lengths)
        end = torch.minimum(end, lens_d)   # rand_span_mask &= mask (cfm.py:264-265): one interval inside [0, len)
        x0 = torch.randn(inp.shape, dtype=torch.float32, device=nd)   # randn_like(x1)
        time = torch.rand((batch,), dtype=torch.float32, device=nd)
        drop_audio_cond = random() < self.audio_drop_prob
        drop_text = False
        if random() < self.cond_drop_prob:
            drop_audio_cond = drop_text = True
        span = list(zip(start.tolist(), end.tolist()))
        sq_sum, count, pred, cond, _ = self.transformer.engine().flow_loss(
            inp, x0, text_cpu, time.tolist(), span, lens=lens.tolist(), drop_audio_cond=drop_audio_cond, drop_text=drop_text,
            want_frame_err=False)
        return self._loss_of(sq_sum, count, self.num_channels), cond, pred

    @torch.no_grad()
    def flow_loss(self, mel, text, lens, *, time, span, x0, drop_audio_cond=False, drop_text=False):
        """forward() with every draw supplied by the caller: time (B floats), span (B (start, end) frame pairs inside [0, lens[b]])
        and the noise x0 [B, N, mel].  Returns (loss, per_item f32[B] -- NaN where an item's span is empty --, pred, cond,
        frame_err f32[B, N]: a frame's mean squared error inside the span, 0 outside), all on the device."""
        mel, text_cpu, lens = self._flow_inputs(mel, text, lens)
        time = [float(v) for v in (time.tolist() if isinstance(time, torch.Tensor) else time)]
        span = [(int(s), int(e)) for s, e in (span.tolist() if isinstance(span, torch.Tensor) else span)]
        sq_sum, count, pred, cond, frame_err = self.transformer.engine().flow_loss(
            mel, x0, text_cpu, time, span, lens=lens.tolist(), drop_audio_cond=drop_audio_cond, drop_text=drop_text)
        per_item = (sq_sum / (count.to(torch.float64) * self.num_channels)).to(torch.float32)
        return self._loss_of(sq_sum, count, self.num_channels), per_item, pred, cond, frame_err

    def load_state_dict(self, sd, strict=True, assign=False):
        """Accepts the reference's CFM state dict (`transformer.*` keys, optional `mel_spec.*` buffers): the backbone
        keeps the weights; everything else in a CFM is parameter-free."""
        return self.transformer.load_state_dict(sd, strict=strict)

    def state_dict(self, *a, **k):
        return {"transformer." + n: t for n, t in self.transformer.state_dict().items()}

    def _prepare(self, cond, text, duration, lens, max_duration, edit_mask) -> SampleInputs:
        """The argument handling sample(), sample_items() and sample_span() share (cfm.py:103-147)."""
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
        # cond = F.pad(cond, (0, 0, 0, N - cond_seq_len)) (cfm.py:145) happens inside the engine: the prompt goes down
        # unpadded with its frame count; no_ref_audio (cfm.py:146-147: an all-zero cond) is "zero prompt frames"
        cond_mask = F.pad(cond_mask, (0, N - cond_mask.shape[-1]), value=False)   # (host tensor)
        return SampleInputs(cond, text_cpu, cond_mask, duration, N, batch, cond_seq_len)

    @property
    def _noise_device(self):
        return self.noise_device if self.noise_device == "cpu" else self.device

    def _finish(self, out, vocoder):
        self.transformer.clear_cache()
        if exists(vocoder):
            out = vocoder(out.permute(0, 2, 1))
        return out

    @torch.no_grad()
    def sample(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None,
               seed: int | None = None, max_duration=65536, vocoder=None, use_epss=True, no_ref_audio=False,
               duplicate_test=False, t_inter=0.1, edit_mask=None):
        a = self._prepare(cond, text, duration, lens, max_duration, edit_mask)
        if duplicate_test:
            test_cond = F.pad(a.cond, (0, 0, a.cond_seq_len, a.N - 2 * a.cond_seq_len), value=0.0)

        # noise (cfm.py:196-201): same seed for every sample, drawn per sample at its own length, zero padded
        y0 = []
        for dur in a.duration.tolist():
            if exists(seed):
                torch.manual_seed(seed)
            y0.append(torch.randn(dur, self.num_channels, device=self._noise_device, dtype=torch.float32))
        y0 = pad_sequence(y0, padding_value=0, batch_first=True)   # stays where it was drawn; Engine.sample copies it asynchronously

        t_start = 0
        if duplicate_test:
            t_start = t_inter
            y0 = (1 - t_start) * y0.to(self.device) + t_start * test_cond
            steps = int(steps * (1 - t_start))
        if t_start == 0 and use_epss:
            t = get_epss_timesteps(steps, device="cpu", dtype=torch.float32)
        else:
            t = torch.linspace(t_start, 1, steps + 1, dtype=torch.float32)
        if sway_sampling_coef is not None:
            t = t + sway_sampling_coef * (torch.cos(torch.pi / 2 * t) - 1 + t)

        eng = self.transformer.engine()
        out, trajectory = eng.sample(None if no_ref_audio else a.cond, a.cond_mask, y0, a.text_cpu, t.tolist(), cfg_strength,
                                     lens=a.duration.tolist() if a.batch > 1 else None, want_traj=True,
                                     method=self.odeint_kwargs.get("method", "euler"))
        return self._finish(out, vocoder), trajectory

    def _no_mmdit(self):
        if getattr(self.transformer, "backbone_name", None) == "MMDiT":
            raise NotImplementedError("per-item and sliced solves are built for the DiT and UNetT backbones, not the MMDiT")

    @torch.no_grad()
    def sample_items(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None, seed=None,
                     use_epss=True, max_duration=65536, vocoder=None, no_ref_audio=False, edit_mask=None):
        """sample() with per-item settings: `steps`, `cfg_strength`, `sway_sampling_coef` and `seed` each take one value for the batch or
        a sequence of one value per item (entries of the last two may be None).  One engine call (f5_sample_items) runs the batch for
        max(steps) steps; an item with fewer steps keeps its final state from then on.  Returns (out, trajectory[max(steps) + 1, B, N, mel])."""
        self._no_mmdit()
        a = self._prepare(cond, text, duration, lens, max_duration, edit_mask)
        steps_i, cfg_i, sway_i, seed_i = item_settings(steps, cfg_strength, sway_sampling_coef, seed, a.batch)
        y0 = item_noise(a.duration.tolist(), seed_i, self.num_channels, self._noise_device)
        grids = item_time_grids(steps_i, sway_i, use_epss)

        eng = self.transformer.engine()
        out, trajectory = eng.sample_items(None if no_ref_audio else a.cond, a.cond_mask, y0, a.text_cpu, [t.tolist() for t in grids], cfg_i,
                                           lens=a.duration.tolist() if a.batch > 1 else None, want_traj=True,
                                           method=self.odeint_kwargs.get("method", "euler"))
        return self._finish(out, vocoder), trajectory

    @torch.no_grad()
    def sample_span(self, cond, text, duration, *, lens=None, steps=32, cfg_strength=1.0, sway_sampling_coef=None, seed=None, start, count,
                    prev=None, use_epss=True, max_duration=65536, no_ref_audio=False, edit_mask=None):
        """Some steps of a sample_items() solve, so that a batch can be re-formed between two calls: item b, whose settings are
        sample_items' (`steps`, `cfg_strength`, `sway_sampling_coef`, `seed`: one value or one per item), runs its steps
        [start[b], min(start[b] + count, steps[b])) in one engine call (f5_sample_span).  prev = (state, rows): the `state` a
        previous call returned and, per item, its row there, or -1 for an item that begins here -- such an item has start 0 and
        gets item_noise's draw for it alone.  prev=None: every item begins here.  The batch runs at N = max(duration) of the items
        it holds now.  The grids are item_time_grids' grids, sliced.  Returns a SpanResult: `out` (where(cond_mask, cond, state):
        an item's result once it is `done`), `state` [B, N, mel] and `done`, per item whether its last step was run."""
        self._no_mmdit()
        a = self._prepare(cond, text, duration, lens, max_duration, edit_mask)
        batch, durs = a.batch, a.duration.tolist()
        steps_i, cfg_i, sway_i, seed_i = item_settings(steps, cfg_strength, sway_sampling_coef, seed, batch)
        count = int(count)
        if count < 1:
            raise ValueError(f"sample_span: count = {count} (a slice runs at least one step)")
        start_i = [int(v) for v in start]
        if len(start_i) != batch:
            raise ValueError(f"sample_span: start has {len(start_i)} entries for a batch of {batch}")
        state, rows = (None, [-1] * batch) if prev is None else prev
        rows = [int(r) for r in rows]
        if len(rows) != batch:
            raise ValueError(f"sample_span: rows has {len(rows)} entries for a batch of {batch}")
        for b in range(batch):
            if not 0 <= start_i[b] < steps_i[b]:
                raise ValueError(f"sample_span: item {b}: start = {start_i[b]} outside [0, steps = {steps_i[b]})")
            if rows[b] < 0 and start_i[b] != 0:
                raise ValueError(f"sample_span: item {b} begins here (row -1) but start = {start_i[b]}")
            if rows[b] >= 0 and (state is None or state.shape[1] < durs[b]):
                have = "no previous state" if state is None else f"the previous state has {state.shape[1]} frames"
                raise ValueError(f"sample_span: item {b} continues row {rows[b]} at {durs[b]} frames, but {have}")
        run = [min(count, n - s) for n, s in zip(steps_i, start_i)]
        # the sub-grids: the items' own grids, sliced on the host (nothing is computed again in another arithmetic)
        grids = [t[s:s + r + 1] for t, s, r in zip(item_time_grids(steps_i, sway_i, use_epss), start_i, run)]

        fresh = [b for b in range(batch) if rows[b] < 0]
        y_new = None
        if fresh:
            drawn = item_noise([durs[b] for b in fresh], [seed_i[b] for b in fresh], self.num_channels, self._noise_device)
            y_new = torch.zeros(batch, a.N, self.num_channels, device=drawn.device, dtype=torch.float32)
            y_new[fresh, :drawn.shape[1]] = drawn

        eng = self.transformer.engine()
        out, new_state = eng.sample_span(None if no_ref_audio else a.cond, a.cond_mask, y_new, state, rows, a.text_cpu,
                                         [t.tolist() for t in grids], cfg_i, lens=durs if batch > 1 else None,
                                         method=self.odeint_kwargs.get("method", "euler"))
        self.transformer.clear_cache()
        return SpanResult(out, new_state, [s + r == n for s, r, n in zip(start_i, run, steps_i)])
