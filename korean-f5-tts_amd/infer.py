"""Inference harness around the hot path, with the reference's function names and behaviour
(src/f5_tts/infer/utils_infer.py) -- SURVEY.md section 8(f) rows 1 and 3:

  chunk_text                         utils_infer.py:83-110      text -> chunks of <= max_chars utf-8 bytes
  convert_peft_state_dict_to_plain   utils_infer.py:198-239     PEFT/LoRA keys -> plain weights (W + B A * alpha / r)
  load_checkpoint                    utils_infer.py:242-286     .pt / .safetensors, EMA prefix, legacy mel buffers
  load_adapter                       (no reference counterpart) a PEFT checkpoint as a RESIDENT adapter of the loaded base
  load_model                         utils_infer.py:292-345     CFM(model_cls(**cfg, text_num_embeds=vocab+1, mel_dim))
  load_vocoder                       utils_infer.py:114-137     local vocos checkpoint only (no network here)
  infer_batch_process / infer_process utils_infer.py:453-778    mono mix, RMS-to-0.1, duration formula, sample(),
                                                                 prompt slicing, fp32 vocoder input, rescale, cross-fade
  synthesize_batch                   eval_infer_batch.py:190-212 a ragged batch: sample(), then ONE vocoder pass over every
                                                                 item's generated frames (Vocos.decode_ragged, or BigVGAN.ragged())
  synthesize_long                    utils_infer.py:711-775      the chunks of one long text as ragged batches (the reference hands them
                                                                 to a ThreadPoolExecutor): one prompt mel, one sample() and one
                                                                 decode_ragged per group of chunks, the cross-fade on the device
                                                                 (f5_wave_crossfade); `batched=True` of infer_process
  normalise_prompt / prompt_batch    eval/utils_eval.py:109-148  many speakers, one sentence each: the prompts' mels in ONE ragged
  synthesize_prompts                 eval_infer_batch.py:183-212 pass (MelSpec.forward_ragged), then synthesize_batch per group
  sinc_resample                      utils_infer.py:530-532      torchaudio's Resample restated (torchaudio is absent): prompts at any
                                                                 rate are brought to 24 kHz, on the host per prompt, or with
                                                                 `prompt_on_device=True` (prompt_batch, synthesize_prompts,
                                                                 synthesize_long) together with the mono mix, the RMS and the gain
                                                                 in ONE pass on the device (MelSpec.prepare_ragged)
  edit_plan / speech_edit            speech_edit.py:137-232      re-speak spans of recordings: the frame arithmetic on the host (edit.py), ONE
  wave_splice                        (no reference counterpart)  ragged mel pass, ONE f5_edit_assemble for the batch's conditioning, per
                                                                 group one sample(edit_mask=...) and one ragged decode; `splice=True`:
                                                                 the original samples outside the edited spans (f5_wave_splice)

  clip_prompts                       utils_infer.py:348-361,385-419 the prompt clip of preprocess_ref_audio_text (cut at pauses to at most
                                                                 12 s, trim the silent edges, append 50 ms of silence) for a ragged batch
                                                                 on the device (f5_silence_analyse, f5_wave_gather; the ranges on the
                                                                 host, silence.py); `clip_silence=True` of the prompt_on_device drivers
  remove_silence                     utils_infer.py:784-793      pauses of 1 s or more cut out of generated waveforms, on the device;
                                                                 `remove_silence=True` of synthesize_prompts and the batched infer_process

  parse_script / script_plan         infer_cli.py:363-383        the multi-voice script ("Multi-Speech"): [voice] tags, each stretch in its
  prepare_voices / synthesize_script infer_cli.py:355-415        voice (script.py); every voice's prompt prepared ONCE and kept on the device
                                                                 (VoiceBank), the chunks of all stretches as ragged batches with one prompt
                                                                 per item, ONE f5_wave_join: cross-fades inside a stretch, none between

  deliver_waves / wave_deliver       eval/utils_eval.py:403-411  generated audio at a client's rate (8 to 192 kHz) as f32 or 16-bit PCM, on the
                                                                 device (f5_wave_deliver): the resampler of the prompt stage, the other way
  stream_chunks / open_stream        socket_server.py:72-177     the serving mode (stream.py): a voice prepared once, the first chunk of a
                                                                 request short, packets at the client's rate while later chunks run
  open_pool / wave_emit              (no reference counterpart)  many clients at once: the chunks of different clients share one sample()
                                                                 and one decode per tick (StreamPool, pool_tick), and ONE f5_wave_emit
                                                                 joins and delivers every client's new audio at its own rate and format

Out of scope here: Whisper ASR (an empty ref_text), forced alignment, pinyin /
Korean G2P tokenisers (text is tokenised per character through `vocab_char_map`, or as utf-8 bytes when the model has no
vocabulary, exactly as CFM.sample does for list[str]).
Only checkpoints are loaded with loaders that execute nothing from the file (safetensors, torch.load(weights_only=True)).
"""
from __future__ import annotations

import math
import re

import numpy as np
import torch

from .cfm import CFM, clamp_durations, is_per_item
from .config import HOP_LENGTH, MEL_DIM, N_FFT, SAMPLE_RATE
from . import silence as _silence
from .edit import edit_mask, edit_plan  # noqa: F401  (part of this module's surface)
from .mel import resample_kernel, resampled_length
from .script import parse_script, script_plan  # noqa: F401  (part of this module's surface)
from .utils import list_str_to_idx, list_str_to_tensor, load_vocab
from .vocos import Vocos
from .stream import (StreamPool, StreamSession, open_pool, open_stream, packet_sizes, pool_tick, request_plan,  # noqa: F401
                     stream_chunks, stream_limits)                               # (part of this module's surface)
from .wave import (cross_fade_plan, deliver_plan, emit_plan, join_plan, ragged_items, silence_flags, wave_crossfade,  # noqa: F401
                   wave_deliver, wave_emit, wave_gather, wave_join, wave_splice)  # (the device calls: wave.py)

target_sample_rate = SAMPLE_RATE
n_mel_channels = MEL_DIM
hop_length = HOP_LENGTH
win_length = N_FFT
n_fft = N_FFT
mel_spec_type = "vocos"
target_rms = 0.1
cross_fade_duration = 0.15
ode_method = "euler"
nfe_step = 32
cfg_strength = 2.0
sway_sampling_coef = -1.0
speed = 1.0
fix_duration = None


def chunk_text(text: str, max_chars: int = 135) -> list[str]:
    chunks, cur = [], ""
    for sent in re.split(r"(?<=[;:,.!?])\s+|(?<=[；：，。！？])", text):
        piece = sent + " " if sent and len(sent[-1].encode("utf-8")) == 1 else sent
        if len(cur.encode("utf-8")) + len(sent.encode("utf-8")) <= max_chars:
            cur += piece
        else:
            if cur:
                chunks.append(cur.strip())
            cur = piece
    if cur:
        chunks.append(cur.strip())
    return chunks


def convert_peft_state_dict_to_plain(state_dict: dict, lora_alpha: float = 32.0, lora_r: int = 16) -> dict:
    """PEFT checkpoints (`base_model.model.*`, `.base_layer.`, `.lora_A/B.default.`) -> plain names with the low-rank
    update merged: W <- W + (B @ A) * alpha / r."""
    prefix = "base_model.model."
    if not any(k.startswith(prefix) for k in state_dict):
        return state_dict
    scale = lora_alpha / lora_r
    plain = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    out = {}
    for k, v in plain.items():
        if ".lora_A." in k or ".lora_B." in k:
            continue
        if k.endswith(".base_layer.weight"):
            stem = k[: -len(".base_layer.weight")]
            a, b = plain.get(stem + ".lora_A.default.weight"), plain.get(stem + ".lora_B.default.weight")
            if a is not None and b is not None:
                out[stem + ".weight"] = (v + (b @ a).to(v.dtype) * scale).to(v.dtype)
            else:
                out[k] = v
        elif k.endswith(".base_layer.bias"):
            out.setdefault(k[: -len(".base_layer.bias")] + ".bias", v)
        else:
            out[k] = v
    return out


def _read_checkpoint_state_dict(ckpt_path: str, use_ema: bool) -> dict:
    """The state dict of a reference checkpoint (utils_infer.py:254-282): .safetensors or .pt, EMA or model weights."""
    if ckpt_path.split(".")[-1] == "safetensors":
        from safetensors.torch import load_file

        ckpt = load_file(ckpt_path, device="cpu")
        ckpt = {"ema_model_state_dict": ckpt} if use_ema else {"model_state_dict": ckpt}
    else:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    if use_ema:
        sd = {k.replace("ema_model.", ""): v for k, v in ckpt["ema_model_state_dict"].items() if k not in ("initted", "step")}
        for legacy in ("mel_spec.mel_stft.mel_scale.fb", "mel_spec.mel_stft.spectrogram.window"):
            sd.pop(legacy, None)
        return sd
    return ckpt["model_state_dict"]


def load_adapter(model, ckpt_path: str, name: str, use_ema: bool = True, *, lora_alpha=32, lora_r=16, alpha_pattern=None,
                 rank_pattern=None):
    """Reads a PEFT / LoRA checkpoint (train/train_lora.py) as adapter `name` of the model's backbone instead of
    merging it into a second model: the low-rank pairs are kept, the non-LoRA tensors that differ from the loaded base
    (the text encoder the recipe trains in full) become replacement tensors, equal ones are dropped; a `base_layer` that
    differs from the base, or a differing tensor that is not replaceable, raises.  Activate with
    `model.transformer.set_adapter(name)`; `set_adapter(None)` returns to the base."""
    from .adapters import split_peft_state_dict

    tr = getattr(model, "transformer", model)
    if getattr(tr, "precision", None) == "f8":   # (before the checkpoint is read: add_adapter would refuse it afterwards)
        raise NotImplementedError("resident adapters are not built for precision 'f8': load the model in 'f16p' to use adapters")
    _, tensors = split_peft_state_dict(_read_checkpoint_state_dict(ckpt_path, use_ema), base=tr.state_dict())
    tr.add_adapter(name, tensors, lora_alpha=lora_alpha, lora_r=lora_r, alpha_pattern=alpha_pattern, rank_pattern=rank_pattern)
    return model


def load_checkpoint(model, ckpt_path: str, device: str, dtype=None, use_ema: bool = True):
    """Loads a reference checkpoint into a CFM whose backbone is a HIP backbone.  `dtype` is accepted for signature
    compatibility; the engine's operand precision is the backbone's `precision` (weights are kept in fp32 on the host
    and converted when they are uploaded)."""
    model.load_state_dict(convert_peft_state_dict_to_plain(_read_checkpoint_state_dict(ckpt_path, use_ema)))
    return model.to(device)


def load_model(model_cls, model_cfg: dict, ckpt_path: str | None, mel_spec_type=mel_spec_type, vocab_file: str = "",
               ode_method=ode_method, use_ema=True, device="cuda", precision="parity", length_bucket=0, isolated_rows=False,
               **_ignored):
    """CFM(transformer=model_cls(**model_cfg, text_num_embeds=vocab_size + 1, mel_dim=100), ...) + load_checkpoint.
    `ckpt_path=None` keeps whatever weights the caller loads afterwards (e.g. init_synthetic()).
    length_bucket (not a reference argument; DiT only): granule, in frames, of the length-bucketed sample() graphs -- one
    captured graph per bucket serves the varying durations of infer_process's chunks (0: off).
    isolated_rows (not a reference argument; DiT only): sample_items() / sample_span() -- and with them synthesize_batch, synthesize_prompts,
    synthesize_script and the stream pool where they run per-item -- compute every row as if it were alone in its batch
    (DiT.set_isolated_rows)."""
    vocab_char_map, vocab_size = load_vocab(vocab_file) if vocab_file else (None, 256)
    tr = model_cls(**model_cfg, text_num_embeds=vocab_size + 1, mel_dim=n_mel_channels, precision=precision)
    if length_bucket:
        tr.set_length_buckets(length_bucket)
    if isolated_rows:
        tr.set_isolated_rows(True)
    model = CFM(transformer=tr,
                mel_spec_kwargs=dict(n_fft=n_fft, hop_length=hop_length, win_length=win_length,
                                     n_mel_channels=n_mel_channels, target_sample_rate=target_sample_rate,
                                     mel_spec_type=mel_spec_type),
                odeint_kwargs=dict(method=ode_method), vocab_char_map=vocab_char_map)
    if ckpt_path:
        model = load_checkpoint(model, ckpt_path, device, use_ema=use_ema)
    return model.to(device)


def load_vocoder(vocoder_name="vocos", is_local=True, local_path="", device="cuda", hf_cache_dir=None, precision="f32"):
    """utils_infer.py:114-153.  vocos: `pytorch_model.bin` of charactr/vocos-mel-24khz; bigvgan: `bigvgan_generator.pt` of
    nvidia/bigvgan_v2_24khz_100band_256x ({"generator": state_dict}, weight-norm pairs folded on load).
    precision (bigvgan only; not a reference argument): "f32" or "f16x3" (split-f16 products, f32-level results, ~2x faster)."""
    if not is_local:
        raise RuntimeError("no network in this environment: pass is_local=True and a directory with the vocoder weights")
    if vocoder_name == "bigvgan":
        from .bigvgan import BigVGAN
        voc = BigVGAN(precision=precision)
        ck = torch.load(f"{local_path}/bigvgan_generator.pt", map_location="cpu", weights_only=True)
        voc.load_state_dict(ck.get("generator", ck))
        return voc.eval().to(device)
    if vocoder_name != "vocos":
        raise ValueError(f"unknown vocoder {vocoder_name!r}")
    voc = Vocos()
    sd = torch.load(f"{local_path}/pytorch_model.bin", map_location="cpu", weights_only=True)
    voc.load_state_dict(sd)
    return voc.eval().to(device)


def sinc_resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
                  rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (resampling_method="sinc_interp_hann",
    lowpass_filter_width=6, rolloff=0.99), which the reference applies to prompts that are not at 24 kHz
    (utils_infer.py:530-532, on the host, before the audio goes to the device).  torchaudio is not installed: this restates
    its published polyphase windowed-sinc algorithm (functional._get_sinc_resample_kernel / _apply_sinc_resample_kernel)
    -- PARITY UNPINNED for this step.  waveform f32[c, n] on the host -> f32[c, ceil(n * new / orig)]."""
    import math
    if orig_freq == new_freq:
        return waveform
    kernels, orig, new, width = resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
    kernels = kernels.to(waveform.dtype)                                       # [new, 1, 2 width + orig]
    n = waveform.shape[-1]
    x = torch.nn.functional.pad(waveform.reshape(-1, n), (width, width + orig))
    y = torch.nn.functional.conv1d(x[:, None], kernels, stride=orig)           # [c, new, frames]
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[..., : math.ceil(new * n / orig)]
    return y.reshape(*waveform.shape[:-1], -1)


def normalise_prompt(audio: torch.Tensor, sr: int, target_rms_: float = target_rms):
    """A prompt as both drivers prepare it (utils_infer.py:523-533, eval/utils_eval.py:111-118): mono mix, RMS, the gain up to
    target_rms when it is below, then resampling to 24 kHz, on the host.  Returns (audio f32[1, nw], rms of the mono input)."""
    if audio.shape[0] > 1:
        audio = torch.mean(audio, dim=0, keepdim=True)
    rms = torch.sqrt(torch.mean(torch.square(audio)))
    if rms < target_rms_:
        audio = audio * target_rms_ / rms
    if sr != target_sample_rate:
        audio = sinc_resample(audio, sr, target_sample_rate)                   # utils_infer.py:530-532
    return audio, float(rms)


def prompt_numerics(audio: torch.Tensor, sr: int, ref_text: str, gen_text: str, speed_: float = speed,
                    fix_duration_=None, target_rms_: float = target_rms):
    """The host arithmetic of process_batch (utils_infer.py:523-533,541-544,678-685) factored out so that it can be
    pinned by hand-computed cases: returns (audio mono RMS-normalised [1, nw], rms, ref_audio_len, duration)."""
    audio, rms = normalise_prompt(audio, sr, target_rms_)
    ref_text, ref_audio_len, duration = text_numerics(audio.shape[-1], ref_text, gen_text, speed_, fix_duration_)
    return audio, rms, ref_text, ref_audio_len, duration


def text_numerics(nw: int, ref_text: str, gen_text: str, speed_: float = speed, fix_duration_=None):
    """prompt_numerics behind the audio: from the prompt's sample count at 24 kHz (mel.resampled_length gives it without
    touching the audio) to (ref_text with the trailing-space rule, ref_audio_len, duration)."""
    if len(ref_text[-1].encode("utf-8")) == 1:
        ref_text = ref_text + " "
    local_speed = 0.3 if len(gen_text.encode("utf-8")) < 10 else speed_
    ref_audio_len = nw // hop_length
    if fix_duration_ is not None:
        duration = int(fix_duration_ * target_sample_rate / hop_length)
    else:
        ref_text_len = len(ref_text.encode("utf-8"))
        gen_text_len = len(gen_text.encode("utf-8"))
        duration = ref_audio_len + int(ref_audio_len / ref_text_len * gen_text_len / local_speed)
    return ref_text, ref_audio_len, duration


def rescale_to_prompt(wave: torch.Tensor, rms, target_rms_: float = target_rms) -> torch.Tensor:
    """The output rescale of both drivers, `wave * rms / target_rms` where the prompt's rms was below target_rms
    (utils_infer.py:706-707).  rms as a python float (the host route): the branch as the reference writes it; as a 0-dim device
    tensor (prompt_on_device): the same two operations selected by torch.where, bit-equal for the same rms, and nothing is read
    back from the device."""
    if isinstance(rms, torch.Tensor):
        return torch.where(rms < target_rms_, wave * rms / target_rms_, wave)
    if rms < target_rms_:
        wave = wave * rms / target_rms_
    return wave


def cross_fade_concat(waves: list[np.ndarray], cross_fade_duration_: float = cross_fade_duration) -> np.ndarray:
    """utils_infer.py:734-775."""
    if cross_fade_duration_ <= 0:
        return np.concatenate(waves)
    final = waves[0]
    for nxt in waves[1:]:
        n = min(int(cross_fade_duration_ * target_sample_rate), len(final), len(nxt))
        if n <= 0:
            final = np.concatenate([final, nxt])
            continue
        mix = final[-n:] * np.linspace(1, 0, n) + nxt[:n] * np.linspace(0, 1, n)
        final = np.concatenate([final[:-n], mix, nxt[n:]])
    return final


MAX_CHUNKS = 64   # pieces of one f5_wave_crossfade call (its per-piece table travels as a kernel argument)


def group_chunks(durations: list[int], batch_frames: int | None, max_chunks: int = MAX_CHUNKS) -> list[range]:
    """Consecutive runs of chunks, in text order, that each run as one ragged batch: a batch costs its row count times its
    longest row, so a run holds len(run) * max(durations in run) <= batch_frames and len(run) <= max_chunks.  A single chunk
    over the budget is a run of its own; batch_frames=None: only max_chunks limits a run."""
    runs, start, longest = [], 0, 0
    for i, d in enumerate(durations):
        count = i - start + 1
        if count > 1 and (count > max_chunks or (batch_frames is not None and count * max(longest, d) > batch_frames)):
            runs.append(range(start, i))
            start, longest = i, 0
        longest = max(longest, d)
    if durations:
        runs.append(range(start, len(durations)))
    return runs


def _check_rates(who, rates, count):
    rates = [int(r) for r in rates]
    if len(rates) != count:
        raise ValueError(f"{who}: {count} audios for {len(rates)} rates (need one rate per audio)")
    for r in rates:
        if not _silence.MIN_RATE <= r <= _silence.MAX_RATE:
            raise ValueError(f"{who}: a rate of {r} Hz; silence clipping takes {_silence.MIN_RATE} to {_silence.MAX_RATE} Hz (below "
                             "11025 Hz pydub would resample the prompt up: clip such a prompt yourself)")
    return rates


def clip_prompts(audios, rates, device=None):
    """What preprocess_ref_audio_text does to a prompt's audio before anything else sees it (utils_infer.py:385-419), for a batch:
    cut at pauses to at most 12 s (split_on_silence at 1000 ms / -50 dB, then at 100 ms / -40 dB, then a hard cut), trim the
    silent edges (remove_silence_edges at -42 dB) and append 50 ms of silence.  audios: a list of f32 [C_i, F_i] (or [F_i])
    tensors, on the host or on a GPU; rates: their sample rates, 11025 to 384000 Hz.  Returns (clipped, frames): clipped[i] is a
    [C_i, frames[i]] view into one packed device buffer, which MelSpec.prepare_ragged reads in place; every sample is the
    16-bit value pydub would hold, q / 32768 (q = round-to-even of x * 32768, clamped).
    Per batch: ONE f5_silence_analyse and one small read of its flags, the ranges on the host (silence.py), ONE analyse of the
    clipped signals through their segment tables (they are not materialised) and one small read, ONE f5_wave_gather.  Prompts
    whose rate is no multiple of 100 Hz and that lose leading silence need their trailing milliseconds on a shifted grid: one
    more analyse over just those.  Each item's result is bit for bit what it gives alone.
    A prompt without any sound comes out as the 50 ms of silence alone, at its own rate and channel count (the reference's is
    551 frames of 11025 Hz mono)."""
    S = _silence
    audios = [a[None] if a.dim() == 1 else a for a in audios]
    if not audios:
        raise ValueError("clip_prompts: no audio")
    if any(a.dim() != 2 or a.shape[0] < 1 or a.shape[1] < 1 for a in audios):
        raise ValueError("clip_prompts: every audio must be [channels, frames] (or [frames]) with at least one frame")
    shapes = [(int(a.shape[0]), int(a.shape[1])) for a in audios]
    items = ragged_items(audios, device, "clip_prompts only runs on a GPU (there is no CPU path)",
                         "clip_prompts: the audios are on different devices")[0]
    rates = _check_rates("clip_prompts", rates, len(items))
    B = len(items)
    lens = [S.ms_len(f, r) for (_, f), r in zip(shapes, rates)]
    first = silence_flags(items, shapes, rates, lens, S.CLIP_QUERIES, S.PROMPT_QSCALE)
    signals = [S.prompt_clip_plan(first[b][0], first[b][1], shapes[b][1], rates[b])[0] for b in range(B)]
    sig_ms = [S.ms_len(S.signal_frames(p), r) for p, r in zip(signals, rates)]
    edges = silence_flags(items, shapes, rates, sig_ms, S.EDGE_QUERIES, S.PROMPT_QSCALE, [S.segment_table(p) for p in signals])
    rests, ms_flags, shifted = [], [None] * B, []
    for b in range(B):
        lead = S.leading_trim(edges[b][0], sig_ms[b])
        rest, same_grid = S.after_lead(signals[b], rates[b], lead)
        rests.append(rest)
        if same_grid:
            ms_flags[b] = edges[b][1][lead:]
        else:
            shifted.append(b)
    if shifted:
        again = silence_flags([items[b] for b in shifted], [shapes[b] for b in shifted], [rates[b] for b in shifted],
                              [S.ms_len(S.signal_frames(rests[b]), rates[b]) for b in shifted], S.EDGE_QUERIES[1:], S.PROMPT_QSCALE,
                              [S.segment_table(rests[b]) for b in shifted])
        for b, fl in zip(shifted, again):
            ms_flags[b] = fl[0]
    tables, frames = [], []
    for b in range(B):
        keep = S.trailing_cut(ms_flags[b], S.signal_frames(rests[b]), rates[b])
        pieces, n = S.finish_prompt(rests[b], keep, rates[b])
        tables.append(S.segment_table(pieces))
        frames.append(n)
    return wave_gather(items, shapes, tables, frames, S.PROMPT_QSCALE), frames


def remove_silence(wavs, lens=None):
    """remove_silence_for_generated_wav (utils_infer.py:784-793; the CLI's and the Gradio app's `remove_silence`) for a batch of
    generated waveforms at 24 kHz, on the device: pauses of 1 s or more at -50 dB are cut out, 500 ms kept around each stretch of
    sound.  wavs: an f32 [B, stride] device tensor with item b in wavs[b, :lens[b]] (decode_ragged's return), or a list of 1-D f32
    device tensors (lens: None).  Returns (a list of 1-D views into one packed device buffer, their lengths); every sample is
    q / 32768 of its source sample, q = round-to-even of x * 32767, clamped (libsndfile's float -> PCM_16 rule; soundfile is not
    installed, so that rule is unpinned).  A waveform without any sound comes out empty.  ONE f5_silence_analyse, one small read
    of its flags, ONE f5_wave_gather."""
    S = _silence
    if isinstance(wavs, torch.Tensor):
        if wavs.dim() != 2 or lens is None or len(lens) != wavs.shape[0]:
            raise ValueError("remove_silence: wavs must be [B, stride] with one length per row, or a list of 1-D tensors")
        wavs = [wavs[b, :int(n)] for b, n in enumerate(lens)]
    wavs = list(wavs)
    if any(w.dim() != 1 for w in wavs):
        raise ValueError("remove_silence: every waveform must be 1-D")
    if any(w.device.type != "cuda" for w in wavs):
        raise RuntimeError("remove_silence only runs on a GPU (there is no CPU path)")
    out, out_lens = [w[:0] for w in wavs], [0] * len(wavs)
    live = [i for i, w in enumerate(wavs) if w.shape[0] > 0]
    if not live:
        return out, out_lens
    items = ragged_items([wavs[i] for i in live], None, "remove_silence only runs on a GPU (there is no CPU path)",
                         "remove_silence: the waveforms are on different devices")[0]
    shapes = [(1, int(w.shape[0])) for w in items]
    rates = [target_sample_rate] * len(items)
    flags = silence_flags(items, shapes, rates, [S.ms_len(f, target_sample_rate) for _, f in shapes], S.REMOVE_QUERIES, S.WAVE_QSCALE)
    plans = [S.remove_silence_plan(flags[k][0], shapes[k][1], target_sample_rate) for k in range(len(items))]
    frames = [S.signal_frames(p) for p in plans]
    views = wave_gather(items, shapes, [S.segment_table(p) for p in plans], frames, S.WAVE_QSCALE)
    for i, v, n in zip(live, views, frames):
        out[i], out_lens[i] = v.reshape(-1), n
    return out, out_lens


_remove_pauses = remove_silence   # (the drivers below have a keyword of that name)


def _require_text_tokenizer(model_obj, text_tokenizer):
    tok_type = getattr(model_obj, "_tokenizer_type", "custom")
    if text_tokenizer is None and isinstance(tok_type, str) and tok_type.startswith("kor_"):
        raise NotImplementedError(f"model tokenizer type {tok_type!r}: pass text_tokenizer= (str -> list[str], the reference's "
                                  "utils_infer.py:549-660 conversion) -- the Korean G2P / allophone front-end is not part of this engine")


def _warn_untokenised(model_obj, toks, stacklevel):
    vocab = getattr(model_obj, "vocab_char_map", None)
    if vocab is not None:
        missing = sum(1 for c in toks if c not in vocab)
        if len(toks) >= 8 and missing > 0.3 * len(toks):
            import warnings
            warnings.warn(f"{missing} of {len(toks)} text tokens are not in the model's vocabulary (they all map to id 0): "
                          "this checkpoint expects a tokenised input (text_tokenizer=)", RuntimeWarning, stacklevel=stacklevel)


def _tokenise(model_obj, texts, text_tokenizer, stacklevel):
    """The text front-end of the batch drivers: `text_tokenizer` per string where one is given, the untokenised-text warning
    (stacklevel as the caller would pass it to warnings.warn: 3 = the frame that called the caller; None: no warning), then
    ids through the model's vocabulary, or utf-8 bytes when it has none, exactly as CFM.sample does for list[str].
    Returns (texts as sample() takes them, ids)."""
    if text_tokenizer is not None:
        texts = [text_tokenizer(t) for t in texts]
    if stacklevel is not None:
        for t in texts:
            _warn_untokenised(model_obj, t, stacklevel=stacklevel + 1)
    vocab = getattr(model_obj, "vocab_char_map", None)
    return texts, (list_str_to_idx(texts, vocab) if vocab is not None else list_str_to_tensor(texts))


def _require_ragged_vocoder(vocoder, who, hint):
    if not hasattr(vocoder, "decode_ragged"):
        raise NotImplementedError(f"{who} decodes through vocoder.decode_ragged; {type(vocoder).__name__} has no ragged "
                                  f"decode (BigVGAN: {hint}, or pass `vocoder.ragged()`)")


def _progress(progress, iterable):
    """`progress`: None or an object with `.tqdm(iterable)` (the reference passes the tqdm module)."""
    return progress.tqdm(iterable) if progress is not None and hasattr(progress, "tqdm") else iterable


def synthesize_long(ref_audio, ref_text, gen_text_batches, model_obj, vocoder, *, mel_spec_type=mel_spec_type, progress=None,
                    target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, cfg_strength=cfg_strength,
                    sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration, device=None, seed=None,
                    text_tokenizer=None, batch_frames=None, prompt_on_device=False, clip_silence=False):
    """The chunks of one long text as ragged batches instead of one B = 1 pass each (the reference submits them to a
    ThreadPoolExecutor, utils_infer.py:725-732): the host arithmetic of infer_batch_process per chunk (prompt_numerics:
    local_speed, the duration formula, the trailing-space rule), then
      ONE prompt mel (`model_obj.mel_spec`), shared by every chunk;
      per group of chunks (group_chunks over the durations sample() runs at, `batch_frames` = the budget of rows x longest row;
      None: one group) ONE `model_obj.sample` with the prompt mel expanded to the group, per-item durations and the prompt's
      frame count as every item's `lens`, and ONE `vocoder.decode_ragged` of each item's frames behind the prompt;
      the RMS rescale `wave * rms / target_rms` on the packed rows, as the sequential path writes it;
      ONE f5_wave_crossfade over the rows of every group.
    Nothing is copied to the host: returns (wave f32[total], sample_rate, combined mel f32[100, T_total]), both on the device.
    At most 64 chunks (ValueError); a vocoder without decode_ragged: NotImplementedError (plain BigVGAN: pass `.ragged()`).
    prompt_on_device=True: the prompt's mono mix, RMS, gain and resampling run on the device (a B = 1
    `model_obj.mel_spec.prepare_ragged`) instead of normalise_prompt on the host; the frame arithmetic comes from
    mel.resampled_length and the rescale takes the device rms (rescale_to_prompt), so nothing is read back.
    clip_silence=True (needs prompt_on_device=True: ValueError otherwise): the prompt goes through clip_prompts first, as the
    reference's preprocess_ref_audio_text does; every length below is then the clipped prompt's.

    Against the sequential path (infer_batch_process, batched=False):
      * the waveform is f32; the sequential one is float64 wherever a cross-fade happened (numpy promotes).  The values are
        the float64 ones rounded once to f32;
      * a chunk's mel in a batch equals the same chunk run alone only where batch items cannot see each other's padding:
        with `attn_mask_enabled=True` the backbone runs the valid rows only (RowPack).  With `attn_mask_enabled=False` (the
        shipped configs) a shorter chunk attends over the padded frames up to the group's longest, exactly as in the
        reference's own batch driver (eval/eval_infer_batch.py, cfm.py:155-158)."""
    _require_text_tokenizer(model_obj, text_tokenizer)
    _require_ragged_vocoder(vocoder, "synthesize_long", "use the sequential path, batched=False")
    gen_text_batches = list(gen_text_batches)
    if not gen_text_batches:
        raise ValueError("synthesize_long: no text to synthesise")
    if len(gen_text_batches) > MAX_CHUNKS:
        raise ValueError(f"synthesize_long: {len(gen_text_batches)} chunks; one call cross-fades at most {MAX_CHUNKS} "
                         "(split the text, or use the sequential path)")
    audio, sr = ref_audio
    device = device if device is not None else model_obj.device
    if clip_silence:
        if not prompt_on_device:
            raise ValueError("synthesize_long: clip_silence=True needs prompt_on_device=True (the clip runs on the device)")
        audio = clip_prompts([audio], [sr], device=device)[0][0]
    texts, durations = [], []
    for gen_text in gen_text_batches:
        if prompt_on_device:
            rtext, ref_len, duration = text_numerics(resampled_length(audio.shape[-1], sr, target_sample_rate), ref_text, gen_text,
                                                     speed, fix_duration)
        else:
            a, rms, rtext, ref_len, duration = prompt_numerics(audio, sr, ref_text, gen_text, speed, fix_duration, target_rms)
        texts.append(rtext + gen_text)
        durations.append(duration)
    texts, idx = _tokenise(model_obj, texts, text_tokenizer, stacklevel=3)
    with torch.inference_mode():
        if prompt_on_device:
            wavs, rms_dev = model_obj.mel_spec.prepare_ragged([audio], [sr], target_rms, device=device)
            a, rms = wavs[0][None], rms_dev[0]
        cond = model_obj.mel_spec(a.to(device)).permute(0, 2, 1)                # [1, T, 100], T = ref_len + 1 (centre padding; bigvgan type: ref_len)
        cond_len = cond.shape[1]
        ends = clamp_durations(idx, torch.full((len(texts),), cond_len, dtype=torch.long), torch.tensor(durations)).tolist()
        groups = group_chunks(ends, batch_frames)
        rows, lens, specs = [], [], []
        for run in _progress(progress, groups):
            B = len(run)
            generated, _ = model_obj.sample(cond=cond.expand(B, -1, -1), text=[texts[k] for k in run],
                                            duration=torch.tensor([durations[k] for k in run]),
                                            lens=torch.full((B,), cond_len, dtype=torch.long), steps=nfe_step,
                                            cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
            generated = generated.to(torch.float32)
            wave, wave_lens = vocoder.decode_ragged(generated.permute(0, 2, 1), ends=[ends[k] for k in run], starts=[ref_len] * B)
            wave = rescale_to_prompt(wave, rms, target_rms)
            rows.append(wave)
            lens += wave_lens
            specs += [generated[b, ref_len:ends[k]].permute(1, 0) for b, k in enumerate(run)]
        if len(rows) == 1:
            packed = rows[0]
        else:
            packed = torch.empty(len(lens), max(lens), device=rows[0].device, dtype=torch.float32)
            r0 = 0
            for wave in rows:
                packed[r0:r0 + wave.shape[0], :wave.shape[1]] = wave
                r0 += wave.shape[0]
        cf = int(cross_fade_duration * target_sample_rate) if cross_fade_duration > 0 else 0
        return wave_crossfade(packed, lens, cf), target_sample_rate, torch.cat(specs, dim=1)


def infer_batch_process(ref_audio, ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type=mel_spec_type,
                        progress=None, target_rms=target_rms, cross_fade_duration=cross_fade_duration,
                        nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                        speed=speed, fix_duration=fix_duration, device=None, streaming=False, chunk_size=2048, seed=None,
                        text_tokenizer=None, batched=False, batch_frames=None, prompt_on_device=False, clip_silence=False,
                        remove_silence=False):
    """A GENERATOR, as in the reference (utils_infer.py:504-522,711-778):
      streaming=False  yields ONE item (final_wave f32 numpy, sample_rate, combined mel [100, T_total]) -- the cross-faded
                       concatenation over the text batches; (None, sample_rate, None) when there is no batch
                       (`infer_process` returns `next(...)` of it);
      streaming=True   yields (wave[j : j + chunk_size], sample_rate) per chunk of every batch's waveform in turn, no cross-fade
                       (the socket server's mode, socket_server.py:138-177).
    `progress`: None or an object with `.tqdm(iterable)` (the reference passes the tqdm module).
    batched=True (not a reference argument; plain BigVGAN: pass `.ragged()`; not with streaming: ValueError) runs the text batches through
    `synthesize_long` -- ragged batches of at most `batch_frames` (rows x longest row; None: one batch), the cross-fade on the
    device -- and yields ONE item (wave.cpu().numpy(), sample_rate, spec.cpu().numpy()).  Two differences from batched=False,
    which is unchanged: the waveform is f32 (the sequential one is float64 wherever a cross-fade happened), and a chunk's mel
    equals the same chunk run alone only with `attn_mask_enabled=True`; with `attn_mask_enabled=False` (the shipped configs) a
    shorter chunk attends over the batch's padded frames, as in the reference's batch driver (see synthesize_long).
    prompt_on_device=True (with batched=True only: ValueError otherwise; the sequential path prepares its prompt on the host)
    is handed to synthesize_long: the prompt is mixed, levelled and resampled on the device.
    clip_silence=True (with prompt_on_device=True only: ValueError otherwise): the prompt is clipped first (clip_prompts).
    remove_silence=True (with batched=True only: ValueError otherwise): pauses of 1 s or more are cut out of the finished
    waveform on the device, behind the cross-fade, as the reference's CLI does to the file it wrote (remove_silence).

    Text front-end: the reference turns `ref_text + gen_text` into tokens per `model_obj._tokenizer_type` -- for the kor_*
    types through Korean G2P / jamo decomposition / allophone rules (utils_infer.py:549-660: g2pk and the repo's own rule
    tables, CPU string work outside this engine's scope).  Here the string is handed to `model_obj.sample`, which maps it
    per character through `vocab_char_map` (the reference's "custom"/char path); a kor_* model therefore needs
    `text_tokenizer`: a callable str -> list[str] producing exactly the reference's tokens.  Without one this raises rather
    than synthesise from ids that are almost all 0 (raw Hangul is not in a jamo / allophone vocabulary)."""
    if batched and streaming:
        raise ValueError("infer_batch_process: batched=True yields one finished waveform; it cannot be combined with streaming=True")
    if prompt_on_device and not batched:
        raise ValueError("infer_batch_process: prompt_on_device=True needs batched=True (the sequential path prepares its prompt on the host)")
    if clip_silence and not prompt_on_device:
        raise ValueError("infer_batch_process: clip_silence=True needs prompt_on_device=True (the clip runs on the device)")
    if remove_silence and not batched:
        raise ValueError("infer_batch_process: remove_silence=True needs batched=True (it runs on the device, behind the cross-fade)")
    audio, sr = ref_audio
    device = device if device is not None else model_obj.device
    _require_text_tokenizer(model_obj, text_tokenizer)
    if batched:
        gen_text_batches = list(gen_text_batches)
        if not gen_text_batches:
            yield None, target_sample_rate, None
            return
        wave, rate, spec = synthesize_long(
            (audio, sr), ref_text, gen_text_batches, model_obj, vocoder, mel_spec_type=mel_spec_type, progress=progress,
            target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, cfg_strength=cfg_strength,
            sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration, device=device, seed=seed,
            text_tokenizer=text_tokenizer, batch_frames=batch_frames, prompt_on_device=prompt_on_device, clip_silence=clip_silence)
        if remove_silence:
            wave = _remove_pauses([wave])[0][0]
        yield wave.cpu().numpy(), rate, spec.cpu().numpy()
        return

    def process_batch(gen_text):
        """One text batch -> (wave f32 numpy [nw], generated mel numpy [100, T])   (utils_infer.py:541-709)."""
        a, rms, rtext, ref_len, duration = prompt_numerics(audio, sr, ref_text, gen_text, speed, fix_duration, target_rms)
        a = a.to(device)
        text_list = [text_tokenizer(rtext + gen_text)] if text_tokenizer is not None else [rtext + gen_text]
        _warn_untokenised(model_obj, text_list[0], stacklevel=3)
        with torch.inference_mode():
            generated, _ = model_obj.sample(cond=a, text=text_list, duration=duration, steps=nfe_step,
                                            cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
            generated = generated.to(torch.float32)[:, ref_len:, :].permute(0, 2, 1)
            wave = vocoder.decode(generated) if mel_spec_type == "vocos" else vocoder(generated)   # utils_infer.py:702-705
            if rms < target_rms:
                wave = wave * rms / target_rms
            return wave.squeeze().cpu().numpy(), generated[0].cpu().numpy()

    batches = _progress(progress, gen_text_batches)
    if streaming:
        for gen_text in batches:
            wave, _spec = process_batch(gen_text)
            for j in range(0, len(wave), chunk_size):
                yield wave[j:j + chunk_size], target_sample_rate
        return
    waves, specs = [], []
    for gen_text in batches:
        wave, spec = process_batch(gen_text)
        waves.append(wave)
        specs.append(spec)
    if not waves:
        yield None, target_sample_rate, None
        return
    yield cross_fade_concat(waves, cross_fade_duration), target_sample_rate, np.concatenate(specs, axis=1)


def _sampler_for(model, who, total, run, *, steps, cfg_strength, sway_sampling_coef, seed):
    """The sampler call of one group of a batched driver: (model.sample, its four settings) as ever when all four are given once;
    when any is a sequence -- one entry per item of the whole call, `total` of them -- (model.sample_items, the settings with every
    sequence cut to the group's items `run`)."""
    kw = dict(steps=steps, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=seed)
    if not is_per_item(*kw.values()):
        return model.sample, kw
    for name, v in kw.items():
        if is_per_item(v):
            if len(v) != total:
                raise ValueError(f"{who}: {name} has {len(v)} entries for {total} items")
            kw[name] = [v[k] for k in run]
    return model.sample_items, kw


def synthesize_batch(model, vocoder, cond, text, duration, *, lens, gain=None, **sample_kw):
    """The reference's batch loop (eval/eval_infer_batch.py:190-212) as one call: `model.sample(cond, text, duration, lens=lens,
    **sample_kw)`, then every item's generated frames [lens_i, duration_i) through the vocoder in ONE ragged pass
    (vocoder.decode_ragged: Vocos, or `BigVGAN.ragged()`) instead of one decode per item.  `duration_i` are the clamped totals sample() ran at.
    Returns (wav f32[B, L_max], wav_lens, mel): wav[i, :wav_lens[i]] is item i's waveform (times gain[i] where given), zeros
    behind it; mel is sample()'s output [B, N, 100], prompts included.  Plain BigVGAN: pass `.ragged()`.
    steps / cfg_strength / sway_sampling_coef / seed given as a sequence of B: the batch runs as `model.sample_items`, each item
    with its own."""
    _require_ragged_vocoder(vocoder, "synthesize_batch", "decode item by item")
    if sample_kw.get("vocoder") is not None:
        raise TypeError("synthesize_batch: pass the vocoder as its second argument, not through sample()'s vocoder=")
    if isinstance(text, list):
        text = _tokenise(model, text, None, stacklevel=None)[1]   # (as before: this driver does not warn)
    lens = torch.as_tensor(lens).to("cpu", torch.long)
    ends = clamp_durations(text.to("cpu", torch.long), lens, duration, sample_kw.get("max_duration", 65536))
    four = ("steps", "cfg_strength", "sway_sampling_coef", "seed")
    sample = model.sample_items if is_per_item(*(sample_kw.get(n) for n in four)) else model.sample
    mel, _ = sample(cond, text, duration, lens=lens, **sample_kw)
    wav, wav_lens = vocoder.decode_ragged(mel.to(torch.float32).permute(0, 2, 1), ends=ends.tolist(), starts=lens.tolist(), gain=gain)
    return wav, wav_lens, mel


def deliver_waves(model, wav, lens, *, out_rate, sample_format="f32"):
    """What synthesize_batch and synthesize_prompts return, at a client's rate and sample format: wav f32 [B, L_max] on the device
    with item i in wav[i, :lens[i]] (or a list of 1-D waveforms; lens may then be None) -> a list of 1-D device tensors, f32 or
    int16 ("s16"), each the finished item resampled from 24 kHz to out_rate (wave_deliver: ONE launch for the batch, the rows
    read where they lie, nothing copied to the host)."""
    if isinstance(wav, torch.Tensor):
        if wav.dim() != 2 or lens is None or len(lens) != wav.shape[0]:
            raise ValueError("deliver_waves: wav must be [B, L_max] with one length per row (or a list of 1-D waveforms)")
        wav = [wav[b, :int(n)] for b, n in enumerate(lens)]
    return wave_deliver(model.mel_spec, wav, out_rate=out_rate, sample_format=sample_format, final=True)


def prompt_batch(prompts, gen_texts, *, speed=speed, target_rms=target_rms, mel_spec, device=None, prompt_on_device=False,
                 clip_silence=False):
    """`get_inference_prompt` for one batch (eval/utils_eval.py:109-148, without the truth-duration branch and the bucketing,
    which is batching.bucket_prompts): prompts is a list of (audio [channels, nw], sample_rate, ref_text), gen_texts the text to
    speak with each.  normalise_prompt per item on the host, then ONE `mel_spec.forward_ragged` over every prompt.  Returns
    dict(cond f32[B, T_max, n_mels] zero-padded (padded_mel_batch), lens = frames per prompt (ref_mel_len), durations =
    total_mel_len per item, texts = prompt text + target text (trailing-space rule), rms per prompt).
    prompt_on_device=True: ONE `mel_spec.prepare_ragged` over every prompt (mono mix, RMS, gain and resampling on the device, the
    raw audio down in one copy) instead of the normalise_prompt loop; `rms` is then a device f32[B] tensor and stays there.
    clip_silence=True (needs prompt_on_device=True: ValueError otherwise): every prompt goes through clip_prompts first, as the
    reference's preprocess_ref_audio_text does; lens and durations are then the clipped prompts'."""
    from .batching import prompt_text_and_frames

    prompts, gen_texts = list(prompts), list(gen_texts)
    if not prompts or len(prompts) != len(gen_texts):
        raise ValueError(f"prompt_batch: {len(prompts)} prompts for {len(gen_texts)} texts (need one text per prompt, at least one)")
    where = {} if device is None else dict(device=device)
    if clip_silence and not prompt_on_device:
        raise ValueError("prompt_batch: clip_silence=True needs prompt_on_device=True (the clip runs on the device)")
    if prompt_on_device:
        raw, rates = [p[0] for p in prompts], [p[1] for p in prompts]
        if clip_silence:
            raw = clip_prompts(raw, rates, **where)[0]
        audios, rms = mel_spec.prepare_ragged(raw, rates, target_rms, **where)
    else:
        audios, rms = [], []
        for audio, sr, _ref_text in prompts:
            a, r = normalise_prompt(audio, sr, target_rms)
            audios.append(a)
            rms.append(r)
    mel, frames = mel_spec.forward_ragged(audios) if device is None else mel_spec.forward_ragged(audios, device=device)
    texts, durations = [], []
    for (_audio, _sr, ref_text), gen_text, n in zip(prompts, gen_texts, frames):
        text, total = prompt_text_and_frames(n, ref_text, gen_text, speed)
        texts.append(text)
        durations.append(total)
    return dict(cond=mel.permute(0, 2, 1), lens=list(frames), durations=durations, texts=texts, rms=rms)


def synthesize_prompts(model, vocoder, prompts, gen_texts, *, speed=speed, target_rms=target_rms, nfe_step=nfe_step,
                       cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=None, text_tokenizer=None,
                       batch_frames=None, prompt_on_device=False, clip_silence=False, remove_silence=False, **sample_kw):
    """The reference's batch job from raw prompt audio to waveforms (eval/utils_eval.py:109-148 + eval_infer_batch.py:183-212):
    many speakers, one sentence each.  prompt_batch (ONE ragged mel pass over every prompt), then per group of items
    (group_chunks over the totals sample() runs at; `batch_frames` = the budget of rows x longest row, None: groups of up to 64)
    ONE synthesize_batch -- sample() and one ragged decode -- with the group's `cond` cut to its longest prompt, then the rescale
    `wave * rms_i / target_rms` on exactly the rows with rms_i < target_rms, as the sequential path writes it (not a
    decode_ragged gain: one multiply is not bit-equal to a multiply and a divide).
    prompt_on_device=True: the prompts are prepared on the device (prompt_batch), their rms stays there and the rescale selects
    with torch.where (rescale_to_prompt): no per-item host arithmetic on audio and no device-to-host read before the waveforms
    are returned.
    clip_silence=True (needs prompt_on_device=True): the prompts are clipped first (prompt_batch, clip_prompts).
    remove_silence=True: pauses of 1 s or more are cut out of every finished waveform, in one pass over all of them (remove_silence).
    nfe_step / cfg_strength / sway_sampling_coef / seed: one value, or a sequence of one value per prompt (model.sample_items).
    Returns (waves: a list of 1-D f32 device tensors, sample_rate, mel: a list of [100, T_i] generated mels).  Plain BigVGAN: pass `.ragged()`."""
    _require_text_tokenizer(model, text_tokenizer)
    _require_ragged_vocoder(vocoder, "synthesize_prompts", "decode item by item")
    prompts, gen_texts = list(prompts), list(gen_texts)
    if not prompts:
        raise ValueError("synthesize_prompts: no prompt to synthesise from")
    if len(prompts) != len(gen_texts):
        raise ValueError(f"synthesize_prompts: {len(prompts)} prompts for {len(gen_texts)} texts (need one text per prompt)")
    with torch.inference_mode():
        pb = prompt_batch(prompts, gen_texts, speed=speed, target_rms=target_rms, mel_spec=model.mel_spec, device=model.device,
                          prompt_on_device=prompt_on_device, clip_silence=clip_silence)
        texts, idx = _tokenise(model, pb["texts"], text_tokenizer, stacklevel=3)
        lens, durations, rms = pb["lens"], pb["durations"], pb["rms"]
        ends = clamp_durations(idx.to("cpu", torch.long), torch.tensor(lens), torch.tensor(durations),
                               sample_kw.get("max_duration", 65536)).tolist()
        waves, mels = [], []
        for run in group_chunks(ends, batch_frames):
            glens = [lens[k] for k in run]
            cond = pb["cond"][run.start:run.stop, :max(glens)].contiguous()
            _, four = _sampler_for(model, "synthesize_prompts", len(prompts), run, steps=nfe_step, cfg_strength=cfg_strength,
                                   sway_sampling_coef=sway_sampling_coef, seed=seed)
            wav, wav_lens, mel = synthesize_batch(model, vocoder, cond, [texts[k] for k in run],
                                                  torch.tensor([durations[k] for k in run]), lens=glens, **four, **sample_kw)
            for b, k in enumerate(run):
                waves.append(rescale_to_prompt(wav[b, :wav_lens[b]], rms[k], target_rms))
                mels.append(mel[b, lens[k]:ends[k]].to(torch.float32).permute(1, 0))
        if remove_silence:
            waves = _remove_pauses(waves)[0]
        return waves, target_sample_rate, mels


def speech_edit(model, vocoder, items, *, target_rms=target_rms, nfe_step=nfe_step, cfg_strength=cfg_strength,
                sway_sampling_coef=sway_sampling_coef, seed=None, text_tokenizer=None, batch_frames=None, prompt_on_device=False,
                splice=False, splice_cross_fade=0.01, **sample_kw):
    """The reference's speech editing script (infer/speech_edit.py) for a batch of recordings: items is a list of
    (audio [C, n], sample_rate, target_text, parts_to_edit, fix_duration | None) -- the whole sentence the recording should say
    instead, the spans to replace as (start, end) in seconds, and optionally the new length of each span.  Finding the spans
    (forced alignment) is the caller's business.
      every recording prepared as the script does (normalise_prompt per item on the host; prompt_on_device=True: ONE
      `mel_spec.prepare_ragged`, the rms stays on the device), and down in one copy;
      ONE `mel_spec.forward_ragged` over all of them, edit_plan per item on the host, ONE `mel_spec.edit_assemble`;
      per group of items (group_chunks over the totals sample() runs at, `batch_frames` = the budget of rows x longest row; None:
      groups of up to 64) ONE `model.sample(cond, text, duration=D, lens=D, edit_mask=mask)`, ONE `vocoder.decode_ragged` over
      frames [0, ends_i) of every item and, with splice=True, ONE `wave_splice`: the samples of every kept span are the prepared
      original's, cross-faded over splice_cross_fade seconds at the inner boundaries (0.01 s = 240 samples; a chosen value);
      then the rescale `wave * rms / target_rms` where the recording was levelled up (rescale_to_prompt).
    ends_i are the totals sample() ran at (clamp_durations): at least D_i + 1 -- the rule `max(text, lens) + 1` gives one
    generated frame behind the recording, and it is decoded, as in the script.
    Returns (waves: a list of 1-D f32 device tensors, sample_rate, mels: a list of [100, ends_i]); nothing is copied to the host.
    A vocoder without decode_ragged: NotImplementedError (plain BigVGAN: pass `.ragged()`).

    Text: tokenised as the other drivers do (per character through the model's vocabulary, utf-8 bytes without one, or
    `text_tokenizer`).  The script's `final_text_list = [text_list]` nesting for non-pinyin tokenisers makes the whole sentence
    ONE token; that is not reproduced here.
    As in every batch driver, an item in a batch equals the item run alone only where items cannot see each other's padding:
    with `attn_mask_enabled=True` the backbone runs the valid rows only and every item equals the item run alone; with
    `attn_mask_enabled=False` (the shipped configs) a shorter item attends over the padded frames up to the group's longest,
    as in the reference's own batch driver (eval/eval_infer_batch.py, cfm.py:155-158)."""
    _require_text_tokenizer(model, text_tokenizer)
    _require_ragged_vocoder(vocoder, "speech_edit", "decode item by item")
    items = list(items)
    if not items:
        raise ValueError("speech_edit: no recording to edit")
    for key in ("edit_mask", "lens", "steps", "vocoder"):
        if key in sample_kw:
            raise TypeError(f"speech_edit: {key}= is set by the driver, not through sample()'s keywords")
    device, ms = model.device, model.mel_spec
    with torch.inference_mode():
        if prompt_on_device:
            audios, rms = ms.prepare_ragged([it[0] for it in items], [it[1] for it in items], target_rms, device=device)
        else:
            host, rms = [], []
            for audio, sr, *_ in items:
                a, r = normalise_prompt(audio, sr, target_rms)
                host.append(a.reshape(-1).to(torch.float32))
                rms.append(r)
            audios = list(torch.cat(host).to(device).split([a.shape[0] for a in host]))     # ONE copy; the splice reads them too
        mel, frames = ms.forward_ragged(audios, device=device)
        plans = [edit_plan(n, it[3], it[4], sample_rate=target_sample_rate, hop_length=hop_length) for n, it in zip(frames, items)]
        cond, mask, D = ms.edit_assemble(mel, frames, plans)
        texts, idx = _tokenise(model, [it[2] for it in items], text_tokenizer, stacklevel=3)
        ends = clamp_durations(idx.to("cpu", torch.long), torch.tensor(D), torch.tensor(D), sample_kw.get("max_duration", 65536)).tolist()
        cf = int(splice_cross_fade * target_sample_rate) if splice_cross_fade > 0 else 0
        waves, mels = [], []
        for run in group_chunks(ends, batch_frames):
            gD = [D[k] for k in run]
            generated, _ = model.sample(cond=cond[run.start:run.stop, :max(gD)].contiguous(), text=[texts[k] for k in run],
                                        duration=torch.tensor(gD), lens=torch.tensor(gD), steps=nfe_step, cfg_strength=cfg_strength,
                                        sway_sampling_coef=sway_sampling_coef, seed=seed,
                                        edit_mask=mask[run.start:run.stop, :max(gD)], **sample_kw)
            generated = generated.to(torch.float32)
            wav, wav_lens = vocoder.decode_ragged(generated.permute(0, 2, 1), ends=[ends[k] for k in run])
            if splice:
                wav = wave_splice(wav, wav_lens, [audios[k] for k in run], [plans[k] for k in run], cf)
            for b, k in enumerate(run):
                waves.append(rescale_to_prompt(wav[b, :wav_lens[b]], rms[k], target_rms))
                mels.append(generated[b, :ends[k]].permute(1, 0))
        return waves, target_sample_rate, mels


class VoiceBank:
    """The prepared prompts of a set of voices (prepare_voices): on the device the padded log-mel `mel` f32 [V, T_max, 100] and
    the RMS of every mono prompt `rms` f32 [V]; on the host what the plan needs -- `names`, `frames` (mel frames per voice, from
    the host plan of the ragged mel pass; sample() takes its `lens` from the host), `samples` (prepared samples at 24 kHz),
    `seconds` (the prompt's length as infer_process sees it), `ref_texts`, `speeds` (a voice's own speed, or None) -- and the
    `target_rms` the prompts were levelled to.  Nothing here is ever read back from the device."""

    def __init__(self, names, mel, rms, frames, samples, seconds, ref_texts, speeds, target_rms):
        self.names, self.mel, self.rms, self.frames, self.samples = list(names), mel, rms, list(frames), list(samples)
        self.seconds, self.ref_texts, self.speeds, self.target_rms = list(seconds), list(ref_texts), list(speeds), target_rms

    def prompts(self):
        """The voices as script_plan takes them."""
        return {name: dict(seconds=self.seconds[v], samples=self.samples[v], ref_text=self.ref_texts[v], speed=self.speeds[v])
                for v, name in enumerate(self.names)}


def prepare_voices(model, voices, *, target_rms=target_rms, clip_silence=False, device=None) -> VoiceBank:
    """What infer_cli.py:355-361 and infer_batch_process do to every voice's prompt, once for all voices: voices is
    {name: dict(ref_audio=(tensor [C, n], sample_rate), ref_text=str, speed=optional)}.  ONE clip_prompts over all of them (with
    clip_silence=True: preprocess_ref_audio_text's clip), ONE `mel_spec.prepare_ragged` (mono mix, RMS, gain, resampling) and ONE
    `mel_spec.forward_ragged`; the audio goes down in one copy and is never read back.  The bank serves any number of
    synthesize_script calls (the socket server's pattern: update_reference once, many requests)."""
    if not voices:
        raise ValueError("prepare_voices: no voice")
    names = list(voices)
    for name in names:
        if not voices[name]["ref_text"]:
            raise ValueError(f"prepare_voices: voice {name!r} has an empty ref_text (transcribing the prompt is not part of this engine)")
    device = device if device is not None else model.device
    raw, rates = [voices[n]["ref_audio"][0] for n in names], [int(voices[n]["ref_audio"][1]) for n in names]
    with torch.inference_mode():
        if clip_silence:
            raw, counts = clip_prompts(raw, rates, device=device)
        else:
            counts = [int(a.shape[-1]) for a in raw]
        wavs, rms = model.mel_spec.prepare_ragged(raw, rates, target_rms, device=device)
        mel, frames = model.mel_spec.forward_ragged(wavs, device=device)
    return VoiceBank(names, mel.permute(0, 2, 1), rms, frames, [int(w.shape[0]) for w in wavs],
                     [n / sr for n, sr in zip(counts, rates)], [voices[n]["ref_text"] for n in names],
                     [voices[n].get("speed") for n in names], target_rms)


def synthesize_script(model, vocoder, voices, script, *, speed=speed, target_rms=target_rms, cross_fade_duration=cross_fade_duration,
                      nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, fix_duration=fix_duration,
                      seed=None, text_tokenizer=None, batch_frames=None, clip_silence=False, remove_silence=False, default="main"):
    """The multi-voice script of infer_cli.py:348-425 (infer_gradio.py's "Multi-Speech") as ragged batches: `script` carries
    [name] tags, each tagged stretch is spoken with that voice's prompt at that voice's own speed (parse_script), chunked as
    infer_process chunks it (script_plan), and the stretches are concatenated -- where the reference runs one infer_process per
    stretch, each preparing its prompt again.  Text in front of the first tag and unknown names go to the voice `default`.  voices: a VoiceBank (prepare_voices), or the dict prepare_voices takes: then only
    the voices the script uses are prepared, with this call's target_rms and clip_silence (a bank keeps its own).  Then
      per group of items (group_chunks over the totals sample() runs at, in script order; `batch_frames` = the budget of rows x
      longest row, None: groups of up to 64) ONE `model.sample` -- cond = the bank's mel rows of the group's voices, cut to the
      group's longest prompt (an index-select on the device), lens = each item's own prompt frames -- and ONE
      `vocoder.decode_ragged` of each item's frames behind its own prompt; the rescale `wave * rms / target_rms` with each row's
      own device rms (rescale_to_prompt);
      ONE wave_join (f5_wave_join) over the rows of every group where they lie: the chunks of a stretch cross-faded, each
      stretch's fade lengths from that stretch's own running length, plain concatenation between stretches;
      remove_silence=True: pauses of 1 s or more cut out of the result (remove_silence).
    Returns (wave f32[total], sample_rate, combined mel f32[100, T_total], segments), wave and mel on the device; segments is a
    host list of (voice, text, start_sample, end_sample) per stretch in the joined waveform (before any pause is removed) -- what
    the reference's save_chunk writes to files.  A stretch without text has start == end.  Any number of chunks up to 65535.
    nfe_step / cfg_strength / sway_sampling_coef / seed: one value, or a sequence of one value per chunk in script order
    (script_plan's items; model.sample_items).
    A vocoder without decode_ragged: NotImplementedError (plain BigVGAN: pass `.ragged()`); kor_* tokenisers need text_tokenizer=.

    Against one infer_process per stretch:
      * the waveform is f32; the sequential one is float64 wherever a cross-fade happened (numpy promotes).  The values are
        the float64 ones rounded once to f32;
      * a chunk's mel in a batch equals the same chunk run alone only where batch items cannot see each other's padding:
        with `attn_mask_enabled=True` the backbone runs the valid rows only (RowPack).  With `attn_mask_enabled=False` (the
        shipped configs) a shorter chunk attends over the padded frames up to the group's longest, exactly as in the
        reference's own batch driver (eval/eval_infer_batch.py, cfm.py:155-158)."""
    _require_text_tokenizer(model, text_tokenizer)
    _require_ragged_vocoder(vocoder, "synthesize_script", "run infer_process per stretch")
    names = voices.names if isinstance(voices, VoiceBank) else list(voices)
    if default not in names:
        raise ValueError(f"synthesize_script: the default voice {default!r} is not among the voices {names}")
    stretches = parse_script(script, names, default)
    if isinstance(voices, VoiceBank):
        bank = voices
    else:
        used = {v for v, _ in stretches}
        bank = prepare_voices(model, {n: voices[n] for n in names if n in used}, target_rms=target_rms, clip_silence=clip_silence)
    plan = script_plan(stretches, bank.prompts(), speed=speed, fix_duration=fix_duration, cross_fade_duration=cross_fade_duration)
    items, fades = plan["items"], plan["fades"]
    if not items:
        raise ValueError("synthesize_script: no stretch of the script has any text")
    voice_of, durations = [it[0] for it in items], [it[3] for it in items]
    lens = [bank.frames[v] for v in voice_of]
    starts = [bank.samples[v] // hop_length for v in voice_of]                  # text_numerics' ref_audio_len
    texts, idx = _tokenise(model, [it[2] for it in items], text_tokenizer, stacklevel=3)
    with torch.inference_mode():
        ends = clamp_durations(idx.to("cpu", torch.long), torch.tensor(lens), torch.tensor(durations)).tolist()
        pieces, specs = [], []
        for run in group_chunks(ends, batch_frames):
            glens = [lens[k] for k in run]
            rows = torch.tensor([voice_of[k] for k in run], device=bank.mel.device)
            sample, four = _sampler_for(model, "synthesize_script", len(items), run, steps=nfe_step, cfg_strength=cfg_strength,
                                        sway_sampling_coef=sway_sampling_coef, seed=seed)
            generated, _ = sample(cond=bank.mel[:, :max(glens)].index_select(0, rows), text=[texts[k] for k in run],
                                  duration=torch.tensor([durations[k] for k in run]), lens=torch.tensor(glens), **four)
            generated = generated.to(torch.float32)
            wave, wave_lens = vocoder.decode_ragged(generated.permute(0, 2, 1), ends=[ends[k] for k in run],
                                                    starts=[starts[k] for k in run])
            wave = rescale_to_prompt(wave, bank.rms.index_select(0, rows)[:, None], bank.target_rms)
            for b, k in enumerate(run):
                pieces.append(wave[b, :wave_lens[b]])
                specs.append(generated[b, starts[k]:ends[k]].permute(1, 0))
        offs, _, total = join_plan([int(p.shape[0]) for p in pieces], fades)
        segments, k = [], 0
        for s, (voice, text) in enumerate(stretches):
            first = k
            while k < len(items) and items[k][1] == s:
                k += 1
            at = offs[first] if first < len(items) else total
            segments.append((voice, text, at, offs[k - 1] + int(pieces[k - 1].shape[0]) if k > first else at))
        wave = wave_join(pieces, fades)
        if remove_silence:
            wave = _remove_pauses([wave])[0][0]
        return wave, target_sample_rate, torch.cat(specs, dim=1), segments


def heldout_draws(lens, mel_dim: int, *, seed=0, frac_lengths=(0.7, 1.0)):
    """The draws of heldout_loss: for utterance u of lens[u] frames, from a CPU generator seeded by (seed, u) alone, the masked span
    (start, end) -- CFM.forward's span arithmetic (utils.py:69-75) with its two uniform draws -- and then the noise x0 [lens[u], mel].
    They depend on nothing else: not on the batch an utterance lands in, not on the adapter.  Returns (spans, noises)."""
    spans, noises = [], []
    for u, n in enumerate(lens):
        g = torch.Generator().manual_seed((int(seed) << 32) + u)
        frac = torch.empty(1).uniform_(*frac_lengths, generator=g)
        length = (frac * int(n)).long()
        start = ((int(n) - length) * torch.rand(1, generator=g)).long().clamp(min=0)
        spans.append((int(start), min(int(start + length), int(n))))
        noises.append(torch.randn(int(n), mel_dim, generator=g))
    return spans, noises


def heldout_rows(lens, times: int, batch_frames: int) -> list[list[tuple[int, int]]]:
    """The batches of heldout_loss: every (utterance, time index) pair is a row of its utterance's length, and the rows are
    grouped by batching.bucket_prompts' frame budget (no duration window, no shuffle)."""
    from .batching import bucket_prompts
    rows = [(u, k) for u in range(len(lens)) for k in range(times)]
    row_lens = [int(lens[u]) for u, _ in rows]
    max_secs = max(40, max(row_lens) * HOP_LENGTH // SAMPLE_RATE + 1)
    groups = bucket_prompts(row_lens, infer_batch_size=int(batch_frames), min_secs=0, max_secs=max_secs, shuffle_seed=None)
    return [[rows[i] for i in g] for g in groups]


def heldout_loss(model, mels, texts, *, adapters=(None,), times=8, seed=0, frac_lengths=(0.7, 1.0), batch_frames=38400):
    """The held-out flow-matching loss of CFM.forward (cfm.py:231-302, no drops) for every adapter in `adapters` (names of resident
    adapters, None: the base) on ONE resident engine: a model-selection number that needs nothing but the model.
    mels: a list of U mels [n_u, mel].  texts: a list of U texts -- strings (tokenised as CFM.sample tokenises list[str]) or token-id
    sequences -- or a mapping adapter name -> such a list (fine-tunes tokenise differently).  Every utterance is evaluated at the
    stratified times (k + 0.5) / times with ONE span and ONE noise (heldout_draws: the same for every time, batch and adapter).
    Returns {adapter: {"loss": float, "per_item": [U], "per_time": [times]}}: the mean squared flow error over the masked elements
    of all rows, per utterance, and per time.  The adapter that was active before the call is active again after it, on an
    exception too.  The only readback is one copy at the end."""
    tr = model.transformer
    mel_dim, U = model.num_channels, len(mels)
    adapters = list(adapters)
    per_adapter = texts if isinstance(texts, dict) else {a: texts for a in adapters}
    for a in adapters:
        if a not in per_adapter or len(per_adapter[a]) != U:
            raise ValueError(f"heldout_loss: adapter {a!r} needs one text per utterance ({U})")

    def tokens(t):
        if isinstance(t, str):
            return (list_str_to_idx([t], model.vocab_char_map) if model.vocab_char_map is not None else list_str_to_tensor([t]))[0]
        return torch.as_tensor(t, dtype=torch.long)

    toks = {a: [tokens(t) for t in per_adapter[a]] for a in adapters}
    lens = [int(m.shape[0]) for m in mels]
    spans, noises = heldout_draws(lens, mel_dim, seed=seed, frac_lengths=frac_lengths)
    batches = heldout_rows(lens, times, batch_frames)
    pad = torch.nn.utils.rnn.pad_sequence
    sums = {a: [] for a in adapters}
    before = tr.active_adapter
    try:
        eng = tr.engine()
        for rows in batches:
            us = [u for u, _ in rows]
            x1 = pad([mels[u].to("cpu", torch.float32) for u in us], batch_first=True)
            x0 = pad([noises[u] for u in us], batch_first=True)
            x1, x0 = x1.to(model.device), x0.to(model.device)   # once per batch: every adapter reads the same device tensors
            t = [(k + 0.5) / times for _, k in rows]
            for a in adapters:
                tr.set_adapter(a)
                text = pad([toks[a][u] for u in us], padding_value=-1, batch_first=True)
                sq, cnt, _, _, _ = eng.flow_loss(x1, x0, text, t, [spans[u] for u in us], lens=[lens[u] for u in us],
                                                 want_pred=False, want_cond=False, want_frame_err=False)
                sums[a].append(sq)
    finally:
        tr.set_adapter(before)
    order = [r for rows in batches for r in rows]
    host = torch.stack([torch.cat(sums[a]) for a in adapters]).cpu().double()   # [adapters, rows]: the one readback
    count = torch.tensor([spans[u][1] - spans[u][0] for u in range(U)], dtype=torch.float64) * mel_dim
    out = {}
    for i, a in enumerate(adapters):
        sq = torch.zeros(U, times, dtype=torch.float64)
        for (u, k), v in zip(order, host[i].tolist()):
            sq[u, k] = v
        out[a] = dict(loss=float(sq.sum() / (count.sum() * times)), per_item=(sq.sum(1) / (count * times)).tolist(),
                      per_time=(sq.sum(0) / count.sum()).tolist())
    return out


def heldout_distance_plan(items, *, duration="truth", speed=1.0, batch_frames=38400):
    """The host arithmetic of heldout_distance, the reference's cross-sentence evaluation (eval/utils_eval.py:109-148): for items
    (prompt_mel [p, mel], prompt_text, target_mel [g, mel], target_text) returns (texts, lens, totals, groups).
    texts[u]: prompt text + target text -- for two strings with the reference's rule that a prompt text whose last character is one
    byte gets a trailing space, for two token sequences their concatenation.  lens[u] = p.  totals[u]: the frames sample() is asked
    for -- duration="truth" (use_truth_duration): p + int(g / speed); duration="text": p + int(p / prompt bytes * target bytes /
    speed), which needs strings.  groups: batching.bucket_prompts over the totals under the frame budget `batch_frames`, no
    duration window and no shuffle (as heldout_rows)."""
    from .batching import bucket_prompts, prompt_text_and_frames
    if duration not in ("truth", "text"):
        raise ValueError(f"heldout_distance: duration = {duration!r} (expected 'truth' or 'text')")
    texts, lens, totals = [], [], []
    for u, (prompt_mel, prompt_text, target_mel, target_text) in enumerate(items):
        p, g = int(prompt_mel.shape[0]), int(target_mel.shape[0])
        both_str = isinstance(prompt_text, str) and isinstance(target_text, str)
        if isinstance(prompt_text, str) != isinstance(target_text, str):
            raise ValueError(f"heldout_distance: item {u}: prompt_text and target_text must both be strings or both token sequences")
        if p < 1 or g < 1:
            raise ValueError(f"heldout_distance: item {u}: prompt_mel and target_mel need at least one frame each")
        if both_str:
            text, by_text = prompt_text_and_frames(p, prompt_text, target_text, speed)
        elif duration == "text":
            raise ValueError(f"heldout_distance: duration='text' is a ratio of byte lengths: item {u}'s prompt_text and target_text must be strings")
        else:
            text, by_text = [int(v) for v in prompt_text] + [int(v) for v in target_text], None
        texts.append(text)
        lens.append(p)
        totals.append(p + int(g / speed) if duration == "truth" else by_text)
    max_secs = max(40, max(totals) * HOP_LENGTH // SAMPLE_RATE + 1)
    groups = bucket_prompts(totals, infer_batch_size=int(batch_frames), min_secs=0, max_secs=max_secs, shuffle_seed=None)
    return texts, lens, totals, groups


def heldout_distance(model, items, *, adapters=(None,), duration="truth", nfe_step=nfe_step, cfg_strength=cfg_strength,
                     sway_sampling_coef=sway_sampling_coef, seed=0, speed=1.0, n_cep=13, batch_frames=38400):
    """The distance of what every adapter in `adapters` (names of resident adapters, None: the base) GENERATES from what was recorded,
    on ONE resident engine: the reference's cross-sentence evaluation (eval/utils_eval.py:109-148 -- every held-out sentence spoken
    from a prompt of the same speaker) scored by DTW-aligned mel-cepstral distortion (metrics.mel_distance; include/f5_hip.h) in
    place of the Whisper / WavLM / UTMOS models, which are not built.  Where heldout_loss is teacher-forced, this runs free from
    noise through sample(): this project's solver, guidance, sway, time grid and operand precision are all in the number.
    items: a list of U (prompt_mel [p, mel], prompt_text, target_mel [g, mel], target_text), texts as strings or token-id sequences --
    or a mapping adapter name -> such a list where fine-tunes tokenise differently (the mels are the first adapter's; so are the
    batches).  duration / speed / batch_frames: heldout_distance_plan.  Per batch the target mels go down ONCE and every adapter
    runs `set_adapter`, ONE sample() (`sample_items` when the model's isolated rows are on: only then is an item's score independent
    of its batch neighbours, as everywhere) and ONE f5_mel_distance of the generated frames [p_b, dur_b), read in place from
    sample()'s output, against the targets.  No vocoder is involved.  The adapter that was active before the call is active again
    after it, on an exception too.  The only readback is one copy at the end.
    Returns {adapter: {"mcd": sum_u D_u / sum_u (n_u + m_u), "per_item": [U]}}, in dB per unit of path weight: an MFCC-style distance
    with MCD's constant, comparable between adapters, precisions and sampler settings on the same items, not to published MCD."""
    from .metrics import mel_distance
    tr = model.transformer
    adapters = list(adapters)
    per_adapter = items if isinstance(items, dict) else {a: items for a in adapters}
    U = len(per_adapter[adapters[0]]) if adapters and adapters[0] in per_adapter else 0
    for a in adapters:
        if a not in per_adapter or len(per_adapter[a]) != U or U == 0:
            raise ValueError(f"heldout_distance: adapter {a!r} needs the same items as the others, at least one")
    plans = {a: heldout_distance_plan(per_adapter[a], duration=duration, speed=speed, batch_frames=batch_frames) for a in adapters}
    first = per_adapter[adapters[0]]
    lens, groups = plans[adapters[0]][1], plans[adapters[0]][3]
    targets = [it[2] for it in first]
    toks = {}
    for a in adapters:
        texts = plans[a][0]
        toks[a] = [(list_str_to_idx([t], model.vocab_char_map) if model.vocab_char_map is not None else list_str_to_tensor([t]))[0]
                   if isinstance(t, str) else torch.as_tensor(t, dtype=torch.long) for t in texts]
        if plans[a][1] != lens:
            raise ValueError(f"heldout_distance: adapter {a!r}'s prompt mels differ in length from the first adapter's")
    pad = torch.nn.utils.rnn.pad_sequence
    sample = model.sample_items if getattr(tr, "isolated_rows", False) else model.sample
    scores = {a: [] for a in adapters}
    weights = {a: [] for a in adapters}
    before = tr.active_adapter
    try:
        for run in groups:
            cond = pad([first[u][0].to("cpu", torch.float32) for u in run], batch_first=True).to(model.device)
            glens = torch.tensor([lens[u] for u in run])
            tgt = ragged_items([targets[u].to(torch.float32) for u in run], model.device, "heldout_distance only runs on a GPU (there is "
                               "no CPU path)", "heldout_distance: the target mels are on different devices")[0]   # once per batch
            tgt = [t.view(-1, model.num_channels) for t in tgt]
            for a in adapters:
                tr.set_adapter(a)
                text = pad([toks[a][u] for u in run], padding_value=-1, batch_first=True)
                total = torch.tensor([plans[a][2][u] for u in run])
                end = clamp_durations(text, glens, total).tolist()
                out, _ = sample(cond, text, total, lens=glens, steps=nfe_step, cfg_strength=cfg_strength,
                                sway_sampling_coef=sway_sampling_coef, seed=seed)
                gen = [(out, b, lens[u], end[b] - lens[u]) for b, u in enumerate(run)]
                scores[a].append(mel_distance(gen, tgt, n_cep=n_cep))
                weights[a] += [end[b] - lens[u] + int(targets[u].shape[0]) for b, u in enumerate(run)]
    finally:
        tr.set_adapter(before)
    order = [u for run in groups for u in run]
    host = torch.stack([torch.cat(scores[a]) for a in adapters]).cpu()          # [adapters, U]: the one readback
    result = {}
    for i, a in enumerate(adapters):
        per_item, D, W = [0.0] * U, 0.0, 0
        for u, v, w in zip(order, host[i].tolist(), weights[a]):
            per_item[u] = v
            D += v * w
            W += w
        result[a] = dict(mcd=D / W, per_item=per_item)
    return result


def prosody_numbers(sums: dict) -> dict:
    """(f0_rmse_cents, f0_corr, vuv_error) of a set of metrics.prosody sums (one item's, or pooled over items), host arithmetic:
    f0_rmse_cents = 1200 sqrt(sum (x - y)^2 / both_voiced), f0_corr the Pearson correlation of x and y over the both-voiced cells,
    vuv_error = vuv_mismatch / cells.  NaN where there is nothing to divide by (no cell voiced on both sides; a constant track)."""
    nan = float("nan")
    N, cells = sums["both_voiced"], sums["cells"]
    rmse = 1200.0 * math.sqrt(sums["diff2"] / N) if N > 0 else nan
    vx, vy = N * sums["x2"] - sums["x"] * sums["x"], N * sums["y2"] - sums["y"] * sums["y"]
    corr = (N * sums["xy"] - sums["x"] * sums["y"]) / math.sqrt(vx * vy) if N > 0 and vx > 0 and vy > 0 else nan
    return dict(f0_rmse_cents=rmse, f0_corr=corr, vuv_error=sums["vuv_mismatch"] / cells if cells > 0 else nan)


def heldout_prosody(model, vocoder, items, *, adapters=(None,), duration="truth", nfe_step=nfe_step, cfg_strength=cfg_strength,
                    sway_sampling_coef=sway_sampling_coef, seed=0, speed=1.0, n_cep=13, batch_frames=38400, window=1024, fmin=60.0,
                    fmax=600.0, threshold=0.15, pitch="yin", p_switch=0.01, p_absent=0.01):
    """heldout_distance with the three prosody numbers of classical objective TTS evaluation beside it, over ONE alignment: what every
    adapter GENERATES is vocoded, pitch-tracked (metrics.pitch_track: YIN on the device) and compared with the recording's track
    along the DTW path of the two mels (metrics.mel_alignment).  items: a list of U (prompt_mel [p, mel], prompt_text, target_wave
    [samples] at the mel front-end's rate, target_text) -- or a mapping adapter -> list as heldout_distance takes it; the sampler
    keywords are heldout_distance's, window / fmin / fmax / threshold pitch_track's.  vocoder: one with decode_ragged (Vocos, or
    `BigVGAN.ragged()`), matching the model's mel front-end.  Per batch the target waves go down ONCE, ONE MelSpec.forward_ragged
    gives their mels and ONE pitch_track their tracks; every adapter then runs `set_adapter`, ONE sample() as in heldout_distance,
    ONE decode_ragged of the generated frames [p_b, dur_b), ONE pitch_track of those waves, ONE mel_alignment of the generated
    frames, in place, against the target mels, and the fold (metrics.prosody).  The adapter that was active before the call is
    active again after it, on an exception too.  The only readback is one copy at the end.
    Returns {adapter: {"mcd", "f0_rmse_cents", "f0_corr", "vuv_error", "per_item": [U dicts: "mcd", metrics.prosody's counts and
    sums, and the three numbers of the item alone]}}.  "mcd" is heldout_distance's for the same items (target_mel = the mel of
    target_wave) and settings, bit for bit.  The other three are pooled from the per-item sums (prosody_numbers): log2-F0 RMSE in
    cents and Pearson correlation over the cells voiced on both sides, and the share of cells voiced on one side only; NaN, not an
    error, where no cell is voiced on both sides.
    pitch: "yin" (the default: raw YIN frames, no smoothing over time, no octave correction -- a few frames of subharmonic energy
    count as an octave error) or "pyin": both the generated and the target tracks come from metrics.pitch_track_pyin (pYIN
    candidates and a Viterbi decode; threshold is not read, p_switch / p_absent are its keywords) over ONE set of tables
    (metrics.pyin_tables(rate, fmin, fmax), built once per call); the returned dict has the same keys.  Either way these are tracks
    of vocoded audio by this project's own tracker: comparable between checkpoints and settings on the same items with the same
    `pitch`, not WORLD's F0 and not comparable with published figures."""
    from .metrics import PROSODY_SUMS, mel_alignment, pitch_track, pitch_track_pyin, prosody, pyin_tables
    if pitch not in ("yin", "pyin"):
        raise ValueError(f"heldout_prosody: pitch = {pitch!r} (expected 'yin' or 'pyin')")
    _require_ragged_vocoder(vocoder, "heldout_prosody", "there is no per-item path")
    tr, spec = model.transformer, model.mel_spec
    hop, rate = spec.hop_length, spec.target_sample_rate
    pad_, _ = spec._variant()
    centre = 0 if spec.mel_spec_type == "vocos" else hop // 2
    adapters = list(adapters)
    per_adapter = items if isinstance(items, dict) else {a: items for a in adapters}
    U = len(per_adapter[adapters[0]]) if adapters and adapters[0] in per_adapter else 0
    for a in adapters:
        if a not in per_adapter or len(per_adapter[a]) != U or U == 0:
            raise ValueError(f"heldout_prosody: adapter {a!r} needs the same items as the others, at least one")
    first = per_adapter[adapters[0]]
    waves = [it[2].reshape(-1) for it in first]
    tframes = [(int(w.shape[0]) + 2 * pad_ - spec.n_fft) // hop + 1 for w in waves]
    if min(tframes) < 1:
        raise ValueError("heldout_prosody: every target_wave needs at least one mel frame")
    # (the plan reads a target mel's frame count alone)
    plans = {a: heldout_distance_plan([(it[0], it[1], torch.empty(g, 0), it[3]) for it, g in zip(per_adapter[a], tframes)],
                                      duration=duration, speed=speed, batch_frames=batch_frames) for a in adapters}
    lens, groups = plans[adapters[0]][1], plans[adapters[0]][3]
    toks = {}
    for a in adapters:
        texts = plans[a][0]
        toks[a] = [(list_str_to_idx([t], model.vocab_char_map) if model.vocab_char_map is not None else list_str_to_tensor([t]))[0]
                   if isinstance(t, str) else torch.as_tensor(t, dtype=torch.long) for t in texts]
        if plans[a][1] != lens:
            raise ValueError(f"heldout_prosody: adapter {a!r}'s prompt mels differ in length from the first adapter's")
    pad = torch.nn.utils.rnn.pad_sequence
    sample = model.sample_items if getattr(tr, "isolated_rows", False) else model.sample
    pitch_kw = dict(sample_rate=rate, hop=hop, first_centre=centre, window=window, fmin=fmin, fmax=fmax)
    if pitch == "yin":
        pitch_kw["threshold"] = threshold
        tracker = pitch_track
    else:
        pitch_kw.update(p_switch=p_switch, p_absent=p_absent, tables=pyin_tables(rate, fmin, fmax))
        tracker = pitch_track_pyin
    names = ("cells", "both_voiced", "vuv_mismatch") + tuple(PROSODY_SUMS)
    rows = {a: [] for a in adapters}                # per batch: f64 [1 + len(names), B]
    weights = {a: [] for a in adapters}
    before = tr.active_adapter
    try:
        for run in groups:
            cond = pad([first[u][0].to("cpu", torch.float32) for u in run], batch_first=True).to(model.device)
            glens = torch.tensor([lens[u] for u in run])
            tw = ragged_items([waves[u].to(torch.float32) for u in run], model.device, "heldout_prosody only runs on a GPU (there is "
                              "no CPU path)", "heldout_prosody: the target waves are on different devices")[0]   # once per batch
            tmel, tf = spec.forward_ragged(tw)
            tmel = tmel.permute(0, 2, 1)            # [B, T_max, mel], the storage as it lies
            tgt = [(tmel, b, 0, tf[b]) for b in range(len(run))]
            t_f0, _, _ = tracker(tw, frames=tf, **pitch_kw)
            for a in adapters:
                tr.set_adapter(a)
                text = pad([toks[a][u] for u in run], padding_value=-1, batch_first=True)
                total = torch.tensor([plans[a][2][u] for u in run])
                end = clamp_durations(text, glens, total).tolist()
                out, _ = sample(cond, text, total, lens=glens, steps=nfe_step, cfg_strength=cfg_strength,
                                sway_sampling_coef=sway_sampling_coef, seed=seed)
                gf = [end[b] - lens[u] for b, u in enumerate(run)]
                wav, wav_lens = vocoder.decode_ragged(out.to(torch.float32).permute(0, 2, 1), ends=end, starts=[lens[u] for u in run])
                g_f0, _, _ = tracker(wav, [int(n) for n in wav_lens], frames=gf, **pitch_kw)
                gen = [(out, b, lens[u], gf[b]) for b, u in enumerate(run)]
                dist, path, path_start, path_len = mel_alignment(gen, tgt, n_cep=n_cep)
                fold = prosody((g_f0, gf), (t_f0, tf), path, path_start, path_len)
                rows[a].append(torch.stack([dist] + [fold[k].to(torch.float64) for k in names]))
                weights[a] += [gf[b] + tf[b] for b in range(len(run))]
    finally:
        tr.set_adapter(before)
    order = [u for run in groups for u in run]
    host = torch.stack([torch.cat(rows[a], dim=1) for a in adapters]).cpu()     # [adapters, 1 + sums, U]: the one readback
    result = {}
    for i, a in enumerate(adapters):
        per_item, D, W = [None] * U, 0.0, 0
        pooled = {k: 0.0 for k in names}
        for col, (u, w) in enumerate(zip(order, weights[a])):
            v = host[i, 0, col].item()
            sums = {k: host[i, 1 + r, col].item() for r, k in enumerate(names)}
            for k in ("cells", "both_voiced", "vuv_mismatch"):
                sums[k] = int(sums[k])
            per_item[u] = dict(mcd=v, **sums, **prosody_numbers(sums))
            D += v * w
            W += w
            for k in names:
                pooled[k] += sums[k]
        result[a] = dict(mcd=D / W, **prosody_numbers(pooled), per_item=per_item)
    return result


def heldout_speaker(model, items, *, adapters=(None,), speakers=None, against=("prompt", "target"), deltas=False, gate_db=None,
                    duration="truth", nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef, seed=0,
                    speed=1.0, n_cep=13, batch_frames=38400):
    """Whether what every adapter in `adapters` GENERATES keeps the voice of its prompt, on ONE resident engine, with no model: the
    Gaussian cepstral divergence (metrics.cepstral_moments / gaussian_divergence; include/f5_hip.h) between the generated frames and
    the prompt's, and the recording's -- text-independent, where heldout_distance and heldout_prosody compare the same sentence
    along an alignment.  It stands where the reference's evaluation has SIM (WavLM-ECAPA, eval/utils_eval.py::run_sim), which is
    not built; it is NOT SIM, not an embedding cosine and not comparable with any published figure.  It is comparable between
    checkpoints and settings on the same items and speakers.
    items, adapters, duration / speed / batch_frames and the sampler keywords: heldout_distance's, as are the plan, the batches, the
    text handling and the choice of `sample` / `sample_items`.  speakers: one label per item (None: every item is its own speaker).
    against: which of "prompt" and "target" to compare with.  deltas, gate_db, n_cep: cepstral_moments'; gate_db = None keeps every
    frame, and no threshold is recommended.  Per batch ONE cepstral_moments takes the prompts and targets together, once; every
    adapter runs `set_adapter`, ONE sample(), ONE cepstral_moments of the generated frames [p_b, dur_b), read in place, and ONE
    gaussian_divergence.  After the walk the records are pooled per speaker (metrics.merge_moments: the moments are additive, so a
    speaker's Gaussian rests on all its frames) and the pooled divergences are ONE more call per adapter.  No vocoder is involved.
    The adapter that was active before the call is active again after it, on an exception too.  The only readback is one copy at
    the end.
    Returns {adapter: {"to_prompt": {"kl", "sphericity"}, "to_target": {...}, "per_speaker": {label: {"to_prompt": {...},
    "to_target": {...}}}, "per_item": [U dicts of the same two], "singular": count}} (only the sides named in `against`).  kl: the
    symmetric Kullback-Leibler divergence of the two Gaussians in nats; sphericity: the arithmetic-harmonic sphericity measure,
    which a constant channel offset does not move (metrics.speaker_numbers).  The headline numbers are the means over speakers of
    the pooled values.  An item or speaker with too few frames for its dimension, or a covariance that is not positive definite, is
    NaN, is left out of the means and is counted in "singular" (items)."""
    from .metrics import cepstral_moments, gaussian_divergence, merge_moments, speaker_numbers, Moments
    who = "heldout_speaker"
    against = tuple(against)
    if not against or any(s not in ("prompt", "target") for s in against) or len(set(against)) != len(against):
        raise ValueError(f"{who}: against = {against!r} (expected 'prompt', 'target' or both)")
    tr = model.transformer
    adapters = list(adapters)
    per_adapter = items if isinstance(items, dict) else {a: items for a in adapters}
    U = len(per_adapter[adapters[0]]) if adapters and adapters[0] in per_adapter else 0
    for a in adapters:
        if a not in per_adapter or len(per_adapter[a]) != U or U == 0:
            raise ValueError(f"{who}: adapter {a!r} needs the same items as the others, at least one")
    speakers = list(range(U)) if speakers is None else list(speakers)
    if len(speakers) != U:
        raise ValueError(f"{who}: {len(speakers)} speaker labels for {U} items")
    plans = {a: heldout_distance_plan(per_adapter[a], duration=duration, speed=speed, batch_frames=batch_frames) for a in adapters}
    first = per_adapter[adapters[0]]
    lens, groups = plans[adapters[0]][1], plans[adapters[0]][3]
    targets = [it[2] for it in first]
    toks = {}
    for a in adapters:
        texts = plans[a][0]
        toks[a] = [(list_str_to_idx([t], model.vocab_char_map) if model.vocab_char_map is not None else list_str_to_tensor([t]))[0]
                   if isinstance(t, str) else torch.as_tensor(t, dtype=torch.long) for t in texts]
        if plans[a][1] != lens:
            raise ValueError(f"{who}: adapter {a!r}'s prompt mels differ in length from the first adapter's")
    pad = torch.nn.utils.rnn.pad_sequence
    sample = model.sample_items if getattr(tr, "isolated_rows", False) else model.sample
    mom_kw = dict(n_cep=n_cep, deltas=deltas, gate_db=gate_db)
    refs = []                                       # per batch: Moments of [prompts of the run | targets of the run]
    gens = {a: [] for a in adapters}                # per batch: Moments of the generated frames
    terms = {a: [] for a in adapters}               # per batch: ([B * sides, 4], [B * sides])
    before = tr.active_adapter
    try:
        for run in groups:
            B = len(run)
            cond = pad([first[u][0].to("cpu", torch.float32) for u in run], batch_first=True).to(model.device)
            glens = torch.tensor([lens[u] for u in run])
            both = ragged_items([first[u][0].to(torch.float32) for u in run] + [targets[u].to(torch.float32) for u in run], model.device,
                                f"{who} only runs on a GPU (there is no CPU path)",
                                f"{who}: the prompt and target mels are on different devices")[0]   # once per batch
            ref = cepstral_moments([t.view(-1, model.num_channels) for t in both], **mom_kw)
            refs.append(ref)
            pairs = [(b, b + B * (side == "target")) for side in against for b in range(B)]
            for a in adapters:
                tr.set_adapter(a)
                text = pad([toks[a][u] for u in run], padding_value=-1, batch_first=True)
                total = torch.tensor([plans[a][2][u] for u in run])
                end = clamp_durations(text, glens, total).tolist()
                out, _ = sample(cond, text, total, lens=glens, steps=nfe_step, cfg_strength=cfg_strength,
                                sway_sampling_coef=sway_sampling_coef, seed=seed)
                gen = cepstral_moments([(out, b, lens[u], end[b] - lens[u]) for b, u in enumerate(run)], **mom_kw)
                gens[a].append(gen)
                terms[a].append(gaussian_divergence(gen, ref, pairs))
    finally:
        tr.set_adapter(before)
    order = [u for run in groups for u in run]
    sizes = [len(run) for run in groups]

    def cat(records, part=None):
        """The records of every batch in one Moments, in `order`; part 0 / 1: the prompt / target half of each batch's references."""
        pick = (lambda t, B: t) if part is None else (lambda t, B: t[part * B:(part + 1) * B])   # noqa: E731
        return Moments(*[torch.cat([pick(getattr(m, f), B) for m, B in zip(records, sizes)]) for f in ("count", "mean", "scatter")],
                       records[0].n_cep, records[0].deltas)
    labels_in_order = [speakers[u] for u in order]
    pooled_ref = {side: merge_moments(cat(refs, part=int(side == "target")), labels_in_order) for side in against}
    labels = pooled_ref[against[0]][1]
    L, dim = len(labels), refs[0].dim
    flat = []
    for a in adapters:
        pooled_gen, _ = merge_moments(cat(gens[a]), labels_in_order)
        for side in against:
            t, s = gaussian_divergence(pooled_gen, pooled_ref[side][0])
            flat.append(torch.cat([t, s.to(torch.float64).unsqueeze(1)], dim=1))
        flat += [torch.cat([t, s.to(torch.float64).unsqueeze(1)], dim=1) for t, s in terms[a]]
    host = torch.cat(flat).cpu().tolist()           # the one readback
    names = {"prompt": "to_prompt", "target": "to_target"}
    result, at = {}, 0
    for a in adapters:
        res = dict(per_speaker={g: {} for g in labels}, per_item=[{} for _ in range(U)], singular=0)
        for side in against:
            rows = host[at:at + L]
            at += L
            nums = speaker_numbers([r[:4] for r in rows], dim)
            for k, g in enumerate(labels):
                res["per_speaker"][g][names[side]] = dict(kl=nums["kl"][k], sphericity=nums["sphericity"][k])
            good = [k for k in range(L) if rows[k][4] == 0]
            res[names[side]] = {key: (math.fsum(nums[key][k] for k in good) / len(good) if good else float("nan"))
                                for key in ("kl", "sphericity")}
        singular = set()
        done = 0
        for B in sizes:
            run = order[done:done + B]
            done += B
            for side in against:
                rows = host[at:at + B]
                at += B
                nums = speaker_numbers([r[:4] for r in rows], dim)
                for b, u in enumerate(run):
                    res["per_item"][u][names[side]] = dict(kl=nums["kl"][b], sphericity=nums["sphericity"][b])
                    if rows[b][4] != 0:
                        singular.add(u)
        res["singular"] = len(singular)
        result[a] = res
    return result


def infer_process(ref_audio, ref_text, gen_text, model_obj, vocoder, mel_spec_type=mel_spec_type, show_info=print, progress=None,
                  target_rms=target_rms, cross_fade_duration=cross_fade_duration, nfe_step=nfe_step, cfg_strength=cfg_strength,
                  sway_sampling_coef=sway_sampling_coef, speed=speed, fix_duration=fix_duration, device=None, seed=None,
                  text_tokenizer=None, batched=False, batch_frames=None, prompt_on_device=False, clip_silence=False,
                  remove_silence=False):
    """ref_audio = (tensor [channels, nw], sample_rate) instead of a path (no torchaudio.load here); otherwise
    utils_infer.py:453-498: max_chars from the prompt's bytes-per-second, chunk, infer_batch_process.
    batched=True (default False: the sequential path, unchanged) runs the chunks as ragged batches of at most `batch_frames`
    and cross-fades on the device (infer_batch_process, synthesize_long): the waveform is then f32 where the sequential one is
    float64 after a cross-fade, and a chunk's mel equals the chunk run alone only with `attn_mask_enabled=True`.
    prompt_on_device=True (batched=True only): the prompt is mixed, levelled and resampled on the device.
    clip_silence=True (prompt_on_device=True only): the prompt is clipped on the device first (clip_prompts), as
    preprocess_ref_audio_text does before the reference calls this function, so max_chars comes from the clipped length.
    remove_silence=True (batched=True only): pauses of 1 s or more are cut out of the result on the device (remove_silence)."""
    audio, sr = ref_audio
    if clip_silence:
        if not (batched and prompt_on_device):
            raise ValueError("infer_process: clip_silence=True needs batched=True and prompt_on_device=True (the clip runs on the device)")
        audio = clip_prompts([audio], [sr], device=device if device is not None else model_obj.device)[0][0]
    max_chars = int(len(ref_text.encode("utf-8")) / (audio.shape[-1] / sr) * (22 - audio.shape[-1] / sr) * speed)
    batches = chunk_text(gen_text, max_chars=max_chars)
    if show_info is not None:
        show_info(f"Generating audio in {len(batches)} batches...")
    return next(infer_batch_process((audio, sr), ref_text, batches, model_obj, vocoder, mel_spec_type=mel_spec_type,
                                    progress=progress, target_rms=target_rms, cross_fade_duration=cross_fade_duration,
                                    nfe_step=nfe_step, cfg_strength=cfg_strength, sway_sampling_coef=sway_sampling_coef,
                                    speed=speed, fix_duration=fix_duration, device=device, seed=seed,
                                    text_tokenizer=text_tokenizer, batched=batched, batch_frames=batch_frames,
                                    prompt_on_device=prompt_on_device, remove_silence=remove_silence))
