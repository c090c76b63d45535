"""CPU: the helpers the drivers of korean-f5-tts_amd/infer.py share -- checkpoint reading (load_checkpoint against
_read_checkpoint_state_dict), the text front-end (_tokenise against the expressions it replaced in synthesize_long,
synthesize_prompts and synthesize_batch) and the frame the untokenised-text warning is attributed to."""
import warnings

import pytest
import torch

from f5_tts_amd import infer as I
from f5_tts_amd.utils import list_str_to_idx, list_str_to_tensor

LEGACY = ("mel_spec.mel_stft.mel_scale.fb", "mel_spec.mel_stft.spectrogram.window")


class Recorder:
    """What load_checkpoint needs of a CFM."""

    def load_state_dict(self, sd):
        self.sd = sd

    def to(self, device):
        self.device = device
        return self


def checkpoint_tensors():
    g = torch.Generator().manual_seed(0)
    plain = {"transformer.a.weight": torch.randn(4, 3, generator=g), "transformer.a.bias": torch.randn(4, generator=g)}
    peft = {"base_model.model.l.base_layer.weight": torch.randn(4, 6, generator=g), "base_model.model.l.base_layer.bias": torch.randn(4, generator=g),
            "base_model.model.l.lora_A.default.weight": torch.randn(2, 6, generator=g),
            "base_model.model.l.lora_B.default.weight": torch.randn(4, 2, generator=g), "base_model.model.t.weight": torch.randn(5, generator=g)}
    legacy = {k: torch.randn(3, generator=g) for k in LEGACY}
    return plain, peft, legacy


def write_checkpoint(tmp_path, kind, use_ema, weights):
    plain, _peft, legacy = checkpoint_tensors()
    ema = {"ema_model." + k: v for k, v in {**weights, **legacy}.items()}
    if kind == "pt":
        path = str(tmp_path / "model.pt")
        torch.save({"ema_model_state_dict": {**ema, "initted": torch.tensor(True), "step": torch.tensor(7)},
                    "model_state_dict": {**weights, **legacy}}, path)
    else:
        save_file = pytest.importorskip("safetensors.torch").save_file
        path = str(tmp_path / "model.safetensors")
        save_file(ema if use_ema else {**weights, **legacy}, path)
    return path


@pytest.mark.parametrize("use_ema", [True, False])
@pytest.mark.parametrize("which", ["plain", "peft"])
@pytest.mark.parametrize("kind", ["pt", "safetensors"])
def test_load_checkpoint_agrees_with_read_checkpoint_state_dict(tmp_path, kind, which, use_ema):
    plain, peft, _legacy = checkpoint_tensors()
    weights = plain if which == "plain" else peft
    path = write_checkpoint(tmp_path, kind, use_ema, weights)
    read = I._read_checkpoint_state_dict(path, use_ema)
    want = I.convert_peft_state_dict_to_plain(read)
    model = Recorder()
    assert I.load_checkpoint(model, path, "cpu", use_ema=use_ema) is model and model.device == "cpu"
    assert list(model.sd) == list(want)
    assert all(torch.equal(model.sd[k], want[k]) for k in want)
    # ... and both are what the file holds: the EMA prefix and bookkeeping gone, the legacy mel buffers dropped from EMA weights only
    assert not any(k.startswith("ema_model.") or k in ("initted", "step") for k in read)
    assert all((k in read) == (not use_ema) for k in LEGACY)
    if which == "plain":
        assert all(torch.equal(model.sd[k], v) for k, v in plain.items())
    else:
        merged = peft["base_model.model.l.base_layer.weight"] + \
            (peft["base_model.model.l.lora_B.default.weight"] @ peft["base_model.model.l.lora_A.default.weight"]) * (32.0 / 16)
        assert torch.equal(model.sd["l.weight"], merged) and torch.equal(model.sd["t.weight"], peft["base_model.model.t.weight"])


class Model:
    device = "cpu"

    def __init__(self, vocab):
        self.vocab_char_map = vocab


VOCAB = {c: i + 1 for i, c in enumerate("abcdefgh ")}
TEXTS = ["abc def", "hgfedcba abc xyz", "a"]


@pytest.mark.parametrize("vocab", [VOCAB, None])
@pytest.mark.parametrize("tokenizer", [None, "given"])
def test_tokenise_equals_the_expressions_it_replaced(vocab, tokenizer):
    # a vocabulary maps tokens (the reference's tokenisers return list[str]); without one the text is utf-8 bytes of a str
    tok = None if tokenizer is None else ((lambda t: [c + c for c in t]) if vocab is not None else str.upper)
    model = Model(vocab)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        texts, idx = I._tokenise(model, TEXTS, tok, stacklevel=2)
    want_texts = [tok(t) for t in TEXTS] if tok is not None else TEXTS          # synthesize_long / synthesize_prompts
    want = list_str_to_idx(want_texts, vocab) if vocab is not None else list_str_to_tensor(want_texts)
    assert texts == want_texts and torch.equal(idx, want)
    if tok is None:                                                            # synthesize_batch's list branch
        assert torch.equal(I._tokenise(model, TEXTS, None, stacklevel=None)[1], want)


class Stop(Exception):
    pass


class WarnModel(Model):
    """A model that stops a driver at its first device call (the warning comes before it)."""

    def mel_spec(self, *a, **k):
        raise Stop

    def sample(self, *a, **k):
        raise Stop


class RaggedMel:
    def forward_ragged(self, wavs, device=None):
        frames = [int(w.shape[-1]) // 256 + 1 for w in wavs]
        return torch.zeros(len(wavs), 100, max(frames)), frames


class RaggedVocoder:
    def decode_ragged(self, *a, **k):
        raise Stop


def test_untokenised_text_warning_points_at_the_public_callers_frame():
    model = WarnModel({c: i for i, c in enumerate("0123456789")})     # no letter is in this vocabulary
    audio = torch.full((1, 24000), 0.05)

    def caught(call):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with pytest.raises(Stop):
                call()
        w = [x for x in w if issubclass(x.category, RuntimeWarning) and "text_tokenizer=" in str(x.message)]
        assert w, "no untokenised-text warning"
        return w

    w = caught(lambda: I.synthesize_long((audio, 24000), "some prompt text", ["first chunk of text.", "second chunk."], model, RaggedVocoder()))
    assert len(w) == 2 and all(x.filename == __file__ for x in w), [x.filename for x in w]
    model.mel_spec = RaggedMel()
    w = caught(lambda: I.synthesize_prompts(model, RaggedVocoder(), [(audio, 24000, "some prompt text")], ["text to say."]))
    assert len(w) == 1 and w[0].filename == __file__, [x.filename for x in w]
    with warnings.catch_warnings(record=True) as none:                         # synthesize_batch itself never warned
        warnings.simplefilter("always")
        with pytest.raises(Stop):
            I.synthesize_batch(model, RaggedVocoder(), torch.zeros(1, 94, 100), ["some prompt text to say."], torch.tensor([200]), lens=[94])
    assert not [x for x in none if "text_tokenizer=" in str(x.message)]
