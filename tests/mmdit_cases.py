"""What the MMDiT tests share: the sample fixtures' names, their weights and their sample() arguments."""
import torch

import f5_tts_amd as P

SAMPLE_FIXTURES = ["mmdit_b1_nfe4", "mmdit_b3_ragged", "mmdit_b2_qknorm", "mmdit_b1_nocfg"]


def mmdit_weights(meta):
    """The fixture's weights: synthetic_state_dict at the std its meta records, checked against its checksum."""
    sd = P.weights.synthetic_state_dict(P.weights.mmdit_param_shapes(meta["arch"], meta["nvocab"]), seed=meta["wseed"], std=meta["std"])
    chk = float(sum(v.double().abs().sum().item() for v in sd.values()))
    assert abs(chk - meta["weights_checksum"]) <= 1e-6 * abs(chk), "synthetic weight generator drifted from the fixtures"
    return sd


def sample_kwargs(meta, a):
    kw = dict(steps=meta["steps"], cfg_strength=meta["cfg_strength"], sway_sampling_coef=meta["sway"], seed=meta["seed"],
              use_epss=meta["use_epss"])
    if meta["lens"] is not None:
        kw["lens"] = torch.tensor(meta["lens"])
    if "edit_mask" in a:
        kw["edit_mask"] = a["edit_mask"]
    dur = meta["duration"]
    return (dur if isinstance(dur, int) else torch.tensor(dur)), kw
