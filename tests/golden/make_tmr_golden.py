#!/usr/bin/env python3
"""Golden outputs of the reference's two TMR encoders (models/temos/motionencoder/actor.py, textencoder/distillbert_actor.py), run on CPU
in fp32 with the seeded weights and inputs of syntalker_amd.synth (synth_tmr_*).  Runs in the build container only.

pytorch_lightning is not installed: a shim supplies LightningModule (nn.Module + save_hyperparameters recording the constructor's
arguments in self.hparams), which is all the temos modules use of it.  DistilBERT is a seeded, synthetic local directory
(synth.synth_tmr_text_model), read offline.  Stored: loc / scale, the state_dict keys and shapes, the token ids and masks.
    python tests/golden/make_tmr_golden.py
"""
import inspect
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, import_reference  # noqa: E402,F401

os.environ["HF_HUB_OFFLINE"] = "1"
from syntalker_amd import synth  # noqa: E402

MOTION_LENGTHS = [128, 97, 64, 33, 1, 128, 128, 2]


def lightning_shim():
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(torch.nn.Module):
        def save_hyperparameters(self, logger=False):
            frame = inspect.currentframe().f_back
            args = inspect.getargvalues(frame)
            hp = {k: args.locals[k] for k in args.args if k != "self"}
            hp.update(args.locals.get(args.keywords, {}) if args.keywords else {})
            self.hparams = types.SimpleNamespace(**hp)
    pl.LightningModule = LightningModule
    sys.modules["pytorch_lightning"] = pl


def main():
    torch.manual_seed(0)
    lightning_shim()
    sys.path.insert(0, os.path.join(REF, "models"))
    from temos.motionencoder.actor import ActorAgnosticEncoder
    from temos.textencoder.distillbert_actor import DistilbertActorAgnosticEncoder
    out = {}
    motion = ActorAgnosticEncoder(nfeats=synth.TMR_NFEATS, vae=True, num_layers=4).eval()
    motion.load_state_dict(synth.synth_tmr_state_dict(motion))
    sd = motion.state_dict()
    out["motion_keys"] = np.array(list(sd.keys()))
    out["motion_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    with torch.no_grad():
        x = synth.synth_tmr_motion(8, 128)
        d = motion(x, MOTION_LENGTHS)
        out["motion8_loc"], out["motion8_scale"] = d.loc.numpy(), d.scale.numpy()
        out["motion8_lengths"] = np.array(MOTION_LENGTHS, np.int32)
        d = motion(synth.synth_tmr_motion(200, 128, seed=34))
        out["motion200_loc"], out["motion200_scale"] = d.loc.numpy(), d.scale.numpy()
    with tempfile.TemporaryDirectory() as td:
        synth.synth_tmr_text_model(td)
        text = DistilbertActorAgnosticEncoder(td, num_layers=4).eval()
        text.load_state_dict(synth.synth_tmr_state_dict(text))
        sd = text.state_dict()
        out["text_keys"] = np.array(list(sd.keys()))
        out["text_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        with torch.no_grad():
            for name, prompts in (("text3", synth.TMR_PROMPTS), ("text1", synth.TMR_PROMPT_ONE)):
                enc = text.tokenizer(prompts, return_tensors="pt", padding=True)
                out[name + "_ids"], out[name + "_mask"] = enc["input_ids"].numpy(), enc["attention_mask"].numpy()
                d = text(prompts)
                out[name + "_loc"], out[name + "_scale"] = d.loc.numpy(), d.scale.numpy()
    path = os.path.join(HERE, "tmr_outputs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
