#!/usr/bin/env python3
"""Golden outputs for DistilBERT on the HIP kernels (tests/test_gpu_distilbert.py): the reference's DistilbertActorAgnosticEncoder
(models/temos/textencoder/distillbert_actor.py) on the CPU in fp32, on the seeded synthetic DistilBERT directories of
synth.synth_tmr_text_model(seed=33) at 2 and 6 layers with synth.synth_tmr_state_dict loaded.  Runs in the build container only.

Stored per depth n (prefix `l{n}_`):
  a  synth.TMR_PROMPTS (`text3`) and TMR_PROMPT_ONE (`text1`): ids, lengths, last_hidden_state's valid rows (concatenated prompt after prompt),
     loc / scale;
  b  (2 layers only, `ragged`) synth.synth_tmr_prompts(synth.TMR_RAGGED_TOKENS): ids, lengths, loc / scale and the hidden rows ROWS of every
     prompt that has them (`ragged_rows`: prompt, row pairs; `ragged_hidden`: the rows in that order).
    python tests/golden/make_distilbert_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402
from make_tmr_golden import lightning_shim  # noqa: E402

os.environ["HF_HUB_OFFLINE"] = "1"
from syntalker_amd import synth  # noqa: E402

ROWS = (0, 1, 15, 16, 63, 64, 65, 127, 128)          # and each prompt's last row


def main():
    torch.manual_seed(0)
    lightning_shim()
    sys.path.insert(0, os.path.join(REF, "models"))
    from temos.textencoder.distillbert_actor import DistilbertActorAgnosticEncoder
    out = {}
    for layers in (2, 6):
        with tempfile.TemporaryDirectory() as td:
            synth.synth_tmr_text_model(td, seed=33, layers=layers)
            text = DistilbertActorAgnosticEncoder(td, num_layers=4).eval()
            text.load_state_dict(synth.synth_tmr_state_dict(text))
            sets = [("text3", synth.TMR_PROMPTS), ("text1", [synth.TMR_PROMPT_ONE])]
            if layers == 2:
                sets.append(("ragged", synth.synth_tmr_prompts(synth.TMR_RAGGED_TOKENS)))
            with torch.no_grad():
                for name, prompts in sets:
                    key = f"l{layers}_{name}_"
                    enc = text.tokenizer(prompts, return_tensors="pt", padding=True)
                    ids, mask = enc["input_ids"], enc["attention_mask"]
                    lengths = mask.sum(1).tolist()
                    hidden = text.text_model(input_ids=ids, attention_mask=mask).last_hidden_state
                    d = text(prompts)
                    out[key + "ids"], out[key + "lengths"] = ids.numpy().astype(np.int32), np.array(lengths, np.int32)
                    out[key + "loc"], out[key + "scale"] = d.loc.numpy(), d.scale.numpy()
                    if name == "ragged":
                        assert tuple(lengths) == synth.TMR_RAGGED_TOKENS, lengths
                        rows = [(b, r) for b, n in enumerate(lengths) for r in sorted({r for r in ROWS if r < n} | {n - 1})]
                        out[key + "rows"] = np.array(rows, np.int32)
                        out[key + "hidden"] = np.stack([hidden[b, r].numpy() for b, r in rows])
                    else:
                        out[key + "hidden"] = np.concatenate([hidden[b, :n].numpy() for b, n in enumerate(lengths)])
    path = os.path.join(HERE, "distilbert_outputs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
