#!/usr/bin/env python3
"""Golden outputs of the reference's FGD evaluator, `VAESKConv.map2latent` (models/motion_representation.py:67-75), run on CPU in fp32 with
the seeded weights of syntalker_amd.synth (synth_evaluator_*).  Runs in the build container only.

smplx, lmdb, fasttext and loguru are stubbed (make_golden.import_reference stubs the last three); `data_path_1` points at a temporary
directory whose SMPL-X npz holds only the kintree_table of tests/golden/smplx_kintree.json.  Stored: the state_dict keys and shapes, each
layer's edges, neighbour lists and pooling lists, the outputs for the inputs of synth.EVALUATOR_CASES (regenerated from their seeds, not
stored) and the fp64 FGD of the two take sets of synth.EVALUATOR_FGD_TAKES over the reference's embeddings.
    python tests/golden/make_evaluator_golden.py
"""
import json
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, import_reference  # noqa: E402,F401

from syntalker_amd import metrics, synth  # noqa: E402

ARGS = dict(vae_layer=4, vae_grow=[1, 1, 2, 1], vae_length=240, vae_test_dim=330, vae_test_len=32, variational=False)


def main():
    torch.manual_seed(0)
    import_reference()
    sys.modules.setdefault("smplx", types.ModuleType("smplx"))
    from models.motion_representation import VAESKConv
    parents = json.load(open(os.path.join(HERE, "smplx_kintree.json")))["parents"]
    out = {}
    with tempfile.TemporaryDirectory() as td:
        os.makedirs(os.path.join(td, "smplx_models", "smplx"))
        np.savez(os.path.join(td, "smplx_models", "smplx", "SMPLX_NEUTRAL_2020.npz"),
                 kintree_table=np.stack([np.array(parents, np.int64), np.arange(len(parents))]))
        m = VAESKConv(SimpleNamespace(data_path_1=td + "/", **ARGS)).eval()
    m.load_state_dict(synth.synth_evaluator_state_dict(m), strict=True)
    sd = m.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    enc = m.encoder
    topo = []
    for i in range(len(enc.layers)):
        blk = enc.layers[i][0]
        topo.append(dict(edges=[list(map(int, e)) for e in enc.topologies[i]], neighbours=blk.shortcut.neighbour_list,
                         pooling=[list(map(int, p)) for p in enc.pooling_list[i]], pooled=len(blk.common) == 2,
                         cin=int(blk.shortcut.weight.shape[1]), cout=int(blk.shortcut.weight.shape[0])))
    out["topology"] = np.array(json.dumps(topo))
    with torch.no_grad():
        for b, n, seed in synth.EVALUATOR_CASES:
            out[f"out_{b}x{n}"] = m.map2latent(synth.synth_evaluator_input(b, n, seed)).numpy()
        emb = {}
        for name, (lengths, seed, scale, shift) in synth.EVALUATOR_FGD_TAKES.items():
            rows = []
            for take in synth.synth_evaluator_takes(lengths, seed, scale, shift):
                n = take.shape[0] - take.shape[0] % ARGS["vae_test_len"]
                rows.append(m.map2latent(take[None, :n]).reshape(-1, ARGS["vae_length"]).numpy())
            emb[name] = np.concatenate(rows, 0)
    out["fgd_rows"] = np.array([emb["rec"].shape[0], emb["tar"].shape[0]])
    out["fgd"] = np.array(metrics.frechet_distance(emb["rec"], emb["tar"]), np.float64)
    path = os.path.join(HERE, "evaluator_outputs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()}, "fgd", float(out["fgd"]))


if __name__ == "__main__":
    main()
