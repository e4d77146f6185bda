#!/usr/bin/env python3
"""The SMPL-X meshes of a results directory as the reference's `test()` writes it (diffusion_rvqvae_trainer.py:702-709: `res_<id>.npz` with `poses`
(n, 165) axis-angle, `expressions` (n, 100), `trans` (n, 3), `betas`): what `render_one_sequence_no_gt` computes with `smplx` before it draws
(utils/other_tools_hf.py:718-730), on the device (syntalker_amd.mesh; `smplx` is not needed).

    python scripts/mesh_from_results.py RESULTS_DIR --smplx-model SMPLX_NEUTRAL_2020.npz [--out DIR]

Writes `verts_<id>.npy` (n, 10475, 3) float32 per take and `faces.npy` (the model's `f`) into --out (default: RESULTS_DIR).  Rendering is not here.
--flat-hand-mean   for results made with a model built with flat_hand_mean=True
--prefix           `res` (default) or `gt`
Prints one JSON line: {"takes", "frames", "vertices", "out"}.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import mesh  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("results_dir")
    ap.add_argument("--smplx-model", required=True)
    ap.add_argument("--out")
    ap.add_argument("--prefix", default="res", choices=("res", "gt"))
    ap.add_argument("--flat-hand-mean", action="store_true")
    a = ap.parse_args(argv)
    head = a.prefix + "_"
    ids = sorted(n[len(head):-len(".npz")] for n in os.listdir(a.results_dir) if n.startswith(head) and n.endswith(".npz"))
    if not ids:
        raise SystemExit(f"mesh_from_results: no {head}<id>.npz in {a.results_dir}")
    out_dir = a.out or a.results_dir
    os.makedirs(out_dir, exist_ok=True)
    model = dict(np.load(a.smplx_model, allow_pickle=True))
    dev = torch.device("cuda")
    to_dev = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dev)
    frames, faces = 0, None
    for i in ids:
        res = np.load(os.path.join(a.results_dir, f"{head}{i}.npz"), allow_pickle=True)
        pose = to_dev(res["poses"])
        n = pose.shape[0]
        ex = np.asarray(res["expressions"], dtype=np.float32).reshape(n, -1)
        m = mesh.smplx_mesh(model, np.asarray(res["betas"], dtype=np.float64).reshape(-1), num_expression_coeffs=ex.shape[1], flat_hand_mean=a.flat_hand_mean)
        verts = mesh.smplx_vertices(m, pose.reshape(n, -1), to_dev(ex), to_dev(res["trans"]).reshape(n, 3))
        np.save(os.path.join(out_dir, f"verts_{i}.npy"), verts.cpu().numpy())
        frames, faces = frames + n, m.faces
    if faces is not None:
        np.save(os.path.join(out_dir, "faces.npy"), faces)
    out = {"takes": len(ids), "frames": int(frames), "vertices": int(verts.shape[1]), "out": out_dir}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
