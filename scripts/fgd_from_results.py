#!/usr/bin/env python3
"""FGD of a results directory as the reference's `test()` writes it (diffusion_rvqvae_trainer.py:693-709: `res_<id>.npz` generated and
`gt_<id>.npz` ground truth, `poses` (n, 165) SMPL-X axis-angle), with the reference's evaluator (VAESKConv, `data_path + e_path`).

    python scripts/fgd_from_results.py RESULTS_DIR -c config.yaml [--random-init]

Each pose goes to the 6D representation (poses.axis_angle_to_rotation_6d), then metrics.fgd (takes trimmed to multiples of
`vae_test_len`).  The SMPL-X tree comes from the config's `data_path_1`.  A file without its partner is skipped (named on stderr).
--random-init   the seeded evaluator weights of synth.synth_evaluator_state_dict instead of the checkpoint.
Prints one JSON line: {"takes", "frames", "fgd"}.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import config, metrics, poses, synth  # noqa: E402


def read_pairs(results_dir: str):
    names = set(os.listdir(results_dir))
    ids = sorted(n[len("res_"):-len(".npz")] for n in names if n.startswith("res_") and n.endswith(".npz"))
    pairs = [i for i in ids if f"gt_{i}.npz" in names]
    lone = sorted({f"res_{i}.npz" for i in ids if i not in pairs} |
                  {n for n in names if n.startswith("gt_") and n.endswith(".npz") and n[len("gt_"):-len(".npz")] not in ids})
    for n in lone:
        print(f"fgd_from_results: {n} has no partner, skipped", file=sys.stderr)
    return pairs


def to_6d(path: str, dev) -> torch.Tensor:
    aa = torch.from_numpy(np.load(path)["poses"]).float().to(dev)
    return poses.axis_angle_to_rotation_6d(aa.reshape(aa.shape[0], -1, 3)).reshape(aa.shape[0], -1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("results_dir")
    ap.add_argument("-c", "--config", required=True)
    ap.add_argument("--random-init", action="store_true")
    a = ap.parse_args(argv)
    args = config.load_args(a.config)
    ev = config.build_evaluator(args, load=not a.random_init)
    if a.random_init:
        ev.load_state_dict(synth.synth_evaluator_state_dict(ev))
    dev = next(ev.parameters()).device
    ids = read_pairs(a.results_dir)
    if not ids:
        raise SystemExit(f"fgd_from_results: no res_<id>.npz / gt_<id>.npz pairs in {a.results_dir}")
    rec = [to_6d(os.path.join(a.results_dir, f"res_{i}.npz"), dev) for i in ids]
    tar = [to_6d(os.path.join(a.results_dir, f"gt_{i}.npz"), dev) for i in ids]
    out = {"takes": len(ids), "frames": int(sum(t.shape[0] for t in rec)),
           "fgd": metrics.fgd(ev, rec, tar, int(getattr(args, "vae_test_len", 32)))}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
