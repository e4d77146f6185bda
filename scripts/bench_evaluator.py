#!/usr/bin/env python3
"""FGD evaluator timing (not the contract bench): VAESKConv.map2latent on the HIP kernels (syn_skel_encode) vs the torch fp32 restatement
(tests/evaluator_ref.py: F.conv1d with the masked weights, F.group_norm, the pooling matmul, tanh) on the same GPU, alternated in one
process, device-event time per call.  Seeded weights, the SMPL-X tree of tests/golden/smplx_kintree.json.

    python scripts/bench_evaluator.py [--reps 20] [--rounds 5]

Cases: one 60 s take (1792 frames at 30 fps, a multiple of 16) and 64 of them.  Also printed: each layer's kept fraction of K chunks."""
import argparse
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import evaluator, synth  # noqa: E402
from tests import evaluator_ref  # noqa: E402

FRAMES = 1792


def build(dev):
    parents = json.load(open(os.path.join(REPO, "tests", "golden", "smplx_kintree.json")))["parents"]
    with tempfile.TemporaryDirectory() as td:
        synth.synth_smplx_model(td, parents)
        m = evaluator.VAESKConv(SimpleNamespace(data_path_1=td + "/", vae_layer=4, vae_grow=[1, 1, 2, 1], vae_length=240,
                                                vae_test_dim=330, variational=False))
    m.load_state_dict(synth.synth_evaluator_state_dict(m))
    return m.to(dev)


def time_pair(hip, ref, reps, rounds):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {"hip": [], "torch": []}
    for _ in range(3):
        hip(), ref()
    for _ in range(rounds):
        for name, fn in (("hip", hip), ("torch", ref)):
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    m = build("cuda")
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    print(json.dumps({"kept_k_fraction": [round(f, 4) for f in m.kept_fraction()]}), flush=True)
    results = []
    with torch.no_grad():
        for b in (1, 64):
            x = torch.randn(b, FRAMES, 330, device="cuda")
            got, want = m.map2latent(x), evaluator_ref.encode(sd, x)
            err = float((got - want).norm() / want.norm())
            t = time_pair(lambda: m.map2latent(x), lambda: evaluator_ref.encode(sd, x), a.reps, a.rounds)
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            r = {"takes": b, "frames": FRAMES, "hip_us": round(med["hip"], 1), "hip_us_range": [round(min(t["hip"]), 1), round(max(t["hip"]), 1)],
                 "torch_fp32_us": round(med["torch"], 1), "torch_us_range": [round(min(t["torch"]), 1), round(max(t["torch"]), 1)],
                 "speedup": round(med["torch"] / med["hip"], 2), "hip_us_per_take": round(med["hip"] / b, 2),
                 "rel_l2_vs_torch_fp32": float(f"{err:.3e}")}
            results.append(r)
            print(json.dumps(r), flush=True)
    return results


if __name__ == "__main__":
    main()
