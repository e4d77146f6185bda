#!/usr/bin/env python3
"""SMPL-X mesh timing (not the contract bench): pose, expression and transl -> the 10 475 vertices per frame, for one take of 60 s (1800 frames at
30 fps) and for 8 of them, on a SYNTHETIC model of the real size (V = 10 475, 55 joints, E = 100; tests/smplx_mesh_ref.synth_model - the model file
is not redistributable and `smplx` is not installed: `smplx` itself was never run, here or anywhere in this project), two ways:

  hip    syntalker_amd.mesh.smplx_vertices: syn_fk_transforms + syn_mesh_vertices (csrc/syn_mesh.inc)
  torch  the same algebra in torch fp32 ops on the same GPU (tests/smplx_mesh_ref.lbs_torch32: dense weights and a 3 x 4 per vertex and frame, as
         `smplx` forms them), `--chunk` frames at a time so that it fits

hip and torch alternate in one process after two warm-up calls each; device-event time per call, median and min..max over the rounds.  Per case the
file records the time per take, the achieved fp32 FLOP/s of the corrective product (2 x frames x 3 V x Kc) against the 157 TF matrix peak, and the
output bytes/s (frames x V x 12 B).

    python scripts/bench_mesh.py [--reps 5] [--rounds 5] [--chunk 200] [--out profiles/mesh_bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import mesh  # noqa: E402
from tests import smplx_mesh_ref as sm  # noqa: E402

FRAMES, V, E = 1800, 10475, 100
PEAK_FP32_MATRIX = 157e12


def timed(fns, reps, rounds):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn(), fn()
    for _ in range(rounds):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / reps)
    return {k: {"us": round(sorted(v)[len(v) // 2], 1), "us_range": [round(min(v), 1), round(max(v), 1)]} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_bench.txt"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    dev = "cuda"
    md = sm.synth_model(0, V, E=E, max_weights=8)
    md_dev = {k: torch.from_numpy(np.ascontiguousarray(md[k].astype(np.float32))).to(dev) for k in ("shapedirs", "v_template", "posedirs", "J_regressor", "weights")}
    md_dev.update({k: md[k] for k in ("hands_meanl", "hands_meanr")})
    lines = [f"# scripts/bench_mesh.py --reps {a.reps} --rounds {a.rounds} --chunk {a.chunk}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# synthetic model of SMPL-X's size (V = {V}, 55 joints, E = {E}, weight lists 8 wide); a take = {FRAMES} frames; `torch` = the same algebra "
             "in torch fp32 on the same GPU; smplx itself was never run.  Times in us per call (median [min, max] over the rounds)"]
    for takes in (1, 8):
        n = takes * FRAMES
        betas = np.random.RandomState(1).randn(takes, 300).astype(np.float32)
        pose_np = np.concatenate([sm.case_inputs(100 + s, FRAMES, E, transl=True)[0] for s in range(takes)])
        r = np.random.RandomState(2)
        pose, ex, tr = torch.from_numpy(pose_np).to(dev), torch.from_numpy(r.randn(n, E).astype(np.float32)).to(dev), torch.from_numpy(r.randn(n, 3).astype(np.float32)).to(dev)
        m = mesh.smplx_mesh(md, betas)

        def hip():
            return mesh.smplx_vertices(m, pose, ex, tr)

        def torch_path():
            return torch.cat([sm.lbs_torch32(md_dev, betas[k], pose[k * FRAMES:(k + 1) * FRAMES], ex[k * FRAMES:(k + 1) * FRAMES], tr[k * FRAMES:(k + 1) * FRAMES],
                                             device=dev, chunk=a.chunk, as_numpy=False)[0] for k in range(takes)])
        agree = float((hip() - torch_path()).abs().max())
        t = timed({"hip": hip, "torch": torch_path}, a.reps, a.rounds)
        flops, out_bytes = 2.0 * n * 3 * V * m.n_dirs, n * V * 12.0
        s = t["hip"]["us"] * 1e-6
        res = {"takes": takes, "frames": n, "vertices": V, "kc": m.n_dirs, "width": m.width, "call": t, "hip_us_per_take": round(t["hip"]["us"] / takes, 1),
               "torch_us_per_take": round(t["torch"]["us"] / takes, 1), "speedup_vs_torch": round(t["torch"]["us"] / t["hip"]["us"], 2),
               "hip_tflops_fp32": round(flops / s / 1e12, 2), "fraction_of_157tf_matrix_peak": round(flops / s / PEAK_FP32_MATRIX, 4),
               "hip_output_gb_per_s": round(out_bytes / s / 1e9, 1), "max_abs_hip_vs_torch": agree}
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
