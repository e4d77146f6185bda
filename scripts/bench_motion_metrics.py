#!/usr/bin/env python3
"""Motion-metric timing (not the contract bench): SMPL-X joints -> speeds -> beats -> beat consistency, plus the L1 diversity, for one take of
60 s (1800 frames at 30 fps) and for 64 of them, three ways:

  hip    the kernels of csrc/syn_joints.inc through syntalker_amd.joints / metrics (one batched call per stage, each take its own L1 mean as test() has it)
  torch  the same arithmetic in torch fp32 ops on the same GPU (batched Rodrigues, 55 matmul steps down the tree, sliced differences, shifted
         comparisons, a broadcast |beat - onset| minimum)
  numpy  a RESTATEMENT on the machine's host cores, not the reference's own code: tests/motion_metrics_ref.py - utils/metric.py restated with its
         inner loops vectorised (the reference's own Python loops are slower), and the fp32 FK chain standing in for smplx

hip and torch alternate in one process, device-event time per call, median and min..max over the rounds; numpy is wall time, once.  Also: the FK
kernel alone against the HBM roofline (12 B in and 12 B out per joint and frame at 8 TB/s).

    python scripts/bench_motion_metrics.py [--reps 10] [--rounds 5] [--out profiles/motion_metrics_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import joints, metrics  # noqa: E402
from tests import motion_metrics_ref as mr  # noqa: E402

FRAMES, FPS, MASK, ORDER, SIGMA, ONSETS = 1800, 30, 60, 7, 0.3, 120
HBM_BYTES_PER_S = 8e12


def torch_fk(parents, rest, aa):
    """rest (S, J, 3), aa (S, n, J, 3) -> (S, n, J, 3)."""
    t = aa.norm(dim=-1)
    small = t < 1e-4
    ts = torch.where(small, torch.ones_like(t), t)
    sh = torch.sin(0.5 * ts)
    a = torch.where(small, 1 - t * t / 6, torch.sin(ts) / ts)[..., None, None]
    b = torch.where(small, 0.5 - t * t / 24, 2 * sh * sh / (ts * ts))[..., None, None]
    x, y, z = aa.unbind(-1)
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(aa.shape[:-1] + (3, 3))
    R = torch.eye(3, device=aa.device) + a * K + b * (K @ K)
    GR, Gt = [None] * len(parents), [None] * len(parents)
    for j, p in enumerate(parents):
        if p < 0:
            GR[j], Gt[j] = R[:, :, j], rest[:, None, j].expand(-1, aa.shape[1], -1)
        else:
            GR[j] = GR[p] @ R[:, :, j]
            Gt[j] = (GR[p] @ (rest[:, None, j] - rest[:, None, p])[..., None])[..., 0] + Gt[p]
    return torch.stack(Gt, 2)


def torch_speed(x, fps, mmae):
    d = torch.cat([x[:, 1:2] - x[:, :1], (x[:, 2:] - x[:, :-2]) / 2, x[:, -1:] - x[:, -2:-1]], 1) * fps
    return d.norm(dim=-1) / mmae


def torch_beats(vel, ts, te, order, thr=0.3):
    s = vel[:, ts:te]
    m = s.shape[1]
    idx = torch.arange(m, device=vel.device)
    ok = vel[:, :m] > thr
    for k in range(1, order + 1):
        ok = ok & (s < s[:, (idx + k).clamp(max=m - 1)]) & (s < s[:, (idx - k).clamp(min=0)])
    return ok


def torch_align(mask, upper, onsets, fps, sigma):
    """mask (S, m, J) bool, onsets (S, M) -> (S,)."""
    m = mask.shape[1]
    t = torch.where(mask[:, :, upper], (torch.arange(m, device=mask.device) / fps)[None, :, None], torch.full((), float("inf"), device=mask.device))
    d = (t[:, None] - onsets[:, :, None, None].float()).abs().amin(2)
    return torch.exp(-(d * d) / (2 * sigma * sigma)).mean(1).mean(1)


def torch_l1(x):
    x = x.double()
    return (x - x.mean(1, keepdim=True)).abs().sum((1, 2))


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_metrics_bench.txt"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    dev = "cuda"
    parents = mr.smplx_parents()
    lines = [f"# scripts/bench_motion_metrics.py --reps {a.reps} --rounds {a.rounds}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# a take = {FRAMES} frames at {FPS} fps, 55 joints, {ONSETS} onsets, mask {MASK}, order {ORDER}, sigma {SIGMA}; times in us per call "
             "(median [min, max] over the rounds)"]
    for takes in (1, 64):
        rest_np = np.stack([mr.synth_rest(s) for s in range(takes)])
        aa_np = np.stack([mr.smooth_rotations(100 + s, FRAMES) for s in range(takes)])
        onsets_np = np.sort(np.random.RandomState(9).uniform(0, (FRAMES - 2 * MASK) / FPS, (takes, ONSETS)), 1)
        skel = joints.Skeleton(parents, rest_np)
        rest, aa, onsets = torch.from_numpy(rest_np).to(dev), torch.from_numpy(aa_np).to(dev), torch.from_numpy(onsets_np).to(dev)
        j0 = joints.forward_kinematics(skel, aa.reshape(-1, 55, 3)).reshape(takes, FRAMES, 55, 3)
        mmae_t = (joints.mean_joint_speed(j0, FPS) * 2.2).clamp_min(1e-6)      # (the root does not move without transl)
        mmae_np = mmae_t.cpu().numpy()
        onset_list = [o for o in onsets_np]

        def hip():
            j = joints.forward_kinematics(skel, aa.reshape(-1, 55, 3)).reshape(takes, FRAMES, 55, 3)
            vel = joints.joint_speed(j, FPS, mmae_t)
            mask = metrics.motion_beat_mask(vel, MASK, FRAMES - MASK, ORDER)
            bc = metrics.beat_align(mask, onset_list, metrics.UPPER_BODY, FPS, SIGMA)[1]
            l1 = metrics.l1_sum(j.reshape(takes, FRAMES, 165))
            return bc, l1

        def torch_path():
            j = torch_fk(parents, rest, aa)
            vel = torch_speed(j, FPS, mmae_t)
            mask = torch_beats(vel, MASK, FRAMES - MASK, ORDER)
            bc = torch_align(mask, list(metrics.UPPER_BODY), onsets, FPS, SIGMA).cpu().numpy()
            l1 = torch_l1(j.reshape(takes, FRAMES, 165)).cpu().numpy()
            return bc, l1

        def numpy_path():
            bcs, l1s = [], []
            for k in range(takes):
                j = mr.fk_oracle(parents, rest_np[k], aa_np[k], dtype=np.float32).reshape(FRAMES, 165)
                vel = mr.speeds_ref(j, FPS, mmae_np, dtype=np.float32)
                mask = mr.beats_ref(vel, MASK, FRAMES - MASK, ORDER)
                bcs.append(mr.bc_ref(mask, onsets_np[k], list(metrics.UPPER_BODY), FPS, SIGMA)[1])
                l1s.append(mr.l1_ref_f32(j))
            return np.asarray(bcs), np.asarray(l1s)

        (bc_h, l1_h), (bc_t, l1_t) = hip(), torch_path()
        t0 = time.perf_counter()
        bc_n, l1_n = numpy_path()
        numpy_us = (time.perf_counter() - t0) * 1e6
        agree = {"bc_hip_vs_torch": float(np.abs(np.asarray(bc_h) - bc_t).max()), "bc_hip_vs_numpy": float(np.abs(np.asarray(bc_h) - bc_n).max()),
                 "l1_rel_hip_vs_torch": float(np.abs(np.asarray(l1_h) / l1_t - 1).max()), "l1_rel_hip_vs_numpy": float(np.abs(np.asarray(l1_h) / l1_n - 1).max())}
        flat = aa.reshape(-1, 55, 3)
        t = timed({"hip": hip, "torch": torch_path}, a.reps, a.rounds)
        fk = timed({"hip_fk": lambda: joints.forward_kinematics(skel, flat), "torch_fk": lambda: torch_fk(parents, rest, aa)}, a.reps * 5, a.rounds)
        fk_bytes = takes * FRAMES * 55 * 24
        r = {"takes": takes, "frames": FRAMES, "pipeline": t, "speedup_vs_torch": round(t["torch"]["us"] / t["hip"]["us"], 2),
             "numpy_restatement_host_us": round(numpy_us, 1), "speedup_vs_numpy_restatement": round(numpy_us / t["hip"]["us"], 1), "fk_only": fk,
             "fk_bytes": fk_bytes, "fk_hbm_roofline_us": round(fk_bytes / HBM_BYTES_PER_S * 1e6, 2),
             "fk_roofline_fraction": round(fk_bytes / HBM_BYTES_PER_S * 1e6 / fk["hip_fk"]["us"], 4), "agreement": agree}
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
