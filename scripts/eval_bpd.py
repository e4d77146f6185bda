#!/usr/bin/env python3
"""Score a model on held-out clips: the per-timestep variational bound and the two MSE curves of the reference's
`GaussianDiffusion.calc_bpd_loop` (diffusion/gaussian_diffusion.py:1548-1603), all timesteps of all clips as batches on the device.

    python scripts/eval_bpd.py cfg.yaml [--random-init] [--ddim] [--clips N] [--inputs clips.npz] [--seed 1] [--every K] [--out bpd.npz]

--random-init   ignore the checkpoint paths of the YAML and use the name-keyed synthetic weights
--ddim          the 50-step ddim50 respacing instead of the 1000-step process
--inputs        clips.npz: x_start (N, 1536, 1, 32) latents of held-out takes and the conditioning of model_kwargs['y'] (audio, word, seed,
                mask, ...) as the trainer builds it; without it, N seeded synthetic clips
Prints t, and the mean over the clips of xstart_mse, mse and vb (every K-th timestep, t = 0 always), then prior_bpd and total_bpd;
--out keeps the full (N, T) arrays.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import config, synth                              # noqa: E402
from syntalker_amd.process import create_gaussian_diffusion         # noqa: E402

PATH_KEYS = ("test_ckpt", "vqvae_upper_path", "vqvae_hands_path", "vqvae_lower_path", "vqvae_lower_trans_path",
             "mean_trans_path", "std_trans_path", "tmr_base_path")


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--ddim", action="store_true")
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--inputs")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--every", type=int)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    args = config.load_args(a.config, **({k: None for k in PATH_KEYS} if a.random_init else {}))
    s = config.build_sampler(args)
    if a.random_init:
        synth.synth_fill_(s.model, 0)
    dev = next(s.model.parameters()).device
    if a.inputs:
        z = np.load(a.inputs)
        x = torch.from_numpy(z["x_start"]).float().to(dev)
        y = {k: torch.from_numpy(z[k]).to(dev) for k in z.files if k != "x_start"}
    else:
        h3d = config.is_h3d(args)
        x = synth.synth_latent(a.clips, seed=a.seed, name="x_start").to(dev)
        y = synth.to_device(synth.synth_clip_inputs(a.clips, seed=a.seed, **(dict(style_dim=256, style_zero=False) if h3d else {})), dev)
    d = create_gaussian_diffusion(use_ddim=a.ddim)
    t0 = time.perf_counter()
    res = d.calc_bpd_loop(s.model, x, clip_denoised=False, model_kwargs={"y": y}, seed=a.seed)
    res = {k: v.cpu().numpy() for k, v in res.items()}
    dt = time.perf_counter() - t0
    T = d.num_timesteps
    every = a.every or max(1, T // 25)
    print(f"{x.shape[0]} clips x {T} timesteps, path: {d.last_path}, {dt:.3f} s")
    print(f"{'t':>5s} {'xstart_mse':>12s} {'mse':>12s} {'vb [bits/dim]':>14s}")
    for t in sorted(set(range(T - 1, -1, -every)) | {0}, reverse=True):
        j = T - 1 - t
        print(f"{t:5d} {res['xstart_mse'][:, j].mean():12.5g} {res['mse'][:, j].mean():12.5g} {res['vb'][:, j].mean():14.5g}")
    print(f"prior_bpd {res['prior_bpd'].mean():.5g}   total_bpd {res['total_bpd'].mean():.6g} (mean over the clips)")
    if a.out:
        np.savez_compressed(a.out, **res)
    return {"path": d.last_path, "clips": int(x.shape[0]), "timesteps": T, "total_bpd": float(res["total_bpd"].mean()),
            "finite": bool(all(np.isfinite(v).all() for v in res.values()))}


if __name__ == "__main__":
    main()
