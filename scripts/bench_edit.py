#!/usr/bin/env python3
"""In-painting timing (not the contract bench): one sampling loop with a lower-body keep mask, three ways, alternated in one process,
device-event time per loop.

    python scripts/bench_edit.py [--batches 1,8,64] [--rounds 5] [--loops ddpm,ddim]

    (a) fused+edit   the fused loop with y['inpainting_mask'] / y['inpainted_motion'] (`syn_denoise_step_edit`, graph replays)
    (b) fused        the fused loop without the two keys
    (c) generic+edit the per-step path the same edit took before the fused loop accepted it (Python between the steps, a model call and
                     torch ops per step), forced with denoised_fn = identity

Loops: DDPM-1000 (`p_sample_loop`, in-library noise) and DDIM-50 (`ddim_sample_loop`, eta 0).  Per (loop, batch): min..max over the rounds
of each variant and the ratios (a) / (b) and (c) / (a) of the medians; one JSON line per case.  (c) at DDPM-1000 is timed over --generic-steps
steps (default 100) of the 1000 and scaled: its steps cost the same at every timestep."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import longform, synth  # noqa: E402
from syntalker_amd.denoiser import MDM  # noqa: E402
from syntalker_amd.process import create_gaussian_diffusion  # noqa: E402


def time_variants(variants: dict, rounds: int) -> dict:
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in variants}
    for fn in variants.values():          # graphs captured, conditioning cached
        fn()
    for _ in range(rounds):
        for name, fn in variants.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--loops", default="ddpm,ddim")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--generic-steps", type=int, default=100)
    a = ap.parse_args()
    dev = "cuda"
    model = synth.synth_fill_(MDM(synth.default_args()).eval(), seed=0).to(dev)
    for kind in a.loops.split(","):
        d = create_gaussian_diffusion(use_ddim=kind == "ddim")
        steps = d.num_timesteps
        for B in (int(v) for v in a.batches.split(",")):
            shape = (B, 1536, 1, 32)
            y = synth.to_device(synth.synth_clip_inputs(B, seed=1), dev)
            x = synth.synth_latent(B, seed=1).to(dev)
            mask = longform.keep_mask(32, ("lower",)).T.reshape(1, 1536, 1, 32).expand(shape).contiguous().to(dev)
            ye = dict(y, inpainting_mask=mask, inpainted_motion=synth.synth_latent(B, seed=2, name="known").to(dev))
            loop = d.ddim_sample_loop if kind == "ddim" else d.p_sample_loop
            g_steps = min(steps, a.generic_steps)
            paths = {}

            def run(name, yy, **kw):
                def fn():
                    out = loop(model, shape, noise=x, clip_denoised=False, model_kwargs={"y": yy}, seed=3, **kw)
                    paths[name] = d.last_path
                    return out
                return fn
            t = time_variants({"fused+edit": run("fused+edit", ye), "fused": run("fused", y),
                               "generic+edit": run("generic+edit", ye, denoised_fn=lambda v: v, skip_timesteps=steps - g_steps)}, a.rounds)
            t["generic+edit"] = [v * steps / g_steps for v in t["generic+edit"]]
            assert paths == {"fused+edit": "fused", "fused": "fused", "generic+edit": "generic"}, paths
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({"loop": f"{kind}-{steps}", "clips": B,
                              **{f"{k}_ms": [round(min(v), 2), round(max(v), 2)] for k, v in t.items()},
                              "edit_over_plain": round(med["fused+edit"] / med["fused"], 4),
                              "generic_over_fused_edit": round(med["generic+edit"] / med["fused+edit"], 2),
                              "generic_steps_timed": g_steps}), flush=True)


if __name__ == "__main__":
    main()
