#!/usr/bin/env python3
"""The guided sampling step (`guided.sample_loop`, cond_fn_with_grad=True with the keyframe objective) beside the unguided fused step: ms per
step under DDIM and under DDPM at 1 / 8 / 64 clips, and the split of one guided step into the node's forward, its backward (with cond_fn's own
autograd work, which runs inside the same `autograd.grad` call), the rest of cond_fn and the update kernel.  One process; device events around
whole loop calls (the loops alternate inside every round) and around the pieces of single steps; min .. max over the rounds.

    python scripts/bench_guided.py [--clips 1,8,64] [--rounds 5] [--steps 20] [--out profiles/guided_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import guided, longform, synth                   # noqa: E402
from syntalker_amd.denoiser import MDM                               # noqa: E402
from syntalker_amd.process import create_gaussian_diffusion         # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="1,8,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    model = synth.synth_fill_(MDM(synth.default_args()).eval(), seed=0).to(dev)
    keep = longform.keep_mask(32, ("lower",), (8, 20)).t().reshape(1, 1536, 1, 32).to(dev)
    n = a.steps
    lines = [f"{torch.cuda.get_device_name(0)}; ms per step, min .. max of {a.rounds} rounds of {n}-step loop calls (loops alternate inside a round); "
             "guided = cond_fn_with_grad with guided.keyframe_cond_fn"]
    for B in (int(v) for v in a.clips.split(",")):
        y4 = synth.synth_clip_inputs(min(B, 4), seed=1)
        rep = -(-B // min(B, 4))
        y = synth.to_device({k: (v.repeat(rep, *([1] * (v.dim() - 1)))[:B] if torch.is_tensor(v) else v) for k, v in y4.items()}, dev)
        x = torch.randn(B, 1536, 1, 32, device=dev)
        target = torch.randn(B, 1536, 1, 32, device=dev)
        fn = guided.keyframe_cond_fn(target, keep, 0.05, True)
        loops = {}
        for tag, d, skip in (("ddim", create_gaussian_diffusion(use_ddim=True), 50 - n), ("ddpm", create_gaussian_diffusion(), 1000 - n)):
            kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip, seed=1)
            loop = d.ddim_sample_loop if tag == "ddim" else d.p_sample_loop
            loops[f"{tag} guided"] = (lambda loop=loop, kw=kw: loop(model, x.shape, cond_fn=fn, cond_fn_with_grad=True, **kw))
            loops[f"{tag} unguided (fused)"] = (lambda loop=loop, kw=kw: loop(model, x.shape, **kw))
        for f in loops.values():                                    # graphs captured, packs built, conditioning cached
            f(); f()
        ms = {k: [] for k in loops}
        for _ in range(a.rounds):
            for k, f in loops.items():
                ms[k].append(timed(f)[0] / n)
        for k, v in ms.items():
            lines.append(f"{B:3d} clips  {k:22s} {min(v):8.3f} .. {max(v):8.3f} ms per step")
        # the pieces of one guided step (t = 500), each between its own pair of events
        with torch.no_grad():
            conds = model.variant_conds(y, [model.own_variant(y)])
        d = create_gaussian_diffusion(use_ddim=True)
        coef = guided.update_coefs(d.tables(), "ddim", 0.0, dev)
        t32 = torch.full((B,), 25, device=dev, dtype=torch.int32)
        tm = torch.full((B,), 500, device=dev)
        parts = {"forward (DenoiseFn)": [], "objective": [], "backward (autograd.grad)": [], "update (syn_guide_update)": []}
        for r in range(a.rounds + 1):
            xr = x.clone().requires_grad_()
            f_ms, x0 = timed(lambda: guided.denoise(model, xr, tm, conds))
            o_ms, logp = timed(lambda: -0.05 * (keep.float() * (x0 - target) ** 2).sum())
            b_ms, g = timed(lambda: torch.autograd.grad(logp, xr)[0])
            u_ms, _ = timed(lambda: guided.guide_update("ddim", x, x0.detach(), g, coef, t32))
            if r:                                                   # (round 0 warms up)
                for k, v in zip(parts, (f_ms, o_ms, b_ms, u_ms)):
                    parts[k].append(v)
        lines.append(f"{B:3d} clips  one guided step, piece by piece: " + "; ".join(f"{k} {min(v):.3f} .. {max(v):.3f}" for k, v in parts.items()) + " ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
