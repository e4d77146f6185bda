#!/usr/bin/env python3
"""PLMS against DDIM on the fused sampling loop, one process, the samplers alternating inside every round, device events around each
whole loop call (50 steps of the ddim50 respacing; PLMS makes 51 model calls).  Prints min .. max over the rounds.

    python scripts/bench_plms.py [--clips 1,64,1024] [--rounds 5] [--out profiles/plms_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import synth                                      # noqa: E402
from syntalker_amd.denoiser import MDM                               # noqa: E402
from syntalker_amd.process import create_gaussian_diffusion         # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="1,64,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    model = synth.synth_fill_(MDM(synth.default_args()).eval(), seed=0).to(dev)
    d = create_gaussian_diffusion(use_ddim=True)
    lines = [f"{torch.cuda.get_device_name(0)}; ms per 50-step loop call, min .. max of {a.rounds} rounds (samplers alternate inside a round)"]
    for B in (int(v) for v in a.clips.split(",")):
        y4 = synth.synth_clip_inputs(min(B, 4), seed=1)
        rep = -(-B // min(B, 4))
        y = synth.to_device({k: (v.repeat(rep, *([1] * (v.dim() - 1)))[:B] if torch.is_tensor(v) else v) for k, v in y4.items()}, dev)
        x = torch.randn(B, 1536, 1, 32, device=dev)
        kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y})
        loops = {"ddim50": lambda: d.ddim_sample_loop(model, x.shape, **kw),
                 "plms50 order 2": lambda: d.plms_sample_loop(model, x.shape, order=2, **kw),
                 "plms50 order 4": lambda: d.plms_sample_loop(model, x.shape, order=4, **kw)}
        for fn in loops.values():                                   # graphs captured, conditioning cached
            fn(); fn()
        ms = {k: [] for k in loops}
        for _ in range(a.rounds):
            for k, fn in loops.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        assert d.last_path == "fused"
        base = min(ms["ddim50"])
        for k, v in ms.items():
            lines.append(f"{B:5d} clips  {k:15s} {min(v):9.3f} .. {max(v):9.3f} ms   x{min(v) / base:.3f} of ddim50   "
                         f"{min(v) / (51 if k.startswith('plms') else 50):.4f} ms per model call")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
