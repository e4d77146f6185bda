#!/usr/bin/env python3
"""calc_bpd_loop on the device against the sampling loops that make the same number of model evaluations, one process: wall time of a
whole call with a device synchronise, after warm-up, median of the rounds and their spread.

    python scripts/bench_bpd.py [--clips 1,40] [--rounds 5] [--generic-clips 1] [--out profiles/bpd_bench.txt]

Per clip count and process (ddim50, the 1000-step one): the fused `calc_bpd_loop` (seeded draws), `ddim_sample_loop` / `p_sample_loop` over
the same clips (T model evaluations per clip as well), and the generic path of `calc_bpd_loop` (one model call per timestep; ddim50 only -
it is forced by clip_denoised=True, which adds one clamp).  Then the parts of one chunk of the fused path at 1024 sequences, each timed on its
own with device events: noise draws, q_sample, the two layout imports, the model evaluation, `syn_bpd_terms`.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import _lib, engine, synth                        # noqa: E402
from syntalker_amd.denoiser import MDM                               # noqa: E402
from syntalker_amd.process import create_gaussian_diffusion         # noqa: E402


def wall(fn, rounds):
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def events(fn, rounds=5):
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="1,40")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--generic-clips", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    model = synth.synth_fill_(MDM(synth.default_args()).eval(), seed=0).to(dev)
    procs = {"ddim50": create_gaussian_diffusion(use_ddim=True), "ddpm1000": create_gaussian_diffusion()}
    lines = [f"{torch.cuda.get_device_name(0)}; ms per call, wall time with a device synchronise, median (min .. max) of {a.rounds} rounds after 2 warm-up calls"]

    def inputs(B):
        y4 = synth.synth_clip_inputs(min(B, 4), seed=1)
        rep = -(-B // min(B, 4))
        y = synth.to_device({k: (v.repeat(rep, *([1] * (v.dim() - 1)))[:B] if torch.is_tensor(v) else v) for k, v in y4.items()}, dev)
        return torch.randn(B, 1536, 1, 32, device=dev), y

    for B in (int(v) for v in a.clips.split(",")):
        x, y = inputs(B)
        for name, d in procs.items():
            T = d.num_timesteps
            loop = d.ddim_sample_loop if name == "ddim50" else d.p_sample_loop
            runs = {"calc_bpd_loop fused": lambda: d.calc_bpd_loop(model, x, clip_denoised=False, model_kwargs={"y": y}, seed=3),
                    f"{loop.__name__} fused": lambda: loop(model, x.shape, noise=x, clip_denoised=False, model_kwargs={"y": y}, seed=3)}
            if name == "ddim50" and B <= a.generic_clips:
                runs["calc_bpd_loop generic"] = lambda: d.calc_bpd_loop(model, x, clip_denoised=True, model_kwargs={"y": y}, seed=3)
            base = None
            for k, fn in runs.items():
                fn(); fn()
                med, lo, hi = wall(fn, a.rounds)
                base = base or med
                lines.append(f"{B:3d} clips {name:9s} {k:24s} {med:10.3f} ({lo:.3f} .. {hi:.3f}) ms   {med / (B * T) * 1e3:8.2f} us per model evaluation"
                             f"   x{med / base:.2f} of the fused calc_bpd_loop")
    # the parts of one chunk: 1024 (clip, timestep) pairs of 40 clips on the 1000-step process
    d, n, B = procs["ddpm1000"], 1024, 40
    x, y = inputs(B)
    pairs = torch.arange(n, device=dev)
    clips, steps = pairs % B, 999 - pairs // B
    hc, hs = clips.tolist(), steps.tolist()
    noise = engine.seeded_noise(3, 0, hc, hs, dev)
    x_t = d.q_sample(x[clips], steps, noise)
    sb = model.step_buffers(n, 1, want_x0=True)
    pm = model.packed()
    _, tmap = d._model_timesteps(dev)
    batch = engine.BpdBatch(model, d.q_sample, engine.bpd_rows(d.tables()), lambda t: tmap[t], x, model.variant_conds(y, [(False, False, None)]), None)
    out = torch.empty(3, n, device=dev)
    batch.run(clips, steps, noise, out)
    x0l = batch._x_start_as(sb)
    t32, c32 = steps.to(torch.int32), clips.to(torch.int32)
    lib = _lib.load()

    def terms():
        _lib.check(lib.syn_bpd_terms(batch.rows.data_ptr(), batch.n_rows, t32.data_ptr(), c32.data_ptr(), x0l.data_ptr(), B, sb.x.data_ptr(),
                                     sb.noise.data_ptr(), sb.x0.data_ptr(), n, out.data_ptr(), _lib.current_stream(dev)), "syn_bpd_terms")

    def evaluate():
        c = sb.c
        saved = (c.x_next, c.pred_x0)
        try:
            c.x_next, c.pred_x0 = sb.x0.data_ptr(), None
            engine.run_step(pm, sb, batch.ident, use_noise=False)
        finally:
            c.x_next, c.pred_x0 = saved
    parts = {"noise draws (seeded_noise)": lambda: engine.seeded_noise(3, 0, hc, hs, dev),
             "gather x_start + q_sample": lambda: d.q_sample(x[clips], steps, noise),
             "layout import of x_t (+ bf16 copy)": lambda: sb.load_x(x_t),
             "layout import of the noise": lambda: sb.load_noise(noise),
             "model evaluation (run_step)": evaluate,
             "syn_bpd_terms": terms,
             "whole chunk (BpdBatch.run)": lambda: batch.run(clips, steps, noise, out)}
    lines.append(f"parts of one chunk of {n} sequences ({'fragment order' if sb.fragment else 'token-major'}), device events, median of 5:")
    for k, fn in parts.items():
        fn()
        ms = events(fn)
        extra = f"   {4 * 196608 * n / ms / 1e6:8.1f} GB/s of the 4 x 196 608 B per sequence it must read" if k == "syn_bpd_terms" else ""
        lines.append(f"    {k:36s} {ms:9.4f} ms{extra}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
