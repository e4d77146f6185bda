#!/usr/bin/env python3
"""Generate tests/golden/plms_outputs*.npz by running the REFERENCE's PLMS sampler (diffusion/gaussian_diffusion.py:1004-1199) on CPU.

The reference is imported as in make_golden.py (same stubs, same seeded synthetic model and inputs); only its OUTPUTS are stored.
    python tests/golden/make_plms_golden.py

Contents (four files, each under the 1 MiB a committed file may have: plms_outputs.npz holds the one-clip loops, the factors and the
signatures, plms_outputs_2clips.npz the two two-clip loops, plms_outputs_pins_sample.npz / _pins_pred_xstart.npz the step pins):
    <case>.sample            the loop's result, cases o2 / o3 / o4 (beatx, 1 clip, all 50 steps of the ddim50 respacing), o3_skip40
                             (skip_timesteps=40), o2_inpaint (2 clips, the in-painting pair of loop_kwargs_outputs.npz), h3d_cfg_o2 (the
                             text-prompt denoiser under ClassifierFreeSampleModel, 2 clips)
    o4.step<k>.sample / .pred_xstart   k = 0, 1, 2, 3, 49 of the order-4 run: the Euler start, each ramp-up order, the last step
    amp.<case>, amp.ddim50   rel-L2 between the reference's run and the same run with a seeded relative perturbation of 5e-3 on every
                             model output: how much the sampler itself amplifies a model-output error (the GPU tests scale their gate by it)
    signatures               name=default of the reference's three plms_* methods
"""
import importlib.util
import inspect
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
synth, f32 = mg.synth, mg.f32

REL = 5e-3
SHAPE = (1536, 1, 32)


class Perturbed(torch.nn.Module):
    """model output * (1 + REL * N(0,1)), the draws from a generator seeded per run."""

    def __init__(self, model, seed):
        super().__init__()
        self.model = model
        self.gen = torch.Generator().manual_seed(seed)

    def forward(self, x, t, **kw):
        out = self.model(x, t, **kw)
        return out * (1 + REL * torch.randn(out.shape, generator=self.gen))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    RefMDM, RefMDMH3D, make_diff, cfgmod, data_path = mg.import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    args = synth.default_args(data_path=data_path)
    model = synth.synth_fill_(RefMDM(args).eval(), seed=0)
    mh = synth.synth_fill_(RefMDMH3D(args).eval(), seed=0)
    diff = make_diff(use_ddim=True)
    out = {}

    y1, xT = synth.synth_clip_inputs(1, seed=2), synth.synth_latent(1, seed=2)
    y2, x2 = synth.synth_clip_inputs(2, seed=31), synth.synth_latent(2, seed=31)
    g = synth._gen("inpainting", 37)
    mask = torch.rand(2, 1536, 1, 32, generator=g) < 0.25
    motion = torch.randn(2, 1536, 1, 32, generator=g)
    yh, xh = synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), synth.synth_latent(2, seed=7)
    cases = {
        "o2": (model, xT, y1, dict(order=2)),
        "o3": (model, xT, y1, dict(order=3)),
        "o4": (model, xT, y1, dict(order=4)),
        "o3_skip40": (model, xT, y1, dict(order=3, skip_timesteps=40)),
        "o2_inpaint": (model, x2, dict(y2, inpainting_mask=mask, inpainted_motion=motion), dict(order=2)),
        "h3d_cfg_o2": (cfgmod.ClassifierFreeSampleModel(mh), xh, dict(yh, scale=torch.ones(1) * 2.5), dict(order=2)),
    }
    with torch.no_grad():
        for k, (name, (m, x, y, kw)) in enumerate(cases.items()):
            shape = (x.shape[0],) + SHAPE
            steps = list(diff.plms_sample_loop_progressive(m, shape, noise=x.clone(), clip_denoised=False, model_kwargs={"y": y}, device="cpu", **kw))
            clean = steps[-1]["sample"]
            out[f"{name}.sample"] = f32(clean)
            if name == "o4":
                for s in (0, 1, 2, 3, 49):
                    out[f"o4.step{s}.sample"], out[f"o4.step{s}.pred_xstart"] = f32(steps[s]["sample"]), f32(steps[s]["pred_xstart"])
            noisy = diff.plms_sample_loop(Perturbed(m, 1000 + k), shape, noise=x.clone(), clip_denoised=False, model_kwargs={"y": y}, device="cpu", **kw)
            out[f"amp.{name}"] = np.float64(rel(noisy, clean))
        clean = diff.ddim_sample_loop(model, (1,) + SHAPE, noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y1}, device="cpu")
        noisy = diff.ddim_sample_loop(Perturbed(model, 999), (1,) + SHAPE, noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y1}, device="cpu")
        out["amp.ddim50"] = np.float64(rel(noisy, clean))

    def sig(fn):
        ps = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
        return ",".join(p.name + ("" if p.default is p.empty else "=" + repr(p.default)) for p in ps)
    out["signatures"] = np.array([f"{n}({sig(getattr(type(diff), n))})" for n in ("plms_sample", "plms_sample_loop", "plms_sample_loop_progressive")])
    files = {"_2clips": lambda k: k in ("o2_inpaint.sample", "h3d_cfg_o2.sample"),
             "_pins_sample": lambda k: k.startswith("o4.step") and k.endswith(".sample"),
             "_pins_pred_xstart": lambda k: k.startswith("o4.step") and k.endswith(".pred_xstart")}
    rest = dict(out)
    for tag, pick in files.items():
        np.savez_compressed(os.path.join(HERE, f"plms_outputs{tag}.npz"), **{k: rest.pop(k) for k in list(rest) if pick(k)})
    np.savez_compressed(os.path.join(HERE, "plms_outputs.npz"), **rest)
    for k, v in out.items():
        print(f"{k:28s} {tuple(v.shape)}" + (f" {float(np.abs(v).mean()):.5g}" if v.dtype.kind == "f" else f" {v}"))


if __name__ == "__main__":
    main()
