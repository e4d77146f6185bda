#!/usr/bin/env python3
"""Generate tests/golden/bpd_outputs*.npz by running the REFERENCE's calc_bpd_loop (diffusion/gaussian_diffusion.py:1201-1234, 1530-1603) on CPU.

The reference is imported as in make_golden.py (same stubs, same seeded synthetic models and inputs); only its OUTPUTS are stored.
    python tests/golden/make_bpd_golden.py

The loop's `th.randn_like` draws are replaced by the rows of `synth.synth_step_noise(T, B, seed=NOISE_SEED)` (row i = iteration i, i.e.
timestep T - 1 - i); the tests regenerate that noise from the seed, it is not stored.

Contents (bpd_outputs.npz; the two full-size pins in bpd_outputs_pins.npz - every committed file stays under 1 MiB):
    <case>.total_bpd / .prior_bpd (B,)  .vb / .xstart_mse / .mse (B, T)     calc_bpd_loop's dictionary; column j is t = T - 1 - j
    <case>.pred_norm / .err_norm (B, T)   ||pred_xstart|| and ||pred_xstart - x_start|| per clip and column, in fp64 (the GPU tests derive
                                          their bound on the scalars from these)
    beatx_ddim50.pred_xstart.t0 / .tlast  clip 0's pred_xstart at t = 0 and t = T - 1 (pins file)
    signatures                            name=default of _vb_terms_bpd, _prior_bpd, calc_bpd_loop
Cases: beatx_ddim50 (2 clips, clip_denoised=False), beatx_ddim50_clipped (the default clip_denoised=True), h3d_cfg_ddim50
(ClassifierFreeSampleModel over the text-prompt denoiser, scale 2.5), beatx_full (the 1000-step process), identity_ddim50 (a model that
returns x_t: the one case whose t = 0 term lies in the interior of the discretised likelihood), toy_ddim50_clipped (make_golden.ToyDenoiser,
clip_denoised=True: the clamp on a model a CPU test can run).
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

NOISE_SEED = 5


class Identity(torch.nn.Module):
    def forward(self, x, t, **kw):
        return x


def run(diff, model, x_start, y, clip_denoised):
    """calc_bpd_loop with the seeded draws; also every iteration's pred_xstart norms, and the first / last iteration's pred_xstart."""
    T, B = diff.num_timesteps, x_start.shape[0]
    noise = synth.synth_step_noise(T, B, seed=NOISE_SEED)
    preds = []
    inner = diff._vb_terms_bpd

    def recording(*a, **k):
        out = inner(*a, **k)
        preds.append(out["pred_xstart"].detach().clone())
        return out
    diff._vb_terms_bpd = recording
    try:
        with mg.InjectNoise(noise) as inj, torch.no_grad():
            res = diff.calc_bpd_loop(model, x_start, clip_denoised=clip_denoised, model_kwargs={"y": y})
            assert inj.k == T
    finally:
        del diff._vb_terms_bpd
    out = {k: f32(v) for k, v in res.items()}
    flat = lambda t: t.double().reshape(B, -1)
    out["pred_norm"] = np.stack([flat(p).norm(dim=1).numpy() for p in preds], 1)
    out["err_norm"] = np.stack([(flat(p) - flat(x_start)).norm(dim=1).numpy() for p in preds], 1)
    return out, preds


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    RefMDM, RefMDMH3D, make_diff, cfgmod, data_path = mg.import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    args = synth.default_args(data_path=data_path)
    model = synth.synth_fill_(RefMDM(args).eval(), seed=0)
    mh = synth.synth_fill_(RefMDMH3D(args).eval(), seed=0)
    ddim, full = make_diff(use_ddim=True), make_diff(use_ddim=False)

    y2, x2 = synth.synth_clip_inputs(2, seed=31), synth.synth_latent(2, seed=31)
    yh, xh = synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), synth.synth_latent(2, seed=7)
    cases = {
        "beatx_ddim50": (ddim, model, x2, y2, False),
        "beatx_ddim50_clipped": (ddim, model, x2, y2, True),
        "h3d_cfg_ddim50": (ddim, cfgmod.ClassifierFreeSampleModel(mh), xh, dict(yh, scale=torch.ones(1) * 2.5), False),
        "identity_ddim50": (ddim, Identity(), x2, {}, False),
        "toy_ddim50_clipped": (ddim, mg.ToyDenoiser(), x2, {"seed": y2["seed"]}, True),
        "beatx_full": (full, model, x2, y2, False),
    }
    out, pins = {}, {}
    for name, (diff, m, x, y, clip) in cases.items():
        res, preds = run(diff, m, x.clone(), y, clip)
        for k, v in res.items():
            out[f"{name}.{k}"] = v
        if name == "beatx_ddim50":
            pins[f"{name}.pred_xstart.tlast"], pins[f"{name}.pred_xstart.t0"] = f32(preds[0][0]), f32(preds[-1][0])

    def sig(fn):
        ps = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
        return ",".join(p.name + ("" if p.default is p.empty else "=" + repr(p.default)) for p in ps)
    out["signatures"] = np.array([f"{n}({sig(getattr(type(ddim), n))})" for n in ("_vb_terms_bpd", "_prior_bpd", "calc_bpd_loop")])
    np.savez_compressed(os.path.join(HERE, "bpd_outputs.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "bpd_outputs_pins.npz"), **pins)
    for k, v in {**out, **pins}.items():
        print(f"{k:40s} {tuple(v.shape)}" + (f" {float(np.abs(v).mean()):.6g}" if v.dtype.kind == "f" else f" {v}"))


if __name__ == "__main__":
    main()
