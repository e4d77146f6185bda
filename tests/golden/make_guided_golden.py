#!/usr/bin/env python3
"""Generate tests/golden/guided_outputs*.npz by running the REFERENCE's gradient guidance (diffusion/gaussian_diffusion.py:427-503, 549-605,
765-848, respace.py:99-103) on CPU.

The reference is imported as in make_golden.py (same stubs, same seeded synthetic model and inputs); only its OUTPUTS are stored.
    python tests/golden/make_guided_golden.py

The model, the inputs, the guidance target, the keep mask and the per-step noise are the seeded `synth` tensors; nothing of them is stored: the
tests rebuild them from `synth` with the seeds listed in the fixture's `recipe`.

Contents (files under the 1 MiB a committed file may have: guided_outputs.npz the surface, the factors and the signatures; guided_outputs_dx.npz
the two model gradients; _loops / _plain the one-clip loops and their unguided twins, _loops2 / _plain2 the two-clip ones, _pins0 / _pins49 the step pins):
    surf.<tag>.*             condition_mean / condition_score and their _with_grad forms on a fixed p_mean_var dict and toy cond_fns, tag ddpm (full
                             process, t = 0, 412, 999) and ddim (ddim50 spacing, t = 0, 23, 49)
    dx.beatx, dx.h3d_cfg     autograd.grad(sum(u * model(x, t, y)), x) of the reference model in eval mode, 2 clips (h3d_cfg: under
                             ClassifierFreeSampleModel, scale 2.5)
    <case>.sample            ddim_grad / ddim_nograd (1 clip, DDIM-50), ddpm_grad / ddpm_nograd (p_sample_loop, skip_timesteps=990), ddim_grad_inpaint
                             (2 clips, the in-painting pair of loop_kwargs_outputs.npz), h3d_cfg_ddim_grad (2 clips under ClassifierFreeSampleModel)
    ddim_grad.step<k>.*      sample, pred_xstart and the cond_fn gradient at steps 0 and 49
    plain.<case>             the unguided twin of each loop on the same noise
    amp.<case>, amp.ddim50   as in make_plms_golden.py: rel-L2 between the reference's run and the same run with a relative perturbation of 5e-3 on
                             every model output
    scale.<case>, keep.*     the guidance scale of each case and the keep mask's recipe (body parts, frame range)
    signatures               name=default of the reference's six methods (GaussianDiffusion's own: SpacedDiffusion's two overrides take *args)

The cond_fns are the keyframe objective restated: with grad  -scale sum keep (pred_xstart - target)^2 differentiated with respect to x, without
the closed form -2 scale keep (x - sqrt(alpha_bar_t) target).
ddpm_grad: the reference's p_sample_loop cannot take cond_fn_with_grad=True - it passes const_noise to p_sample_with_grad, which has no such
parameter (:727-737 against :559-568, a TypeError) - so that case runs the reference's own p_sample_with_grad step by step, as its loop would.

Asserted here: rel-L2(guided, plain) >= 10 x gate(case), gate = 3e-2 max(1, amp.case / amp.ddim50): a zero or wrong-signed gradient cannot pass.
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
KEEP_PARTS, KEEP_FRAMES = ("lower",), (8, 20)
# chosen on the reference alone so that every guided run ends >= 10 gates away from its unguided twin while the sampler stays in its stable range
# (amp.case ~ amp.ddim50): with grad the objective acts through the model's Jacobian, the closed form acts on x directly, DDPM through the
# posterior variance of its last ten steps (1e-5 .. 1e-4)
SCALE = {"ddim_grad": 0.05, "ddim_nograd": 5.0, "ddpm_grad": 30.0, "ddpm_nograd": 5000.0, "ddim_grad_inpaint": 0.05, "h3d_cfg_ddim_grad": 0.05}


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


def keep_tensor():
    m = torch.zeros(1, 1536, 1, 32, dtype=torch.bool)
    for name in KEEP_PARTS:
        k = ("upper", "hands", "lower").index(name)
        m[:, 512 * k:512 * (k + 1)] = True
    m[..., KEEP_FRAMES[0]:KEEP_FRAMES[1]] = True
    return m


def keyframe(target, keep, scale, with_grad, root_ab):
    if with_grad:
        def cond_fn(x, t, p_mean_var, **kw):
            logp = -scale * (keep.float() * (p_mean_var["pred_xstart"] - target) ** 2).sum()
            return torch.autograd.grad(logp, x)[0]
        return cond_fn

    def cond_fn(x, t, **kw):
        return -2.0 * scale * keep.float() * (x - root_ab[t].view(-1, 1, 1, 1) * target)
    return cond_fn


class Tap:
    """Records what a cond_fn returned, call by call."""

    def __init__(self, fn):
        self.fn, self.grads = fn, []

    def __call__(self, *a, **k):
        g = self.fn(*a, **k)
        self.grads.append(g.detach().clone())
        return g


def surface(make_diff, out):
    x, other, y = mg.surface_inputs()
    toy = lambda x, t, **kw: -0.3 * (x - 0.0004 * t.view(-1, 1, 1, 1).float()) + 0.01 * kw["y"]["seed"].mean(dim=(1, 2)).view(-1, 1, 1, 1)
    toy_g = lambda x, t, p, **kw: 0.2 * p["pred_xstart"] - 0.1 * x + 0.003 * t.view(-1, 1, 1, 1).float() * p["variance"]
    with torch.no_grad():
        for tag, ddim, t in (("ddpm", False, torch.tensor([0, 412, 999])), ("ddim", True, torch.tensor([0, 23, 49]))):
            d = make_diff(use_ddim=ddim)
            mean, var, logvar = d.q_posterior_mean_variance(x_start=other, x_t=x, t=t)
            p = {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": other}
            kw = {"y": y}
            out[f"surf.{tag}.condition_mean"] = f32(d.condition_mean(toy, dict(p), x, t, model_kwargs=kw))
            out[f"surf.{tag}.condition_mean_with_grad"] = f32(d.condition_mean_with_grad(toy_g, dict(p), x, t, model_kwargs=kw))
            for name, fn in (("condition_score", toy), ("condition_score_with_grad", toy_g)):
                r = getattr(d, name)(fn, dict(p), x, t, model_kwargs=kw)
                out[f"surf.{tag}.{name}.pred_xstart"], out[f"surf.{tag}.{name}.mean"] = f32(r["pred_xstart"]), f32(r["mean"])


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    RefMDM, RefMDMH3D, make_diff, cfgmod, data_path = mg.import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    args = synth.default_args(data_path=data_path)
    model = synth.synth_fill_(RefMDM(args).eval(), seed=0)
    mh = synth.synth_fill_(RefMDMH3D(args).eval(), seed=0)
    cfg = cfgmod.ClassifierFreeSampleModel(mh)
    out = {}
    surface(make_diff, out)

    # ---- the model's gradient with respect to x --------------------------------------------------------------------------------
    y2, x2 = synth.synth_clip_inputs(2, seed=31), synth.synth_latent(2, seed=31)
    yh, xh = synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), synth.synth_latent(2, seed=7)
    u = synth.synth_latent(2, seed=83, name="guided.u")
    t2 = torch.tensor([500, 37])
    for name, m, x, y in (("beatx", model, x2, y2), ("h3d_cfg", cfg, xh, dict(yh, scale=torch.ones(1) * 2.5))):
        xr = x.clone().requires_grad_()
        o = m(xr, t2, y=y)
        out[f"dx.{name}"] = f32(torch.autograd.grad((u * o).sum(), xr)[0])

    # ---- loops -----------------------------------------------------------------------------------------------------------------------
    ddim, ddpm = make_diff(use_ddim=True), make_diff(use_ddim=False)
    root = {id(ddim): torch.from_numpy(np.sqrt(ddpm.alphas_cumprod)).float(),       # without grad the spaced process maps t to the base process
            id(ddpm): torch.from_numpy(np.sqrt(ddpm.alphas_cumprod)).float()}
    keep = keep_tensor()
    y1, xT = synth.synth_clip_inputs(1, seed=2), synth.synth_latent(1, seed=2)
    g = synth._gen("inpainting", 37)
    mask = torch.rand(2, 1536, 1, 32, generator=g) < 0.25
    motion = torch.randn(2, 1536, 1, 32, generator=g)
    target = synth.synth_latent(2, seed=91, name="guided.target")
    sn10 = synth.synth_step_noise(10, 1, seed=93)
    cases = {
        "ddim_grad": (ddim, model, xT, y1, True, {}),
        "ddim_nograd": (ddim, model, xT, y1, False, {}),
        "ddpm_grad": (ddpm, model, xT, y1, True, dict(skip_timesteps=990)),
        "ddpm_nograd": (ddpm, model, xT, y1, False, dict(skip_timesteps=990)),
        "ddim_grad_inpaint": (ddim, model, x2, dict(y2, inpainting_mask=mask, inpainted_motion=motion), True, {}),
        "h3d_cfg_ddim_grad": (ddim, cfg, xh, dict(yh, scale=torch.ones(1) * 2.5), True, {}),
    }

    def run(d, m, x, y, fn, with_grad, kw):
        """The reference's loop -> the list of its steps' dicts."""
        shape = (x.shape[0],) + SHAPE
        common = dict(noise=x.clone(), clip_denoised=False, model_kwargs={"y": y}, device="cpu")
        if d is ddim:
            return list(d.ddim_sample_loop_progressive(m, shape, cond_fn=fn, cond_fn_with_grad=with_grad and fn is not None, **common, **kw))
        with mg.InjectNoise([sn10[k] for k in range(10)]):
            if not (with_grad and fn is not None):
                return list(d.p_sample_loop_progressive(m, shape, cond_fn=fn, **common, **kw))
            img = d.q_sample(torch.zeros_like(x), torch.full((x.shape[0],), 9), x.clone())     # (:705-712, skip_timesteps=990 without an init_image)
            steps = []
            for i in range(9, -1, -1):
                with torch.no_grad():
                    steps.append(d.p_sample_with_grad(m, img, torch.tensor([i] * x.shape[0]), clip_denoised=False, cond_fn=fn, model_kwargs={"y": y}))
                img = steps[-1]["sample"]
            return steps

    with torch.no_grad():
        clean = ddim.ddim_sample_loop(model, (1,) + SHAPE, noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y1}, device="cpu")
        noisy = ddim.ddim_sample_loop(Perturbed(model, 999), (1,) + SHAPE, noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y1}, device="cpu")
    out["amp.ddim50"] = np.float64(rel(noisy, clean))
    short = []
    for k, (name, (d, m, x, y, with_grad, kw)) in enumerate(cases.items()):
        n = x.shape[0]
        fn = Tap(keyframe(target[:n], keep, SCALE[name], with_grad, root[id(d)]))
        steps = run(d, m, x, y, fn, with_grad, kw)
        guided = steps[-1]["sample"]
        plain = run(d, m, x, y, None, with_grad, kw)[-1]["sample"]
        fnp = keyframe(target[:n], keep, SCALE[name], with_grad, root[id(d)])
        noisy = run(d, Perturbed(m, 2000 + k), x, y, fnp, with_grad, kw)[-1]["sample"]
        out[f"{name}.sample"], out[f"plain.{name}"] = f32(guided), f32(plain)
        out[f"amp.{name}"], out[f"scale.{name}"] = np.float64(rel(noisy, guided)), np.float64(SCALE[name])
        if name == "ddim_grad":
            for s in (0, 49):
                out[f"ddim_grad.step{s}.sample"], out[f"ddim_grad.step{s}.pred_xstart"] = f32(steps[s]["sample"]), f32(steps[s]["pred_xstart"])
                out[f"ddim_grad.step{s}.grad"] = f32(fn.grads[s])
        gate = 3e-2 * max(1.0, float(out[f"amp.{name}"]) / float(out["amp.ddim50"]))
        moved = rel(guided, plain)
        print(f"{name:20s} moved {moved:.3f}  gate {gate:.4f}  amp {float(out[f'amp.{name}']):.4g}", flush=True)
        short += [(name, moved, gate)] if moved < 10 * gate else []
    assert not short, short
    out["keep.parts"], out["keep.frames"] = np.array(KEEP_PARTS), np.array(KEEP_FRAMES)
    out["recipe"] = np.array(["model synth_fill_ seed 0", "beatx 2 clips: synth_clip_inputs / synth_latent seed 31", "h3d: seed 7, style_dim 256, style_zero False",
                              "1 clip: seed 2", "u: synth_latent(2, 83, 'guided.u')", "target: synth_latent(2, 91, 'guided.target')",
                              "ddpm step noise: synth_step_noise(10, 1, 93)", "inpainting: synth._gen('inpainting', 37): rand < 0.25, randn", "dx timesteps 500, 37"])

    def sig(fn):
        ps = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
        return ",".join(p.name + ("" if p.default is p.empty else "=" + repr(p.default)) for p in ps)
    base = type(ddim).__mro__[1]
    out["signatures"] = np.array([f"{n}({sig(getattr(base, n))})" for n in ("condition_mean", "condition_mean_with_grad", "condition_score",
                                                                              "condition_score_with_grad", "p_sample_with_grad", "ddim_sample_with_grad")])
    files = {"_dx": lambda k: k.startswith("dx."),
             "_pins0": lambda k: k.startswith("ddim_grad.step0."),
             "_pins49": lambda k: k.startswith("ddim_grad.step49."),
             "_loops2": lambda k: k in ("ddim_grad_inpaint.sample", "h3d_cfg_ddim_grad.sample"),
             "_plain2": lambda k: k in ("plain.ddim_grad_inpaint", "plain.h3d_cfg_ddim_grad"),
             "_loops": lambda k: k.endswith(".sample"),
             "_plain": lambda k: k.startswith("plain.")}
    rest = dict(out)
    for tag, pick in files.items():
        np.savez_compressed(os.path.join(HERE, f"guided_outputs{tag}.npz"), **{k: rest.pop(k) for k in list(rest) if pick(k)})
    np.savez_compressed(os.path.join(HERE, "guided_outputs.npz"), **rest)
    for k, v in out.items():
        print(f"{k:40s} {tuple(v.shape)}" + (f" {float(np.abs(v).mean()):.5g}" if v.dtype.kind == "f" else f" {v}"))


if __name__ == "__main__":
    main()
