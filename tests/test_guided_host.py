"""Gradient guidance, host side (no GPU): the reference's condition_* arithmetic against its recorded outputs (tests/golden/guided_outputs.npz,
tests/golden/make_guided_golden.py), the signatures, the single-step `_with_grad` samplers on a small differentiable torch module against a
hand-written autograd restatement, the ready-made keyframe objective, what the loops still refuse, and the slicing / padding plan of the node."""
import ast
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from syntalker_amd import guided, longform, process, synth
from tests.conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "guided_outputs.npz"))


def _surface_inputs():
    """make_golden.surface_inputs without importing the module (its import pulls the reference tree onto sys.path)."""
    src = open(os.path.join(GOLDEN, "make_golden.py")).read()
    keep = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "surface_inputs"]
    ns = {"torch": torch, "synth": synth}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "make_golden.py", "exec"), ns)
    return ns["surface_inputs"]()


def test_condition_methods_equal_the_reference(fx):
    """condition_mean / condition_score and their _with_grad forms on a fixed p_mean_var dict, full and ddim50-spaced process: the spaced process hands
    cond_fn the BASE process's timesteps in the two forms without grad (respace.py:99-103) and its own indices in the other two."""
    x, other, y = _surface_inputs()
    toy = lambda x, t, **kw: -0.3 * (x - 0.0004 * t.view(-1, 1, 1, 1).float()) + 0.01 * kw["y"]["seed"].mean(dim=(1, 2)).view(-1, 1, 1, 1)
    toy_g = lambda x, t, p, **kw: 0.2 * p["pred_xstart"] - 0.1 * x + 0.003 * t.view(-1, 1, 1, 1).float() * p["variance"]

    def close(a, name):
        return np.allclose(a.numpy(), fx[name], rtol=2e-6, atol=1e-6 * float(np.abs(fx[name]).max()))
    with torch.no_grad():
        for tag, ddim, t in (("ddpm", False, torch.tensor([0, 412, 999])), ("ddim", True, torch.tensor([0, 23, 49]))):
            d = process.create_gaussian_diffusion(use_ddim=ddim)
            mean, var, logvar = d.q_posterior_mean_variance(other, x, t)
            p = {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": other}
            kw = {"y": y}
            assert close(d.condition_mean(toy, dict(p), x, t, model_kwargs=kw), f"surf.{tag}.condition_mean"), tag
            assert close(d.condition_mean_with_grad(toy_g, dict(p), x, t, model_kwargs=kw), f"surf.{tag}.condition_mean_with_grad"), tag
            for name, fn in (("condition_score", toy), ("condition_score_with_grad", toy_g)):
                r = getattr(d, name)(fn, dict(p), x, t, model_kwargs=kw)
                assert close(r["pred_xstart"], f"surf.{tag}.{name}.pred_xstart") and close(r["mean"], f"surf.{tag}.{name}.mean"), (tag, name)
                assert r is not p and r["variance"] is p["variance"]          # a shallow copy with pred_xstart and mean replaced, like the reference's


def test_signatures_equal_the_reference_parameters_plus_keyword_only_extras(fx):
    want = {s.split("(", 1)[0]: s.split("(", 1)[1][:-1] for s in fx["signatures"]}
    assert len(want) == 6
    extras = {"p_sample_with_grad": ["noise"], "ddim_sample_with_grad": ["noise"]}
    for name, ref in want.items():
        ps = [p for p in inspect.signature(getattr(process.SpacedDiffusion, name)).parameters.values() if p.name != "self"]
        pos = [p for p in ps if p.kind is p.POSITIONAL_OR_KEYWORD]
        assert ",".join(p.name + ("" if p.default is p.empty else "=" + repr(p.default)) for p in pos) == ref, name
        assert [p.name for p in ps if p.kind is p.KEYWORD_ONLY] == extras.get(name, []) and len(ps) == len(pos) + len(extras.get(name, []))
    for name in ("p_sample", "ddim_sample"):
        assert "cond_fn" in inspect.signature(getattr(process.SpacedDiffusion, name)).parameters


class Toy(torch.nn.Module):
    """A small denoiser that is differentiable in x and depends on t."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(0.7))

    def forward(self, x, t, y=None):
        return self.w * torch.tanh(x) + 0.001 * t.view(-1, 1, 1, 1).float() * x.roll(1, dims=3)


@pytest.mark.parametrize("ddim", [False, True])
def test_single_step_with_grad_samplers_against_a_hand_written_restatement(ddim):
    """p_sample_with_grad / ddim_sample_with_grad (gaussian_diffusion.py:559-605, 793-848) and cond_fn on p_sample / ddim_sample, any model: against the
    formulas written out from the schedule tables in fp64-free plain torch."""
    d = process.create_gaussian_diffusion(use_ddim=ddim)
    g = torch.Generator().manual_seed(1)
    x, noise, target = (torch.randn(3, 8, 1, 4, generator=g) for _ in range(3))
    t = torch.tensor([0, 7, d.num_timesteps - 1])
    toy = Toy()
    tm = torch.tensor(d.timestep_map)[t]
    tab = lambda n: torch.from_numpy(getattr(d, n)).float()[t].view(-1, 1, 1, 1)
    cond = lambda x_, t_, p, **kw: torch.autograd.grad(-(0.4 * (p["pred_xstart"] - target) ** 2).sum(), x_)[0]
    xr = x.clone().requires_grad_()
    x0 = toy(xr, tm)
    grad = torch.autograd.grad(-(0.4 * (x0 - target) ** 2).sum(), xr)[0]
    x0 = x0.detach()
    nz = (t != 0).float().view(-1, 1, 1, 1)
    if not ddim:
        got = d.p_sample_with_grad(toy, x, t, clip_denoised=False, cond_fn=cond, model_kwargs={}, noise=noise)
        mean = tab("posterior_mean_coef1") * x0 + tab("posterior_mean_coef2") * x
        want = mean + tab("posterior_variance") * grad + nz * torch.exp(0.5 * tab("posterior_log_variance_clipped")) * noise
    else:
        got = d.ddim_sample_with_grad(toy, x, t, clip_denoised=False, cond_fn=cond, model_kwargs={}, eta=0.5, noise=noise)
        r, m, ab, abp = tab("sqrt_recip_alphas_cumprod"), tab("sqrt_recipm1_alphas_cumprod"), tab("alphas_cumprod"), tab("alphas_cumprod_prev")
        eps = (r * x - x0) / m - (1 - ab).sqrt() * grad
        x0g = r * x - m * eps
        eps = (r * x - x0g) / m
        sigma = 0.5 * torch.sqrt((1 - abp) / (1 - ab)) * torch.sqrt(1 - ab / abp)
        want = x0g * abp.sqrt() + torch.sqrt(1 - abp - sigma ** 2) * eps + nz * sigma * noise
    assert torch.allclose(got["sample"].detach(), want, rtol=1e-5, atol=1e-5)
    assert torch.allclose(got["pred_xstart"], x0, rtol=1e-6, atol=1e-6) and not got["pred_xstart"].requires_grad      # the UNGUIDED one (:557, :791, :848)
    # without grad: cond_fn(x, t) sees the base process's timestep
    seen = []
    plain = lambda x_, t_, **kw: (seen.append(t_.clone()), 0.1 * x_)[1]
    with torch.no_grad():
        step = d.ddim_sample if ddim else d.p_sample
        out = step(toy, x, t, clip_denoised=False, cond_fn=plain, model_kwargs={}, noise=noise)
        base = step(toy, x, t, clip_denoised=False, model_kwargs={}, noise=noise)
    assert torch.equal(seen[0], tm) and not torch.allclose(out["sample"], base["sample"]) and torch.equal(out["pred_xstart"], base["pred_xstart"])


def test_keyframe_closed_form_equals_autograd_of_its_objective():
    d = process.create_gaussian_diffusion()
    g = torch.Generator().manual_seed(2)
    x, target = torch.randn(2, 1536, 1, 32, generator=g), torch.randn(2, 1536, 1, 32, generator=g)
    keep = longform.keep_mask(32, ("lower",), (8, 20)).t().reshape(1, 1536, 1, 32)
    assert int(keep.sum()) == 512 * 32 + 1024 * 12
    t = torch.tensor([3, 700])
    closed = guided.keyframe_cond_fn(target, keep, 1.5, with_grad=False)(x, t, y={})
    xr = x.clone().requires_grad_()
    root = torch.from_numpy(np.sqrt(d.alphas_cumprod)).float()[t].view(-1, 1, 1, 1)
    want = torch.autograd.grad((-1.5 * keep.float() * (xr - root * target) ** 2).sum(), xr)[0]
    assert torch.allclose(closed, want, rtol=1e-6, atol=1e-6) and bool((closed[~keep.expand_as(closed)] == 0).all())
    # with grad: the gradient through pred_xstart = f(x)
    xr = x.clone().requires_grad_()
    x0 = torch.tanh(xr) * 2
    got = guided.keyframe_cond_fn(target, keep, 1.5, with_grad=True)(xr, t, {"pred_xstart": x0}, y={})
    want = -2 * 1.5 * keep.float() * (x0.detach() - target) * 2 * (1 - torch.tanh(x) ** 2)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


def test_loops_with_a_generic_model_still_refuse_cond_fn():
    toy = Toy()
    fn = lambda *a, **k: 0
    for d, names in ((process.create_gaussian_diffusion(), ("p_sample_loop",)), (process.create_gaussian_diffusion(use_ddim=True), ("ddim_sample_loop",))):
        for name in names:
            for kw in ({"cond_fn": fn}, {"cond_fn": fn, "cond_fn_with_grad": True}, {"cond_fn_with_grad": True}, {"randomize_class": True}):
                with pytest.raises(NotImplementedError):
                    getattr(d, name)(toy, (1, 8, 1, 4), device="cpu", skip_timesteps=d.num_timesteps - 1, **kw)
                with pytest.raises(NotImplementedError):
                    next(getattr(d, name + "_progressive")(toy, (1, 8, 1, 4), device="cpu", skip_timesteps=d.num_timesteps - 1, **kw))
    # a HIP MDM that is not on the GPU (or in train mode) is no guided model either
    from syntalker_amd.denoiser import MDM
    m = MDM(synth.default_args()).eval()
    d = process.create_gaussian_diffusion(use_ddim=True)
    with pytest.raises(NotImplementedError):
        d.ddim_sample_loop(m, (1, 1536, 1, 32), cond_fn=fn, model_kwargs={"y": {}}, device="cpu")
    with pytest.raises(NotImplementedError):
        d.plms_sample_loop(m, (1, 1536, 1, 32), cond_fn=fn, model_kwargs={"y": {}}, device="cpu")


def test_slicing_and_padding_plan():
    """4 | n_seq <= 64 per launch of the persistent block kernels: other counts pad with zero sequences, more run as consecutive slices."""
    assert guided.plan(1) == [(0, 1, 1, 4)]
    assert guided.plan(5) == [(0, 5, 5, 8)]
    assert guided.plan(6) == [(0, 6, 6, 8)]
    assert guided.plan(64) == [(0, 64, 64, 64)]
    assert guided.plan(68) == [(0, 64, 64, 64), (64, 68, 4, 4)]
    assert guided.plan(3, 2) == [(0, 3, 6, 8)]                                    # a clip's variants stay in one launch
    assert guided.plan(40, 3) == [(0, 21, 63, 64), (21, 40, 57, 60)]
    for n, v in ((1, 1), (7, 9), (200, 2), (65, 1)):
        sl = guided.plan(n, v)
        assert sl[0][0] == 0 and sl[-1][1] == n and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(live == (hi - lo) * v and live <= pad <= 64 and pad % 4 == 0 and pad - live < 4 for lo, hi, live, pad in sl)
    for bad in ((0, 1), (4, 0), (4, 65)):
        with pytest.raises(ValueError):
            guided.plan(*bad)


def test_new_entry_points_are_declared_bound_and_refuse_null_arguments():
    import ctypes
    import re
    from syntalker_amd import _lib
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    for name, n_args in (("syn_guide_in_fwd", 13), ("syn_guide_in_bwd", 8), ("syn_guide_update", 14)):
        assert re.search(rf"^int\s+{name}\s*\(", header, flags=re.M) and name in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} missing: run __graft_entry__.build()")
    lib = _lib.load()
    assert len(lib.syn_guide_in_fwd.argtypes) == 13 and len(lib.syn_guide_in_bwd.argtypes) == 8 and len(lib.syn_guide_update.argtypes) == 14
    # host-side validation only: nothing is launched for a NULL pointer or an empty batch (no GPU needed)
    assert lib.syn_guide_in_fwd(None, 1, None, None, None, 1, None, None, None, 1, 4, None, None) != 0 and b"syn_guide_in_fwd" in lib.syn_last_error()
    assert lib.syn_guide_in_bwd(None, None, None, None, 4, 0, None, None) != 0 and b"syn_guide_in_bwd" in lib.syn_last_error()
    assert lib.syn_guide_update(0, None, None, None, None, 0, 0, 0, None, 0, None, 0, None, None) != 0 and b"syn_guide_update" in lib.syn_last_error()
    assert lib.syn_version() == 9
