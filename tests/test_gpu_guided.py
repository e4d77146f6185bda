"""Gradient-guided sampling on the GPU (`syntalker_amd/guided.py`, csrc/syn_guide.inc): the three kernels alone against torch restatements, the
node that is differentiable in x_t against the fused forward and against the reference model's recorded gradients, and the guided loops against
the reference's recorded runs (tests/golden/guided_outputs*.npz, tests/golden/make_guided_golden.py).

Gates: forward 2e-2 and gradient 3e-2 (tests/test_gpu_parity.py), loops 3e-2 scaled per case by max(1, amp.case / amp.ddim50) as in
tests/test_gpu_sampler_plms.py.  Measured on an MI355X (DESIGN.md 19 has the table): input stage forward 1.4e-3, its gradient 2.4e-3, adjoint
defect <= 1.2e-5; update kernel 4e-8 .. 8e-8; node output against the fused step 3.3e-3 (beatx) / 4.6e-3 (h3d under guidance); dx against the
reference 6.3e-3 / 1.0e-2; loops 6.9e-3 .. 1.2e-2: every figure under half its gate."""
import gc
import os

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, conditioning, engine, guided, longform, synth
from tests.conftest import GOLDEN
from tests.conftest import rel_l2 as _rel_l2
from tests.refmodel import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (1536, 1, 32)
FWD_TOL, GRAD_TOL, LOOP_TOL = 2e-2, 3e-2, 3e-2


def rel_l2(a, b):
    """(device results against the fixtures' numpy arrays: compared on the host)"""
    return _rel_l2(torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu())


def _model(variant="beatx"):
    if variant == "h3d":
        from syntalker_amd.denoiser_h3d import MDM
    else:
        from syntalker_amd.denoiser import MDM
    m = MDM(synth.default_args()).eval()
    missing, unexpected = m.load_state_dict(synth_state_dict(variant), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def beatx():
    return _model("beatx")


@pytest.fixture(scope="module")
def h3d():
    return _model("h3d")


@pytest.fixture(scope="module")
def fx():
    out = {}
    for part in ("", "_dx", "_loops", "_plain", "_loops2", "_plain2", "_pins0", "_pins49"):
        out.update(np.load(os.path.join(GOLDEN, f"guided_outputs{part}.npz")))
    return out


def gate(fx, case):
    return LOOP_TOL * max(1.0, float(fx[f"amp.{case}"]) / float(fx["amp.ddim50"]))


# ---- the input-stage kernels alone ---------------------------------------------------------------------------------------------------------
def _rot(h, cs, sn, inverse=False):
    """models/denoiser.py:178-186 on rows (n, 32, 512) in fp64: the (j, j + 32) pairs of every 64-wide group; inverse: the transpose."""
    n = h.shape[0]
    g = h.view(n, 32, 8, 2, 32)
    u, w = g[..., 0, :], g[..., 1, :]
    c, s = cs.view(1, 32, 1, 32), (-sn if inverse else sn).view(1, 32, 1, 32)
    return torch.stack([u * c - w * s, w * c + u * s], dim=-2).reshape(n, 32, 512)


@pytest.fixture(scope="module")
def stage():
    """Random operands of the input stage, shared by its tests: A (512, 1536) at the folded weight's scale, a time table, rotary tables."""
    g = torch.Generator().manual_seed(5)
    A = torch.randn(512, 1536, generator=g) / 1536 ** 0.5
    te = torch.randn(16, 512, generator=g)
    cs, sn = conditioning.rotary_tables(1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64)), 32)
    to = lambda t: t.to(DEV).contiguous()
    return dict(A=A, te=te, cs=cs, sn=sn, A_p=engine.pack_weight(to(A)), At_p=engine.pack_weight(to(A.t().contiguous())), te_d=to(te), cs_d=to(cs), sn_d=to(sn))


def _in_fwd(s, x, cond, t_model, n_seq, n_x=None):
    live = cond.shape[0] // 32
    h0 = torch.full((n_seq * 32, 512), float("nan"), device=DEV)
    t32 = t_model.to(DEV, torch.int32)
    _lib.check(_lib.load().syn_guide_in_fwd(x.data_ptr(), n_x or x.shape[0], s["A_p"].data_ptr(), cond.data_ptr(), s["te_d"].data_ptr(), 16, t32.data_ptr(),
                                            s["cs_d"].data_ptr(), s["sn_d"].data_ptr(), live, n_seq, h0.data_ptr(), _lib.current_stream(DEV)), "syn_guide_in_fwd")
    return h0


def _in_bwd(s, dh, n, accumulate=False, dx=None):
    dx = torch.full((n,) + SHAPE, float("nan"), device=DEV) if dx is None else dx
    _lib.check(_lib.load().syn_guide_in_bwd(dh.data_ptr(), s["At_p"].data_ptr(), s["cs_d"].data_ptr(), s["sn_d"].data_ptr(), n, int(accumulate), dx.data_ptr(),
                                            _lib.current_stream(DEV)), "syn_guide_in_bwd")
    return dx


@pytest.mark.parametrize("B,n_seq", [(4, 4), (5, 8), (12, 12), (64, 64)])
def test_input_stage_kernels_against_fp64(stage, B, n_seq):
    """syn_guide_in_fwd / _bwd on B live sequences in a launch of n_seq: forward, gradient, the adjoint identity between them, zero padding rows."""
    s = stage
    g = torch.Generator().manual_seed(100 + B)
    x = torch.randn(B, *SHAPE, generator=g)
    cond = torch.randn(B * 32, 512, generator=g)
    t = torch.randint(0, 16, (B,), generator=g)
    h0 = _in_fwd(s, x.to(DEV), cond.to(DEV), t, n_seq).cpu()
    rows = x.double().squeeze(2).permute(0, 2, 1)
    want = _rot(rows @ s["A"].double().t() + cond.double().view(B, 32, 512) + s["te"].double()[t].view(B, 1, 512), s["cs"].double(), s["sn"].double())
    err_f = rel_l2(h0[:B * 32], want)
    assert bool((h0[B * 32:] == 0).all()), "padding sequences must be zero rows"
    dh = torch.randn(B * 32, 512, generator=g)
    dx = _in_bwd(s, dh.to(DEV), B).cpu()
    want_dx = (_rot(dh.double().view(B, 32, 512), s["cs"].double(), s["sn"].double(), inverse=True) @ s["A"].double()).permute(0, 2, 1).unsqueeze(2)
    err_b = rel_l2(dx, want_dx)
    # <fwd(x) - fwd(0), dh> = <x, bwd(dh)>: the two kernels are each other's transpose, up to the bf16 rounding of x on one side and of dh on the other
    h00 = _in_fwd(s, torch.zeros_like(x).to(DEV), cond.to(DEV), t, n_seq).cpu()
    lin = (h0 - h00)[:B * 32].double()
    lhs, rhs = float((lin * dh.double()).sum()), float((x.double() * dx.double()).sum())
    adj = abs(lhs - rhs) / float(lin.norm() * dh.double().norm())
    print(f"input stage B={B} n_seq={n_seq}: forward rel-L2 {err_f:.3e}, gradient rel-L2 {err_b:.3e}, adjoint defect {adj:.3e}")
    assert err_f < FWD_TOL and err_b < GRAD_TOL and adj < GRAD_TOL, (err_f, err_b, adj)


def test_input_stage_variants_share_a_latent_and_accumulate_sums(stage):
    """n_x < n_live: sequence s reads clip s % n_x.  accumulate: a second call adds to dx what a first call alone would have written."""
    s = stage
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, *SHAPE, generator=g).to(DEV)
    cond = torch.randn(6 * 32, 512, generator=g).to(DEV)
    t = torch.tensor([3, 1, 4, 1, 5, 9])
    two = _in_fwd(s, x, cond, t, 8, n_x=3)
    twice = _in_fwd(s, torch.cat([x, x]), cond, t, 8)
    assert torch.equal(two, twice) and bool((two[6 * 32:] == 0).all())
    dh1, dh2 = (torch.randn(3 * 32, 512, generator=g).to(DEV) for _ in range(2))
    a, b = _in_bwd(s, dh1, 3), _in_bwd(s, dh2, 3)
    acc = _in_bwd(s, dh2, 3, accumulate=True, dx=a.clone())
    assert torch.equal(acc, a + b)


def test_input_stage_launchers_refuse_bad_arguments(stage):
    lib, s = _lib.load(), stage
    x, cond, h0, t = torch.zeros(4, *SHAPE, device=DEV), torch.zeros(128, 512, device=DEV), torch.zeros(128, 512, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    ok = [x.data_ptr(), 4, s["A_p"].data_ptr(), cond.data_ptr(), s["te_d"].data_ptr(), 16, t.data_ptr(), s["cs_d"].data_ptr(), s["sn_d"].data_ptr(), 4, 4, h0.data_ptr(), None]
    for i, bad in ((0, None), (1, 0), (1, 5), (5, 0), (9, 0), (9, 5), (10, 0), (11, None)):
        a = list(ok)
        a[i] = bad
        assert lib.syn_guide_in_fwd(*a) != 0 and b"syn_guide_in_fwd" in lib.syn_last_error(), (i, bad)
    assert lib.syn_guide_in_bwd(None, s["At_p"].data_ptr(), s["cs_d"].data_ptr(), s["sn_d"].data_ptr(), 4, 0, x.data_ptr(), None) != 0
    assert lib.syn_guide_in_bwd(h0.data_ptr(), s["At_p"].data_ptr(), s["cs_d"].data_ptr(), s["sn_d"].data_ptr(), 0, 0, x.data_ptr(), None) != 0
    assert lib.syn_guide_update(2, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 0, 0, 0, cond.data_ptr(), 4, t.data_ptr(), 4, x.data_ptr(), None) != 0
    assert lib.syn_guide_update(1, x.data_ptr(), None, x.data_ptr(), None, 0, 0, 0, cond.data_ptr(), 4, t.data_ptr(), 4, x.data_ptr(), None) != 0
    assert lib.syn_guide_update(0, x.data_ptr(), None, x.data_ptr(), None, 0, 0, 0, cond.data_ptr(), 4, t.data_ptr(), 0, x.data_ptr(), None) != 0


# ---- the update kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.7)])
def test_update_kernel_against_the_torch_restatement(kind, eta):
    """Both modes against the generic path's arithmetic (condition_mean + p_sample, condition_score + ddim_sample) in fp32 torch on the device;
    a clip at t = 0 takes no noise (its noise rows are NaN: they are not read)."""
    from syntalker_amd.process import create_gaussian_diffusion
    d = create_gaussian_diffusion(use_ddim=kind == "ddim")
    g = torch.Generator().manual_seed(3)
    B = 5
    top = d.num_timesteps - 1
    t = torch.tensor([0, 1, top // 2, top, 0], device=DEV)
    x, x0, grad, noise = (torch.randn(B, *SHAPE, generator=g).to(DEV) for _ in range(4))
    noise[t == 0] = float("nan")
    coef = guided.update_coefs(d.tables(), kind, eta, DEV)
    fn = lambda a, t_, **kw: grad
    safe = torch.nan_to_num(noise)
    if kind == "ddpm":
        mean, var, logvar = d.q_posterior_mean_variance(x0, x, t)
        got = guided.guide_update("ddpm", mean, x0, grad, coef, t.to(torch.int32), noise)
        p = {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": x0}
        want = d.condition_mean(fn, p, x, t) + d._nonzero(t, x) * torch.exp(0.5 * logvar) * safe
    else:
        got = guided.guide_update("ddim", x, x0, grad, coef, t.to(torch.int32), noise if eta else None)
        mean, var, logvar = d.q_posterior_mean_variance(x0, x, t)
        out = d.condition_score(fn, {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": x0}, x, t)
        want = d._ddim_update(out["pred_xstart"], x0, x, t, eta, safe)["sample"]
    err = rel_l2(got, want)
    print(f"syn_guide_update {kind} eta={eta}: rel-L2 {err:.3e}")
    assert bool(torch.isfinite(got).all()) and err < 1e-6, err


def test_update_kernel_draws_the_step_kernels_noise_bitwise():
    """a = 0, grad = 0, sigma = 1: the output IS the draw - equal to syn_randn for (seed, global clip, step) through `engine.seeded_noise`; t = 0 draws nothing."""
    B, seed, first = 3, 1234567, 5
    coef = torch.zeros(8, 8, device=DEV)
    coef[:, 1] = 1.0
    t = torch.tensor([7, 0, 3], dtype=torch.int32, device=DEV)
    z = torch.zeros(B, *SHAPE, device=DEV)
    got = guided.guide_update("ddpm", z, None, z, coef, t, None, seed, first)
    want = engine.seeded_noise(seed, first, [0, 1, 2], [7, 0, 3], DEV)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and bool((got[1] == 0).all())
    assert 0.9 < float(got[0].std()) < 1.1


# ---- the node -------------------------------------------------------------------------------------------------------------------------------------
def _grad_of(model, x, t, y, u):
    xr = x.clone().requires_grad_()
    out = model(xr, t, y=y)
    return out.detach(), torch.autograd.grad((u * out).sum(), xr)[0]


def test_node_output_equals_the_fused_step_and_dx_equals_the_reference(beatx, fx):
    y, x = synth.to_device(synth.synth_clip_inputs(2, seed=31), DEV), synth.synth_latent(2, seed=31).to(DEV)
    u, t = synth.synth_latent(2, seed=83, name="guided.u").to(DEV), torch.tensor([500, 37], device=DEV)
    out, dx = _grad_of(beatx, x, t, y, u)
    with torch.no_grad():
        fused = beatx(x, t, y=y)
    e_out, e_dx = rel_l2(out, fused), rel_l2(dx, fx["dx.beatx"])
    print(f"DenoiseFn beatx: output vs fused step {e_out:.3e}, dx vs reference {e_dx:.3e}")
    assert e_out < FWD_TOL and e_dx < GRAD_TOL, (e_out, e_dx)
    out2, dx2 = _grad_of(beatx, x, t, y, u)
    assert torch.equal(out, out2) and torch.equal(dx, dx2), "two runs must be bit-equal"


def test_node_under_classifier_free_guidance_dx_equals_the_reference(h3d, fx):
    from syntalker_amd.guidance import ClassifierFreeSampleModel
    y = synth.to_device(dict(synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), scale=torch.ones(1) * 2.5), DEV)
    x, u = synth.synth_latent(2, seed=7).to(DEV), synth.synth_latent(2, seed=83, name="guided.u").to(DEV)
    model = ClassifierFreeSampleModel(h3d)
    t = torch.tensor([500, 37], device=DEV)
    out, dx = _grad_of(model, x, t, y, u)
    with torch.no_grad():
        fused = model(x, t, y=y)
    e_out, e_dx = rel_l2(out, fused), rel_l2(dx, fx["dx.h3d_cfg"])
    print(f"DenoiseFn h3d under CFG 2.5: output vs fused step {e_out:.3e}, dx vs reference {e_dx:.3e}")
    assert e_out < FWD_TOL and e_dx < GRAD_TOL, (e_out, e_dx)
    assert torch.equal(dx, _grad_of(model, x, t, y, u)[1])


def test_padded_and_sliced_batches_equal_their_clips_alone(beatx, h3d):
    """B = 1 (1 -> 4 sequences), B = 3 with V = 2 (6 -> 8) and B = 68 (slices of 64 and 4): a clip's output and gradient do not depend on what shares its
    launch - every kernel of the node works row by row or sequence by sequence, with one summation order per element whatever the row count."""
    from syntalker_amd.guidance import ClassifierFreeSampleModel
    assert guided.plan(68) == [(0, 64, 64, 64), (64, 68, 4, 4)] and guided.plan(3, 2) == [(0, 3, 6, 8)] and guided.plan(1) == [(0, 1, 1, 4)]
    n = 68
    y, x = synth.to_device(synth.synth_clip_inputs(n, seed=41), DEV), synth.synth_latent(n, seed=41).to(DEV)
    u = synth.synth_latent(n, seed=42, name="guided.u").to(DEV)
    t = (torch.arange(n, device=DEV) * 13) % 1000
    cut = lambda lo, hi: {k: (v[lo:hi] if torch.is_tensor(v) and v.dim() and v.shape[0] == n else v) for k, v in y.items()}
    out, dx = _grad_of(beatx, x, t, y, u)
    for lo, hi in ((0, 1), (64, 68)):
        o, d = _grad_of(beatx, x[lo:hi], t[lo:hi], cut(lo, hi), u[lo:hi])
        assert torch.equal(o, out[lo:hi]) and torch.equal(d, dx[lo:hi]), (lo, hi)
    n = 3
    y = synth.to_device(dict(synth.synth_clip_inputs(3, seed=43, style_dim=256, style_zero=False), scale=torch.ones(1) * 2.5), DEV)
    x, u, t = synth.synth_latent(3, seed=43).to(DEV), synth.synth_latent(3, seed=44, name="guided.u").to(DEV), torch.tensor([900, 20, 333], device=DEV)
    model = ClassifierFreeSampleModel(h3d)
    out, dx = _grad_of(model, x, t, y, u)
    cut3 = lambda lo, hi: {k: (v[lo:hi] if torch.is_tensor(v) and v.dim() and v.shape[0] == 3 else v) for k, v in y.items()}
    o, d = _grad_of(model, x[1:2], t[1:2], cut3(1, 2), u[1:2])
    assert torch.equal(o, out[1:2]) and torch.equal(d, dx[1:2])


def test_training_after_the_guided_node_is_unchanged(beatx):
    """The node packs its own transposed weights and touches neither `StackFn` nor the step's pack caches: the same training step gives the same
    loss and gradients before and after it ran (eval-mode statistics, so that the step is deterministic)."""
    from syntalker_amd.process import create_gaussian_diffusion
    d = create_gaussian_diffusion()
    y, x0 = synth.to_device(synth.synth_clip_inputs(4, seed=51), DEV), synth.synth_latent(4, seed=51).to(DEV)
    y["mask"] = torch.ones(4, 1, 1, 32, dtype=torch.bool, device=DEV)
    t, noise = torch.tensor([10, 400, 700, 999], device=DEV), synth.synth_latent(4, seed=52).to(DEV)

    def step():
        beatx.zero_grad(set_to_none=True)
        beatx.differentiable_eval = True
        try:
            loss = d.training_losses(beatx, x0, t, model_kwargs={"y": y}, noise=noise)["loss"].mean()
            loss.backward()
        finally:
            beatx.differentiable_eval = False
        return loss.detach().clone(), beatx.mytimmblocks[3].attn.qkv.weight.grad.clone(), beatx.input_process.poseEmbedding.weight.grad.clone()
    before = step()
    _grad_of(beatx, x0, t, y, noise)
    after = step()
    beatx.zero_grad(set_to_none=True)
    for a, b in zip(before, after):
        assert rel_l2(b, a) < 1e-6


# ---- the loops -----------------------------------------------------------------------------------------------------------------------------------------
def _keep(fx):
    a, b = (int(v) for v in fx["keep.frames"])
    return longform.keep_mask(32, tuple(str(p) for p in fx["keep.parts"]), (a, b)).t().reshape(1, 1536, 1, 32).to(DEV)


def _case(fx, name, beatx, h3d):
    from syntalker_amd.guidance import ClassifierFreeSampleModel
    from syntalker_amd.process import create_gaussian_diffusion
    ddim = name.startswith(("ddim", "h3d"))
    d = create_gaussian_diffusion(use_ddim=ddim)
    kw, model = {}, beatx
    if name in ("ddim_grad", "ddim_nograd", "ddpm_grad", "ddpm_nograd"):
        y, x = synth.synth_clip_inputs(1, seed=2), synth.synth_latent(1, seed=2)
        if not ddim:
            kw = dict(skip_timesteps=990, step_noise=synth.synth_step_noise(10, 1, seed=93))
    elif name == "ddim_grad_inpaint":
        y, x = synth.synth_clip_inputs(2, seed=31), synth.synth_latent(2, seed=31)
        g = synth._gen("inpainting", 37)
        y["inpainting_mask"] = torch.rand(2, 1536, 1, 32, generator=g) < 0.25
        y["inpainted_motion"] = torch.randn(2, 1536, 1, 32, generator=g)
    else:
        y, x = dict(synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), scale=torch.ones(1) * 2.5), synth.synth_latent(2, seed=7)
        model = ClassifierFreeSampleModel(h3d)
    n = x.shape[0]
    with_grad = "nograd" not in name
    target = synth.synth_latent(2, seed=91, name="guided.target")[:n].to(DEV)
    fn = guided.keyframe_cond_fn(target, _keep(fx), float(fx[f"scale.{name}"]), with_grad)
    loop = d.ddim_sample_loop_progressive if ddim else d.p_sample_loop_progressive
    args = dict(noise=x.to(DEV), clip_denoised=False, cond_fn=fn, cond_fn_with_grad=with_grad, model_kwargs={"y": synth.to_device(y, DEV)}, **kw)
    return d, model, loop, (n,) + SHAPE, args, target


@pytest.mark.parametrize("name", ["ddim_grad", "ddim_nograd", "ddpm_grad", "ddpm_nograd", "ddim_grad_inpaint", "h3d_cfg_ddim_grad"])
def test_guided_loops_against_the_reference(fx, beatx, h3d, name):
    d, model, loop, shape, args, target = _case(fx, name, beatx, h3d)
    grads = []
    fn = args["cond_fn"]
    args["cond_fn"] = lambda *a, **k: (grads.append(fn(*a, **k)), grads[-1])[1]
    steps = list(loop(model, shape, **args))
    assert d.last_path == "guided"
    err = rel_l2(steps[-1]["sample"], fx[f"{name}.sample"])
    moved = rel_l2(steps[-1]["sample"], fx[f"plain.{name}"])
    print(f"guided loop {name}: rel-L2 vs reference {err:.3e} (gate {gate(fx, name):.3e}), distance from the unguided run {moved:.3f}")
    assert err < gate(fx, name), (err, gate(fx, name))
    if name != "h3d_cfg_ddim_grad":
        # the direction: nearer the target on `keep` than the unguided twin.  (Not under classifier-free guidance at 2.5: there the REFERENCE's
        # own guided run ends farther on this measure than its plain one, 1098.3 against 1094.7 - the objective acts on the combined output
        # while the distance is dominated by what the guidance scale amplifies - so the fixture decides that case, not the direction.)
        keep = _keep(fx).float()
        near = lambda v: float((keep * (torch.as_tensor(v).to(DEV) - target)).norm())
        assert near(steps[-1]["sample"]) < near(fx[f"plain.{name}"]), "guidance must pull the kept entries towards the target"
    if name == "ddim_grad":
        for s in (0, 49):
            for key, got in (("sample", steps[s]["sample"]), ("pred_xstart", steps[s]["pred_xstart"])):
                e = rel_l2(got, fx[f"ddim_grad.step{s}.{key}"])
                print(f"  step {s} {key}: {e:.3e}")
                assert e < gate(fx, name), (s, key, e)
        e = rel_l2(grads[0], fx["ddim_grad.step0.grad"])
        print(f"  step 0 cond_fn gradient: {e:.3e}")
        assert e < gate(fx, name), e


def test_loop_returns_the_progressive_steps_and_seed_reproduces(fx, beatx, h3d):
    d, model, loop, shape, args, _ = _case(fx, "ddpm_grad", beatx, h3d)
    args.pop("step_noise")
    run = lambda seed: d.p_sample_loop(model, shape, **args, seed=seed)
    a, b, c = run(11), run(11), run(12)
    assert torch.equal(a, b) and not torch.equal(a, c)
    d2, _, loop2, _, args2, _ = _case(fx, "ddim_grad", beatx, h3d)
    args2["skip_timesteps"] = 46
    steps = list(loop2(model, shape, **args2))
    assert len(steps) == 4 and torch.equal(steps[-1]["sample"], d2.ddim_sample_loop(model, shape, **args2))


def test_scale_zero_is_the_unguided_loop_bit_for_bit_under_ddpm(fx, beatx):
    """A cond_fn that returns zero leaves the sampler's arithmetic: the guided DDPM loop (mean mode) against the generic per-step loop on the same
    x_T and the same injected noise, end to end, EQUAL - `mean + variance * 0` is exact, `syn_guide_update` rounds `mean + sigma * noise` as torch
    does and takes sigma from the same torch.exp(0.5 * log_variance); model kernel and posterior mean are shared - and so is every step."""
    from syntalker_amd.process import create_gaussian_diffusion
    d = create_gaussian_diffusion()
    y, x = synth.to_device(synth.synth_clip_inputs(1, seed=2), DEV), synth.synth_latent(1, seed=2).to(DEV)
    zero = guided.keyframe_cond_fn(torch.zeros(1, *SHAPE, device=DEV), _keep(fx), 0.0, False)
    kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=990, step_noise=synth.synth_step_noise(10, 1, seed=93))
    got = list(d.p_sample_loop_progressive(beatx, (1,) + SHAPE, cond_fn=zero, **kw))
    assert d.last_path == "guided" and len(got) == 10
    want = list(d.p_sample_loop_progressive(beatx, (1,) + SHAPE, denoised_fn=lambda v: v, **kw))
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a["pred_xstart"], b["pred_xstart"]) and torch.equal(a["sample"], b["sample"]), k
    assert torch.equal(d.p_sample_loop(beatx, (1,) + SHAPE, cond_fn=zero, **kw), d.p_sample_loop(beatx, (1,) + SHAPE, denoised_fn=lambda v: v, **kw))
    assert d.last_path == "generic"


def test_scale_zero_under_ddim_equals_the_generic_step_at_every_step(fx, beatx):
    """Score mode (DDIM) re-derives pred_xstart from eps even for a zero gradient (condition_score, :469-478), so it is not the unguided step bit for
    bit, in the reference either.  Every step of the guided run, FROM ITS OWN x_t, against the generic step: pred_xstart bit-equal, the sample equal to
    fp32 rounding (measured 6.7e-8).  The end-to-end distance to the unguided generic loop is printed, not asserted: the fused step answers a
    one-ulp difference in x_t (26 342 of 49 152 elements after step 1, rel-L2 9e-8) with a 3e-3 difference in pred_xstart - measured on the
    generic path alone, fed the two step-1 samples - and 50 such steps end 4.4e-3 apart."""
    from syntalker_amd.process import create_gaussian_diffusion
    d = create_gaussian_diffusion(use_ddim=True)
    y, x = synth.to_device(synth.synth_clip_inputs(1, seed=2), DEV), synth.synth_latent(1, seed=2).to(DEV)
    zero = guided.keyframe_cond_fn(torch.zeros(1, *SHAPE, device=DEV), _keep(fx), 0.0, False)
    kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y})
    steps = list(d.ddim_sample_loop_progressive(beatx, (1,) + SHAPE, cond_fn=zero, **kw))
    assert d.last_path == "guided" and len(steps) == 50
    cur, worst = x, 0.0
    with torch.no_grad():
        for k, st in enumerate(steps):
            ref = d.ddim_sample(beatx, cur, torch.tensor([49 - k], device=DEV), clip_denoised=False, model_kwargs={"y": y})
            assert torch.equal(ref["pred_xstart"], st["pred_xstart"]), k
            worst = max(worst, rel_l2(st["sample"], ref["sample"]))
            cur = st["sample"]
    want = d.ddim_sample_loop(beatx, (1,) + SHAPE, denoised_fn=lambda v: v, **kw)
    print(f"scale 0, DDIM: worst single step vs the generic step {worst:.3e}; end to end vs the unguided generic loop {rel_l2(steps[-1]['sample'], want):.3e}")
    assert worst < 1e-6, worst          # a dozen fp32 operations per element in two orders


def test_per_clip_guidance_scales_sliced_over_two_launches(h3d):
    """A (B, 3, V) weight table - `y['scale']` with one value per clip - over a batch that runs as two slices (40 clips x 2 variants = 64 + 16
    sequences): a clip's output and gradient equal the clip alone with its own scalar scale (the scales and 1 - scale are exact in fp32)."""
    from syntalker_amd.guidance import ClassifierFreeSampleModel
    n = 40
    assert guided.plan(n, 2) == [(0, 32, 64, 64), (32, 40, 16, 16)]
    scale = 1.0 + 0.25 * (torch.arange(n) % 8).float()
    base = synth.synth_clip_inputs(n, seed=61, style_dim=256, style_zero=False)
    x, u = synth.synth_latent(n, seed=61).to(DEV), synth.synth_latent(n, seed=62, name="guided.u").to(DEV)
    t = ((torch.arange(n) * 29) % 1000).to(DEV)
    model = ClassifierFreeSampleModel(h3d)
    out, dx = _grad_of(model, x, t, synth.to_device(dict(base, scale=scale), DEV), u)
    for b in (3, 37):
        yb = {k: (v[b:b + 1] if torch.is_tensor(v) and v.dim() and v.shape[0] == n else v) for k, v in base.items()}
        o, g = _grad_of(model, x[b:b + 1], t[b:b + 1], synth.to_device(dict(yb, scale=scale[b:b + 1].clone()), DEV), u[b:b + 1])
        assert torch.equal(o, out[b:b + 1]) and torch.equal(g, dx[b:b + 1]), b


def test_sample_from_config_guide_from(tmp_path):
    """scripts/sample_from_config.py --guide-from / --guide-parts / --guide-frames / --guide-scale: one window on the guided loop; the guided parts end
    nearer the take than an unguided run's from the same seed (and are not copies of it)."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sample_from_config", os.path.join(repo, "scripts", "sample_from_config.py"))
    drv = importlib.util.module_from_spec(spec); spec.loader.exec_module(drv)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("vqvae_type: rvqvae\nvqvae_squeeze_scale: 4\nvqvae_latent_scale: 5\nuse_trans: True\naudio_f: 256\nword_f: 256\n"
                   "pose_length: 128\npre_frames: 4\npose_fps: 30\naudio_rep: onset+amplitude\n")
    B, n = 2, 150
    g = torch.Generator().manual_seed(9)
    np.savez(tmp_path / "take.npz", pose=(0.3 * torch.randn(B, n, 165, generator=g)).numpy(), trans_v=(0.1 * torch.randn(B, n, 3, generator=g)).numpy())
    common = [str(cfg), "--random-init", "--ddim", "--takes", str(B), "--seconds", "5"]
    sel = ["--guide-from", str(tmp_path / "take.npz"), "--guide-parts", "lower", "--guide-frames", "0:5"]
    rep = drv.main(common + sel)
    off = drv.main(common + sel + ["--guide-scale", "0"])
    assert rep["finite"] and rep["latents"] == [B, 32, 1536] and rep["guide"]["path"] == "guided"
    assert rep["guide"]["guided_fraction"] == round(1 / 3 + 2 / 3 * 5 / 32, 4)
    print(f"--guide-from: rel distance of the guided entries to the take {rep['guide']['rel_distance_to_take']} (scale 0: {off['guide']['rel_distance_to_take']})")
    assert 0 < rep["guide"]["rel_distance_to_take"] < off["guide"]["rel_distance_to_take"]
    with pytest.raises(SystemExit):
        drv.main(common + ["--guide-parts", "lower"])
    with pytest.raises(SystemExit):
        drv.main(common + ["--guide-from", str(tmp_path / "take.npz")])
