"""calc_bpd_loop on the device (`syn_bpd_terms`, `engine.BpdBatch`, the fused path of `GaussianDiffusion.calc_bpd_loop`): the reduction kernel
alone against fp64 evaluations of the reference's formulas (K1-K3), and whole calls against the reference's recorded outputs
(tests/golden/bpd_outputs*.npz, E1-E5).

Bound on the scalars of a whole call.  The project's forward gate is rel-L2(pred_x0) <= 2e-2.  With k = ||pred_ref|| / ||pred_ref - x_start||
(stored per clip and timestep with the fixture) an error of that size moves ||pred - x_start|| by at most rho = 2e-2 k relative, and
xstart_mse - its square over a constant - by 2 rho + rho^2; mse and the KL are that quantity times a constant of t.  k is about 0.95 for the
random-weight models, so the bound is about 3.9e-2: loose on purpose, derived, not tuned.  The t = 0 term is no multiple of xstart_mse: it
is held to the kernel's own rule (K2) on the device's returned pred_xstart, and pred_xstart to the forward gate at two pins.

(The module's name sorts it behind tests/test_gpu_rvq_train.py, like tests/test_gpu_sampler_plms.py and for its reason: one test there depends on
what the modules before it left in PyTorch's caching allocator.)"""
import gc
import os

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, engine, process, synth, tape
from tests.conftest import GOLDEN, rel_l2
from tests.refmodel import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (1536, 1, 32)
N = 32 * 1536
FWD_GATE = 2e-2
NOISE_SEED = 5
KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


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
    out = dict(np.load(os.path.join(GOLDEN, "bpd_outputs.npz")))
    out.update(np.load(os.path.join(GOLDEN, "bpd_outputs_pins.npz")))
    return out


@pytest.fixture(scope="module")
def ddim():
    return process.create_gaussian_diffusion(use_ddim=True)


@pytest.fixture(scope="module")
def noise50():
    return synth.synth_step_noise(50, 2, seed=NOISE_SEED).to(DEV)


# ---- the reference's formulas on the CPU, in a chosen precision ------------------------------------------------------------------------
def ref_terms(rows, t_row, clip, x_start, x_t, noise, pred, dtype):
    """(vb, xstart_mse, mse) per sequence from the table values as the kernel holds them (fp32), evaluated in `dtype` with the generic
    path's functions (process.normal_kl / discretized_gaussian_log_likelihood: the reference's, op for op)."""
    out = np.zeros((3, len(t_row)))
    for i, (t, c) in enumerate(zip(t_row, clip)):
        r = {k: torch.tensor(float(rows[k][t]), dtype=dtype) for k in ("c1", "c2", "log_var", "r", "inv_m")}
        x0, xt, nz, p = (v.to(dtype) for v in (x_start[c], x_t[i], noise[i], pred[i]))
        true_mean, mean = r["c1"] * x0 + r["c2"] * xt, r["c1"] * p + r["c2"] * xt
        lv = r["log_var"].expand(x0.shape)
        if rows["first"][t]:
            vb = -process.discretized_gaussian_log_likelihood(x0, means=mean, log_scales=0.5 * lv)
        else:
            vb = process.normal_kl(true_mean, lv, mean, lv)
        eps = (r["r"] * xt - p) * r["inv_m"]
        out[:, i] = (float(vb.mean() / np.log(2.0)), float(((p - x0) ** 2).mean()), float(((eps - nz) ** 2).mean()))
    return out


def device_rows(rows):
    return torch.from_numpy(rows.view(np.uint8).reshape(len(rows), -1).copy()).to(DEV)


def run_kernel(rows, t_row, clip, x_start, x_t, noise, pred):
    """x_start (n_clips, 49152), the others (n_seq, 49152): fp32 CPU tensors, in any one layout."""
    n_seq = len(t_row)
    dev = lambda t: t.contiguous().to(DEV)
    tab, tr = device_rows(rows), torch.tensor(t_row, dtype=torch.int32, device=DEV)
    cl = None if clip is None else torch.tensor(clip, dtype=torch.int32, device=DEV)
    a, b, c, d = dev(x_start), dev(x_t), dev(noise), dev(pred)
    out = torch.full((3, n_seq), float("nan"), device=DEV)
    _lib.check(_lib.load().syn_bpd_terms(tab.data_ptr(), len(rows), tr.data_ptr(), _lib.ptr(cl), a.data_ptr(), a.shape[0], b.data_ptr(),
                                         c.data_ptr(), d.data_ptr(), n_seq, out.data_ptr(), _lib.current_stream(DEV)), "syn_bpd_terms")
    torch.cuda.synchronize()
    return out.cpu()


def first_term_rule(hip, want64, got32):
    """K2's rule: the fp32 formula itself loses the tail of the discretised likelihood (cdf+ - cdf- cancels, then the 1e-12 clamp), so the
    yardstick is the reference's own fp32 error against fp64; the factor 2: a second fp32 realisation lands on other sides of the clamp."""
    gap = abs(got32 - want64) / want64
    err = abs(hip - want64) / want64
    return err, max(1e-5, 2 * gap), gap


def k1_inputs(ddim, seed=11):
    g = torch.Generator().manual_seed(seed)
    rows = engine.bpd_rows(ddim.tables())
    t_row, clip = [0, 49, 17, 0, 1], [0, 1, 1, 0, 1]
    x_start = torch.randn(2, N, generator=g)
    noise = torch.randn(5, N, generator=g)
    a, s = torch.from_numpy(ddim.sqrt_alphas_cumprod).float()[t_row], torch.from_numpy(ddim.sqrt_one_minus_alphas_cumprod).float()[t_row]
    x_t = a[:, None] * x_start[clip] + s[:, None] * noise
    pred = x_start[clip] + torch.randn(5, N, generator=g)
    return rows, t_row, clip, x_start, x_t, noise, pred


# ---- K1 ------------------------------------------------------------------------------------------------------------------------------
def test_kernel_sums_against_fp64_in_both_layouts(ddim):
    """rtol 1e-5: the sum itself is exact over the 16-byte groups, a group's four terms and the element-wise work add a few ulp of fp32
    (6e-8 each); an fp32 tree sum would be good to log2(49152) 2^-24 = 1e-6 - the gate leaves a factor of ten over that."""
    rows, t_row, clip, x_start, x_t, noise, pred = k1_inputs(ddim)
    want = ref_terms(rows, t_row, clip, x_start, x_t, noise, pred, torch.float64)
    want32 = ref_terms(rows, t_row, clip, x_start, x_t, noise, pred, torch.float32)
    got = run_kernel(rows, t_row, clip, x_start, x_t, noise, pred)
    err = (got.double().numpy() - want) / want
    print("relative error against fp64 (rows vb, xstart_mse, mse):\n", err)
    assert np.isfinite(got.numpy()).all()
    kl = [i for i, t in enumerate(t_row) if t != 0]
    assert np.abs(err[1:]).max() <= 1e-5 and np.abs(err[0, kl]).max() <= 1e-5
    for i in (0, 3):                                                      # the two t == 0 sequences: K2's rule
        e, bound, gap = first_term_rule(float(got[0, i]), want[0, i], want32[0, i])
        print(f"t = 0, sequence {i}: hip {float(got[0, i]):.7g} fp64 {want[0, i]:.7g} fp32 {want32[0, i]:.7g}: err {e:.3e} bound {bound:.3e}")
        assert e <= bound
    # the same tensors in fragment order: the same 16-byte groups, permuted - bitwise the same outputs
    frag = lambda t: tape.to_fragment_order(t.view(-1, 32, 1536)).reshape(t.shape[0], N)
    assert torch.equal(run_kernel(rows, t_row, clip, frag(x_start), frag(x_t), frag(noise), frag(pred)), got)
    # one sequence; clip = NULL (sequence i takes clip i)
    for i in range(5):
        one = run_kernel(rows, [t_row[i]], [clip[i]], x_start, x_t[i:i + 1], noise[i:i + 1], pred[i:i + 1])
        assert torch.equal(one[:, 0], got[:, i]), i
    ident = run_kernel(rows, [t_row[0], t_row[1]], None, x_start, x_t[:2], noise[:2], pred[:2])
    assert torch.equal(ident, got[:, :2])                                # (clip[0], clip[1] = 0, 1)
    one = run_kernel(rows, [t_row[0]], None, x_start, x_t[:1], noise[:1], pred[:1])
    assert torch.equal(one[:, 0], got[:, 0])


def test_kernel_answers_nan_for_an_index_outside_its_table(ddim):
    rows, t_row, clip, x_start, x_t, noise, pred = k1_inputs(ddim)
    got = run_kernel(rows, t_row, clip, x_start, x_t, noise, pred)
    bad = run_kernel(rows, [0, 50, 17, -1, 1], [0, 1, 2, 0, -1], x_start, x_t, noise, pred)
    assert torch.isnan(bad[:, 1:]).all() and torch.equal(bad[:, 0], got[:, 0])


# ---- K2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_ddim", [False, True], ids=["full", "ddim50"])
def test_kernel_first_term_against_the_reference_formula(use_ddim):
    d = process.create_gaussian_diffusion(use_ddim=use_ddim)
    rows = engine.bpd_rows(d.tables())
    sigma0 = float(np.exp(0.5 * rows["log_var"][0].astype(np.float64)))
    g = torch.Generator().manual_seed(23)
    ms = [0.3, 3.0, 30.0, 2000.0]
    x_start = torch.randn(1, N, generator=g)
    noise = torch.randn(len(ms), N, generator=g)
    x_t = float(d.sqrt_alphas_cumprod[0]) * x_start + float(d.sqrt_one_minus_alphas_cumprod[0]) * noise
    pred = torch.stack([x_start[0] + m * sigma0 * torch.randn(N, generator=g) for m in ms])
    t_row, clip = [0] * len(ms), [0] * len(ms)
    want64 = ref_terms(rows, t_row, clip, x_start, x_t, noise, pred, torch.float64)
    want32 = ref_terms(rows, t_row, clip, x_start, x_t, noise, pred, torch.float32)
    got = run_kernel(rows, t_row, clip, x_start, x_t, noise, pred)
    worst = 0.0
    edge = float(((x_start < -0.999) | (x_start > 0.999)).float().mean())
    print(f"sigma_0 {sigma0:.4e}, elements in an edge branch {edge:.3f}")
    for i, m in enumerate(ms):
        e, bound, gap = first_term_rule(float(got[0, i]), want64[0, i], want32[0, i])
        worst = max(worst, e / bound)
        print(f"m = {m}: hip {float(got[0, i]):.7g} fp64 {want64[0, i]:.7g} fp32 {want32[0, i]:.7g}: gap {gap:.3e} err {e:.3e} bound {bound:.3e}")
    print(f"worst err / bound {worst:.3f}")
    for i, m in enumerate(ms):
        e, bound, _ = first_term_rule(float(got[0, i]), want64[0, i], want32[0, i])
        assert e <= bound, m
    err = np.abs(got[1:].double().numpy() - want64[1:]) / want64[1:]
    assert err.max() <= 1e-5                                             # xstart_mse and mse of the same sequences


# ---- K3 ------------------------------------------------------------------------------------------------------------------------------
def test_kernel_is_bitwise_reproducible_and_independent_of_the_launch(ddim):
    rows, t_row, clip, x_start, x_t, noise, pred = k1_inputs(ddim, seed=12)
    a = run_kernel(rows, t_row, clip, x_start, x_t, noise, pred)
    b = run_kernel(rows, t_row, clip, x_start, x_t, noise, pred)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    for i in range(5):
        alone = run_kernel(rows, [t_row[i]], [clip[i]], x_start, x_t[i:i + 1], noise[i:i + 1], pred[i:i + 1])
        assert torch.equal(alone[:, 0], a[:, i]), i
    order = [4, 2, 0, 3, 1]                                              # ... and of its place in it
    p = run_kernel(rows, [t_row[i] for i in order], [clip[i] for i in order], x_start, x_t[order], noise[order], pred[order])
    assert torch.equal(p, a[:, order])


# ---- whole calls -----------------------------------------------------------------------------------------------------------------------
def scalar_bound(fx, case):
    rho = FWD_GATE * fx[f"{case}.pred_norm"] / fx[f"{case}.err_norm"]
    return 2 * rho + rho ** 2                                            # (B, T), loop order


def first_term_on_cpu(d, x_start, pred_t0, dtype):
    """vb at t = 0 from a pred_xstart: c1 = 1 and c2 = 0 there, so the mean is pred."""
    lv = torch.tensor(float(np.float32(d.posterior_log_variance_clipped[0])), dtype=dtype).expand(x_start.shape)
    nll = -process.discretized_gaussian_log_likelihood(x_start.to(dtype), means=pred_t0.to(dtype), log_scales=0.5 * lv)
    return (process.mean_flat(nll) / np.log(2.0)).double().numpy()


def check_against_reference(d, res, fx, case, x_start, label, pins=False):
    B, T = fx[f"{case}.vb"].shape
    bound = scalar_bound(fx, case)
    got = {k: res[k].cpu().double().numpy() for k in KEYS}
    assert all(got[k].shape == fx[f"{case}.{k}"].shape for k in KEYS) and all(np.isfinite(got[k]).all() for k in KEYS)
    worst = 0.0
    for k, cols in (("xstart_mse", slice(0, T)), ("mse", slice(0, T)), ("vb", slice(0, T - 1))):
        ratio = np.abs(got[k][:, cols] / fx[f"{case}.{k}"][:, cols].astype(np.float64) - 1) / bound[:, cols]
        worst = max(worst, float(ratio.max()))
        print(f"{label} {k}: worst |ratio - 1| / bound {float(ratio.max()):.3f} (bound {float(bound.min()):.3e} .. {float(bound.max()):.3e})")
    assert worst <= 1.0
    if "pred_xstart" in res:
        pred_t0 = res["pred_xstart"][-1].cpu()
        w64, w32 = first_term_on_cpu(d, x_start.cpu(), pred_t0, torch.float64), first_term_on_cpu(d, x_start.cpu(), pred_t0, torch.float32)
        for b in range(B):
            e, bnd, gap = first_term_rule(got["vb"][b, -1], w64[b], w32[b])
            print(f"{label} t = 0, clip {b}: hip {got['vb'][b, -1]:.7g} fp64 {w64[b]:.7g} fp32 {w32[b]:.7g} reference {fx[f'{case}.vb'][b, -1]:.7g}: "
                  f"err {e:.3e} bound {bnd:.3e}")
            assert e <= bnd
        if pins:
            for tag, row in (("tlast", 0), ("t0", -1)):
                e = rel_l2(res["pred_xstart"][row, 0].cpu(), fx[f"{case}.pred_xstart.{tag}"])
                print(f"{label} pred_xstart {tag}: rel-L2 {e:.3e}")
                assert e <= FWD_GATE
    assert np.allclose(got["prior_bpd"], fx[f"{case}.prior_bpd"], rtol=1e-5, atol=0)
    slack = (bound * fx[f"{case}.vb"].astype(np.float64)).sum(1)
    delta = np.abs(got["total_bpd"] - fx[f"{case}.total_bpd"])
    print(f"{label} total_bpd: |delta| / slack {float((delta / slack).max()):.3f}")
    assert (delta <= slack).all()


def beatx_inputs():
    return synth.synth_latent(2, seed=31).to(DEV), synth.to_device(synth.synth_clip_inputs(2, seed=31), DEV)


# ---- E1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [8, None, 64], ids=["chunk8-small-batch-kernel", "one-batch-of-100-split-tiles", "chunk64"])
def test_fused_call_vs_reference(beatx, ddim, fx, noise50, chunk):
    x, y = beatx_inputs()
    res = ddim.calc_bpd_loop(beatx, x, clip_denoised=False, model_kwargs={"y": y}, noise=noise50, chunk=chunk, return_pred_xstart=True)
    assert ddim.last_path == "fused" and res["pred_xstart"].shape == (50, 2, *SHAPE)
    check_against_reference(ddim, res, fx, "beatx_ddim50", x, f"beatx_ddim50 chunk={chunk}", pins=True)


# ---- E2 ------------------------------------------------------------------------------------------------------------------------------
def test_fused_call_over_the_full_process_vs_reference(beatx, fx):
    """2000 sequences: by default one batch of two passes of the wave-per-sequence kernel in fragment order (976 left over a full pass is
    more than half a pass); chunk=256: whole tiles of the whole-step kernel, and a remainder of 208."""
    d = process.create_gaussian_diffusion()
    x, y = beatx_inputs()
    noise = synth.synth_step_noise(1000, 2, seed=NOISE_SEED)
    for chunk in (None, 256):
        res = d.calc_bpd_loop(beatx, x, clip_denoised=False, model_kwargs={"y": y}, noise=noise, chunk=chunk, return_pred_xstart=True)
        assert d.last_path == "fused"
        res["pred_xstart"] = res["pred_xstart"][-1:]
        check_against_reference(d, res, fx, "beatx_full", x, f"beatx_full chunk={chunk}")
        del res


# ---- E3 ------------------------------------------------------------------------------------------------------------------------------
def test_guided_h3d_call_vs_reference(h3d, ddim, fx, noise50):
    from syntalker_amd.guidance import ClassifierFreeSampleModel
    y = synth.to_device(synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), DEV)
    x = synth.synth_latent(2, seed=7).to(DEV)
    res = ddim.calc_bpd_loop(ClassifierFreeSampleModel(h3d), x, clip_denoised=False, model_kwargs={"y": dict(y, scale=torch.ones(1, device=DEV) * 2.5)},
                             noise=noise50, return_pred_xstart=True)
    assert ddim.last_path == "fused"
    check_against_reference(ddim, res, fx, "h3d_cfg_ddim50", x, "h3d_cfg_ddim50")


# ---- E4 ------------------------------------------------------------------------------------------------------------------------------
def test_clipping_and_inpainting_take_the_generic_path(beatx, ddim, fx, noise50):
    x, y = beatx_inputs()
    res = ddim.calc_bpd_loop(beatx, x, model_kwargs={"y": y}, noise=noise50, return_pred_xstart=True)          # the reference's default: clip_denoised=True
    assert ddim.last_path == "generic"
    assert float(res["pred_xstart"].abs().max()) <= 1.0
    check_against_reference(ddim, res, fx, "beatx_ddim50_clipped", x, "beatx_ddim50_clipped (generic)")
    g = synth._gen("inpainting", 37)
    mask = (torch.rand(2, *SHAPE, generator=g) < 0.25).to(DEV)
    motion = torch.randn(2, *SHAPE, generator=g).to(DEV)
    res = ddim.calc_bpd_loop(beatx, x, clip_denoised=False, model_kwargs={"y": dict(y, inpainting_mask=mask, inpainted_motion=motion)}, noise=noise50,
                             return_pred_xstart=True)
    assert ddim.last_path == "generic" and torch.isfinite(res["total_bpd"]).all()
    assert torch.equal(res["pred_xstart"][:, mask], motion[mask].expand(50, -1))


# ---- E5 ------------------------------------------------------------------------------------------------------------------------------
def test_seeded_draws_do_not_depend_on_the_sharding(beatx, ddim, fx):
    from syntalker_amd.sharding import shard_kwargs
    x, y = beatx_inputs()
    run = lambda xx, yy, **kw: ddim.calc_bpd_loop(beatx, xx, clip_denoised=False, model_kwargs={"y": yy}, seed=7, **kw)
    whole = run(x, y)
    assert ddim.last_path == "fused"
    again = run(x, y)
    assert all(torch.equal(whole[k], again[k]) for k in KEYS)
    parts = [run(x[b:b + 1], shard_kwargs(y, b, b + 1, 2), first_clip=b) for b in range(2)]
    bound = 2 * scalar_bound(fx, "beatx_ddim50")
    for k, cols in (("xstart_mse", slice(0, 50)), ("mse", slice(0, 50)), ("vb", slice(0, 49))):
        got = torch.cat([p[k] for p in parts], 0).cpu().double().numpy()
        ratio = np.abs(got[:, cols] / whole[k].cpu().double().numpy()[:, cols] - 1) / bound[:, cols]
        print(f"two one-clip calls against one two-clip call, {k}: worst |ratio - 1| / (2 x bound) {float(ratio.max()):.3e}")
        assert ratio.max() <= 1.0
    other = ddim.calc_bpd_loop(beatx, x, clip_denoised=False, model_kwargs={"y": y}, seed=8)
    assert not torch.equal(other["mse"], whole["mse"])
    # the draws themselves: pair (b, t) is keyed by the global clip index and the timestep, whatever the call's batch is
    both = engine.seeded_noise(7, 0, [0, 1, 0, 1], [49, 49, 3, 3], DEV)
    second = engine.seeded_noise(7, 1, [0, 0], [49, 3], DEV)
    assert torch.equal(both[1], second[0]) and torch.equal(both[3], second[1]) and not torch.equal(both[0], both[2])
    for bad in (torch.zeros(50, 1, *SHAPE), torch.zeros(49, 2, *SHAPE), torch.zeros(2, 50, *SHAPE)):
        with pytest.raises(ValueError, match="noise must have shape"):
            ddim.calc_bpd_loop(beatx, x, clip_denoised=False, model_kwargs={"y": y}, noise=bad)


def test_eval_bpd_script_prints_its_table(tmp_path, capsys):
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_bpd", os.path.join(repo, "scripts", "eval_bpd.py"))
    drv = importlib.util.module_from_spec(spec); spec.loader.exec_module(drv)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("vqvae_type: rvqvae\nvqvae_squeeze_scale: 4\nvqvae_latent_scale: 5\nuse_trans: True\naudio_f: 256\nword_f: 256\n"
                   "pose_length: 128\npre_frames: 4\npose_fps: 30\naudio_rep: onset+amplitude\n")
    rep = drv.main([str(cfg), "--random-init", "--ddim", "--clips", "3", "--out", str(tmp_path / "bpd.npz")])
    assert rep == dict(rep, path="fused", clips=3, timesteps=50, finite=True)
    text = capsys.readouterr().out
    assert "xstart_mse" in text and "total_bpd" in text and sum(line.split()[0].isdigit() for line in text.splitlines() if line.split()) >= 26
    z = np.load(tmp_path / "bpd.npz")
    assert z["vb"].shape == (3, 50) and z["total_bpd"].shape == (3,)
