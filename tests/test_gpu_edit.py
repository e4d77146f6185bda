"""In-painting on the fused sampling loop (`syn_denoise_step_edit`): the blend x0 = keep ? known : x0 in each of the token-major output
stages, bit for bit against the same step without an edit; the loops against the reference's own output and the CPU oracle; graph and
buffer reuse; long takes.  Tolerances: `LOOP_TOL` is the project's loop bound (tests/test_gpu_parity.py); the step-level bound is worked
out in `test_step_blend_in_every_output_stage`."""
import os

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, engine, longform, synth
from tests.conftest import GOLDEN, rel_l2
from tests.refmodel import synth_state_dict

pytestmark = pytest.mark.gpu
LOOP_TOL = 3e-2
DEV = "cuda"
SHAPE = (1536, 1, 32)


def _model(variant="beatx"):
    if variant == "h3d":
        from syntalker_amd.denoiser_h3d import MDM
    else:
        from syntalker_amd.denoiser import MDM
    m = MDM(synth.default_args()).eval()
    missing, unexpected = m.load_state_dict(synth_state_dict(variant), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(DEV)


@pytest.fixture(scope="module")
def beatx():
    return _model("beatx")


@pytest.fixture(scope="module")
def h3d():
    return _model("h3d")


def _token_major(t_bct):
    """(B,1536,1,32) -> [B*32][1536], the layout of x_t / keep / known, by torch ops (independent of `load_edit`)."""
    return t_bct[:, :, 0, :].permute(0, 2, 1).reshape(-1, 1536).contiguous()


def _random_edit(B, g, p=0.5):
    """Bernoulli(p) mask per element (4-wide groups are mixed), last row and last column of the token-major tensor set, random motion."""
    mask = torch.rand(B, *SHAPE, generator=g) < p
    mask[B - 1, :, 0, 31] = True          # last token-major row: clip B-1, frame 31
    mask[:, 1535, 0, :] = True            # last column: channel 1535
    return mask, torch.randn(B, *SHAPE, generator=g)


def _part_mask(B, part="lower"):
    k = longform.PARTS.index(part)
    mask = torch.zeros(B, *SHAPE, dtype=torch.bool)
    mask[:, 512 * k:512 * (k + 1)] = True
    return mask


# ---- step level -----------------------------------------------------------------------------------------------------------------
# The smallest batches that reach each output stage under the library's own kernel choice (step_impl), plus the one 64-row-tile size
# (k_stack<64> has its own edit instance) and the small-batch kernel's whole-clip guided layout (ws_x0v = NULL).
STEP_CASES = [
    pytest.param(1, 1, 0, True, id="B1-k_lat"),
    pytest.param(2, 2, 0, True, id="B2V2-k_lat+k_guided_update"),
    pytest.param(2, 2, 0, False, id="B2V2-k_lat-whole-clips"),
    pytest.param(9, 1, 0, True, id="B9-k_stack-split4"),
    pytest.param(66, 1, 0, True, id="B66-k_stack-split2"),
    pytest.param(130, 1, 0, True, id="B130-k_stack-fused-output"),
    pytest.param(260, 1, 0, True, id="B260-k_stack-64-row-tiles"),
    pytest.param(40, 4, 0, True, id="B40V4-k_combine+k_gemm-EPI_OUT"),
    pytest.param(3, 1, 1, True, id="B3-layer_mode1-EPI_OUT"),
]


@pytest.mark.parametrize("B,V,layer_mode,x0v", STEP_CASES)
def test_step_blend_in_every_output_stage(beatx, B, V, layer_mode, x0v):
    """One evaluation through StepBuffers / run_step, with and without the edit, same inputs.
    Coefficient row (1, 0, 0): x_next and pred_x0 are where(keep, known, x0 of the unedited call) bit for bit.
    A posterior row with injected noise: entries that are not kept are bit-equal to the unedited call's; kept entries are the fp32
    expression c0*known + c1*x_t + sigma*eps, which takes four fp32 roundings of 6e-8 relative each (three products and sums, fused or not) -
    bound 1e-6 * (|c0 known| + |c1 x_t| + |sigma eps|), a 4x margin.  The bf16 shadow is the rounding of x_next."""
    from syntalker_amd.process import create_gaussian_diffusion
    pm = beatx.packed()
    g = torch.Generator().manual_seed(1000 * B + V)
    R = V * B * 32
    cond = (torch.randn(R, 512, generator=g) * 0.5).to(DEV)
    x, eps = torch.randn(B, *SHAPE, generator=g).to(DEV), torch.randn(B, *SHAPE, generator=g).to(DEV)
    t_model = torch.randint(0, 1000, (B,), generator=g).to(torch.int32).repeat(V).to(DEV)
    w = torch.randn(3, V, generator=g)
    w[:, -1] = 1.0 - w[:, :-1].sum(1)                          # guidance weights sum to 1 per block
    mask, motion = _random_edit(B, g)
    keep, known = _token_major(mask).to(DEV), _token_major(motion).to(DEV)
    post = engine.posterior_coefs(create_gaussian_diffusion().tables(), DEV)
    ident = engine.identity_coefs(DEV)

    def run(edit, coef, row, noisy):
        sb = engine.StepBuffers(B, V, DEV, want_x0=True, layer_mode=layer_mode, edit=edit)
        assert not sb.fragment
        if not x0v:
            sb.c.ws_x0v = None
        sb.cond.copy_(cond); sb.load_x(x); sb.load_noise(eps); sb.t_model.copy_(t_model); sb.t_coef.fill_(row)
        if V > 1:
            sb.cfg_w.copy_(w.to(DEV))
        if edit:
            sb.load_edit(mask, motion)
            assert torch.equal(sb.keep.bool(), keep) and torch.equal(sb.known, known)
        x_t = sb.x.clone()
        engine.run_step(pm, sb, coef, use_noise=noisy)
        torch.cuda.synchronize()
        sb.check_sync()
        return sb.x.clone(), sb.xb.clone(), sb.x0.clone(), x_t, sb.noise.clone()

    # (1, 0, 0): the blend itself
    p_x, _, p_x0, _, _ = run(False, ident, 0, False)
    e_x, e_xb, e_x0, _, _ = run(True, ident, 0, False)
    want = torch.where(keep, known, p_x0)
    assert torch.isfinite(p_x0).all()
    assert torch.equal(e_x0, want) and torch.equal(e_x, want)
    assert torch.equal(e_xb, e_x.to(torch.bfloat16))
    # a posterior row, injected noise
    row = 500
    p_x, _, p_x0, x_t, nz = run(False, post, row, True)
    e_x, e_xb, e_x0, _, _ = run(True, post, row, True)
    assert torch.equal(e_x0, torch.where(keep, known, p_x0))
    assert torch.equal(e_x[~keep], p_x[~keep])
    c = post[row].double()
    terms = [c[0] * known.double(), c[1] * x_t.double(), c[2] * nz.double()]
    err = (e_x.double() - (terms[0] + terms[1] + terms[2])).abs()
    bound = 1e-6 * (terms[0].abs() + terms[1].abs() + terms[2].abs())
    worst = float((err[keep] / bound[keep].clamp_min(1e-30)).max())
    print(f"B={B} V={V}: kept entries, worst error / bound = {worst:.3f}")
    assert (err[keep] <= bound[keep]).all()
    assert torch.equal(e_xb, e_x.to(torch.bfloat16))


def test_captured_edited_step_replays_equal_to_the_eager_call(beatx):
    """`syn_denoise_step_edit` allocates and synchronises nothing: a torch.cuda.graph capture of it replays to the eager result."""
    B = 2
    pm = beatx.packed()
    g = torch.Generator().manual_seed(11)
    sb = engine.StepBuffers(B, 1, DEV, want_x0=True, edit=True)
    cond, x = (torch.randn(B * 32, 512, generator=g) * 0.5).to(DEV), torch.randn(B, *SHAPE, generator=g).to(DEV)
    mask, motion = _random_edit(B, g)
    sb.cond.copy_(cond); sb.t_model.fill_(321); sb.t_coef.zero_(); sb.load_edit(mask, motion)
    ident = engine.identity_coefs(DEV)
    sb.load_x(x)
    engine.run_step(pm, sb, ident, use_noise=False)
    torch.cuda.synchronize()
    eager = sb.x.clone()
    graph = torch.cuda.CUDAGraph()
    sb.load_x(x)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        engine.run_step(pm, sb, ident, use_noise=False)
    sb.load_x(x)
    sb.x0.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sb.x, eager) and torch.equal(sb.x0, eager)
    keep, known = _token_major(mask).to(DEV), _token_major(motion).to(DEV)
    assert torch.equal(sb.x[keep], known[keep])


# ---- loop level -----------------------------------------------------------------------------------------------------------------
def test_reference_inpainting_output_on_the_fused_path(beatx):
    """The reference's own p_sample_loop output with y['inpainting_mask'] / y['inpainted_motion'] (loop_kwargs_outputs.npz), reproduced by
    the fused loop."""
    from syntalker_amd.process import create_gaussian_diffusion
    from tests.test_oracle_golden import _loop_kwargs_cases
    key, steps, seed, kw, extra = _loop_kwargs_cases()[4]
    assert key == "inpainting"
    fx = np.load(os.path.join(GOLDEN, "loop_kwargs_outputs.npz"))
    y = synth.to_device(dict(synth.synth_clip_inputs(2, seed=31), **extra), DEV)
    d = create_gaussian_diffusion()
    got = d.p_sample_loop(beatx, (2, *SHAPE), noise=synth.synth_latent(2, seed=31).to(DEV), model_kwargs={"y": y}, clip_denoised=False,
                          step_noise=synth.synth_step_noise(steps, 2, seed=seed), **kw)
    e = rel_l2(got.cpu(), fx[key])
    print(f"inpainting, fused path: rel-L2 vs the reference {e:.3e}")
    assert d.last_path == "fused"
    assert got.shape == fx[key].shape and e < LOOP_TOL, e
    # the paths that stay generic: a mask without a motion, a float mask
    d.p_sample_loop(beatx, (2, *SHAPE), noise=synth.synth_latent(2, seed=31).to(DEV), clip_denoised=False, skip_timesteps=999,
                    model_kwargs={"y": {k: v for k, v in y.items() if k != "inpainted_motion"}})
    assert d.last_path == "generic"


def _h3d_oracle():
    """model_fn(x, t, y) of the h3d restatement with the conditioning hoisted per (flags, style) set, as the product hoists it."""
    from oracle import denoiser_ref as dr
    sd = synth_state_dict("h3d")
    fw = dr.fold_weights(sd, variant="h3d")
    te = dr.time_table(sd, fw)
    cache = {}

    def fn(x, t, y):
        st = y["style_feature"]
        key = (bool(y.get("uncond")), bool(y.get("uncond_audio")), None if y.get("uncond") else tuple(st.flatten()[:3].tolist()),
               tuple(y["seed"].shape), float(y["seed"].flatten()[:16].sum()))
        if key not in cache:
            cache[key] = dr.clip_conditioning(sd, y, fw, variant="h3d")
        return dr.mdm_forward_folded(sd, fw, cache[key], te, x, t)
    return fn


def test_guided_edit_loops_vs_oracle(h3d):
    """10 steps under guidance with an edit, against the CPU restatement with the same mask: CFG at B = 2 (V = 2, the small-batch kernel's
    per-sequence groups + k_guided_update; DDPM, injected noise) and the body-part TwoCFG wrapper at B = 1 (V = 4; DDIM)."""
    from oracle import guidance_ref as gr
    from oracle.process_ref import RefProcess
    from syntalker_amd import guidance as G
    from syntalker_amd.process import create_gaussian_diffusion
    fn = _h3d_oracle()
    g = torch.Generator().manual_seed(21)
    # CFG, B = 2, DDPM tail of 10 steps
    B = 2
    y = synth.synth_clip_inputs(B, seed=71, style_dim=256, style_zero=False)
    mask, motion = _random_edit(B, g)
    mask |= _part_mask(B, "lower")
    y = dict(y, scale=torch.tensor([2.5, 1.5]), inpainting_mask=mask, inpainted_motion=motion)
    x, sn = synth.synth_latent(B, seed=71), synth.synth_step_noise(10, B, seed=72)
    d = create_gaussian_diffusion()
    got = d.p_sample_loop(G.ClassifierFreeSampleModel(h3d), (B, *SHAPE), noise=x.to(DEV), clip_denoised=False,
                          model_kwargs={"y": synth.to_device(y, DEV)}, skip_timesteps=990, step_noise=sn).cpu()
    assert d.last_path == "fused"
    with torch.no_grad():
        want = RefProcess(False).p_sample_loop(lambda a, b, c: gr.cfg(fn, a, b, c), (B, *SHAPE), dict(y), noise=x.clone(), step_noise=sn,
                                               skip_timesteps=990)
    e = rel_l2(got, want)
    print(f"CFG (V=2) + edit, 10 DDPM steps: rel-L2 vs oracle {e:.3e}")
    assert e < LOOP_TOL and torch.equal(got[mask], motion[mask])
    # body-part TwoCFG, B = 1, DDIM tail of 10 steps
    y1 = synth.synth_clip_inputs(1, seed=8, style_dim=256, style_zero=False)
    gp = synth._gen("part_prompts", 8)
    parts = {"upper_mask": torch.randn(1, 256, generator=gp), "hands_mask": None, "lower_mask": torch.randn(1, 256, generator=gp)}
    mask, motion = _random_edit(1, g)
    x = synth.synth_latent(1, seed=8)
    extra = {"scale": torch.ones(1), "inpainting_mask": mask, "inpainted_motion": motion}
    d = create_gaussian_diffusion(use_ddim=True)
    dparts = {k: (None if v is None else v.to(DEV)) for k, v in parts.items()}
    got = d.ddim_sample_loop(G.TwoClassifierFreeSampleModel_Bodypart(h3d), (1, *SHAPE), noise=x.to(DEV), clip_denoised=False,
                             model_kwargs={"y": dict(synth.to_device(dict(y1, **extra), DEV), style_feature=dparts)}, skip_timesteps=40).cpu()
    assert d.last_path == "fused"
    with torch.no_grad():
        want = RefProcess(True).ddim_sample_loop(lambda a, b, c: gr.two_cfg_bodypart(fn, a, b, c), (1, *SHAPE),
                                                 dict(y1, style_feature=parts, **extra), noise=x.clone(),
                                                 step_noise=torch.zeros(10, 1, *SHAPE), skip_timesteps=40)
    e = rel_l2(got, want)
    print(f"body-part TwoCFG (V=4) + edit, 10 DDIM steps: rel-L2 vs oracle {e:.3e}")
    assert e < LOOP_TOL and torch.equal(got[mask], motion[mask])


@pytest.mark.parametrize("B", [1, 9])
def test_all_false_mask_equals_the_call_without_an_edit(beatx, B):
    """An edit that keeps nothing is the plain loop, bit for bit: DDPM (20 steps, in-library noise) and DDIM at eta 0 and 0.5."""
    from syntalker_amd.process import create_gaussian_diffusion
    y = synth.to_device(synth.synth_clip_inputs(B, seed=81), DEV)
    x = synth.synth_latent(B, seed=81).to(DEV)
    none = torch.zeros(B, *SHAPE, dtype=torch.bool, device=DEV)
    ye = dict(y, inpainting_mask=none, inpainted_motion=torch.randn(B, *SHAPE, device=DEV))
    d = create_gaussian_diffusion()
    run = lambda yy: d.p_sample_loop(beatx, (B, *SHAPE), noise=x.clone(), clip_denoised=False, model_kwargs={"y": yy}, skip_timesteps=980, seed=17)
    plain, edited = run(y), run(ye)
    assert d.last_path == "fused" and torch.isfinite(plain).all() and torch.equal(plain, edited)
    d = create_gaussian_diffusion(use_ddim=True)
    for eta in (0.0, 0.5):
        run = lambda yy: d.ddim_sample_loop(beatx, (B, *SHAPE), noise=x.clone(), clip_denoised=False, model_kwargs={"y": yy}, eta=eta, seed=23)
        plain, edited = run(y), run(ye)
        assert d.last_path == "fused" and torch.equal(plain, edited), eta


def test_kept_entries_are_the_motion_and_buffers_are_refilled(beatx):
    """A body-part mask: the kept entries of the result are `inpainted_motion` bit for bit (the last step is x_next = x0), for DDPM and DDIM,
    also through `dump_steps` and `progress`.  A second loop of the same shapes with another mask and motion follows the new ones and
    reuses the buffers and the captured graphs (they hold the buffers' pointers: refilled, not reallocated)."""
    from syntalker_amd.process import create_gaussian_diffusion
    B = 2
    y = synth.to_device(synth.synth_clip_inputs(B, seed=91), DEV)
    x = synth.synth_latent(B, seed=91).to(DEV)
    g = torch.Generator().manual_seed(5)
    lower, upper = _part_mask(B, "lower").to(DEV), _part_mask(B, "upper").to(DEV)
    m1, m2 = torch.randn(B, *SHAPE, generator=g).to(DEV), torch.randn(B, *SHAPE, generator=g).to(DEV)
    d = create_gaussian_diffusion()
    run = lambda mask, motion, **kw: d.p_sample_loop(beatx, (B, *SHAPE), noise=x.clone(), clip_denoised=False, skip_timesteps=985, seed=3,
                                                     model_kwargs={"y": dict(y, inpainting_mask=mask, inpainted_motion=motion)}, **kw)
    a = run(lower, m1)
    sb = beatx.step_buffers(B, 1, edit=True)
    ptrs, n_graphs = (sb.keep.data_ptr(), sb.known.data_ptr(), sb.x.data_ptr()), len(beatx._syn_graphs)
    assert d.last_path == "fused" and torch.equal(a[lower], m1[lower]) and not torch.equal(a[upper], m1[upper])
    b = run(upper, m2)
    assert torch.equal(b[upper], m2[upper]) and not torch.equal(b[lower], m1[lower])
    assert beatx.step_buffers(B, 1, edit=True) is sb and (sb.keep.data_ptr(), sb.known.data_ptr(), sb.x.data_ptr()) == ptrs
    assert len(beatx._syn_graphs) == n_graphs
    assert torch.equal(run(lower, m1), a)                                             # and back: nothing of the second loop is left behind
    assert torch.equal(run(lower, m1, progress=True)[lower], m1[lower])
    dumped = run(lower, m1, dump_steps=[0, 14])
    assert len(dumped) == 2 and torch.equal(dumped[1][lower], m1[lower]) and not torch.equal(dumped[0][lower], m1[lower])
    assert rel_l2(dumped[1].cpu(), a.cpu()) < 5e-3                  # (one step per replay instead of ten: the same steps)
    d = create_gaussian_diffusion(use_ddim=True)
    for eta in (0.0, 0.5):
        c = d.ddim_sample_loop(beatx, (B, *SHAPE), noise=x.clone(), clip_denoised=False, eta=eta, seed=4, skip_timesteps=35,
                               init_image=m2, model_kwargs={"y": dict(y, inpainting_mask=lower, inpainted_motion=m1)})
        assert d.last_path == "fused" and torch.isfinite(c).all() and torch.equal(c[lower], m1[lower])


def test_edit_at_a_size_the_wave_per_sequence_kernel_claims(beatx):
    """768 clips: `syn_prefers_fragment_order` says fragment order, which takes no edit - the buffers are token-major and the whole-step
    kernel (64-row tiles) runs the two steps."""
    from syntalker_amd.process import create_gaussian_diffusion
    B = 768
    assert _lib.load().syn_prefers_fragment_order(B, 1) == 1
    y4 = synth.synth_clip_inputs(4, seed=31)
    y = synth.to_device({k: (v.repeat(B // 4, *([1] * (v.dim() - 1))) if torch.is_tensor(v) else v) for k, v in y4.items()}, DEV)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, *SHAPE, generator=g).to(DEV)
    mask, motion = _part_mask(B, "lower").to(DEV), torch.randn(B, *SHAPE, generator=g).to(DEV)
    d = create_gaussian_diffusion(use_ddim=True)
    got = d.ddim_sample_loop(beatx, (B, *SHAPE), noise=x, clip_denoised=False, skip_timesteps=48,
                             model_kwargs={"y": dict(y, inpainting_mask=mask, inpainted_motion=motion)})
    assert d.last_path == "fused"
    assert beatx.step_buffers(B, 1, edit=True).fragment is False and beatx.step_buffers(B, 1).fragment is True
    assert torch.isfinite(got).all() and torch.equal(got[mask], motion[mask])


# ---- long takes -----------------------------------------------------------------------------------------------------------------
def test_sample_long_with_an_edit(beatx):
    """2 takes of 352 pose frames (3 windows), DDIM, the last 5 of the 50 steps; keep = the lower third everywhere plus every channel at
    latent frames 10..20.  Kept entries of the stitched latents are `known_latent` bit for bit; the whole result against the same windows
    through the CPU oracle one by one; an all-False keep is `sample_long` without an edit."""
    from oracle import denoiser_ref as dr
    from oracle.process_ref import RefProcess
    from syntalker_amd.process import create_gaussian_diffusion
    sd = synth_state_dict("beatx")
    n, B, W, skip = 128 + 2 * 112, 2, 3, 45
    g = torch.Generator().manual_seed(5)
    audio = torch.randn(B, n * 533, 2, generator=g)
    word = torch.randint(0, synth.VOCAB, (B, n), generator=g)
    seed = torch.randn(B, n // 4, 1536, generator=g)
    known = torch.randn(B, n // 4, 1536, generator=g)
    keep = longform.keep_mask(n // 4, ("lower",), frames=(10, 21))
    xs = [torch.randn(B, *SHAPE, generator=g) for _ in range(W)]
    d = create_gaussian_diffusion(use_ddim=True)
    run = lambda **kw: longform.sample_long(d, beatx, audio.to(DEV), word.to(DEV), seed.to(DEV), n, use_ddim=True,
                                            noise_fn=lambda i: xs[i].to(DEV), skip_timesteps=skip, **kw).cpu()
    got = run(edit=(known.to(DEV), keep))
    assert d.last_path == "fused" and got.shape == (B, W * 28 + 4, 1536)
    kb = keep.expand(B, -1, -1)
    assert torch.equal(got[kb], known[kb])
    proc, last, pieces = RefProcess(True), None, []
    with torch.no_grad():
        for i in range(W):
            y = longform.window_inputs(i, audio, word, seed, last, 112)
            y["inpainted_motion"], y["inpainting_mask"] = longform.window_edit(i, known, keep, 112)
            s = proc.ddim_sample_loop(lambda a, b, c: dr.mdm_forward(sd, a, b, c), (B, *SHAPE), y, noise=xs[i].clone(),
                                      step_noise=torch.zeros(50 - skip, B, *SHAPE), skip_timesteps=skip)
            last = s[:, :, 0, :].permute(0, 2, 1)
            pieces.append(last if i == 0 else last[:, 4:])
    want = torch.cat(pieces, 1)
    e = rel_l2(got, want)
    print(f"3-window take with an edit: rel-L2 vs oracle {e:.3e}")
    assert e < LOOP_TOL
    assert torch.equal(run(edit=(known.to(DEV), torch.zeros_like(keep))), run())


# ---- the caller -----------------------------------------------------------------------------------------------------------------
def test_sample_from_config_keep_from(tmp_path):
    """scripts/sample_from_config.py --keep-from / --keep-parts / --keep-frames: a recorded take through `poses.encode_take`, two windows
    on the fused loop, the kept entries of the sampled latents equal to the take's."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sample_from_config", os.path.join(repo, "scripts", "sample_from_config.py"))
    drv = importlib.util.module_from_spec(spec); spec.loader.exec_module(drv)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("vqvae_type: rvqvae\nvqvae_squeeze_scale: 4\nvqvae_latent_scale: 5\nuse_trans: True\naudio_f: 256\nword_f: 256\n"
                   "pose_length: 128\npre_frames: 4\npose_fps: 30\naudio_rep: onset+amplitude\n")
    B, n = 2, 240                                               # 8 s at 30 fps: two windows, 60 latent frames
    g = torch.Generator().manual_seed(9)
    np.savez(tmp_path / "take.npz", pose=(0.3 * torch.randn(B, n, 165, generator=g)).numpy(),
             trans_v=(0.1 * torch.randn(B, n, 3, generator=g)).numpy())
    common = [str(cfg), "--random-init", "--ddim", "--takes", str(B), "--seconds", "8"]
    rep = drv.main(common + ["--keep-from", str(tmp_path / "take.npz"), "--keep-parts", "lower", "--keep-frames", "0:5"])
    assert rep["finite"] and rep["windows"] == 2 and rep["latents"] == [B, 60, 1536]
    assert rep["edit"] == {"path": "fused", "kept_fraction": round(1 / 3 + 2 / 3 * 5 / 60, 4), "kept_exact": True}
    with pytest.raises(SystemExit):                              # what to keep, but no take to keep it from
        drv.main(common + ["--keep-parts", "lower"])
    with pytest.raises(SystemExit):                              # a take, but nothing named to keep
        drv.main(common + ["--keep-from", str(tmp_path / "take.npz")])
