"""The PLMS sampler on the fused loop (`syn_plms_update`, `engine.PlmsLoop`, `plms_sample_loop`): the history kernel alone against its
fp64 formula, one PLMS step through every step kernel, the loops against the reference's recorded outputs (tests/golden/plms_outputs*.npz),
and the agreement of the paths.

Loop gate: the project's loop bound 3e-2 (tests/test_gpu_parity.py; 4.3x its measured DDIM-50 error), scaled for case c by
max(1, amp.c / amp.ddim50) - how much more the reference's own sampler amplifies a relative model-output error of 5e-3 than DDIM-50 does,
measured on the reference alone and stored with the fixture.

(The module's name sorts it behind tests/test_gpu_rvq_train.py: one test there asserts that a parameter moved to the CPU and back gets another
device address, which holds or not with what the modules before it left in PyTorch's caching allocator - it held in whole-suite runs without
this module in front of it and not with it.)"""
import gc
import os

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, engine, longform, synth, tape
from tests.conftest import GOLDEN, rel_l2
from tests.refmodel import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (1536, 1, 32)
LOOP_TOL = 3e-2


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
    """After the module (its models, buffers and captured graphs are finalised first): hand the cached blocks back, so that the allocator
    the next module meets is the one this module met."""
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
    for part in ("", "_2clips", "_pins_sample", "_pins_pred_xstart"):          # (four files: a committed file stays under 1 MiB)
        out.update(np.load(os.path.join(GOLDEN, f"plms_outputs{part}.npz")))
    return out


@pytest.fixture(scope="module")
def ddim():
    from syntalker_amd.process import create_gaussian_diffusion
    return create_gaussian_diffusion(use_ddim=True)


def gate(fx, case):
    return LOOP_TOL * max(1.0, float(fx[f"amp.{case}"]) / float(fx["amp.ddim50"]))


def device_rows(tab):
    """`plms_coefs` rows as the device table: [L][32 bytes] uint8, and the same values as the kernel holds them (fp32) in fp64."""
    L = len(tab["store"])
    rows = np.zeros(L, dtype=[("f", np.float32, 7), ("store", np.int32)])
    rows["f"], rows["store"] = tab["hist"], tab["store"]
    return torch.from_numpy(rows.view(np.uint8).reshape(L, -1).copy()).to(DEV), rows["f"].astype(np.float64), rows["store"]


# ---- the update kernel alone ------------------------------------------------------------------------------------------------------
def well_conditioned_inputs(n, f, store, seed):
    """x_t, x0_hat and three ring slots with magnitudes log-uniform over 1e-3 .. 30 and random signs, such that at every element both sums
    the kernel forms - r x - x0 and H - are at least half the sum of their terms' magnitudes (elements that are not are redrawn).  fp32
    cannot give a per-element RELATIVE bound on a sum that cancels; with that condition the bound is: e_new two roundings (2 x 6e-8, x2 for
    the condition), H at most five fused multiply-adds (5 x 6e-8 x 2) plus e_new's error through its term (2.4e-7 x 2): 1.1e-6 < 2e-6."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda m: (torch.exp(torch.empty(m, dtype=torch.float64).uniform_(np.log(1e-3), np.log(30.0), generator=g))
                      * (torch.randint(0, 2, (m,), generator=g) * 2 - 1)).float()
    v = torch.stack([draw(n) for _ in range(5)])                      # x_t, x0, ring 0..2
    for _ in range(200):
        x, x0, ring = v[0].double(), v[1].double(), v[2:].double()
        e_terms = torch.stack([f[0] * x, -x0])
        e = e_terms.sum(0) * f[1]
        h_terms = torch.stack([f[2] * x, f[3] * e] + [f[4 + k] * ring[k] * (k != store) for k in range(3)])
        bad = (e_terms.sum(0).abs() < 0.5 * e_terms.abs().sum(0)) | (h_terms.sum(0).abs() < 0.5 * h_terms.abs().sum(0))
        m = int(bad.sum())
        if m == 0:
            return v[0], v[1], v[2:].contiguous(), e, h_terms.sum(0)
        v[:, bad] = torch.stack([draw(m) for _ in range(5)])
    raise AssertionError("could not draw well-conditioned inputs")


def run_update(rows_dev, idx, back, x, x0, ring, n):
    counter = torch.tensor([idx + back], dtype=torch.int32, device=DEV)
    x, x0, ring = x.to(DEV), x0.to(DEV), ring.clone().to(DEV)
    H = torch.full((n,), float("nan"), device=DEV)
    _lib.check(_lib.load().syn_plms_update(rows_dev.data_ptr(), rows_dev.shape[0], counter.data_ptr(), back, x.data_ptr(), x0.data_ptr(),
                                           ring.data_ptr(), H.data_ptr(), n, _lib.current_stream(DEV)), "syn_plms_update")
    torch.cuda.synchronize()
    return ring.cpu(), H.cpu()


# rows 0..7 of an order-4 loop: the start's two launches (h_x; ring only, nothing kept), the ramp, then every phase of the ring
@pytest.mark.parametrize("B,rows", [(1, range(8)), (3, range(8)), (9, range(8)), (44, (0, 6))], ids=["B1", "B3", "B9", "B44-more-than-one-grid-pass"])
def test_update_kernel_against_its_fp64_formula_in_both_layouts(ddim, B, rows):
    """e_new and H per element at <= 2e-6 relative (`well_conditioned_inputs` derives it), every other ring slot untouched, at every
    ring phase; the same call on the fragment-order images of the inputs gives the fragment-order images of the outputs bit for bit.
    44 clips are 540 672 float4s: more than one pass of the 2048 x 256-thread grid, the second one partial."""
    tab = engine.plms_coefs(ddim.tables(), 4, 50)
    rows_dev, f64, store = device_rows(tab)
    n = B * 32 * 1536
    frag = lambda t: tape.to_fragment_order(t.view(B, 32, 1536)).reshape(-1)
    worst = 0.0
    for idx in rows:
        f, st = f64[idx], int(store[idx])
        x, x0, ring, e_want, h_want = well_conditioned_inputs(n, f, st, seed=100 * B + idx)
        ring_out, H = run_update(rows_dev, idx, 3, x, x0, ring, n)
        for k in range(3):
            if k != st:
                assert torch.equal(ring_out[k], ring[k]), (idx, k)
        if st >= 0:
            err = ((ring_out[st].double() - e_want).abs() / e_want.abs()).max()
            worst = max(worst, float(err))
            assert err <= 2e-6, (idx, float(err))
        err = ((H.double() - h_want).abs() / h_want.abs()).max()
        worst = max(worst, float(err))
        assert err <= 2e-6, (idx, float(err))
        ring_f, H_f = run_update(rows_dev, idx, 3, frag(x), frag(x0), torch.stack([frag(r) for r in ring]), n)
        assert torch.equal(H_f, frag(H)) and all(torch.equal(ring_f[k], frag(ring_out[k])) for k in range(3)), idx
    print(f"B={B}: worst relative error per element {worst:.3e}")


def test_update_kernel_leaves_everything_alone_outside_its_table_and_on_empty_rows(ddim):
    tab = engine.plms_coefs(ddim.tables(), 2, 50)
    rows_dev, f64, store = device_rows(tab)
    n = 32 * 1536
    x, x0, ring = torch.randn(n), torch.randn(n), torch.randn(3, n)
    assert store[50] == -1 and not f64[50, 2:].any()                  # the update after the last step
    for idx in (50, 51, 5000, -2):
        ring_out, H = run_update(rows_dev[:51], idx, 1, x, x0, ring, n)
        assert torch.equal(ring_out, ring) and torch.isnan(H).all(), idx


# ---- one PLMS step through every step kernel ----------------------------------------------------------------------------------------
STEP_CASES = [
    pytest.param(1, 1, 0, False, id="B1-k_lat"),
    pytest.param(9, 1, 0, False, id="B9-k_stack-split-tiles"),
    pytest.param(3, 2, 0, False, id="B3V2-guided"),
    pytest.param(3, 4, 0, False, id="B3V4-guided"),
    pytest.param(2, 1, 0, True, id="B2-edit"),
    pytest.param(4, 1, 5, False, id="B4-k_seq-fragment-order"),
]


@pytest.mark.parametrize("B,V,mode,edit", STEP_CASES)
def test_one_plms_step_through_every_step_kernel(beatx, ddim, B, V, mode, edit):
    """Launch 6 of an order-4 loop (steady state: own weight 55/24, history injected as `noise`) from latent 0 into latent 1 through
    `PlmsLoop`: x_next = c_x0 pred_x0 + c_xt x_t + beta H in fp64 from the kernel's own pred_x0 (rel-L2 1e-6, the bound of the DDIM step
    tests), x_t untouched, then the update's e_new and next H from the same pred_x0.  This is the wiring, not the model."""
    pm = beatx.packed()
    g = torch.Generator().manual_seed(7 * B + V)
    sb = engine.StepBuffers(B, V, DEV, layer_mode=mode, edit=edit, plms=True)
    assert sb.fragment == (mode == 5) and sb.x0 is not None
    loop = engine.PlmsLoop(pm, sb)
    tab = engine.plms_coefs(ddim.tables(), 4, 50)
    loop.load(("test", 4, 50), lambda: tab, lambda t: int(ddim.timestep_map[t]))
    sb.cond.copy_(torch.randn(V * B * 32, 512, generator=g) * 0.5)
    if V > 1:
        w = torch.randn(3, V, generator=g)
        w[:, -1] = 1.0 - w[:, :-1].sum(1)
        sb.cfg_w.copy_(w.to(DEV))
    if edit:
        mask = torch.rand(B, *SHAPE, generator=g) < 0.5
        sb.load_edit(mask, torch.randn(B, *SHAPE, generator=g))
    sb.load_x(torch.randn(B, *SHAPE, generator=g).to(DEV))
    sb.noise.copy_(torch.randn(B * 32, 1536, generator=g))
    sb.ring.copy_(torch.randn(3, B * 32, 1536, generator=g))
    L = 6
    loop.counter.fill_(L)
    x_t, H, ring = sb.x.clone(), sb.noise.clone(), sb.ring.clone()
    loop.issue(0, eager=True)
    torch.cuda.synchronize()
    sb.check_sync()
    assert int(loop.counter) == L + 1 and int(sb.t_coef[0]) == L and int(sb.t_model[0]) == ddim.timestep_map[tab["t"][L]]
    assert torch.equal(sb.x, x_t)
    c = loop.coef[L].double()
    x0 = sb.x0.double()
    assert torch.isfinite(x0).all()
    if edit:
        assert torch.equal(sb.x0[sb.keep.bool()], sb.known[sb.keep.bool()])
    want = c[0] * x0 + c[1] * x_t.double() + c[2] * H.double()
    e = rel_l2(sb.x2.double().cpu(), want.cpu())
    print(f"B={B} V={V}: x_next rel-L2 vs the fp64 row {e:.2e}")
    assert e < 1e-6
    if not sb.fragment:                                       # (fragment order: the bf16 operand has its own element order, tests/test_gpu_seq.py)
        assert torch.equal(sb.xb2, sb.x2.to(torch.bfloat16))
    f, st = torch.tensor(np.asarray(tab["hist"][L], np.float32)).double(), int(tab["store"][L])
    e_new = (f[0] * x_t.double() - x0) * f[1]
    h_next = f[3] * e_new + sum(f[4 + k] * ring[k].double() for k in range(3) if k != st)
    assert st == (L - 1) % 3 and rel_l2(sb.ring[st].double().cpu(), e_new.cpu()) < 1e-6
    assert rel_l2(sb.noise.double().cpu(), h_next.cpu()) < 1e-6
    assert all(torch.equal(sb.ring[k], ring[k]) for k in range(3) if k != st)


# ---- loops against the reference ----------------------------------------------------------------------------------------------------
def _beatx_case(B, seed):
    return synth.to_device(synth.synth_clip_inputs(B, seed=seed), DEV), synth.synth_latent(B, seed=seed).to(DEV)


@pytest.mark.parametrize("case,order,skip", [("o2", 2, 0), ("o3", 3, 0), ("o4", 4, 0), ("o3_skip40", 3, 40)])
def test_beatx_loops_vs_reference(beatx, ddim, fx, case, order, skip):
    y, xT = _beatx_case(1, 2)
    got = ddim.plms_sample_loop(beatx, (1, *SHAPE), noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y}, order=order,
                                skip_timesteps=skip)
    assert ddim.last_path == "fused"
    e = rel_l2(got.cpu(), fx[f"{case}.sample"])
    print(f"plms {case}: rel-L2 vs reference {e:.3e} (gate {gate(fx, case):.3e})")
    assert e < gate(fx, case)


def test_order_four_step_pins_vs_reference(beatx, ddim, fx):
    """`sample` and `pred_xstart` after steps 0 (the two-call start), 1, 2, 3 (orders 2, 3, 4) and 49, each within the loop's gate."""
    y, xT = _beatx_case(1, 2)
    kw = {"y": y}
    mdm, plan_fn = ddim._fusable(beatx, kw, None, None, False, False, False, False, (1, *SHAPE))
    seen = {}

    def each(k, sb, x):
        if k in (0, 1, 2, 3, 49):
            seen[k] = (sb.read(x).cpu(), sb.read(sb.x0).cpu())
    final = ddim._fused("plms", mdm, plan_fn, (1, *SHAPE), xT.clone(), kw, 0.0, 0, None, None, None, False, each, 0, order=4)
    assert sorted(seen) == [0, 1, 2, 3, 49] and torch.equal(final.cpu(), seen[49][0])
    for k, (sample, x0) in seen.items():
        es, e0 = rel_l2(sample, fx[f"o4.step{k}.sample"]), rel_l2(x0, fx[f"o4.step{k}.pred_xstart"])
        print(f"plms o4 step {k}: sample {es:.3e}, pred_xstart {e0:.3e} (gate {gate(fx, 'o4'):.3e})")
        assert es < gate(fx, "o4") and e0 < gate(fx, "o4"), k


def test_inpainting_loop_vs_reference(beatx, ddim, fx):
    y, x = _beatx_case(2, 31)
    g = synth._gen("inpainting", 37)
    mask = torch.rand(2, *SHAPE, generator=g) < 0.25
    motion = torch.randn(2, *SHAPE, generator=g)
    got = ddim.plms_sample_loop(beatx, (2, *SHAPE), noise=x.clone(), clip_denoised=False, order=2,
                                model_kwargs={"y": dict(y, inpainting_mask=mask.to(DEV), inpainted_motion=motion.to(DEV))})
    assert ddim.last_path == "fused"
    e = rel_l2(got.cpu(), fx["o2_inpaint.sample"])
    print(f"plms o2_inpaint: rel-L2 vs reference {e:.3e} (gate {gate(fx, 'o2_inpaint'):.3e})")
    assert e < gate(fx, "o2_inpaint")
    assert torch.equal(got.cpu()[mask], motion[mask])


def test_guided_h3d_loop_vs_reference(h3d, ddim, fx):
    from syntalker_amd.guidance import ClassifierFreeSampleModel
    y = synth.to_device(synth.synth_clip_inputs(2, seed=7, style_dim=256, style_zero=False), DEV)
    x = synth.synth_latent(2, seed=7).to(DEV)
    got = ddim.plms_sample_loop(ClassifierFreeSampleModel(h3d), (2, *SHAPE), noise=x.clone(), clip_denoised=False, order=2,
                                model_kwargs={"y": dict(y, scale=torch.ones(1, device=DEV) * 2.5)})
    assert ddim.last_path == "fused"
    e = rel_l2(got.cpu(), fx["h3d_cfg_o2.sample"])
    print(f"plms h3d_cfg_o2: rel-L2 vs reference {e:.3e} (gate {gate(fx, 'h3d_cfg_o2'):.3e})")
    assert e < gate(fx, "h3d_cfg_o2")


# ---- agreement of the paths -----------------------------------------------------------------------------------------------------------
def test_fused_loop_equals_generic_loop(beatx, ddim):
    """Order 3, 10 steps, 2 clips: the bound test_gpu_parity.py puts on DDPM's fused against generic loop (the bf16 re-rounding floor)."""
    y, xT = _beatx_case(2, 21)
    kw = dict(noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y}, order=3, skip_timesteps=40)
    fused = ddim.plms_sample_loop(beatx, (2, *SHAPE), **kw)
    assert ddim.last_path == "fused"
    final = None
    for out in ddim.plms_sample_loop_progressive(beatx, (2, *SHAPE), **kw):
        final = out["sample"]
    e = rel_l2(fused.cpu(), final.cpu())
    print(f"plms fused vs generic: {e:.3e}")
    assert e < 1e-2


@pytest.mark.parametrize("B", [1, 9])
def test_graph_replays_equal_the_eager_launches_bitwise(beatx, ddim, B):
    """13 steps of order 4: the start graph, one ten-step graph, two single-step graphs (one per direction) against the same launches made
    eagerly."""
    pm = beatx.packed()
    y, xT = _beatx_case(B, 40 + B)
    sb = engine.StepBuffers(B, 1, DEV, plms=True)
    sb.cond.copy_(beatx.variant_conds(y, [(False, False, None)]).reshape(-1, 512))
    loop = engine.PlmsLoop(pm, sb)
    outs = []
    for eager in (True, False, False):
        sb.load_x(xT)
        loop.load((4, 13), lambda: engine.plms_coefs(ddim.tables(), 4, 13), lambda t: int(ddim.timestep_map[t]))
        outs.append(sb.read(loop.run(eager=eager)))
    assert set(loop.graphs) == {"start", "multi", 0, 1}
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


def test_batch_whole_and_as_two_slices_is_bitwise_equal(beatx, ddim):
    from syntalker_amd.sharding import shard_kwargs
    y, xT = _beatx_case(5, 51)
    run = lambda yy, x, **kw: ddim.plms_sample_loop(beatx, (x.shape[0], *SHAPE), noise=x.clone(), clip_denoised=False,
                                                    model_kwargs={"y": yy}, order=3, skip_timesteps=38, **kw)
    whole = run(y, xT)
    parts = [run(shard_kwargs(y, lo, hi, 5), xT[lo:hi], first_clip=lo) for lo, hi in ((0, 2), (2, 5))]
    assert ddim.last_path == "fused" and torch.equal(whole, torch.cat(parts, 0))


def test_ddim_loop_is_what_it_was_after_a_plms_loop(beatx, ddim):
    y, xT = _beatx_case(3, 61)
    run = lambda: ddim.ddim_sample_loop(beatx, (3, *SHAPE), noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y})
    before = run()
    for order in (2, 4):
        ddim.plms_sample_loop(beatx, (3, *SHAPE), noise=xT.clone(), clip_denoised=False, model_kwargs={"y": y}, order=order)
    assert torch.equal(run(), before)


def test_sample_long_with_the_plms_sampler_is_the_window_by_window_loop(beatx, ddim):
    n, B = 128 + 112, 2
    g = torch.Generator().manual_seed(6)
    audio = torch.randn(B, n * 533, 2, generator=g).to(DEV)
    word = torch.randint(0, synth.VOCAB, (B, n), generator=g).to(DEV)
    seed = torch.randn(B, n // 4, 1536, generator=g).to(DEV)
    xs = [torch.randn(B, *SHAPE, generator=g).to(DEV) for _ in range(2)]
    got = longform.sample_long(ddim, beatx, audio, word, seed, n, sampler="plms", plms_order=3, noise_fn=lambda i: xs[i], skip_timesteps=42)
    assert ddim.last_path == "fused" and got.shape == (B, 2 * 28 + 4, 1536)
    last, pieces = None, []
    for i in range(2):
        yw = longform.window_inputs(i, audio, word, seed, last, 112)
        s = ddim.plms_sample_loop(beatx, (B, *SHAPE), noise=xs[i], clip_denoised=False, model_kwargs={"y": yw}, order=3, skip_timesteps=42)
        last = s[:, :, 0, :].permute(0, 2, 1).contiguous()
        pieces.append(last if i == 0 else last[:, 4:])
    assert torch.equal(got, torch.cat(pieces, 1))
    with pytest.raises(ValueError):
        longform.sample_long(ddim, beatx, audio, word, seed, n, sampler="heun")


def test_sample_from_config_with_plms(tmp_path):
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sample_from_config", os.path.join(repo, "scripts", "sample_from_config.py"))
    drv = importlib.util.module_from_spec(spec); spec.loader.exec_module(drv)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("vqvae_type: rvqvae\nvqvae_squeeze_scale: 4\nvqvae_latent_scale: 5\nuse_trans: True\naudio_f: 256\nword_f: 256\n"
                   "pose_length: 128\npre_frames: 4\npose_fps: 30\naudio_rep: onset+amplitude\n")
    rep = drv.main([str(cfg), "--random-init", "--plms", "--plms-order", "3", "--takes", "2", "--seconds", "8"])
    assert rep["finite"] and rep["windows"] == 2 and rep["latents"] == [2, 60, 1536] and rep["sampler"] == "plms50-order3"
    with pytest.raises(SystemExit):
        drv.main([str(cfg), "--random-init", "--plms", "--ddim"])
