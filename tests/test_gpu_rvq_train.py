"""Codec training on the HIP kernels (syntalker_amd/rvq_training.py over csrc/syn_rvq_train.inc) against the reference's own train-mode outputs
(tests/golden/rvq_train_step*.npz) and the fp32 torch restatement of the step (tests/rvq_train_ref.py, itself pinned to that fixture by
tests/test_rvq_train_host.py).  Every random input of a step is injected (`draws`).

Bounds: the quantiser is fp32 and a discrete decision - indices EQUAL, outputs 1e-6, commit 1e-4, perplexity 1e-3 (tests/test_gpu_rvq.py's), EMA state
1e-5; rec_pose 2e-2 rel-L2 (the eval path's bound); every parameter gradient 3e-2 rel-L2 against the restatement's autograd fed the HIP indices
(the gate tests/test_gpu_parity.py puts on bf16-operand gradients).  Measured values: DESIGN.md 16.5.
Shapes: (N 3, T 16, dim 57) has 4 latent frames, fewer than the dilation of 9 - every non-centre tap of those convolutions reads padding and the
weight gradient's shifted reads leave the clip - an odd N, and 12 rows < 512 codes (`_tile`'s repeat-and-noise branch); (2, 64, 78) runs with
start = 2 (layers 3 .. 5 skipped); dims 57 / 78 / 180 are no multiples of 32 (padded lanes in the first weight gradient and the last data gradient);
(8, 256, 57) has 512 latent rows, the first count at which `_tile` takes no noise, and K up to 2048.  The quantiser alone also runs at 511 / 512 /
513 / 1030 rows (section 1b), where its indices are judged in fp64 along the kernel's own picks instead of being asked to equal an fp32 chain's.
Draws the fixture does not hold come from `ref.make_draws`; every step asserts that its indices spread over more than one code per layer (an
earlier version of the Gumbel expression was NaN everywhere and every row picked code 0: tests/test_rvq_train_host.py).
The kernels one at a time, at far tighter bounds: tests/test_gpu_rvq_train_kernels.py."""
import os

import numpy as np
import pytest
import torch

from syntalker_amd import rvq_training, rvqvae, synth
from tests import rvq_train_ref as ref
from tests.rvq_train_ref import make_draws

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(GOLDEN)


def to_dev(draws):
    mv = lambda v: v.to(DEV) if torch.is_tensor(v) else v
    return {k: ([[mv(z) for z in v] if isinstance(v, list) else mv(v) for v in val] if isinstance(val, list) else val) for k, val in draws.items()}


def new_trainer(dim, **kw):
    model = rvqvae.build(dim)
    model.load_state_dict(synth.synth_vq_state_dict(dim))
    return rvq_training.RVQTrainer(model.to(DEV), **kw)


def check_state(tr, q, codebook, code_sum, code_count, pre=None, fx=None):
    """EMA state of layer q within 1e-5: against the fixture's samples / norms, or against full tensors."""
    got = (tr.model.get_buffer(f"quantizer.layers.{q}.codebook").cpu(), tr.code_sum[q].cpu())
    for name, g, want in zip(("codebook", "code_sum"), got, (codebook, code_sum)):
        if fx is not None:
            nrm, smp = ref.sample(g)
            assert np.abs(smp.numpy() - fx[pre + f"{name}{q}.sample"]).max() <= 1e-5, (name, q)
            assert abs(nrm - float(fx[pre + f"{name}{q}.norm"])) <= 1e-5 * max(1.0, nrm), (name, q)
        else:
            assert float((g - want).abs().max()) <= 1e-5, (name, q)
    want_n = torch.from_numpy(fx[pre + f"code_count{q}"]) if fx is not None else code_count
    assert float((tr.code_count[q].cpu() - want_n).abs().max()) <= 1e-5, q


# ---- 1. the quantiser alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_quantiser_equals_the_reference(fx, case):
    """The fixture's fp32 latents and draws through RVQTrainer.quantize: n_active 6 (two steps: the first initialises every codebook, the second
    replaces the dead codes of initialised ones) and n_active 3 (first-step initialisation, layers 3 .. 5 untouched)."""
    n, t, dim, _, steps = (int(v) for v in fx["cases"][case])
    tr = new_trainer(dim)
    untouched = tr.model.get_buffer("quantizer.layers.5.codebook").clone()
    for s in range(steps):
        pre = f"c{case}.s{s}."
        if s == 1:
            assert (fx[pre + "code_count0"] < 1.0).any()                  # dead codes on an initialised codebook: this step resets them
        out = tr.quantize(torch.from_numpy(fx[pre + "latent"]).to(DEV), to_dev(ref.fixture_draws(fx, case, s)))
        assert np.array_equal(out["idx"].cpu().numpy(), fx[pre + "idx"])
        assert float((out["xq"].cpu() - torch.from_numpy(fx[pre + "xq"])).abs().max()) <= 1e-6
        commit, perp = float(out["commit"]), float(out["perplexity"])
        print(f"case {case} step {s}: commit {commit:.6e} (ref {fx[pre + 'scalars'][2]:.6e}) perplexity {perp:.4f} (ref {fx[pre + 'scalars'][3]:.4f})")
        assert abs(commit - float(fx[pre + "scalars"][2])) <= 1e-4 and abs(perp - float(fx[pre + "scalars"][3])) <= 1e-3
        for q in range(out["n_active"]):
            check_state(tr, q, None, None, None, pre, fx)
        assert tr.init == [q < out["n_active"] for q in range(6)]
    if case == 1:
        assert torch.equal(tr.model.get_buffer("quantizer.layers.5.codebook"), untouched) and float(tr.code_count[5].abs().max()) == 0.0


def test_quantiser_with_one_active_layer(fx):
    """n_active = 1 (start = 0) on case 0's latents, against the restatement (which equals the reference bit for bit on the fixture)."""
    lat = torch.from_numpy(fx["c0.s0.latent"])
    draws = ref.fixture_draws(fx, 0, 0)
    draws["start"] = 0
    tr = new_trainer(57)
    out = tr.quantize(lat.to(DEV), to_dev(draws))
    st = ref.new_state()
    cbs = [synth.synth_vq_state_dict(57)[f"quantizer.layers.{q}.codebook"].clone() for q in range(6)]
    xq, idx, commit, perp, n_active = ref.residual_vq(cbs, st, lat.permute(0, 2, 1).clone(), draws)
    assert n_active == 1 == out["n_active"] and np.array_equal(out["idx"].cpu().numpy(), idx.numpy()) and (idx[:, 1:] == -1).all()
    assert float((out["xq"].cpu() - xq.permute(0, 2, 1)).abs().max()) <= 1e-6
    assert abs(float(out["commit"]) - float(commit)) <= 1e-4 and abs(float(out["perplexity"]) - float(perp)) <= 1e-3
    check_state(tr, 0, cbs[0], st["code_sum"][0], st["code_count"][0])


# ---- 1b. the quantiser at the workload's row counts --------------------------------------------------------------------------------------
# rows = N x T': 511 is the last shape on `_tile`'s noise side, 512 the first without noise (a null noise pointer, dead codes reset from row c of
# the batch), 513 leaves a tail of one row in k_quantize_train<4> and makes k_code_update walk chunks of 256 + 256 + 1 rows, 1030 runs
# k_quantize_train<16> with 6 clamped tail rows and sums sqerr over 65 groups.  Latent frames need no pose: `quantize` takes (N, T', 512).
QUANT_SHAPES = {511: (7, 73), 512: (8, 64), 513: (9, 57), 1030: (5, 206)}


@pytest.fixture(scope="module")
def vq_sd():
    return synth.synth_vq_state_dict(57)


def check_quantiser_step(tr, vq_sd, rows, step, draws=None):
    """One `RVQTrainer.quantize` from the trainer's current state.  The indices are judged in fp64 along the kernel's own picks
    (ref.judge_picks / check_picks: "indices equal" cannot be asked of an fp32 distance chain over a thousand rows), everything else against
    the restatement started from the same state and fed those picks."""
    n, t4 = QUANT_SHAPES[rows]
    init = list(tr.init)
    cbs = [tr.model.get_buffer(f"quantizer.layers.{q}.codebook").cpu().clone() for q in range(6)]
    code_sum, code_count = list(tr.code_sum.cpu().clone()), list(tr.code_count.cpu().clone())
    lat = ref.quantiser_latents(vq_sd, n, t4, seed=3 + step)
    draws = make_draws(n, 4 * t4, None, 50 + step, init, keep=False) if draws is None else draws
    assert [len(z) for z in draws["tile"]] == [((1 if i else 2) if rows < 512 else 0) for i in init]
    out = tr.quantize(lat.to(DEV), to_dev(draws))
    idx = out["idx"].cpu().long()
    assert out["n_active"] == 6 and int(idx.min()) >= 0 and int(idx.max()) < 512 and tr.init == [True] * 6
    x = lat.reshape(-1, 512)
    judged = ref.judge_picks(x, cbs, init, idx, draws["gumbel"], 6)
    off = sum(int((idx[:, q] != j["argmax"]).sum()) for q, j in enumerate(judged))
    share = ref.check_picks(judged, idx)
    want = ref.quantiser_step_ref(lat, cbs, code_sum, code_count, init, draws, idx)
    err_xq = float((out["xq"].cpu() - want["xq"]).abs().max())
    commit, perp = float(out["commit"]), float(out["perplexity"])
    print(f"{rows} rows, step {step}, init {init[0]}: near-tie share {share:.4f}, picks off the fp64 argmax {off} of {idx.numel()}, xq {err_xq:.2e}, "
          f"commit {commit:.6e} (ref {float(want['commit']):.6e}), perplexity {perp:.4f} (ref {float(want['perplexity']):.4f})")
    assert err_xq <= 1e-6
    assert abs(commit - float(want["commit"])) <= 1e-4 and abs(perp - float(want["perplexity"])) <= 1e-3
    inputs, resets = ref.layer_inputs(x, cbs, init, idx, 6), []
    for q in range(6):
        check_state(tr, q, want["codebooks"][q], want["code_sum"][q], want["code_count"][q])
        assert torch.equal(tr._weights["bcount"][q].cpu(), torch.bincount(idx[:, q], minlength=512).float()), q
        reset = tr.code_count[q].cpu() < 1.0
        assert torch.equal(reset, want["code_count"][q] < 1.0), q
        resets.append(int(reset.sum()))
        if rows >= 512:                                                   # a dead code becomes row c of the layer's input, bit for bit: no noise term
            assert torch.equal(tr.model.get_buffer(f"quantizer.layers.{q}.codebook").cpu()[reset], inputs[q][0][:512][reset]), q
    print(f"    codes reset per layer {resets}, most rows on one code {[int(torch.bincount(idx[:, q]).max()) for q in range(6)]}")
    return resets


@pytest.mark.parametrize("rows", list(QUANT_SHAPES))
def test_quantiser_at_workload_row_counts(vq_sd, rows):
    """Two consecutive steps on two latent batches from an initialised EMA state in which a sixth of the codes sit below the usage threshold:
    every layer quantises, updates and resets on both steps, and the second step's resets read rows that are not the codebook."""
    tr = new_trainer(57)
    sd = tr.state_dict()
    sd["code_sum"], sd["code_count"] = ref.initialised_state(vq_sd)
    sd["init"] = [True] * 6
    tr.load_state_dict(sd)
    for step in range(2):
        resets = check_quantiser_step(tr, vq_sd, rows, step)
        assert min(resets) > 50, resets


def test_quantiser_first_step_at_513_rows(vq_sd):
    """The reference's first step at >= 512 rows: layer 0's codebook is the first 512 rows of the batch, so those rows leave zero residuals
    and the later layers initialise from them.  Kept, because it is what training does."""
    tr = new_trainer(57)
    check_quantiser_step(tr, vq_sd, 513, 0)


def test_noise_boundary_and_the_trainers_own_draws(vq_sd):
    """511 rows need `_tile`'s normals - leaving them out raises - and 512 rows take none; `RVQTrainer.draw` at 513 rows returns no normals and
    finite Gumbel noise, on which the quantiser's picks hold up in fp64 as well."""
    assert [len(z) for z in make_draws(7, 4 * 73, None, 1, [True] * 6, keep=False)["tile"]] == [1] * 6
    assert [len(z) for z in make_draws(8, 4 * 64, None, 1, [False] * 6, keep=False)["tile"]] == [0] * 6
    tr = new_trainer(57)
    untouched = tr.model.get_buffer("quantizer.layers.0.codebook").clone()
    draws = make_draws(7, 4 * 73, None, 1, [False] * 6, keep=False)
    draws["tile"] = [[] for _ in range(6)]
    with pytest.raises(ValueError):
        tr.quantize(ref.quantiser_latents(vq_sd, 7, 73, seed=3).to(DEV), to_dev(draws))
    assert tr.init == [False] * 6 and torch.equal(tr.model.get_buffer("quantizer.layers.0.codebook"), untouched)
    n, t4 = QUANT_SHAPES[513]
    own = tr.draw(n, 4 * t4, DEV)
    assert [len(z) for z in own["tile"]] == [0] * 6 and len(own["keep"]) == 12
    assert all(g is None or (tuple(g.shape) == (513, 512) and bool(torch.isfinite(g).all())) for g in own["gumbel"])
    own = {"gumbel": [torch.empty(513, 512, device=DEV).exponential_().log_().neg_().cpu() if g is None else g.cpu() for g in own["gumbel"]],
           "start": None, "tile": own["tile"], "keep": []}               # (a quantise-dropout draw would skip layers: judge all six)
    assert all(bool(torch.isfinite(g).all()) for g in own["gumbel"])
    check_quantiser_step(tr, vq_sd, 513, 0, draws=own)


# ---- 2, 3. forward and backward with injected draws --------------------------------------------------------------------------------------
# the last case is the first shape on the workload's side of `_tile`: 512 latent rows (no noise, resets from the batch's own rows) and
# K = 2048 / 1024 / 512 positions per weight gradient
STEP_CASES = {"n3_t16_dim57": (0, None), "n2_t64_dim78_start2": (1, None), "n2_t32_dim180": (None, (2, 32, 180, "hands", None)),
              "n8_t256_dim57": (None, (8, 256, 57, "lower_trans", None))}


@pytest.fixture(scope="module")
def step_results(fx):
    """One HIP forward + backward and one restatement step (fed the HIP indices) per case, shared by the tests below."""
    out = {}
    for name, (case, shape) in STEP_CASES.items():
        if case is not None:
            n, t, dim = (int(v) for v in fx["cases"][case][:3])
            part, draws = str(fx["parts"][case]), ref.fixture_draws(fx, case, 0)
        else:
            n, t, dim, part, start = shape
            draws = make_draws(n, t, start, 17, [False] * 6)
        pose = synth.synth_vq_pose(part, dim, n=n, t=t, seed=3)
        tr = new_trainer(dim)
        got = tr.forward_backward(pose.to(DEV), to_dev(draws))
        hip = {"rec_pose": got["rec_pose"].cpu(), "idx": got["idx"].cpu().long(), "grads": {k: v.cpu().clone() for k, v in got["grads"].items()},
               "scalars": [float(got[k]) for k in ("loss", "recons", "commit", "perplexity")]}
        used = [int(hip["idx"][:, q].unique().numel()) for q in range(got["n_active"])]
        print(f"{name}: distinct codes per active layer {used}")
        assert min(used) > 1, (name, used)                                # a step whose every row picks one code checks next to nothing
        want = ref.train_step(synth.synth_vq_state_dict(dim), ref.new_state(), pose, draws, forced_idx=hip["idx"])
        out[name] = (hip, want, case)
    return out


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_forward_equals_the_restatement(fx, step_results, name):
    hip, want, case = step_results[name]
    if case is not None:
        assert np.array_equal(hip["idx"].numpy(), fx[f"c{case}.s0.idx"])  # on the fixture's cases the HIP indices are the reference's
    err = rel_l2(hip["rec_pose"], want["rec_pose"])
    print(f"{name}: rec_pose rel-L2 {err:.3e}; loss/recons/commit/perplexity {hip['scalars']} vs {[float(want[k]) for k in ('loss', 'recons', 'commit', 'perplexity')]}")
    assert err <= 2e-2
    assert abs(hip["scalars"][1] - float(want["recons"])) <= 2e-2 * float(want["recons"])
    assert abs(hip["scalars"][2] - float(want["commit"])) <= 1e-4 and abs(hip["scalars"][3] - float(want["perplexity"])) <= 1e-3
    assert abs(hip["scalars"][0] - (hip["scalars"][1] + 0.02 * hip["scalars"][2])) <= 1e-6 * max(1.0, hip["scalars"][0])


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_backward_equals_the_restatements_autograd(step_results, name):
    hip, want, _ = step_results[name]
    assert sorted(hip["grads"]) == sorted(want["grads"])
    errs = {k: rel_l2(hip["grads"][k], want["grads"][k]) for k in want["grads"]}
    worst = max(errs, key=errs.get)
    print(f"{name}: worst gradient rel-L2 {errs[worst]:.3e} ({worst}); last conv {errs['decoder.model.6.weight']:.3e}, first conv {errs['encoder.model.0.weight']:.3e}")
    assert errs[worst] < 3e-2, {k: v for k, v in errs.items() if v >= 3e-2}


def test_plain_bf16_forward_stays_available_as_a_diagnostic(step_results):
    """forward_products=1 (scripts/diag_rvq_train_forward.py): the forward alone still meets the eval path's bound; its gradients are what the
    default's two extra products are for and are not held to the gate here."""
    hip, want, _ = step_results["n2_t32_dim180"]
    draws = make_draws(2, 32, None, 17, [False] * 6)
    got = new_trainer(180, forward_products=1).forward_backward(synth.synth_vq_pose("hands", 180, n=2, t=32, seed=3).to(DEV), to_dev(draws), forward_only=True)
    single, triple = rel_l2(got["rec_pose"], want["rec_pose"]), rel_l2(hip["rec_pose"], want["rec_pose"])
    print(f"rec_pose rel-L2: {single:.3e} with one product, {triple:.3e} with three")
    assert triple < single <= 2e-2
    with pytest.raises(ValueError):
        new_trainer(57, forward_products=2)


@pytest.mark.parametrize("kind", ["l1", "l1_smooth"])
def test_other_reconstruction_losses(kind):
    """L1 and SmoothL1 (rvq_beatx_train.py:57-62): the loss value and the gradient of the last convolution, which is the loss gradient times h."""
    n, t, dim = 2, 16, 57
    pose, draws = 3.0 * synth.synth_vq_pose("lower", dim, n=n, t=t, seed=5), make_draws(2, 16, None, 23, [False] * 6)     # |diff| on both sides of 1
    got = new_trainer(dim, recons_loss=kind).forward_backward(pose.to(DEV), to_dev(draws))
    want = ref.train_step(synth.synth_vq_state_dict(dim), ref.new_state(), pose, draws, forced_idx=got["idx"].cpu().long(), recons=kind)
    assert abs(float(got["recons"]) - float(want["recons"])) <= 1e-3 * float(want["recons"])
    for k in ("decoder.model.6.weight", "decoder.model.6.bias", "encoder.model.0.weight"):
        assert rel_l2(got["grads"][k].cpu(), want["grads"][k]) < 3e-2, k


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_runs_with_the_same_draws_are_bit_equal():
    n, t, dim = 3, 16, 57
    runs = []
    for _ in range(2):
        tr = new_trainer(dim, warm_up_iter=0)
        losses = []
        for s in range(2):
            draws = make_draws(n, t, None if s == 0 else 3, 31 + s, tr.init)
            out = tr.step(synth.synth_vq_pose("lower", dim, n=n, t=t, seed=3 + s).to(DEV), to_dev(draws))
            losses += [out[k].clone() for k in ("loss", "recons", "commit", "perplexity")]
        runs.append((losses, [v.clone() for v in tr.model.state_dict().values()], tr.code_sum.clone(), tr.code_count.clone()))
    a, b = runs
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert all(bool(torch.isfinite(x)) for x in a[0])


# ---- 5. the eval-mode model sees the trained weights; the checkpoint is the reference's ----------------------------------------------------
def test_model_follows_the_steps_and_save_net_round_trips(tmp_path):
    n, t, dim = 2, 32, 78
    tr = new_trainer(dim, warm_up_iter=0, seed=3)
    pose = synth.synth_vq_pose("upper", dim, n=n, t=t, seed=3).to(DEV)
    before = tr.model.map2latent(pose).clone()                           # packs the initial weights: the steps must invalidate that cache
    torch.manual_seed(7)
    for _ in range(3):
        tr.step(pose)
    assert tr.iteration == 3
    path = str(tmp_path / "net_last.pth")
    tr.save_net(path)
    ckpt = torch.load(path, map_location="cpu")
    keys = [str(k) for k in np.load(os.path.join(GOLDEN, "vq_outputs.npz"))["upper.state_keys"]]
    assert list(ckpt) == ["net"] and [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in ckpt["net"].items()] == keys
    fresh = rvqvae.build(dim)
    fresh.load_state_dict(ckpt["net"])
    fresh = fresh.to(DEV)
    lat = tr.model.map2latent(pose)
    assert not torch.equal(lat, before)
    assert torch.equal(lat, fresh.map2latent(pose))
    for a, b in zip(tr.model.latent2origin(lat), fresh.latent2origin(lat)):
        assert torch.equal(a, b)
    # the trainer's own state restores the EMA state and the init flags (a `net` checkpoint alone re-initialises the codebooks)
    other = rvq_training.RVQTrainer(rvqvae.build(dim).to(DEV))
    other.load_state_dict(tr.state_dict())
    assert other.init == tr.init and other.iteration == 3 and torch.equal(other.code_sum, tr.code_sum) and torch.equal(other.code_count, tr.code_count)


def test_adam_moments_survive_a_move_of_the_parameters():
    """model.to(...) re-allocates the parameters: the trainer rebuilds its pointer tables and optimiser, and must carry the moments across."""
    n, t, dim = 2, 16, 57
    tr = new_trainer(dim, warm_up_iter=0)
    pose = synth.synth_vq_pose("lower", dim, n=n, t=t, seed=3).to(DEV)
    tr.step(pose, to_dev(make_draws(n, t, None, 41, tr.init)))
    p = tr.model.get_parameter("decoder.model.6.weight")
    before = {k: v.clone() for k, v in tr._opt.state[p].items()}
    ptr = p.data_ptr()
    tr.model.to("cpu")
    tr.model.to(DEV)
    assert p.data_ptr() != ptr
    tr.step(pose, to_dev(make_draws(n, t, None, 42, tr.init)))
    after = tr._opt.state[p]
    assert float(after["step"]) == 2.0 and float(before["step"]) == 1.0
    assert float(before["exp_avg"].abs().max()) > 0 and not torch.equal(after["exp_avg"], before["exp_avg"])
    # the second step's first moment is 0.9 * the first's + 0.1 * the new gradient: the old moment is in it
    want = 0.9 * before["exp_avg"] + 0.1 * p.grad
    assert float((after["exp_avg"] - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-12


# ---- 6. it learns as the reference does ---------------------------------------------------------------------------------------------------
def test_hundred_steps_learn_like_the_reference():
    """100 steps at the fixture's --loop shape from the same initial weights on the same batches: recons(100) / recons(1) must not exceed the
    LARGEST such ratio of the reference's seeds (tests/golden/rvq_train_loop.npz) times 1.25 - the margin for bf16 operands in the backward and
    a different noise stream (the reference's own ratios differ by 2.5 % between seeds)."""
    loop = np.load(os.path.join(GOLDEN, "rvq_train_loop.npz"))
    n, t, dim, steps = (int(v) for v in loop["shape"])
    ratios = loop["recons_last"] / loop["recons_first"]
    assert ratios.max() / ratios.min() <= 1.25                           # else: widen the fixture to five seeds (never the factor)
    tr = new_trainer(dim, warm_up_iter=0, seed=1)
    torch.manual_seed(1)
    recons = []
    for it in range(steps):
        recons.append(tr.step(synth.synth_vq_motion(n, t, dim, step=it).to(DEV))["recons"])
    first, last = float(recons[0]), float(recons[-1])
    print(f"recons {first:.5f} -> {last:.5f}: ratio {last / first:.4f}; reference ratios {ratios}, bound {ratios.max() * 1.25:.4f}")
    assert abs(first - float(loop["recons_first"].mean())) <= 0.10 * first    # same weights, same batch: only the noise draws differ (the reference's own seeds spread by 3 %)
    assert last / first <= float(ratios.max()) * 1.25
