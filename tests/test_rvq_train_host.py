"""Codec training, host side: the torch restatement of the train-mode step (tests/rvq_train_ref.py) against the reference's own outputs
(tests/golden/rvq_train_step*.npz), the new C ABI entry points, the learning-rate schedule and the surface of RVQTrainer.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, rvq_training, rvqvae, synth
from tests import rvq_train_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture(GOLDEN)


def run_case(fx, case, forced=None):
    """The restatement over every step of a fixture case; yields (step, result, quantiser state)."""
    n, t, dim, _, steps = (int(v) for v in fx["cases"][case])
    sd = synth.synth_vq_state_dict(dim)
    st = ref.new_state()
    for s in range(steps):
        pose = synth.synth_vq_pose(str(fx["parts"][case]), dim, n=n, t=t, seed=3 + s)
        out = ref.train_step(sd, st, pose, ref.fixture_draws(fx, case, s), forced_idx=None if forced is None else forced[s], with_grads=s == 0)
        for q in range(ref.NUM_Q):
            sd[f"quantizer.layers.{q}.codebook"] = out["codebooks"][q]
        yield s, out, st


@pytest.mark.parametrize("case", [0, 1])
def test_restatement_equals_the_reference(fx, case):
    """Indices exact; loss, recons and commit within 1e-5 absolute, perplexity within 1e-5 relative; codebook state within 1e-5; gradient samples and
    norms within 1e-4 (of the tensor's largest sample / of the norm)."""
    for s, out, st in run_case(fx, case):
        pre = f"c{case}.s{s}."
        assert np.array_equal(out["idx"].numpy(), fx[pre + "idx"])
        got = np.array([float(out[k]) for k in ("loss", "recons", "commit", "perplexity")])
        want = fx[pre + "scalars"].astype(np.float64)
        assert np.abs(got[:3] - want[:3]).max() <= 1e-5, (got, want)                  # loss, recons, commit: absolute
        assert abs(got[3] - want[3]) <= 1e-5 * want[3], (got, want)                  # perplexity (12 .. 31): relative
        assert np.abs(out["latent"].numpy() - fx[pre + "latent"]).max() <= 1e-5
        assert np.abs(out["xq"].numpy() - fx[pre + "xq"]).max() <= 1e-5
        assert np.abs(out["rec_pose"].numpy() - fx[pre + "rec_pose"]).max() <= 1e-5
        for q in range(out["n_active"]):
            for name, tns in (("codebook", out["codebooks"][q]), ("code_sum", st["code_sum"][q])):
                nrm, smp = ref.sample(tns)
                assert np.abs(smp.numpy() - fx[pre + f"{name}{q}.sample"]).max() <= 1e-5, (name, q)
                assert abs(nrm - float(fx[pre + f"{name}{q}.norm"])) <= 1e-5 * max(1.0, nrm), (name, q)
            assert np.abs(st["code_count"][q].numpy() - fx[pre + f"code_count{q}"]).max() <= 1e-5
        assert not any(st["init"][out["n_active"]:]) and all(st["init"][:out["n_active"]])      # a skipped layer stays uninitialised
        if s == 0:
            g = f"c{case}.grad."
            names, off = [str(k) for k in fx[g + "names"]], fx[g + "offsets"]
            assert sorted(names) == sorted(out["grads"])
            for i, k in enumerate(names):
                nrm, smp = ref.sample(out["grads"][k])
                want = fx[g + "samples"][off[i]:off[i + 1]]
                assert np.abs(smp.numpy() - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-30), k
                assert abs(nrm - float(fx[g + "norms"][i])) <= 1e-4 * float(fx[g + "norms"][i]), k


def test_fixture_covers_what_it_is_for(fx):
    """Both quantise-dropout branches, the first-step initialisation, a reset of dead codes on an initialised codebook, `_tile`'s noise branch."""
    assert [int(v) for v in fx["cases"][0]] == [3, 16, 57, -1, 2] and [int(v) for v in fx["cases"][1]] == [2, 64, 78, 2, 1]
    assert fx["c0.s0.gumbel"].shape == (6, 12, 512) and fx["c1.s0.gumbel"].shape == (3, 32, 512)
    assert (fx["c1.s0.idx"][:, 3:] == -1).all() and (fx["c1.s0.idx"][:, :3] >= 0).all()
    assert (fx["c0.s0.tile_calls"] >= 0).all() and (fx["c0.s1.tile_calls"][:, 1] == -1).all()     # init + update draws, then update only
    assert (fx["c0.s1.code_count0"] < 1.0).sum() > 0                                                # dead codes: replaced in step 2
    for f in ref.FIXTURE_FILES:                                           # the generator's own budget (its docstring): four small files, each under 1 MiB
        assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f


def test_forced_indices_replace_the_argmax(fx):
    forced = [torch.from_numpy(fx[f"c1.s0.idx"])]
    s, out, _ = next(run_case(fx, 1, forced))
    assert np.array_equal(out["idx"].numpy(), fx["c1.s0.idx"]) and abs(float(out["loss"]) - float(fx["c1.s0.scalars"][0])) <= 1e-6
    other = forced[0].clone()
    other[:, 0] = (other[:, 0] + 1) % 512
    s, out2, _ = next(run_case(fx, 1, [other]))
    assert np.array_equal(out2["idx"].numpy(), other.numpy()) and float(out2["commit"]) > float(out["commit"])


def test_learning_rate_schedule_is_the_reference_loop():
    """rvq_beatx_train.py:333-381 run on a dummy parameter: warm-up by update_lr_warm_up, then MultiStepLR (which continues from the last warm-up value)."""
    for warm, milestones in ((5, (3, 6)), (1, (2, 4)), (0, (2,))):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.AdamW([p], lr=2e-4, betas=(0.9, 0.99), weight_decay=0.0)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(milestones), gamma=0.05)
        seen = []
        for nb_iter in range(1, warm):
            for g in opt.param_groups:
                g["lr"] = 2e-4 * (nb_iter + 1) / (warm + 1)
            seen.append(opt.param_groups[0]["lr"])
        for nb_iter in range(1, 9):
            seen.append(opt.param_groups[0]["lr"])
            p.grad = torch.zeros(1)
            opt.step()
            sched.step()
        got = [rvq_training.lr_at(i, 2e-4, warm, milestones, 0.05) for i in range(len(seen))]
        assert np.allclose(got, seen, rtol=1e-12, atol=0), (warm, got, seen)
        assert np.allclose(got, [ref.lr_at(i, 2e-4, warm, milestones, 0.05) for i in range(len(seen))], rtol=1e-12, atol=0)


def test_new_exports_are_declared_bound_and_present():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int32_t|int64_t)\s+(syn_vq_train_[a-z_0-9]+)\s*\(", header, flags=re.M))
    assert declared == set(rvq_training.ENTRY_POINTS) and declared <= set(_lib.EXPORTS), declared ^ set(rvq_training.ENTRY_POINTS)
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.syn_version() == 9


def test_training_is_a_separate_object():
    model = rvqvae.build(57)
    with pytest.raises(NotImplementedError):
        model.train()
    with pytest.raises(NotImplementedError):
        rvq_training.RVQTrainer(model, weight_decay=0.01)
    with pytest.raises(ValueError):
        rvq_training.RVQTrainer(model, recons_loss="huber")
    with pytest.raises(_lib.SynHipError):
        rvq_training.RVQTrainer(model).step(torch.zeros(2, 16, 57))      # CPU tensors: no fallback
    assert not model.training


def test_trainer_state_dict_round_trip_on_the_host():
    """state_dict carries the model's reference-keyed state, the quantiser's EMA state and init flags, the optimiser moments and the iteration."""
    model = rvqvae.build(57)
    model.load_state_dict(synth.synth_vq_state_dict(57))
    tr = rvq_training.RVQTrainer(model, seed=5)
    sd = tr.state_dict()
    assert set(sd) == {"net", "code_sum", "code_count", "init", "optimizer", "iteration", "coin"}
    assert list(sd["net"]) == list(model.state_dict()) and sd["init"] == [False] * 6 and sd["iteration"] == 0
    sd["init"], sd["iteration"] = [True, True, False, False, False, False], 7
    sd["code_count"] = torch.full((6, 512), 2.0)
    other = rvq_training.RVQTrainer(rvqvae.build(57))
    other.load_state_dict(sd)
    assert other.iteration == 7 and other.init == sd["init"] and torch.equal(other.code_count.cpu(), sd["code_count"])
    assert all(torch.equal(a, b) for a, b in zip(other.model.state_dict().values(), model.state_dict().values()))
    assert [other.quantize_dropout_start() for _ in range(20)] == [tr.quantize_dropout_start() for _ in range(20)]     # the coin's generator travels too


def test_body_part_masks_have_the_reference_widths():
    """dim_pose of every branch of rvq_beatx_train.py:210-295, and a few channels written out from it."""
    widths = {("upper", "beatx"): 78, ("hands", "beatx"): 180, ("lower", "beatx"): 54, ("lower_trans", "beatx"): 57, ("whole_trans", "beatx"): 315,
              ("upper", "h3d_623"): 156, ("hands", "h3d_623"): 360, ("lower_trans", "h3d_623"): 107, ("lower", "h3d_623"): 54}
    for (part, data), dim in widths.items():
        m = rvq_training.body_part_mask(part, data)
        assert len(m) == dim == len(set(m)), (part, data)
    assert rvq_training.body_part_mask("upper")[:7] == [18, 19, 20, 21, 22, 23, 36]
    assert rvq_training.body_part_mask("lower_trans")[-4:] == [71, 330, 331, 332]
    h = rvq_training.body_part_mask("upper", "h3d_623")
    assert h[:12] == [10, 11, 12, 4 + 153 + 12, 4 + 153 + 13, 4 + 153 + 14, 4 + 153 + 15, 4 + 153 + 16, 4 + 153 + 17, 4 + 459 + 9, 4 + 459 + 10, 4 + 459 + 11]
    lt = rvq_training.body_part_mask("lower_trans", "h3d_623")
    assert lt[:8] == [0, 1, 2, 3, 619, 620, 621, 622] and lt[8:11] == [4 + 459, 4 + 459 + 1, 4 + 459 + 2]      # joint 0: velocity only
    with pytest.raises(ValueError):
        rvq_training.body_part_mask("whole")


# ---- the draws the GPU suite injects, and how sharp its comparisons are ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 32, None), (3, 16, None)])
def test_made_draws_are_gumbel_noise_and_spread_the_picks(shape):
    """`make_draws` once wrote -log(-log(u).clamp_min(1e-20)): the clamp bound to log(u) <= 0, every element came out NaN, argmax picked code 0
    for every row of every layer and the kernel agreed.  Gumbel noise is finite and has mean 0.5772 (Euler's constant; an (N T / 4) x 512
    draw has a standard error below 0.02), and a step on it uses more than one code in every active layer."""
    n, t, start = shape
    draws = ref.make_draws(n, t, start, 17, [False] * 6)
    for g in draws["gumbel"]:
        assert g.shape == (n * t // 4, 512) and bool(torch.isfinite(g).all())
        assert abs(float(g.double().mean()) - 0.5772) <= 0.05
    assert [len(z) for z in draws["tile"]] == [2] * 6 and [tuple(k.shape) for k in draws["keep"][:4]] == [(n, 512, t // 2)] * 3 + [(n, 512, t // 4)]
    out = ref.train_step(synth.synth_vq_state_dict(57), ref.new_state(), synth.synth_vq_pose("lower", 57, n=n, t=t, seed=3), draws, with_grads=False)
    used = [int(out["idx"][:, q].unique().numel()) for q in range(out["n_active"])]
    print(f"{shape}: distinct codes per layer {used}")
    assert out["n_active"] == 6 and min(used) > 1, used


def test_wgrad_comparison_sees_each_wrong_read():
    """tests/test_gpu_rvq_train_kernels.py holds k_wgrad to 2 K 2^-24 sum |dy x| per element against fp64 on WGRAD_CASES.  Four wrong kernels,
    applied to that fp64 reference instead of being built: a tap shift that ignores the dilation, a read that ignores the clip boundary, a
    dropped `>> up`, a partial chunk's last position left out.  Every case a mutation can touch must put some element over its bound; the
    distances, in units of the bound, are in DESIGN.md 16.5."""
    def strays(case):
        """Some shifted read leaves its clip and still lands inside the buffer (one-frame clips under dilation 9 leave the buffer altogether)."""
        taps, stride, dil, pad, up, _ = ref.WGRAD_GEOMETRY[case[0]]
        clips, t_out = case[5], case[6]
        t_in = t_out * stride if not up else t_out // 2
        return any(not 0 <= t * stride + tap * dil - pad < (t_in << up) and 0 <= n * t_in + ((t * stride + tap * dil - pad) >> up) < clips * t_in
                   for n in range(clips) for t in range(t_out) for tap in range(taps))

    touches = {"dilation": lambda c: ref.WGRAD_GEOMETRY[c[0]][2] > 1, "clip": strays,
               "up": lambda c: ref.WGRAD_GEOMETRY[c[0]][4] == 1, "last": lambda c: c[5] * c[6] % 64 != 0}
    worst, seen = {m: float("inf") for m in touches}, {m: set() for m in touches}
    for case in ref.WGRAD_CASES:
        geo, cout, _, cin, _, clips, t_out = case
        if cout * cin * clips * t_out > 128 * 192 * 130:                  # the 512-channel twins of a small case add nothing here
            continue
        dy, x, _ = ref.wgrad_operands(case)
        args = (dy[..., :cout], x[..., :cin]) + ref.WGRAD_GEOMETRY[geo]
        want, mag, _, _ = ref.wgrad_ref(*args)
        bound = ref.wgrad_bound(mag, clips * t_out)
        for m, applies in touches.items():
            if not applies(case):
                continue
            got = ref.wgrad_ref(*args, mutate=m)[0]
            over = (got - want).abs() > bound
            assert bool(over.any()), (m, case)
            ratio = float(((got - want).abs()[over] / bound[over].clamp_min(1e-300)).max())
            worst[m], _ = min(worst[m], ratio), seen[m].add(geo)
    print("smallest of the per-case largest |mutant - right| / bound:", {m: f"{v:.3g}" for m, v in worst.items()})
    assert seen["dilation"] == {"dil3", "dil9"} and seen["up"] == {"up"} and seen["clip"] == set(ref.WGRAD_GEOMETRY) - {"k1"}
    assert seen["last"] == set(ref.WGRAD_GEOMETRY)                        # every geometry meets a partial last chunk
    for geo in ref.WGRAD_GEOMETRY:                                        # ... an odd K (`up` has an even t_out) and several chunks with a partial tail
        ks = {c[5] * c[6] for c in ref.WGRAD_CASES if c[0] == geo}
        assert any(k > 64 and k % 64 for k in ks) and (geo == "up" or any(k % 2 for k in ks)), (geo, ks)
    # dilation 9 on clips of one frame: every off-centre tap reads padding, the gradient there is exactly zero with a zero bound
    case = next(c for c in ref.WGRAD_CASES if c[0] == "dil9" and c[6] == 1)
    dy, x, _ = ref.wgrad_operands(case)
    want, mag, _, _ = ref.wgrad_ref(dy[..., :case[1]], x[..., :case[3]], *ref.WGRAD_GEOMETRY["dil9"])
    assert float(mag[:, :, [0, 2]].max()) == 0.0 and float(want[:, :, [0, 2]].abs().max()) == 0.0 and float(mag[:, :, 1].median()) > 0.0


def test_code_update_comparison_sees_a_lost_chunk_and_stray_noise():
    """The quantiser tests at 512 rows and more hold code_sum / code_count / codebook to 1e-5 and the reset rows to bit equality.  Two wrong
    kernels, applied to the restatement: the second 256-row chunk of the per-code sums left out, `_tile`'s noise added to the reset rows."""
    sd = synth.synth_vq_state_dict(57)
    cbs = [sd[f"quantizer.layers.{q}.codebook"].float() for q in range(6)]
    code_sum, code_count = ref.initialised_state(sd)
    lat = ref.quantiser_latents(sd, 9, 57, seed=3)
    draws = ref.make_draws(9, 4 * 57, None, 50, [True] * 6, keep=False)
    idx = ref.residual_vq([c.clone() for c in cbs], {"init": [True] * 6, "code_sum": list(code_sum.clone()), "code_count": list(code_count.clone())},
                          lat.permute(0, 2, 1).clone(), draws)[1]
    run = lambda m: ref.quantiser_step_ref(lat, cbs, list(code_sum), list(code_count), [True] * 6, draws, idx, mutate=m)
    want, same, chunk, noise = run(None), run("same"), run("second_chunk"), run("noise")
    dist = lambda a, k: min(float((a[k][q] - want[k][q]).abs().max()) for q in range(6)) / 1e-5
    assert max(dist(same, k) for k in ("codebooks", "code_sum", "code_count")) == 0.0     # the re-written update IS the restatement's
    print("in units of the 1e-5 bound, smallest over the layers: lost chunk", {k: f"{dist(chunk, k):.3g}" for k in ("code_sum", "code_count")},
          "stray noise", f"{dist(noise, 'codebooks'):.3g}")
    assert dist(chunk, "code_sum") > 1 and dist(chunk, "code_count") > 1 and dist(noise, "codebooks") > 1
    for q in range(6):
        reset = want["code_count"][q] < 1
        x = ref.layer_inputs(lat.reshape(-1, 512), cbs, [True] * 6, idx, 6)[q][0]
        assert int(reset.sum()) > 50 and torch.equal(want["codebooks"][q][reset], x[:512][reset]) and not torch.equal(noise["codebooks"][q][reset], x[:512][reset])
