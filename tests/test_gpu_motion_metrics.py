"""Motion metrics on the device (csrc/syn_joints.inc; syntalker_amd/joints.py, metrics.py) against tests/golden/motion_metrics.npz - what the
reference's own code returned - and the fp64 restatements of tests/motion_metrics_ref.py, which test_motion_metrics_host.py pins to it.

Gates.  FK and speeds: the same chain in plain fp32 on the CPU has a max abs error E against the fp64 oracle on the case's own inputs; the
device may be 4 E away (another product order, its own sincos).  Beats: identical masks - the fixture's margins (make_motion_metrics_golden.py)
make that a fair demand.  BC: 1e-5 absolute (terms in [0, 1], beat times exact multiples of 1 / 30, expf good to ~1e-7).  L1div: relative
max(4 R, 1e-6), R the reference's own float32 result against fp64.  recover_from_ric: 4 x the reference's own fp32-against-fp64 error."""
import os

import numpy as np
import pytest
import torch

from tests import motion_metrics_ref as mr
from tests.conftest import GOLDEN

from syntalker_amd import joints, metrics, poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "motion_metrics.npz")))


@pytest.fixture(scope="module")
def skel(gold):
    return joints.Skeleton(mr.smplx_parents(), gold["take.rest"])


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def fk_case(parents, rest, rot, transl=None, label=""):
    """Device FK of one take against the fp64 oracle at 4 E.  Returns (device joints, E)."""
    want = mr.fk_oracle(parents, rest, rot, transl)
    e = float(np.abs(mr.fk_torch32(parents, rest, rot, transl) - want).max())
    got = joints.forward_kinematics(joints.Skeleton(parents, rest), dev(rot), None if transl is None else dev(transl)).cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"fk {label}: N = {len(rot)}, E = {e:.3e}, device error = {err:.3e}, gate = {4 * e:.3e}")
    assert got.shape == want.shape and err <= 4 * e, (label, err, e)
    return got, e


# ---- forward kinematics ---------------------------------------------------------------------------------------------------------------
def test_fk_smplx_tree_against_the_fp64_oracle(gold):
    par, rest, aa, tr = mr.smplx_parents(), gold["take.rest"], gold["take.aa"], gold["take.transl"]
    fk_case(par, rest, aa, tr, "fixture take, transl")
    fk_case(par, rest, aa, None, "fixture take")
    fk_case(par, rest, aa[:1], tr[:1], "one frame")
    fk_case(par, rest, aa[:joints.FK_FRAME_TILE + 1], None, "one frame past the tile")
    big = mr.smooth_rotations(5, 37, amp=2.5)                       # angles up to ~ 2 rad, several workgroups, a ragged last tile
    fk_case(par, rest, big, None, "large angles")


def test_fk_three_joint_chain_with_hand_computed_positions():
    par, rest = np.array([-1, 0, 1]), np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float32)
    rot = np.zeros((1, 3, 3), dtype=np.float32)
    rot[0, 0, 2] = rot[0, 1, 2] = np.float32(np.pi / 2)            # a quarter turn about z at the root and at joint 1
    rot[0, 2] = [0.3, -0.2, 0.1]                                    # the last joint's own rotation moves nothing
    hand = np.array([[[0, 0, 0], [0, 1, 0], [-1, 1, 0]]], dtype=np.float64)
    assert np.abs(mr.fk_oracle(par, rest, rot) - hand).max() < 1e-7  # (pi / 2 is rounded to float32 before the oracle sees it)
    got, e = fk_case(par, rest, rot, None, "3-joint chain")
    assert np.abs(got - hand).max() <= 4 * e + 1e-7
    tr = np.array([[0.5, -1.0, 2.0]], dtype=np.float32)
    got, e = fk_case(par, rest, rot, tr, "3-joint chain, transl")
    assert np.abs(got - (hand + tr[:, None])).max() <= 4 * e + 1e-7


def test_fk_zero_rotation_and_angles_next_to_pi(gold):
    par, rest = mr.smplx_parents(), gold["take.rest"]
    zero = np.zeros((3, 55, 3), dtype=np.float32)
    got, _ = fk_case(par, rest, zero, None, "rotation exactly 0")
    assert np.abs(got - rest[None]).max() <= 1e-6                    # the rest pose itself (sums of offsets, no rotation error at all)
    mixed = gold["take.aa"][:5].copy()
    mixed[:, ::3] = 0                                               # exact zeros among ordinary rotations
    fk_case(par, rest, mixed, None, "some rotations exactly 0")
    r = np.random.RandomState(8)
    axis = r.randn(4, 55, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    near_pi = (axis * (np.pi - r.uniform(0, 1e-3, (4, 55, 1)))).astype(np.float32)
    fk_case(par, rest, near_pi, None, "angles within 1e-3 of pi")
    tiny = (axis * r.uniform(1e-6, 3e-4, (4, 55, 1))).astype(np.float32)      # either side of the small-angle branch
    fk_case(par, rest, tiny, None, "tiny angles")


def test_fk_two_takes_with_their_own_rest_joints_in_one_launch(gold):
    par = mr.smplx_parents()
    rest2 = np.stack([gold["take.rest"], mr.synth_rest(7)])
    n = joints.FK_FRAME_TILE + 1                                    # the takes' boundary falls inside a workgroup's tile
    aa = gold["take.aa"][:2 * n]
    sk = joints.Skeleton(par, rest2)
    want = np.concatenate([mr.fk_oracle(par, rest2[0], aa[:n]), mr.fk_oracle(par, rest2[1], aa[n:])])
    e = max(float(np.abs(mr.fk_torch32(par, rest2[k], aa[k * n:(k + 1) * n]) - want[k * n:(k + 1) * n]).max()) for k in range(2))
    got = joints.forward_kinematics(sk, dev(aa)).cpu().numpy()
    assert np.abs(got - want).max() <= 4 * e
    tof = np.arange(2 * n) % 2                                       # and with an explicit, interleaved frame-to-take index
    want_i = mr.fk_oracle(par, rest2, aa, take_of_frame=tof)
    got_i = joints.forward_kinematics(sk, dev(aa), take_of_frame=torch.from_numpy(tof).to(DEV)).cpu().numpy()
    assert np.abs(got_i - want_i).max() <= 4 * e
    assert np.abs(want_i[0] - want_i[1]).max() > 1e-2                # (the two rest sets do differ)
    bad = joints.forward_kinematics(sk, dev(aa[:2]), take_of_frame=torch.tensor([0, 5], device=DEV)).cpu().numpy()
    assert np.isfinite(bad[0]).all() and np.isnan(bad[1]).all()     # a take outside the table: NaN, nothing read


def test_fk_axis_angle_and_6d_inputs_agree(gold, skel):
    par, rest, aa = mr.smplx_parents(), gold["take.rest"], gold["take.aa"][:20]
    d6 = poses.axis_angle_to_rotation_6d(dev(aa))
    want = mr.fk_oracle(par, rest, aa)
    e_aa = float(np.abs(mr.fk_torch32(par, rest, aa) - want).max())
    e_6d = float(np.abs(mr.fk_torch32(par, rest, d6.cpu().numpy()) - want).max())       # includes the conversion's own rounding
    got_aa = joints.forward_kinematics(skel, dev(aa)).cpu().numpy()
    got_6d = joints.forward_kinematics(skel, d6).cpu().numpy()
    print(f"fk 6D: E_aa = {e_aa:.3e}, E_6d = {e_6d:.3e}, |aa - oracle| = {np.abs(got_aa - want).max():.3e}, |6d - oracle| = {np.abs(got_6d - want).max():.3e}")
    assert np.abs(got_6d - want).max() <= 4 * e_6d and np.abs(got_aa - want).max() <= 4 * e_aa
    assert np.abs(got_6d - got_aa).max() <= 4 * (e_aa + e_6d)
    # the 6D oracle on the very same 6D numbers, unnormalised: Gram-Schmidt is part of the kernel
    raw = (d6.cpu().numpy() * np.random.RandomState(2).uniform(0.5, 2.0, (20, 55, 1))).astype(np.float32)
    fk_case(par, rest, raw, None, "6D, unnormalised")
    # smplx_joints: (n, 165) and (n, 330) in, (n, 165) out
    flat = joints.smplx_joints(skel, dev(aa).reshape(20, 165))
    assert flat.shape == (20, 165) and torch.equal(flat, torch.from_numpy(got_aa).to(DEV).reshape(20, 165))
    assert torch.equal(joints.smplx_joints(skel, d6.reshape(1, 20, 330)), torch.from_numpy(got_6d).to(DEV).reshape(20, 165))


def test_fk_hand_mean_pose_moves_the_hands_as_the_oracle_says(gold, skel):
    """SMPL-X adds the model's hand mean pose to the axis-angle vectors of joints 25..54 (`full_pose += pose_mean`, flat_hand_mean=False): the
    oracle is FK of (pose + mean).  Joints upstream of the hands do not move; 6D input goes through axis-angle first, as in test()."""
    par, rest, aa = mr.smplx_parents(), gold["take.rest"], gold["take.aa"][:joints.FK_FRAME_TILE + 3]
    mean = np.zeros((55, 3), dtype=np.float32)
    mean[25:] = (np.random.RandomState(21).randn(30, 3) * 0.25).astype(np.float32)
    sk = joints.Skeleton(par, rest, pose_mean=mean)
    want = mr.fk_oracle(par, rest, aa.astype(np.float64) + mean)
    e = float(np.abs(mr.fk_torch32(par, rest, aa + mean) - want).max())
    plain = joints.forward_kinematics(skel, dev(aa)).cpu().numpy()
    got = joints.forward_kinematics(sk, dev(aa)).cpu().numpy()
    print(f"fk hand mean: E = {e:.3e}, device error = {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= 4 * e
    assert np.array_equal(got[:, :25], plain[:, :25])                # body, jaw and eyes do not move (bitwise: the same arithmetic)
    assert np.abs(got[:, 25:] - plain[:, 25:]).max() > 1e-3          # the fingers do
    assert np.abs(plain - mr.fk_oracle(par, rest, aa)).max() < np.abs(plain - want).max()          # (and the two oracles are told apart)
    d6 = poses.axis_angle_to_rotation_6d(dev(aa))                    # 6D in: to axis-angle, plus the mean, as test() :621-622 + smplx
    back = poses.rotation_6d_to_axis_angle(d6).cpu().numpy()
    e6 = float(np.abs(mr.fk_torch32(par, rest, back + mean) - want).max())      # includes the round trip's own rounding
    got6 = joints.smplx_joints(sk, d6.reshape(-1, 330)).cpu().numpy().reshape(-1, 55, 3)
    assert np.abs(got6 - want).max() <= 4 * e6
    zero = joints.Skeleton(par, rest, pose_mean=np.zeros((55, 3)))   # flat_hand_mean=True: exactly the plain result
    assert zero.pose_mean is None and np.array_equal(joints.forward_kinematics(zero, dev(aa)).cpu().numpy(), plain)


# ---- speeds ---------------------------------------------------------------------------------------------------------------------------
def test_joint_speeds_against_the_fixture(gold):
    g, fps = gold, int(gold["take.fps"])
    for key, rows in (("take.vel", len(g["take.joints"])), ("take2.vel", 2)):            # n = 2: the least the differences allow
        x, want = g["take.joints"][:rows], g[key]
        e = float(np.abs(mr.speeds_ref(x, fps, g["take.mmae"], dtype=np.float32) - want).max())
        got = joints.joint_speed(dev(x), fps, g["take.mmae"]).cpu().numpy()
        err = float(np.abs(got - want).max())
        print(f"speeds {key}: E = {e:.3e}, device error = {err:.3e}")
        assert got.shape == want.shape and err <= 4 * e
    plain = mr.speeds_ref(g["take.joints"], fps)
    e = float(np.abs(mr.speeds_ref(g["take.joints"], fps, dtype=np.float32) - plain).max())
    x = dev(g["take.joints"])
    assert np.abs(joints.joint_speed(x.reshape(-1, 55, 3), fps).cpu().numpy() - plain).max() <= 4 * e
    assert np.abs(joints.mean_joint_speed(x, fps).cpu().numpy() - plain.mean(0)).max() <= 4 * e
    two = joints.joint_speed(torch.stack([x[:40], x[40:]]).reshape(2, 40, 55, 3), fps).cpu().numpy()     # takes do not see each other's frames
    assert np.abs(two[0] - mr.speeds_ref(g["take.joints"][:40], fps)).max() <= 4 * e
    assert np.abs(two[1] - mr.speeds_ref(g["take.joints"][40:], fps)).max() <= 4 * e
    with pytest.raises(ValueError):
        joints.joint_speed(x[:1], fps)


# ---- beats ----------------------------------------------------------------------------------------------------------------------------
def test_beat_mask_is_the_fixtures_entry_for_entry(gold):
    g = gold
    ts, te, order, fps = int(g["take.t_start"]), int(g["take.t_end"]), int(g["take.order"]), int(g["take.fps"])
    vel = joints.joint_speed(dev(g["take.joints"]), fps, g["take.mmae"])
    mask = metrics.motion_beat_mask(vel, ts, te, order).cpu().numpy()
    assert mask.dtype == np.uint8 and np.array_equal(mask, g["take.beats"])
    assert not np.array_equal(mask, g["take.beats_corrected"])       # the verbatim threshold rule, vel[j], not vel[j + t_start]
    differs = np.argwhere(g["take.beats"] != g["take.beats_corrected"])
    assert len(differs) and all(mask[j, i] == g["take.beats"][j, i] for j, i in differs)
    assert np.array_equal(metrics.motion_beat_mask(vel, 0, len(vel), order).cpu().numpy(), g["take.beats_t0"])          # t_start = 0
    short = metrics.motion_beat_mask(vel, ts, ts + 2 * order - 4, order).cpu().numpy()                                   # n_slice < 2 order + 1
    assert short.shape == (2 * order - 4, 55) and np.array_equal(short, mr.beats_ref(g["take.vel"], ts, ts + 2 * order - 4, order))
    both = metrics.motion_beat_mask(torch.stack([vel, vel.flip(0)]), ts, te, order).cpu().numpy()                        # two takes in one launch
    assert np.array_equal(both[0], g["take.beats"]) and np.array_equal(both[1], mr.beats_ref(g["take.vel"][::-1], ts, te, order))
    assert metrics.motion_beat_mask(vel, 30, 30, order).shape == (0, 55)


def test_beats_plateau_and_clipped_ends():
    col = lambda *v: np.asarray(v, dtype=np.float32)
    vel = np.stack([col(.9, .8, .5, .5, .8, .9, .7, .4, .7, .9),     # a plateau of two equal values: strict < gives no beat; then a strict minimum
                    col(.1, .8, .9, .8, .7, .8, .9, .8, .9, .05),    # the slice's ends never qualify however low they are
                    col(.9, .8, .2, .8, .9, .9, .9, .9, .9, .9)], 1)  # a minimum below the threshold is no beat; a flat stretch has none
    got = metrics.motion_beat_mask(dev(vel), 0, 10, 2).cpu().numpy()
    want = np.zeros((10, 3), dtype=np.uint8)
    want[7, 0] = want[4, 1] = 1
    assert np.array_equal(got, want) and np.array_equal(mr.beats_ref(vel, 0, 10, 2), want)


# ---- beat consistency -----------------------------------------------------------------------------------------------------------------
def test_beat_consistency_against_the_fixture(gold):
    g = gold
    fps, sigma = int(g["take.fps"]), float(g["take.sigma"])
    mask = torch.from_numpy(g["take.beats"]).to(DEV)
    per, bc = metrics.beat_align(mask, g["take.onsets"], mr.UPPER_BODY, fps, sigma)
    print(f"bc: device {bc:.9f}, reference {float(g['take.bc']):.9f}")
    assert abs(bc - float(g["take.bc"])) <= 1e-5 and np.abs(per - g["take.per_joint"]).max() <= 1e-5
    quiet = [k for k, i in enumerate(mr.UPPER_BODY) if g["take.beats"][:, i].sum() == 0]
    assert quiet and all(per[k] == 0.0 for k in quiet)               # a joint without beats contributes exactly 0
    assert metrics.beat_align(torch.zeros_like(mask), g["take.onsets"], mr.UPPER_BODY, fps, sigma)[1] == 0.0
    some = g["take.onsets"][3:4]                                     # two takes, different onset counts, one launch
    per2, bc2 = metrics.beat_align(torch.stack([mask, mask]), [g["take.onsets"], some], mr.UPPER_BODY, fps, sigma)
    assert bc2[0] == np.float32(bc) and abs(bc2[1] - mr.bc_ref(g["take.beats"], some, mr.UPPER_BODY, fps, sigma)[1]) <= 1e-5
    with pytest.raises(ValueError, match="onsets"):
        metrics.beat_align(mask, [], mr.UPPER_BODY, fps, sigma)
    with pytest.raises(ValueError, match="onsets"):
        metrics.beat_consistency(dev(g["take.joints"]), np.zeros(0), g["take.mmae"], align_mask=int(g["take.t_start"]))
    # late onsets: times near 60 s keep their float64 precision on the way to the device
    late = np.zeros((1800, 55), dtype=np.uint8)
    late[1700:1790:15, 3] = 1
    on = 1700 / 30 + np.array([0.0123456789, 1.49, 2.2])
    assert abs(metrics.beat_align(torch.from_numpy(late).to(DEV), on, [3], 30, 0.3)[1] - mr.bc_ref(late, on, [3], 30, 0.3)[1]) <= 1e-6


# ---- L1 diversity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fixture", "ragged"])
def test_l1div_against_fp64_and_across_geometries(gold, case):
    x = gold["take.joints"] if case == "fixture" else (np.random.RandomState(4).randn(1003, 165) * 0.3 + np.linspace(-1, 1, 165)).astype(np.float32)
    want = mr.l1_ref(x)
    r = abs(mr.l1_ref_f32(x) - want) / want
    t = dev(x)
    before = t.clone()
    got = metrics.l1_sum(t)
    print(f"l1div {case}: R = {r:.3e}, device relative error = {abs(got - want) / want:.3e}")
    assert abs(got - want) / want <= max(4 * r, 1e-6)
    assert all(metrics.l1_sum(t, blocks=b) == got for b in (0, 1, 7, 333))           # launch geometries and repeated runs: the same bits
    both = metrics.l1_sum(torch.stack([t, t.flip(0) * 2]))           # two takes in one call: each its own mean, the same bits as alone
    assert both.shape == (2,) and both[0] == got and both[1] == metrics.l1_sum(t.flip(0) * 2)
    assert torch.equal(t, before)                                    # the input is only read
    calc = metrics.L1div()
    calc.run(t)
    calc.run(x)                                                      # numpy in, as test() calls it
    assert calc.counter == 2 * len(x) and abs(calc.avg() - want / len(x)) / (want / len(x)) <= max(4 * r, 1e-6)
    calc.reset()
    assert calc.counter == 0 and calc.sum == 0


# ---- recover_from_ric -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mr.RIC_CASES))
def test_recover_from_ric(gold, name):
    b, n, c, jn, seed = mr.RIC_CASES[name]
    assert name != "b1_n257" or n == joints.RIC_SCAN_TILE + 1       # one frame past the scan tile
    x, ref = mr.ric_inputs(b, n, c, seed), gold[f"ric.{name}"]
    f64 = mr.ric_ref(x, jn)
    e = float(np.abs(ref - f64).max())
    got = joints.recover_from_ric(dev(x), jn).cpu().numpy()
    print(f"ric {name}: reference fp32 error = {e:.3e}, device vs fp64 = {np.abs(got - f64).max():.3e}, device vs reference = {np.abs(got - ref).max():.3e}")
    assert got.shape == ref.shape == (b, n, jn, 3)
    assert np.abs(got - f64).max() <= 4 * e and np.abs(got - ref).max() <= 4 * e
    quat, pos = joints.recover_root_rot_pos(dev(x))
    assert quat.shape == (b, n, 4) and np.array_equal(pos.cpu().numpy(), got[:, :, 0])
    ang = np.concatenate([np.zeros((b, 1)), np.cumsum(x[..., :-1, 0].astype(np.float64), -1)], -1)
    q = quat.cpu().numpy()
    assert np.abs(q[..., 0] - np.cos(ang)).max() <= 1e-5 and np.abs(q[..., 2] - np.sin(ang)).max() <= 1e-5 and not q[..., 1::2].any()


# ---- the reference's test() sequence on one take, numpy in and out ---------------------------------------------------------------------
def test_the_reference_test_sequence_end_to_end(gold, skel):
    g = gold
    ts, te, order, fps, sigma = int(g["take.t_start"]), int(g["take.t_end"]), int(g["take.order"]), int(g["take.fps"]), float(g["take.sigma"])
    joints_rec = joints.smplx_joints(skel, dev(g["take.aa"].reshape(-1, 165)), dev(g["take.transl"])).cpu().numpy()
    assert joints_rec.shape == g["take.joints"].shape and joints_rec.dtype == np.float32
    kept = joints_rec.copy()
    l1 = metrics.L1div()
    l1.run(joints_rec)
    assert np.array_equal(joints_rec, kept)
    want = mr.l1_ref(g["take.joints"]) / len(kept)
    r = abs(float(g["take.l1_avg"]) - want) / want
    e_fk = float(np.abs(mr.fk_torch32(mr.smplx_parents(), g["take.rest"], g["take.aa"], g["take.transl"]).reshape(-1, 165) - g["take.joints"]).max())
    # the joints themselves may be 4 E_fk off; |x - mean| moves by at most twice that per entry
    assert abs(l1.avg() - want) <= max(4 * r, 1e-6) * want + 2 * 4 * e_fk * 165
    al = metrics.alignment(sigma, order, g["take.mmae"])
    beat_vel = al.load_pose(joints_rec, ts, te, fps, True)
    assert len(beat_vel) == 55 and all(isinstance(b, np.ndarray) for b in beat_vel)
    for i, b in enumerate(beat_vel):
        assert np.array_equal(b, np.nonzero(g["take.beats"][:, i])[0]), i
    bc = al.calculate_align(g["take.onsets"], beat_vel, fps)
    assert isinstance(bc, float) and abs(bc - float(g["take.bc"])) <= 1e-5
    one = metrics.beat_consistency(joints_rec, g["take.onsets"], g["take.mmae"], align_mask=ts, sigma=sigma, order=order)
    assert te == len(kept) - ts and abs(one - float(g["take.bc"])) <= 1e-5


# ---- scripts/motion_metrics_from_results.py on a synthetic results directory ------------------------------------------------------------
def test_results_script_weights_the_takes_as_test_does(gold, tmp_path):
    import importlib.util
    from tests.conftest import REPO
    spec = importlib.util.spec_from_file_location("motion_metrics_from_results", os.path.join(REPO, "scripts", "motion_metrics_from_results.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    g, r = gold, np.random.RandomState(12)
    V, K, mask = 20, 300, int(gold["take.t_start"])
    reg = r.rand(55, V)
    reg /= reg.sum(1, keepdims=True)
    model = {"v_template": r.randn(V, 3) * 0.5, "shapedirs": r.randn(V, 3, 400) * 0.01, "J_regressor": reg,
             "hands_meanl": r.randn(45) * 0.2, "hands_meanr": r.randn(45) * 0.2,
             "kintree_table": np.stack([np.concatenate([[2 ** 32 - 1], mr.smplx_parents()[1:]]), np.arange(55)]).astype(np.uint32)}
    np.savez(tmp_path / "model.npz", **model)
    np.save(tmp_path / "mean_vel.npy", g["take.mmae"])
    os.makedirs(tmp_path / "res")
    os.makedirs(tmp_path / "onsets")
    want_l1, want_align, frames = 0.0, 0.0, 0
    for k, n in enumerate((80, 61)):
        betas, pose = r.randn(K), g["take.aa"][:n].reshape(n, 165)
        np.savez(tmp_path / "res" / f"res_take{k}.npz", poses=pose, trans=np.zeros((n, 3), np.float32), betas=betas)
        onsets = g["take.onsets"][: 11 - 6 * k] * (n - 2 * mask) / 48.0
        np.save(tmp_path / "onsets" / f"take{k}.npy", onsets)
        # the same kernels called directly: what the script adds is the reading, the per-subject rest joints and test()'s weighting
        skel = joints.smplx_rest_joints(model, betas)
        want_rest = reg @ (model["v_template"] + model["shapedirs"][..., :K] @ betas)
        assert np.abs(skel.rest_joints[0].numpy() - want_rest).max() < 1e-6 and skel.pose_mean is not None     # the model's hand mean is in
        jt = joints.smplx_joints(skel, dev(pose))
        want_l1 += metrics.l1_sum(jt)
        want_align += metrics.beat_consistency(jt, onsets, g["take.mmae"], align_mask=mask) * (n - 2 * mask)
        frames += n
    out = script.main([str(tmp_path / "res"), "--smplx-model", str(tmp_path / "model.npz"), "--mean-vel", str(tmp_path / "mean_vel.npy"),
                       "--onsets", str(tmp_path / "onsets"), "--mask", str(mask)])
    assert out["takes"] == 2 and out["frames"] == frames and out["bc_takes"] == 2 and out["bc_frames"] == frames - 2 * 2 * mask
    assert out["l1div"] == want_l1 / frames                          # l1_calculator.avg(): sum over the takes / frames
    assert out["bc"] == want_align / (frames - 2 * 2 * mask)         # align / (total_length - 2 * takes * mask)
    no_onsets = script.main([str(tmp_path / "res"), "--smplx-model", str(tmp_path / "model.npz"), "--mean-vel", str(tmp_path / "mean_vel.npy")])
    assert "bc" not in no_onsets and no_onsets["l1div"] == out["l1div"]
