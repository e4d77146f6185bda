"""Motion metrics, host side: the fixture tests/golden/motion_metrics.npz regenerates bit for bit where the reference tree is at hand; the numpy
restatements of tests/motion_metrics_ref.py reproduce what the reference returned (so the GPU tests' oracles are pinned); smplx_rest_joints on a
synthetic model; the header's declarations; the refusals."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import motion_metrics_ref as mr
from tests.conftest import GOLDEN, REPO

from syntalker_amd import _lib, joints, metrics


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "motion_metrics.npz")))


def test_golden_regenerates_bit_identically(gold):
    spec = importlib.util.spec_from_file_location("make_motion_metrics_golden", os.path.join(GOLDEN, "make_motion_metrics_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(gen)                                   # (the generators put their own directories on sys.path)
    finally:
        sys.path[:] = path
    if not os.path.isdir(os.path.join(gen.REF, "utils")):
        pytest.skip("the reference tree is not on this machine")
    again = gen.build()
    assert sorted(again) == sorted(gold)
    for k, v in again.items():
        v = np.asarray(v)
        assert v.dtype == gold[k].dtype and v.shape == gold[k].shape and v.tobytes() == gold[k].tobytes(), k


def test_fixture_has_the_properties_the_gpu_tests_lean_on(gold):
    g = gold
    ts, te, order = int(g["take.t_start"]), int(g["take.t_end"]), int(g["take.order"])
    assert int(g["take.n"]) <= 128 and g["take.joints"].shape == (int(g["take.n"]), 165) and g["take.joints"].dtype == np.float32
    assert float(g["take.margin"]) >= 1e-4
    assert (g["take.beats"] != g["take.beats_corrected"]).any()                           # (b)
    assert any(g["take.beats"][:, i].sum() == 0 for i in mr.UPPER_BODY)                   # (c)
    assert any(g["take.beats"][:, i].sum() > 0 for i in mr.UPPER_BODY)                    # (d)
    assert g["take.beats"][0].sum() == 0 and g["take.beats"][-1].sum() == 0                # the slice's ends never qualify
    assert te - ts >= 2 * order + 1


def test_restatements_reproduce_the_reference(gold):
    g = gold
    ts, te, order, fps, sigma = int(g["take.t_start"]), int(g["take.t_end"]), int(g["take.order"]), int(g["take.fps"]), float(g["take.sigma"])
    # the joints are the fp64 oracle's, rounded
    want = mr.fk_oracle(mr.smplx_parents(), g["take.rest"], g["take.aa"], g["take.transl"]).astype(np.float32).reshape(-1, 165)
    assert np.array_equal(want, g["take.joints"])
    # speeds: the reference's float32 differences over a float64 mmae; the fp64 restatement within float32 rounding of the differences
    vel = mr.speeds_ref(g["take.joints"], fps, g["take.mmae"])
    assert np.abs(vel - g["take.vel"]).max() <= 1e-5 * np.abs(g["take.vel"]).max()
    assert np.array_equal(g["take.vel"][ts:te], g["take.vel_slice"])
    v2 = mr.speeds_ref(g["take.joints"][:2], fps, g["take.mmae"])
    assert np.abs(v2 - g["take2.vel"]).max() <= 1e-5 * np.abs(g["take2.vel"]).max()
    # beats: identical masks, for the slice, for t_start = 0, from the reference's speeds and from the restated ones
    for v in (g["take.vel"], vel):
        assert np.array_equal(mr.beats_ref(v, ts, te, order), g["take.beats"])
        assert np.array_equal(mr.beats_ref(v, 0, len(v), order), g["take.beats_t0"])
        assert np.array_equal(mr.beats_ref(v, ts, te, order, corrected=True), g["take.beats_corrected"])
    # BC and its per-joint terms
    per, bc = mr.bc_ref(g["take.beats"], g["take.onsets"], mr.UPPER_BODY, fps, sigma)
    assert abs(bc - float(g["take.bc"])) < 1e-12 and np.abs(per - g["take.per_joint"]).max() < 1e-12
    quiet = [k for k, i in enumerate(mr.UPPER_BODY) if g["take.beats"][:, i].sum() == 0]
    assert quiet and all(g["take.per_joint"][k] == 0.0 for k in quiet)
    # L1div: the as-written float32 path bitwise, the fp64 restatement within float32 summation error
    assert mr.l1_ref_f32(g["take.joints"]) == float(g["take.l1_sum"])
    assert float(g["take.l1_avg"]) == float(np.float32(g["take.l1_sum"]) / np.float32(len(g["take.joints"])))      # (the reference's sum is a float32)
    assert abs(mr.l1_ref(g["take.joints"]) - float(g["take.l1_sum"])) <= 1e-5 * float(g["take.l1_sum"])
    # recover_from_ric: the restatement in float32 against the reference's torch float32, and fp64 close behind
    for name, (b, n, c, jn, seed) in mr.RIC_CASES.items():
        x, ref = mr.ric_inputs(b, n, c, seed), g[f"ric.{name}"]
        assert ref.shape == (b, n, jn, 3)
        scale = max(1.0, np.abs(ref).max())
        assert np.abs(mr.ric_ref(x, jn, np.float32) - ref).max() <= 2e-5 * scale, name
        assert np.abs(mr.ric_ref(x, jn) - ref).max() <= 2e-5 * scale, name
    assert np.array_equal(mr.ric_ref(mr.ric_inputs(*mr.RIC_CASES["b1_n1"][:3], mr.RIC_CASES["b1_n1"][4]), 52, np.float32), g["ric.b1_n1"])   # yaw 0: exact


def test_host_static_helpers_match_the_reference(gold):
    g = gold
    fps, sigma = int(g["take.fps"]), float(g["take.sigma"])
    k = 0
    for i in range(55):
        if i not in mr.UPPER_BODY:
            continue
        beats = np.nonzero(g["take.beats"][:, i])[0]
        got = metrics.alignment.GAHR(metrics.alignment.motion_frames2time(beats, 0, fps), g["take.onsets"], sigma)
        assert abs(got - g["take.per_joint"][k]) < 1e-12
        k += 1
    with pytest.raises(ValueError):
        metrics.alignment.GAHR([0.5], [], sigma)
    with pytest.raises(ValueError, match="no audio onsets"):
        metrics.alignment(sigma, 7, g["take.mmae"]).calculate_align(np.zeros(0), [np.array([3])] * 55, fps)


def test_smplx_rest_joints_on_a_synthetic_model():
    r = np.random.RandomState(3)
    V, J, K = 20, 55, 10
    reg = r.rand(J + 3, V)
    reg /= reg.sum(1, keepdims=True)
    kin = np.stack([np.concatenate([[2 ** 32 - 1], mr.smplx_parents()[1:], [0, 0, 0]]), np.arange(J + 3)]).astype(np.uint32)
    model = {"v_template": r.randn(V, 3), "shapedirs": r.randn(V, 3, 16) * 0.1, "J_regressor": reg, "kintree_table": kin}
    betas = r.randn(K)
    skel = joints.smplx_rest_joints(model, betas)
    want = np.zeros((J, 3))
    for j in range(J):
        for v in range(V):
            want[j] += reg[j, v] * (model["v_template"][v] + sum(model["shapedirs"][v, :, k] * betas[k] for k in range(K)))
    assert skel.n_joints == 55 and skel.n_takes == 1
    assert np.array_equal(skel.parents, mr.smplx_parents().astype(np.int32))
    assert np.abs(skel.rest_joints[0].numpy() - want).max() < 1e-6
    two = joints.smplx_rest_joints(model, np.stack([betas, np.zeros(K)]))
    assert two.n_takes == 2 and np.abs(two.rest_joints[1].numpy() - reg[:J] @ model["v_template"]).max() < 1e-6
    # the hands' mean pose: smplx adds the model's hands_meanl / hands_meanr to joints 25..39 / 40..54 unless built with flat_hand_mean=True
    assert skel.pose_mean is None                                    # (a model without the arrays has none)
    hands = dict(model, hands_meanl=r.randn(45) * 0.2, hands_meanr=r.randn(45) * 0.2)
    with_mean = joints.smplx_rest_joints(hands, betas)
    assert with_mean.pose_mean.shape == (55, 3) and not with_mean.pose_mean[:25].any()
    assert np.array_equal(with_mean.pose_mean[25:40].numpy().reshape(-1), hands["hands_meanl"].astype(np.float32))
    assert np.array_equal(with_mean.pose_mean[40:].numpy().reshape(-1), hands["hands_meanr"].astype(np.float32))
    assert np.array_equal(with_mean.rest_joints.numpy(), skel.rest_joints.numpy())
    assert joints.smplx_rest_joints(hands, betas, flat_hand_mean=True).pose_mean is None
    with pytest.raises(ValueError):
        joints.Skeleton(mr.smplx_parents(), np.zeros((55, 3)), pose_mean=np.ones(10))
    with pytest.raises(ValueError):
        joints.smplx_rest_joints(model, r.randn(17))
    with pytest.raises(ValueError, match="topologically"):
        joints.Skeleton([-1, 2, 1], np.zeros((3, 3)))
    with pytest.raises(ValueError):
        joints.Skeleton([-1] * 65, np.zeros((65, 3)))


NEW_EXPORTS = ("syn_fk_joints", "syn_joint_speed", "syn_motion_beats", "syn_beat_align", "syn_l1div_workspace_bytes", "syn_l1div", "syn_recover_from_ric")


def test_header_declares_the_new_exports_and_the_abi_version_stays():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert re.search(r"^#define SYN_ABI_VERSION 9\b", header, flags=re.M) and _lib.ABI_VERSION == 9
    for name in NEW_EXPORTS:
        assert re.search(r"^int(64_t)?\s+%s\s*\(" % name, header, flags=re.M), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.syn_version() == 9
    assert len(lib.syn_fk_joints.argtypes) == 13 and len(lib.syn_beat_align.argtypes) == 13 and len(lib.syn_recover_from_ric.argtypes) == 8
    src = open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_kernels.hip")).read()
    assert '#include "syn_joints.inc"' in src
    assert joints.FK_FRAME_TILE == int(re.search(r"kFkFrames = (\d+)", open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_joints.inc")).read()).group(1))
    assert joints.RIC_SCAN_TILE == int(re.search(r"kRicTile = (\d+)", open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_joints.inc")).read()).group(1))


def test_cpu_tensors_raise(gold):
    skel = joints.Skeleton(mr.smplx_parents(), gold["take.rest"])
    with pytest.raises(_lib.SynHipError):
        joints.forward_kinematics(skel, torch.zeros(2, 55, 3))
    with pytest.raises(_lib.SynHipError):
        joints.smplx_joints(skel, torch.zeros(2, 330))
    with pytest.raises(_lib.SynHipError):
        joints.joint_speed(torch.zeros(4, 55, 3))
    with pytest.raises(_lib.SynHipError):
        joints.mean_joint_speed(torch.zeros(4, 165))
    with pytest.raises(_lib.SynHipError):
        joints.recover_from_ric(torch.zeros(1, 4, 263), 22)
    with pytest.raises(_lib.SynHipError):
        joints.recover_root_rot_pos(torch.zeros(1, 4, 263))
    with pytest.raises(_lib.SynHipError):
        metrics.l1_sum(torch.zeros(4, 165))
    with pytest.raises(_lib.SynHipError):
        metrics.L1div().run(torch.zeros(4, 165))
    with pytest.raises(_lib.SynHipError):
        metrics.motion_beat_mask(torch.zeros(40, 55), 0, 40, 7)
    with pytest.raises(_lib.SynHipError):
        metrics.beat_align(torch.zeros(40, 55, dtype=torch.uint8), [0.5])
    with pytest.raises(_lib.SynHipError):
        metrics.beat_consistency(torch.zeros(200, 165), [0.5], np.ones(55))


def test_load_audio_without_librosa_raises_the_documented_error(monkeypatch):
    monkeypatch.setitem(sys.modules, "librosa", None)              # an import of it now raises ImportError, installed or not
    with pytest.raises(ImportError, match="needs librosa"):
        metrics.alignment(0.3, 7, np.ones(55)).load_audio(np.zeros(16000, dtype=np.float32), without_file=True)


def test_dropin_seam_reexports_the_classes():
    from syntalker_amd.dropin.utils import metric
    assert metric.L1div is metrics.L1div and metric.alignment is metrics.alignment
    import inspect
    assert str(inspect.signature(metrics.alignment.__init__)) == "(self, sigma, order, mmae=None, upper_body=[3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21])"
    assert str(inspect.signature(metrics.alignment.load_pose)) == "(self, pose, t_start, t_end, pose_fps, without_file=False)"
    assert str(inspect.signature(metrics.alignment.calculate_align)) == "(self, onset_bt_rms, beat_vel, pose_fps=30)"
    assert str(inspect.signature(metrics.alignment.load_audio)) == "(self, wave, t_start=None, t_end=None, without_file=False, sr_audio=16000)"
