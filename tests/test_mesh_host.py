"""The mesh oracle (tests/smplx_mesh_ref.py) and the host side of syntalker_amd/mesh.py, without a GPU: the oracle is pinned to the FK oracle and to
closed-form cases, the loader's products, the weight compaction and the direction layout to numpy restatements."""
import numpy as np
import pytest

from tests import motion_metrics_ref as mr
from tests import smplx_mesh_ref as sm

from syntalker_amd import joints, mesh

V = 203


@pytest.fixture(scope="module")
def model():
    return sm.synth_model(3, V)


@pytest.fixture(scope="module")
def take():
    return sm.case_inputs(4, 7, 100, transl=True)


def test_oracle_joints_are_the_fk_oracles_on_the_loaders_skeleton(model, take):
    pose, _, betas, tr = take
    skel = joints.smplx_rest_joints(model, betas)
    _, got = sm.lbs_oracle(model, betas, pose, None, tr)
    rot = pose.reshape(-1, 55, 3).astype(np.float64) + sm.pose_mean(model)[None]
    want = mr.fk_oracle(skel.parents, skel.rest_joints[0].numpy(), rot, tr)
    assert np.abs(got - want).max() < 2e-6                      # (the skeleton's rest joints are rounded to fp32: 6e-8 a joint, 11 levels deep)
    assert np.array_equal(skel.pose_mean.numpy(), sm.pose_mean(model, dtype=np.float32))


def test_zero_pose_with_flat_hands_is_the_shaped_template(model, take):
    _, ex, betas, _ = take
    p = sm.lbs_oracle(model, betas, np.zeros((7, 165)), ex, None, flat_hand_mean=True, parts=True)
    wsum = model["weights"].astype(np.float64).sum(1)[None, :, None]       # fp32 weights add up to 1 within 6e-8 only, and A = [I | 0] for every joint
    assert np.abs(p["vertices"] - p["v_shaped"] * wsum).max() < 1e-13 and np.abs(p["vertices"] - p["v_shaped"]).max() < 1e-7
    assert np.abs(p["joints"] - p["j_rest"]).max() < 1e-13
    q = sm.lbs_oracle(model, betas, np.zeros((7, 165)), ex, None, flat_hand_mean=False, parts=True)
    assert np.abs(q["vertices"] - q["v_shaped"]).max() > 1e-3    # the hands' mean pose is a pose


def test_one_hot_weights_give_a_rigid_transform_per_vertex(model, take):
    pose, ex, betas, tr = take
    hot = dict(model)
    owner = np.arange(V) % 55
    hot["weights"] = np.eye(55, dtype=np.float32)[owner]
    p = sm.lbs_oracle(hot, betas, pose, ex, tr, parts=True)
    rel = p["v_posed"] - p["j_rest"][:, owner]
    want = np.einsum("nvab,nvb->nva", p["GR"][:, owner], rel) + p["Gt"][:, owner] + tr[:, None]
    assert np.abs(p["vertices"] - want).max() < 1e-12


def test_expression_moves_the_rest_joints_and_the_mesh_needs_it(model, take):
    pose, ex, betas, _ = take
    m = mesh.smplx_mesh(model, betas)
    with_ex = sm.lbs_oracle(model, betas, pose, ex, parts=True)
    without = sm.lbs_oracle(model, betas, pose, None, parts=True)
    moved = with_ex["j_rest"] - without["j_rest"]
    assert np.abs(moved).max() > 1e-3
    assert np.abs(np.einsum("jce,ne->njc", m.joint_dirs.numpy().astype(np.float64), ex) - moved).max() < 1e-6
    assert np.abs(m.skeleton.rest_joints[0].numpy() - without["j_rest"][0]).max() < 1e-6
    wrong, _ = sm.lbs_oracle(model, betas, pose, ex, rest_follows_expression=False)
    assert np.abs(wrong - with_ex["vertices"]).max() > 1e-4       # far above any fp32 gate (~1e-6)


def test_loader_products(model, take):
    _, _, betas, _ = take
    m = mesh.smplx_mesh(model, np.stack([betas, 0.5 * betas]), num_expression_coeffs=10)
    assert (m.n_subjects, m.n_vertices, m.n_expression, m.n_dirs) == (2, V, 10, 496)
    sd = model["shapedirs"].astype(np.float64)
    want = model["v_template"] + sd[..., :300] @ (0.5 * betas.astype(np.float64))
    assert np.abs(m.v_shaped[1].numpy() - want).max() < 1e-6
    assert np.array_equal(m.exprdirs.numpy(), model["shapedirs"][..., 300:310]) and np.array_equal(m.faces, model["f"])
    short = mesh.smplx_mesh(model, betas[:10], num_expression_coeffs=0)
    assert short.n_dirs == 486 and short.n_expression == 0
    assert np.abs(short.v_shaped[0].numpy() - (model["v_template"] + sd[..., :10] @ betas[:10].astype(np.float64))).max() < 1e-6
    assert mesh.smplx_mesh(model, betas, flat_hand_mean=True).skeleton.pose_mean is None


@pytest.mark.parametrize("width", [1, 6, 55])
def test_weight_compaction_round_trips(width):
    w = sm.synth_model(5, 70, E=0, max_weights=width)["weights"]
    idx, val = mesh.compact_weights(w)
    assert idx.shape == val.shape == (70, width) and idx.dtype == np.int32 and val.dtype == np.float32
    assert width == int((w != 0).sum(1).max())
    assert np.array_equal(mesh.dense_weights(idx, val, 55), w)
    for v in (0, 1, 69):                                            # a vertex's entries in joint order, the padding at its end
        k = int((w[v] != 0).sum())
        assert np.array_equal(idx[v, :k], np.nonzero(w[v])[0]) and not val[v, k:].any() and not idx[v, k:].any()


@pytest.mark.parametrize("E", [0, 10, 100])
def test_direction_layout_round_trips(E):
    r = np.random.RandomState(E)
    v = mesh.MESH_VERTEX_BLOCK + 1
    pd, ed = r.randn(v, 3, 486).astype(np.float32), r.randn(v, 3, E).astype(np.float32)
    packed = mesh.pack_dirs_host(pd, ed)
    kcp = -(-(486 + E) // mesh.DIR_GROUP) * mesh.DIR_GROUP
    assert packed.shape == (2 * mesh.MESH_VERTEX_BLOCK // 16, kcp // mesh.DIR_GROUP, 3, 64, 4)
    assert np.array_equal(mesh.unpack_dirs_host(packed, v, 486 + E), np.concatenate([pd, ed], -1))
    full = np.concatenate([pd, ed, np.zeros((v, 3, kcp - 486 - E), np.float32)], -1)
    for t, g, p, l, u in [(0, 0, 0, 0, 0), (4, 30, 2, 16, 3), (3, kcp // 16 - 1, 1, 63, 3), (1, 7, 2, 37, 1), (4, 2, 0, 1, 0)]:
        vert, k = 16 * t + (l & 15), 16 * g + 4 * (l >> 4) + u       # the kernel's index arithmetic, spelled out
        assert packed[t, g, p, l, u] == (full[vert, p, k] if vert < v else 0)
    assert not packed.reshape(-1, kcp // 16, 3, 4, 16, 4)[4, :, :, :, 1:].any()          # vertices past V
    if kcp > 486 + E:
        assert not mesh.unpack_dirs_host(packed, v, kcp)[..., 486 + E:].any()             # directions past Kc


def test_vel_loss_as_written_is_the_simplified_one_up_to_rounding():
    r = np.random.RandomState(0)
    tar = np.cumsum(r.randn(40, 90) * 0.01, 0).astype(np.float32) + 1.0
    rec = (tar + r.randn(40, 90) * 3e-3).astype(np.float32)
    l2, lvel = sm.losses_ref(rec, tar)
    simple = float(np.abs(rec[1:].astype(np.float64) - tar[1:]).mean())
    assert abs(lvel - simple) < 1e-15                               # in fp64 the previous target frame cancels
    l2_32, lvel_32 = sm.losses_ref(rec, tar, np.float32)
    assert 0 < abs(lvel_32 - simple) / simple < 1e-4                # in fp32 it leaves its rounding behind
    t2, tv = sm.losses_torch32(rec, tar)
    assert abs(t2 - l2) / l2 < 1e-5 and abs(tv - lvel) / lvel < 1e-4


def test_loader_errors(model, take):
    _, _, betas, _ = take
    with pytest.raises(ValueError, match="betas"):
        mesh.smplx_mesh(model, np.zeros(301))
    with pytest.raises(ValueError, match="expression"):
        mesh.smplx_mesh(model, betas, num_expression_coeffs=101)
    bad = dict(model)
    bad["weights"] = model["weights"].copy()
    bad["weights"][17] = 0
    with pytest.raises(ValueError, match="vertex 17"):
        mesh.smplx_mesh(bad, betas)
    with pytest.raises(ValueError, match="vertex 17"):
        mesh.compact_weights(bad["weights"])
