"""The SMPL-X mesh on the device (csrc/syn_mesh.inc; syntalker_amd/mesh.py, metrics.vertex_losses / face_losses) against the fp64 restatement of
tests/smplx_mesh_ref.py, which test_mesh_host.py pins.  `smplx` itself cannot run here; the oracle is the algebra.

Gates.  Vertices and joints: the same chain in plain fp32 torch on the CPU has a max abs error E against the fp64 oracle on the case's own inputs;
the device may be 4 E away (the project's FK rule).  Checked on the CPU for V = 203, n = 19, E = 100, sigma = 0.35 rad: E = 4.7e-7 at a vertex scale
of 1.4 m, and a strictly k-ordered fp32 chain - what the MFMA computes - lands on the same E.  Where the error is 0 by construction (zero pose, flat
hands, no expression): 1e-6 absolute.  Losses: relative error against fp64 numpy at most max(4 R, 1e-6), R the relative error of the reference's own
torch fp32 expression (the L1div rule).

Shapes: the smallest at which the kernels can go wrong - V one below / one above a vertex block and several blocks plus a ragged one; 1, tile + 1 and
2 tile + 3 frames; E in {0, 10, 100} (Kc 486, 496, 586: two need K padding); weight lists 1, 6 and 55 wide."""
import numpy as np
import pytest
import torch

from tests import smplx_mesh_ref as sm

from syntalker_amd import _lib, joints, mesh, metrics, poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, BLOCK = mesh.MESH_FRAME_TILE, mesh.MESH_VERTEX_BLOCK


def dev(x, dtype=torch.float32):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


_models = {}


def model_of(V, E, width, seed=3):
    key = (V, E, width, seed)
    if key not in _models:
        _models[key] = sm.synth_model(seed, V, E=E, max_weights=width)
    return _models[key]


def mesh_case(md, betas, pose, ex, tr, flat=False, label="", n_expr=None):
    """Device vertices and joints of one take against the fp64 oracle at 4 E.  Returns (vertices, joints, E_vertices, E_joints)."""
    want_v, want_j = sm.lbs_oracle(md, betas, pose, ex, tr, flat_hand_mean=flat)
    t_v, t_j = sm.lbs_torch32(md, betas, pose, ex, tr, flat_hand_mean=flat)
    e_v, e_j = float(np.abs(t_v - want_v).max()), float(np.abs(t_j - want_j).max())
    e = md["shapedirs"].shape[-1] - 300 if n_expr is None else n_expr
    m = mesh.smplx_mesh(md, betas, num_expression_coeffs=e, flat_hand_mean=flat)
    got_v, got_j = mesh.smplx_vertices(m, dev(pose), dev(ex), dev(tr), return_joints=True)
    got_v, got_j = got_v.cpu().numpy(), got_j.cpu().numpy()
    err_v, err_j = float(np.abs(got_v - want_v).max()), float(np.abs(got_j - want_j).max())
    print(f"mesh {label}: n = {len(pose)}, V = {want_v.shape[1]}, Kc = {m.n_dirs}, W = {m.width}: vertices E = {e_v:.3e}, device error = {err_v:.3e}, "
          f"gate = {4 * e_v:.3e}; joints E = {e_j:.3e}, device error = {err_j:.3e}, gate = {4 * e_j:.3e}")
    assert got_v.shape == want_v.shape and got_j.shape == want_j.shape
    assert err_v <= 4 * e_v and err_j <= 4 * e_j, (label, err_v, e_v, err_j, e_j)
    return got_v, got_j, e_v, e_j


# ---- every shape ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n,E,width", [(BLOCK - 1, 1, 0, 1), (BLOCK + 1, TILE + 1, 10, 6), (203, 2 * TILE + 3, 100, 6), (203, TILE + 1, 100, 55),
                                         (BLOCK - 1, 2 * TILE + 3, 10, 55), (BLOCK + 1, 1, 100, 1), (203, 1, 0, 6)])
def test_vertices_and_joints_against_the_fp64_oracle(V, n, E, width):
    pose, ex, betas, tr = sm.case_inputs(11 + n, n, E, transl=True)
    mesh_case(model_of(V, E, width), betas, pose, ex, tr, label=f"V{V} n{n} E{E} W{width}")
    mesh_case(model_of(V, E, width), betas, pose, ex, None, label=f"V{V} n{n} E{E} W{width}, no transl")


def test_large_angles_and_angles_next_to_pi():
    md = model_of(203, 100, 6)
    pose, ex, betas, _ = sm.case_inputs(5, 37, 100, amp=2.5)
    mesh_case(md, betas, pose, ex, None, label="large angles")
    r = np.random.RandomState(8)
    axis = r.randn(4, 55, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    near_pi = (axis * (np.pi - r.uniform(0, 1e-3, (4, 55, 1)))).astype(np.float32).reshape(4, 165)
    mesh_case(md, betas, near_pi, ex[:4], None, flat=True, label="angles within 1e-3 of pi")


def test_zero_pose_flat_hands_no_expression_is_the_shaped_template():
    md = model_of(203, 0, 6)
    _, _, betas, _ = sm.case_inputs(2, 3, 0)
    m = mesh.smplx_mesh(md, betas, num_expression_coeffs=0, flat_hand_mean=True)
    v, j = mesh.smplx_vertices(m, torch.zeros(3, 165, device=DEV), return_joints=True)
    assert np.abs(v.cpu().numpy() - m.v_shaped.numpy()).max() <= 1e-6       # (no rotation error at all: the weights' sum and the offsets' sums remain)
    assert np.abs(j.cpu().numpy() - m.skeleton.rest_joints.numpy()).max() <= 1e-6


def test_hand_mean_pose_on_and_off():
    md = model_of(203, 100, 6)
    pose, ex, betas, _ = sm.case_inputs(6, 5, 100)
    on, _, e_on, _ = mesh_case(md, betas, pose, ex, None, flat=False, label="hand mean pose")
    off, _, e_off, _ = mesh_case(md, betas, pose, ex, None, flat=True, label="flat hands")
    assert np.abs(on - off).max() > 1e3 * (e_on + e_off)


def test_6d_input_equals_axis_angle_input_within_the_gate():
    md = model_of(203, 100, 6)
    pose, ex, betas, tr = sm.case_inputs(7, 20, 100, transl=True)
    got_aa, _, e_aa, _ = mesh_case(md, betas, pose, ex, tr, label="axis-angle")
    m = mesh.smplx_mesh(md, betas)
    d6 = poses.axis_angle_to_rotation_6d(dev(pose).reshape(20, 55, 3))
    back = poses.rotation_6d_to_axis_angle(d6).reshape(20, 165).cpu().numpy()           # the conversion's own rounding is part of the 6D path's E
    want, _ = sm.lbs_oracle(md, betas, pose, ex, tr)
    e_6d = float(np.abs(sm.lbs_torch32(md, betas, back, ex, tr)[0] - want).max())
    got_6d = mesh.smplx_vertices(m, d6.reshape(20, 330), dev(ex), dev(tr)).cpu().numpy()
    print(f"mesh 6D: E_aa = {e_aa:.3e}, E_6d = {e_6d:.3e}, |6d - oracle| = {np.abs(got_6d - want).max():.3e}, |6d - aa| = {np.abs(got_6d - got_aa).max():.3e}")
    assert np.abs(got_6d - want).max() <= 4 * e_6d
    assert np.abs(got_6d - got_aa).max() <= 4 * (e_aa + e_6d)


# ---- takes ------------------------------------------------------------------------------------------------------------------------------------------
def test_two_takes_with_their_own_betas_in_one_launch():
    md = model_of(203, 100, 6)
    n = TILE + 1                                                     # the takes' boundary falls inside a frame tile
    pose, ex, b0, tr = sm.case_inputs(9, 2 * n, 100, transl=True)
    b1 = sm.case_inputs(10, 1, 100)[2]
    m = mesh.smplx_mesh(md, np.stack([b0, b1]))
    halves = [(b0, slice(0, n)), (b1, slice(n, 2 * n))]
    want = [sm.lbs_oracle(md, b, pose[s], ex[s], tr[s]) for b, s in halves]
    t32 = [sm.lbs_torch32(md, b, pose[s], ex[s], tr[s]) for b, s in halves]
    e_v = max(float(np.abs(t[0] - w[0]).max()) for t, w in zip(t32, want))
    e_j = max(float(np.abs(t[1] - w[1]).max()) for t, w in zip(t32, want))
    want_v, want_j = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    v, j = mesh.smplx_vertices(m, dev(pose), dev(ex), dev(tr), return_joints=True)
    assert np.abs(v.cpu().numpy() - want_v).max() <= 4 * e_v and np.abs(j.cpu().numpy() - want_j).max() <= 4 * e_j
    assert np.abs(sm.lbs_oracle(md, b1, pose[:n], ex[:n], tr[:n])[0] - want_v[:n]).max() > 1e-2       # (the two subjects do differ)
    # an explicit, interleaved frame-to-take index
    tof = np.arange(2 * n) % 2
    vi, ji = mesh.smplx_vertices(m, dev(pose), dev(ex), dev(tr), take_of_frame=torch.from_numpy(tof).to(DEV), return_joints=True)
    for k, b in enumerate((b0, b1)):
        sel = tof == k
        wv, wj = sm.lbs_oracle(md, b, pose[sel], ex[sel], tr[sel])
        tv, tj = sm.lbs_torch32(md, b, pose[sel], ex[sel], tr[sel])
        assert np.abs(vi.cpu().numpy()[sel] - wv).max() <= 4 * float(np.abs(tv - wv).max())
        assert np.abs(ji.cpu().numpy()[sel] - wj).max() <= 4 * float(np.abs(tj - wj).max())
    # a take outside the table: NaN for that frame's vertices and joints, the others finite
    bad_v, bad_j = mesh.smplx_vertices(m, dev(pose[:3]), dev(ex[:3]), dev(tr[:3]), take_of_frame=torch.tensor([0, 5, 1], device=DEV), return_joints=True)
    bad_v, bad_j = bad_v.cpu().numpy(), bad_j.cpu().numpy()
    assert np.isnan(bad_v[1]).all() and np.isnan(bad_j[1]).all()
    assert np.isfinite(bad_v[[0, 2]]).all() and np.isfinite(bad_j[[0, 2]]).all()
    neg = mesh.smplx_vertices(m, dev(pose[:2]), dev(ex[:2]), take_of_frame=torch.tensor([-1, 1], device=DEV)).cpu().numpy()
    assert np.isnan(neg[0]).all() and np.isfinite(neg[1]).all()
    with pytest.raises(ValueError, match="split evenly"):
        mesh.smplx_vertices(m, dev(pose[:3]))


def test_joints_are_forward_kinematics_bit_for_bit_without_expression():
    md = model_of(203, 100, 6)
    pose, _, betas, tr = sm.case_inputs(12, TILE + 5, 100, transl=True)
    for flat in (False, True):
        m = mesh.smplx_mesh(md, betas, flat_hand_mean=flat)
        _, j = mesh.smplx_vertices(m, dev(pose), return_joints=True)
        assert torch.equal(j, joints.forward_kinematics(m.skeleton, dev(pose).reshape(-1, 55, 3)))
        _, j = mesh.smplx_vertices(m, dev(pose), None, dev(tr), return_joints=True)
        assert torch.equal(j, joints.forward_kinematics(m.skeleton, dev(pose).reshape(-1, 55, 3), dev(tr)))


# ---- bitwise ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_frames_vertices_do_not_depend_on_the_launch():
    md = model_of(203, 100, 6)
    n, k = 2 * TILE + 3, 5                                           # k is no multiple of the frame tile: every frame changes its row and tile
    pose, ex, betas, tr = sm.case_inputs(13, n, 100, transl=True)
    m = mesh.smplx_mesh(md, betas)
    full_v, full_j = mesh.smplx_vertices(m, dev(pose), dev(ex), dev(tr), return_joints=True)
    again_v, again_j = mesh.smplx_vertices(m, dev(pose), dev(ex), dev(tr), return_joints=True)
    assert torch.equal(full_v, again_v) and torch.equal(full_j, again_j)
    part_v, part_j = mesh.smplx_vertices(m, dev(pose[k:]), dev(ex[k:]), dev(tr[k:]), return_joints=True)
    assert torch.equal(part_v, full_v[k:]) and torch.equal(part_j, full_j[k:])
    one = mesh.smplx_vertices(m, dev(pose[n - 1:]), dev(ex[n - 1:]), dev(tr[n - 1:]))
    assert torch.equal(one, full_v[n - 1:])


def test_device_packing_is_the_host_layout():
    for V, E in ((BLOCK + 1, 0), (203, 100)):
        md = model_of(V, E, 6)
        m = mesh.smplx_mesh(md, np.zeros(10), num_expression_coeffs=E)
        got = m.on(DEV)["dirs"].cpu().numpy()
        want = mesh.pack_dirs_host(m.posedirs.numpy(), m.exprdirs.numpy())
        assert got.size == want.size and np.array_equal(got, want.reshape(-1))


def test_no_frames_gives_empty_tensors():
    m = mesh.smplx_mesh(model_of(BLOCK - 1, 0, 1), np.zeros(10), num_expression_coeffs=0)
    v, j = mesh.smplx_vertices(m, torch.zeros(0, 165, device=DEV), return_joints=True)
    assert v.shape == (0, BLOCK - 1, 3) and j.shape == (0, 55, 3)
    with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
        mesh.smplx_vertices(m, torch.zeros(2, 165))


# ---- the face losses --------------------------------------------------------------------------------------------------------------------------------
def loss_gate(got, rec, tar, label):
    want, t32 = sm.losses_ref(rec, tar), sm.losses_torch32(rec, tar)
    for name, g, w, t in zip(("l2", "lvel"), got, want, t32):
        r = abs(t - w) / abs(w)
        rel = abs(g - w) / abs(w)
        print(f"losses {label} {name}: fp64 = {w:.9e}, device = {g:.9e}, rel = {rel:.3e}, R = {r:.3e}, gate = {max(4 * r, 1e-6):.3e}")
        assert rel <= max(4 * r, 1e-6), (label, name, g, w, r)


@pytest.mark.parametrize("n,c", [(2, 7), (33, 609), (70, 1000)])
def test_vertex_losses_against_fp64_and_bitwise(n, c):
    r = np.random.RandomState(n)
    tar = (np.cumsum(r.randn(n, c) * 0.01, 0) + r.randn(1, c) * 0.4).astype(np.float32)
    rec = (tar + r.randn(n, c) * 3e-3).astype(np.float32)
    got = metrics.vertex_losses(dev(rec), dev(tar))
    loss_gate(got, rec, tar, f"n{n} c{c}")
    assert got == metrics.vertex_losses(dev(rec), dev(tar))
    assert got == metrics.vertex_losses(dev(rec), dev(tar), blocks=1) == metrics.vertex_losses(dev(rec), dev(tar), blocks=7)
    assert got == metrics.vertex_losses(dev(rec).reshape(n, -1, 1), dev(tar).reshape(n, -1, 1))
    if n == 2:
        one = metrics.vertex_losses(dev(rec[:1]), dev(tar[:1]))
        assert np.isnan(one[1]) and abs(one[0] - sm.losses_ref(rec[:1], tar[:1])[0]) <= 1e-6 * one[0]     # (a single frame has no velocity)


def test_face_losses_as_the_reference_runs_them():
    """:640-673: both meshes with the jaw pose and the expression only - and the hands' mean pose, which smplx adds to a zero pose too."""
    md = model_of(203, 100, 6)
    n = TILE + 3
    rec_pose, rec_ex, betas, _ = sm.case_inputs(20, n, 100)
    tar_pose, tar_ex, _, _ = sm.case_inputs(21, n, 100)
    rec_pose = (tar_pose + 0.05 * rec_pose).astype(np.float32)
    rec_ex = (tar_ex + 0.1 * rec_ex).astype(np.float32)
    m = mesh.smplx_mesh(md, betas)

    def jaw_only(p):
        z = np.zeros_like(p)
        z[:, 66:69] = p[:, 66:69]
        return z
    want_rec = sm.lbs_oracle(md, betas, jaw_only(rec_pose), rec_ex)[0].reshape(n, -1)
    want_tar = sm.lbs_oracle(md, betas, jaw_only(tar_pose), tar_ex)[0].reshape(n, -1)
    want = sm.losses_ref(want_rec, want_tar)
    got = metrics.face_losses(m, dev(rec_pose), dev(tar_pose), dev(rec_ex), dev(tar_ex))
    # the device meshes are 4 E from the oracle's; a loss of differences of size d moves by at most 2 x 4 E / d relative (l2: twice that)
    e = max(float(np.abs(sm.lbs_torch32(md, betas, jaw_only(p), x)[0].reshape(n, -1) - w).max()) for p, x, w in ((rec_pose, rec_ex, want_rec), (tar_pose, tar_ex, want_tar)))
    d = float(np.abs(want_rec - want_tar).mean())
    print(f"face losses: fp64 = {want}, device = {got}, E = {e:.3e}, mean |rec - tar| = {d:.3e}")
    assert abs(got[1] - want[1]) <= 8 * e and abs(got[0] - want[0]) <= 2 * 8 * e * np.sqrt(want[0]) + (8 * e) ** 2
    assert got == metrics.face_losses(m, dev(rec_pose), dev(tar_pose), dev(rec_ex), dev(tar_ex))
    # the guard of the zeroing: with the body pose let through the numbers are others
    through = metrics.vertex_losses(mesh.smplx_vertices(m, dev(rec_pose), dev(rec_ex)), mesh.smplx_vertices(m, dev(tar_pose), dev(tar_ex)))
    assert abs(through[0] - got[0]) > 0.5 * got[0] and abs(through[1] - got[1]) > 0.5 * got[1]
    # ... and the jaw and the expression are each mesh's own
    swapped = metrics.face_losses(m, dev(tar_pose), dev(tar_pose), dev(rec_ex), dev(tar_ex))
    assert swapped != got
    same = metrics.face_losses(m, dev(tar_pose), dev(tar_pose), dev(tar_ex), dev(tar_ex))
    assert same[0] == 0.0 and same[1] == 0.0


# ---- the C ABI refuses what it cannot run, before any launch ----------------------------------------------------------------------------------------
def test_c_abi_argument_checks():
    lib = _lib.load()
    buf = torch.zeros(4096, device=DEV)
    ibuf = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p, ip = buf.data_ptr(), ibuf.data_ptr()
    st = _lib.current_stream(torch.device(DEV))

    def refused(rc, word):
        assert rc != 0 and word in lib.syn_last_error().decode(), (rc, lib.syn_last_error())

    def verts(dirs=p, V=16, kc=486, feat=p, xf=p, J=55, vs=p, takes=1, si=ip, sw=p, W=6, tr=None, tof=None, per=4, n=4, out=p):
        return lib.syn_mesh_vertices(dirs, V, kc, feat, xf, J, vs, takes, si, sw, W, tr, tof, per, n, out, st)

    def xform(par=ip, J=55, rest=p, takes=1, pose=p, mean=None, jd=None, ex=None, E=0, kc=486, tr=None, tof=None, per=4, n=4, feat=p, xf=p, jout=p):
        return lib.syn_fk_transforms(par, J, rest, takes, pose, mean, jd, ex, E, kc, tr, tof, per, n, feat, xf, jout, st)
    for name in ("dirs", "feat", "xf", "vs", "si", "sw", "out"):
        refused(verts(**{name: None}), "null")
    refused(verts(J=65), "64 joints")
    refused(verts(W=0), "wide")
    refused(verts(W=56), "wide")
    refused(verts(V=0), "vertices")
    refused(verts(V=-3), "vertices")
    refused(verts(kc=1025), "1024")
    refused(verts(n=-1), "negative")
    refused(verts(takes=0), "takes")
    refused(verts(per=0), "frames per take")
    refused(verts(per=3), "more frames")
    refused(verts(feat=p + 4), "aligned")
    assert verts(n=0) == 0
    for name in ("par", "rest", "pose", "feat", "xf", "jout"):
        refused(xform(**{name: None}), "null")
    refused(xform(J=65), "64 joints")
    refused(xform(J=1), "64 joints")
    refused(xform(E=-1), "negative")
    refused(xform(kc=1025), "1024")
    refused(xform(kc=485), "row length")
    refused(xform(E=10, kc=486), "row length")
    refused(xform(E=10, kc=496), "needs")
    refused(xform(n=-1), "negative")
    refused(xform(per=0), "frames per take")
    assert xform(n=0) == 0
    refused(lib.syn_mesh_pack_dirs(None, None, 16, 486, 0, p, st), "null")
    refused(lib.syn_mesh_pack_dirs(p, None, 16, 486, 10, p, st), "null")
    refused(lib.syn_mesh_pack_dirs(p, p, 0, 486, 10, p, st), "vertices")
    refused(lib.syn_mesh_pack_dirs(p, p, 16, 486, -1, p, st), "directions")
    refused(lib.syn_mesh_pack_dirs(p, p, 16, 1000, 100, p, st), "1024")
    assert lib.syn_vertex_losses_workspace_bytes(0, 5) == -1 and lib.syn_vertex_losses_workspace_bytes(5, -1) == -1
    assert lib.syn_vertex_losses_workspace_bytes(33, 10) == 2 * (2 * 10 + 10) * 8
    dbuf = torch.zeros(64, dtype=torch.float64, device=DEV).data_ptr()
    refused(lib.syn_vertex_losses(None, p, 4, 4, dbuf, 0, dbuf, st), "null")
    refused(lib.syn_vertex_losses(p, p, 4, 4, None, 0, dbuf, st), "null")
    refused(lib.syn_vertex_losses(p, p, 0, 4, dbuf, 0, dbuf, st), "empty")
    refused(lib.syn_vertex_losses(p, p, 4, -2, dbuf, 0, dbuf, st), "empty")
    refused(lib.syn_vertex_losses(p, p, 4, 4, dbuf + 4, 0, dbuf, st), "aligned")
    torch.cuda.synchronize()
    assert not buf.any() and not ibuf.any()                        # nothing ran
