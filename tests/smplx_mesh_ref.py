"""The SMPL-X mesh restated, and seeded models, for test_mesh_host.py, test_gpu_mesh.py and scripts/bench_mesh.py.

`smplx` is not installed and its model file is not here, so nothing can execute the reference's `smplx(...)`.  What it computes is linear blend
skinning, stated step by step in syntalker_amd/mesh.py's docstring; `lbs_oracle` is that statement in numpy at a chosen precision (fp64: THE oracle of
the mesh tests, as motion_metrics_ref.fk_oracle is for the joints - test_mesh_host.py pins the two to each other), `lbs_torch32` the same chain in
plain fp32 torch, whose error against the oracle is the yardstick E of the GPU gates.  `synth_model` makes a dict in the model file's layout with
realistic magnitudes from a seed."""
import numpy as np

from tests import motion_metrics_ref as mr

J = 55
SHAPE_SPACE = 300


def synth_model(seed, V, E=100, max_weights=6):
    """A dict with the arrays of SMPLX_NEUTRAL_2020.npz at V vertices: template ~ 0.4 m, shape directions ~ 5e-3, expression directions ~ 3e-3,
    posedirs ~ 1e-2, non-negative J_regressor and weights rows summing to 1 (every vertex 1 .. max_weights non-zero weights, vertex 0 exactly
    max_weights), the 55-joint tree of golden/smplx_kintree.json with the root's parent stored as 2^32 - 1, non-zero hand mean poses."""
    r = np.random.RandomState(seed)
    par = mr.smplx_parents()
    m = {}
    m["v_template"] = (r.randn(V, 3) * 0.4).astype(np.float32)
    sd = r.randn(V, 3, SHAPE_SPACE + E).astype(np.float32)
    sd[..., :SHAPE_SPACE] *= 5e-3
    sd[..., SHAPE_SPACE:] *= 3e-3
    m["shapedirs"] = sd
    m["posedirs"] = (r.randn(V, 3, 9 * (J - 1)) * 1e-2).astype(np.float32)
    reg = np.zeros((J, V))
    for j in range(J):                                     # a joint is regressed from a handful of vertices
        pick = r.choice(V, size=min(V, 8), replace=False)
        reg[j, pick] = r.uniform(0.1, 1.0, pick.size)
    m["J_regressor"] = (reg / reg.sum(1, keepdims=True)).astype(np.float32)
    w = np.zeros((V, J))
    for v in range(V):
        k = max_weights if v == 0 else r.randint(1, max_weights + 1)
        pick = r.choice(J, size=k, replace=False)
        w[v, pick] = r.uniform(0.05, 1.0, k)
    m["weights"] = (w / w.sum(1, keepdims=True)).astype(np.float32)
    kt = np.stack([np.where(par < 0, 2 ** 32 - 1, par), np.arange(J)]).astype(np.uint32)
    m["kintree_table"] = kt
    m["f"] = r.randint(0, V, (2 * V, 3)).astype(np.uint32)
    m["hands_meanl"] = (r.randn(45) * 0.2).astype(np.float32)
    m["hands_meanr"] = (r.randn(45) * 0.2).astype(np.float32)
    return m


def pose_mean(model, flat_hand_mean=False, dtype=np.float64):
    mean = np.zeros((J, 3), dtype=dtype)
    if not flat_hand_mean:
        mean[25:40] = np.asarray(model["hands_meanl"], dtype=dtype).reshape(15, 3)
        mean[40:55] = np.asarray(model["hands_meanr"], dtype=dtype).reshape(15, 3)
    return mean


def lbs_oracle(model, betas, pose, expression=None, transl=None, dtype=np.float64, flat_hand_mean=False, parts=False, rest_follows_expression=True):
    """The seven steps of the mesh contract.  betas (K,); pose (n, 165) axis-angle; expression (n, E) or None; transl (n, 3) or None ->
    (vertices (n, V, 3), joints (n, 55, 3)) in `dtype`; parts=True: a dict of the intermediates as well.  rest_follows_expression=False is the WRONG
    model that regresses the joints before the expression term (what `joints.smplx_rest_joints` may assume for test()'s zero expression only)."""
    par = mr.smplx_parents()
    pose = np.asarray(pose, dtype=dtype).reshape(len(pose), J, 3)
    n = len(pose)
    betas = np.asarray(betas, dtype=dtype).reshape(-1)
    sd = np.asarray(model["shapedirs"], dtype=dtype)
    R = mr.aa_matrix(pose + pose_mean(model, flat_hand_mean, dtype)[None], dtype)                    # 1
    v_shaped = np.asarray(model["v_template"], dtype=dtype) + sd[..., :betas.size] @ betas             # 2
    v_shaped = np.broadcast_to(v_shaped, (n,) + v_shaped.shape)
    v_neutral = v_shaped
    if expression is not None:
        ex = np.asarray(expression, dtype=dtype)
        v_shaped = v_shaped + np.einsum("vce,ne->nvc", sd[..., SHAPE_SPACE:SHAPE_SPACE + ex.shape[1]], ex)
    j_rest = np.einsum("jv,nvc->njc", np.asarray(model["J_regressor"], dtype=dtype)[:J], v_shaped if rest_follows_expression else v_neutral)     # 3
    feature = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(n, 9 * (J - 1))                            # 4
    v_posed = v_shaped + np.einsum("vck,nk->nvc", np.asarray(model["posedirs"], dtype=dtype), feature)  # 5
    GR, Gt = [None] * J, [None] * J                                                                # 6
    for j, p in enumerate(par):
        if p < 0:
            GR[j], Gt[j] = R[:, j], j_rest[:, j]
        else:
            GR[j] = GR[p] @ R[:, j]
            Gt[j] = (GR[p] @ (j_rest[:, j] - j_rest[:, p])[..., None])[..., 0] + Gt[p]
    GR, Gt = np.stack(GR, 1), np.stack(Gt, 1)
    At = Gt - (GR @ j_rest[..., None])[..., 0]
    w = np.asarray(model["weights"], dtype=dtype)[:, :J]                                             # 7
    per_joint = np.einsum("njab,nvb->nvja", GR, v_posed) + At[:, None]
    verts = np.einsum("vj,nvja->nva", w, per_joint)
    joints = Gt
    if transl is not None:
        t = np.asarray(transl, dtype=dtype)
        verts, joints = verts + t[:, None], joints + t[:, None]
    if parts:
        return dict(vertices=verts, joints=joints, v_shaped=v_shaped, j_rest=j_rest, v_posed=v_posed, GR=GR, Gt=Gt, feature=feature)
    return verts.astype(dtype), joints.astype(dtype)


def rodrigues32(aa):
    """fp32 torch: Rodrigues with sin t / t and (1 - cos t) / t^2, their series below 1e-4 (motion_metrics_ref.fk_torch32's)."""
    import torch
    t = aa.norm(dim=-1)
    small = t < 1e-4
    ts = torch.where(small, torch.ones_like(t), t)
    a = torch.where(small, 1 - t * t / 6, torch.sin(ts) / ts)[..., None, None]
    b = torch.where(small, 0.5 - t * t / 24, (1 - torch.cos(ts)) / (ts * ts))[..., None, None]
    x, y, z = aa[..., 0], aa[..., 1], aa[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(aa.shape[:-1] + (3, 3))
    return torch.eye(3, device=aa.device) + a * K + b * (K @ K)


def lbs_torch32(model, betas, pose, expression=None, transl=None, flat_hand_mean=False, device="cpu", chunk=None, as_numpy=True):
    """The same chain in plain fp32 torch (dense weights, a 3 x 4 per vertex and joint as `smplx` forms it), `chunk` frames at a time."""
    import torch
    par = mr.smplx_parents()
    f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=device) if not torch.is_tensor(a) else a.to(device).float()
    pose = f(pose).reshape(-1, J, 3)
    n = pose.shape[0]
    betas = f(betas).reshape(-1)
    sd, vt, pd = f(model["shapedirs"]), f(model["v_template"]), f(model["posedirs"])
    reg, w = f(model["J_regressor"])[:J], f(model["weights"])[:, :J]
    mean = f(pose_mean(model, flat_hand_mean, np.float32))
    shaped0 = vt + sd[..., :betas.numel()] @ betas
    ex_all = None if expression is None else f(expression)
    tr_all = None if transl is None else f(transl)
    verts, joints = [], []
    step = chunk or max(n, 1)
    for s in range(0, n, step):
        R = rodrigues32(pose[s:s + step] + mean)
        m = R.shape[0]
        v_shaped = shaped0.expand(m, -1, -1)
        if ex_all is not None:
            ex = ex_all[s:s + step]
            v_shaped = v_shaped + torch.einsum("vce,ne->nvc", sd[..., SHAPE_SPACE:SHAPE_SPACE + ex.shape[1]], ex)
        j_rest = torch.einsum("jv,nvc->njc", reg, v_shaped)
        feature = (R[:, 1:] - torch.eye(3, device=device)).reshape(m, 9 * (J - 1))
        v_posed = v_shaped + torch.einsum("vck,nk->nvc", pd, feature)
        GR, Gt = [None] * J, [None] * J
        for j, p in enumerate(par):
            if p < 0:
                GR[j], Gt[j] = R[:, j], j_rest[:, j]
            else:
                GR[j] = GR[p] @ R[:, j]
                Gt[j] = (GR[p] @ (j_rest[:, j] - j_rest[:, p])[..., None])[..., 0] + Gt[p]
        GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
        A = torch.cat([GR, (Gt - (GR @ j_rest[..., None])[..., 0])[..., None]], -1)           # (m, J, 3, 4)
        T = torch.einsum("vj,njab->nvab", w, A)                                                # (m, V, 3, 4): the per-vertex transform
        v = (T[..., :3] @ v_posed[..., None])[..., 0] + T[..., 3]
        if tr_all is not None:
            v, Gt = v + tr_all[s:s + step, None], Gt + tr_all[s:s + step, None]
        verts.append(v)
        joints.append(Gt)
    verts, joints = torch.cat(verts), torch.cat(joints)
    return (verts.cpu().numpy(), joints.cpu().numpy()) if as_numpy else (verts, joints)


def losses_ref(rec, tar, dtype=np.float64):
    """(l2, lvel) as test() writes them (:672-673), in `dtype` throughout."""
    r, t = np.asarray(rec, dtype=dtype).reshape(len(rec), -1), np.asarray(tar, dtype=dtype).reshape(len(tar), -1)
    l2 = ((r - t) ** 2).mean(dtype=dtype)
    lvel = np.abs((r[1:] - t[:-1]) - (t[1:] - t[:-1])).mean(dtype=dtype)
    return float(l2), float(lvel)


def losses_torch32(rec, tar):
    """The reference's own expression in torch fp32: nn.L1Loss and nn.MSELoss on float32 tensors."""
    import torch
    r = torch.as_tensor(np.asarray(rec, dtype=np.float32)).reshape(len(rec), -1)
    t = torch.as_tensor(np.asarray(tar, dtype=np.float32)).reshape(len(tar), -1)
    lvel = torch.nn.L1Loss()(r[1:] - t[:-1], t[1:] - t[:-1])
    return float(torch.nn.MSELoss()(r, t)), float(lvel)


def case_inputs(seed, n, E, amp=0.35, transl=False):
    """pose (n, 165) band-limited axis-angle noise of amplitude `amp`, expression (n, E) ~ N(0, 1) (None for E = 0), betas (300,), transl."""
    r = np.random.RandomState(seed)
    pose = mr.smooth_rotations(seed, n, amp=amp).reshape(n, 165)
    ex = r.randn(n, E).astype(np.float32) if E else None
    betas = r.randn(SHAPE_SPACE).astype(np.float32)
    tr = (r.randn(n, 3) * 0.5).astype(np.float32) if transl else None
    return pose, ex, betas, tr
