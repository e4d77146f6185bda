"""The SMPL-X mesh on the device: what `smplx(...)["vertices"]` gives the reference's `test()` (diffusion_rvqvae_trainer.py:640-675) and its renderers
(utils/other_tools.py render_one_sequence*, demo.py) - pose, expression and shape in, the model's vertices per frame out (csrc/syn_mesh.inc,
DESIGN.md §21).  `smplx` is not imported; the algebra is linear blend skinning:

    v_shaped = v_template + shapedirs[:, :, :K] . betas + shapedirs[:, :, 300:300 + E] . expression
    J_rest   = J_regressor[:55] . v_shaped                     (so a frame's rest joints move with its expression)
    v_posed  = v_shaped + posedirs . concat_j (R_j - I)        R_j = Rodrigues(full_pose_j + pose_mean_j)
    vertex   = sum_j weights[v, j] (A_j^R v_posed + A_j^t) + transl,   A_j = [G_j^R | G_j^t - G_j^R J_rest,j],  joint_j = G_j^t + transl

`smplx_mesh` does the per-subject part once on the host in fp64 (as `joints.smplx_rest_joints` does); `smplx_vertices` runs the per-frame part in two
launches, `syn_fk_transforms` and `syn_mesh_vertices`.  The first 55 joints come along; the other 72 entries of `smplx(...)["joints"]` (vertex-selected
joints, face landmarks) stay out.  Drawing the vertices is `syntalker_amd/render.py`, the video with its sound track (Motion-JPEG AVI, PCM)
`syntalker_amd/video.py`, audio resampling `syntalker_amd/audio.py`; H.264 / mp4 stay out.  Device tensors only, like the rest of the package: a CPU tensor or a missing library raises."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, engine
from .joints import Skeleton, smplx_rest_joints

MESH_FRAME_TILE = 32       # csrc/syn_mesh.inc kFrameTile: frames per workgroup
MESH_VERTEX_BLOCK = 64     # csrc/syn_mesh.inc kVertexBlock: vertices per workgroup
DIR_GROUP = 16             # csrc/syn_mesh.inc kGroup: directions per packed group
MAX_DIRECTIONS = 1024      # csrc/syn_mesh.inc kMaxKc
SHAPE_SPACE = 300          # SMPL-X: shapedirs[..., :300] are shape directions, the expression directions follow
N_JOINTS = 55


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def compact_weights(weights):
    """Dense skin weights (V, J) -> (index (V, W) int32, weight (V, W) float32), W the largest count of non-zero weights of a vertex: each vertex's
    non-zero weights in joint order, shorter lists padded with (0, 0.0)."""
    w = np.asarray(weights)
    if w.ndim != 2:
        raise ValueError(f"compact_weights: weights are (V, J), got {w.shape}")
    nz = w != 0
    count = nz.sum(1)
    if (count == 0).any():
        raise ValueError(f"compact_weights: vertex {int(np.argmin(count))} has no non-zero skin weight")
    width = int(count.max())
    order = np.argsort(~nz, axis=1, kind="stable")[:, :width]               # non-zero columns first, in joint order
    keep = np.take_along_axis(nz, order, 1)
    idx = np.where(keep, order, 0).astype(np.int32)
    val = np.where(keep, np.take_along_axis(w, order, 1), 0).astype(np.float32)
    return np.ascontiguousarray(idx), np.ascontiguousarray(val)


def dense_weights(index, weight, n_joints: int):
    """The inverse of `compact_weights`: (V, n_joints) float32."""
    idx, val = np.asarray(index), np.asarray(weight, dtype=np.float32)
    out = np.zeros((idx.shape[0], n_joints), dtype=np.float32)
    np.add.at(out, (np.arange(idx.shape[0])[:, None], idx), val)
    return out


def pack_dirs_host(posedirs, exprdirs):
    """`syn_mesh_pack_dirs` in numpy: posedirs (V, 3, P) and exprdirs (V, 3, E) -> float32 [Vp / 16][Kcp / 16][3][64][4], element (t, g, p, l, u) =
    direction 16 g + 4 (l >> 4) + u (pose correctives, then expressions) of coordinate p of vertex 16 t + (l & 15); zero beyond Kc = P + E and V."""
    pd = np.asarray(posedirs, dtype=np.float32)
    ed = np.asarray(exprdirs, dtype=np.float32).reshape(pd.shape[0], 3, -1)
    v, kc = pd.shape[0], pd.shape[2] + ed.shape[2]
    vp, kcp = _round_up(v, MESH_VERTEX_BLOCK), _round_up(kc, DIR_GROUP)
    full = np.zeros((vp, 3, kcp), dtype=np.float32)
    full[:v, :, :pd.shape[2]] = pd
    full[:v, :, pd.shape[2]:kc] = ed
    # (t, i = l & 15, p, g, q = l >> 4, u) -> (t, g, p, q, i, u)
    return np.ascontiguousarray(full.reshape(vp // 16, 16, 3, kcp // DIR_GROUP, 4, 4).transpose(0, 3, 2, 4, 1, 5)).reshape(vp // 16, kcp // DIR_GROUP, 3, 64, 4)


def unpack_dirs_host(packed, n_verts: int, n_dirs: int):
    """The inverse of `pack_dirs_host`: (V, 3, Kc)."""
    p = np.asarray(packed)
    t, g = p.shape[0], p.shape[1]
    full = p.reshape(t, g, 3, 4, 16, 4).transpose(0, 4, 2, 1, 3, 5).reshape(t * 16, 3, g * DIR_GROUP)
    return np.ascontiguousarray(full[:n_verts, :, :n_dirs])


class SmplxMesh:
    """One model for one or several subjects: v_shaped (S, V, 3), `skeleton` (rest joints at zero expression, parents, hand mean pose), joint_dirs
    (J, 3, E) = J_regressor . expression directions, the compacted skin weights skin_index / skin_weight (V, W), posedirs (V, 3, 9 (J - 1)), exprdirs
    (V, 3, E), faces (F, 3) as the file has them.  `on(device)` moves everything once and packs the directions there."""

    def __init__(self, v_shaped, skeleton: Skeleton, joint_dirs, skin_index, skin_weight, posedirs, exprdirs, faces=None):
        self.v_shaped = torch.as_tensor(np.asarray(v_shaped, dtype=np.float32)).contiguous()
        if self.v_shaped.dim() == 2:
            self.v_shaped = self.v_shaped[None]
        self.skeleton = skeleton
        v, j = self.v_shaped.shape[1], skeleton.n_joints
        self.posedirs = torch.as_tensor(np.asarray(posedirs, dtype=np.float32)).contiguous()
        self.exprdirs = torch.as_tensor(np.asarray(exprdirs, dtype=np.float32)).reshape(v, 3, -1).contiguous()
        self.joint_dirs = torch.as_tensor(np.asarray(joint_dirs, dtype=np.float32)).reshape(j, 3, -1).contiguous()
        self.skin_index = torch.as_tensor(np.asarray(skin_index, dtype=np.int32)).contiguous()
        self.skin_weight = torch.as_tensor(np.asarray(skin_weight, dtype=np.float32)).contiguous()
        self.faces = None if faces is None else np.asarray(faces)
        if self.v_shaped.shape[0] != skeleton.n_takes:
            raise ValueError(f"SmplxMesh: {self.v_shaped.shape[0]} shaped templates for {skeleton.n_takes} skeletons")
        if tuple(self.posedirs.shape) != (v, 3, 9 * (j - 1)):
            raise ValueError(f"SmplxMesh: posedirs are (V, 3, 9 (J - 1)) = ({v}, 3, {9 * (j - 1)}), got {tuple(self.posedirs.shape)}")
        if self.joint_dirs.shape[2] != self.exprdirs.shape[2]:
            raise ValueError("SmplxMesh: joint_dirs and exprdirs disagree about the number of expression coefficients")
        if self.n_dirs > MAX_DIRECTIONS:
            raise ValueError(f"SmplxMesh: {self.n_dirs} directions, the kernel takes {MAX_DIRECTIONS}")
        w = self.skin_index.shape[1] if self.skin_index.dim() == 2 else 0
        if self.skin_index.shape != self.skin_weight.shape or self.skin_index.shape[0] != v or not 1 <= w <= j:
            raise ValueError(f"SmplxMesh: skin lists are (V, W) with V = {v}, 1 <= W <= {j}, got {tuple(self.skin_index.shape)}, {tuple(self.skin_weight.shape)}")
        if int(self.skin_index.min()) < 0 or int(self.skin_index.max()) >= j:
            raise ValueError("SmplxMesh: a skin index outside the joints")
        self._on = {}

    n_subjects = property(lambda self: int(self.v_shaped.shape[0]))
    n_vertices = property(lambda self: int(self.v_shaped.shape[1]))
    n_expression = property(lambda self: int(self.exprdirs.shape[2]))
    n_dirs = property(lambda self: int(self.posedirs.shape[2] + self.exprdirs.shape[2]))
    width = property(lambda self: int(self.skin_index.shape[1]))

    def on(self, device):
        """dict(v_shaped, joint_dirs, skin_index, skin_weight, dirs) on `device`: moved once, `dirs` packed there by `syn_mesh_pack_dirs`."""
        key = str(torch.device(device))
        if key not in self._on:
            dev = torch.device(device)
            pd, ed = self.posedirs.to(dev), self.exprdirs.to(dev)
            e = self.n_expression
            packed = torch.empty(_round_up(self.n_vertices, MESH_VERTEX_BLOCK) * 3 * _round_up(self.n_dirs, DIR_GROUP), dtype=torch.float32, device=dev)
            _lib.check(_lib.load().syn_mesh_pack_dirs(pd.data_ptr(), ed.data_ptr() if e else None, self.n_vertices, pd.shape[2], e, packed.data_ptr(),
                                                      _lib.current_stream(dev)), "syn_mesh_pack_dirs")
            torch.cuda.current_stream(dev).synchronize()            # (pd and ed are dropped below)
            self._on[key] = dict(v_shaped=self.v_shaped.to(dev), joint_dirs=self.joint_dirs.to(dev) if e else None,
                                 skin_index=self.skin_index.to(dev), skin_weight=self.skin_weight.to(dev), dirs=packed)
        return self._on[key]


def smplx_mesh(npz_path_or_dict, betas, num_expression_coeffs: int = 100, flat_hand_mean: bool = False) -> SmplxMesh:
    """The mesh model of one or several subjects from an SMPL-X model file (SMPLX_NEUTRAL_2020.npz) or a dict with its arrays, as
    `smplx.create(..., num_betas=K, num_expression_coeffs=E, use_pca=False, flat_hand_mean=...)` builds it.  betas (K,) or (S, K), K <= 300.  All products
    on the host in fp64: v_shaped, the rest joints (`joints.smplx_rest_joints`), joint_dirs = J_regressor[:55] . shapedirs[:, :, 300:300 + E].  E = 0 is
    allowed (no expression input)."""
    m = np.load(npz_path_or_dict, allow_pickle=True) if isinstance(npz_path_or_dict, (str, bytes)) or hasattr(npz_path_or_dict, "__fspath__") \
        else npz_path_or_dict
    b = np.asarray(betas, dtype=np.float64)
    b = b.reshape(1, -1) if b.ndim <= 1 else b.reshape(b.shape[0], -1)
    e = int(num_expression_coeffs)
    shapedirs = np.asarray(m["shapedirs"], dtype=np.float64)
    if b.shape[1] > min(SHAPE_SPACE, shapedirs.shape[-1]):
        raise ValueError(f"smplx_mesh: {b.shape[1]} betas, the model has {min(SHAPE_SPACE, shapedirs.shape[-1])} shape directions")
    if e < 0 or (e > 0 and SHAPE_SPACE + e > shapedirs.shape[-1]):
        raise ValueError(f"smplx_mesh: {e} expression coefficients, the model file holds {max(0, shapedirs.shape[-1] - SHAPE_SPACE)}")
    skel = smplx_rest_joints(m, b, N_JOINTS, flat_hand_mean)
    v_shaped = np.asarray(m["v_template"], dtype=np.float64)[None] + np.einsum("vck,sk->svc", shapedirs[..., :b.shape[1]], b)
    exprdirs = shapedirs[..., SHAPE_SPACE:SHAPE_SPACE + e]
    reg = np.asarray(m["J_regressor"], dtype=np.float64)[:N_JOINTS]
    joint_dirs = np.einsum("jv,vce->jce", reg, exprdirs)
    weights = np.asarray(m["weights"], dtype=np.float64)[:, :N_JOINTS]
    if (weights.sum(1) == 0).any():
        raise ValueError(f"smplx_mesh: vertex {int(np.argmin(weights.sum(1) != 0))} has no skin weight on the {N_JOINTS} joints")
    idx, val = compact_weights(weights)
    posedirs = np.asarray(m["posedirs"], dtype=np.float64)
    posedirs = posedirs.reshape(posedirs.shape[0], 3, -1)[..., :9 * (N_JOINTS - 1)]
    return SmplxMesh(v_shaped, skel, joint_dirs, idx, val, posedirs, exprdirs, np.asarray(m["f"]) if "f" in m else None)


def smplx_vertices(model: SmplxMesh, pose: torch.Tensor, expression: torch.Tensor | None = None, transl: torch.Tensor | None = None,
                   take_of_frame: torch.Tensor | None = None, return_joints: bool = False):
    """pose (n, 165) axis-angle or (n, 330) 6D (global orient, 21 body joints, jaw, eyes, 15 + 15 hand joints: `test()`'s rec_pose); expression (n, E)
    or None (zero); transl (n, 3) or None -> vertices (n, V, 3), with return_joints=True also the 55 joints (n, 55, 3).  With several subjects in
    `model`, frame n uses subject take_of_frame[n] (int tensor (n,)), or n // (n / S) without one; a subject outside the model gives NaN.  6D rotations go
    through `poses.rotation_6d_to_axis_angle`, as test() takes them to axis-angle before SMPL-X (:621-624)."""
    engine._require_cuda(pose, "pose")
    sk = model.skeleton
    j, v, e = sk.n_joints, model.n_vertices, model.n_expression
    p = pose.detach().float().reshape(-1, pose.shape[-1])
    if p.shape[1] not in (3 * j, 6 * j):
        raise ValueError(f"smplx_vertices: poses are (n, {3 * j}) axis-angle or (n, {6 * j}) 6D, got {tuple(pose.shape)}")
    n, dev = p.shape[0], p.device
    out = torch.empty(n, v, 3, dtype=torch.float32, device=dev)
    jout = torch.empty(n, j, 3, dtype=torch.float32, device=dev)
    if n == 0:
        return (out, jout) if return_joints else out
    if p.shape[1] == 6 * j:
        from . import poses
        p = poses.rotation_6d_to_axis_angle(p.reshape(n, j, 6))
    p = p.reshape(n, j, 3).contiguous()
    ex = tr = tof = None
    if expression is not None and e > 0:
        engine._require_cuda(expression, "expression")
        ex = expression.detach().float().reshape(-1, expression.shape[-1]).contiguous()
        if tuple(ex.shape) != (n, e):
            raise ValueError(f"smplx_vertices: expression is (n, E) = ({n}, {e}), got {tuple(expression.shape)}")
    elif expression is not None and expression.numel():
        raise ValueError("smplx_vertices: the model was built without expression coefficients")
    if transl is not None:
        engine._require_cuda(transl, "transl")
        tr = transl.detach().float().reshape(-1, 3).contiguous()
        if tr.shape[0] != n:
            raise ValueError(f"smplx_vertices: transl is (n, 3) with n = {n}, got {tuple(transl.shape)}")
    per_take = n
    if take_of_frame is not None:
        engine._require_cuda(take_of_frame, "take_of_frame")
        tof = take_of_frame.detach().to(torch.int32).reshape(-1).contiguous()
        if tof.shape[0] != n:
            raise ValueError(f"smplx_vertices: take_of_frame is (n,) with n = {n}, got {tuple(take_of_frame.shape)}")
    elif model.n_subjects > 1:
        if n % model.n_subjects:
            raise ValueError(f"smplx_vertices: {n} frames do not split evenly over {model.n_subjects} subjects; pass take_of_frame")
        per_take = n // model.n_subjects
    parents, rest, mean = sk.on(dev)
    m = model.on(dev)
    kc = model.n_dirs
    feat = torch.empty(n, _round_up(kc, DIR_GROUP), dtype=torch.float32, device=dev)
    xf = torch.empty(n, j, 12, dtype=torch.float32, device=dev)
    lib, stream = _lib.load(), _lib.current_stream(dev)
    _lib.check(lib.syn_fk_transforms(parents.data_ptr(), j, rest.data_ptr(), model.n_subjects, p.data_ptr(), _lib.ptr(mean), _lib.ptr(m["joint_dirs"]),
                                     _lib.ptr(ex), e if ex is not None else 0, kc, _lib.ptr(tr), _lib.ptr(tof), per_take, n, feat.data_ptr(), xf.data_ptr(),
                                     jout.data_ptr(), stream), "syn_fk_transforms")
    _lib.check(lib.syn_mesh_vertices(m["dirs"].data_ptr(), v, kc, feat.data_ptr(), xf.data_ptr(), j, m["v_shaped"].data_ptr(), model.n_subjects,
                                     m["skin_index"].data_ptr(), m["skin_weight"].data_ptr(), model.width, _lib.ptr(tr), _lib.ptr(tof), per_take, n,
                                     out.data_ptr(), stream), "syn_mesh_vertices")
    return (out, jout) if return_joints else out
