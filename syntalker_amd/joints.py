"""Skeleton joints on the device: what the reference's `test()` asks of SMPL-X (diffusion_rvqvae_trainer.py:626-638, 668) and what its h3d
`test()` asks of `recover_from_ric` (h3d_diffusion_new_trainer.py:877, utils/plot_script.py:15-52).

All the metrics take from `smplx(...)["joints"]` is its first 55 entries - the skeleton joints.  SMPL-X regresses them from the SHAPED template
(before the pose correctives), and `test()` passes zero expression and zero transl, so they are forward kinematics over the 55-joint tree from one
set of rest joints per subject: `smplx_rest_joints` is that one host product (numpy, no `smplx` import), `forward_kinematics` the tree walk
(`syn_fk_joints`, csrc/syn_joints.inc).  One more thing SMPL-X does to the pose is kept: a model built with `flat_hand_mean=False` - the library's
default, and what the reference's `smplx.create(..., use_pca=False)` gives - adds the hands' mean pose to the axis-angle vector of the 30 hand
joints (`full_pose += pose_mean`); `smplx_rest_joints` reads it from the model file (`hands_meanl` / `hands_meanr`) into `Skeleton.pose_mean`.
The vertices and the face losses are `syntalker_amd/mesh.py` (which runs `syn_fk_joints`' kernel for its joint transforms); the pictures are
`syntalker_amd/render.py`, the video with its sound track (Motion-JPEG AVI, PCM) `syntalker_amd/video.py`, audio resampling `syntalker_amd/audio.py`; H.264 / mp4 stay out.  Device tensors only, like the rest of the package: a CPU tensor or a missing library raises."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, engine

MAX_JOINTS = 64          # csrc/syn_joints.inc kMaxJ
FK_FRAME_TILE = 8        # csrc/syn_joints.inc kFkFrames: frames per workgroup
RIC_SCAN_TILE = 256      # csrc/syn_joints.inc kRicTile: frames per scan step


class Skeleton:
    """A joint tree and its rest joints.  parents [J]: every parent an earlier joint, roots -1.  rest_joints (J, 3), or (S, J, 3): one set per take
    (subject) of a batched call.  pose_mean (J, 3) or None: an axis-angle vector per joint that is ADDED to the pose's before it becomes a rotation
    (SMPL-X's `pose_mean`: zero except for the hands of a model without `flat_hand_mean`)."""

    def __init__(self, parents, rest_joints, pose_mean=None):
        p = np.asarray(parents).astype(np.int64).reshape(-1)
        if not 1 <= p.size <= MAX_JOINTS:
            raise ValueError(f"Skeleton: 1 to {MAX_JOINTS} joints, got {p.size}")
        for j, q in enumerate(p):
            if not (q == -1 or 0 <= q < j):
                raise ValueError(f"Skeleton: parents must be topologically ordered with roots at -1; joint {j} has parent {int(q)}")
        r = torch.as_tensor(np.asarray(rest_joints) if not torch.is_tensor(rest_joints) else rest_joints).detach().float()
        if r.dim() == 2:
            r = r[None]
        if r.dim() != 3 or r.shape[1:] != (p.size, 3):
            raise ValueError(f"Skeleton: rest joints are (J, 3) or (S, J, 3) with J = {p.size}, got {tuple(r.shape)}")
        self.parents = p.astype(np.int32)
        self.rest_joints = r.contiguous()
        self.pose_mean = None
        if pose_mean is not None:
            m = torch.as_tensor(np.asarray(pose_mean, dtype=np.float32) if not torch.is_tensor(pose_mean) else pose_mean).detach().float().reshape(-1)
            if m.numel() != 3 * p.size:
                raise ValueError(f"Skeleton: pose_mean is (J, 3) with J = {p.size}, got {m.numel()} values")
            if bool((m != 0).any()):
                self.pose_mean = m.reshape(p.size, 3).contiguous()
        self._on = {}

    @property
    def n_joints(self) -> int:
        return int(self.parents.size)

    @property
    def n_takes(self) -> int:
        return int(self.rest_joints.shape[0])

    def on(self, device):
        """(parents, rest_joints, pose_mean or None) on `device`, moved once."""
        key = str(torch.device(device))
        if key not in self._on:
            self._on[key] = (torch.from_numpy(self.parents).to(device), self.rest_joints.to(device),
                             None if self.pose_mean is None else self.pose_mean.to(device))
        return self._on[key]


def smplx_rest_joints(npz_path_or_dict, betas, n_joints: int = 55, flat_hand_mean: bool = False) -> Skeleton:
    """The skeleton of one or several subjects from an SMPL-X model file (SMPLX_NEUTRAL_2020.npz) or a dict with its arrays: rest joints
    J_regressor @ (v_template + shapedirs[..., :len(betas)] @ betas) on the host in numpy (fp64), parents from kintree_table[0], the first
    `n_joints` joints.  betas (K,) or (S, K).  flat_hand_mean=False (smplx's default, the reference's setting): the model's `hands_meanl` /
    `hands_meanr` (45 values each) become the mean pose of joints 25..39 / 40..54, as `SMPLX.__init__` puts them into `pose_mean` with
    `use_pca=False`; True, or a model without these arrays: no mean pose."""
    m = np.load(npz_path_or_dict, allow_pickle=True) if isinstance(npz_path_or_dict, (str, bytes)) or hasattr(npz_path_or_dict, "__fspath__") \
        else npz_path_or_dict
    b = np.asarray(betas, dtype=np.float64)
    b = b.reshape(1, -1) if b.ndim <= 1 else b.reshape(b.shape[0], -1)
    shapedirs = np.asarray(m["shapedirs"], dtype=np.float64)
    if b.shape[1] > shapedirs.shape[-1]:
        raise ValueError(f"smplx_rest_joints: {b.shape[1]} betas, the model has {shapedirs.shape[-1]} shape directions")
    v = np.asarray(m["v_template"], dtype=np.float64)[None] + np.einsum("vck,sk->svc", shapedirs[..., :b.shape[1]], b)
    reg = np.asarray(m["J_regressor"], dtype=np.float64)[:n_joints]
    rest = np.einsum("jv,svc->sjc", reg, v)
    par = np.asarray(m["kintree_table"])[0][:n_joints].astype(np.int64)
    par = np.where((par < 0) | (par >= n_joints), -1, par)          # (the files store the root's parent as 2^32 - 1)
    mean = None
    if not flat_hand_mean and n_joints == 55 and "hands_meanl" in m and "hands_meanr" in m:
        mean = np.zeros((55, 3))
        mean[25:40] = np.asarray(m["hands_meanl"], dtype=np.float64).reshape(15, 3)
        mean[40:55] = np.asarray(m["hands_meanr"], dtype=np.float64).reshape(15, 3)
    return Skeleton(par, rest.astype(np.float32), mean)


def forward_kinematics(skel: Skeleton, rot: torch.Tensor, transl: torch.Tensor | None = None, take_of_frame: torch.Tensor | None = None) -> torch.Tensor:
    """rot (N, J, 3) axis-angle or (N, J, 6) -> joints (N, J, 3): G_j = G_parent . [R_j | rest_j - rest_parent], the root at rest_0 (+ transl (N, 3)).
    With several takes in `skel`, frame n uses rest joints take_of_frame[n] (int tensor (N,)), or n // (N / S) without one.  `skel.pose_mean` is added
    to the axis-angle vectors first; 6D rotations then go through `poses.rotation_6d_to_axis_angle`, as test() takes them to axis-angle before
    SMPL-X (:621-622)."""
    engine._require_cuda(rot, "joint rotations")
    j = skel.n_joints
    if rot.dim() != 3 or rot.shape[1] != j or rot.shape[2] not in (3, 6):
        raise ValueError(f"forward_kinematics: rotations are (N, {j}, 3) or (N, {j}, 6), got {tuple(rot.shape)}")
    x = rot.detach().float().contiguous()
    n, dev = x.shape[0], x.device
    out = torch.empty(n, j, 3, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    parents, rest, mean = skel.on(dev)
    if mean is not None and x.shape[2] == 6:
        from . import poses
        x = poses.rotation_6d_to_axis_angle(x)
    tr = tof = None
    if transl is not None:
        engine._require_cuda(transl, "transl")
        tr = transl.detach().float().reshape(-1, 3).contiguous()
        if tr.shape[0] != n:
            raise ValueError(f"forward_kinematics: transl is (N, 3) with N = {n}, got {tuple(transl.shape)}")
    per_take = n
    if take_of_frame is not None:
        engine._require_cuda(take_of_frame, "take_of_frame")
        tof = take_of_frame.detach().to(torch.int32).reshape(-1).contiguous()
        if tof.shape[0] != n:
            raise ValueError(f"forward_kinematics: take_of_frame is (N,) with N = {n}, got {tuple(take_of_frame.shape)}")
    elif skel.n_takes > 1:
        if n % skel.n_takes:
            raise ValueError(f"forward_kinematics: {n} frames do not split evenly over {skel.n_takes} takes; pass take_of_frame")
        per_take = n // skel.n_takes
    _lib.check(_lib.load().syn_fk_joints(parents.data_ptr(), j, rest.data_ptr(), skel.n_takes, x.data_ptr(), int(x.shape[2] == 6), _lib.ptr(tr),
                                         _lib.ptr(tof), per_take, n, _lib.ptr(mean), out.data_ptr(), _lib.current_stream(dev)), "syn_fk_joints")
    return out


def smplx_joints(skel: Skeleton, pose: torch.Tensor, transl: torch.Tensor | None = None) -> torch.Tensor:
    """pose (n, 165) axis-angle or (n, 330) 6D (or with a leading batch of 1) -> (n, 165): `test()`'s `joints_rec`, the first 55 of
    smplx(...)["joints"] flattened per frame."""
    p = pose.reshape(-1, pose.shape[-1])
    j = skel.n_joints
    if p.shape[1] not in (3 * j, 6 * j):
        raise ValueError(f"smplx_joints: poses are (n, {3 * j}) axis-angle or (n, {6 * j}) 6D, got {tuple(pose.shape)}")
    return forward_kinematics(skel, p.reshape(p.shape[0], j, p.shape[1] // j), transl).reshape(p.shape[0], 3 * j)


def _takes(joints: torch.Tensor, what: str):
    """(n, J * 3), (n, J, 3) or (T, n, J, 3) -> contiguous fp32 (T, n, J, 3) and whether a take dimension was given."""
    engine._require_cuda(joints, what)
    x = joints.detach().float()
    if x.dim() == 2:
        if x.shape[1] % 3:
            raise ValueError(f"{what}: (n, J * 3) needs a multiple of 3 channels, got {tuple(joints.shape)}")
        x = x.reshape(x.shape[0], -1, 3)
    if x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError(f"{what}: (n, J * 3), (n, J, 3) or (T, n, J, 3), got {tuple(joints.shape)}")
    return (x[None] if x.dim() == 3 else x).contiguous(), x.dim() == 4


def joint_speed(joints: torch.Tensor, fps: float = 30.0, mmae=None) -> torch.Tensor:
    """Per-joint speeds (utils/metric.py:98-109): forward / central / backward differences times fps, Euclidean norm, optionally divided by
    mmae (J,).  joints (n, J * 3) | (n, J, 3) -> (n, J); (T, n, J, 3) -> (T, n, J), differences within each take."""
    x, batched = _takes(joints, "joints")
    t, n, j, _ = x.shape
    if n < 2:
        raise ValueError(f"joint_speed: the differences need at least 2 frames, got {n}")
    mm = None
    if mmae is not None:
        mm = torch.as_tensor(np.asarray(mmae, dtype=np.float32) if not torch.is_tensor(mmae) else mmae).detach().float().reshape(-1).to(x.device).contiguous()
        if mm.shape[0] != j:
            raise ValueError(f"joint_speed: mmae has {mm.shape[0]} entries for {j} joints")
    out = torch.empty(t, n, j, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().syn_joint_speed(x.data_ptr(), t, n, j, float(fps), _lib.ptr(mm), out.data_ptr(), _lib.current_stream(x.device)), "syn_joint_speed")
    return out if batched else out[0]


def mean_joint_speed(joints: torch.Tensor, fps: float = 30.0) -> torch.Tensor:
    """(J,): the speeds of `joint_speed` without a divisor, averaged over the frames (and takes) - a take's share of the reference's
    `mean_vel_*.npy` (dataloaders/beat_sep_lower.py:182-197)."""
    v = joint_speed(joints, fps)
    return v.reshape(-1, v.shape[-1]).mean(0)


def _recover(data: torch.Tensor, joints_num: int, want_quat: bool):
    engine._require_cuda(data, "HumanML3D features")
    if data.dim() < 2:
        raise ValueError(f"recover_from_ric: features are (..., n, C), got {tuple(data.shape)}")
    x = data.detach().float().contiguous()
    lead, n, c = x.shape[:-2], x.shape[-2], x.shape[-1]
    if c < 4 + 3 * (joints_num - 1) or joints_num < 1:
        raise ValueError(f"recover_from_ric: {joints_num} joints need {4 + 3 * (joints_num - 1)} channels, got {c}")
    b = int(np.prod(lead)) if lead else 1
    out = torch.empty(*lead, n, joints_num, 3, dtype=torch.float32, device=x.device)
    quat = torch.empty(*lead, n, 4, dtype=torch.float32, device=x.device) if want_quat else None
    if b * n:
        _lib.check(_lib.load().syn_recover_from_ric(x.data_ptr(), b, n, c, joints_num, out.data_ptr(), _lib.ptr(quat), _lib.current_stream(x.device)),
                   "syn_recover_from_ric")
    return out, quat


def recover_root_rot_pos(data: torch.Tensor):
    """utils/plot_script.py:15-34: (r_rot_quat (..., n, 4), r_pos (..., n, 3)) of HumanML3D features (..., n, C >= 4)."""
    out, quat = _recover(data, 1, True)
    return quat, out[..., 0, :]


def recover_from_ric(data: torch.Tensor, joints_num: int) -> torch.Tensor:
    """utils/plot_script.py:37-52: HumanML3D features (..., n, C >= 4 + 3 (joints_num - 1)) -> joint positions (..., n, joints_num, 3)."""
    return _recover(data, int(joints_num), False)[0]
