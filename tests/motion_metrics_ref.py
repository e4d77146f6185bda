"""Restatements and seeded inputs for the motion-metric tests (test_motion_metrics_host.py, test_gpu_motion_metrics.py) and their fixture
(golden/make_motion_metrics_golden.py).

* `fk_oracle`: the joint transforms of linear blend skinning - G_j = G_parent . [R_j | rest_j - rest_parent] - in numpy at a chosen precision.
  `smplx` is not installed, so nothing can execute the reference's FK: THIS fp64 restatement is the FK oracle.  `fk_torch32` is the same chain in
  plain fp32 torch on the CPU; its error against the oracle is the yardstick E of the GPU gates.
* `speeds_ref`, `beats_ref`, `bc_ref`, `l1_ref`, `ric_ref`: utils/metric.py:98-127, 205-241, 12-27 and utils/plot_script.py:15-52 restated; the host
  test pins them to what the reference itself returned (golden/motion_metrics.npz), so they are oracles of known standing.
* `take_inputs`, `ric_inputs`: the fixture's inputs from seeds alone.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UPPER_BODY = [3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21]


def smplx_parents():
    return np.asarray(json.load(open(os.path.join(HERE, "golden", "smplx_kintree.json")))["parents"], dtype=np.int64)


# ---- forward kinematics ---------------------------------------------------------------------------------------------------------------
def aa_matrix(aa, dtype=np.float64):
    """(..., 3) axis-angle -> (..., 3, 3): Rodrigues with the unit axis, I at angle 0."""
    v = np.asarray(aa, dtype=dtype)
    t = np.sqrt((v * v).sum(-1))
    safe = np.where(t > 0, t, 1).astype(dtype)
    k = v / safe[..., None]
    x, y, z = k[..., 0], k[..., 1], k[..., 2]
    zero = np.zeros_like(x)
    K = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(v.shape[:-1] + (3, 3))
    s, c = np.sin(t)[..., None, None], np.cos(t)[..., None, None]
    return (np.eye(3, dtype=dtype) + s * K + (1 - c) * (K @ K)).astype(dtype)


def rot6d_matrix(d6, dtype=np.float64):
    """(..., 6) -> (..., 3, 3), rows b1, b2, b3 (utils/rotation_conversions.py:511-533)."""
    d = np.asarray(d6, dtype=dtype)
    a1, a2 = d[..., :3], d[..., 3:]
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(-1, keepdims=True)), 1e-12)
    b2 = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = b2 / np.maximum(np.sqrt((b2 * b2).sum(-1, keepdims=True)), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)], -2).astype(dtype)


def fk_oracle(parents, rest, rot, transl=None, take_of_frame=None, dtype=np.float64):
    """parents [J]; rest (J, 3) or (S, J, 3); rot (N, J, 3) axis-angle or (N, J, 6); transl (N, 3) -> joints (N, J, 3) in `dtype`."""
    rot = np.asarray(rot)
    R = (rot6d_matrix if rot.shape[-1] == 6 else aa_matrix)(rot, dtype)
    rest = np.asarray(rest, dtype=dtype)
    n, J = R.shape[0], len(parents)
    if rest.ndim == 3:
        tof = np.asarray(take_of_frame) if take_of_frame is not None else np.arange(n) // (n // rest.shape[0])
        rest = rest[tof]
    else:
        rest = np.broadcast_to(rest, (n, J, 3))
    GR, Gt = [None] * J, [None] * J
    for j, p in enumerate(parents):
        if p < 0:
            GR[j], Gt[j] = R[:, j], rest[:, j] + (0 if transl is None else np.asarray(transl, dtype=dtype))
        else:
            GR[j] = GR[p] @ R[:, j]
            Gt[j] = (GR[p] @ (rest[:, j] - rest[:, p])[..., None])[..., 0] + Gt[p]
    return np.stack(Gt, 1).astype(dtype)


def fk_torch32(parents, rest, rot, transl=None):
    """The same chain in plain fp32 torch on the CPU (axis-angle by Rodrigues with sin t / t and (1 - cos t) / t^2; 6D by Gram-Schmidt)."""
    import torch
    rot = torch.as_tensor(np.asarray(rot, dtype=np.float32))
    rest = torch.as_tensor(np.asarray(rest, dtype=np.float32))
    if rot.shape[-1] == 6:
        a1, a2 = rot[..., :3], rot[..., 3:]
        b1 = torch.nn.functional.normalize(a1, dim=-1)
        b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
        R = torch.stack([b1, b2, torch.cross(b1, b2, dim=-1)], -2)
    else:
        t = rot.norm(dim=-1)
        small = t < 1e-4
        ts = torch.where(small, torch.ones_like(t), t)
        a = torch.where(small, 1 - t * t / 6, torch.sin(ts) / ts)[..., None, None]
        b = torch.where(small, 0.5 - t * t / 24, (1 - torch.cos(ts)) / (ts * ts))[..., None, None]
        x, y, z = rot[..., 0], rot[..., 1], rot[..., 2]
        zero = torch.zeros_like(x)
        K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(rot.shape[:-1] + (3, 3))
        R = torch.eye(3) + a * K + b * (K @ K)
    GR, Gt = [None] * len(parents), [None] * len(parents)
    for j, p in enumerate(parents):
        if p < 0:
            GR[j], Gt[j] = R[:, j], rest[j] + (0 if transl is None else torch.as_tensor(np.asarray(transl, dtype=np.float32)))
            Gt[j] = Gt[j].expand(R.shape[0], 3)
        else:
            GR[j] = GR[p] @ R[:, j]
            Gt[j] = (GR[p] @ (rest[j] - rest[p])[:, None])[..., 0] + Gt[p]
    return torch.stack(Gt, 1).numpy()


# ---- utils/metric.py restated -------------------------------------------------------------------------------------------------------
def speeds_ref(joints, fps, mmae=None, dtype=np.float64):
    """(n, J * 3) -> (n, J): metric.py:97-109."""
    x = np.asarray(joints, dtype=dtype).reshape(len(joints), -1, 3)
    d = np.concatenate([x[1:2] - x[:1], (x[2:] - x[:-2]) / 2, x[-1:] - x[-2:-1]], 0) * dtype(fps)
    v = np.sqrt((d * d).sum(-1))
    return v if mmae is None else v / np.asarray(mmae, dtype=dtype)


def beats_ref(vel, t_start, t_end, order, threshold=0.3, corrected=False):
    """(n, J) speeds -> (n_slice, J) uint8: strict local minima of the slice over `order` neighbours a side, indices clipped to the slice, kept
    where vel[j] > threshold - `corrected`: where vel[j + t_start] > threshold, the rule the reference does NOT implement."""
    vel = np.asarray(vel)
    s = vel[t_start:t_end]
    m, idx = len(s), np.arange(len(s))
    ok = np.ones(s.shape, dtype=bool)
    for k in range(1, order + 1):
        ok &= (s < s[np.clip(idx + k, 0, m - 1)]) & (s < s[np.clip(idx - k, 0, m - 1)])
    above = (vel[t_start:t_end] if corrected else vel[:m]) > threshold
    return (ok & above).astype(np.uint8)


def bc_ref(mask, onsets, upper_body, pose_fps, sigma):
    """(n_slice, J) beat mask, onset times -> (per joint of upper_body, their mean): metric.py:205-241 in fp64."""
    onsets = np.asarray(onsets, dtype=np.float64)
    per = []
    for i in upper_body:
        t = np.nonzero(mask[:, i])[0] / pose_fps
        per.append(0.0 if t.size == 0 else float(np.exp(-np.abs(t[None] - onsets[:, None]).min(1) ** 2 / (2 * sigma ** 2)).sum() / onsets.size))
    return np.asarray(per), float(sum(per) / len(per))


def l1_ref(x):
    """sum |x - mean over rows| in fp64 (metric.py:16-22 without the overwrite)."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(x - x.mean(0)).sum())


def l1_ref_f32(x):
    """metric.py:16-22 as written, on a float32 copy: the reference's own number."""
    r = np.array(x, dtype=np.float32)
    mean = np.mean(r, 0)
    for i in range(r.shape[0]):
        r[i, :] = abs(r[i, :] - mean)
    return float(np.sum(r))


# ---- utils/plot_script.py:15-52 restated ----------------------------------------------------------------------------------------------
def ric_ref(data, joints_num, dtype=np.float64):
    """(B, n, C) -> (B, n, joints_num, 3): the yaw as the exclusive prefix sum of channel 0, the quaternion (cos a, 0, sin a, 0) inverted, qrot."""
    d = np.asarray(data, dtype=dtype)
    ang = np.zeros(d.shape[:-1], dtype=dtype)
    ang[..., 1:] = d[..., :-1, 0]
    ang = np.cumsum(ang, -1, dtype=dtype)
    c, q = np.cos(ang), -np.sin(ang)                       # qinv: the vector part (0, sin a, 0) negated

    def rot(x, z, c, q):
        uvx, uvz = q * z, -(q * x)
        uuvx, uuvz = q * uvz, -(q * uvx)
        return x + 2 * (c * uvx + uuvx), z + 2 * (c * uvz + uuvz)
    vx, vz = np.zeros_like(ang), np.zeros_like(ang)
    vx[..., 1:], vz[..., 1:] = d[..., :-1, 1], d[..., :-1, 2]
    px, pz = rot(vx, vz, c, q)
    rx, rz = np.cumsum(px, -1, dtype=dtype), np.cumsum(pz, -1, dtype=dtype)
    loc = d[..., 4:4 + 3 * (joints_num - 1)].reshape(d.shape[:-1] + (joints_num - 1, 3))
    jx, jz = rot(loc[..., 0], loc[..., 2], c[..., None], q[..., None])
    pos = np.stack([jx + rx[..., None], loc[..., 1], jz + rz[..., None]], -1)
    root = np.stack([rx, d[..., 3], rz], -1)
    return np.concatenate([root[..., None, :], pos], -2).astype(dtype)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def synth_rest(seed=0, parents=None):
    """Plausible rest joints for a tree: every joint 5 - 25 cm from its parent in a seeded direction."""
    parents = smplx_parents() if parents is None else parents
    r = np.random.RandomState(seed)
    rest = np.zeros((len(parents), 3))
    for j, p in enumerate(parents):
        d = r.randn(3)
        rest[j] = (rest[p] if p >= 0 else 0) + d / np.linalg.norm(d) * r.uniform(0.05, 0.25)
    return rest.astype(np.float32)


def smooth_rotations(seed, n, joints=55, amp=0.35, max_cycles=3.0, fps=30.0):
    """Band-limited noise: (n, joints, 3) axis-angle, each channel a sum of 4 sinusoids of at most `max_cycles` Hz with seeded phases."""
    r = np.random.RandomState(seed)
    t = np.arange(n)[:, None, None, None] / fps
    f = r.uniform(0.2, max_cycles, (1, joints, 3, 4))
    ph = r.uniform(0, 2 * np.pi, (1, joints, 3, 4))
    a = r.uniform(0.2, 1.0, (1, joints, 3, 4)) * amp / 2
    return (a * np.sin(2 * np.pi * f * t + ph)).sum(-1).astype(np.float32)


def ric_inputs(b, n, channels, seed):
    """HumanML3D-like features: small yaw and root velocities, metre-scale local joints."""
    r = np.random.RandomState(seed)
    x = r.randn(b, n, channels).astype(np.float32)
    x[..., 0] *= 0.05
    x[..., 1:3] *= 0.03
    x[..., 3] = 0.9 + 0.02 * x[..., 3]
    x[..., 4:] *= 0.4
    return x


RIC_CASES = {"b1_n1": (1, 1, 623, 52, 11), "b1_n2": (1, 2, 623, 52, 12), "b3_n196": (3, 196, 263, 22, 13), "b1_n257": (1, 257, 623, 52, 14)}   # (B, n, C, joints, seed)
