"""Stick-figure videos of h3d takes: the scene of the reference's `utils/plot_script.py:86-177` (`plot_3d_motion`) - one perspective camera, one
translucent ground rectangle, the root's past trajectory and 5 or 15 polylines of given colour and width - as a software rasteriser of thick lines
in HIP (csrc/syn_plot.inc).  matplotlib and ffmpeg are not imported: the frames are drawn where the joints are and become a
Motion-JPEG AVI through `video.write_video`.

What is the reference's: the data preparation (`prepare`), the camera (`reference_camera`: axes limits, `view_init(120, -90)`, `dist` 5.5, focal
length 1, a 10 x 10 inch figure), the layers and their order, the chains, colours and widths.  The camera was checked against matplotlib 3.10 only
(tests/golden/plot_scene.npz); the reference was written for an older one.  What is this project's own: positions on a 1/16-pixel grid, thick
lines as capsules (round caps and joins - matplotlib's solid caps are "projecting", so a figure differs by half a width at the free end of a
chain), 16 samples per pixel, layers painted in list order (matplotlib sorts its artists by depth), no title (there is no text rendering).

Device tensors only, like the rest of the package: a CPU tensor or a missing library raises `SynHipError`."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, engine, video

SUBPIXEL = 16              # csrc/syn_plot.inc kSub: units per pixel
TILE = 32                  # kTile: pixels a side of a workgroup's tile
CHUNK = 256                # kChunk: records set up in the LDS at a time
WALK = 1024                # 256 kWalk: records a tile's workgroup tests per round of its walk over the frame's slots
MAX_DIM = 4096             # kMaxDim
MAX_R = 4095               # kMaxR
W_MIN = 0.0625             # kWMin: segments and the ground are cut at this w
GROUND_INTS = 24           # kGroundInts
EMPTY_RECORD = (0, 0, 0, 0, -1, 0, 1, 1)

SMPL_CHAINS = ((0, 2, 5, 8, 11), (0, 1, 4, 7, 10), (0, 3, 6, 9, 12, 15), (9, 14, 17, 19, 21), (9, 13, 16, 18, 20))
SMPLX_CHAINS = SMPL_CHAINS + tuple((21, k, k + 1, k + 2) for k in range(37, 52, 3)) + tuple((20, k, k + 1, k + 2) for k in range(22, 37, 3))
COLOURS = {"red": (255, 0, 0), "blue": (0, 0, 255), "black": (0, 0, 0), "darkblue": (0, 0, 139), "darkred": (139, 0, 0)}      # matplotlib's named colours
CHAIN_COLOURS = ("red", "blue", "black", "red", "blue") + ("darkblue",) * 5 + ("darkred",) * 5
TRAJECTORY_COLOUR, TRAJECTORY_PT = "blue", 1.0


def chain_width_pt(i: int) -> float:
    """The line width of chain i in points: 4 for the first five (the body), 2 for the fingers."""
    return 4.0 if i < 5 else 2.0


def half_width(pt: float, size: int) -> int:
    """R = max(1, rint(16 pt dpi / 72 / 2)) units of 1/16 pixel, dpi = size / 10 (a 10 inch figure)."""
    return max(1, int(np.rint(16.0 * pt * (size / 10.0) / 72.0 / 2.0)))


def reference_camera(size: int = 1000, radius: float = 4.0, elev: float = 120.0, azim: float = -90.0, dist: float = 5.5):
    """(M (4, 4), A (2, 3)) fp64: matplotlib's 3-D projection of `plot_3d_motion` and the map from projected (u, v) to pixel (col, row), row 0 on
    top, of a 10 x 10 inch figure of `size` pixels a side.  Axes limits x [-r/2, r/2], y [0, r], z [0, r]; box aspect 4 : 4 : 3 scaled by matplotlib's
    constant; the eye at `dist` from the box centre in direction (elev, azim), z vertical (pointing down, since |elev| > 90); focal length 1.  The 2-D
    side: subplot 111 of the default figure (left 0.125, right 0.9, bottom 0.11, top 0.88) shrunk to a square of 0.77, whose 2-D limits are
    [-0.095, 0.09] on both axes."""
    aspect = np.asarray([4.0, 4.0, 3.0])
    box = aspect * (1.8294640721620434 * 25 / 24 / np.linalg.norm(aspect))
    lim = np.asarray([[-radius / 2, radius / 2], [0.0, radius], [0.0, radius]], dtype=np.float64)
    d = (lim[:, 1] - lim[:, 0]) / box
    world = np.eye(4)
    world[[0, 1, 2], [0, 1, 2]] = 1 / d
    world[:3, 3] = -lim[:, 0] / d
    e, a = np.deg2rad(elev), np.deg2rad(azim)
    centre = 0.5 * box
    eye = centre + dist * np.asarray([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    w = eye - centre
    w = w / np.linalg.norm(w)
    wrapped = (elev + 180.0) % 360.0 - 180.0
    up = np.asarray([0.0, 0.0, -1.0 if abs(np.deg2rad(wrapped)) > np.pi / 2 else 1.0])
    u = np.cross(up, w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    rot, shift = np.eye(4), np.eye(4)
    rot[:3, :3] = [u, v, w]
    shift[:3, 3] = -eye
    zf, zb = -dist, dist
    persp = np.asarray([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, (zf + zb) / (zf - zb), -2 * (zf * zb) / (zf - zb)], [0, 0, -1.0, 0]])
    m = persp @ (rot @ shift) @ world
    scale = 0.77 * size / 0.185
    a2 = np.asarray([[scale, 0.0, scale * 0.095 + 0.1275 * size], [0.0, -scale, size - (scale * 0.095 + 0.11 * size)]])
    return m, a2


class Plot:
    """The camera, colours and widths of a stick-figure picture: chains (lists of joint indices; `SMPL_CHAINS` for 22 joints, `SMPLX_CHAINS` for
    52), size pixels a side (1 .. 4096; the reference's figure is 1000), radius the reference's axes range.  `segments` (S, 4) int32 {joint a,
    joint b, layer, half-width}: the chains' segments in list order, layer 2 + chain; `colours` (2 + chains,) int32 r | g << 8 | b << 16 per layer
    (0 the ground, 1 the trajectory).  camera=(M, A) replaces the reference's projection, half_widths (one per chain, units of 1/16 pixel) the
    reference's line widths."""

    def __init__(self, chains=SMPL_CHAINS, size: int = 1000, radius: float = 4.0, camera=None, half_widths=None):
        if int(size) != size or not 1 <= size <= MAX_DIM:
            raise ValueError(f"Plot: size is 1 to {MAX_DIM} pixels, got {size!r}")
        self.size, self.radius = int(size), float(radius)
        self.chains = tuple(tuple(int(j) for j in c) for c in chains)
        if not 1 <= len(self.chains) <= len(CHAIN_COLOURS) or any(len(c) < 2 or min(c) < 0 for c in self.chains):
            raise ValueError(f"Plot: 1 to {len(CHAIN_COLOURS)} chains of at least two joints each (the reference has colours for that many)")
        self.n_joints = max(max(c) for c in self.chains) + 1
        self.M, self.A = reference_camera(self.size, self.radius) if camera is None else (np.asarray(m, dtype=np.float64) for m in camera)
        if self.M.shape != (4, 4) or self.A.shape != (2, 3):
            raise ValueError(f"Plot: camera is (M (4, 4), A (2, 3)), got {self.M.shape} and {self.A.shape}")
        self.camera = np.concatenate([self.M.reshape(-1), self.A.reshape(-1)])
        widths = [half_width(chain_width_pt(i), self.size) for i in range(len(self.chains))] if half_widths is None else [int(r) for r in half_widths]
        if len(widths) != len(self.chains) or min(widths) < 1:
            raise ValueError("Plot: half_widths are one positive integer per chain")
        seg = [(c[k], c[k + 1], 2 + i, widths[i]) for i, c in enumerate(self.chains) for k in range(len(c) - 1)]
        self.segments = np.asarray(seg, dtype=np.int32)
        self.traj_half_width = half_width(TRAJECTORY_PT, self.size)
        rgb = [(128, 128, 128), COLOURS[TRAJECTORY_COLOUR]] + [COLOURS[CHAIN_COLOURS[i]] for i in range(len(self.chains))]
        self.colours = np.asarray([r | g << 8 | b << 16 for r, g, b in rgb], dtype=np.int32)
        if max(int(self.segments[:, 3].max()), self.traj_half_width) > min(MAX_R, SUBPIXEL * self.size):
            raise ValueError("Plot: a half-width beyond min(4095, 16 size) units")
        self._on = {}

    def on(self, device):
        """dict(segments, colours, camera) on `device`, moved once."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = str(dev)
        if key not in self._on:
            self._on[key] = dict(segments=torch.from_numpy(self.segments).to(dev), colours=torch.from_numpy(self.colours).to(dev),
                                 camera=torch.from_numpy(self.camera).to(dev))
        return self._on[key]


def prepare(joints):
    """`plot_script.py:115-132` on joints (n, J, 3), numpy or torch (on any device), in their own precision: (data, trajec, mins, maxs).  mins / maxs
    are the take's extremes BEFORE anything moves; then the lowest y goes to 0, trajec (n, 2) is the root's (x, z), and every frame is moved so that
    its root stands on x = z = 0."""
    if torch.is_tensor(joints):
        data = joints.detach().clone().reshape(len(joints), -1, 3)
        if data.shape[0] < 1 or data.shape[1] < 1:
            raise ValueError(f"plot.prepare: joints are (n, J, 3) with n, J >= 1, got {tuple(joints.shape)}")
        mins, maxs = data.amin(dim=(0, 1)), data.amax(dim=(0, 1))
        data[:, :, 1] -= mins[1]
        trajec = data[:, 0, [0, 2]].clone()
        data[..., 0] -= data[:, 0:1, 0].clone()
        data[..., 2] -= data[:, 0:1, 2].clone()
        return data, trajec, mins, maxs
    data = np.array(joints).reshape(len(joints), -1, 3)
    if data.shape[0] < 1 or data.shape[1] < 1:
        raise ValueError(f"plot.prepare: joints are (n, J, 3) with n, J >= 1, got {np.shape(joints)}")
    mins, maxs = data.min(axis=0).min(axis=0), data.max(axis=0).max(axis=0)
    data[:, :, 1] -= mins[1]
    trajec = data[:, 0, [0, 2]]
    data[..., 0] -= data[:, 0:1, 0].copy()
    data[..., 2] -= data[:, 0:1, 2].copy()
    return data, trajec, mins, maxs


def trajectory_segments(index: int) -> int:
    """Segments of the trajectory layer of frame `index`: the polyline trajec[:index], drawn for index > 1 - it ends one point short of the frame."""
    return max(0, int(index) - 1) if index > 1 else 0


class Records:
    """What `setup` left in its workspace for `paint`: records (m, n_slots, 8) int32 and grounds (m, 24) int32 are views of it."""

    def __init__(self, workspace, n_frames, n_slots):
        self.workspace, self.n_frames, self.n_slots = workspace, n_frames, n_slots
        cut = 32 * n_frames * n_slots
        self.records = workspace[:cut].view(torch.int32).view(n_frames, n_slots, 8)
        self.grounds = workspace[cut:].view(torch.int32).view(n_frames, GROUND_INTS)


def setup(p: Plot, data: torch.Tensor, trajec: torch.Tensor, mins, maxs, frames=None) -> Records:
    """`prepare`'s outputs on the device -> the frames' records (syn_plot_setup).  frames: indices into the take (None: all); a list, or an int32
    tensor on the device (nothing is read back, the slots are then sized for the longest trajectory the take can have - what a graph capture
    needs)."""
    engine._require_cuda(data, "data")
    engine._require_cuda(trajec, "trajec")
    if data.dim() != 3 or data.shape[2] != 3 or trajec.dim() != 2 or tuple(trajec.shape) != (data.shape[0], 2) or data.shape[0] < 1:
        raise ValueError(f"plot.draw: data is (n, J, 3) and trajec (n, 2) with n >= 1, got {tuple(data.shape)} and {tuple(trajec.shape)}")
    n, J, dev = int(data.shape[0]), int(data.shape[1]), data.device
    if J < p.n_joints:
        raise ValueError(f"plot.draw: the chains name joint {p.n_joints - 1}, the take has {J} joints")
    data, trajec = data.detach().float().contiguous(), trajec.detach().float().contiguous()
    S = len(p.segments)
    if torch.is_tensor(frames):
        engine._require_cuda(frames, "frames")
        if frames.dim() != 1 or frames.dtype != torch.int32:
            raise ValueError(f"plot.draw: frames on the device are (m,) int32, got {tuple(frames.shape)} {frames.dtype}")
        index, n_slots = frames.contiguous(), S + max(0, n - 2)
    else:
        picks = list(range(n)) if frames is None else [int(k) for k in frames]
        if any(k < 0 or k >= n for k in picks):
            raise ValueError(f"plot.draw: frames are indices into the take's {n} frames")
        index, n_slots = torch.tensor(picks, dtype=torch.int32, device=dev), S + max([trajectory_segments(k) for k in picks], default=0)
    m = int(index.numel())
    if m == 0:
        return Records(torch.empty(0, dtype=torch.uint8, device=dev), 0, n_slots)
    bounds = torch.stack([torch.as_tensor(mins)[0], torch.as_tensor(maxs)[0], torch.as_tensor(mins)[2], torch.as_tensor(maxs)[2]]).to(dev, torch.float32)
    drawn = data.index_select(0, index.long())
    lib, t = _lib.load(), p.on(dev)
    ws = torch.empty(lib.syn_plot_workspace_bytes(m, n_slots), dtype=torch.uint8, device=dev)
    _lib.check(lib.syn_plot_setup(drawn.data_ptr(), m, J, trajec.data_ptr(), n, index.data_ptr(), bounds.data_ptr(), t["segments"].data_ptr(), S,
                                  t["camera"].data_ptr(), p.size, p.traj_half_width, n_slots, ws.data_ptr(), _lib.current_stream(dev)), "syn_plot_setup")
    return Records(ws, m, n_slots)


def paint(p: Plot, r: Records) -> torch.Tensor:
    """The records -> rgb (m, size, size, 3) uint8 (syn_plot_draw)."""
    dev = r.workspace.device
    rgb = torch.empty(r.n_frames, p.size, p.size, 3, dtype=torch.uint8, device=dev)
    if r.n_frames:
        _lib.check(_lib.load().syn_plot_draw(r.workspace.data_ptr(), r.n_frames, r.n_slots, p.on(dev)["colours"].data_ptr(), len(p.colours), p.size,
                                             rgb.data_ptr(), _lib.current_stream(dev)), "syn_plot_draw")
    return rgb


def draw_prepared(p: Plot, data: torch.Tensor, trajec: torch.Tensor, mins, maxs, frames=None, return_records: bool = False):
    """`setup` then `paint`: rgb (m, size, size, 3) uint8.  return_records=True: (rgb, records (m, n_slots, 8) int32, grounds (m, 24) int32)."""
    r = setup(p, data, trajec, mins, maxs, frames)
    rgb = paint(p, r)
    return (rgb, r.records, r.grounds) if return_records else rgb


def draw(p: Plot, joints: torch.Tensor, frames=None):
    """joints (n, J, 3) on the device (what `joints.recover_from_ric` gives) -> rgb (m, size, size, 3) uint8 on the device: frame k of the picture
    `plot_3d_motion` shows.  frames: indices into the take, None for all of them (a long take is better fed in chunks, as the script does)."""
    engine._require_cuda(joints, "joints")
    data, trajec, mins, maxs = prepare(joints.float())
    return draw_prepared(p, data, trajec, mins, maxs, frames)


def plot_3d_motion(save_path, kinematic_tree, joints, title=None, fps=30, radius=4, size: int = 1000, wave=None, wave_sr: int = 16000, quality: int = 90,
                   chunk: int = 64, device=None) -> dict:
    """The reference's call (`h3d_diffusion_new_trainer.py:870-891`): joints (n, J, 3), numpy or torch, -> a Motion-JPEG AVI at `save_path`, every
    frame at `fps`.  `title` is ignored (no text rendering; the trainer passes 'None').  wave / wave_sr: an optional sound track, written at its own
    rate.  Returns `video.write_video`'s dict(frames, samples, bytes)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    j = (joints if torch.is_tensor(joints) else torch.from_numpy(np.ascontiguousarray(joints))).to(dev, torch.float32)
    j = j.reshape(len(j), -1, 3)
    p = Plot(kinematic_tree, size=size, radius=radius)
    data, trajec, mins, maxs = prepare(j)
    n, step = len(j), max(1, int(chunk))
    chunks = (draw_prepared(p, data, trajec, mins, maxs, range(k, min(n, k + step))) for k in range(0, n, step))
    return video.write_video(save_path, chunks, fps, wave=wave, wave_sr=wave_sr, quality=quality)
