"""Drawing the takes on the device: the scene of the reference's `utils/fast_render.py:16-43` - one mesh, one orthographic camera (`ymag` 1, pose
`create_pose_camera(-2)`), one directional light (`create_pose_light(-30)`), one uniform grey (220) on pyrender's white background - as a software
rasteriser in HIP (csrc/syn_render.inc).  An Instinct card has no graphics pipeline and `pyrender` is not imported.

Three stages, one call each: `project` (vertices -> screen positions snapped to 1/16 pixel, distance in front of the camera, smooth vertex normals),
`rasterize` (-> the covering face and its depth per pixel: integer edge functions, top-left fill rule, nearest fragment wins, ties to the lower
face index) and `shade` (-> uint8 RGB).  `render` chains them, `render_pair` puts two panels side by side as `write_images_from_queue` does.

What is the reference's: camera and light poses, `ymag`, the colour, the panel layout, the frame sampling (`frame_indices`), BMP as the image
type.  What is this project's own: the 1/16-pixel grid, and the tone - `base * min(1, ambient + diffuse * max(0, n . l))` is a Lambert term, NOT
pyrender's metallic-roughness shader, and will not match it pixel for pixel.  Coverage and depth follow the reference's camera; tone does not.  The
pixel mapping of the orthographic camera (ymag spans half the height, square pixels) is recalled from pyrender, not checked against it: pyrender is
not installed here.  The frames become a video with sound in syntalker_amd/video.py (Motion-JPEG AVI, PCM); H.264 / mp4 stay out, audio
resampling is syntalker_amd/audio.py (`load_wave`).

Device tensors only, like the rest of the package: a CPU tensor or a missing library raises `SynHipError`."""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib, engine

SUBPIXEL = 16              # csrc/syn_render.inc kSub: xy_sub units per pixel
SUPERTILE = 64             # kSuper: pixels a side of a workgroup's supertile
TILE_ROWS = 16             # kTileRows: a wave's tile is 64 x 16 pixels
RASTER_CHUNK = 256         # kChunk: faces set up in the LDS at a time; a supertile with more draws them in several chunks
RASTER_WALK = 1024         # 256 kWalk: face boxes a supertile's workgroup tests per round of its walk over the frame's faces
MAX_DIM = 8192             # kMaxDim
SENTINEL = -2 ** 31        # xy_sub of a vertex that is not finite
BASE_GREY = (220 / 255,) * 3


def _rot_x_pose(angle_deg, ty, tz):
    a = np.deg2rad(angle_deg)
    pose = np.eye(4)
    pose[1:3, 1:3] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    pose[1, 3], pose[2, 3] = ty, tz
    return pose


def reference_camera(angle_deg: float = -2.0):
    """The 4 x 4 camera pose of fast_render.py `create_pose_camera`: a turn about x by `angle_deg`, at (0, 1, 5), looking down its own -z."""
    return _rot_x_pose(angle_deg, 1.0, 5.0)


def reference_light(angle_deg: float = -30.0):
    """The 4 x 4 pose of fast_render.py `create_pose_light`: a turn about x by `angle_deg`, at (0, 0, 3); the light shines down its own -z, so the
    unit vector towards it is the pose's +z axis."""
    return _rot_x_pose(angle_deg, 0.0, 3.0)


def vertex_faces_csr(faces, n_vertices: int):
    """(offsets (V + 1,), incident (3 F,)) int32: vertex v's faces are incident[offsets[v]:offsets[v + 1]] in ascending face index (a face that names
    a vertex twice is listed once for it)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vert = f.reshape(-1)
    face = np.repeat(np.arange(len(f), dtype=np.int64), 3)
    pairs = np.unique(np.stack([vert, face], 1), axis=0)                    # sorted by vertex, then face
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    np.add.at(offsets, pairs[:, 0] + 1, 1)
    return np.cumsum(offsets).astype(np.int32), np.ascontiguousarray(pairs[:, 1].astype(np.int32))


class Scene:
    """The mesh's faces (F, 3) and everything about the picture that is not a vertex.  camera_pose / light_pose: 4 x 4 (defaults: the reference's);
    base: RGB in [0, 1]; background: RGB bytes.  The faces are validated and the vertex -> faces index is built here, once, on the host; `on(device)`
    moves faces, index and view matrix once."""

    def __init__(self, faces, n_vertices: int | None = None, camera_pose=None, ymag: float = 1.0, znear: float = 0.05, zfar: float = 100.0, light_pose=None,
                 base=BASE_GREY, background=(255, 255, 255), ambient: float = 0.3, diffuse: float = 0.7):
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"Scene: faces are (F, 3) integers with F >= 1, got {f.dtype} {f.shape}")
        f = f.astype(np.int64)
        v = int(f.max()) + 1 if n_vertices is None else int(n_vertices)
        if f.min() < 0 or f.max() >= v:
            raise ValueError(f"Scene: a face index outside the {v} vertices (faces span {int(f.min())} .. {int(f.max())})")
        if f.shape[0] > 2 ** 31 // 3:
            raise ValueError("Scene: too many faces")
        self.faces = np.ascontiguousarray(f.astype(np.int32))
        self.n_vertices, self.n_faces = v, int(f.shape[0])
        self.vf_offsets, self.vf_faces = vertex_faces_csr(self.faces, v)
        self.camera_pose = np.asarray(reference_camera() if camera_pose is None else camera_pose, dtype=np.float64).reshape(4, 4)
        self.light_pose = np.asarray(reference_light() if light_pose is None else light_pose, dtype=np.float64).reshape(4, 4)
        self.view = np.linalg.inv(self.camera_pose)[:3]                      # world -> camera, fp64 on the host
        z = self.light_pose[:3, 2]
        self.light = z / np.linalg.norm(z)
        if not ymag > 0 or not 0 <= znear < zfar:
            raise ValueError(f"Scene: ymag > 0 and 0 <= znear < zfar, got ymag {ymag}, znear {znear}, zfar {zfar}")
        self.ymag, self.znear, self.zfar = float(ymag), float(znear), float(zfar)
        self.base = tuple(float(c) for c in base)
        self.background = tuple(int(c) for c in background)
        if len(self.base) != 3 or len(self.background) != 3 or min(self.background) < 0 or max(self.background) > 255:
            raise ValueError("Scene: base is three floats, background three bytes")
        self.ambient, self.diffuse = float(ambient), float(diffuse)
        self._on = {}

    def on(self, device):
        """dict(faces, vf_offsets, vf_faces, view) on `device`, moved once."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())      # "cuda" and "cuda:0" are one entry
        key = str(dev)
        if key not in self._on:
            self._on[key] = dict(faces=torch.from_numpy(self.faces).to(dev), vf_offsets=torch.from_numpy(self.vf_offsets).to(dev),
                                 vf_faces=torch.from_numpy(self.vf_faces).to(dev),
                                 view=torch.from_numpy(np.ascontiguousarray(self.view, dtype=np.float32)).to(dev))
        return self._on[key]


def _check_image(width, height):
    if not (1 <= int(width) <= MAX_DIM and 1 <= int(height) <= MAX_DIM):
        raise ValueError(f"render: width and height are 1 to {MAX_DIM} pixels, got {width} x {height}")
    return int(width), int(height)


def _frames(scene: Scene, t: torch.Tensor, what: str, tail, dtype):
    engine._require_cuda(t, what)
    if t.dtype != dtype or tuple(t.shape[1:]) != tail or t.dim() != len(tail) + 1:
        raise ValueError(f"render: {what} is (n, {', '.join(str(d) for d in tail)}) {dtype}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def project(scene: Scene, vertices: torch.Tensor, width: int, height: int):
    """vertices (n, V, 3) world space -> xy_sub (n, V, 2) int32 = rint(16 x_pix), rint(16 y_pix) (SENTINEL for a vertex that is not finite), z (n, V)
    = the distance in front of the camera, normal (n, V, 3) the smooth vertex normal in world space."""
    engine._require_cuda(vertices, "vertices")
    width, height = _check_image(width, height)
    if vertices.dim() != 3 or tuple(vertices.shape[1:]) != (scene.n_vertices, 3):
        raise ValueError(f"render.project: vertices are (n, {scene.n_vertices}, 3), got {tuple(vertices.shape)}")
    v = vertices.detach().float().contiguous()
    n, dev = v.shape[0], v.device
    xy = torch.empty(n, scene.n_vertices, 2, dtype=torch.int32, device=dev)
    z = torch.empty(n, scene.n_vertices, dtype=torch.float32, device=dev)
    normal = torch.empty(n, scene.n_vertices, 3, dtype=torch.float32, device=dev)
    if n:
        s = scene.on(dev)
        _lib.check(_lib.load().syn_render_project(v.data_ptr(), n, scene.n_vertices, s["view"].data_ptr(), width, height, scene.ymag, s["faces"].data_ptr(),
                                                  scene.n_faces, s["vf_offsets"].data_ptr(), s["vf_faces"].data_ptr(), int(s["vf_faces"].numel()),
                                                  xy.data_ptr(), z.data_ptr(), normal.data_ptr(), _lib.current_stream(dev)), "syn_render_project")
    return xy, z, normal


def rasterize(scene: Scene, xy_sub: torch.Tensor, z: torch.Tensor, width: int, height: int):
    """xy_sub (n, V, 2) int32, z (n, V) -> face_id (n, H, W) int32 (-1: background), depth (n, H, W) float32 (+inf: background)."""
    width, height = _check_image(width, height)
    xy = _frames(scene, xy_sub, "xy_sub", (scene.n_vertices, 2), torch.int32)
    zz = _frames(scene, z, "z", (scene.n_vertices,), torch.float32)
    n, dev = xy.shape[0], xy.device
    if zz.shape[0] != n:
        raise ValueError(f"render.rasterize: {n} frames of xy_sub, {zz.shape[0]} of z")
    face_id = torch.empty(n, height, width, dtype=torch.int32, device=dev)
    depth = torch.empty(n, height, width, dtype=torch.float32, device=dev)
    if n:
        lib, s = _lib.load(), scene.on(dev)
        ws = torch.empty(lib.syn_render_workspace_bytes(n, scene.n_faces), dtype=torch.uint8, device=dev)
        _lib.check(lib.syn_render_raster(xy.data_ptr(), zz.data_ptr(), n, scene.n_vertices, s["faces"].data_ptr(), scene.n_faces, width, height, scene.znear,
                                         scene.zfar, ws.data_ptr(), face_id.data_ptr(), depth.data_ptr(), _lib.current_stream(dev)), "syn_render_raster")
    return face_id, depth


def shade(scene: Scene, face_id: torch.Tensor, xy_sub: torch.Tensor, normal: torch.Tensor):
    """face_id (n, H, W) int32, xy_sub (n, V, 2), normal (n, V, 3) -> rgb (n, H, W, 3) uint8."""
    engine._require_cuda(face_id, "face_id")
    if face_id.dim() != 3 or face_id.dtype != torch.int32:
        raise ValueError(f"render.shade: face_id is (n, H, W) int32, got {tuple(face_id.shape)} {face_id.dtype}")
    n, height, width = face_id.shape
    width, height = _check_image(width, height)
    xy = _frames(scene, xy_sub, "xy_sub", (scene.n_vertices, 2), torch.int32)
    nr = _frames(scene, normal, "normal", (scene.n_vertices, 3), torch.float32)
    if xy.shape[0] != n or nr.shape[0] != n:
        raise ValueError(f"render.shade: {n} frames of face_id, {xy.shape[0]} of xy_sub, {nr.shape[0]} of normal")
    dev = face_id.device
    rgb = torch.empty(n, height, width, 3, dtype=torch.uint8, device=dev)
    if n:
        s = scene.on(dev)
        _lib.check(_lib.load().syn_render_shade(face_id.contiguous().data_ptr(), xy.data_ptr(), nr.data_ptr(), n, scene.n_vertices, s["faces"].data_ptr(),
                                                scene.n_faces, width, height, *(float(c) for c in scene.light), *scene.base, scene.ambient, scene.diffuse,
                                                *scene.background, rgb.data_ptr(), _lib.current_stream(dev)), "syn_render_shade")
    return rgb


def render(scene: Scene, vertices: torch.Tensor, width: int = 960, height: int = 720, return_buffers: bool = False):
    """vertices (n, V, 3) -> rgb (n, H, W, 3) uint8 on the device; 960 x 720 is one panel of the reference's 1920 x 720 (`render_video_width // 2`).
    return_buffers=True: (rgb, dict(xy_sub, z, normal, face_id, depth))."""
    xy, z, normal = project(scene, vertices, width, height)
    face_id, depth = rasterize(scene, xy, z, width, height)
    rgb = shade(scene, face_id, xy, normal)
    return (rgb, dict(xy_sub=xy, z=z, normal=normal, face_id=face_id, depth=depth)) if return_buffers else rgb


def render_pair(scene: Scene, res_vertices: torch.Tensor, gt_vertices: torch.Tensor, width: int = 1920, height: int = 720):
    """Two panels of width // 2 side by side, the result on the left, as `write_images_from_queue` stacks them: (n, H, 2 (width // 2), 3) uint8."""
    if tuple(res_vertices.shape) != tuple(gt_vertices.shape):
        raise ValueError(f"render_pair: {tuple(res_vertices.shape)} result vertices, {tuple(gt_vertices.shape)} ground-truth vertices")
    panel = int(width) // 2
    return torch.cat([render(scene, res_vertices, panel, height), render(scene, gt_vertices, panel, height)], dim=2)


def frame_indices(n_frames: int, fps) -> list:
    """The frames the reference draws of a 30 fps take for a video of `fps` (`distribute_frames`): every max(1, int(30 // fps))-th."""
    step = max(1, int(30 // fps))
    return list(range(0, int(n_frames), step))


def write_bmp(path, image) -> None:
    """image (H, W, 3) uint8 RGB -> a 24-bit BMP (the reference's `render_tmp_img_filetype`): rows bottom-up, BGR, padded to 4 bytes."""
    img = np.asarray(image)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"write_bmp: image is (H, W, 3) uint8, got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    row = (3 * w + 3) // 4 * 4
    body = np.zeros((h, row), dtype=np.uint8)
    body[:, :3 * w] = img[::-1, :, ::-1].reshape(h, 3 * w)
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", 54 + row * h, 0, 0, 54))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, row * h, 2835, 2835, 0, 0))
        f.write(body.tobytes())
