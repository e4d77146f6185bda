"""The renderer's restatement (tests/render_ref.py) and the host side of syntalker_amd/render.py, without a GPU: the fill rule on cases counted by
hand, the camera and light of the reference, the vertex -> faces index, the frame sampling, the BMP writer, and the C ABI's declarations."""
import os
import re
import struct

import numpy as np
import pytest

from tests import render_ref as rr

from syntalker_amd import _lib, render

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def px(points):
    """Pixel-corner coordinates -> xy_sub."""
    return np.asarray(points, dtype=np.int64) * rr.SUB


# ---- the fill rule ----------------------------------------------------------------------------------------------------------------------------------
def test_right_triangle_on_pixel_corners_covers_the_counted_samples():
    # corners (0, 0), (8, 0), (0, 8): sample (i + 1/2, j + 1/2) is strictly inside for i + j <= 6 (28 samples); the 8 samples with i + j = 7 lie ON
    # the hypotenuse, which is a right / bottom edge of this triangle: not covered
    count = rr.coverage_count(px([(0, 0), (8, 0), (0, 8)]), [[0, 1, 2]], 10, 10)
    i, j = np.meshgrid(np.arange(10), np.arange(10))
    assert np.array_equal(count, (i + j <= 6).astype(int)) and count.sum() == 28
    assert np.array_equal(count, rr.coverage_count(px([(0, 0), (8, 0), (0, 8)]), [[0, 2, 1]], 10, 10))          # either winding
    # the other half of the square: the hypotenuse is its top-left edge, the 8 samples on it belong to it
    other = rr.coverage_count(px([(8, 8), (0, 8), (8, 0)]), [[0, 1, 2]], 10, 10)
    assert np.array_equal(other, ((i + j >= 7) & (i < 8) & (j < 8)).astype(int)) and other.sum() == 36
    # samples on the left and top edges (x = 0 / y = 0 through pixel centres) are covered, on the right and bottom edges not
    half = rr.coverage_count(px([(0, 0), (4, 0), (4, 4), (0, 4)]) + 8, rr.quad_faces(), 6, 6)
    want = np.zeros((6, 6), dtype=int)
    want[0:4, 0:4] = 1
    assert np.array_equal(half, want)


@pytest.mark.parametrize("flip", [False, True])
def test_quad_whose_diagonal_runs_through_pixel_centres_covers_each_sample_once(flip):
    count = rr.coverage_count(px([(1, 1), (9, 1), (9, 9), (1, 9)]), rr.quad_faces(flip), 11, 11)
    want = np.zeros((11, 11), dtype=int)
    want[1:9, 1:9] = 1
    assert np.array_equal(count, want)
    fid, depth = rr.rasterize_ref(px([(1, 1), (9, 1), (9, 9), (1, 9)])[None], np.full((1, 4), 2.0, np.float32), rr.quad_faces(flip), 11, 11)
    assert np.array_equal(fid >= 0, want[None] == 1) and (depth[fid >= 0] == 2.0).all() and np.isinf(depth[fid < 0]).all()
    assert set(np.unique(fid)) == {-1, 0, 1}


def test_closed_convex_mesh_covers_every_sample_zero_or_two_times():
    v, f = rr.uv_sphere(16, 10, (0.1, 1.0, 0.0), 0.12)
    assert v.shape == (146, 3) and f.shape == (288, 3)
    view = rr.view_of(rr.camera_pose())
    xy, z, normal = rr.project_ref(v[None], f, view, 128, 96)
    count = rr.coverage_count(xy[0], f, 128, 96)
    covered = int((count > 0).sum())
    print(f"sphere at 128 x 96: cover counts {sorted(set(count.reshape(-1)))}, {covered} covered pixels")
    assert set(count.reshape(-1)) == {0, 2}
    assert covered == 103
    # fp32 snapping (the device's chain: fma dot products, then the pixel scale) agrees with fp64 on every vertex here
    v32, m32 = v.astype(np.float32), view.astype(np.float32)
    cam = v32 @ m32[:, :3].T + m32[:, 3]
    s = np.float32(48.0)
    xy32 = np.stack([np.rint(np.float32(16) * (np.float32(64) + cam[:, 0] * s)), np.rint(np.float32(16) * (np.float32(48) - cam[:, 1] * s))], -1)
    assert np.array_equal(xy32.astype(np.int64), xy[0])
    # outward normals of a sphere point away from its centre (a coarse, diagonally split grid: within 8 degrees); the depth is the distance along
    # the camera's axis
    assert ((normal[0] * (v - [0.1, 1.0, 0.0]) / 0.12).sum(-1) > 0.99).all() and np.allclose(np.linalg.norm(normal[0], axis=-1), 1.0)
    assert np.abs(z[0] - 5.0).max() < 0.2


def test_nearer_fragment_wins_and_ties_go_to_the_lower_face():
    quad = px([(0, 0), (4, 0), (4, 4), (0, 4)])
    xy = np.concatenate([quad, quad, quad])[None]
    faces = np.concatenate([rr.quad_faces() + 8, rr.quad_faces(), rr.quad_faces() + 4]).astype(np.int32)       # faces 0, 1 far; 2, 3 and 4, 5 near, equal depth
    z = np.asarray([[1.0] * 8 + [3.0] * 4], dtype=np.float32)
    fid, depth = rr.rasterize_ref(xy, z, faces, 4, 4)
    assert set(np.unique(fid)) == {2, 3} and (depth == 1.0).all()
    fid, depth = rr.rasterize_ref(xy, z, faces, 4, 4, znear=2.0)            # the near quads are clipped away
    assert set(np.unique(fid)) == {0, 1} and (depth == 3.0).all()
    fid, _ = rr.rasterize_ref(xy, z, faces, 4, 4, znear=1.5, zfar=2.5)
    assert (fid == -1).all()


def test_dropped_faces():
    w = h = 8
    g = rr.SUB * 8
    assert rr.oriented(px([(0, 0), (4, 4), (8, 8)]), [0, 1, 2], w, h) is None                              # zero area
    assert rr.oriented(px([(0, 0), (4, 0), (4, 0)]), [0, 1, 2], w, h) is None
    assert rr.oriented(np.asarray([(0, 0), (64, 0), (rr.SENTINEL, rr.SENTINEL)]), [0, 1, 2], w, h) is None    # a vertex that is not finite
    assert rr.oriented(np.asarray([(-g - 1, 0), (64, 0), (0, 64)]), [0, 1, 2], w, h) is None               # just outside the guard band
    inside = rr.oriented(np.asarray([(-g, 0), (64, 0), (0, 64)]), [0, 1, 2], w, h)
    assert inside is not None and inside[3] > 0
    assert rr.oriented(px([(0, 0), (0, 8), (8, 0)]), [0, 1, 2], w, h)[4] == [0, 2, 1]                      # oriented: vertices 1 and 2 swapped


def test_shade_ref_background_and_lambert_term():
    quad = px([(0, 0), (4, 0), (4, 4), (0, 4)])[None]
    fid, _ = rr.rasterize_ref(quad, np.ones((1, 4), np.float32), rr.quad_faces(), 6, 4)
    light = rr.light_of(rr.light_pose())
    assert np.allclose(light, [0.0, 0.5, np.sqrt(0.75)])
    towards = np.broadcast_to(light, (1, 4, 3))
    img = rr.shade_ref(fid, quad, towards, rr.quad_faces(), light)
    assert (img[0, :, 4:] == 255).all() and np.allclose(img[0, :, :4], 220.0)                 # full light: base x min(1, 0.3 + 0.7)
    away = rr.shade_ref(fid, quad, -towards, rr.quad_faces(), light, background=(1, 2, 3))
    assert np.allclose(away[0, :, :4], 220.0 * 0.3) and (away[0, :, 4:] == [1, 2, 3]).all()     # turned away: ambient only, no flip


# ---- the reference's scene --------------------------------------------------------------------------------------------------------------------------
def test_camera_and_light_are_the_references():
    c, s = np.cos(np.deg2rad(2.0)), np.sin(np.deg2rad(2.0))
    cam = render.reference_camera()
    assert np.allclose(cam, [[1, 0, 0, 0], [0, c, s, 1], [0, -s, c, 5], [0, 0, 0, 1]], atol=1e-15)         # create_pose_camera(-2)
    assert abs(cam[1, 2] - 0.0348994967) < 1e-9 and abs(cam[1, 1] - 0.9993908270) < 1e-9
    lit = render.reference_light()
    assert np.allclose(lit, [[1, 0, 0, 0], [0, np.sqrt(0.75), 0.5, 0], [0, -0.5, np.sqrt(0.75), 3], [0, 0, 0, 1]], atol=1e-15)   # create_pose_light(-30)
    assert np.array_equal(cam, rr.camera_pose()) and np.array_equal(lit, rr.light_pose())
    sc = render.Scene(rr.quad_faces())
    assert np.allclose(sc.view, rr.view_of(rr.camera_pose())) and np.allclose(sc.light, [0, 0.5, np.sqrt(0.75)])
    assert (sc.ymag, sc.znear, sc.zfar, sc.ambient, sc.diffuse) == (1.0, 0.05, 100.0, 0.3, 0.7)
    assert sc.base == (220 / 255,) * 3 and sc.background == (255, 255, 255)
    # a point on the camera's axis lands on the image centre, one unit up lands half a height higher
    centre = rr.world_from_pixels(np.asarray([480.0]), np.asarray([360.0]), 4.0, cam, 960, 720)
    up = centre + cam[:3, 1]
    xy, z, _ = rr.project_ref(np.stack([centre, up], 1), [[0, 1, 1]], sc.view, 960, 720)
    assert np.array_equal(xy[0], [[480 * 16, 360 * 16], [480 * 16, 0]]) and np.allclose(z, 4.0)


def test_vertex_faces_index_round_trips():
    r = np.random.RandomState(0)
    faces = r.randint(0, 40, (90, 3)).astype(np.int32)
    faces[7] = [3, 3, 5]                                              # a face that names a vertex twice is listed once for it
    off, inc = render.vertex_faces_csr(faces, 43)
    want_off, want_inc = rr.vertex_faces_csr(faces, 43)
    assert off.dtype == inc.dtype == np.int32 and np.array_equal(off, want_off) and np.array_equal(inc, want_inc)
    for v in range(43):
        mine = inc[off[v]:off[v + 1]]
        assert np.array_equal(mine, np.nonzero((faces == v).any(1))[0])               # every face of the vertex, ascending
    sc = render.Scene(faces, n_vertices=43)
    assert (sc.n_vertices, sc.n_faces) == (43, 90) and np.array_equal(sc.vf_offsets, off) and off[-1] == len(inc)
    assert render.Scene(faces).n_vertices == int(faces.max()) + 1


def test_scene_refuses_bad_faces_and_sizes():
    with pytest.raises(ValueError, match="outside"):
        render.Scene(np.asarray([[0, 1, 5]]), n_vertices=5)
    with pytest.raises(ValueError, match="outside"):
        render.Scene(np.asarray([[0, -1, 2]]), n_vertices=5)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        render.Scene(np.zeros((0, 3), dtype=np.int32))
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        render.Scene(np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="ymag"):
        render.Scene(rr.quad_faces(), ymag=0.0)
    with pytest.raises(ValueError, match="bytes"):
        render.Scene(rr.quad_faces(), background=(0, 0, 256))


@pytest.mark.parametrize("fps", [30, 15, 10, 7, 60])
def test_frame_indices_are_the_references_sampling(fps):
    for frames in (0, 1, 7, 64):
        want = []
        interval = max(1, int(30 // fps))
        for i in range(frames):                                        # fast_render.py distribute_frames
            if i % interval != 0:
                continue
            want.append(i)
        assert render.frame_indices(frames, fps) == want
    assert len(render.frame_indices(64, fps)) == {30: 64, 15: 32, 10: 22, 7: 16, 60: 64}[fps]


def test_write_bmp(tmp_path):
    r = np.random.RandomState(1)
    img = r.randint(0, 256, (5, 7, 3)).astype(np.uint8)               # 21 bytes a row: padded to 24
    path = tmp_path / "frame_0.bmp"
    render.write_bmp(path, img)
    raw = path.read_bytes()
    assert raw[:2] == b"BM" and struct.unpack("<I", raw[2:6])[0] == len(raw) == 54 + 24 * 5 and struct.unpack("<I", raw[10:14])[0] == 54
    size, w, h, planes, bits, compression = struct.unpack("<IiiHHI", raw[14:34])
    assert (size, w, h, planes, bits, compression) == (40, 7, 5, 1, 24, 0)
    rows = np.frombuffer(raw[54:], dtype=np.uint8).reshape(5, 24)
    assert np.array_equal(rows[::-1, :21].reshape(5, 7, 3)[:, :, ::-1], img) and not rows[:, 21:].any()
    with pytest.raises(ValueError, match="uint8"):
        render.write_bmp(path, img.astype(np.float32))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("syn_render_workspace_bytes", "syn_render_project", "syn_render_raster", "syn_render_shade")


def test_abi_is_additive_and_declared():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert re.search(r"#define\s+SYN_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9
    for name in NEW_EXPORTS:
        assert re.search(rf"^int(?:64_t)?\s+{name}\s*\(", header, flags=re.M) and name in _lib.EXPORTS, name
    i32, i64, f32, vp = _lib.i32, _lib.i64, _lib.C.c_float, _lib.vp
    assert _lib.PROTOTYPES["syn_render_workspace_bytes"] == (i64, [i64, i32])
    assert _lib.PROTOTYPES["syn_render_raster"] == (_lib.C.c_int, [vp, vp, i64, i32, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp])
    src = open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_kernels.hip")).read()
    assert '#include "syn_render.inc"' in src
    inc = open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_render.inc")).read()
    for const, name in ((render.SUBPIXEL, "kSub"), (render.SUPERTILE, "kSuper"), (render.TILE_ROWS, "kTileRows"), (render.RASTER_CHUNK, "kChunk"),
                        (render.MAX_DIM, "kMaxDim")):
        assert const == int(re.search(rf"constexpr int {name} = (\d+);", inc).group(1)), name
    assert render.RASTER_WALK == 256 * int(re.search(r"constexpr int kWalk = (\d+);", inc).group(1))
    for name in NEW_EXPORTS:                                           # each entry point is defined once
        assert len(re.findall(rf"^int(?:64_t)?\s+{name}\s*\(", inc, flags=re.M)) == 1, name
    assert "atomic" not in inc.replace("no atomics of any kind", "")
