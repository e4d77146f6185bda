"""The renderer on the device (csrc/syn_render.inc, syntalker_amd/render.py) against the numpy restatement of tests/render_ref.py, which
test_render_host.py pins.  `pyrender` cannot run here; the oracle is the rules of DESIGN.md §22.

Gates, none of them measured on the code under test:
  project    xy_sub within 1 unit (1/16 pixel) of the fp64 restatement at every vertex: the fp32 error of the transform is orders below that, so another
             snap can only be the neighbouring one.  z and normal: the project's FK rule - the same chain in plain fp32 torch on the CPU has a max abs
             error E against fp64 on the case's own inputs, the device may be 4 E away.
  rasterize  fed the DEVICE's own xy_sub and z, the restatement's face_id and depth are BIT-EQUAL on every pixel of every case: integer coverage and
             the prescribed depth expression leave nothing to tolerate.
  shade      fed the device's face_id, xy_sub and normal, every channel within 1 level of rint(fp64) (a rounding boundary can flip one level), background
             pixels exact.

Shapes: 64 x 48, 65 x 47 (ragged tiles and supertiles), 16 x 16 (one tile) and 70 x 130 (2 x 3 supertiles, both ragged); 1 and 3 frames.  Meshes: the
sphere, two spheres running through each other, a sphere of 624 faces over one supertile (more than two LDS chunks of render.RASTER_CHUNK), one of 2520 faces partly off the image (three rounds of
render.RASTER_WALK in a supertile's walk), a NaN
vertex, and a mesh built in screen space: a triangle larger than the image, zero areas, triangles outside and across each border, a vertex on a
pixel centre, faces on top of each other, a vertex beyond the guard band, a sentinel."""
import numpy as np
import pytest
import torch

from tests import render_ref as rr

from syntalker_amd import _lib, render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGES = [(64, 48), (65, 47), (16, 16), (70, 130)]
SHIFTS = np.asarray([(0.0, 0.0, 0.0), (0.31, -0.2, 0.3), (-0.9, 0.55, -0.2)])          # frames 1 and 2 hang over the image's borders


@pytest.fixture(scope="module", autouse=True)
def own_memory_pool():
    """This module's device memory comes from a pool of its own, released at its end (with the cached scenes, which hold device tensors), so that
    the modules after it meet PyTorch's caching allocator as they would without it.  The reason is one assertion that runs later,
    test_gpu_rvq_train.py `test_adam_moments_survive_a_move_of_the_parameters`: after model.to("cpu"), model.to(DEV) it requires a parameter's
    address to have CHANGED, which holds or not by which free block the allocator picks - it failed once with this module's blocks and live
    scene tensors in the shared pool.  Nothing here needs the pool for itself: the kernels allocate nothing, and
    `test_native_calls_with_an_exact_workspace_and_the_c_abi_checks` checks that they write nothing outside their outputs."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _stages.clear()
    del pool


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


_meshes = {}


def mesh_of(name):
    """(vertices (3, V, 3) float32 world space, faces): three frames of the named mesh."""
    if name not in _meshes:
        if name == "sphere":
            v, f = rr.uv_sphere(16, 10, (0.1, 1.0, 0.0), 0.7)
        elif name == "pair":
            v, f = rr.sphere_pair(16, 10, (-0.15, 1.0, 0.0), 0.5, (0.4, 0.1, 0.1))
        elif name == "dense":
            v, f = rr.uv_sphere(24, 14, (0.0, 1.05, 0.0), 0.8)
            assert len(f) > 2 * render.RASTER_CHUNK
        elif name == "walk":                                           # 2520 faces, part of them off the image: three rounds of the supertiles' walk
            v, f = rr.uv_sphere(36, 36, (0.6, 1.0, 0.0), 0.9)
            assert len(f) > 2 * render.RASTER_WALK
        _meshes[name] = ((v[None] + SHIFTS[:, None]).astype(np.float32), f)
    return _meshes[name]


_stages = {}


def stages_of(name, size, n):
    """The device's buffers of the first n frames of a mesh, and its scene: computed once per case."""
    key = (name, size, n)
    if key not in _stages:
        v, f = mesh_of(name)
        sc = render.Scene(f, n_vertices=v.shape[1])
        rgb, buf = render.render(sc, dev(v[:n]), size[0], size[1], return_buffers=True)
        torch.cuda.synchronize()
        _stages[key] = (sc, rgb.cpu().numpy(), {k: t.cpu().numpy() for k, t in buf.items()})
    return _stages[key]


def assert_raster_bit_equal(label, xy, z, faces, size, face_id, depth, znear=0.05, zfar=100.0):
    want_id, want_depth = rr.rasterize_ref(xy, z, faces, size[0], size[1], znear, zfar)
    wrong = int((face_id != want_id).sum()), int((depth.view(np.int32) != want_depth.view(np.int32)).sum())
    print(f"raster {label} {size[0]} x {size[1]}: {int((want_id >= 0).sum())} covered pixels of {want_id.size}, {len(np.unique(want_id)) - 1} faces seen, "
          f"{wrong[0]} face ids and {wrong[1]} depths differ")
    assert face_id.shape == want_id.shape and depth.dtype == np.float32
    assert wrong == (0, 0), (label, size, wrong)
    return want_id


# ---- project ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size,n", [("sphere", (64, 48), 3), ("pair", (65, 47), 1), ("dense", (70, 130), 3), ("sphere", (16, 16), 1)])
def test_project_against_fp64(name, size, n):
    v, f = mesh_of(name)
    sc, _, buf = stages_of(name, size, n)
    want_xy, want_z, want_n = rr.project_ref(v[:n], f, sc.view, size[0], size[1])
    t_z, t_n = rr.project_torch32(v[:n], f, sc.view)
    e_z, e_n = float(np.abs(t_z - want_z).max()), float(np.abs(t_n - want_n).max())
    d_xy = int(np.abs(buf["xy_sub"].astype(np.int64) - want_xy).max())
    err_z, err_n = float(np.abs(buf["z"] - want_z).max()), float(np.abs(buf["normal"] - want_n).max())
    print(f"project {name} {size}: xy_sub differs by at most {d_xy} unit(s) ({int((buf['xy_sub'] != want_xy).sum())} coordinates); z E = {e_z:.3e}, device "
          f"error = {err_z:.3e}, gate = {4 * e_z:.3e}; normal E = {e_n:.3e}, device error = {err_n:.3e}, gate = {4 * e_n:.3e}")
    assert buf["xy_sub"].dtype == np.int32 and buf["xy_sub"].shape == want_xy.shape
    assert d_xy <= 1
    assert err_z <= 4 * e_z and err_n <= 4 * e_n


def test_project_scales_with_ymag_and_marks_what_is_not_finite():
    v, f = mesh_of("sphere")
    sc = render.Scene(f, ymag=1.7)
    xy, z, _ = render.project(sc, dev(v[:1]), 64, 48)
    want_xy, _, _ = rr.project_ref(v[:1], f, sc.view, 64, 48, ymag=1.7)
    assert np.abs(xy.cpu().numpy() - want_xy).max() <= 1
    bad = v[:1].copy()
    bad[0, 5] = [np.nan, 0.0, 0.0]
    bad[0, 9] = [0.0, np.inf, 0.0]
    bad[0, 11] = [3e38, 3e38, 3e38]                                  # finite, but not on the screen
    bad[0, 12] = [1e6, 1.0, 0.0]                                     # finite on the screen: clamped far outside every guard band
    xy = render.project(sc, dev(bad), 64, 48)[0].cpu().numpy()
    assert (xy[0, [5, 9, 11]] == render.SENTINEL).all() and xy[0, 12, 0] > 16 * 8192 * 3 and xy[0, 12, 0] <= 2 ** 30
    keep = np.ones(v.shape[1], bool)
    keep[[5, 9, 11, 12]] = False
    assert np.abs(xy[0, keep] - want_xy[0, keep]).max() <= 1


# ---- rasterize --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", IMAGES)
@pytest.mark.parametrize("name,n", [("sphere", 3), ("pair", 1), ("dense", 3)])
def test_rasterize_is_the_restatement_bit_for_bit(name, n, size):
    _, f = mesh_of(name)
    _, _, buf = stages_of(name, size, n)
    want_id = assert_raster_bit_equal(name, buf["xy_sub"], buf["z"], f, size, buf["face_id"], buf["depth"])
    assert (want_id[0] >= 0).any() or size == (16, 16)
    assert np.isinf(buf["depth"][buf["face_id"] < 0]).all() and np.isfinite(buf["depth"][buf["face_id"] >= 0]).all()


def walk_rounds(xy, faces, size):
    """What the walk of each supertile's workgroup does with one frame, from the kernel's constants: per supertile the list's length after each round's
    append, and how many chunks that round then drew."""
    boxes = []
    for tri in faces:
        o = rr.oriented(xy, tri, size[0], size[1])
        boxes.append((o and rr._samples(o[:3], size[0], size[1])) or None)
    out = {}
    for sy in range(-(-size[1] // render.SUPERTILE)):
        for sx in range(-(-size[0] // render.SUPERTILE)):
            x0, y0 = sx * render.SUPERTILE, sy * render.SUPERTILE
            hit = [b is not None and b[0] <= x0 + render.SUPERTILE - 1 and b[1] >= x0 and b[2] <= y0 + render.SUPERTILE - 1 and b[3] >= y0 for b in boxes]
            count, rounds = 0, []
            for base in range(0, len(faces), render.RASTER_WALK):
                kept, count = count, count + sum(hit[base:base + render.RASTER_WALK])
                rounds.append((kept, count, count // render.RASTER_CHUNK))
                if count >= render.RASTER_CHUNK:
                    count %= render.RASTER_CHUNK
            out[(sx, sy)] = rounds
    return out


@pytest.mark.parametrize("size", [(64, 48), (70, 130)])
def test_rasterize_when_the_walk_takes_several_rounds(size):
    """More faces than one round of a supertile's walk tests (render.RASTER_WALK): the list's remainder is carried into the next round, new hits
    are appended behind it, rounds end with and without a chunk to draw - the regime of the real mesh (20 908 faces: 21 rounds)."""
    _, f = mesh_of("walk")
    _, _, buf = stages_of("walk", size, 3)
    assert_raster_bit_equal("walk", buf["xy_sub"], buf["z"], f, size, buf["face_id"], buf["depth"])
    rounds = [r for frame in range(3) for per_tile in walk_rounds(buf["xy_sub"][frame], f, size).values() for r in [per_tile]]
    flat = [r for per_tile in rounds for r in per_tile]
    carried_and_drew = sum(1 for kept, count, drew in flat if kept > 0 and drew > 0)
    carried_no_draw = sum(1 for kept, count, drew in flat if count > 0 and drew == 0 and kept < count)
    longest = max(count for _, count, _ in flat)
    print(f"walk {size}: {len(rounds)} supertile walks of {len(rounds[0])} rounds; rounds that appended behind a remainder and drew: {carried_and_drew}, "
          f"rounds that ended below a chunk: {carried_no_draw}, longest list {longest}, most chunks in a round {max(d for _, _, d in flat)}")
    assert len(rounds[0]) == 3 and carried_and_drew > 0 and carried_no_draw > 0 and longest > render.RASTER_CHUNK


def screen_mesh(width, height):
    """xy_sub (V, 2), z (V,), faces, and the faces that must never show: built in screen space, so every coordinate is exact."""
    s, g = rr.SUB, rr.SUB * max(width, height)
    w, h = s * width, s * height
    tris = [                                                                                   # (three (x, y, z), may it show)
        ([(-g + 1, -g + 2, 5.0), (w + g - 1, -7, 6.0), (5, h + g - 3, 7.0)], True),            # 0 larger than the image: lands in every tile
        ([(s * 5 + 8, s * 7 + 8, 2.0), (s * 12 + 8, s * 7 + 8, 2.5), (s * 5 + 8, s * 13 + 8, 3.0)], True),     # 1 vertices on pixel centres, edges through centres
        ([(s * 5 + 8, s * 7 + 8, 2.0), (s * 5 + 8, s * 13 + 8, 3.0), (s * 12 + 8, s * 7 + 8, 2.5)], False),    # 2 face 1 again, other winding: the tie goes to face 1
        ([(20, 20, 1.0), (60, 60, 1.0), (100, 100, 1.0)], False),                              # 3 zero area: collinear
        ([(40, 24, 1.0), (40, 24, 1.0), (90, 70, 1.0)], False),                                # 4 zero area: a vertex twice
        ([(w + 16, 30, 1.0), (w + 100, 40, 1.0), (w + 50, 90, 1.0)], False),                   # 5 wholly outside
        ([(-40, h // 2 - 30, 1.5), (50, h // 2, 1.5), (-40, h // 2 + 30, 1.5)], True),         # 6 across the left border
        ([(w - 50, h // 2 - 31, 1.5), (w + 45, h // 2 + 3, 1.5), (w - 50, h // 2 + 35, 1.5)], True),          # 7 the right
        ([(w // 2 - 33, -41, 1.5), (w // 2 + 37, -41, 1.5), (w // 2 + 2, 52, 1.5)], True),     # 8 the top
        ([(w // 2 - 33, h + 41, 1.5), (w // 2 + 3, h - 52, 1.5), (w // 2 + 37, h + 41, 1.5)], True),          # 9 the bottom
        ([(-g - 1, 10, 1.0), (w // 2, 10, 1.0), (w // 2, h - 10, 1.0)], False),                # 10 a vertex beyond the guard band: dropped whole
        ([(rr.SENTINEL, rr.SENTINEL, 1.0), (w // 2, 10, 1.0), (w // 2, h - 10, 1.0)], False),  # 11 a sentinel vertex
        ([(30, 30, 0.01), (w - 30, 40, 0.01), (w // 2, h - 30, 0.01)], False),                 # 12 nearer than znear
        ([(30, 30, 4.0), (w - 30, 40, 4.0), (w // 2, h - 30, 200.0)], True),                   # 13 runs out beyond zfar: cut by the depth test per fragment
    ]
    pts = np.asarray([p for t, _ in tris for p in t], dtype=np.float64)
    faces = np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)
    return pts[:, :2].astype(np.int32), pts[:, 2].astype(np.float32), faces, [k for k, (_, show) in enumerate(tris) if not show]


@pytest.mark.parametrize("size", IMAGES + [(2048, 16)])              # 2048 wide: the large triangle's edge values pass 2^31, the kernel's 64-bit path
def test_rasterize_screen_space_cases(size):
    xy, z, faces, hidden = screen_mesh(*size)
    sc = render.Scene(faces)
    # three frames: the mesh, the mesh moved by a third of a pixel, and the mesh with frame 0's depths reversed
    xy3 = np.stack([xy, np.where(xy == rr.SENTINEL, xy, xy + 5), xy])
    z3 = np.stack([z, z, np.float32(8.0) - z])
    face_id, depth = render.rasterize(sc, dev(xy3, torch.int32), dev(z3), size[0], size[1])
    face_id, depth = face_id.cpu().numpy(), depth.cpu().numpy()
    want_id = assert_raster_bit_equal("screen-space mesh", xy3, z3, faces, size, face_id, depth)
    assert not np.isin(want_id[0], hidden).any()
    assert not np.isin(want_id[1], [k for k in hidden if k != 10]).any() and (want_id[1] == 10).any()    # moved by 5 units, face 10 is inside the guard band
    assert (want_id[0] >= 0).mean() > 0.8 and (want_id[0] == 0).any()  # the large triangle fills the image, or all but a corner of it
    if size != (16, 16):
        assert set(np.unique(want_id[0])) >= {0, 1, 6, 7, 8, 9}
        assert want_id[0, 7, 5] == 1 and depth[0, 7, 5] == 2.0         # the sample ON the vertex of face 1 (its top-left corner) is that face's


def test_a_nan_vertex_takes_its_faces_away_and_nothing_else():
    v, f = mesh_of("sphere")
    sc, _, clean = stages_of("sphere", (64, 48), 1)
    # the vertex nearest to the camera: its faces are in front
    k = int(np.argmin(clean["z"][0]))
    bad = v[:1].copy()
    bad[0, k] = np.nan
    rgb, buf = render.render(sc, dev(bad), 64, 48, return_buffers=True)
    buf = {n: t.cpu().numpy() for n, t in buf.items()}
    assert (buf["xy_sub"][0, k] == render.SENTINEL).all()
    gone = np.nonzero((f == k).any(1))[0]
    assert_raster_bit_equal("NaN vertex", buf["xy_sub"], buf["z"], f, (64, 48), buf["face_id"], buf["depth"])
    assert not np.isin(buf["face_id"], gone).any() and np.isin(clean["face_id"], gone).any()
    rest = ~np.isin(clean["face_id"], gone)
    assert np.array_equal(buf["face_id"][rest], clean["face_id"][rest]) and np.array_equal(buf["depth"][rest], clean["depth"][rest])
    # the normals of its neighbours leave its faces out (the restatement's rule) and stay finite; the picture has no hole to the background inside
    want_n = rr.project_ref(bad, f, sc.view, 64, 48)[2]
    others = np.arange(v.shape[1]) != k
    assert np.isfinite(buf["normal"][0, others]).all() and np.abs(buf["normal"][0, others] - want_n[0, others]).max() < 1e-5
    assert_shade_within_one_level("NaN vertex", sc, rgb.cpu().numpy(), buf, f)


# ---- shade ------------------------------------------------------------------------------------------------------------------------------------------
def assert_shade_within_one_level(label, sc, rgb, buf, faces):
    want = rr.shade_ref(buf["face_id"], buf["xy_sub"], buf["normal"], faces, sc.light, sc.base, sc.background, sc.ambient, sc.diffuse)
    diff = np.abs(rgb.astype(np.int64) - np.rint(want).astype(np.int64))
    covered = buf["face_id"] >= 0
    print(f"shade {label}: {int(covered.sum())} covered pixels, {int((diff == 1).sum())} channels one level off, max {int(diff.max())}; levels "
          f"{int(rgb[covered].min()) if covered.any() else '-'} .. {int(rgb[covered].max()) if covered.any() else '-'}")
    assert rgb.dtype == np.uint8 and rgb.shape == want.shape
    assert diff.max() <= 1
    assert (rgb[~covered] == np.asarray(sc.background, dtype=np.uint8)).all()
    # Where fp64 is not within 1e-3 of a rounding boundary the byte is exact: the fp32 chain (three quotients, the interpolation, one normalisation, one
    # dot product, a few ulps of 6e-8 each on numbers <= 1) puts c off by under 1e-6, 255 c by under 3e-4.
    safe = np.abs(want - np.floor(want) - 0.5) > 1e-3
    assert (diff[safe] == 0).all()


@pytest.mark.parametrize("name,size,n", [("sphere", (64, 48), 3), ("pair", (65, 47), 1), ("dense", (70, 130), 3), ("sphere", (16, 16), 1), ("pair", (70, 130), 1)])
def test_shade_against_fp64(name, size, n):
    _, f = mesh_of(name)
    sc, rgb, buf = stages_of(name, size, n)
    assert_shade_within_one_level(f"{name} {size}", sc, rgb, buf, f)
    covered = buf["face_id"] >= 0
    if covered.any():
        lit = rgb[covered]
        assert (lit[:, 0] == lit[:, 1]).all() and (lit[:, 1] == lit[:, 2]).all()                  # a grey
        assert lit.min() >= 66 and lit.max() <= 220                                          # 220 x 0.3 .. 220 x 1.0


def test_shade_takes_colours_and_light_from_the_scene():
    v, f = mesh_of("sphere")
    sc = render.Scene(f, base=(0.8, 0.5, 0.1), background=(3, 40, 250), ambient=0.1, diffuse=1.2, light_pose=rr.rot_x_pose(40.0, 0.0, 3.0))
    rgb, buf = render.render(sc, dev(v[:1]), 65, 47, return_buffers=True)
    assert_shade_within_one_level("coloured", sc, rgb.cpu().numpy(), {k: t.cpu().numpy() for k, t in buf.items()}, f)
    covered = buf["face_id"] >= 0
    assert int(rgb[..., 0][covered].max()) == 204 and int(rgb[..., 2][covered].min()) == 3    # min(1, .) saturates at 255 x 0.8; turned away: 25.5 x 0.1 -> 3


# ---- the chain, the panels, determinism -------------------------------------------------------------------------------------------------------------
def test_render_is_the_three_stages_chained_and_deterministic():
    v, f = mesh_of("pair")
    sc = render.Scene(f)
    vd = dev(v)
    rgb, buf = render.render(sc, vd, 65, 47, return_buffers=True)
    xy, z, normal = render.project(sc, vd, 65, 47)
    face_id, depth = render.rasterize(sc, xy, z, 65, 47)
    assert torch.equal(xy, buf["xy_sub"]) and torch.equal(z, buf["z"]) and torch.equal(normal, buf["normal"])
    assert torch.equal(face_id, buf["face_id"]) and torch.equal(depth, buf["depth"])
    assert torch.equal(render.shade(sc, face_id, xy, normal), rgb) and torch.equal(render.render(sc, vd, 65, 47), rgb)
    assert rgb.shape == (3, 47, 65, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda
    # frame k alone is frame k of the batch, bit for bit, in every buffer
    for k in range(3):
        one, b1 = render.render(sc, vd[k:k + 1], 65, 47, return_buffers=True)
        assert torch.equal(one[0], rgb[k])
        for name in buf:
            assert torch.equal(b1[name][0], buf[name][k]), (k, name)


def test_render_pair_is_the_two_panels_side_by_side():
    v, f = mesh_of("sphere")
    sc = render.Scene(f)
    res, gt = dev(v[:2]), dev(v[1:3])
    pair = render.render_pair(sc, res, gt, width=130, height=47)
    assert pair.shape == (2, 47, 130, 3)
    assert torch.equal(pair, torch.cat([render.render(sc, res, 65, 47), render.render(sc, gt, 65, 47)], dim=2))
    assert not torch.equal(pair[:, :, :65], pair[:, :, 65:])
    with pytest.raises(ValueError, match="ground-truth"):
        render.render_pair(sc, res, gt[:1])


def test_stages_in_a_cuda_graph():
    v, f = mesh_of("sphere")
    sc = render.Scene(f)
    vd = dev(v[:2])
    want = render.render(sc, vd, 64, 48)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        render.render(sc, vd, 64, 48)                                # warm: the scene is on the device before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = render.render(sc, vd, 64, 48)
    vd.copy_(dev(v[1:3]))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, render.render(sc, vd, 64, 48)) and not torch.equal(got, want)
    vd.copy_(dev(v[:2]))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- the script ------------------------------------------------------------------------------------------------------------------------------------
def test_render_from_results_writes_the_frames_it_promises(tmp_path, capsys):
    import importlib.util
    import json
    import os
    from tests import smplx_mesh_ref as sm
    from syntalker_amd import mesh
    spec = importlib.util.spec_from_file_location("render_from_results", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                                                                                      "render_from_results.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    md = sm.synth_model(3, 203)
    np.savez(tmp_path / "model.npz", **md)
    takes = {}
    for prefix, seed in (("res", 31), ("gt", 32)):
        pose, ex, betas, tr = sm.case_inputs(seed, 7, 100, amp=0.1, transl=True)
        tr = (0.1 * tr + [0.0, 1.0, 0.0]).astype(np.float32)
        betas = sm.case_inputs(31, 1, 100)[2]
        np.savez(tmp_path / f"{prefix}_0.npz", poses=pose, expressions=ex, trans=tr, betas=betas)
        takes[prefix] = (pose, ex, tr, betas)
    out = script.main([str(tmp_path), "--smplx-model", str(tmp_path / "model.npz"), "--out", str(tmp_path / "o"), "--gt", "--fps", "15", "--width", "130",
                       "--height", "47", "--chunk", "3"])
    assert out == {"takes": 1, "frames": 4, "width": 130, "height": 47, "out": str(tmp_path / "o")}
    printed = capsys.readouterr().out
    assert json.loads(printed.strip().splitlines()[-1]) == out and "ffmpeg" in printed and "frame_%d.bmp" in printed
    assert sorted(os.listdir(tmp_path / "o" / "frames_0")) == [f"frame_{k}.bmp" for k in range(4)]
    m = mesh.smplx_mesh(md, takes["res"][3])
    sc = render.Scene(md["f"].astype(np.int64), n_vertices=203)
    pick = [0, 2, 4, 6]                                               # every second frame of the 7
    verts = [mesh.smplx_vertices(m, dev(t[0][pick]), dev(t[1][pick]), dev(t[2][pick])) for t in (takes["res"], takes["gt"])]
    want = render.render_pair(sc, verts[0], verts[1], 130, 47).cpu().numpy()
    assert (want != 255).any()
    for k in range(4):
        raw = (tmp_path / "o" / "frames_0" / f"frame_{k}.bmp").read_bytes()
        rows = np.frombuffer(raw[54:], dtype=np.uint8).reshape(47, 392)                       # 390 bytes a row, padded to 392
        assert np.array_equal(rows[::-1, :390].reshape(47, 130, 3)[:, :, ::-1], want[k])
    one = script.main([str(tmp_path), "--smplx-model", str(tmp_path / "model.npz"), "--out", str(tmp_path / "p"), "--width", "130", "--height", "47"])
    assert one == {"takes": 1, "frames": 7, "width": 65, "height": 47, "out": str(tmp_path / "p")}
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(SystemExit, match="bmp"):
            script.main([str(tmp_path), "--smplx-model", str(tmp_path / "model.npz"), "--format", "png"])


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    v, f = mesh_of("sphere")
    sc = render.Scene(f)
    with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
        render.render(sc, torch.from_numpy(v[:1]), 64, 48)
    with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
        render.rasterize(sc, torch.zeros(1, 146, 2, dtype=torch.int32), torch.zeros(1, 146), 64, 48)
    with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
        render.shade(sc, torch.zeros(1, 48, 64, dtype=torch.int32), torch.zeros(1, 146, 2, dtype=torch.int32, device=DEV), torch.zeros(1, 146, 3, device=DEV))
    with pytest.raises(ValueError, match="outside"):
        render.Scene(f, n_vertices=100)
    for w, h in ((0, 48), (64, 0), (-3, 48), (render.MAX_DIM + 1, 48)):
        with pytest.raises(ValueError, match="width and height"):
            render.render(sc, dev(v[:1]), w, h)
    with pytest.raises(ValueError, match="146"):
        render.render(sc, dev(v[:1, :100]), 64, 48)
    with pytest.raises(ValueError, match="int32"):
        render.rasterize(sc, torch.zeros(1, 146, 2, device=DEV), torch.zeros(1, 146, device=DEV), 64, 48)
    rgb, buf = render.render(sc, dev(v[:0]), 64, 48, return_buffers=True)                     # no frames: empty buffers, nothing launched
    assert rgb.shape == (0, 48, 64, 3) and rgb.dtype == torch.uint8
    assert buf["xy_sub"].shape == (0, 146, 2) and buf["z"].shape == (0, 146) and buf["normal"].shape == (0, 146, 3)
    assert buf["face_id"].shape == (0, 48, 64) and buf["depth"].shape == (0, 48, 64)
    assert render.render_pair(sc, dev(v[:0]), dev(v[:0]), 128, 48).shape == (0, 48, 128, 3)


def test_native_calls_with_an_exact_workspace_and_the_c_abi_checks():
    v, f = mesh_of("sphere")
    sc, rgb_want, want = stages_of("sphere", (65, 47), 3)
    lib, st = _lib.load(), _lib.current_stream(torch.device(DEV))
    s = sc.on(DEV)
    n, V, F, W, H = 3, v.shape[1], len(f), 65, 47
    vd = dev(v)
    nbytes = lib.syn_render_workspace_bytes(n, F)
    assert nbytes == (n * F * 8 + 15) // 16 * 16 + 16 * n
    assert lib.syn_render_workspace_bytes(0, F) == -1 and lib.syn_render_workspace_bytes(n, 0) == -1
    # every buffer a kernel writes lies in one arena with 256 bytes of 0x5A before, between and behind them, which must stay as they are
    sizes = {"xy": n * V * 8, "z": n * V * 4, "nr": n * V * 12, "fid": n * H * W * 4, "dep": n * H * W * 4, "rgb": n * H * W * 3, "ws": nbytes}
    offsets, end = {}, 256
    for name, size in sizes.items():
        offsets[name], end = end, (end + size + 255) // 256 * 256 + 256
    arena = torch.full((end,), 0x5A, dtype=torch.uint8, device=DEV)
    part = {name: arena[o:o + sizes[name]] for name, o in offsets.items()}
    padding = torch.ones(end, dtype=torch.bool, device=DEV)
    for name, o in offsets.items():
        padding[o:o + sizes[name]] = False
    xy, z, nr = part["xy"].view(torch.int32).view(n, V, 2), part["z"].view(torch.float32).view(n, V), part["nr"].view(torch.float32).view(n, V, 3)
    fid, dep = part["fid"].view(torch.int32).view(n, H, W), part["dep"].view(torch.float32).view(n, H, W)
    rgb, ws = part["rgb"].view(n, H, W, 3), part["ws"]
    xy.zero_(), z.zero_(), nr.zero_(), fid.fill_(-7), dep.zero_(), rgb.zero_()

    def project(verts=vd.data_ptr(), frames=n, nv=V, view=s["view"].data_ptr(), w=W, h=H, ymag=1.0, faces=s["faces"].data_ptr(), nf=F,
                off=s["vf_offsets"].data_ptr(), inc=s["vf_faces"].data_ptr(), ninc=int(s["vf_faces"].numel()), o_xy=xy.data_ptr(), o_z=z.data_ptr(),
                o_n=nr.data_ptr()):
        return lib.syn_render_project(verts, frames, nv, view, w, h, ymag, faces, nf, off, inc, ninc, o_xy, o_z, o_n, st)

    def raster(i_xy=xy.data_ptr(), i_z=z.data_ptr(), frames=n, nv=V, faces=s["faces"].data_ptr(), nf=F, w=W, h=H, work=ws.data_ptr(), o_id=fid.data_ptr(),
               o_d=dep.data_ptr()):
        return lib.syn_render_raster(i_xy, i_z, frames, nv, faces, nf, w, h, 0.05, 100.0, work, o_id, o_d, st)

    def shade(i_id=fid.data_ptr(), i_xy=xy.data_ptr(), i_n=nr.data_ptr(), frames=n, nv=V, faces=s["faces"].data_ptr(), nf=F, w=W, h=H, bg=255, out=rgb.data_ptr()):
        return lib.syn_render_shade(i_id, i_xy, i_n, frames, nv, faces, nf, w, h, *(float(c) for c in sc.light), *sc.base, 0.3, 0.7, bg, 255, 255, out, st)

    def refused(rc, word):
        assert rc != 0 and word in lib.syn_last_error().decode(), (rc, lib.syn_last_error())

    # what cannot run is refused before any launch
    for name in ("verts", "view", "faces", "off", "inc", "o_xy", "o_z", "o_n"):
        refused(project(**{name: None}), "null")
    for name in ("i_xy", "i_z", "faces", "work", "o_id", "o_d"):
        refused(raster(**{name: None}), "null")
    for name in ("i_id", "i_xy", "i_n", "faces", "out"):
        refused(shade(**{name: None}), "null")
    for call in (project, raster, shade):
        refused(call(w=0), "8192")
        refused(call(h=8193), "8192")
        refused(call(nv=0), "vertices")
        refused(call(nf=0), "faces")
        refused(call(frames=-1), "negative")
        assert call(frames=0) == 0
    refused(project(ymag=0.0), "ymag")
    refused(project(ninc=-1), "negative")
    refused(raster(work=ws.data_ptr() + 8), "aligned")
    refused(raster(i_xy=xy.data_ptr() + 4), "aligned")
    refused(shade(bg=256), "bytes")
    torch.cuda.synchronize()
    assert not xy.any() and not rgb.any() and (fid == -7).all() and (ws == 0x5A).all() and (arena[padding] == 0x5A).all()      # nothing ran
    # the three calls with a workspace of exactly the size asked for
    assert project() == 0 and raster() == 0 and shade() == 0
    torch.cuda.synchronize()
    assert np.array_equal(xy.cpu().numpy(), want["xy_sub"]) and np.array_equal(z.cpu().numpy(), want["z"]) and np.array_equal(nr.cpu().numpy(), want["normal"])
    assert np.array_equal(fid.cpu().numpy(), want["face_id"]) and np.array_equal(dep.cpu().numpy(), want["depth"])
    assert np.array_equal(rgb.cpu().numpy(), rgb_want)
    assert (arena[padding] == 0x5A).all()                            # no stage wrote a byte outside its outputs or the workspace it asked for
