"""The stick-figure rasteriser's restatement (tests/plot_ref.py) and the host side of syntalker_amd/plot.py, without a GPU: the camera, chains and
colours against what matplotlib and the reference say (tests/golden/plot_scene.npz, written by tests/golden/make_plot_golden.py), the capsule rule
against Python integers, the OR rule, the ground polygon on cases worked out by hand, the data preparation, and the C ABI's declarations."""
import math
import os
import re

import numpy as np
import pytest

from tests import plot_ref as pr

from syntalker_amd import _lib, plot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(REPO, "tests", "golden", "plot_scene.npz"))


# ---- the reference's part ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1000, 64])
def test_reference_camera_puts_points_where_matplotlib_does(size):
    """Both sides are fp64 evaluations of the same chain; the condition is 1/256 pixel, so that snapping to 1/16 differs from matplotlib's position
    only at ties.  Measured: 2.3e-13 pixel at 1000, 1.4e-14 at 64."""
    M, A = plot.reference_camera(size)
    worst = 0.0
    for p, want in zip(GOLDEN["points"], GOLDEN[f"pixels_{size}"]):
        got = pr.to_pixel(A, pr.to_clip(M, p))
        worst = max(worst, abs(got[0] - want[0]), abs(got[1] - want[1]))
    print(f"reference_camera at {size}: largest difference to matplotlib {GOLDEN['matplotlib_version']} over {len(GOLDEN['points'])} points = {worst:.3e} pixel")
    assert len(GOLDEN["points"]) == 64 and worst < 1 / 256
    assert M.dtype == np.float64 and M.shape == (4, 4) and A.shape == (2, 3)
    if size == 1000:                                                   # the world origin, as the issue quotes it
        col, row = pr.to_pixel(A, pr.to_clip(M, (0.0, 0.0, 0.0)))
        assert abs(col - 522.905) < 1e-3 and abs((size - row) - 308.695) < 1e-3


def test_chains_colours_and_widths_are_the_references():
    for key, chains in (("smpl", plot.SMPL_CHAINS), ("smplx", plot.SMPLX_CHAINS)):
        lengths = GOLDEN[f"{key}_chain_lengths"]
        assert [len(c) for c in chains] == list(lengths)
        assert [j for c in chains for j in c] == list(GOLDEN[f"{key}_chain_joints"])
    assert len(plot.SMPL_CHAINS) == 5 and len(plot.SMPLX_CHAINS) == 15
    names = [str(n) for n in GOLDEN["colour_names"]]
    for name, rgb in zip(names, GOLDEN["colour_rgb"]):
        assert plot.COLOURS[name] == tuple(int(v) for v in np.rint(255 * rgb))
    assert [names[k] for k in GOLDEN["chain_colours"]] == list(plot.CHAIN_COLOURS)
    assert [plot.half_width(pt, 1000) for pt in (4.0, 2.0, 1.0)] == [44, 22, 11]
    assert plot.half_width(1.0, 8) == 1                                 # never below one unit
    p = plot.Plot(plot.SMPLX_CHAINS, size=1000)
    assert p.segments.shape == (51, 4) and plot.Plot().segments.shape == (21, 4)
    assert list(p.segments[:21, 3]) == [44] * 21 and list(p.segments[21:, 3]) == [22] * 30 and p.traj_half_width == 11
    assert list(p.segments[:, 2]) == sorted(p.segments[:, 2]) and p.segments[0, 2] == 2 and p.segments[-1, 2] == 16
    assert p.colours[1] == 255 << 16 and p.colours[2] == 255 and p.colours[4] == 0 and p.colours[7] == 139 << 16 and p.colours[16] == 139
    with pytest.raises(ValueError, match="4096"):
        plot.Plot(size=4097)


def test_prepare_is_the_references_lines():
    rng = np.random.default_rng(3)
    walk = np.cumsum(rng.normal(0, 0.05, (50, 1, 3)), 0) + rng.normal(0, 0.4, (50, 22, 3))
    joints = walk.astype(np.float32)
    want = pr.transcribed_prepare(joints)
    got = plot.prepare(joints)
    import torch
    got_t = plot.prepare(torch.from_numpy(joints))
    for w, g, t in zip(want, got, got_t):
        assert g.dtype == np.float32 and np.array_equal(w, g) and np.array_equal(w, t.numpy())
    assert np.array_equal(joints, walk.astype(np.float32))             # the caller's array is left alone
    assert (got[0][:, 0, 0] == 0).all() and (got[0][:, 0, 2] == 0).all() and got[0][..., 1].min() == 0


def test_trajectory_layer_ends_one_point_short_of_the_frame():
    assert [plot.trajectory_segments(k) for k in (0, 1, 2, 5)] == [0, 0, 1, 4]
    p = plot.Plot(size=64)
    j = pr.walking_take(6, 22, plot.SMPL_CHAINS)
    data, trajec, mins, maxs = plot.prepare(j)
    idx = [0, 1, 2, 5]
    rec, gr = pr.setup_ref(data[idx], trajec, idx, (mins[0], maxs[0], mins[2], maxs[2]), p.segments, p.M, p.A, 64, p.traj_half_width, 21 + 4)
    assert [int((rec[f, :, 5] >> 16 == 1).sum()) for f in range(4)] == [0, 0, 1, 4]
    assert [int(gr[f, 1]) for f in range(4)] == [21, 21, 22, 25]
    # frame 5's path runs trajec[0] .. trajec[4], seen from trajec[5]: its last point is NOT the root's own (0, 0)
    last = pr.segment_record(p.M, p.A, 64, (*(trajec[3] - trajec[5])[:1], 0.0, (trajec[3] - trajec[5])[1]), (*(trajec[4] - trajec[5])[:1], 0.0, (trajec[4] - trajec[5])[1]),
                             p.traj_half_width, 1)
    assert tuple(rec[3, 3]) == last and (rec[3, 4:, 5] >> 16 >= 2).all()


# ---- the capsule rule -------------------------------------------------------------------------------------------------------------------------------
def test_isqrt_is_exact_at_perfect_squares():
    for r in (1, 2, 3, 44, 4095, 2 ** 20 + 1, 2 ** 30 - 1, 1518500249):             # the last: floor(sqrt(2^61))
        assert pr.isqrt(r * r) == r and pr.isqrt(r * r + 1) == r and pr.isqrt(r * r - 1) == r - 1


def test_capsule_rule_is_cross_squared_against_r_squared_l_squared():
    """|cross| <= isqrt(R^2 L2) is cross^2 <= R^2 L2 for integers; plot_ref's arrays (int64) against Python integers (unbounded) on 10 000 random
    segments and samples, zero lengths and coordinates at the guard band of a 4096-pixel image included."""
    rng = np.random.default_rng(11)
    lo, hi = -16 * 4096, 2 * 16 * 4096
    n = 10000
    a = rng.integers(lo, hi + 1, (n, 2))
    b = np.where(rng.random((n, 1)) < 0.5, a + rng.integers(-300, 301, (n, 2)), rng.integers(lo, hi + 1, (n, 2))).clip(lo, hi)
    b[:200] = a[:200]                                                  # zero length
    a[200:300] = rng.choice([lo, hi], (100, 2))                        # ends on the band's corners and sides
    b[300:400] = rng.choice([lo, hi], (100, 2))
    R = rng.choice([1, 11, 22, 44, 182, 4095], n)
    # samples near the segment: an end, or a point of it, moved by about R
    t = rng.random((n, 1))
    s = np.rint(a + t * (b - a) + rng.normal(0, 1, (n, 2)) * R[:, None]).astype(np.int64)
    s[:1000] = a[:1000] + rng.integers(-2, 3, (1000, 2))
    T = np.asarray([pr.isqrt(int(r) ** 2 * (int(d[0]) ** 2 + int(d[1]) ** 2)) if (d != 0).any() else -1 for r, d in zip(R, b - a)], dtype=np.int64)
    got = pr.capsule_covers(a[:, 0], a[:, 1], b[:, 0], b[:, 1], R, T, s[:, 0], s[:, 1])
    assert got.dtype == bool and np.abs(T).max() < 2 ** 31
    covered = 0
    for k in range(n):
        ax, ay, bx, by, sx, sy, r = (int(v) for v in (*a[k], *b[k], *s[k], R[k]))
        dx, dy, px, py = bx - ax, by - ay, sx - ax, sy - ay
        L2, dot, cross = dx * dx + dy * dy, px * dx + py * dy, dx * py - dy * px
        want = (L2 > 0 and 0 <= dot <= L2 and cross * cross <= r * r * L2) or px * px + py * py <= r * r or (sx - bx) ** 2 + (sy - by) ** 2 <= r * r
        assert bool(got[k]) == want, (k, a[k], b[k], s[k], r)
        covered += want
    print(f"capsule rule: {covered} of {n} samples covered, largest T {int(T.max())}")
    assert 0.2 * n < covered < 0.8 * n                                 # the cases sit on the boundary, not far inside or outside


def paint(records, size, colours, ground=None):
    rec = np.asarray(records, dtype=np.int64)[None]
    g = np.zeros((1, pr.GROUND_INTS), dtype=np.int64)
    g[0, :4] = (0, rec.shape[1], 1, 1)
    if ground is not None:
        g[0] = ground
    return pr.draw_ref(rec, g, colours, size)[0]


def test_a_split_polyline_and_a_reversed_chain_paint_the_same_bytes():
    """The OR rule: a joint inside a layer is not painted twice, and the order of a layer's segments does not matter."""
    colours = [0, 0xff0000, 0x0000ff]
    a, c, b = (100, 130), (100 + 3 * 40, 130 + 3 * 25), (100 + 7 * 40, 130 + 7 * 25)          # c on a-b, all on the grid
    whole = paint([pr.snapped_record(*a, *b, 20, 2, 40)], 40, colours)
    split = paint([pr.snapped_record(*a, *c, 20, 2, 40), pr.snapped_record(*c, *b, 20, 2, 40)], 40, colours)
    assert np.array_equal(whole, split) and (whole != 255).any() and len(np.unique(whole[..., 1])) > 4      # partly covered pixels are there
    chain = [(60, 500), (300, 420), (330, 200), (560, 90)]
    fwd = [pr.snapped_record(*chain[k], *chain[k + 1], 30, 2, 40) for k in range(3)]
    back = [pr.snapped_record(*chain[k + 1], *chain[k], 30, 2, 40) for k in (2, 1, 0)]
    assert np.array_equal(paint(fwd, 40, colours), paint(back, 40, colours))
    # two LAYERS over each other are painted twice: the second over the first
    twice = paint([pr.snapped_record(*a, *b, 20, 1, 40), pr.snapped_record(*a, *b, 20, 2, 40)], 40, colours)
    assert not np.array_equal(twice, whole) and (twice[whole[..., 1] == 255] == 255).all()
    # a zero-length segment is its disc: 16 R^2 pi / 256 pixels of ink, about
    disc = paint([pr.snapped_record(322, 322, 322, 322, 64, 2, 40)], 40, colours)
    ink = (255 - disc[..., 1].astype(np.int64)).sum() / 255
    assert abs(ink - math.pi * 16) < 1.0


# ---- the ground -------------------------------------------------------------------------------------------------------------------------------------
def test_two_triangles_sharing_a_diagonal_cover_each_sample_once():
    quad = [(2, 2), (130, 2), (130, 130), (2, 130)]                    # the diagonal (2, 2) - (130, 130) runs through samples
    sx, sy = pr._samples(0, 9, 0, 9)
    t1, t2 = pr.polygon_covers([quad[0], quad[1], quad[2]], sx, sy), pr.polygon_covers([quad[0], quad[2], quad[3]], sx, sy)
    whole = pr.polygon_covers(quad, sx, sy)
    assert not (t1 & t2).any() and np.array_equal(t1 | t2, whole)
    on_diagonal = (np.broadcast_to(sx, whole.shape) == np.broadcast_to(sy, whole.shape)) & whole
    assert on_diagonal.sum() == 32 and (t1 ^ t2)[on_diagonal].all()
    # samples on the left and top edges belong to the quad, on the right and bottom edges not: 128 / 4 = 32 samples a side
    assert whole.sum() == 32 * 32 and whole[0, 0, 0, 0] and not whole[8, 8].any()


def test_ground_quad_reaching_behind_the_camera_is_cut_where_worked_out_by_hand():
    # clip = (x, 1, ., z): u = x / z, v = 1 / z.  The quad x, z in [-1, 1] has two corners at z = -1 < 1/16.  Edge (-1, -1) -> (-1, 1) is cut at t = (1 -
    # 1/16) / 2 from the corner in front: (u, v) = (-16, 16); likewise (16, 16) on the other side; the corners in front are (-1, 1) and (1, 1).
    M = np.asarray([[1.0, 0, 0, 0], [0, 0, 0, 1.0], [0, 0, 0, 0], [0, 0, 1.0, 0]])
    quad = [(-1.0, 0.0, -1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0), (1.0, 0.0, -1.0)]
    A = np.asarray([[2.0, 0, 32.0], [0, 2.0, 0.0]])                    # col = 2 u + 32, row = 2 v: inside the guard band of a 64-pixel image
    assert pr.ground_corners(M, A, 64, quad) == [(0, 512), (480, 32), (544, 32), (1024, 512)]
    # four times the scale: the cut corners (-96, 128) and (160, 128) pixels leave the band [-64, 128], whose sides cut them off: six corners
    A = np.asarray([[8.0, 0, 32.0], [0, 8.0, 0.0]])
    assert pr.ground_corners(M, A, 64, quad) == [(-1024, 1536), (384, 128), (640, 128), (2048, 1536), (2048, 2048), (-1024, 2048)]
    turned = pr.ground_corners(M, A, 64, quad[::-1])                   # the other winding: oriented to the same cycle
    assert turned[turned.index((-1024, 1536)):] + turned[:turned.index((-1024, 1536))] == pr.ground_corners(M, A, 64, quad)
    assert pr.ground_corners(M, A, 64, [(x, y, -z) for x, y, z in quad]) != []               # (mirrored: still two corners in front)
    assert pr.ground_corners(M, A, 64, [(x, y, z - 3.0) for x, y, z in quad]) == []          # wholly behind
    assert pr.ground_corners(M, A, 64, [(np.nan, 0.0, 1.0)] + quad[1:]) == []
    # the ground paints c = (255 (32 - k) + 128 k + 16) >> 5: 128 where all 16 samples are covered... of alpha 0.5: (255 + 128) / 2 = 191.5 -> 192
    g = pr.ground_record(M, np.asarray([[2.0, 0, 32.0], [0, 2.0, 0.0]]), 64, quad, 0)
    img = pr.draw_ref(np.zeros((1, 1, 8), np.int64), np.asarray([g]), [0, 0], 64)[0]
    assert img[20, 32].tolist() == [192, 192, 192] and img[1, 32].tolist() == [255, 255, 255] and set(np.unique(img)) <= set(range(192, 256))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("syn_plot_workspace_bytes", "syn_plot_setup", "syn_plot_draw")


def test_abi_is_additive_and_declared():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert re.search(r"#define\s+SYN_ABI_VERSION\s+9\b", header) and _lib.ABI_VERSION == 9
    inc = open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_plot.inc")).read()
    for name in NEW_EXPORTS:
        assert len(re.findall(rf"^int(?:64_t)?\s+{name}\s*\(", header, flags=re.M)) == 1 and name in _lib.EXPORTS, name
        assert len(re.findall(rf"^int(?:64_t)?\s+{name}\s*\(", inc, flags=re.M)) == 1, name
    i32, i64, vp = _lib.i32, _lib.i64, _lib.vp
    assert _lib.PROTOTYPES["syn_plot_workspace_bytes"] == (i64, [i64, i32])
    assert _lib.PROTOTYPES["syn_plot_setup"] == (_lib.C.c_int, [vp, i64, i32, vp, i64, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp])
    assert _lib.PROTOTYPES["syn_plot_draw"] == (_lib.C.c_int, [vp, i64, i32, vp, i32, i32, vp, vp])
    src = open(os.path.join(REPO, "syntalker_amd", "csrc", "syn_kernels.hip")).read()
    assert src.count('#include "syn_plot.inc"') == 1
    for const, name in ((plot.SUBPIXEL, "kSub"), (plot.TILE, "kTile"), (plot.CHUNK, "kChunk"), (plot.MAX_DIM, "kMaxDim"), (plot.MAX_R, "kMaxR"),
                        (plot.GROUND_INTS, "kGroundInts")):
        assert const == int(re.search(rf"constexpr int {name} = (\d+);", inc).group(1)), name
    assert plot.WALK == 256 * int(re.search(r"constexpr int kWalk = (\d+);", inc).group(1))
    assert plot.W_MIN == float(re.search(r"constexpr double kWMin = ([\d.]+);", inc).group(1)) == pr.W_MIN
    assert "atomic" not in inc.replace("no atomics of any kind", "")
    for path in ("syntalker_amd/plot.py", "scripts/plot_from_results.py", "tests/plot_ref.py"):                  # matplotlib is the fixture generator's alone
        assert not re.search(r"^\s*(import|from)\s+(matplotlib|mpl_toolkits)", open(os.path.join(REPO, path)).read(), flags=re.M), path
