"""The stick-figure rasteriser on the device (csrc/syn_plot.inc, syntalker_amd/plot.py) against the numpy restatement of tests/plot_ref.py, which
test_plot_host.py pins.  matplotlib is not imported; the oracle is the rules of DESIGN.md §26.

Gates, none of them measured on the code under test:
  setup   the records and the ground records are EQUAL to the restatement's: both sides are fp64 evaluations of the same operations in the same
          order, each rounded once, and integers behind the snap.
  draw    the image bytes are BIT-EQUAL to the restatement's on every pixel of every case: integer coverage and integer blending leave nothing to
          tolerate.

Shapes: 64 (two tiles a side), 80 (a ragged last tile) and 200; 1, 3 and 40 frames; the 22-joint and the 52-joint chains; one frame at 1000.  Inputs: a
walking figure that turns and moves, a NaN joint, a joint behind the camera (its segment is cut at w = 1/16), a ground quad that reaches behind the
camera, a ground that leaves the image on every side, a zero-length segment, a segment wholly outside the image, an end one unit beyond the guard band
and the same end moved onto it, and the last two frames of an 1100-frame take (two rounds of the record walk, several LDS chunks in a tile)."""
import importlib.util
import io
import json
import os
import wave as wave_file

import numpy as np
import pytest
import torch

from tests import jpeg_ref as jr
from tests import plot_ref as pr

from syntalker_amd import _lib, joints, plot, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = {"smpl": (plot.SMPL_CHAINS, 22), "smplx": (plot.SMPLX_CHAINS, 52)}


@pytest.fixture(scope="module", autouse=True)
def own_memory_pool():
    """This module's device memory comes from a pool of its own, released at its end (with the cached cases, which hold device tensors), so that
    the modules after it meet PyTorch's caching allocator as they would without it - the reason DESIGN.md §22 gives for test_gpu_render.py: a later
    test asserts that an address CHANGES, which holds or not by which free block the allocator picks.  Nothing here needs the pool for itself."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _plots.clear()
    del pool


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


_plots, _takes = {}, {}


def plot_of(chains, size):
    if (chains, size) not in _plots:
        _plots[(chains, size)] = plot.Plot(CHAINS[chains][0], size=size)
    return _plots[(chains, size)]


def take_of(chains, n=40, **kw):
    """prepare()'s outputs of a walking take, as numpy: computed once."""
    key = (chains, n, tuple(sorted(kw.items())))
    if key not in _takes:
        _takes[key] = plot.prepare(pr.walking_take(n, CHAINS[chains][1], CHAINS[chains][0], **kw))
    return _takes[key]


def check(label, p, data, trajec, mins, maxs, frames):
    """Draws `frames` on the device; records and bytes against the restatement.  -> (rgb, records, grounds, want_records) as numpy."""
    frames = list(frames)
    rgb, rec, gr = plot.draw_prepared(p, dev(data), dev(trajec), dev(mins), dev(maxs), frames, return_records=True)
    torch.cuda.synchronize()
    rgb, rec, gr = rgb.cpu().numpy(), rec.cpu().numpy(), gr.cpu().numpy()
    want_rec, want_gr = pr.setup_ref(data[frames], trajec, frames, (mins[0], maxs[0], mins[2], maxs[2]), p.segments, p.M, p.A, p.size, p.traj_half_width,
                                     rec.shape[1])
    want = pr.draw_ref(want_rec, want_gr, p.colours, p.size)
    kept = int((want_rec[..., 6] != 1).sum())
    print(f"plot {label} {p.size} x {p.size}, {len(frames)} frame(s) of {rec.shape[1]} slots: {int((rec != want_rec).any(-1).sum())} records and "
          f"{int((gr != want_gr).any(-1).sum())} ground records differ ({kept} records with pixels, grounds of {sorted(set(want_gr[:, 0]))} corners); "
          f"{int((rgb != want).any(-1).sum())} of {want[..., 0].size} pixels differ, {int((want != 255).any(-1).sum())} painted")
    assert rec.shape == want_rec.shape and gr.shape == want_gr.shape and rgb.shape == want.shape and rgb.dtype == np.uint8
    assert np.array_equal(rec, want_rec) and np.array_equal(gr, want_gr)
    assert np.array_equal(rgb, want)
    return rgb, rec, gr, want_rec


# ---- the walking figure -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains,size,n", [("smpl", 64, 40), ("smplx", 64, 3), ("smpl", 80, 3), ("smplx", 80, 40), ("smplx", 80, 1), ("smpl", 200, 1),
                                           ("smplx", 200, 3), ("smpl", 64, 1)])
def test_walking_take_is_the_restatement_bit_for_bit(chains, size, n):
    data, trajec, mins, maxs = take_of(chains)
    frames = {1: [17], 3: [0, 1, 39], 40: range(40)}[n]
    rgb, rec, gr, _ = check(f"walk {chains}", plot_of(chains, size), data, trajec, mins, maxs, frames)
    assert (gr[:, 0] == 4).all() and (rgb != 255).any(-1).mean() > 0.05                     # the ground and the figure are in the picture
    assert (rgb[..., 0].astype(np.int64) - rgb[..., 1] > 40).any() and (rgb[..., 2].astype(np.int64) - rgb[..., 1] > 40).any()      # red and blue ink


def test_one_frame_at_the_references_size():
    data, trajec, mins, maxs = take_of("smplx")
    rgb, rec, gr, _ = check("walk smplx", plot_of("smplx", 1000), data, trajec, mins, maxs, [30])
    assert list(rec[0, 29:50, 5] & 0xffff) == [44] * 21 and list(rec[0, :29, 5] & 0xffff) == [11] * 29
    assert (rgb[0] == (255, 0, 0)).all(-1).any() and (rgb[0] == (0, 0, 0)).all(-1).any() and (rgb[0] == (192, 192, 192)).all(-1).any()


# ---- the edges --------------------------------------------------------------------------------------------------------------------------------------
def eye_of(M):
    """The world point with clip x = y = w = 0: the camera's eye."""
    return np.linalg.solve(M[[0, 1, 3], :3], -M[[0, 1, 3], 3])


def x_that_snaps_to(p, y, z, target):
    """A float32 x whose point (x, y, z) snaps to column `target` (units), by bisection over the restatement's own projection (monotone in x)."""
    snapped = lambda x: pr.rint(16.0 * pr.to_pixel(p.A, pr.to_clip(p.M, (np.float32(x), y, z)))[0])
    lo, hi = -60.0, 0.0
    assert snapped(lo) < target < snapped(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if snapped(mid) < target else (lo, mid)
    for x in (np.float32(hi), np.nextafter(np.float32(hi), np.float32(1)), np.float32(lo)):
        if snapped(x) == target:
            return x
    raise AssertionError("no float32 x snaps there")


def edge_take(p):
    """Six frames of the 22-joint walk, prepared, each with one thing wrong; and what to expect of the segment concerned."""
    data, trajec, mins, maxs = (np.array(v) for v in take_of("smpl", 8))
    data = data[:6].copy()
    seg = {tuple(s[:2]): k for k, s in enumerate(p.segments)}
    data[0, 7] = np.nan                                                 # frame 0: both segments of joint 7 go
    eye = eye_of(p.M)
    a = data[1, 12].astype(np.float64)
    data[1, 15] = eye + 0.02 * (eye - a) + (0.05, 0.0, 0.0)             # frame 1: joint 15 just behind the eye, a little to the side of the line of sight
    data[2, 21] = data[2, 19]                                           # frame 2: a zero-length segment
    data[3, 18], data[3, 20] = (-6.0, 0.9, 0.3), (-5.5, 1.0, 0.2)       # frame 3: segment 18 - 20 left of the image, inside the guard band
    g = 16 * p.size
    data[4, 11, 0] = x_that_snaps_to(p, data[4, 11, 1], data[4, 11, 2], -g - 1)      # frame 4: joint 11 one unit beyond the band
    data[5, 11] = data[4, 11]
    data[5, 11, 0] = x_that_snaps_to(p, data[5, 11, 1], data[5, 11, 2], -g)          # frame 5: the same joint moved onto it
    return data, trajec[:6], mins, maxs, seg


def test_edges_nan_behind_the_camera_zero_length_outside_and_the_guard_band():
    p = plot_of("smpl", 80)
    data, trajec, mins, maxs, seg = edge_take(p)
    rgb, rec, gr, want = check("edges", p, data, trajec, mins, maxs, range(6))
    empty = np.asarray(plot.EMPTY_RECORD)
    slot = lambda f, pair: rec[f, plot.trajectory_segments(f) + seg[pair]]
    assert (slot(0, (4, 7)) == empty).all() and (slot(0, (7, 10)) == empty).all() and (slot(0, (1, 4))[6] != 1)
    assert pr.to_clip(p.M, data[1, 15])[2] < pr.W_MIN < pr.to_clip(p.M, data[1, 12])[2]
    cut = slot(1, (12, 15))
    assert cut[6] != 1 and cut[4] > 0, cut                              # kept, cut at w = 1/16, with pixels in the image
    assert slot(2, (19, 21))[4] == -1 and tuple(slot(2, (19, 21))[:2]) == tuple(slot(2, (19, 21))[2:4]) and slot(2, (19, 21))[6] != 1     # a disc
    out = slot(3, (18, 20))
    assert out[6] == 1 and out[7] == 1 and out[4] > 0 and max(out[0], out[2]) < 0           # set up, no pixel
    assert (slot(4, (8, 11)) == empty).all()
    on = slot(5, (8, 11))
    assert on[2] == -16 * 80 and on[4] > 0 and on[6] != 1              # kept; the part inside the image is drawn
    for k in range(6):                                                 # frame k alone is frame k of the chunk, records included
        one, r1, g1 = plot.draw_prepared(p, dev(data), dev(trajec), dev(mins), dev(maxs), [k], return_records=True)
        assert np.array_equal(one[0].cpu().numpy(), rgb[k]) and np.array_equal(g1[0].cpu().numpy(), gr[k])
        assert np.array_equal(r1[0].cpu().numpy(), rec[k, :r1.shape[1]]) and (rec[k, r1.shape[1]:] == empty).all()


def test_ground_behind_the_camera_and_ground_beyond_every_border():
    p = plot_of("smpl", 80)
    data, trajec, mins, maxs = (np.array(v) for v in take_of("smpl", 8))
    far = maxs.copy()
    far[2] = 60.0                                                       # the quad reaches behind the camera
    corners = [(mins[0] - trajec[3, 0], 0.0, far[2] - trajec[3, 1]), (mins[0] - trajec[3, 0], 0.0, mins[2] - trajec[3, 1])]
    assert pr.to_clip(p.M, corners[0])[2] < pr.W_MIN < pr.to_clip(p.M, corners[1])[2]
    rgb, rec, gr, _ = check("ground behind the camera", p, data, trajec, mins, far, [3])
    assert gr[0, 0] >= 4
    wide_lo, wide_hi = np.asarray([-50.0, mins[1], -50.0], np.float32), np.asarray([50.0, maxs[1], 20.0], np.float32)
    rgb, rec, gr, _ = check("ground beyond every border", p, data, trajec, wide_lo, wide_hi, [3, 4])
    assert (gr[:, 0] >= 4).all() and rgb.max(axis=-1).max() < 255 and (rgb[:, [0, -1]] == 192).all() and (rgb[:, :, [0, -1]] == 192).all()
    part_lo, part_hi = np.asarray([-50.0, mins[1], -50.0], np.float32), np.asarray([6.0, maxs[1], 20.0], np.float32)
    _, _, gr5, _ = check("ground with a slanted side through the band", p, data, trajec, part_lo, part_hi, [3])
    assert gr5[0, 0] > 4                                                # the side x = 6 runs from inside the band out of it: a corner more
    g = 16 * 80
    assert (np.abs(gr[:, 4:22]).max() <= 2 * g) and (gr[:, 4:22].min() == -g) and (gr[:, 4:22].max() == 2 * g)      # cut at the band on every side


def test_screen_space_segments_at_the_limits_of_the_integers():
    """A camera that hands the joints through (clip = (x, y, ., 1), pixel = clip / 16) puts every end on a chosen grid point of a 512-pixel image: the
    longest segment the guard band holds at the largest half-width (R^2 L2 = 2.0e16, past the integers a double holds), T at perfect squares above
    2^53 and at squares +- 1, a disc on the band's corner, a segment one unit inside the band's far corner."""
    size, g = 512, 16 * 512
    ends = [((-g, -g), (2 * g, 2 * g), 4095),                          # corner to corner of the band: L2 = 2 x 24576^2
            ((100, 16000), (100 + 14400, 16000 - 19200), 4095),        # a 3-4-5 triangle: R^2 L2 = (4095 x 24000)^2 = 9.66e15 > 2^53, T = 98 280 000
            ((-g, 3000), (-g + 20000, 3200), 1),                       # L2 = 20001^2 - 1: T = 20000
            ((2 * g, 5000), (2 * g - 24000, 5001), 1),                 # L2 = 24000^2 + 1: T = 24000
            ((-g, 2 * g), (-g, 2 * g), 4095),                          # a disc on the band's corner: it reaches no pixel
            ((4000, 4000), (4000, 4000), 44),                          # a disc in the picture
            ((2 * g - 1, 2 * g - 1), (1000, 6000), 22),
            ((3000, 100), (3000, 8100), 182)]                          # vertical: L2 a perfect square
    chains = tuple((2 * k, 2 * k + 1) for k in range(len(ends)))
    M = np.asarray([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1.0]])
    p = plot.Plot(chains, size=size, camera=(M, np.asarray([[1 / 16, 0, 0], [0, 1 / 16, 0]])), half_widths=[r for _, _, r in ends])
    data = np.asarray([[(x, y, 0.0) for a, b, _ in ends for x, y in (a, b)]], dtype=np.float32)
    zero = np.zeros(3, np.float32)
    rgb, rec, gr, _ = check("screen space", p, data, np.zeros((1, 2), np.float32), zero, zero, [0])
    for k, (a, b, r) in enumerate(ends):
        assert tuple(rec[0, k, :4]) == (*a, *b) and rec[0, k, 5] == (r | (2 + k) << 16)
    assert list(rec[0, :6, 4]) == [pr.isqrt(4095 ** 2 * 2 * 24576 ** 2), 98280000, 20000, 24000, -1, -1] and rec[0, 7, 4] == 182 * 8000
    assert rec[0, 4, 6] == 1 and rec[0, 0, 6] == 511 << 16 and gr[0, 0] == 0 and (rgb[0] != 255).any(-1).mean() > 0.3


def walk_rounds(rec, nrec, size):
    """What the walk of each tile's workgroup does with one frame, from the kernel's constants: per tile the list's length after each round's
    append, and how many chunks that round then drew."""
    out = {}
    x0, x1, y0, y1 = rec[:nrec, 6] & 0xffff, rec[:nrec, 6] >> 16, rec[:nrec, 7] & 0xffff, rec[:nrec, 7] >> 16
    for ty in range(-(-size // plot.TILE)):
        for tx in range(-(-size // plot.TILE)):
            X0, Y0 = tx * plot.TILE, ty * plot.TILE
            hit = (x0 <= x1) & (x0 <= X0 + plot.TILE - 1) & (x1 >= X0) & (y0 <= Y0 + plot.TILE - 1) & (y1 >= Y0)
            count, rounds = 0, []
            for base in range(0, nrec, plot.WALK):
                kept, count = count, count + int(hit[base:base + plot.WALK].sum())
                rounds.append((kept, count, count // plot.CHUNK))
                if count >= plot.CHUNK:
                    count %= plot.CHUNK
            out[(tx, ty)] = rounds
    return out


def test_a_long_take_walks_the_records_in_rounds_and_draws_in_chunks():
    """The last two frames of an 1100-frame take whose root circles on the spot: 1119 slots are more than one round of a tile's walk (plot.WALK), the
    tile under the root lists more than plot.CHUNK of them, a remainder is carried into the second round and drawn behind it."""
    p = plot_of("smpl", 64)
    data, trajec, mins, maxs = take_of("smpl", 1100, step=0.0004, turn=0.05, burst=90)
    rgb, rec, gr, _ = check("long take", p, data, trajec, mins, maxs, [1098, 1099])
    assert rec.shape[1] == 21 + 1098 and list(gr[:, 1]) == [21 + 1097, 21 + 1098]
    flat = [r for f in range(2) for per_tile in walk_rounds(rec[f], int(gr[f, 1]), 64).values() for r in [per_tile]]
    rounds = [r for per_tile in flat for r in per_tile]
    carried_and_drew = sum(1 for kept, count, drew in rounds if kept > 0 and drew > 0)
    several_chunks = sum(1 for kept, count, drew in rounds if drew > 1)
    print(f"long take: {len(flat)} tile walks of {len(flat[0])} rounds; rounds that appended behind a remainder and drew: {carried_and_drew}, rounds that drew "
          f"several chunks: {several_chunks}, longest list {max(c for _, c, _ in rounds)}")
    assert len(flat[0]) == 2 and carried_and_drew > 0 and several_chunks > 0 and max(c for _, c, _ in rounds) > plot.CHUNK


# ---- determinism, graphs ----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal_and_draw_is_prepare_then_draw_prepared():
    p = plot_of("smplx", 80)
    j = dev(pr.walking_take(12, 52, plot.SMPLX_CHAINS))
    first = plot.draw(p, j)
    assert first.shape == (12, 80, 80, 3) and first.dtype == torch.uint8 and first.is_cuda
    assert torch.equal(first, plot.draw(p, j)) and torch.equal(first[[2, 11]], plot.draw(p, j, frames=[2, 11]))
    data, trajec, mins, maxs = plot.prepare(j)
    assert torch.equal(first[5:9], plot.draw_prepared(p, data, trajec, mins, maxs, range(5, 9)))
    assert plot.draw(p, j, frames=[]).shape == (0, 80, 80, 3)


def test_stages_in_a_cuda_graph():
    p = plot_of("smpl", 64)
    take = pr.walking_take(10, 22, plot.SMPL_CHAINS)
    data, trajec, mins, maxs = (dev(np.array(v)) for v in plot.prepare(take))
    frames = torch.tensor([2, 9, 5], dtype=torch.int32, device=DEV)
    want = plot.draw_prepared(p, data, trajec, mins, maxs, [2, 9, 5])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        assert torch.equal(plot.draw_prepared(p, data, trajec, mins, maxs, frames), want)          # warm: the tables are on the device before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = plot.draw_prepared(p, data, trajec, mins, maxs, frames)
    frames.copy_(torch.tensor([7, 0, 1], dtype=torch.int32, device=DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, plot.draw_prepared(p, data, trajec, mins, maxs, [7, 0, 1])) and not torch.equal(got, want)
    frames.copy_(torch.tensor([2, 9, 5], dtype=torch.int32, device=DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- the script and the reference's call ------------------------------------------------------------------------------------------------------------
def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_plot_from_results_writes_videos_that_decode_to_the_frames(tmp_path, capsys):
    """The files' frames are `video.jpeg_frames` of `plot.draw`'s output byte for byte, and PIL decodes them as close to it as DESIGN.md §24 gates the
    encoder: not more than 0.5 dB below PIL's own encoder at the same quality and 4:2:0 on the same picture."""
    from PIL import Image
    spec = importlib.util.spec_from_file_location("plot_from_results", os.path.join(REPO, "scripts", "plot_from_results.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    take = pr.walking_take(5, 52, plot.SMPLX_CHAINS, seed=4)
    feats = (0.1 * np.random.default_rng(8).normal(size=(4, 623))).astype(np.float32)
    feats[:, 3] += 0.9
    np.save(tmp_path / "rec_a.npy", take)
    np.save(tmp_path / "rec_b.npy", feats)
    sound = (0.3 * np.sin(np.arange(4000) * 0.05)).astype(np.float32)
    for name in ("rec_a", "rec_b"):
        with wave_file.open(str(tmp_path / f"{name}.wav"), "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(8000)
            f.writeframes(np.rint(32767 * sound).astype("<i2").tobytes())
    out = script.main([str(tmp_path), "--out", str(tmp_path / "o"), "--size", "80", "--fps", "20", "--smplx-chains", "--chunk", "2", "--waves", str(tmp_path)])
    videos = [str(tmp_path / "o" / "rec_a.avi"), str(tmp_path / "o" / "rec_b.avi")]
    assert out == {"takes": 2, "frames": 9, "size": 80, "out": str(tmp_path / "o"), "videos": videos}
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == out
    p = plot.Plot(plot.SMPLX_CHAINS, size=80)
    for path, j in ((videos[0], dev(take)), (videos[1], joints.recover_from_ric(dev(feats), 52))):
        avi = jr.read_avi(open(path, "rb").read())
        want = plot.draw(p, j)
        assert len(avi["frames"]) == len(want) and avi["frames"] == video.jpeg_frames(want, 90) and len(avi["audio"]) == len(want)
        want = want.cpu().numpy()
        assert (want != 255).any()
        for k, raw in enumerate(avi["frames"]):
            got = np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))
            buf = io.BytesIO()
            Image.fromarray(want[k]).save(buf, "JPEG", quality=90, subsampling=2)
            pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
            ours, theirs = psnr(got, want[k]), psnr(pil, want[k])
            print(f"{os.path.basename(path)} frame {k}: PIL's decode of our file {ours:.2f} dB, of PIL's own encode {theirs:.2f} dB")
            assert got.shape == (80, 80, 3) and ours >= theirs - 0.5
    # the reference's call: numpy joints in, a file out; a 22-joint tree, a title that is ignored
    stats = plot.plot_3d_motion(str(tmp_path / "call.avi"), plot.SMPL_CHAINS, take[:3, :22], title="None", fps=30, radius=4, size=64, chunk=2)
    avi = jr.read_avi(open(tmp_path / "call.avi", "rb").read())
    assert stats["frames"] == 3 and avi["frames"] == video.jpeg_frames(plot.draw(plot.Plot(size=64), dev(take[:3, :22])), 90)


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    p = plot_of("smplx", 64)
    take = pr.walking_take(4, 52, plot.SMPLX_CHAINS)
    with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
        plot.draw(p, torch.from_numpy(take))
    with pytest.raises(ValueError, match="joint 51"):
        plot.draw(p, dev(take[:, :22]))
    with pytest.raises(ValueError, match="indices into the take"):
        plot.draw(p, dev(take), frames=[4])
    with pytest.raises(ValueError, match="int32"):
        plot.draw(p, dev(take), frames=torch.zeros(2, dtype=torch.int64, device=DEV))


def test_native_calls_with_an_exact_workspace_and_the_c_abi_checks():
    p = plot_of("smpl", 80)
    data, trajec, mins, maxs, _ = edge_take(p)
    frames = [0, 1, 2, 3, 4, 5]
    rgb_want, rec_want, gr_want = (t.cpu().numpy() for t in plot.draw_prepared(p, dev(data), dev(trajec), dev(mins), dev(maxs), frames, return_records=True))
    lib, st, t = _lib.load(), _lib.current_stream(torch.device(DEV)), p.on(DEV)
    m, J, S, n, size, P = 6, 22, 21, 6, 80, 21 + 4
    nbytes = lib.syn_plot_workspace_bytes(m, P)
    assert nbytes == 32 * m * P + 96 * m and lib.syn_plot_workspace_bytes(0, P) == -1 and lib.syn_plot_workspace_bytes(m, 0) == -1
    # both buffers the kernels write lie in one arena with 256 bytes of 0x5A before, between and behind them, which must stay as they are
    sizes = {"ws": nbytes, "rgb": m * size * size * 3}
    offsets, end = {}, 256
    for name, sz in sizes.items():
        offsets[name], end = end, (end + sz + 255) // 256 * 256 + 256
    arena = torch.full((end,), 0x5A, dtype=torch.uint8, device=DEV)
    padding = torch.ones(end, dtype=torch.bool, device=DEV)
    for name, o in offsets.items():
        padding[o:o + sizes[name]] = False
    ws, rgb = arena[offsets["ws"]:offsets["ws"] + nbytes], arena[offsets["rgb"]:offsets["rgb"] + sizes["rgb"]]
    d, tr, ix = dev(data), dev(trajec), torch.tensor(frames, dtype=torch.int32, device=DEV)
    bounds = dev(np.asarray([mins[0], maxs[0], mins[2], maxs[2]], np.float32))

    def setup(data=d.data_ptr(), frames=m, nj=J, trajec=tr.data_ptr(), take=n, index=ix.data_ptr(), bnd=bounds.data_ptr(), seg=t["segments"].data_ptr(), ns=S,
              cam=t["camera"].data_ptr(), sz=size, tr_r=p.traj_half_width, slots=P, work=ws.data_ptr()):
        return lib.syn_plot_setup(data, frames, nj, trajec, take, index, bnd, seg, ns, cam, sz, tr_r, slots, work, st)

    def draw(work=ws.data_ptr(), frames=m, slots=P, col=t["colours"].data_ptr(), layers=len(p.colours), sz=size, out=rgb.data_ptr()):
        return lib.syn_plot_draw(work, frames, slots, col, layers, sz, out, st)

    def refused(rc, word):
        assert rc != 0 and word in lib.syn_last_error().decode(), (rc, lib.syn_last_error())

    # what cannot run is refused before any launch
    for name in ("data", "trajec", "index", "bnd", "seg", "cam", "work"):
        refused(setup(**{name: None}), "null")
    for name in ("work", "col", "out"):
        refused(draw(**{name: None}), "null")
    for call in (setup, draw):
        refused(call(sz=0), "4096")
        refused(call(sz=4097), "4096")
        refused(call(frames=-1), "negative")
        assert call(frames=0) == 0
        refused(call(work=ws.data_ptr() + 8), "aligned")
    refused(setup(nj=0), "joints")
    refused(setup(ns=0), "segments")
    refused(setup(take=0), "take")
    refused(setup(slots=S - 1), "n_slots")
    refused(setup(tr_r=0), "4095")
    refused(setup(tr_r=4096), "4095")
    refused(setup(seg=t["segments"].data_ptr() + 4), "aligned")
    refused(draw(slots=0), "slots")
    refused(draw(layers=1), "layers")
    torch.cuda.synchronize()
    assert (arena == 0x5A).all()                                        # nothing ran
    # the two calls with a workspace of exactly the size asked for
    assert setup() == 0 and draw() == 0
    torch.cuda.synchronize()
    cut = 32 * m * P
    assert np.array_equal(ws[:cut].view(torch.int32).view(m, P, 8).cpu().numpy(), rec_want)
    assert np.array_equal(ws[cut:].view(torch.int32).view(m, 24).cpu().numpy(), gr_want)
    assert np.array_equal(rgb.view(m, size, size, 3).cpu().numpy(), rgb_want)
    assert (arena[padding] == 0x5A).all()                               # no kernel wrote a byte outside its outputs or the workspace it asked for
    # an index outside the take: no ground, no trajectory, the chains still drawn; a layer outside the colour table is skipped
    ix.copy_(torch.tensor([0, 1, 2, 3, 4, 99], dtype=torch.int32, device=DEV))
    assert setup() == 0 and draw(layers=4) == 0
    torch.cuda.synchronize()
    got_gr = ws[cut:].view(torch.int32).view(m, 24).cpu().numpy()
    assert got_gr[5, 0] == 0 and got_gr[5, 1] == S and np.array_equal(got_gr[:5], gr_want[:5])
    want = pr.draw_ref(ws[:cut].view(torch.int32).view(m, P, 8).cpu().numpy(), got_gr, p.colours, size, n_layers=4)
    assert np.array_equal(rgb.view(m, size, size, 3).cpu().numpy(), want) and (arena[padding] == 0x5A).all()
