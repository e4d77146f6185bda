#!/usr/bin/env python3
"""Stick-figure timing (not the contract bench): a 196-frame and an 1800-frame take (tests/plot_ref.walking_take: a figure that walks a turning path)
drawn at 1000 x 1000, the reference's figure, with the 5 body chains (22 joints) and with all 15 (52 joints).

There is nothing to compare against on the device: the parent has no stick-figure renderer and the reference's (matplotlib + ffmpeg) is another
renderer on the host.  No speed-up is claimed and no time is gated.  Per case: us per frame of `setup` (syn_plot_setup: the record and the ground
kernels) and of `draw` (syn_plot_draw), device events around each call, `--chunk` frames a call, summed over the take, the median of `--rounds` rounds
after a warm-up; the same per chunk for the first, the middle and the last full chunk of the take (the trajectory, and with it the slots a tile walks, grows
with the frame index); and the share of 32 x 32 tiles that no record's pixel box meets, counted on the host from the device's records of sampled
frames (such a tile stores white, or white under the ground, without drawing).  Where matplotlib imports (and without --no-matplotlib), the host's Agg renderer
draws a few frames of the same scene beside it: a different renderer (other caps, other anti-aliasing, depth-sorted artists), timed on the host clock.

    python scripts/bench_plot.py [--chunk 64] [--rounds 3] [--frames 196 1800] [--size 1000] [--no-matplotlib] [--out profiles/plot_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import plot  # noqa: E402
from tests import plot_ref as pr  # noqa: E402


def empty_tile_share(rec, nrec, size):
    """One frame: the share of tiles that no record's pixel box meets, and the mean records per tile that one meets."""
    r = rec[:nrec]
    x0, x1, y0, y1 = r[:, 6] & 0xffff, r[:, 6] >> 16, r[:, 7] & 0xffff, r[:, 7] >> 16
    ok = x0 <= x1
    nt = -(-size // plot.TILE)
    acc = np.zeros((nt + 1, nt + 1), dtype=np.int64)
    tx0, tx1, ty0, ty1 = x0[ok] // plot.TILE, x1[ok] // plot.TILE, y0[ok] // plot.TILE, y1[ok] // plot.TILE
    np.add.at(acc, (ty0, tx0), 1), np.add.at(acc, (ty1 + 1, tx1 + 1), 1), np.add.at(acc, (ty0, tx1 + 1), -1), np.add.at(acc, (ty1 + 1, tx0), -1)
    count = acc.cumsum(0).cumsum(1)[:nt, :nt]
    met = count > 0
    return float(1 - met.mean()), float(count[met].mean()) if met.any() else 0.0


def matplotlib_ms_per_frame(take, chains, size, frames):
    """Host milliseconds per frame of matplotlib's Agg renderer on the reference's scene (None when matplotlib does not import)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from mpl_toolkits.mplot3d.art3d import Poly3DCollection
    except ImportError:
        return None
    data, trajec, mins, maxs = plot.prepare(take)
    fig = plt.figure(figsize=(10, 10), dpi=size / 10)
    ax = fig.add_subplot(111, projection="3d")
    t0 = time.perf_counter()
    for k in frames:
        ax.cla()
        ax.view_init(elev=120, azim=-90)
        ax._dist = 5.5
        ax.set_xlim3d([-2, 2]), ax.set_ylim3d([0, 4]), ax.set_zlim3d([0, 4])
        x0, x1, z0, z1 = mins[0] - trajec[k, 0], maxs[0] - trajec[k, 0], mins[2] - trajec[k, 1], maxs[2] - trajec[k, 1]
        quad = Poly3DCollection([[[x0, 0, z0], [x0, 0, z1], [x1, 0, z1], [x1, 0, z0]]])
        quad.set_facecolor((0.5, 0.5, 0.5, 0.5))
        ax.add_collection3d(quad)
        if k > 1:
            ax.plot3D(trajec[:k, 0] - trajec[k, 0], np.zeros(k), trajec[:k, 1] - trajec[k, 1], linewidth=1.0, color="blue")
        for i, chain in enumerate(chains):
            ax.plot3D(data[k, list(chain), 0], data[k, list(chain), 1], data[k, list(chain), 2], linewidth=plot.chain_width_pt(i), color=plot.CHAIN_COLOURS[i])
        plt.axis("off")
        fig.canvas.draw()
    ms = (time.perf_counter() - t0) * 1e3 / len(frames)
    plt.close(fig)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[196, 1800])
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--no-matplotlib", dest="matplotlib", action="store_false", help="leave the host renderer out")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plot_bench.txt"))
    a = ap.parse_args()
    dev = "cuda"
    lines = [f"# scripts/bench_plot.py --chunk {a.chunk} --rounds {a.rounds} --size {a.size}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# a walking figure at {a.size} x {a.size}, {a.chunk} frames a call; us per frame (median over the rounds of the take's total); nothing on the "
             "device to compare against: no speed-up claimed, no time gated"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for n in a.frames:
        for name, chains, J in (("smpl", plot.SMPL_CHAINS, 22), ("smplx", plot.SMPLX_CHAINS, 52)):
            take = pr.walking_take(n, J, chains)
            p = plot.Plot(chains, size=a.size)
            data, trajec, mins, maxs = plot.prepare(torch.from_numpy(take).to(dev))
            starts = list(range(0, n, a.chunk))
            per_chunk = {"setup": np.zeros((a.rounds, len(starts))), "draw": np.zeros((a.rounds, len(starts)))}
            stats = []
            for rnd in range(a.rounds + 1):                          # round 0 warms up
                for c, k in enumerate(starts):
                    frames = range(k, min(n, k + a.chunk))
                    torch.cuda.synchronize()
                    ev[0].record()
                    r = plot.setup(p, data, trajec, mins, maxs, frames)
                    ev[1].record()
                    rgb = plot.paint(p, r)
                    ev[2].record()
                    torch.cuda.synchronize()
                    if rnd:
                        per_chunk["setup"][rnd - 1, c] = ev[0].elapsed_time(ev[1]) * 1e3
                        per_chunk["draw"][rnd - 1, c] = ev[1].elapsed_time(ev[2]) * 1e3
                    elif c % max(1, len(starts) // 6) == 0:
                        rec, gr = r.records[0].cpu().numpy(), r.grounds[0].cpu().numpy()
                        stats.append(empty_tile_share(rec, int(gr[1]), a.size) + (float((rgb[0] != 255).any(-1).float().mean()),))
                    del r, rgb
            sizes = np.asarray([min(n, k + a.chunk) - k for k in starts])
            full = max(1, int((sizes == a.chunk).sum()))             # (a short last chunk carries a call's fixed cost on few frames: not shown)
            totals = {k: v.sum(1) / n for k, v in per_chunk.items()}
            med = {k: float(np.median(v)) for k, v in totals.items()}
            growth = {k: {f"frames {starts[c]}-{starts[c] + sizes[c] - 1}": round(float(np.median(v[:, c]) / sizes[c]), 1) for c in sorted({0, full // 2, full - 1})}
                      for k, v in per_chunk.items()}
            st = np.asarray(stats).mean(0)
            res = {"frames": n, "chains": name, "segments": int(len(p.segments)), "size": a.size, "chunk": a.chunk,
                   "frames_per_s": round(1e6 / (med["setup"] + med["draw"]), 1), "us_per_frame": {k: round(v, 1) for k, v in med.items()},
                   "us_per_frame_range": {k: [round(float(v.min()), 1), round(float(v.max()), 1)] for k, v in totals.items()},
                   "us_per_frame_by_chunk": growth, "tiles_no_record_meets": round(float(st[0]), 4), "records_per_met_tile": round(float(st[1]), 1),
                   "painted_share_of_image": round(float(st[2]), 4), "output_gb_per_s_draw": round(a.size * a.size * 3 / med["draw"] / 1e3, 1)}
            if a.matplotlib:
                ms = matplotlib_ms_per_frame(take, chains, a.size, list(range(0, n, max(1, n // 5)))[:5])
                res["matplotlib_agg_host_ms_per_frame_a_different_renderer"] = None if ms is None else round(ms, 1)
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
