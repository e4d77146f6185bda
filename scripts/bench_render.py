#!/usr/bin/env python3
"""Renderer timing (not the contract bench): 1 and 8 takes of 60 s (1800 frames at 30 fps each) drawn at 960 x 720, one panel of the reference's video,
on a SYNTHETIC mesh of SMPL-X's size: the vertices of tests/smplx_mesh_ref.synth_model (V = 10 475) posed by syntalker_amd.mesh, and a synthetic
face list of 20 908 triangles that joins every template vertex to near neighbours (the model file is not redistributable).  The synthetic body is a
cloud, not a skin: more layers behind each other and larger triangles than the real mesh, so the table is an upper bound for it rather than its time.

There is nothing to compare against: the parent has no renderer on the device and the reference's (pyrender) runs neither here nor on the GPU box.
No speed-up is claimed.  Per case: frames/s over the three stages, us per frame of each stage (device events around the stage's launches, `--chunk`
frames per call, summed over the take; `raster` = the box, union and bin-and-draw kernels, which one entry point enqueues - the bin and the draw of a
supertile share a workgroup and cannot be timed apart from outside; see `boxes`), the share of empty tiles (64 x 16 pixels, a wave's) and supertiles (64 x
64, a workgroup's), and the mean number of faces whose box meets a non-empty one, counted on the host from the device's xy_sub of sampled frames.

`boxes` (left out with --no-split) times the raster entry point on the same vertices seen by a camera 50 m to the side: every face is outside the guard band, so the box
kernel drops them all, the union is empty and every supertile leaves at once and stores its background - `boxes` is the box and union kernels plus
the stores, and `raster` - `boxes` what binning and drawing cost together.

    python scripts/bench_render.py [--chunk 120] [--rounds 3] [--takes 1 8] [--no-split] [--out profiles/render_bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import mesh, render  # noqa: E402
from tests import smplx_mesh_ref as sm  # noqa: E402

FRAMES, V, E, FACES, W, H = 1800, 10475, 100, 20908, 960, 720


def neighbour_faces(points, n_faces):
    """Triangles (v, a, b) over each vertex's nearest neighbours: (v, nn1, nn2), then (v, nn2, nn3), ... until n_faces."""
    p = torch.from_numpy(np.asarray(points, dtype=np.float32))
    nn = []
    for s in range(0, len(p), 1024):
        d = torch.cdist(p[s:s + 1024], p)
        nn.append(d.topk(4, largest=False).indices[:, 1:])          # (the nearest is the vertex itself)
    nn = torch.cat(nn).numpy()
    v = np.arange(len(p))
    faces = np.concatenate([np.stack([v, nn[:, 0], nn[:, 1]], 1), np.stack([v, nn[:, 1], nn[:, 2]], 1)])
    return np.ascontiguousarray(faces[:n_faces].astype(np.int32))


def tile_stats(xy, faces, tile_w, tile_h):
    """One frame: (share of empty tiles, mean faces whose pixel box meets a non-empty tile)."""
    g = 16 * max(W, H)
    t = xy[faces]                                                   # (F, 3, 2)
    ok = ((t[..., 0] >= -g) & (t[..., 0] <= 16 * W + g) & (t[..., 1] >= -g) & (t[..., 1] <= 16 * H + g)).all(1)
    x0, x1 = np.maximum((t[..., 0].min(1) + 7) >> 4, 0), np.minimum((t[..., 0].max(1) - 8) >> 4, W - 1)
    y0, y1 = np.maximum((t[..., 1].min(1) + 7) >> 4, 0), np.minimum((t[..., 1].max(1) - 8) >> 4, H - 1)
    ok &= (x0 <= x1) & (y0 <= y1)
    nx, ny = -(-W // tile_w), -(-H // tile_h)
    acc = np.zeros((ny + 1, nx + 1), dtype=np.int64)
    tx0, tx1, ty0, ty1 = x0[ok] // tile_w, x1[ok] // tile_w, y0[ok] // tile_h, y1[ok] // tile_h
    np.add.at(acc, (ty0, tx0), 1), np.add.at(acc, (ty1 + 1, tx1 + 1), 1), np.add.at(acc, (ty0, tx1 + 1), -1), np.add.at(acc, (ty1 + 1, tx0), -1)
    count = acc.cumsum(0).cumsum(1)[:ny, :nx]
    full = count > 0
    return float(1 - full.mean()), float(count[full].mean()) if full.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--takes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--no-split", dest="split", action="store_false", help="leave the `boxes` column out (a third fewer raster calls)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_bench.txt"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    dev = "cuda"
    md = sm.synth_model(0, V, E=E, max_weights=8)
    faces = neighbour_faces(md["v_template"], FACES)
    scene = render.Scene(faces, n_vertices=V)
    away = render.Scene(faces, n_vertices=V, camera_pose=render.reference_camera() + np.asarray([[0, 0, 0, 50.0]] + [[0, 0, 0, 0]] * 3))
    lines = [f"# scripts/bench_render.py --chunk {a.chunk} --rounds {a.rounds}{'' if a.split else ' --no-split'}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# synthetic mesh of SMPL-X's size (V = {V}, {FACES} faces over nearest neighbours), {W} x {H}, a take = {FRAMES} frames, {a.chunk} frames a "
             "call; us per frame (median over the rounds of the take's total); no renderer to compare against: no speed-up claimed"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for takes in a.takes:
        betas = np.random.RandomState(1).randn(300).astype(np.float32) * 0.3
        m = mesh.smplx_mesh(md, betas, flat_hand_mean=True)
        totals = {k: [] for k in ("project", "raster", "shade") + (("boxes",) if a.split else ())}
        stats, covered = [], []
        tr = np.zeros((FRAMES, 3), np.float32)                       # standing on the reference's floor, swaying 0.2 m
        tr[:, 1] = 1.0
        tr[:, 0] = 0.2 * np.sin(np.arange(FRAMES) / 90.0)
        inputs = [sm.case_inputs(100 + take, FRAMES, E, amp=0.08)[:2] for take in range(takes)]
        for rnd in range(a.rounds + 1):                              # round 0 warms up
            t = dict.fromkeys(totals, 0.0)
            for take in range(takes):
                pose, ex = inputs[take]
                for c in range(0, FRAMES, a.chunk):
                    s = slice(c, c + a.chunk)
                    verts = mesh.smplx_vertices(m, torch.from_numpy(pose[s]).to(dev), torch.from_numpy(ex[s]).to(dev), torch.from_numpy(tr[s]).to(dev))
                    torch.cuda.synchronize()
                    ev[0].record()
                    xy, z, normal = render.project(scene, verts, W, H)
                    ev[1].record()
                    face_id, depth = render.rasterize(scene, xy, z, W, H)
                    ev[2].record()
                    rgb = render.shade(scene, face_id, xy, normal)
                    ev[3].record()
                    torch.cuda.synchronize()
                    for k, name in enumerate(("project", "raster", "shade")):
                        t[name] += ev[k].elapsed_time(ev[k + 1]) * 1e3
                    if a.split:
                        axy, az, _ = render.project(away, verts, W, H)
                        torch.cuda.synchronize()
                        ev[0].record()
                        render.rasterize(away, axy, az, W, H)
                        ev[1].record()
                        torch.cuda.synchronize()
                        t["boxes"] += ev[0].elapsed_time(ev[1]) * 1e3
                    if rnd == 0 and take == 0 and c % (5 * a.chunk) == 0:
                        x = xy[0].cpu().numpy().astype(np.int64)
                        stats.append(tile_stats(x, faces, 64, 16) + tile_stats(x, faces, 64, 64))
                        covered.append(float((face_id[0] >= 0).float().mean()))
                    del verts, xy, z, normal, face_id, depth, rgb
            if rnd:
                for k in totals:
                    totals[k].append(t[k] / (takes * FRAMES))
        med = {k: sorted(v)[len(v) // 2] for k, v in totals.items()}
        st = np.asarray(stats).mean(0)
        per_frame = med["project"] + med["raster"] + med["shade"]
        res = {"takes": takes, "frames": takes * FRAMES, "width": W, "height": H, "vertices": V, "faces": FACES, "chunk": a.chunk,
               "frames_per_s": round(1e6 / per_frame, 1), "us_per_frame": {k: round(v, 1) for k, v in med.items()},
               "us_per_frame_range": {k: [round(min(v), 1), round(max(v), 1)] for k, v in totals.items()},
               "covered_share_of_image": round(float(np.mean(covered)), 4),
               "empty_tiles_64x16": round(st[0], 4), "faces_per_nonempty_tile": round(st[1], 1),
               "empty_supertiles_64x64": round(st[2], 4), "faces_per_nonempty_supertile": round(st[3], 1),
               "output_gb_per_s": {"raster": round(W * H * 8 / med["raster"] / 1e3, 1), "shade": round(W * H * 3 / med["shade"] / 1e3, 1)}}
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
