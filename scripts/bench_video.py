#!/usr/bin/env python3
"""JPEG encoder timing (not the contract bench): 1 and 8 takes of 60 s (1800 frames each) at 960 x 720 (one panel) and 1920 x 720 (two panels side
by side), drawn by syntalker_amd.render on scripts/bench_render.py's synthetic mesh and encoded where they were drawn (syntalker_amd/video.py,
csrc/syn_jpeg.inc).  The synthetic body is a cloud that covers four fifths of the panel, not a grey body on white: it compresses worse than a real
take, so bytes per frame are an upper bound.

Per case, us per frame (device events around each native call, `--chunk` frames a call, summed over the take, median over the rounds): `transform`
(colour, 4:2:0, DCT, quantisation), `count` (the entropy coder counting, and the offsets), `write` (the entropy coder again, storing); `files` is
`video.jpeg_frames` on the host clock - the three stages, the synchronisation for the offsets and the copy of the files to the host; bytes per frame.

Beside them two host paths on the first `--chunk` frames of the first take (host clock, us per frame): `bmp` = the raw frames copied to the host and
written by render.write_bmp into a temporary directory (what scripts/render_from_results.py did before --format avi), `pil` = the raw frames copied
and encoded by PIL's libjpeg at the same quality and 4:2:0 on 16 threads (left out where PIL is missing).  No target is set and no speed-up claimed.

    python scripts/bench_video.py [--chunk 120] [--rounds 2] [--takes 1 8] [--quality 90] [--out profiles/video_bench.txt]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import _lib, mesh, render, video  # noqa: E402
from tests import smplx_mesh_ref as sm  # noqa: E402

_spec = importlib.util.spec_from_file_location("bench_render", os.path.join(REPO, "scripts", "bench_render.py"))
bench_render = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench_render)
FRAMES, V, E, FACES, H = bench_render.FRAMES, bench_render.V, bench_render.E, bench_render.FACES, bench_render.H


def staged(rgb, quality, ev):
    """video._encode with an event between the native calls: -> (us of transform, count, write; bytes)."""
    n, height, width = rgb.shape[:3]
    lib, st = _lib.load(), _lib.current_stream(rgb.device)
    ws = torch.empty(lib.syn_jpeg_workspace_bytes(n, width, height), dtype=torch.uint8, device=rgb.device)
    head = video._header_on(rgb.device, width, height, quality)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=rgb.device)
    ev[0].record()
    _lib.check(lib.syn_jpeg_transform(rgb.data_ptr(), int(rgb.stride(0)), n, width, height, quality, ws.data_ptr(), st), "syn_jpeg_transform")
    ev[1].record()
    _lib.check(lib.syn_jpeg_measure(n, width, height, int(head.numel()), ws.data_ptr(), offsets.data_ptr(), st), "syn_jpeg_measure")
    ev[2].record()
    total = int(offsets[-1].item())
    data = torch.empty(total, dtype=torch.uint8, device=rgb.device)
    ev[3].record()
    _lib.check(lib.syn_jpeg_write(n, width, height, head.data_ptr(), int(head.numel()), ws.data_ptr(), offsets.data_ptr(), data.data_ptr(), total, st), "syn_jpeg_write")
    ev[4].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3, ev[1].elapsed_time(ev[2]) * 1e3, ev[3].elapsed_time(ev[4]) * 1e3, total


def host_paths(rgb, quality):
    """us per frame of the two host paths over the frames of `rgb`, and PIL's bytes per frame."""
    n = rgb.shape[0]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = rgb.cpu().numpy()
        for k in range(n):
            render.write_bmp(os.path.join(tmp, f"frame_{k}.bmp"), img[k])
        out["bmp_us"] = (time.perf_counter() - t0) * 1e6 / n
    try:
        from PIL import Image
    except ImportError:
        return out
    import io
    from concurrent.futures import ThreadPoolExecutor

    def one(frame):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "JPEG", quality=quality, subsampling=2)
        return buf.getbuffer().nbytes

    with ThreadPoolExecutor(16) as pool:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sizes = list(pool.map(one, rgb.cpu().numpy()))
        out["pil_us"] = (time.perf_counter() - t0) * 1e6 / n
    out["pil_bytes"] = sum(sizes) / n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--takes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--widths", type=int, nargs="+", default=[960, 1920])
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "video_bench.txt"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    dev = "cuda"
    md = sm.synth_model(0, V, E=E, max_weights=8)
    faces = bench_render.neighbour_faces(md["v_template"], FACES)
    scene = render.Scene(faces, n_vertices=V)
    m = mesh.smplx_mesh(md, np.random.RandomState(1).randn(300).astype(np.float32) * 0.3, flat_hand_mean=True)
    tr = np.zeros((FRAMES, 3), np.float32)
    tr[:, 1] = 1.0
    tr[:, 0] = 0.2 * np.sin(np.arange(FRAMES) / 90.0)
    lines = [f"# scripts/bench_video.py --chunk {a.chunk} --rounds {a.rounds} --quality {a.quality}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# bench_render.py's synthetic mesh (V = {V}, {FACES} faces; it covers four fifths of a panel), a take = {FRAMES} frames, {a.chunk} frames a call; us per "
             "frame, median over the rounds of the take's total; host paths on the first chunk only; no target, no speed-up claimed"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    for width in a.widths:
        host = None
        for takes in a.takes:
            inputs = [sm.case_inputs(100 + take, FRAMES, E, amp=0.08)[:2] for take in range(takes)]
            totals = {k: [] for k in ("transform", "count", "write", "files")}
            nbytes = 0
            for rnd in range(a.rounds + 1):                          # round 0 warms up
                t = dict.fromkeys(totals, 0.0)
                nbytes = 0
                for take in range(takes):
                    pose, ex = inputs[take]
                    for c in range(0, FRAMES, a.chunk):
                        s = slice(c, c + a.chunk)
                        verts = mesh.smplx_vertices(m, torch.from_numpy(pose[s]).to(dev), torch.from_numpy(ex[s]).to(dev), torch.from_numpy(tr[s]).to(dev))
                        rgb = render.render(scene, verts, 960, H)
                        if width == 1920:
                            rgb = torch.cat([rgb, rgb.flip(0)], dim=2)         # the second panel: the same chunk backwards
                        torch.cuda.synchronize()
                        us = staged(rgb, a.quality, ev)
                        for k, name in enumerate(("transform", "count", "write")):
                            t[name] += us[k]
                        nbytes += us[3]
                        t0 = time.perf_counter()
                        files = video.jpeg_frames(rgb, a.quality)
                        t["files"] += (time.perf_counter() - t0) * 1e6
                        assert sum(len(f) for f in files) == us[3]
                        if host is None and rnd == 1:
                            host = host_paths(rgb, a.quality)
                        del verts, rgb, files
                if rnd:
                    for k in totals:
                        totals[k].append(t[k] / (takes * FRAMES))
            med = {k: sorted(v)[len(v) // 2] for k, v in totals.items()}
            res = {"takes": takes, "frames": takes * FRAMES, "width": width, "height": H, "quality": a.quality, "chunk": a.chunk,
                   "us_per_frame": {k: round(v, 1) for k, v in med.items()},
                   "us_per_frame_range": {k: [round(min(v), 1), round(max(v), 1)] for k, v in totals.items()},
                   "bytes_per_frame": round(nbytes / (takes * FRAMES)), "raw_bytes_per_frame": 3 * width * H,
                   "host_us_per_frame": {k: round(v, 1) for k, v in (host or {}).items()}}
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
