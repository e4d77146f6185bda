#!/usr/bin/env python3
"""The takes of a results directory as the reference's `test()` writes it (`res_<id>.npz`, with --gt also `gt_<id>.npz`: `poses` (n, 165) axis-angle,
`expressions` (n, 100), `trans` (n, 3), `betas`), drawn on the device: what `render_one_sequence` / `render_one_sequence_no_gt` do with `smplx` and
`pyrender` up to the frames they hand to ffmpeg - the mesh by syntalker_amd.mesh, the picture by syntalker_amd.render (neither library is needed).

    python scripts/render_from_results.py RESULTS_DIR --smplx-model SMPLX_NEUTRAL_2020.npz [--out DIR] [--gt] [--fps 30] [--width 1920 --height 720]
                                          [--chunk 64] [--format bmp|png|avi] [--quality 90] [--waves WAVE_DIR]

Writes `frames_<id>/frame_<k>.<ext>` into --out (default: RESULTS_DIR), k counting the drawn frames (every max(1, int(30 // fps))-th frame of the take,
as the reference samples them).  A panel is width // 2 pixels wide, as in the reference; with --gt the result's panel stands left of the ground
truth's, without it the frame is the one panel.  Frames are made --chunk at a time: a minute of vertices is 226 MB and a minute of pictures 3.7 GB, so
neither is held whole.  `png` needs PIL; `bmp` (the reference's `render_tmp_img_filetype`) needs nothing.  The tone is this project's Lambert term,
not pyrender's shader (syntalker_amd/render.py).  H.264 / mp4 encoding stays out: with `bmp` / `png` the ffmpeg line that makes the silent mp4 of each
take is printed.  Prints one JSON line: {"takes", "frames", "width", "height", "out"}.
--format avi       one playable file per take instead of frames: `video_<id>.avi`, Motion-JPEG encoded on the device (syntalker_amd/video.py, JPEG --quality
                   Q), and with --waves WAVE_DIR the take's `<id>.wav` (any rate, int16 or float, first channel) as its PCM sound track at its own rate,
                   cut at the video's end.  The video runs at 30 / max(1, int(30 // fps)) frames a second, the rate the drawn frames have in the take.
                   No frame files and no ffmpeg line; the JSON line gains "videos".  The track is not resampled.
--flat-hand-mean   for results made with a model built with flat_hand_mean=True
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import mesh, render, video  # noqa: E402


def image_writer(fmt):
    if fmt == "bmp":
        return render.write_bmp
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit("render_from_results: --format png needs PIL, which is not installed here; use --format bmp")
    return lambda path, img: Image.fromarray(img).save(path)


def sound_track(wave_dir, take_id):
    """(samples, rate) of WAVE_DIR/<id>.wav: int16 or float, the first channel of several."""
    path = os.path.join(wave_dir, f"{take_id}.wav")
    if not os.path.isfile(path):
        raise SystemExit(f"render_from_results: --waves: {path} is missing")
    from scipy.io import wavfile
    rate, y = wavfile.read(path)
    if y.dtype != np.int16 and y.dtype.kind != "f":
        raise SystemExit(f"render_from_results: {path}: int16 or float samples, got {y.dtype}")
    return np.ascontiguousarray(y[:, 0] if y.ndim == 2 else y), int(rate)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("results_dir")
    ap.add_argument("--smplx-model", required=True)
    ap.add_argument("--out")
    ap.add_argument("--gt", action="store_true")
    ap.add_argument("--fps", type=float, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--format", default="bmp", choices=("bmp", "png", "avi"))
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--waves")
    ap.add_argument("--flat-hand-mean", action="store_true")
    a = ap.parse_args(argv)
    if a.chunk < 1 or a.fps <= 0 or a.width < 2:
        raise SystemExit("render_from_results: --chunk >= 1, --fps > 0, --width >= 2")
    as_video = a.format == "avi"
    if not as_video and (a.waves or a.quality != 90):
        raise SystemExit("render_from_results: --quality and --waves belong to --format avi")
    if not 1 <= a.quality <= 100:
        raise SystemExit("render_from_results: --quality is 1 to 100")
    write = None if as_video else image_writer(a.format)
    ids = sorted(n[len("res_"):-len(".npz")] for n in os.listdir(a.results_dir) if n.startswith("res_") and n.endswith(".npz"))
    if not ids:
        raise SystemExit(f"render_from_results: no res_<id>.npz in {a.results_dir}")
    out_dir = a.out or a.results_dir
    model = dict(np.load(a.smplx_model, allow_pickle=True))
    dev = torch.device("cuda")
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    scene, frames, panel, videos = None, 0, a.width // 2, []

    def take(prefix, i):
        res = np.load(os.path.join(a.results_dir, f"{prefix}_{i}.npz"), allow_pickle=True)
        n = res["poses"].shape[0]
        ex = np.asarray(res["expressions"], dtype=np.float32).reshape(n, -1)
        m = mesh.smplx_mesh(model, np.asarray(res["betas"], dtype=np.float64).reshape(-1), num_expression_coeffs=ex.shape[1], flat_hand_mean=a.flat_hand_mean)
        return m, np.asarray(res["poses"], dtype=np.float32).reshape(n, -1), ex, np.asarray(res["trans"], dtype=np.float32).reshape(n, 3)

    for i in ids:
        m, pose, ex, tr = take("res", i)
        if m.faces is None:
            raise SystemExit("render_from_results: the model file has no faces (`f`)")
        if scene is None:
            scene = render.Scene(np.asarray(m.faces).astype(np.int64), n_vertices=m.n_vertices)
        picked = render.frame_indices(pose.shape[0], a.fps)
        if a.gt:
            gm, gpose, gex, gtr = take("gt", i)
            picked = [k for k in picked if k < gpose.shape[0]]
        writer = None
        if as_video:
            os.makedirs(out_dir, exist_ok=True)
            wave, rate = sound_track(a.waves, i) if a.waves else (None, 16000)
            videos.append(os.path.join(out_dir, f"video_{i}.avi"))
            writer = video.AviWriter(videos[-1], 2 * panel if a.gt else panel, a.height, 30 / max(1, int(30 // a.fps)), wave=wave, wave_sr=rate, quality=a.quality)
        else:
            take_dir = os.path.join(out_dir, f"frames_{i}")
            os.makedirs(take_dir, exist_ok=True)
        for c in range(0, len(picked), a.chunk):
            sel = np.asarray(picked[c:c + a.chunk])
            verts = mesh.smplx_vertices(m, to_dev(pose[sel]), to_dev(ex[sel]), to_dev(tr[sel]))
            if a.gt:
                img = render.render_pair(scene, verts, mesh.smplx_vertices(gm, to_dev(gpose[sel]), to_dev(gex[sel]), to_dev(gtr[sel])), a.width, a.height)
            else:
                img = render.render(scene, verts, panel, a.height)
            if as_video:
                writer.write(img)                # encoded where they were drawn: the frames cross to the host as JPEG
                continue
            img = img.cpu().numpy()
            for k in range(len(sel)):
                write(os.path.join(take_dir, f"frame_{c + k}.{a.format}"), img[k])
        frames += len(picked)
        if as_video:
            writer.close()
            continue
        print(f"# ffmpeg -y -framerate {a.fps:g} -i {os.path.join(take_dir, f'frame_%d.{a.format}')} -c:v libx264 -pix_fmt yuv420p "
              f"{os.path.join(out_dir, f'silence_video_{i}.mp4')}", flush=True)
    out = {"takes": len(ids), "frames": int(frames), "width": 2 * panel if a.gt else panel, "height": a.height, "out": out_dir}
    if as_video:
        out["videos"] = videos
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
