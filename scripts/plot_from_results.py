#!/usr/bin/env python3
"""The h3d takes of a results directory as stick-figure videos: what the reference's trainer does with `plot_3d_motion` on the output of
`recover_from_ric(., 52)` (`h3d_diffusion_new_trainer.py:870-891`), drawn on the device by syntalker_amd.plot and written as Motion-JPEG AVI by
syntalker_amd.video - neither matplotlib nor ffmpeg is needed.

    python scripts/plot_from_results.py RESULTS_DIR [--out DIR] [--size 1000] [--fps 30] [--smplx-chains] [--waves WAVE_DIR] [--quality 90] [--chunk 64]

Reads every `rec_*.npy` as the trainer saves it: (n, 52, 3) joints (or (n, J, 3) with J >= 22), or (n, 623) HumanML3D features, which go through
`joints.recover_from_ric(., 52)`.  Writes `rec_*.avi` into --out (default: RESULTS_DIR), every frame of the take at --fps.  The 5 body chains are
drawn; --smplx-chains adds the 10 finger chains (52 joints).  --waves WAVE_DIR: `<name>.wav` beside `<name>.npy` (any rate) becomes the PCM sound
track, brought to 16 kHz by `audio.load_wave`.  Frames are drawn and encoded --chunk at a time.  There is no title (no text rendering) and no
H.264 / mp4.  Prints one JSON line: {"takes", "frames", "size", "out", "videos"}."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import audio, joints, plot, video  # noqa: E402


def take_joints(path, dev):
    """(n, J, 3) float32 on the device."""
    x = np.load(path)
    if x.ndim == 3 and x.shape[2] == 3:
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    if x.ndim == 2 and x.shape[1] == 623:
        return joints.recover_from_ric(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev), 52)
    raise SystemExit(f"plot_from_results: {path}: (n, J, 3) joints or (n, 623) features, got {x.shape}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("results_dir")
    ap.add_argument("--out")
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--fps", type=float, default=30)
    ap.add_argument("--smplx-chains", action="store_true")
    ap.add_argument("--waves")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--chunk", type=int, default=64)
    a = ap.parse_args(argv)
    if a.chunk < 1 or a.fps <= 0 or not 1 <= a.quality <= 100 or not 1 <= a.size <= plot.MAX_DIM:
        raise SystemExit(f"plot_from_results: --chunk >= 1, --fps > 0, --quality 1 to 100, --size 1 to {plot.MAX_DIM}")
    names = sorted(n[:-len(".npy")] for n in os.listdir(a.results_dir) if n.startswith("rec_") and n.endswith(".npy"))
    if not names:
        raise SystemExit(f"plot_from_results: no rec_*.npy in {a.results_dir}")
    out_dir = a.out or a.results_dir
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda")
    p = plot.Plot(plot.SMPLX_CHAINS if a.smplx_chains else plot.SMPL_CHAINS, size=a.size)
    frames, videos = 0, []
    for name in names:
        j = take_joints(os.path.join(a.results_dir, f"{name}.npy"), dev)
        if j.shape[1] < p.n_joints:
            raise SystemExit(f"plot_from_results: {name}.npy has {j.shape[1]} joints, the chains need {p.n_joints}")
        wave = None
        if a.waves:
            path = os.path.join(a.waves, f"{name}.wav")
            if not os.path.isfile(path):
                raise SystemExit(f"plot_from_results: --waves: {path} is missing")
            wave = audio.load_wave(path, 16000)
        data, trajec, mins, maxs = plot.prepare(j)
        n = int(j.shape[0])
        chunks = (plot.draw_prepared(p, data, trajec, mins, maxs, range(k, min(n, k + a.chunk))) for k in range(0, n, a.chunk))
        videos.append(os.path.join(out_dir, f"{name}.avi"))
        frames += video.write_video(videos[-1], chunks, a.fps, wave=wave, wave_sr=16000, quality=a.quality)["frames"]
    out = {"takes": len(names), "frames": int(frames), "size": a.size, "out": out_dir, "videos": videos}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
