#!/usr/bin/env python3
"""L1 diversity and beat consistency of a results directory as the reference's `test()` writes it (diffusion_rvqvae_trainer.py:702-709:
`res_<id>.npz` with `poses` (n, 165) SMPL-X axis-angle, `trans`, `betas`), the way `test()` computes them (:626-638, 668, 677-684, 722-728).

    python scripts/motion_metrics_from_results.py RESULTS_DIR --smplx-model SMPLX_NEUTRAL_2020.npz --mean-vel mean_vel_smplxflame_30.npy [--onsets DIR | --waves DIR [--resample]] [--face]

Per take: rest joints and the hands' mean pose from the model file and the take's betas (joints.smplx_rest_joints, host), the 55 skeleton joints by
forward kinematics on the device with zero transl as `test()` passes it (joints.smplx_joints; the hand mean pose is added to the hand joints'
axis-angle vectors, as smplx does for the reference's model, built without flat_hand_mean), L1div.run on them, and - with --onsets - the beat
consistency of the slice [mask, n - mask) against the take's audio onsets (with --waves: found on the device from the take's 16 kHz waveform).
--mean-vel   the reference's `avg_vel` (55,): data_path + weights/mean_vel_<pose_rep>.npy
--onsets     a directory with `<id>.npy`: onset times in seconds (what alignment.load_audio returns for the take's audio cut to the slice,
             librosa.onset.onset_detect); a take without its file, or with no onsets, is left out of `bc` (named on stderr)
--waves      a directory with `<id>.wav` (or `<id>.npy`): the take's waveform at --audio-sr (16000: the reference's wave16k/), from which the onsets are
             detected as test() does (:681-683; metrics.beat_consistency_from_audio, syntalker_amd.audio - no librosa).  A file at another rate is
             refused: resampling is out of scope - unless --resample is given.  --onsets and --waves together are an error; with neither there is no `bc`
--resample   with --waves: a `.wav` at any rate is brought to --audio-sr on the device first (syntalker_amd.audio.load_wave)
--flat-hand-mean   for results made with a model built with flat_hand_mean=True: no hand mean pose is added
--face       also test()'s `l2 loss` and `lvel loss` (:640-675, :713-714): the face meshes of `res_<id>.npz` against `gt_<id>.npz` (jaw pose and
             `expressions` of each, everything else zero; metrics.face_losses), accumulated as test() does: sum(value x n) / frames
--mask       frames dropped at either end (align_mask, default 60); takes of 2 mask frames or fewer are left out of `bc`
Prints one JSON line: {"takes", "frames", "l1div"[, "bc", "bc_takes", "bc_frames"][, "l2", "lvel"]}; bc = sum(align x (n - 2 mask)) / bc_frames over the bc_takes takes
that have onsets, bc_frames = their frames - 2 bc_takes mask: the reference's weighting (:684, :722) when bc_takes == takes, and a partial figure,
recognisable by bc_takes < takes, otherwise.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import audio, joints, mesh, metrics  # noqa: E402


def read_ids(results_dir: str):
    return sorted(n[len("res_"):-len(".npz")] for n in os.listdir(results_dir) if n.startswith("res_") and n.endswith(".npz"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("results_dir")
    ap.add_argument("--smplx-model", required=True)
    ap.add_argument("--mean-vel", required=True)
    ap.add_argument("--onsets")
    ap.add_argument("--waves")
    ap.add_argument("--audio-sr", type=int, default=16000)
    ap.add_argument("--resample", action="store_true")
    ap.add_argument("--flat-hand-mean", action="store_true")
    ap.add_argument("--face", action="store_true")
    ap.add_argument("--mask", type=int, default=60)
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--order", type=int, default=7)
    a = ap.parse_args(argv)
    if a.onsets is not None and a.waves is not None:
        ap.error("--onsets and --waves exclude each other: the onsets are read, or detected from the waveforms")
    if a.resample and a.waves is None:
        ap.error("--resample applies to the files of --waves")
    ids = read_ids(a.results_dir)
    if not ids:
        raise SystemExit(f"motion_metrics_from_results: no res_<id>.npz in {a.results_dir}")
    model = dict(np.load(a.smplx_model, allow_pickle=True))
    mmae = np.load(a.mean_vel)
    dev = torch.device("cuda")
    l1, align, bc_frames, bc_takes, frames = metrics.L1div(), 0.0, 0, 0, 0
    l2_all, lvel_all = 0.0, 0.0
    for i in ids:
        res = np.load(os.path.join(a.results_dir, f"res_{i}.npz"), allow_pickle=True)
        pose = torch.from_numpy(np.asarray(res["poses"], dtype=np.float32)).to(dev)
        n = pose.shape[0]
        skel = joints.smplx_rest_joints(model, np.asarray(res["betas"], dtype=np.float64).reshape(-1), flat_hand_mean=a.flat_hand_mean)
        joints_rec = joints.smplx_joints(skel, pose.reshape(n, -1))
        l1.run(joints_rec)
        frames += n
        if a.face:
            gt = np.load(os.path.join(a.results_dir, f"gt_{i}.npz"), allow_pickle=True)
            face = mesh.smplx_mesh(model, np.asarray(res["betas"], dtype=np.float64).reshape(-1), flat_hand_mean=a.flat_hand_mean)
            to_dev = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dev)
            l2, lvel = metrics.face_losses(face, pose.reshape(n, -1), to_dev(gt["poses"]).reshape(n, -1), to_dev(res["expressions"]).reshape(n, -1),
                                           to_dev(gt["expressions"]).reshape(n, -1))
            l2_all += l2 * n
            lvel_all += lvel * n
        if a.onsets is None and a.waves is None:
            continue
        if a.waves is not None:
            path = next((p for p in (os.path.join(a.waves, f"{i}.wav"), os.path.join(a.waves, f"{i}.npy")) if os.path.exists(p)), None)
            onsets = np.zeros(0)
            if path is not None and n > 2 * a.mask:
                wave = audio.load_wave(path, a.audio_sr) if a.resample else audio.read_wave(path, a.audio_sr)
                short = metrics.audio_slice_of_test(wave, n, a.mask, a.audio_sr, 30.0)
                onsets = audio.onset_detect(short, sr=a.audio_sr, hop_length=512, units="time") if len(short) else onsets
        else:
            path = os.path.join(a.onsets, f"{i}.npy")
            onsets = np.load(path).reshape(-1) if os.path.exists(path) else np.zeros(0)
        if onsets.size == 0 or n <= 2 * a.mask:
            print(f"motion_metrics_from_results: {i} has no onsets (or is not longer than twice the mask), left out of bc", file=sys.stderr)
            continue
        align += metrics.beat_consistency(joints_rec, onsets, mmae, align_mask=a.mask, sigma=a.sigma, order=a.order) * (n - 2 * a.mask)
        bc_frames += n - 2 * a.mask
        bc_takes += 1
    out = {"takes": len(ids), "frames": int(frames), "l1div": l1.avg()}
    if a.onsets is not None or a.waves is not None:
        out.update({"bc": align / bc_frames if bc_frames else None, "bc_takes": bc_takes, "bc_frames": int(bc_frames)})
    if a.face:
        out.update({"l2": l2_all / frames, "lvel": lvel_all / frames})
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
