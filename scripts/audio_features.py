#!/usr/bin/env python3
"""The reference's `onset_amplitude/<id>.npy` cache files from 16 kHz waveforms, on the device and without librosa.

    python scripts/audio_features.py WAV_DIR --out DIR [--sr 16000] [--batch 8] [--resample [--via 22050]]

The reference's dataloader (dataloaders/beat_sep_lower.py:387-409) reads `<data>/onset_amplitude/<id>.npy` before it calls librosa; a file written here
is what it would have written itself: (n, 2) float64, column 0 the rolling maximum of |y| over 1024 samples, column 1 a one-hot of the onset frames
(syntalker_amd.audio.onset_amplitude).  Point --out at that directory and the reference's dataloaders take these features unchanged.

WAV_DIR holds `<id>.wav` (scipy.io.wavfile: int16 -> / 32768, float samples as they are) or `<id>.npy` waveforms, which must already be at --sr:
a file at another rate is refused - resampling is out of scope (the reference loads at 22.05 kHz and resamples to 16 kHz; its `wave16k/` files are
16 kHz already) - unless --resample is given: then a `.wav` at any rate (int16, int32, uint8 or float PCM) is brought to --sr on the device first
(syntalker_amd.audio.load_waves; a group's files are resampled rate by rate and then batched as before), in one step or, with
--via 22050, in the reference's two (file rate -> 22050 -> --sr).  --batch takes share one launch sequence; a take's features do not depend on its
batch mates.
Prints one JSON line: {"files", "samples", "onsets"}.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import audio  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("wav_dir")
    ap.add_argument("--out", required=True)
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--resample", action="store_true")
    ap.add_argument("--via", type=int)
    a = ap.parse_args(argv)
    if a.via is not None and not a.resample:
        ap.error("--via names the intermediate rate of --resample")
    names = sorted(n for n in os.listdir(a.wav_dir) if n.endswith((".wav", ".npy")))
    if not names:
        raise SystemExit(f"audio_features: no .wav or .npy in {a.wav_dir}")
    os.makedirs(a.out, exist_ok=True)
    samples = onsets = 0
    for k in range(0, len(names), max(1, a.batch)):
        group = names[k:k + max(1, a.batch)]
        try:
            if a.resample:
                waves = audio.load_waves([os.path.join(a.wav_dir, n) for n in group], a.sr, a.via)
            else:
                waves = [audio.read_wave(os.path.join(a.wav_dir, n), a.sr) for n in group]
        except ValueError as e:
            raise SystemExit(f"audio_features: {e}")
        for name, feat in zip(group, audio.onset_amplitude(waves, sr=a.sr)):
            f = feat.double().cpu().numpy()
            np.save(os.path.join(a.out, os.path.splitext(name)[0] + ".npy"), f)
            samples += len(f)
            onsets += int(f[:, 1].sum())
    out = {"files": len(names), "samples": int(samples), "onsets": int(onsets)}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
