#!/usr/bin/env python3
"""Timing of the audio front end (csrc/syn_audio.inc): 1 and 8 takes of 60 s at 16 kHz.

    python scripts/bench_audio.py [--seconds 60] [--repeat 5] [--out profiles/audio_bench.txt]

Per batch size: microseconds per take of the whole `onset_amplitude` call and of each stage (amplitude envelope; power spectrum = the fp64 MFMA GEMM;
mel + dB = syn_audio_mel_db minus the spectrum; envelope; peak picking), stream-synchronised medians over --repeat runs after a warm-up.  The GEMM's
rate counts 2 * 2048 * 2050 floating-point operations per frame (the [cos | -sin] product; the 15 padding columns of the last tile are not counted).
Against it: the fp64 numpy restatement (tests/audio_features_ref.py, an FFT) on the host, per take, and - where torch.stft runs - a float32 torch
pipeline on the same device.  The device's envelope error against the restatement is printed beside the float32 pipelines'.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import _lib, audio  # noqa: E402
from tests import audio_features_ref as ar  # noqa: E402


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def torch_f32_envelope(y, sr, fb):
    """The pipeline in float32 torch ops on the device: what an eager port would compute."""
    spec = torch.stft(y, 2048, hop_length=512, window=torch.hann_window(2048, device=y.device), center=True, pad_mode="constant", return_complex=True)
    mel = fb @ (spec.real ** 2 + spec.imag ** 2)
    s = 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
    s = torch.maximum(s, s.max() - 80.0)
    flux = torch.clamp(s[:, 1:] - s[:, :-1], min=0).mean(0)
    return torch.cat([torch.zeros(3, device=y.device), flux])[: s.shape[1]]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "audio_bench.txt"))
    a = ap.parse_args(argv)
    sr, hop, n = 16000, 512, int(a.seconds * 16000)
    lines = [f"audio front end, {a.seconds:g} s takes at {sr} Hz ({n} samples, {1 + n // hop} frames), {torch.cuda.get_device_name(0)}, median of {a.repeat}"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    waves = [ar.speech_like(20 + k, n) for k in range(8)]
    lib = _lib.load()
    for batch in (1, 8):
        b = audio._Batch(waves[:batch], hop)
        total, stream = int(b.foff_host[-1]), _lib.current_stream(b.dev)
        p = torch.empty(total, 1025, dtype=torch.float64, device=b.dev)
        env, x = audio._envelopes(b, sr, hop)
        s = audio._mel_db(b, sr, hop)
        t_all = timed(lambda: audio.onset_amplitude(waves[:batch]), a.repeat)
        t_amp = timed(lambda: audio._amplitude(b, 1024), a.repeat)
        t_pow = timed(lambda: _lib.check(lib.syn_audio_power_spectrum(b.y.data_ptr(), b.soff.data_ptr(), b.foff.data_ptr(), batch, max(b.frames), total, hop,
                                                                      p.data_ptr(), stream), "syn_audio_power_spectrum"), a.repeat)
        t_mel = timed(lambda: audio._mel_db(b, sr, hop), a.repeat)
        t_env = timed(lambda: _lib.check(lib.syn_audio_onset_env(s.data_ptr(), b.foff.data_ptr(), batch, max(b.frames), hop, env.data_ptr(), x.data_ptr(), stream), "env"), a.repeat)
        t_pick = timed(lambda: audio._peak_pick(x, env, b.foff, batch, (0, 1, 3, 4, 0), 0.07), a.repeat)
        flops = 2.0 * 2048 * 2050 * total
        say(f"{batch} take(s): onset_amplitude {t_all / batch:9.1f} us/take | amplitude {t_amp / batch:8.1f} | power spectrum {t_pow / batch:8.1f} "
            f"({flops / t_pow * 1e-6:.2f} TFLOP/s fp64 MFMA) | mel + dB {(t_mel - t_pow) / batch:8.1f} | envelope {t_env / batch:7.1f} | peak pick {t_pick / batch:7.1f}")
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    t0 = time.perf_counter()
    want = ar.onset_strength(waves[0], sr, hop)
    ar.amplitude_envelope(waves[0])
    ar.peak_pick(ar.normalise(want), 0, 1, 3, 4, 0)
    say(f"host, fp64 numpy restatement (FFT): {(time.perf_counter() - t0) * 1e6:9.1f} us/take")
    got = audio.onset_strength(waves[0]).cpu().numpy()
    say(f"envelope error / max: device {np.abs(got - want).max() / want.max():.3e}, numpy float32 {np.abs(ar.onset_strength(waves[0], sr, hop, np.float32) - want).max() / want.max():.3e}")
    try:
        y = torch.from_numpy(waves[0]).cuda()
        fb = torch.from_numpy(ar.mel_filterbank(sr).astype(np.float32)).cuda()
        e32 = torch_f32_envelope(y, sr, fb).cpu().numpy()
        t = timed(lambda: torch_f32_envelope(y, sr, fb), a.repeat)
        say(f"torch float32 pipeline (torch.stft) on the device: {t:9.1f} us/take, envelope error / max {np.abs(e32 - want).max() / want.max():.3e}")
    except Exception as e:                                    # torch.stft needs an FFT library the box may not have
        say(f"torch float32 pipeline: torch.stft does not run here ({type(e).__name__}: {str(e).splitlines()[0][:120]})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
