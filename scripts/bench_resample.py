#!/usr/bin/env python3
"""Timing of the audio resampler (csrc/syn_audio_resample.inc): 1 and 8 takes of 60 s from 22050, 44100 and 48000 Hz to 16000 Hz.

    python scripts/bench_resample.py [--seconds 60] [--repeat 7] [--out profiles/resample_bench.txt]

Per source rate and batch size: microseconds per take of the kernel alone (`syn_audio_resample` on a batch that is already on the device, fp32 out; 20
launches back to back per timed window) and of the whole `audio.resample` call on device tensors (offsets, allocation, the launch), device-event
medians over --repeat windows after a warm-up; the kernel's rate in fp64 fma per second (outputs x T, the taps a thread walks) and the bytes of taps
its threads ask for.  The three rates differ in the table access: at 48000 Hz L = 1 and every thread of a wave reads the same taps (one address),
at 22050 and 44100 Hz a wave reads 1 KB of consecutive table a step (profiles/resample_layout_ab.txt: what other layouts cost).  Beside it:
scipy.signal.resample_poly on the host with the same taps, per take, and the device's fp64 sums against the numpy
restatement (tests/resample_ref.py) on every 61st output of one take - all phases, both ends.
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
from tests import resample_ref as rr  # noqa: E402


def timed(fn, repeat, inner=1):
    """Median over `repeat` windows of `inner` back-to-back calls each, microseconds per call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return float(np.median(out))


def main(argv=None):
    import scipy.signal
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_bench.txt"))
    a = ap.parse_args(argv)
    target = 16000
    lines = [f"audio resampling to {target} Hz, {a.seconds:g} s takes, {torch.cuda.get_device_name(0)}, median of {a.repeat}"]
    say = lambda s: (print(s, flush=True), lines.append(s))
    lib = _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    for orig in (22050, 44100, 48000):
        n = int(a.seconds * orig)
        L, M, K, h = audio.resample_taps(orig, target)
        T, n_out = 2 * (K // L) + 2, audio.resample_length(n, L, M)
        waves = [ar.speech_like(60 + k, n, sr=orig) for k in range(8)]
        on_dev = [torch.from_numpy(w).cuda() for w in waves]
        for batch in (1, 8):
            b = audio._Batch(on_dev[:batch])
            taps = audio._device_taps(L, M, K, h, b.dev)
            ooff = torch.from_numpy(np.arange(batch + 1, dtype=np.int64) * n_out).to(b.dev)
            out = torch.empty(batch * n_out, dtype=torch.float32, device=b.dev)
            stream = _lib.current_stream(b.dev)
            t_k = timed(lambda: _lib.check(lib.syn_audio_resample(b.y.data_ptr(), b.soff.data_ptr(), ooff.data_ptr(), batch, n, L, M, taps.data_ptr(), taps.numel(),
                                                                  out.data_ptr(), None, stream), "syn_audio_resample"), a.repeat, inner=20)
            t_all = timed(lambda: audio.resample(on_dev[:batch], orig, target), a.repeat)
            fma = float(batch) * n_out * T
            say(f"{orig} Hz (L = {L}, M = {M}, K = {K}, {T} taps an output, table {L * T * 8 / 1e6:.2f} MB), {batch} take(s): kernel {t_k / batch:8.1f} us/take "
                f"({fma / t_k * 1e-6:.2f} T fma/s fp64, {fma * 8 / t_k * 1e-6:.2f} TB/s of taps asked for) | audio.resample {t_all / batch:8.1f} us/take")
        x = waves[0].astype(np.float64)
        t0 = time.perf_counter()
        scipy.signal.resample_poly(x, L, M, window=h)
        t_host = (time.perf_counter() - t0) * 1e6
        which = np.arange(0, n_out, 61, dtype=np.int64)
        which = np.unique(np.concatenate([which, np.arange(min(300, n_out)), np.arange(max(0, n_out - 300), n_out)]))
        want = rr.resample(waves[0], orig, target, outputs=which)
        got = audio.resample(on_dev[0], orig, target, dtype=torch.float64).cpu().numpy()[which]
        say(f"{orig} Hz: host scipy.signal.resample_poly, same taps: {t_host:10.1f} us/take | device fp64 against the restatement on {len(which)} outputs: "
            f"max |delta| {np.abs(got - want).max():.3e} (max |y| {np.abs(want).max():.3f})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
