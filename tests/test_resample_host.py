"""Audio resampling, host side: tests/resample_ref.py - the fp64 restatement the GPU tests compare with - pinned to scipy's polyphase
resampler fed the same taps and to analytic sines; the tap table of syntalker_amd.audio pinned to the restatement's, bit for bit; the kernel's table
layout; the argument checks (which raise before anything touches the device); the C ABI; and what stays refused."""
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_ref as rr
from tests.conftest import REPO

from syntalker_amd import _lib, audio

EPS = 2.0 ** -53


def lengths(M):
    """1, 7, M - 1, M, M + 1 and 3000 samples (M - 1 = 0 at M = 1 is no take: the shortest is 1)."""
    return sorted({1, 7, max(1, M - 1), M, M + 1, 3000})


@pytest.mark.parametrize("orig,target", rr.PAIRS)
def test_restatement_against_scipy_resample_poly(orig, target):
    """An independent polyphase implementation on the same taps (scipy multiplies a given filter by `up`; its output length is the same ceil).
    Bound: both sums have at most N terms, each implementation is at worst (N + 2) 2^-53 sum |terms| off, sum |terms| <= max |x| max_p sum |H_p|."""
    import scipy.signal
    L, M, K, g, h = rr.taps(orig, target)
    N, norm = rr.taps_per_output(L, K), rr.phase_norm(L, K, h)
    r = np.random.RandomState(L + M)
    for n in lengths(M):
        x = r.randn(n).astype(np.float32)
        got = rr.resample(x, orig, target)
        want = scipy.signal.resample_poly(x.astype(np.float64), L, M, window=h) / L
        bound = 2 * (N + 2) * EPS * np.abs(x).max() * norm
        err = np.abs(got - want).max()
        print(f"{orig} -> {target}, {n} samples: {len(got)} out, max |delta| {err:.3e} (bound {bound:.3e})")
        assert len(got) == len(want) == -(-n * L // M)
        assert err <= bound


@pytest.mark.parametrize("orig,target", rr.PAIRS + ((22050, 16001),))
def test_tap_table_is_the_restatements_bit_for_bit(orig, target):
    L, M, K, g, h = rr.taps(orig, target)
    L2, M2, K2, h2 = audio.resample_taps(orig, target)
    assert (L2, M2, K2) == (L, M, K) and h2.dtype == np.float64 and h2.shape == (2 * K + 1,) and np.array_equal(h2, h)
    assert audio.resample_taps(orig, target)[3] is h2 and not h2.flags.writeable          # cached
    assert audio.resample_length(3001, L, M) == rr.out_length(3001, L, M)


def test_table_sizes_are_the_documented_ones():
    assert [rr.taps(o, t)[:3] for o, t in rr.PAIRS] == [(320, 441, 29784), (160, 441, 29784), (1, 3, 202), (1, 2, 135), (2, 1, 135), (441, 320, 29784)]
    assert [rr.taps_per_output(*rr.taps(o, 16000)[0:3:2]) for o in (22050, 44100, 48000)] == [188, 374, 406]
    L, M, K, g, h = rr.taps(22050, 16001)
    assert L == 16001 and 2 * K + 1 < rr.MAX_TAPS and 2 * K + 1 > 2_900_000


@pytest.mark.parametrize("orig,target", rr.PAIRS)
def test_table_properties(orig, target):
    L, M, K, g, h = rr.taps(orig, target)
    assert np.array_equal(h, h[::-1]) and h[K] == g
    gains = rr.phase_gains(L, K, h)
    print(f"{orig} -> {target}: per-phase DC gain {gains.min() - 1:+.2e} .. {gains.max() - 1:+.2e}, max_p sum |H_p| = {rr.phase_norm(L, K, h):.3f}")
    assert gains.min() >= 1 - 1e-7 and gains.max() <= 1 + 1e-7


def interior(orig, target, n_out):
    """The outputs whose every term lies inside the take: a filter half-width (in output samples) from either end."""
    L, M, K, g, h = rr.taps(orig, target)
    edge = int(np.ceil((K // L + 2) * L / M)) + 1
    assert n_out > 4 * edge
    return slice(edge, n_out - edge)


@pytest.mark.parametrize("orig", (22050, 44100, 48000))
def test_tones(orig):
    """Pass band: a unit sine below the band edge comes out as the analytic sine at the new rate, within 2^-25 (the float32 rounding of the input)
    times sum |h| = 2.6, plus 2e-8 of window ripple: 2e-7.  Stop band: 9 and 10 kHz, above the new Nyquist rate, leave an rms of 1e-6 at the most."""
    n = orig // 2
    j = np.arange(n, dtype=np.float64)
    for f in (440.0, 1000.0, 7000.0):
        x = np.sin(2 * np.pi * f * j / orig).astype(np.float32)
        y = rr.resample(x, orig, 16000)
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / 16000.0)
        keep = interior(orig, 16000, len(y))
        err = np.abs(y - want)[keep].max()
        print(f"{orig} -> 16000, {f:g} Hz: max |y - sine| in the interior {err:.2e}")
        assert err <= 2e-7
    for f in (9000.0, 10000.0):
        x = np.sin(2 * np.pi * f * j / orig).astype(np.float32)
        y = rr.resample(x, orig, 16000)
        rms = float(np.sqrt(np.mean(y[interior(orig, 16000, len(y))] ** 2)))
        print(f"{orig} -> 16000, {f:g} Hz: rms in the interior {rms:.2e}")
        assert rms <= 1e-6


@pytest.mark.parametrize("orig,target", ((22050, 16000), (48000, 16000), (16000, 22050), (8000, 16000)))
def test_packed_table_is_the_kernels_layout(orig, target):
    """Column m mod L of the packed table against x[j0 - W + t], t ascending, is the restatement's sum term by term: equal bits (a zero tap adds 0.0)."""
    L, M, K, h = audio.resample_taps(orig, target)
    table = audio.pack_taps(L, M, K, h)
    W = K // L
    assert table.shape == (W + 1, L, 2) and table.dtype == np.float64 and table.flags.c_contiguous
    x = np.random.RandomState(3).randn(700).astype(np.float32).astype(np.float64)
    want = rr.resample(x, orig, target)
    xp = np.concatenate([np.zeros(W + 1), x, np.zeros(W + 2 + M)])
    got = np.zeros(len(want))
    m = np.arange(len(want), dtype=np.int64)
    j0, p = np.divmod(m * M, L)
    for t in range(2 * W + 2):
        got = got + xp[j0 + t + 1] * table[t // 2, m % L, t % 2]
    assert np.array_equal(got, want)


def test_argument_checks_raise_before_the_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(audio, "_Batch", lambda *a, **k: pytest.fail("a batch went to the device"))
    y = np.zeros(400, dtype=np.float32)
    for orig, target in ((0, 16000), (22050, 0), (-22050, 16000), (22050.5, 16000), (22050, 16000.25), ("22050", 16000), (None, 16000), (True, 16000)):
        with pytest.raises(ValueError, match="positive integer"):
            audio.resample(y, orig, target)
    with pytest.raises(ValueError, match="44100.*16001"):
        audio.resample(y, 44100, 16001)
    with pytest.raises(ValueError, match="44100.*16001"):
        audio.resample_taps(44100, 16001)
    for bad in (np.zeros((2, 400), np.float32), torch.zeros(1, 400), np.float32(1.0), [y, np.zeros((400, 1), np.float32)], [], np.zeros(0, np.float32)):
        with pytest.raises(ValueError):
            audio.resample(bad, 22050, 16000)
    with pytest.raises(ValueError, match="dtype"):
        audio.resample(y, 22050, 16000, dtype=torch.float16)
    assert audio.resample(y, 16000, 16000) is y and audio.resample(y, 22050.0, 22050) is y
    both = [y, torch.ones(3)]
    assert audio.resample(both, 48000, 48000) is both
    assert len(audio.resample_taps(22050, 16000)[3]) == 2 * 29784 + 1       # a float rate with an integer value is that integer
    assert audio.resample_taps(22050.0, 16000)[3] is audio.resample_taps(44100, 32000)[3]


def test_header_declares_the_export_once_and_the_abi_version_stays():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert re.search(r"^#define SYN_ABI_VERSION 9\b", header, flags=re.M) and _lib.ABI_VERSION == 9
    names = sorted(n for n in os.listdir(os.path.join(REPO, "syntalker_amd", "csrc")) if n.endswith((".inc", ".hip")))
    srcs = "".join(open(os.path.join(REPO, "syntalker_amd", "csrc", n)).read() for n in names)
    assert "syn_audio_resample.inc" in names and srcs.count('#include "syn_audio_resample.inc"') == 1
    assert len(re.findall(r"^int\s+syn_audio_resample\s*\(", header, flags=re.M)) == 1 and "syn_audio_resample" in _lib.EXPORTS
    assert len(re.findall(r"^int\s+syn_audio_resample\s*\([^;{]*\{", srcs, flags=re.M)) == 1                  # defined once
    lib = _lib.load()
    assert lib.syn_version() == 9 and hasattr(lib, "syn_audio_resample") and len(lib.syn_audio_resample.argtypes) == 12
    assert lib.syn_audio_resample(None, None, None, 1, 1, 1, 1, None, 2, None, None, None) != 0
    assert b"syn_audio_resample" in lib.syn_last_error()


def test_decode_wave_and_what_read_wave_still_refuses(tmp_path):
    from scipy.io import wavfile
    r = np.random.RandomState(0)
    y = (0.5 * r.randn(300)).clip(-1, 1).astype(np.float32)
    i16, i32, u8 = np.round(y * 32767).astype(np.int16), np.round(y.astype(np.float64) * (2 ** 31 - 1)).astype(np.int32), np.round(y * 127 + 128).astype(np.uint8)
    for name, rate, data in (("i16", 22050, i16), ("i32", 44100, i32), ("u8", 8000, u8), ("f32", 48000, y), ("st", 22050, np.stack([i16, -i16], 1))):
        wavfile.write(tmp_path / f"{name}.wav", rate, data)
    want = {"i16": i16.astype(np.float32) / 32768.0, "i32": (i32 / 2.0 ** 31).astype(np.float32), "u8": (u8.astype(np.float32) - 128.0) / 128.0,
            "f32": y, "st": i16.astype(np.float32) / 32768.0}
    for name, rate in (("i16", 22050), ("i32", 44100), ("u8", 8000), ("f32", 48000), ("st", 22050)):
        got_rate, got = audio.decode_wave(str(tmp_path / f"{name}.wav"))
        assert got_rate == rate and got.dtype == np.float32 and got.ndim == 1 and np.array_equal(got, want[name]), name
    with pytest.raises(ValueError, match="resampling is out of scope"):
        audio.read_wave(str(tmp_path / "i16.wav"))
    with pytest.raises(ValueError, match="resampling is out of scope"):
        audio.read_wave(str(tmp_path / "f32.wav"), 22050)
