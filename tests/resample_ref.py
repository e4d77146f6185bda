"""Audio resampling restated in fp64 numpy, for test_resample_host.py, test_gpu_resample.py and scripts/bench_resample.py.

Written from the definition, with no librosa, resampy or soxr code: band-limited interpolation with a Kaiser-windowed sinc, evaluated exactly on the
rational grid.  For orig_sr -> target_sr, d = gcd, L = target_sr / d, M = orig_sr / d, g = rolloff min(1, L / M), K = floor(Z L / g):

    h[k] = g sinc(g k / L) I0(beta sqrt(1 - u^2)) / I0(beta),  u = g k / (L Z),  |k| <= K;   h[k] = 0 otherwise
    y[m] = sum_j x[j] h[m M - j L],  m = 0 .. ceil(n L / M) - 1,  x zero outside 0 .. n - 1

The table is built here on its own (the non-negative half, mirrored), not taken from syntalker_amd.audio.resample_taps: test_resample_host.py asks
the two to be equal bit for bit, and scipy.signal.resample_poly - an independent polyphase implementation - to agree with `resample` on these taps.
The sum runs over ASCENDING j, the kernel's documented order (one chain from 0.0; numpy multiplies and adds where the kernel uses fma, which is
within the bound the tests compute and exact where a sum has one term).
"""
import math

import numpy as np

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
MAX_TAPS = 1 << 22

PAIRS = ((22050, 16000), (44100, 16000), (48000, 16000), (32000, 16000), (8000, 16000), (16000, 22050))

_cache = {}


def ratio(orig_sr, target_sr):
    d = math.gcd(int(orig_sr), int(target_sr))
    return int(target_sr) // d, int(orig_sr) // d


def taps(orig_sr, target_sr):
    """(L, M, K, g, h): h float64 of 2 K + 1 taps, h[K + k] for k = -K .. K."""
    L, M = ratio(orig_sr, target_sr)
    if (L, M) not in _cache:
        g = ROLLOFF * min(1, L / M)
        K = int(np.floor(Z * L / g))
        if 2 * K + 1 > MAX_TAPS:
            raise ValueError(f"{orig_sr} -> {target_sr}: {2 * K + 1} taps")
        k = np.arange(0, K + 1, dtype=np.float64)
        u = g * k / (L * Z)
        half = g * np.sinc(g * k / L) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(BETA)
        _cache[(L, M)] = (L, M, K, g, np.concatenate([half[:0:-1], half]))
    return _cache[(L, M)]


def out_length(n, L, M):
    return (n * L + M - 1) // M


def taps_per_output(L, K):
    """N of the error bounds: the most terms a sum can have, 2 (K // L) + 2."""
    return 2 * (K // L) + 2


def phase_norm(L, K, h):
    """max over the phases p of sum_i |h[p + i L]|: the largest sum |taps| any output sees."""
    a = np.abs(h)
    return max(float(a[(K + p) % L::L].sum()) for p in range(L))


def phase_gains(L, K, h):
    """sum_i h[p + i L] per phase p: the gain of a constant input, 1 in exact band-limited interpolation."""
    return np.array([h[(K + p) % L::L].sum() for p in range(L)])


def resample(x, orig_sr, target_sr, outputs=None):
    """float64 y[m] for every m (or for the int64 indices `outputs` only): the sum over j ascending, vectorised over the outputs."""
    L, M, K, g, h = taps(orig_sr, target_sr)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    m = np.arange(out_length(n, L, M), dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64)
    assert n >= 1 and (len(m) == 0 or (0 <= m.min() and m.max() < out_length(n, L, M)))
    W = K // L
    j0, p = np.divmod(m * M, L)
    acc = np.zeros(len(m))
    for t in range(2 * W + 2):                                  # j = j0 - W + t: ascending for every output at once
        j = j0 - W + t
        k = m * M - j * L
        ok = (j >= 0) & (j < n) & (np.abs(k) <= K)
        acc = acc + np.where(ok, x[np.where(ok, j, 0)] * h[np.where(ok, k + K, 0)], 0.0)
    return acc
