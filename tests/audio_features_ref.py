"""The audio front end restated in fp64 numpy, for test_audio_host.py, test_gpu_audio.py and scripts/bench_audio.py.

Written from the algorithm's text, not from librosa's code.  The transform is an FFT (`scipy.fft.rfft`), so nothing here shares its summation
structure with the device's GEMM.  `dtype=np.float32` runs the spectrum and everything behind it in float32, as librosa does; that variant is only
ever used to REPORT what float32 arithmetic costs, never as a reference.

Also here: the deterministic speech-like generator the tests use, the restated dataloader lines (`onset_amplitude_ref`) and the margin report that
says which frames of a take are too close to a decision boundary to be compared.
"""
import numpy as np
import scipy.fft

N_FFT, N_MELS = 2048, 128
TINY = 1.1754943508222875e-38

# (seed, samples): 17 frames - one more than a 16-row tile; 32 frames; 126 frames; 313 frames - several row tiles; the shortest legal take
CASES = ((3, 8320), (0, 16000), (1, 64000), (2, 160000), (4, 1024))
SILENCE = 64000                                       # 4.0 s of zeros
RATES = ((16000, 512), (22050, 512))


def speech_like(seed: int, n: int, sr: int = 16000) -> np.ndarray:
    """Gated harmonic bursts at 4 per second: f0 90-250 Hz, 11 harmonics, 10 ms attack / 30 ms release, plus 1e-3 white noise, peak 0.8, float32."""
    r = np.random.RandomState(1000 + seed)
    t = np.arange(n) / sr
    y = np.zeros(n)
    for k in range(int(np.ceil(n / sr * 4))):
        start = k / 4.0 + r.uniform(0.0, 0.08)
        dur = r.uniform(0.06, 0.15)
        f0 = r.uniform(90.0, 250.0)
        amps = r.uniform(0.3, 1.0, 11) / np.arange(1, 12)
        phase = r.uniform(0, 2 * np.pi, 11)
        lo, hi = max(0, int(start * sr) - 1), min(n, int((start + dur + 0.030) * sr) + 2)      # the gate is zero outside
        tt = t[lo:hi]
        gate = np.clip((tt - start) / 0.010, 0.0, 1.0) * np.clip((start + dur + 0.030 - tt) / 0.030, 0.0, 1.0)
        y[lo:hi] += gate * sum(a * np.sin(2 * np.pi * f0 * h * tt + p) for h, (a, p) in enumerate(zip(amps, phase), start=1))
    y += 1e-3 * r.randn(n)
    return (0.8 * y / np.abs(y).max()).astype(np.float32)


def gpu_takes():
    return [speech_like(seed, n) for seed, n in CASES]


# ---- steps 1-2 ------------------------------------------------------------------------------------------------------------------------------
def hann(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


def frames_of(y, hop=512, dtype=np.float64):
    y = np.asarray(y, dtype=dtype)
    T = 1 + len(y) // hop
    ypad = np.concatenate([np.zeros(N_FFT // 2, dtype), y, np.zeros(N_FFT // 2, dtype)])
    return np.stack([ypad[t * hop: t * hop + N_FFT] for t in range(T)])


def power_spectrum(y, hop=512, dtype=np.float64):
    spec = scipy.fft.rfft(frames_of(y, hop, dtype) * hann(dtype), axis=1)
    assert spec.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    return (spec.real ** 2 + spec.imag ** 2).astype(dtype)


# ---- step 3 ---------------------------------------------------------------------------------------------------------------------------------
def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_edges(sr):
    return mel_to_hz(np.linspace(0.0, float(hz_to_mel(sr / 2.0)), N_MELS + 2))


def mel_filterbank(sr):
    f = mel_edges(sr)
    fft_f = np.arange(N_FFT // 2 + 1) * (sr / N_FFT)
    lower = (fft_f[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    upper = (f[2:, None] - fft_f[None, :]) / (f[2:] - f[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]


# ---- steps 4-6 ------------------------------------------------------------------------------------------------------------------------------
def mel_db(y, sr=16000, hop=512, dtype=np.float64):
    M = power_spectrum(y, hop, dtype) @ mel_filterbank(sr).astype(dtype).T
    S = 10.0 * np.log10(np.maximum(dtype(1e-10), M))
    return np.maximum(S, S.max() - dtype(80.0)).astype(dtype)


def onset_strength(y, sr=16000, hop=512, dtype=np.float64):
    S = mel_db(y, sr, hop, dtype)
    flux = np.maximum(0.0, S[1:] - S[:-1]).mean(axis=1)
    lag = 1 + N_FFT // (2 * hop)                        # the difference's lag plus the centring shift: 3 at hop 512
    return np.concatenate([np.zeros(lag, dtype), flux])[: len(S)].astype(dtype)


def normalise(env):
    x = env - env.min()
    return x / (x.max() + TINY)


# ---- step 7 ---------------------------------------------------------------------------------------------------------------------------------
def peak_params(sr, hop):
    return (int(0.03 * sr // hop), int(0.0 * sr // hop + 1), int(0.1 * sr // hop), int(0.1 * sr // hop + 1), int(0.03 * sr // hop))


def peak_pick(x, pre_max, post_max, pre_avg, post_avg, wait, delta=0.07, margins=None):
    """The onset frames of x.  `margins` (a list) receives per frame (i, |x - mean - delta|, x - the largest OTHER value of the max window)."""
    T, peaks, last = len(x), [], None
    for i in range(T):
        win = x[max(0, i - pre_max): min(T, i + post_max)]
        mean = x[max(0, i - pre_avg): min(T, i + post_avg)].mean()
        if margins is not None:
            others = np.delete(win, min(i, pre_max))
            margins.append((i, abs(x[i] - mean - delta), float(x[i] - others.max()) if len(others) else np.inf))
        if x[i] == win.max() and x[i] >= mean + delta and (last is None or i - last > wait):
            peaks.append(i)
            last = i
    return np.asarray(peaks, dtype=np.int64)


def onset_detect(y, sr=16000, hop=512, units="frames", delta=0.07, dtype=np.float64, params=None):
    env = onset_strength(y, sr, hop, dtype)
    if not env.any():
        frames = np.zeros(0, dtype=np.int64)
    else:
        frames = peak_pick(normalise(env.astype(np.float64)), *(params or peak_params(sr, hop)), delta=delta)
    return frames if units == "frames" else frames * hop if units == "samples" else frames * hop / float(sr)


def unsafe_frames(y, sr=16000, hop=512, delta=0.07, eps=1e-6):
    """Frames of the take whose decision the restatement itself takes within eps of a boundary: |x - mean - delta| < eps, or a tie (to eps) for the
    maximum of the max window in a frame that the threshold test does not already rule out by more than eps (the envelope's leading zeros tie
    exactly, and are 0.07 below the threshold).  Only these may be left out of a comparison of onset sets.  Returns (frames, the smallest threshold
    margin)."""
    env = onset_strength(y, sr, hop)
    if not env.any():
        return np.zeros(0, dtype=np.int64), np.inf
    m, x = [], normalise(env)
    params = peak_params(sr, hop)
    peak_pick(x, *params, delta=delta, margins=m)
    bad = []
    for i, thr, tie in m:
        mean = x[max(0, i - params[2]): min(len(x), i + params[3])].mean()
        if thr < eps or (abs(tie) < eps and x[i] - mean - delta > -eps):
            bad.append(i)
    return np.asarray(bad, dtype=np.int64), min(thr for _, thr, _ in m)


# ---- the amplitude envelope and the dataloader's array ----------------------------------------------------------------------------------------
def amplitude_envelope(y, frame_length=1024):
    """dataloaders/beat_sep_lower.py:393-402 restated: a rolling view of frame_length samples, max |.|, the last value repeated frame_length - 1 times."""
    y = np.ascontiguousarray(y)
    view = np.lib.stride_tricks.sliding_window_view(y, frame_length)
    a = np.abs(view).max(axis=1)
    return np.pad(a, (0, frame_length - 1), mode="constant", constant_values=a[-1])


def onset_amplitude_ref(y, sr=16000):
    """:391-409 restated: (n, 2) float64 - the amplitude envelope, and a one-hot of the onset FRAMES used as sample indices."""
    onset = np.zeros(len(y), dtype=float)
    onset[onset_detect(y, sr=sr, hop=512, units="frames")] = 1.0
    return np.concatenate([amplitude_envelope(y).reshape(-1, 1), onset.reshape(-1, 1)], axis=1)
