"""The audio front end on the device: amplitude envelope and onset detection of a waveform (csrc/syn_audio.inc).

What the reference takes from numpy stride tricks and `librosa.onset.onset_detect` - the `(n, 2)` `onset+amplitude` input of the model
(dataloaders/beat_sep_lower.py:391-409) and the onset times of the beat consistency (utils/metric.py:64-76) - restated from the algorithm, without
librosa: centred 2048-sample frames, periodic Hann window, power spectrum, 128 Slaney mel bands, dB with an 80 dB floor under the take's maximum, the
mean positive band difference (lag 1, shifted by 2 frames), min-max normalisation and librosa's peak picking.  Everything behind the fp32 samples is
fp64 on the device, in a fixed order: a take's result does not depend on what shares its launch.

Differences to librosa, on purpose:
* `onset_strength` returns float64 (librosa: float32 - its spectrogram is complex64).  The onsets are decisions on the float64 envelope.
* the feature functions do not resample: their input IS the waveform at `sr`, and `read_wave` refuses a file of another rate.  A file at any other
  rate goes through `load_wave` / `resample` first (csrc/syn_audio_resample.inc): the reference's `librosa.load` + `librosa.resample`
  restated as a Kaiser-windowed sinc on the exact rational grid, fp64 behind the fp32 samples - the project's own definition, not soxr's bits.

Every function takes a numpy array, a CPU tensor or a device tensor (arrays and CPU tensors are copied to the current device), or a list of takes of
different lengths, which is ONE batched launch sequence and returns a list.  Arguments are checked (ValueError) before anything touches the device.
"""
from __future__ import annotations

import numpy as np

N_FFT = 2048
FRAME_LENGTH = 1024
UNITS = ("frames", "samples", "time")


def peak_pick_defaults(sr, hop_length):
    """(pre_max, post_max, pre_avg, post_avg, wait) of librosa.onset.onset_detect in frames: 0.03 s, 0 s + 1, 0.1 s, 0.1 s + 1, 0.03 s."""
    return (int(0.03 * sr // hop_length), int(0.0 * sr // hop_length + 1), int(0.1 * sr // hop_length), int(0.1 * sr // hop_length + 1),
            int(0.03 * sr // hop_length))


def n_frames(n_samples: int, hop_length: int = 512) -> int:
    return 1 + n_samples // hop_length


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def _as_list(y):
    return (list(y), True) if isinstance(y, (list, tuple)) else ([y], False)


def _check_takes(takes, what, min_len, dim=1):
    import torch
    if not takes:
        raise ValueError(f"{what}: an empty list of takes")
    for t in takes:
        shape = tuple(t.shape) if torch.is_tensor(t) else np.shape(t)
        if len(shape) != dim:
            raise ValueError(f"{what}: a take is a {dim}-D array of samples, got shape {shape}")
        if shape[0] < min_len:
            raise ValueError(f"{what}: a take of {shape[0]} samples is shorter than {min_len}")


def _check_hop(hop_length, what):
    if int(hop_length) != hop_length or not 1 <= hop_length <= N_FFT:
        raise ValueError(f"{what}: hop_length must be an integer in 1..{N_FFT}, got {hop_length!r}")


def _check_sr(sr, what):
    if not sr > 0:
        raise ValueError(f"{what}: the sample rate must be positive, got {sr!r}")


def _to_device(t, dtype):
    import torch
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64 if dtype == torch.float64 else np.float32)))
    return t.detach().to(device=t.device if t.is_cuda else "cuda", dtype=dtype).contiguous()


class _Batch:
    """Takes back to back on the device, with their sample and frame offsets."""

    def __init__(self, takes, hop_length=None):
        import torch
        parts = [_to_device(t, torch.float32) for t in takes]
        self.dev = parts[0].device
        self.y = torch.cat(parts) if len(parts) > 1 else parts[0]
        self.lens = [int(p.numel()) for p in parts]
        self.soff_host = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.soff = torch.from_numpy(self.soff_host).to(self.dev)
        if hop_length is not None:
            self.frames = [n_frames(n, hop_length) for n in self.lens]
            self.foff_host = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
            self.foff = torch.from_numpy(self.foff_host).to(self.dev)

    def split_samples(self, x):
        return [x[self.soff_host[i]:self.soff_host[i + 1]] for i in range(len(self.lens))]

    def split_frames(self, x):
        return [x[self.foff_host[i]:self.foff_host[i + 1]] for i in range(len(self.lens))]


# ---- the stages ---------------------------------------------------------------------------------------------------------------------------
def _amplitude(b: _Batch, frame_length: int):
    import torch
    from . import _lib
    out = torch.empty_like(b.y)
    _lib.check(_lib.load().syn_audio_amplitude(b.y.data_ptr(), b.soff.data_ptr(), len(b.lens), max(b.lens), int(frame_length), out.data_ptr(),
                                               _lib.current_stream(b.dev)), "syn_audio_amplitude")
    return out


def power_spectrum(y, hop_length: int = 512):
    """(T, 1025) float64 on the device: |DFT|^2 of the centred, Hann-windowed 2048-sample frames (`syn_audio_power_spectrum`)."""
    import torch
    from . import _lib
    takes, many = _as_list(y)
    _check_takes(takes, "power_spectrum", 1)
    _check_hop(hop_length, "power_spectrum")
    b = _Batch(takes, int(hop_length))
    total = int(b.foff_host[-1])
    p = torch.empty(total, N_FFT // 2 + 1, dtype=torch.float64, device=b.dev)
    _lib.check(_lib.load().syn_audio_power_spectrum(b.y.data_ptr(), b.soff.data_ptr(), b.foff.data_ptr(), len(b.lens), max(b.frames), total, int(hop_length),
                                                    p.data_ptr(), _lib.current_stream(b.dev)), "syn_audio_power_spectrum")
    out = b.split_frames(p)
    return out if many else out[0]


def _mel_db(b: _Batch, sr, hop_length):
    import torch
    from . import _lib
    lib = _lib.load()
    total = int(b.foff_host[-1])
    ws = torch.empty(lib.syn_audio_workspace_bytes(total) // 8, dtype=torch.float64, device=b.dev)
    s = torch.empty(total, 128, dtype=torch.float64, device=b.dev)
    _lib.check(lib.syn_audio_mel_db(b.y.data_ptr(), b.soff.data_ptr(), b.foff.data_ptr(), len(b.lens), max(b.frames), total, float(sr), int(hop_length),
                                    ws.data_ptr(), s.data_ptr(), _lib.current_stream(b.dev)), "syn_audio_mel_db")
    return s


def _envelopes(b: _Batch, sr, hop_length):
    """(raw, normalised) envelopes of all takes, frames back to back, float64 on the device."""
    import torch
    from . import _lib
    s = _mel_db(b, sr, hop_length)
    env, x = torch.empty(s.shape[0], dtype=torch.float64, device=b.dev), torch.empty(s.shape[0], dtype=torch.float64, device=b.dev)
    _lib.check(_lib.load().syn_audio_onset_env(s.data_ptr(), b.foff.data_ptr(), len(b.lens), max(b.frames), int(hop_length), env.data_ptr(), x.data_ptr(), _lib.current_stream(b.dev)),
               "syn_audio_onset_env")
    return env, x


def _peak_pick(x, raw, foff, n_takes, params, delta):
    """-> (mask uint8 over all frames, count int32 per take), on the device."""
    import torch
    from . import _lib
    mask = torch.empty(x.shape[0], dtype=torch.uint8, device=x.device)
    count = torch.empty(n_takes, dtype=torch.int32, device=x.device)
    _lib.check(_lib.load().syn_audio_peak_pick(x.data_ptr(), None if raw is None else raw.data_ptr(), foff.data_ptr(), n_takes, *[int(p) for p in params],
                                               float(delta), mask.data_ptr(), count.data_ptr(), _lib.current_stream(x.device)), "syn_audio_peak_pick")
    return mask, count


# ---- the public functions -----------------------------------------------------------------------------------------------------------------
def amplitude_envelope(y, frame_length: int = FRAME_LENGTH):
    """a[i] = max |y[i : i + frame_length]| for i <= n - frame_length, the last frame_length - 1 entries repeating a[n - frame_length]: (n,) float32
    on the device, exact (dataloaders/beat_sep_lower.py:393-402).  A take shorter than frame_length is a ValueError (the reference fails there too)."""
    takes, many = _as_list(y)
    if int(frame_length) != frame_length or not 1 <= frame_length <= 4096:
        raise ValueError(f"amplitude_envelope: frame_length must be an integer in 1..4096, got {frame_length!r}")
    _check_takes(takes, "amplitude_envelope", int(frame_length))
    b = _Batch(takes)
    out = b.split_samples(_amplitude(b, int(frame_length)))
    return out if many else out[0]


def onset_strength(y, sr=16000, hop_length: int = 512):
    """The onset strength envelope librosa.onset.onset_strength(y=y, sr=sr, hop_length=hop_length) computes with its defaults, (1 + n // hop_length,)
    FLOAT64 on the device (librosa: float32): env[t] = mean over 128 mel bands of max(0, S[t - lag + 1] - S[t - lag]), S in dB, env[:lag] = 0, lag = 1 +
    2048 // (2 hop_length) = 3 at hop 512."""
    takes, many = _as_list(y)
    _check_takes(takes, "onset_strength", 1)
    _check_hop(hop_length, "onset_strength")
    _check_sr(sr, "onset_strength")
    b = _Batch(takes, int(hop_length))
    out = b.split_frames(_envelopes(b, sr, hop_length)[0])
    return out if many else out[0]


def _detect(b, raw, x, sr, hop_length, units, delta, params):
    """Peak picking over a batch -> (per-take results in `units` as numpy, mask on the device)."""
    mask, _ = _peak_pick(x, raw, b.foff, len(b.frames), params, delta)
    host = mask.cpu().numpy()
    out = []
    for i in range(len(b.frames)):
        frames = np.flatnonzero(host[b.foff_host[i]:b.foff_host[i + 1]]).astype(np.int64)
        out.append(frames if units == "frames" else frames * int(hop_length) if units == "samples" else frames * int(hop_length) / float(sr))
    return out, mask


class _FrameBatch:
    """Envelopes handed in by the caller: only the frame offsets exist."""

    def __init__(self, envs):
        import torch
        self.frames = [int(e.numel()) for e in envs]
        self.dev = envs[0].device
        self.foff_host = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)
        self.foff = torch.from_numpy(self.foff_host).to(self.dev)


def onset_detect(y=None, sr=16000, hop_length: int = 512, units: str = "frames", onset_envelope=None, normalize: bool = True, delta: float = 0.07,
                 wait=None, pre_max=None, post_max=None, pre_avg=None, post_avg=None):
    """librosa.onset.onset_detect(y=y, sr=sr, hop_length=hop_length, units=units, ...) without backtracking: the onset frames (int64 numpy), samples
    (frames * hop_length) or times (frames * hop_length / sr, float64 numpy) of one take, or a list of them for a list of takes.  A window parameter
    left at None is librosa's default in frames (`peak_pick_defaults`; (0, 1, 3, 4, 0) at sr 16000, hop 512).  `onset_envelope`: detect on this
    envelope (or one per take) instead of computing it from y.  A take whose envelope is zero everywhere has no onsets."""
    import torch
    if units not in UNITS:
        raise ValueError(f"onset_detect: units must be one of {UNITS}, got {units!r}")
    _check_hop(hop_length, "onset_detect")
    _check_sr(sr, "onset_detect")
    given = (pre_max, post_max, pre_avg, post_avg, wait)
    params = tuple(d if g is None else g for g, d in zip(given, peak_pick_defaults(sr, int(hop_length))))
    if any(int(p) != p for p in params) or min(params[0], params[2], params[4]) < 0 or min(params[1], params[3]) < 1:
        raise ValueError(f"onset_detect: pre_max, pre_avg, wait must be integers >= 0 and post_max, post_avg >= 1, got {params}")
    if not np.isfinite(delta):
        raise ValueError(f"onset_detect: delta must be finite, got {delta!r}")
    if onset_envelope is not None:
        envs, many = _as_list(onset_envelope)
        _check_takes(envs, "onset_detect (onset_envelope)", 1)
        envs = [_to_device(e, torch.float64) for e in envs]
        b = _FrameBatch(envs)
        raw = torch.cat(envs) if len(envs) > 1 else envs[0]
        x = raw
        if normalize:                                   # the arithmetic of k_onset_env's last line, per take
            x = torch.cat([(e - e.min()) / ((e.max() - e.min()) + 1.1754943508222875e-38) for e in envs])
    else:
        if y is None:
            raise ValueError("onset_detect: y or onset_envelope must be given")
        takes, many = _as_list(y)
        _check_takes(takes, "onset_detect", 1)
        b = _Batch(takes, int(hop_length))
        raw, x = _envelopes(b, sr, hop_length)
        if not normalize:
            x = raw
    out, _ = _detect(b, raw, x, sr, hop_length, units, delta, params)
    return out if many else out[0]


def onset_amplitude(y, sr=16000):
    """The model's `onset+amplitude` audio input, (n, 2) float32 on the device, as dataloaders/beat_sep_lower.py:391-409 builds it from a waveform at
    `sr`: column 0 = amplitude_envelope(y, 1024); column 1 = zero, with 1.0 at INDEX f for every onset frame f of onset_detect(y, sr, units='frames') -
    the reference indexes samples by frame numbers; its cache files and the trained models were made that way, so it is kept."""
    import torch
    takes, many = _as_list(y)
    _check_takes(takes, "onset_amplitude", FRAME_LENGTH)
    _check_sr(sr, "onset_amplitude")
    b = _Batch(takes, 512)
    amp = _amplitude(b, FRAME_LENGTH)
    raw, x = _envelopes(b, sr, 512)
    mask, _ = _peak_pick(x, raw, b.foff, len(b.lens), peak_pick_defaults(sr, 512), 0.07)
    out = []
    for i, n in enumerate(b.lens):
        o = torch.zeros(n, 2, dtype=torch.float32, device=b.dev)
        o[:, 0] = amp[b.soff_host[i]:b.soff_host[i + 1]]
        o[: b.frames[i], 1] = mask[b.foff_host[i]:b.foff_host[i + 1]].float()       # frames <= n // 512 < n
        out.append(o)
    return out if many else out[0]


def read_wave(path, sr=16000):
    """A `.wav` (scipy.io.wavfile: int16 -> / 32768, float as it is; the first channel of several) or `.npy` waveform as float32.  A `.wav` at another
    rate than `sr` is refused: resampling is out of scope here, bring the 16 kHz waveform the reference's `wave16k/` holds - or use `load_wave`."""
    if str(path).endswith(".npy"):
        y = np.load(path)
    else:
        from scipy.io import wavfile
        rate, y = wavfile.read(path)
        if rate != sr:
            raise ValueError(f"{path}: sample rate {rate}, expected {sr}; resampling is out of scope - convert the file to {sr} Hz first, or use load_wave")
        if y.dtype == np.int16:
            y = y.astype(np.float32) / 32768.0
        elif y.dtype.kind != "f":
            raise ValueError(f"{path}: int16 or float samples, got {y.dtype}")
    y = np.asarray(y, dtype=np.float32)
    return np.ascontiguousarray(y[:, 0] if y.ndim == 2 else y)


# ---- resampling (csrc/syn_audio_resample.inc) -------------------------------------------------------------------------------------------
RESAMPLE_ZEROS = 64                          # zero crossings of the sinc on either side
RESAMPLE_ROLLOFF = 0.9475937167399596        # the pass band's edge as a fraction of the lower Nyquist rate
RESAMPLE_BETA = 14.769656459379492           # of the Kaiser window
RESAMPLE_MAX_TAPS = 1 << 22                  # 2 K + 1 may not exceed this


def _check_rates(orig_sr, target_sr, what):
    for name, sr in (("orig_sr", orig_sr), ("target_sr", target_sr)):
        if isinstance(sr, bool) or not isinstance(sr, (int, float, np.integer, np.floating)) or not sr > 0 or int(sr) != sr or sr >= 2 ** 31:
            raise ValueError(f"{what}: {name} must be a positive integer number of Hz, got {sr!r}")
    return int(orig_sr), int(target_sr)


_taps_cache = {}


def resample_taps(orig_sr, target_sr):
    """(L, M, K, h) of the conversion orig_sr -> target_sr: L / M = target_sr / orig_sr in lowest terms, h the 2 K + 1 taps h[-K .. K] (float64 numpy,
    read-only, natural order: h[K + k]) of g sinc(g k / L) I0(beta sqrt(1 - u^2)) / I0(beta), u = g k / (64 L), g = rolloff min(1, L / M),
    K = floor(64 L / g).  Built once per (L, M) on the host.  A table of more than 2^22 taps is a ValueError naming both rates."""
    import math
    orig_sr, target_sr = _check_rates(orig_sr, target_sr, "resample_taps")
    d = math.gcd(orig_sr, target_sr)
    L, M = target_sr // d, orig_sr // d
    if (L, M) not in _taps_cache:
        g = RESAMPLE_ROLLOFF * min(1, L / M)
        K = int(math.floor(RESAMPLE_ZEROS * L / g))
        if 2 * K + 1 > RESAMPLE_MAX_TAPS:
            raise ValueError(f"resample: {orig_sr} Hz -> {target_sr} Hz needs a table of {2 * K + 1} taps (L = {L}, M = {M}), more than {RESAMPLE_MAX_TAPS}: "
                             "choose rates with a larger common divisor")
        k = np.arange(-K, K + 1, dtype=np.float64)
        u = g * k / (L * RESAMPLE_ZEROS)
        h = g * np.sinc(g * k / L) * np.i0(RESAMPLE_BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(RESAMPLE_BETA)
        h.setflags(write=False)
        _taps_cache[(L, M)] = (L, M, K, h)
    return _taps_cache[(L, M)]


def pack_taps(L, M, K, h):
    """The kernel's layout of the table (include/syn_hip.h): (T / 2, L, 2) float64, T = 2 (K // L) + 2, entry [t // 2, r, t % 2] = h[p + (W - t) L]
    with W = K // L and p = (r M) mod L the phase of the outputs m = r (mod L); zero where the index leaves -K .. K."""
    W = K // L
    p = (np.arange(L, dtype=np.int64) * M) % L
    k = p[None, :] + (W - np.arange(2 * W + 2, dtype=np.int64)[:, None]) * L          # [t, r]
    inside = np.abs(k) <= K
    table = np.where(inside, h[np.where(inside, k + K, 0)], 0.0)
    return np.ascontiguousarray(table.reshape(W + 1, 2, L).transpose(0, 2, 1))


_device_taps_cache = {}


def _device_taps(L, M, K, h, dev):
    import torch
    key = (L, M, str(dev))
    if key not in _device_taps_cache:
        if len(_device_taps_cache) >= 8:                # a handful of ratios at most stay resident (a table is 0.5 MB at 320 / 441, 24 MB at L = 16001)
            _device_taps_cache.pop(next(iter(_device_taps_cache)))
        _device_taps_cache[key] = torch.from_numpy(pack_taps(L, M, K, h)).to(dev)
    return _device_taps_cache[key]


def resample_length(n, L, M):
    return -((-n * L) // M)


def resample(y, orig_sr, target_sr, dtype=None):
    """The take(s) at `orig_sr` brought to `target_sr`: ceil(n L / M) samples each, on the device, y[m] = sum_j x[j] h[m M - j L] with the taps of
    `resample_taps` - every sum an fp64 fma chain over ascending j, rounded once to float32 (`dtype=torch.float64`: the sums themselves).  One launch
    for a list of takes; a take's bits do not depend on its batch mates.  `orig_sr == target_sr` returns what it was given, without a launch."""
    import torch
    from . import _lib
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"resample: dtype is torch.float32 or torch.float64, got {dtype!r}")
    orig_sr, target_sr = _check_rates(orig_sr, target_sr, "resample")
    takes, many = _as_list(y)
    _check_takes(takes, "resample", 1)
    if orig_sr == target_sr:
        return y
    L, M, K, h = resample_taps(orig_sr, target_sr)
    b = _Batch(takes)
    taps = _device_taps(L, M, K, h, b.dev)
    lens = [resample_length(n, L, M) for n in b.lens]
    ooff_host = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ooff = torch.from_numpy(ooff_host).to(b.dev)
    out = torch.empty(int(ooff_host[-1]), dtype=dtype, device=b.dev)
    _lib.check(_lib.load().syn_audio_resample(b.y.data_ptr(), b.soff.data_ptr(), ooff.data_ptr(), len(b.lens), max(b.lens), L, M, taps.data_ptr(), taps.numel(),
                                              out.data_ptr() if dtype == torch.float32 else None, out.data_ptr() if dtype == torch.float64 else None,
                                              _lib.current_stream(b.dev)), "syn_audio_resample")
    parts = [out[ooff_host[i]:ooff_host[i + 1]] for i in range(len(lens))]
    return parts if many else parts[0]


def decode_wave(path):
    """(rate, samples) of a `.wav` as scipy.io.wavfile reads it: float32 samples, the first channel of several; int16 / 2^15, int32 / 2^31 (24-bit
    files arrive as int32), uint8 (v - 128) / 128, float as it is."""
    from scipy.io import wavfile
    rate, y = wavfile.read(path)
    if y.dtype == np.int16:
        y = y.astype(np.float32) / 32768.0
    elif y.dtype == np.int32:
        y = (y.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif y.dtype == np.uint8:
        y = (y.astype(np.float32) - 128.0) / 128.0
    elif y.dtype.kind != "f":
        raise ValueError(f"{path}: int16, int32, uint8 or float samples, got {y.dtype}")
    y = np.asarray(y, dtype=np.float32)
    return int(rate), np.ascontiguousarray(y[:, 0] if y.ndim == 2 else y)


def load_waves(paths, sr=16000, via=None):
    """`load_wave` of several files: the files of one rate share one `resample` launch (per step), and come back in the order given."""
    import torch
    orig = []
    for path in paths:
        if str(path).endswith(".npy"):
            y = np.asarray(np.load(path), dtype=np.float32)
            orig.append((int(sr), np.ascontiguousarray(y[:, 0] if y.ndim == 2 else y)))
        else:
            orig.append(decode_wave(path))
    if via is not None:
        _check_rates(via, sr, "load_wave (via)")
    out = [None] * len(orig)
    for rate in sorted({r for r, _ in orig}):
        idx = [i for i, (r, _) in enumerate(orig) if r == rate]
        waves = [orig[i][1] for i in idx]
        for w, path in zip(waves, (paths[i] for i in idx)):
            if w.ndim != 1 or len(w) < 1:
                raise ValueError(f"{path}: no samples")
        if rate != sr:
            steps = [(rate, sr)] if via is None else [(rate, int(via)), (int(via), sr)]
            for a, b in steps:
                waves = resample(waves, a, b)
        for i, w in zip(idx, waves):
            out[i] = _to_device(w, torch.float32)
    return out


def load_wave(path, sr=16000, via=None):
    """A `.wav` at ANY rate (or a `.npy` waveform, taken to be at `sr`) as a float32 DEVICE tensor at `sr`: decoded like `read_wave` (plus int32 and
    uint8 PCM) and, where the file's rate differs, resampled in one step (`resample`).  `via=22050` runs the reference's own two steps instead
    (librosa.load's 22.05 kHz, then librosa.resample to `sr`).  mp3 and flac are not decoded."""
    return load_waves([path], sr, via)[0]
