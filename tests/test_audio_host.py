"""The audio front end, host side: tests/audio_features_ref.py (the fp64 restatement the GPU tests compare with) pinned to independent code - scipy's
STFT, closed-form anchors of the Slaney filterbank, scipy.ndimage's filters for the peak picking, the reference's stride-trick lines - plus the
margins of the GPU test's own inputs, the C ABI and the argument checks of syntalker_amd.audio (which raise before anything touches the device)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import audio_features_ref as ar
from tests.conftest import REPO

from syntalker_amd import _lib, audio, metrics


def test_stft_stage_against_scipy_signal():
    import scipy.signal
    y = ar.speech_like(0, 16000)
    for hop in (512, 300):
        _, _, z = scipy.signal.stft(y.astype(np.float64), window=ar.hann(), nperseg=2048, noverlap=2048 - hop, nfft=2048, boundary="zeros", padded=False,
                                    scaling="psd", return_onesided=True)
        # scipy scales the spectrum by 1 / sqrt(sum w^2) ('psd', fs = 1); undo it
        want = (np.abs(z.T) ** 2) * (ar.hann() ** 2).sum()
        got = ar.power_spectrum(y, hop)
        T = min(len(want), len(got))
        assert len(got) == 1 + len(y) // hop and T >= len(got) - 1          # scipy drops a last frame that does not fit whole
        assert np.abs(got[:T] - want[:T]).max() <= 1e-10 * want.max()


def test_mel_filterbank_against_closed_form_anchors():
    for sr in (16000, 22050):
        f, W = ar.mel_edges(sr), ar.mel_filterbank(sr)
        assert W.shape == (128, 1025) and (W >= 0).all()
        assert ((W > 0).sum(0) <= 2).all()                                  # at most two filters over an FFT bin
        assert f[0] == 0.0 and abs(f[-1] - sr / 2) <= 1e-9 and len(f) == 130
        top_mel = 15.0 + np.log(sr / 2 / 1000.0) / (np.log(6.4) / 27.0)
        mels = np.linspace(0, top_mel, 130)
        below = mels < 15.0
        assert np.allclose(f[below], mels[below] * 200.0 / 3.0, rtol=1e-13)                    # linear: 200/3 Hz per mel
        assert abs(float(ar.mel_to_hz(15.0)) - 1000.0) <= 1e-10 and abs(float(ar.hz_to_mel(1000.0)) - 15.0) <= 1e-12
        assert abs(float(ar.mel_to_hz(15.0 + 27.0)) - 6400.0) <= 1e-9                            # 27 log steps = a factor 6.4
        # a triangle of unit height sampled every df sums to ~ (width / 2) / df, the bins under it; the rows are that times 2 / width:
        # row_sum * width / 2 ~ width / (2 df), the bin density
        df = sr / 2048
        width = f[2:] - f[:-2]
        wide = width > 8 * df
        assert wide.sum() > 40 and np.abs(W.sum(1) * width / 2.0 / (width / (2.0 * df)) - 1.0)[wide].max() < 0.05


@pytest.mark.parametrize("params", [(0, 1, 3, 4, 0), (1, 1, 4, 5, 1)])
def test_peak_picking_against_scipy_ndimage(params):
    import scipy.ndimage as ndi
    pre_max, post_max, pre_avg, post_avg, wait = params
    r = np.random.RandomState(5)
    x = ar.normalise(np.abs(r.randn(400)) * (r.rand(400) > 0.5))
    got = ar.peak_pick(x, *params)
    # the filters' windows, centred: max over [i - pre_max, i + post_max), mean over [i - pre_avg, i + post_avg)
    n_max, n_avg = pre_max + post_max, pre_avg + post_avg
    mx = ndi.maximum_filter1d(x, n_max, mode="constant", cval=x.min(), origin=int(np.ceil(0.5 * (pre_max - post_max))))
    av = ndi.uniform_filter1d(x, n_avg, mode="nearest", origin=int(np.ceil(0.5 * (pre_avg - post_avg))))
    cand = (x == mx) & (x >= av + 0.07)
    want, last = [], -np.inf
    for i in np.flatnonzero(cand):
        if i - last > wait:
            want.append(i)
            last = i
    lo, hi = max(pre_max, pre_avg), len(x) - max(post_max, post_avg)       # the interior: the filters pad, the specification truncates
    inside = lambda v: [i for i in v if lo <= i < hi]
    if wait == 0:
        assert inside(got) == inside(want) and len(inside(got)) > 20
    else:                                                                   # with waiting the edges reach inwards only through a kept peak: compare the candidates
        mine = [i for i in range(len(x)) if x[i] == x[max(0, i - pre_max): i + post_max].max()
                and x[i] >= x[max(0, i - pre_avg): i + post_avg].mean() + 0.07]
        assert inside(mine) == inside(np.flatnonzero(cand)) and len(inside(mine)) > 20
        assert all(b - a > wait for a, b in zip(got[:-1], got[1:])) and set(got) <= set(mine)
        kept = set(got)
        assert all(any(0 < i - p <= wait for p in kept) for i in mine if i not in kept)       # whatever was dropped had a kept peak within `wait`


def test_amplitude_envelope_against_the_reference_lines_restated():
    y = ar.speech_like(1, 5000)
    frame_length = 1024
    shape = (y.shape[-1] - frame_length + 1, frame_length)
    rolling = np.lib.stride_tricks.as_strided(y, shape=shape, strides=(y.strides[-1], y.strides[-1]))
    want = np.max(np.abs(rolling), axis=1)
    want = np.pad(want, (0, frame_length - 1), mode="constant", constant_values=want[-1])
    got = ar.amplitude_envelope(y)
    assert got.dtype == np.float32 and got.shape == y.shape and np.array_equal(got, want)
    brute = np.array([np.abs(y[i:i + 1024]).max() for i in range(len(y) - 1023)])
    assert np.array_equal(got[: len(brute)], brute) and (got[len(brute):] == brute[-1]).all()


def test_gpu_inputs_keep_their_distance_from_every_decision():
    """The takes test_gpu_audio.py compares onset sets on: the restatement leaves out no frame at either rate, every take long enough to have a
    non-zero envelope (more than 3 frames) has onsets, and some frames are not onsets."""
    for (seed, n), y in zip(ar.CASES, ar.gpu_takes()):
        assert y.dtype == np.float32 and len(y) == n and abs(np.abs(y).max() - 0.8) < 1e-6
        for sr, hop in ar.RATES:
            bad, margin = ar.unsafe_frames(y, sr, hop)
            frames = ar.onset_detect(y, sr, hop)
            print(f"seed {seed}, {n} samples, sr {sr}: {len(frames)} onsets of {1 + n // hop} frames, smallest threshold margin {margin:.2e}")
            assert len(bad) == 0
            assert (len(frames) >= 1) == (1 + n // hop > 3) and len(frames) < 1 + n // hop
    assert len(ar.onset_detect(np.zeros(ar.SILENCE, np.float32))) == 0
    assert [1 + n // 512 for _, n in ar.CASES] == [17, 32, 126, 313, 3]


def test_float32_variant_is_librosa_grade_and_the_units_follow_the_frames():
    y = ar.speech_like(1, 64000)
    e64, e32 = ar.onset_strength(y), ar.onset_strength(y, dtype=np.float32)
    assert e32.dtype == np.float32 and 1e-8 < np.abs(e64 - e32).max() / e64.max() < 1e-5
    f = ar.onset_detect(y)
    assert np.array_equal(ar.onset_detect(y, units="samples"), f * 512) and np.array_equal(ar.onset_detect(y, units="time"), f * 512 / 16000.0)
    oa = ar.onset_amplitude_ref(y)
    assert oa.shape == (64000, 2) and oa.dtype == np.float64 and np.array_equal(np.flatnonzero(oa[:, 1]), f)      # frames used as sample indices


NEW_EXPORTS = ("syn_audio_workspace_bytes", "syn_audio_amplitude", "syn_audio_power_spectrum", "syn_audio_mel_db", "syn_audio_onset_env", "syn_audio_peak_pick")


def test_header_declares_the_audio_exports_and_the_abi_version_stays():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert re.search(r"^#define SYN_ABI_VERSION 9\b", header, flags=re.M) and _lib.ABI_VERSION == 9
    srcs = "".join(open(os.path.join(REPO, "syntalker_amd", "csrc", n)).read() for n in sorted(os.listdir(os.path.join(REPO, "syntalker_amd", "csrc")))
                   if n.endswith((".inc", ".hip")))
    assert '#include "syn_audio.inc"' in srcs
    for name in NEW_EXPORTS:
        assert re.search(rf"^int(?:64_t)?\s+{name}\s*\(", header, flags=re.M) and name in _lib.EXPORTS, name
        assert len(re.findall(rf"^int(?:64_t)?\s+{name}\s*\([^;{{]*\{{", srcs, flags=re.M)) == 1, name          # defined once
    lib = _lib.load()
    assert lib.syn_version() == 9
    assert all(hasattr(lib, n) for n in NEW_EXPORTS)
    assert lib.syn_audio_workspace_bytes(0) == -1 and lib.syn_audio_workspace_bytes(313) == 313 * 1025 * 8
    assert len(lib.syn_audio_peak_pick.argtypes) == 13 and len(lib.syn_audio_mel_db.argtypes) == 11
    assert lib.syn_audio_mel_db(None, None, None, 1, 1, 1, 16000.0, 512, None, None, None) != 0 and b"syn_audio_mel_db" in lib.syn_last_error()


def test_argument_checks_raise_before_the_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(audio, "_Batch", lambda *a, **k: pytest.fail("a batch went to the device"))
    y = np.zeros(4000, dtype=np.float32)
    for bad in (np.zeros((2, 4000), np.float32), torch.zeros(1, 4000), np.float32(1.0), [y, np.zeros((4000, 1), np.float32)], []):
        for fn in (audio.amplitude_envelope, audio.onset_strength, audio.onset_detect, audio.onset_amplitude, audio.power_spectrum):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (audio.amplitude_envelope, audio.onset_amplitude):
        with pytest.raises(ValueError, match="shorter than 1024"):
            fn(np.zeros(1023, dtype=np.float32))
        with pytest.raises(ValueError, match="shorter than 1024"):
            fn([y, torch.zeros(100)])
    for hop in (0, 2049, -1, 1.5):
        with pytest.raises(ValueError, match="hop_length"):
            audio.onset_strength(y, hop_length=hop)
        with pytest.raises(ValueError, match="hop_length"):
            audio.onset_detect(y, hop_length=hop)
    with pytest.raises(ValueError, match="units"):
        audio.onset_detect(y, units="seconds")
    with pytest.raises(ValueError, match="frame_length"):
        audio.amplitude_envelope(y, frame_length=0)
    with pytest.raises(ValueError):
        audio.onset_detect(y, post_max=0)
    with pytest.raises(ValueError):
        audio.onset_detect(None)
    with pytest.raises(ValueError, match="sample rate"):
        audio.onset_detect(y, sr=0)
    assert audio.peak_pick_defaults(16000, 512) == (0, 1, 3, 4, 0) == ar.peak_params(16000, 512)
    assert audio.peak_pick_defaults(22050, 512) == (1, 1, 4, 5, 1) == ar.peak_params(22050, 512)


def test_read_wave_and_the_metrics_surface(tmp_path):
    import inspect
    from scipy.io import wavfile
    y = ar.speech_like(0, 2000)
    wavfile.write(tmp_path / "a.wav", 16000, np.round(y * 32767).astype(np.int16))
    wavfile.write(tmp_path / "f.wav", 16000, y)
    wavfile.write(tmp_path / "b.wav", 22050, y)
    np.save(tmp_path / "c.npy", y)
    got = audio.read_wave(str(tmp_path / "a.wav"))
    assert got.dtype == np.float32 and np.array_equal(got, np.round(y * 32767).astype(np.int16).astype(np.float32) / 32768.0)
    assert np.array_equal(audio.read_wave(str(tmp_path / "f.wav")), y) and np.array_equal(audio.read_wave(str(tmp_path / "c.npy")), y)
    with pytest.raises(ValueError, match="resampling is out of scope"):
        audio.read_wave(str(tmp_path / "b.wav"))
    assert str(inspect.signature(metrics.alignment.load_audio_hip)) == str(inspect.signature(metrics.alignment.load_audio))
    assert "audio_sr" in inspect.signature(metrics.beat_consistency_from_audio).parameters
