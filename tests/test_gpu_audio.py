"""The audio front end on the device (csrc/syn_audio.inc, syntalker_amd/audio.py) against the fp64 FFT restatement tests/audio_features_ref.py, which
test_audio_host.py pins to independent code.  Takes: 17, 32, 126 and 313 frames (one frame more than a 16-row tile, two whole tiles, several tiles
with a ragged last one), the shortest legal take (1024 samples, 3 frames) and 4 s of silence.  The envelope may be 1e-9 of its maximum away from
the restatement (the same GEMM-shaped fp64 product on a CPU lands at 3e-15; float32 arithmetic, librosa's, at 1e-6); the amplitude envelope, the
batching and the onset sets are exact."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import audio_features_ref as ar
from tests import motion_metrics_ref as mr
from tests.conftest import GOLDEN, REPO

from syntalker_amd import audio, metrics

pytestmark = pytest.mark.gpu
ENV_BOUND = 1e-9


@pytest.fixture(scope="module")
def takes():
    return ar.gpu_takes()


@pytest.fixture(scope="module")
def ref_env(takes):
    return {(i, sr, hop): ar.onset_strength(y, sr, hop) for i, y in enumerate(takes) for sr, hop in ar.RATES}


@pytest.fixture(scope="module")
def dev_env(takes):
    """Each take alone, at both rates: the raw envelopes."""
    return {(i, sr, hop): audio.onset_strength(y, sr, hop).cpu().numpy() for i, y in enumerate(takes) for sr, hop in ar.RATES}


def test_power_spectrum_against_the_fft(takes):
    """The MFMA's fragment layout and the basis on data that cannot hide a transposition: an impulse train with integer amplitudes (every frame and
    every bin differs, re and im both matter), then a speech-like take; hop 512 and a hop that is no multiple of anything.  Bound: a 2048-term fp64
    sum is at worst 2048 * 2^-53 * sum |terms| = 2.3e-13 sum |terms| off, P = re^2 + im^2 twice that relative to its largest entry when sum |terms| is
    of the size of the largest |re| - a few times that here: 1e-11 (a transposed fragment or a wrong basis index is off by O(1))."""
    y = np.zeros(9000, dtype=np.float32)
    y[np.arange(7, 9000, 613)] = np.arange(1, 1 + len(np.arange(7, 9000, 613)), dtype=np.float32)
    for wave, hop in ((y, 512), (takes[0], 512), (takes[1], 300)):
        want = ar.power_spectrum(wave, hop)
        got = audio.power_spectrum(wave, hop).cpu().numpy()
        err = np.abs(got - want).max() / want.max()
        print(f"power spectrum, {len(wave)} samples, hop {hop}: max |delta| / max = {err:.3e}")
        assert got.shape == want.shape == (1 + len(wave) // hop, 1025) and err <= 1e-11


def test_amplitude_envelope_is_numpys_bit_for_bit(takes):
    for y in takes + [np.zeros(ar.SILENCE, np.float32), ar.speech_like(7, 3000)]:
        got = audio.amplitude_envelope(y)
        assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), ar.amplitude_envelope(y))
    y = takes[1]
    for length in (1, 2, 100, 1000, 4096):                                  # other windows: not a power of two, longer than a scan's block
        assert np.array_equal(audio.amplitude_envelope(y, frame_length=length).cpu().numpy(), ar.amplitude_envelope(y, length)), length
    t = torch.from_numpy(y)
    assert torch.equal(audio.amplitude_envelope(t), audio.amplitude_envelope(t.cuda()))       # CPU tensor, device tensor


def test_envelope_accuracy(takes, ref_env, dev_env):
    for (i, sr, hop), want in ref_env.items():
        got = dev_env[(i, sr, hop)]
        assert got.dtype == np.float64 and got.shape == want.shape == (1 + len(takes[i]) // hop,)
        if not want.any():
            assert not got.any()                                             # 3 frames: the lag and the centring shift leave only zeros
            continue
        err = np.abs(got - want).max() / want.max()
        f32 = np.abs(ar.onset_strength(takes[i], sr, hop, np.float32) - want).max() / want.max()
        print(f"take {i} ({len(takes[i])} samples, sr {sr}): device {err:.3e} of the envelope's maximum (float32 arithmetic: {f32:.3e})")
        assert err <= ENV_BOUND
    for hop, lag in ((300, 4), (2048, 1), (100, 11)):                        # other hops: another centring shift; 2048 is the largest row tile the LDS holds
        want, got = ar.onset_strength(takes[2], 16000, hop), audio.onset_strength(takes[2], 16000, hop).cpu().numpy()
        assert got.shape == want.shape and not got[:lag].any() and got[lag] > 0
        assert np.abs(got - want).max() <= ENV_BOUND * want.max()
        assert np.array_equal(audio.onset_detect(takes[2], hop_length=hop), ar.onset_detect(takes[2], 16000, hop))


@pytest.mark.parametrize("sr,hop", ar.RATES)
def test_onsets_are_the_restatements(takes, sr, hop):
    got_all = audio.onset_detect(takes, sr=sr, hop_length=hop)
    for i, y in enumerate(takes):
        want, got = ar.onset_detect(y, sr, hop), got_all[i]
        bad, _ = ar.unsafe_frames(y, sr, hop)
        assert len(bad) <= 0.01 * (1 + len(y) // hop)
        keep = lambda f: [int(v) for v in f if v not in set(bad.tolist())]
        assert got.dtype == np.int64 and keep(got) == keep(want), (i, sr)
        assert np.array_equal(audio.onset_detect(y, sr=sr, hop_length=hop), got)               # alone: the same frames
    # the envelope handed in, and the general rule at parameters of its own
    env = ar.onset_strength(takes[2], sr, hop)
    assert np.array_equal(audio.onset_detect(onset_envelope=env, sr=sr, hop_length=hop), ar.onset_detect(takes[2], sr, hop))
    x = ar.normalise(env)
    for params in ((2, 3, 5, 2, 4), (0, 1, 1, 1, 7)):
        got = audio.onset_detect(onset_envelope=x, sr=sr, hop_length=hop, normalize=False, delta=0.05, pre_max=params[0], post_max=params[1],
                                 pre_avg=params[2], post_avg=params[3], wait=params[4])
        assert np.array_equal(got, ar.peak_pick(x, *params, delta=0.05)) and len(got) > 3


def test_silence_has_no_onsets():
    z = np.zeros(ar.SILENCE, dtype=np.float32)
    assert audio.onset_detect(z).shape == (0,) and not audio.onset_strength(z).any()
    assert audio.onset_detect(z, delta=-1.0).shape == (0,)                  # an all-zero envelope has none, whatever the threshold
    oa = audio.onset_amplitude(z)
    assert oa.shape == (ar.SILENCE, 2) and not oa.any()
    both = audio.onset_detect([z, ar.speech_like(0, 16000)])
    assert both[0].shape == (0,) and np.array_equal(both[1], ar.onset_detect(ar.speech_like(0, 16000)))


def test_a_take_does_not_depend_on_its_batch_mates(takes):
    mid = takes[1:4]
    env = audio.onset_strength(mid)
    amp = audio.amplitude_envelope(mid)
    feats = audio.onset_amplitude(mid)
    frames = audio.onset_detect(mid)
    for k, y in enumerate(mid):
        assert torch.equal(env[k], audio.onset_strength(y)) and torch.equal(amp[k], audio.amplitude_envelope(y))
        assert torch.equal(feats[k], audio.onset_amplitude(y)) and np.array_equal(frames[k], audio.onset_detect(y))
    again = audio.onset_strength(list(reversed(mid)))
    assert all(torch.equal(a, b) for a, b in zip(env, reversed(again)))      # another order in the launch, the same bits


def test_onset_amplitude_is_the_dataloaders_array_and_the_script_writes_it(takes, tmp_path):
    from scipy.io import wavfile
    for y in takes:
        got = audio.onset_amplitude(y)
        want = ar.onset_amplitude_ref(y)
        assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().astype(np.float64), want)
    y = takes[2]
    frames = ar.onset_detect(y)
    assert len(frames) and np.array_equal(np.flatnonzero(audio.onset_amplitude(y)[:, 1].cpu().numpy()), frames)    # frame numbers as sample indices
    spec = importlib.util.spec_from_file_location("audio_features", os.path.join(REPO, "scripts", "audio_features.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    os.makedirs(tmp_path / "wave16k")
    pcm = np.round(takes[1] * 32767).astype(np.int16)
    wavfile.write(tmp_path / "wave16k" / "a.wav", 16000, pcm)
    wavfile.write(tmp_path / "wave16k" / "b.wav", 16000, takes[2])
    np.save(tmp_path / "wave16k" / "c.npy", takes[0])
    out = script.main([str(tmp_path / "wave16k"), "--out", str(tmp_path / "onset_amplitude"), "--batch", "2"])
    assert out["files"] == 3
    for name, wave in (("a", pcm.astype(np.float32) / 32768.0), ("b", takes[2]), ("c", takes[0])):
        f = np.load(tmp_path / "onset_amplitude" / f"{name}.npy")
        assert f.dtype == np.float64 and np.array_equal(f, ar.onset_amplitude_ref(wave)), name
    os.makedirs(tmp_path / "other")
    wavfile.write(tmp_path / "other" / "a.wav", 22050, takes[1])
    with pytest.raises(SystemExit, match="resampling is out of scope"):
        script.main([str(tmp_path / "other"), "--out", str(tmp_path / "nowhere")])


def test_units_follow_the_frames(takes):
    y = takes[2]
    f = audio.onset_detect(y)
    s, t = audio.onset_detect(y, units="samples"), audio.onset_detect(y, units="time")
    assert s.dtype == np.int64 and np.array_equal(s, f * 512) and t.dtype == np.float64 and np.array_equal(t, f * 512 / 16000.0)
    t22 = audio.onset_detect(y, sr=22050, units="time")
    assert np.array_equal(t22, audio.onset_detect(y, sr=22050) * 512 / 22050.0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "motion_metrics.npz"))


def take_wave(n_pose, extra, seed=6):
    """16 kHz audio for n_pose frames at 30 fps, `extra` samples longer than the motion."""
    return ar.speech_like(seed, int(16000 / 30 * n_pose) + extra)


def test_beat_consistency_from_the_waveform(gold):
    g = gold
    joints_rec, mmae, mask = g["take.joints"], g["take.mmae"], int(g["take.t_start"])
    n = len(joints_rec)
    a_offset = int(mask * (16000 / 30))
    for extra in (40000, 5000, 0):                                          # a file longer than the motion by more than a_offset, by less, not at all
        wave = take_wave(n, extra)
        short = wave[:int(16000 / 30 * n)][a_offset:len(wave) - a_offset]   # trainer lines 681-683 as written
        assert len(short) == min(int(16000 / 30 * n), len(wave) - a_offset) - a_offset
        want_on = ar.onset_detect(short, 16000, 512, units="time")
        assert len(want_on) > 2 and len(ar.unsafe_frames(short)[0]) == 0
        al = metrics.alignment(float(g["take.sigma"]), int(g["take.order"]), mmae)
        got_on = al.load_audio_hip(wave[:int(16000 / 30 * n)], a_offset, len(wave) - a_offset, True)
        assert got_on.dtype == np.float64 and np.array_equal(got_on, want_on)
        want = metrics.beat_consistency(joints_rec, want_on, mmae, align_mask=mask, sigma=float(g["take.sigma"]), order=int(g["take.order"]))
        got = metrics.beat_consistency_from_audio(joints_rec, wave, mmae, align_mask=mask, sigma=float(g["take.sigma"]), order=int(g["take.order"]))
        assert abs(got - want) <= 1e-12
        assert abs(metrics.beat_consistency_from_audio(joints_rec, torch.from_numpy(wave).cuda(), mmae, align_mask=mask, sigma=float(g["take.sigma"]),
                                                       order=int(g["take.order"])) - want) <= 1e-12


def test_results_script_detects_the_onsets_it_is_otherwise_given(gold, tmp_path, capsys):
    from scipy.io import wavfile
    spec = importlib.util.spec_from_file_location("motion_metrics_from_results", os.path.join(REPO, "scripts", "motion_metrics_from_results.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    g, r = gold, np.random.RandomState(12)
    V, K, mask = 20, 300, int(gold["take.t_start"])
    reg = r.rand(55, V)
    reg /= reg.sum(1, keepdims=True)
    model = {"v_template": r.randn(V, 3) * 0.5, "shapedirs": r.randn(V, 3, 400) * 0.01, "J_regressor": reg,
             "hands_meanl": r.randn(45) * 0.2, "hands_meanr": r.randn(45) * 0.2,
             "kintree_table": np.stack([np.concatenate([[2 ** 32 - 1], mr.smplx_parents()[1:]]), np.arange(55)]).astype(np.uint32)}
    np.savez(tmp_path / "model.npz", **model)
    np.save(tmp_path / "mean_vel.npy", g["take.mmae"])
    for d in ("res", "onsets", "waves"):
        os.makedirs(tmp_path / d)
    a_offset = int(mask * (16000 / 30))
    for k, n in enumerate((len(g["take.aa"]), len(g["take.aa"]) - 7)):
        np.savez(tmp_path / "res" / f"res_take{k}.npz", poses=g["take.aa"][:n].reshape(n, 165), trans=np.zeros((n, 3), np.float32), betas=r.randn(K))
        wave = take_wave(n, 3000 * k, seed=8 + k)
        if k:
            np.save(tmp_path / "waves" / f"take{k}.npy", wave)
        else:
            wavfile.write(tmp_path / "waves" / f"take{k}.wav", 16000, wave)
        short = wave[:int(16000 / 30 * n)][a_offset:len(wave) - a_offset]
        assert len(ar.unsafe_frames(short)[0]) == 0
        np.save(tmp_path / "onsets" / f"take{k}.npy", ar.onset_detect(short, units="time"))
    common = [str(tmp_path / "res"), "--smplx-model", str(tmp_path / "model.npz"), "--mean-vel", str(tmp_path / "mean_vel.npy"), "--mask", str(mask)]
    given = script.main(common + ["--onsets", str(tmp_path / "onsets")])
    found = script.main(common + ["--waves", str(tmp_path / "waves")])
    assert found["bc_takes"] == 2 and found == given and found["bc"] is not None
    assert '"bc"' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        script.main(common + ["--onsets", str(tmp_path / "onsets"), "--waves", str(tmp_path / "waves")])
    assert "bc" not in script.main(common)
