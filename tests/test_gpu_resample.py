"""Audio resampling on the device (csrc/syn_audio_resample.inc, syntalker_amd.audio.resample / load_wave) against the fp64 restatement
tests/resample_ref.py, which test_resample_host.py pins to scipy's polyphase resampler and to analytic sines.  Impulses are compared bit for bit (a
sum of one term has no rounding to argue about: a wrong phase, offset, table layout or end condition is off by O(1)); speech-like takes within the
rounding of an N-term fp64 chain, (N + 2) 2^-53 max |x| max_p sum |H_p|, computed here from the taps; batch mates, file loading and the feature
script exactly."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import audio_features_ref as ar
from tests import resample_ref as rr
from tests.conftest import REPO

from syntalker_amd import _lib, audio

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def bound64(orig, target, x):
    L, M, K, g, h = rr.taps(orig, target)
    return (rr.taps_per_output(L, K) + 2) * EPS * float(np.abs(x).max()) * rr.phase_norm(L, K, h)


@pytest.mark.parametrize("orig,target", rr.PAIRS)
def test_impulses_are_single_taps_bit_for_bit(orig, target):
    L, M, K, g, h = rr.taps(orig, target)
    assert K // L + 1 <= 203                                                 # the widest half-width in input samples: the impulses never share an output
    x = np.zeros(1000, dtype=np.float32)
    spikes = {0: 1.0, 450: 3.0, 999: -2.0}
    for j, a in spikes.items():
        x[j] = a
    n_out = rr.out_length(1000, L, M)
    m = np.arange(n_out, dtype=np.int64)
    want = np.zeros(n_out)
    hits = 0
    for j, a in spikes.items():
        k = m * M - j * L
        ok = np.abs(k) <= K
        assert not (want[ok] != 0).any()
        want[ok] = a * h[k[ok] + K]
        hits += int(ok.sum())
    got64 = audio.resample(x, orig, target, dtype=torch.float64)
    got32 = audio.resample(x, orig, target)
    assert got64.is_cuda and got64.dtype == torch.float64 and got32.dtype == torch.float32 and got64.shape == got32.shape == (n_out,)
    assert hits >= 2 * (K // M) and np.count_nonzero(want) >= 100              # one tap per output in reach of an impulse, nearly all non-zero
    assert np.array_equal(got64.cpu().numpy(), want)
    assert np.array_equal(got32.cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("orig,target", rr.PAIRS)
def test_accuracy_on_speech_like_takes(orig, target):
    L, M, K, g, h = rr.taps(orig, target)
    takes = [ar.speech_like(30 + i, n, sr=orig) for i, n in enumerate((1, 2, M, M + 1, 3000, 22050))]
    got64 = audio.resample(takes, orig, target, dtype=torch.float64)        # all takes of the pair in ONE call
    got32 = audio.resample(takes, orig, target)
    assert isinstance(got64, list) and len(got64) == len(got32) == len(takes)
    for x, g64, g32 in zip(takes, got64, got32):
        want = rr.resample(x, orig, target)
        b = bound64(orig, target, x)
        e64 = np.abs(g64.cpu().numpy() - want).max()
        e32 = np.abs(g32.double().cpu().numpy() - want)
        print(f"{orig} -> {target}, {len(x)} samples: fp64 max |delta| {e64:.3e} (bound {b:.3e}), fp32 {e32.max():.3e}")
        assert g64.shape == g32.shape == want.shape == (-(-len(x) * L // M),)
        assert e64 <= b
        assert (e32 <= b + 2.0 ** -24 * np.abs(want)).all()


@pytest.mark.parametrize("orig,target", ((22050, 16000), (48000, 16000), (16000, 22050)))
def test_a_take_does_not_depend_on_its_batch_mates(orig, target):
    r = np.random.RandomState(9)
    loud_a, loud_b = (1e3 * r.randn(700)).astype(np.float32), (1e3 * r.randn(300)).astype(np.float32)
    small = np.array([0.5, -0.25, 0.125, 0.75, -1.0], dtype=np.float32)
    for dtype in (torch.float64, torch.float32):
        alone = audio.resample(small, orig, target, dtype=dtype)
        mates = audio.resample([loud_a, small, loud_b], orig, target, dtype=dtype)
        back = audio.resample([loud_b, small, loud_a], orig, target, dtype=dtype)
        assert torch.equal(mates[1], alone) and torch.equal(back[1], alone)
        assert torch.equal(mates[0], back[2]) and torch.equal(mates[2], back[0])
        assert torch.equal(mates[0], audio.resample(torch.from_numpy(loud_a).cuda(), orig, target, dtype=dtype))
    want = rr.resample(small, orig, target)                                  # a read across a take boundary would be off by 1e3
    got = audio.resample([loud_a, small, loud_b], orig, target, dtype=torch.float64)[1].cpu().numpy()
    assert got.shape == want.shape and np.abs(got - want).max() <= bound64(orig, target, small)


def test_indices_past_2_to_the_31_on_a_general_ratio():
    """22050 -> 16001: L = 16001 (a 2.98 M-entry table, under the cap), and m M passes 2^31 at m = 97391 of a 6.2 s take."""
    orig, target = 22050, 16001
    L, M, K, g, h = rr.taps(orig, target)
    x = ar.speech_like(40, int(6.2 * orig), sr=orig)
    n_out = rr.out_length(len(x), L, M)
    cross = 2 ** 31 // M
    assert L == 16001 and (n_out - 1) * M > 2 ** 31 and cross + 1000 < n_out
    which = np.concatenate([np.arange(cross - 1000, cross + 1000), np.arange(n_out - 2000, n_out)]).astype(np.int64)
    want = rr.resample(x, orig, target, outputs=which)
    got = audio.resample(x, orig, target, dtype=torch.float64)
    assert got.shape == (n_out,)
    err = np.abs(got.cpu().numpy()[which] - want).max()
    print(f"22050 -> 16001, {len(x)} samples, outputs around m = {cross} and the last 2000: max |delta| {err:.3e} (bound {bound64(orig, target, x):.3e})")
    assert np.abs(want).max() > 0.05 and err <= bound64(orig, target, x)
    assert torch.equal(audio.resample(x, orig, target), got.float())


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", f"{name}.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_files_at_other_rates_through_load_wave_and_the_feature_script(tmp_path):
    from scipy.io import wavfile
    os.makedirs(tmp_path / "waves")
    a22 = np.round(ar.speech_like(50, 22050, sr=22050) * 32767).astype(np.int16)
    b48 = ar.speech_like(51, 40000, sr=48000)
    c16 = ar.speech_like(52, 9000)
    wavfile.write(tmp_path / "waves" / "a.wav", 22050, a22)
    wavfile.write(tmp_path / "waves" / "b.wav", 48000, b48)
    wavfile.write(tmp_path / "waves" / "c.wav", 16000, c16)
    a = audio.load_wave(str(tmp_path / "waves" / "a.wav"))
    b = audio.load_wave(str(tmp_path / "waves" / "b.wav"))
    c = audio.load_wave(str(tmp_path / "waves" / "c.wav"))
    assert a.is_cuda and a.dtype == torch.float32 and a.shape == (16000,) and b.shape == (-(-40000 // 3),)
    assert torch.equal(a, audio.resample(a22.astype(np.float32) / 32768.0, 22050, 16000)) and torch.equal(b, audio.resample(b48, 48000, 16000))
    assert torch.equal(c.cpu(), torch.from_numpy(c16))                        # a file at the rate asked for: its samples
    via = audio.load_wave(str(tmp_path / "waves" / "b.wav"), via=22050)
    assert torch.equal(via, audio.resample(audio.resample(b48, 48000, 22050), 22050, 16000)) and not torch.equal(via, b)
    assert torch.equal(audio.load_wave(str(tmp_path / "waves" / "a.wav"), via=22050), a)         # already at 22050: one step
    many = audio.load_waves([str(tmp_path / "waves" / f"{n}.wav") for n in "abc"])
    assert all(torch.equal(p, q) for p, q in zip(many, (a, b, c)))
    script = load_script("audio_features")
    out = script.main([str(tmp_path / "waves"), "--out", str(tmp_path / "onset_amplitude"), "--resample", "--batch", "3"])
    assert out["files"] == 3 and out["samples"] == 16000 + b.numel() + 9000
    for name, wave in (("a", a), ("b", b), ("c", c)):
        w = wave.cpu().numpy()                                               # the device's own resampled samples: the onset chain on identical input
        assert len(ar.unsafe_frames(w)[0]) == 0
        f = np.load(tmp_path / "onset_amplitude" / f"{name}.npy")
        assert f.dtype == np.float64 and np.array_equal(f, ar.onset_amplitude_ref(w)), name
    script.main([str(tmp_path / "waves"), "--out", str(tmp_path / "via"), "--resample", "--via", "22050", "--batch", "2"])
    assert np.array_equal(np.load(tmp_path / "via" / "b.npy"), audio.onset_amplitude(via).double().cpu().numpy())
    with pytest.raises(SystemExit, match="resampling is out of scope"):
        script.main([str(tmp_path / "waves"), "--out", str(tmp_path / "nowhere")])


def test_results_script_takes_waves_at_another_rate(tmp_path):
    """motion_metrics_from_results.py --waves DIR --resample on a 44.1 kHz file prints the `bc` it prints for the onsets of `load_wave`'s 16 kHz wave;
    without the flag the file is refused as before."""
    from scipy.io import wavfile
    from tests import motion_metrics_ref as mr
    from tests.conftest import GOLDEN
    from syntalker_amd import metrics
    g, r = np.load(os.path.join(GOLDEN, "motion_metrics.npz")), np.random.RandomState(12)
    V, mask, n = 20, int(g["take.t_start"]), len(g["take.aa"])
    reg = r.rand(55, V)
    reg /= reg.sum(1, keepdims=True)
    model = {"v_template": r.randn(V, 3) * 0.5, "shapedirs": r.randn(V, 3, 400) * 0.01, "J_regressor": reg,
             "hands_meanl": r.randn(45) * 0.2, "hands_meanr": r.randn(45) * 0.2,
             "kintree_table": np.stack([np.concatenate([[2 ** 32 - 1], mr.smplx_parents()[1:]]), np.arange(55)]).astype(np.uint32)}
    np.savez(tmp_path / "model.npz", **model)
    np.save(tmp_path / "mean_vel.npy", g["take.mmae"])
    for d in ("res", "onsets", "waves"):
        os.makedirs(tmp_path / d)
    np.savez(tmp_path / "res" / "res_take0.npz", poses=g["take.aa"].reshape(n, 165), trans=np.zeros((n, 3), np.float32), betas=r.randn(300))
    wavfile.write(tmp_path / "waves" / "take0.wav", 44100, ar.speech_like(8, int(44100 / 30 * n) + 5000, sr=44100))
    wave16 = audio.load_wave(str(tmp_path / "waves" / "take0.wav"))
    short = metrics.audio_slice_of_test(wave16, n, mask, 16000, 30.0)
    assert len(ar.unsafe_frames(short.cpu().numpy())[0]) == 0
    onsets = audio.onset_detect(short, units="time")
    assert len(onsets) > 2
    np.save(tmp_path / "onsets" / "take0.npy", onsets)
    script = load_script("motion_metrics_from_results")
    common = [str(tmp_path / "res"), "--smplx-model", str(tmp_path / "model.npz"), "--mean-vel", str(tmp_path / "mean_vel.npy"), "--mask", str(mask)]
    given = script.main(common + ["--onsets", str(tmp_path / "onsets")])
    found = script.main(common + ["--waves", str(tmp_path / "waves"), "--resample"])
    assert found["bc_takes"] == 1 and found == given and found["bc"] is not None
    with pytest.raises(ValueError, match="resampling is out of scope"):
        script.main(common + ["--waves", str(tmp_path / "waves")])


def test_c_abi_refusals_leave_the_output_untouched():
    lib = _lib.load()
    dev = torch.device("cuda")
    L, M, K, h = audio.resample_taps(48000, 16000)
    taps = torch.from_numpy(audio.pack_taps(L, M, K, h)).to(dev)
    y = torch.ones(64, device=dev)
    soff, ooff = torch.tensor([0, 64], device=dev), torch.tensor([0, 22], device=dev)
    out32 = torch.full((64,), float("nan"), device=dev)
    out64 = torch.full((65,), float("nan"), dtype=torch.float64, device=dev)
    s = _lib.current_stream(dev)
    good = dict(y=y.data_ptr(), soff=soff.data_ptr(), ooff=ooff.data_ptr(), n_takes=1, max_samples=64, up=1, down=3, taps=taps.data_ptr(), n_taps=taps.numel(),
                out32=out32.data_ptr(), out64=out64.data_ptr())
    cases = [({"y": None}, "null"), ({"soff": None}, "null"), ({"ooff": None}, "null"), ({"taps": None}, "null"), ({"out32": None, "out64": None}, "null"),
             ({"n_takes": 0}, "takes"), ({"up": 0}, "at least 1"), ({"down": 0}, "at least 1"), ({"down": -3}, "at least 1"),
             ({"up": 2, "down": 4, "n_taps": 4 * (taps.numel() // 2)}, "coprime"), ({"n_taps": -1}, "negative"), ({"n_taps": taps.numel() - 1}, "table size"),
             ({"taps": taps.data_ptr() + 8}, "misaligned"), ({"out64": out64.data_ptr() + 4}, "misaligned"), ({"max_samples": 0}, "max_samples")]
    for change, word in cases:
        k = dict(good, **change)
        rc = lib.syn_audio_resample(k["y"], k["soff"], k["ooff"], k["n_takes"], k["max_samples"], k["up"], k["down"], k["taps"], k["n_taps"], k["out32"],
                                    k["out64"], s)
        msg = lib.syn_last_error().decode()
        assert rc != 0 and "syn_audio_resample" in msg and word in msg, (change, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out32).all()) and bool(torch.isnan(out64).all())
    k = good                                                                  # and the same operands, unchanged, are accepted: both outputs at once
    _lib.check(lib.syn_audio_resample(k["y"], k["soff"], k["ooff"], 1, 64, 1, 3, k["taps"], k["n_taps"], k["out32"], k["out64"], s), "syn_audio_resample")
    want = rr.resample(np.ones(64), 48000, 16000)
    assert np.array_equal(out64[:22].cpu().numpy(), want) and np.array_equal(out32[:22].cpu().numpy(), want.astype(np.float32))
    assert bool(torch.isnan(out32[22:]).all()) and bool(torch.isnan(out64[22:]).all())     # exactly ceil(64 / 3) values, nothing else
