"""The JPEG encoder on the device (csrc/syn_jpeg.inc, syntalker_amd/video.py) against the numpy restatement of tests/jpeg_ref.py, which
test_video_host.py pins to PIL's decoder and tables.  Every rule is integer, so the gate is equality of bytes: there is nothing to tolerate.

Pictures: the set of jpeg_ref.pictures() (each is there for a corner of the coder that test_video_host.py asserts on its stream: DC category 11, AC
category 10, blocks without EOB, three ZRL in a row, stuffed bytes, RST7 -> RST0, DC-only blocks, ragged MCUs, one MCU), and two wide ones of this
file's own, because the entropy kernel takes a row's blocks 64 at a time: 200 x 20 noise (78 blocks a row: two rounds, thousands of bits carried
between them, more words in a round than lanes) and a 400 x 33 ellipse (150 blocks: three rounds, the last one ragged).  No test here needs PIL."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as jr
from tests import render_ref as rr

from syntalker_amd import _lib, render, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PICTURES = dict(jr.pictures(), wide_noise=jr.noise(200, 20, seed=9), wide_ellipse=jr.ellipse(400, 33))
_want = {}


def want(name, quality):
    if (name, quality) not in _want:
        _want[(name, quality)] = jr.encode(PICTURES[name], quality)
    return _want[(name, quality)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return f"{len(a)} bytes against {len(b)}, first difference at {int(d[0]) if len(d) else n}"


@pytest.mark.parametrize("quality", jr.QUALITIES)
@pytest.mark.parametrize("name", sorted(PICTURES))
def test_the_device_writes_the_restatement_s_bytes(name, quality):
    got = video.jpeg_frames(dev(PICTURES[name][None]), quality)
    assert len(got) == 1 and isinstance(got[0], bytes)
    assert got[0] == want(name, quality), first_difference(got[0], want(name, quality))


def test_the_wide_pictures_take_several_rounds_of_64_blocks():
    for name, rounds in (("wide_noise", 2), ("wide_ellipse", 3)):
        blocks = 6 * ((PICTURES[name].shape[1] + 15) // 16)
        assert -(-blocks // 64) == rounds and blocks % 64
    # a row of 78 noise blocks is thousands of bytes: a round of 64 of them fills many times the 64 words (256 bytes) the lanes build at once
    assert (len(want("wide_noise", 100)) - len(video.jpeg_header(200, 20, 100))) // 2 > 16 * 256


def test_a_mixed_batch_is_each_frame_alone():
    batch = np.stack([PICTURES["ellipse65x47"], PICTURES["noise"], PICTURES["colour"], 255 - PICTURES["colour"]])
    data, offsets = video.encode_jpeg(dev(batch), 90)
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and data.is_cuda and offsets.is_cuda and offsets.shape == (5,)
    alone = [video.jpeg_frames(dev(batch[k:k + 1]), 90)[0] for k in range(4)]
    assert alone[:3] == [want("ellipse65x47", 90), want("noise", 90), want("colour", 90)] and alone[3] == jr.encode(batch[3], 90)
    assert offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(a) for a in alone])]).tolist() and data.numel() == sum(len(a) for a in alone)
    assert data.cpu().numpy().tobytes() == b"".join(alone)
    assert video.jpeg_frames(dev(batch), 90) == alone
    # every second frame of a larger tensor: the frames lie two frames apart, nothing is copied
    big = torch.zeros(8, 47, 65, 3, dtype=torch.uint8, device=DEV)
    big[1::2] = 0x5A
    big[::2] = dev(batch)
    assert not big[::2].is_contiguous() and video.jpeg_frames(big[::2], 90) == alone
    # frames that are not dense inside (the left panel of a pair) are gathered first
    pair = torch.cat([dev(batch), dev(batch[::-1].copy())], dim=2)
    assert video.jpeg_frames(pair[:, :, :65], 90) == alone
    # two frames more than 2^31 bytes apart: the frame's place is a 64-bit product
    far = 2 ** 31 + 4096
    buf = torch.empty(far + 47 * 65 * 3, dtype=torch.uint8, device=DEV)
    apart = torch.as_strided(buf, (2, 47, 65, 3), (far, 65 * 3, 3, 1))
    apart[0], apart[1] = dev(batch[1]), dev(batch[2])
    assert video.jpeg_frames(apart, 90) == alone[1:3]
    del apart, buf
    # no frames: nothing is launched
    data, offsets = video.encode_jpeg(dev(batch[:0]), 90)
    assert data.numel() == 0 and offsets.cpu().tolist() == [0] and video.jpeg_frames(dev(batch[:0])) == []


def test_two_chunk_sizes_give_the_same_file(tmp_path):
    base = PICTURES["ellipse65x47"]
    frames = dev(np.stack([np.roll(base, 3 * k, axis=1) for k in range(5)]))
    wave = np.sin(np.arange(3000) / 5.0).astype(np.float32)
    files = []
    for step in (2, 5):
        with video.AviWriter(tmp_path / f"s{step}.avi", 65, 47, 30, wave=wave, wave_sr=16000) as w:
            for c in range(0, 5, step):
                w.write(frames[c:c + step])
        files.append((tmp_path / f"s{step}.avi").read_bytes())
    assert files[0] == files[1]
    avi = jr.read_avi(files[0])
    assert avi["frames"] == [jr.encode(f, 90) for f in frames.cpu().numpy()] and len(avi["audio"]) == 5
    out = video.write_video(tmp_path / "w.avi", [frames[:1], frames[1:]], 30, wave=wave)
    assert out["frames"] == 5 and (tmp_path / "w.avi").read_bytes() == files[0]
    with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
        video.write_video(tmp_path / "c.avi", [frames.cpu()], 30)


@pytest.mark.parametrize("size", [(65, 47), (70, 130)])
def test_rendered_frames_through_the_encoder(size):
    """The small synthetic mesh of the renderer's tests (a sphere, three frames that hang over the borders), drawn and encoded without leaving the device."""
    v, f = rr.uv_sphere(16, 10, (0.1, 1.0, 0.0), 0.7)
    verts = (v[None] + np.asarray([(0.0, 0.0, 0.0), (0.31, -0.2, 0.3), (-0.9, 0.55, -0.2)])[:, None]).astype(np.float32)
    rgb = render.render(render.Scene(f, n_vertices=v.shape[0]), dev(verts), size[0], size[1])
    got = video.jpeg_frames(rgb, 90)
    host = rgb.cpu().numpy()
    assert (host != 255).any() and host.shape == (3, size[1], size[0], 3)
    for k in range(3):
        ref = jr.encode(host[k], 90)
        assert got[k] == ref, (k, first_difference(got[k], ref))


def test_render_from_results_writes_one_video_per_take(tmp_path, capsys):
    from scipy.io import wavfile
    from tests import smplx_mesh_ref as sm
    spec = importlib.util.spec_from_file_location("render_from_results_avi", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts",
                                                                                          "render_from_results.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    np.savez(tmp_path / "model.npz", **sm.synth_model(3, 203))
    for prefix, seed in (("res", 31), ("gt", 32)):
        pose, ex, _, tr = sm.case_inputs(seed, 7, 100, amp=0.1, transl=True)
        np.savez(tmp_path / f"{prefix}_0.npz", poses=pose, expressions=ex, trans=(0.1 * tr + [0.0, 1.0, 0.0]).astype(np.float32), betas=sm.case_inputs(31, 1, 100)[2])
    os.makedirs(tmp_path / "waves")
    wave = (0.8 * np.sin(np.arange(22050) / 11.0)).astype(np.float32)                            # one second; the video is 4 frames at 15 fps
    wavfile.write(tmp_path / "waves" / "0.wav", 22050, wave)
    args = [str(tmp_path), "--smplx-model", str(tmp_path / "model.npz"), "--out", str(tmp_path / "o"), "--gt", "--fps", "15", "--width", "130", "--height", "47",
            "--chunk", "3", "--format", "avi", "--quality", "80", "--waves", str(tmp_path / "waves")]
    out = script.main(args)
    path = str(tmp_path / "o" / "video_0.avi")
    assert out == {"takes": 1, "frames": 4, "width": 130, "height": 47, "out": str(tmp_path / "o"), "videos": [path]}
    printed = capsys.readouterr().out
    assert json.loads(printed.strip().splitlines()[-1]) == out and "ffmpeg" not in printed
    assert os.listdir(tmp_path / "o") == ["video_0.avi"]                                          # no frame files
    with open(path, "rb") as fh:
        avi = jr.read_avi(fh.read())
    assert len(avi["frames"]) == len(render.frame_indices(7, 15)) == 4 and avi["avih"]["total_frames"] == 4
    assert (avi["avih"]["width"], avi["avih"]["height"]) == (130, 47)
    vh, ah = avi["streams"][0][0], avi["streams"][1][0]
    assert (vh["rate"], vh["scale"], vh["length"]) == (15, 1, 4) and ah["rate"] / ah["scale"] == 22050 and ah["length"] == 4 * 22050 // 15
    pcm = np.clip(np.rint(32767.0 * wave.astype(np.float64)), -32768, 32767).astype(np.int16)
    assert np.array_equal(np.frombuffer(b"".join(avi["audio"]), "<i2"), pcm[:4 * 22050 // 15])
    for jpg in avi["frames"]:
        assert jpg.startswith(video.jpeg_header(130, 47, 80)) and jr.stream_stats(jpg)["blocks"] == 6 * 9 * 3
    args[args.index("--waves") + 1] = str(tmp_path / "nowhere")
    with pytest.raises(SystemExit, match="nowhere.*0.wav"):
        script.main(args)
    with pytest.raises(SystemExit, match="--format avi"):
        script.main(args[:-6] + ["--waves", str(tmp_path / "waves")])


def test_native_calls_write_nothing_outside_their_buffers_and_refuse_what_cannot_run():
    batch = np.stack([PICTURES["noise"], PICTURES["colour"], PICTURES["ellipse65x47"]])
    frames = [want("noise", 100), want("colour", 100), want("ellipse65x47", 100)]
    total = sum(len(f) for f in frames)
    lib, st = _lib.load(), _lib.current_stream(torch.device(DEV))
    n, W, H = 3, 65, 47
    nbytes = lib.syn_jpeg_workspace_bytes(n, W, H)
    intervals, mcus = n * 3, n * 3 * 5
    assert nbytes == (mcus * 768 + intervals * 4 + 15) // 16 * 16 + intervals * 8
    assert lib.syn_jpeg_workspace_bytes(0, W, H) == -1 and lib.syn_jpeg_workspace_bytes(n, 0, H) == -1 and lib.syn_jpeg_workspace_bytes(n, W, 8193) == -1
    head = dev(np.frombuffer(video.jpeg_header(W, H, 100), np.uint8).copy())
    rgb = dev(batch)
    # the three buffers the kernels write lie in one arena with 256 bytes of 0x5A before, between and behind them
    sizes = {"ws": nbytes, "off": 8 * (n + 1), "data": total}
    offsets, end = {}, 256
    for name, size in sizes.items():
        offsets[name], end = end, (end + size + 255) // 256 * 256 + 256
    arena = torch.full((end,), 0x5A, dtype=torch.uint8, device=DEV)
    part = {name: arena[o:o + sizes[name]] for name, o in offsets.items()}
    padding = torch.ones(end, dtype=torch.bool, device=DEV)
    for name, o in offsets.items():
        padding[o:o + sizes[name]] = False
    ws, off, data = part["ws"], part["off"].view(torch.int64), part["data"]

    def transform(src=rgb.data_ptr(), stride=3 * W * H, frames=n, w=W, h=H, quality=100, work=ws.data_ptr()):
        return lib.syn_jpeg_transform(src, stride, frames, w, h, quality, work, st)

    def measure(frames=n, w=W, h=H, hb=int(head.numel()), work=ws.data_ptr(), o=off.data_ptr()):
        return lib.syn_jpeg_measure(frames, w, h, hb, work, o, st)

    def write(frames=n, w=W, h=H, hd=head.data_ptr(), hb=int(head.numel()), work=ws.data_ptr(), o=off.data_ptr(), out=data.data_ptr(), capacity=total):
        return lib.syn_jpeg_write(frames, w, h, hd, hb, work, o, out, capacity, st)

    def refused(rc, word):
        assert rc != 0 and word in lib.syn_last_error().decode(), (rc, lib.syn_last_error())

    for call, names in ((transform, ("src", "work")), (measure, ("work", "o")), (write, ("hd", "work", "o", "out"))):
        for name in names:
            refused(call(**{name: None}), "null")
        refused(call(w=0), "8192")
        refused(call(h=8193), "8192")
        refused(call(frames=-1), "negative")
        refused(call(work=ws.data_ptr() + 8), "aligned")
        assert call(frames=0) == 0
    refused(transform(quality=0), "quality")
    refused(transform(quality=101), "quality")
    refused(transform(stride=3 * W * H - 1), "frame_stride")
    refused(measure(hb=-1), "header_bytes")
    refused(write(capacity=-1), "capacity")
    torch.cuda.synchronize()
    assert (arena == 0x5A).all()                                      # nothing ran
    assert transform() == 0 and measure() == 0
    assert write(capacity=total - 1) == 0                             # a buffer one byte short of the counted size: no byte of it is written
    torch.cuda.synchronize()
    assert (data == 0x5A).all() and off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(f) for f in frames])]).tolist()
    assert write() == 0
    torch.cuda.synchronize()
    assert data.cpu().numpy().tobytes() == b"".join(frames)
    assert (arena[padding] == 0x5A).all()                             # no stage wrote a byte outside the workspace it asked for, the offsets or the counted bytes
