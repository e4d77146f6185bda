"""The host side of syntalker_amd/video.py and the numpy restatement of the device's JPEG encoder (tests/jpeg_ref.py), without a GPU.

The oracle is outside this project: PIL's libjpeg gives the quantisation and Huffman tables, decodes every stream of the restatement, and sets the
quality bar (its own encoder at the same `quality` and 4:2:0).  The AVI files are walked chunk by chunk (jpeg_ref.walk_riff / read_avi); no player is
installed, so playback is not checked.

PSNR of PIL's decode against the source, the restatement's stream / PIL's own encode at the same quality and 4:2:0 (dB), measured with this file
(test_quality_is_pil_s_within_half_a_db prints it with -s; PIL 12.2, libjpeg-turbo):
    picture            q 50             q 90             q 100
    ellipse65x47       29.14 / 29.14    41.27 / 41.26    61.11 / 61.49
    ellipse130x160     34.59 / 34.59    46.51 / 46.51    62.46 / 62.81
    ellipse16x16       24.11 / 24.11    37.98 / 37.84    62.21 / 59.20
    colour             38.28 / 38.18    45.26 / 45.18    49.20 / 49.14
The gate is PIL - 0.5 dB: the 13-bit DCT basis and the chroma rounding are where the rules differ from libjpeg's (the largest gap is -0.38 dB, at
quality 100, where every divisor is 1 and the basis' rounding is all that is left)."""
import io
import os
import re
import struct
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_ref as jr

from syntalker_amd import _lib, video

PICTURES = jr.pictures()
_streams = {}


def stream_of(name, quality):
    if (name, quality) not in _streams:
        _streams[(name, quality)] = jr.encode(PICTURES[name], quality)
    return _streams[(name, quality)]


def pil_decode(data):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    return im


def pil_encode(rgb, quality, **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------------------
def dqt_tables(data):
    """{id: 64 values in natural order} from a file's DQT segments."""
    out = {}
    for marker, body in jr.segments(data)[0]:
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                table = np.empty(64, dtype=np.int64)
                table[jr.ZIGZAG] = list(body[1:65])
                out[body[0] & 15], body = table, body[65:]
    return out


@pytest.mark.parametrize("quality", range(1, 101))
def test_quant_tables_are_libjpeg_s(quality):
    ours = video.quant_tables(quality)
    pil = dqt_tables(pil_encode(PICTURES["colour"], quality))
    assert ours.shape == (2, 64) and np.array_equal(ours[0], pil[0]) and np.array_equal(ours[1], pil[1])
    assert np.array_equal(ours, jr.quant_tables(quality))
    if quality in (1, 50, 90, 100):                                   # Image.quantization holds the same tables (in the file's zigzag order or in natural order, by PIL version)
        q = Image.open(io.BytesIO(pil_encode(PICTURES["colour"], quality))).quantization
        for k in range(2):
            assert list(q[k]) in (ours[k].tolist(), ours[k][list(video.ZIGZAG)].tolist())


def test_huffman_tables_are_annex_k_as_pil_writes_them():
    pil = {}
    for marker, body in jr.segments(pil_encode(PICTURES["colour"], 90, optimize=False))[0]:
        if marker == 0xC4:
            while body:
                n = sum(body[1:17])
                pil[body[0]] = (tuple(body[1:17]), tuple(body[17:17 + n]))
                body = body[17 + n:]
    ours = video.huffman_tables()
    assert set(ours) == set(pil) == {0x00, 0x10, 0x01, 0x11}
    for key in ours:
        assert (tuple(ours[key][0]), tuple(ours[key][1])) == pil[key], hex(key)
        assert [list(ours[key][0]), list(ours[key][1])] == [list(x) for x in jr.HUFFMAN[key]], hex(key)


def test_header_is_the_restatement_s_and_says_what_the_frame_is():
    for (w, h), q in (((65, 47), 90), ((16, 16), 50), ((8192, 1), 100)):
        head = video.jpeg_header(w, h, q)
        assert head == jr.header(w, h, q)
        markers = [m for m, _ in jr.segments(head + b"\xff\xd9")[0]]
        assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert stream_of("colour", 90).startswith(video.jpeg_header(65, 47, 90))


# ---- the streams ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", jr.QUALITIES)
@pytest.mark.parametrize("name", sorted(PICTURES))
def test_pil_decodes_every_stream(name, quality):
    rgb = PICTURES[name]
    im = pil_decode(stream_of(name, quality))
    assert im.size == (rgb.shape[1], rgb.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
    stats = jr.stream_stats(stream_of(name, quality))
    assert stats["blocks"] == 6 * ((rgb.shape[0] + 15) // 16) * ((rgb.shape[1] + 15) // 16)
    assert stats["rst"] == (rgb.shape[0] + 15) // 16 - 1


def test_the_pictures_reach_the_corners_of_the_coder():
    """Each picture is in the set for a condition; the stream says whether it still meets it."""
    st = {key: jr.stream_stats(stream_of(*key)) for key in [("squares", 100), ("checkerboard", 100), ("cos77", 50), ("ellipse65x47", 90), ("ellipse130x160", 90),
                                                             ("ellipse16x16", 90)]}
    for key, s in st.items():
        print(key, {k: v for k, v in s.items() if k != "rst_sequence"})
    assert PICTURES["squares"].shape == (48, 64, 3) and st[("squares", 100)]["dc_category"] == 11
    cb = st[("checkerboard", 100)]
    assert PICTURES["checkerboard"].shape == (160, 32, 3)
    assert cb["ac_category"] == 10 and cb["full"] > 0 and cb["rst"] >= 9 and cb["rst_sequence"][:9] == [0, 1, 2, 3, 4, 5, 6, 7, 0] and cb["stuffed"] >= 200
    assert PICTURES["cos77"].shape == (32, 32, 3) and st[("cos77", 50)]["zero_run"] >= 48
    for name, rows in (("ellipse65x47", 3), ("ellipse130x160", 10)):
        s = st[(name, 90)]
        assert s["dc_only"] > 0 and s["rst"] == rows - 1
        assert PICTURES[name].shape[1] % 16                                           # a ragged right MCU
    assert PICTURES["ellipse65x47"].shape[0] % 16                                     # and a ragged bottom row
    one = st[("ellipse16x16", 90)]
    assert one["blocks"] == 6 and one["rst"] == 0
    for quality in jr.QUALITIES:
        assert jr.stream_stats(stream_of("noise", quality))["stuffed"] > 0, quality
    c = PICTURES["colour"].astype(np.int64)
    assert (c[..., 0] != c[..., 1]).any() and (c[..., 1] != c[..., 2]).any() and (c[..., 0] != c[..., 2]).any()


def test_quality_is_pil_s_within_half_a_db():
    """On the smooth pictures PIL's decode of our stream is at least as near the source as PIL's own encode at the same quality and 4:2:0, minus 0.5 dB."""
    rows = []
    for name in ("ellipse65x47", "ellipse130x160", "ellipse16x16", "colour"):
        rgb = PICTURES[name]
        for quality in jr.QUALITIES:
            ours = psnr(np.asarray(pil_decode(stream_of(name, quality))), rgb)
            pil = psnr(np.asarray(pil_decode(pil_encode(rgb, quality, subsampling=2))), rgb)
            size = len(stream_of(name, quality)), len(pil_encode(rgb, quality, subsampling=2))
            rows.append((name, quality, ours, pil, size))
            print(f"psnr {name:15s} q {quality:3d}: ours {ours:6.2f} dB, PIL {pil:6.2f} dB, gap {ours - pil:+.2f} dB; {size[0]} bytes, PIL {size[1]}")
    for name, quality, ours, pil, _ in rows:
        assert ours >= pil - 0.5, (name, quality, ours, pil)


def worst_case_blocks():
    """(64, 64, 3) grey: block (v, u) holds s = 127 where M[v][y] M[u][x] > 0, else -128 - the input that drives coefficient (v, u) furthest."""
    m = jr.dct_matrix()
    img = np.zeros((64, 64), dtype=np.uint8)
    for v in range(8):
        for u in range(8):
            img[8 * v:8 * v + 8, 8 * u:8 * u + 8] = np.where(m[v][:, None] * m[u][None, :] > 0, 255, 0)
    return np.repeat(img[:, :, None], 3, axis=2)


@pytest.mark.parametrize("quality", jr.QUALITIES)
def test_the_rules_fit_int32(quality):
    for rgb in (PICTURES["checkerboard"], worst_case_blocks(), 255 - worst_case_blocks(), np.zeros((16, 16, 3), np.uint8), np.full((16, 16, 3), 255, np.uint8)):
        wide = jr.transform(rgb, quality, np.int64)
        assert np.array_equal(jr.transform(rgb, quality, np.int32), wide)
        assert np.abs(wide).max() <= 1024
    assert jr.encode(PICTURES["checkerboard"], quality, np.int32) == stream_of("checkerboard", quality)
    assert np.abs(jr.dct_matrix()).sum(axis=1).max() == 23168                                   # the bound of include/syn_hip.h: row 0


# ---- AVI --------------------------------------------------------------------------------------------------------------------------------------------
def restatement_encoder(chunk, quality):
    return [jr.encode(np.asarray(f), quality) for f in chunk]


def avi_frames(n=5):
    base = jr.ellipse(65, 47)
    return np.stack([np.roll(base, 3 * k, axis=1) for k in range(n)])


@pytest.mark.parametrize("fps,rate,scale", [(30, 30, 1), (7.5, 15, 2)])
@pytest.mark.parametrize("sound", ["none", "longer", "shorter", "int16"])
def test_avi_walks_clean(tmp_path, fps, rate, scale, sound):
    frames, sr = avi_frames(5), 22050
    want_jpg = restatement_encoder(frames, 90)
    assert any(len(j) & 1 for j in want_jpg) and any(not len(j) & 1 for j in want_jpg)            # a pad byte is exercised, and its absence
    video_samples = 5 * sr * scale // rate
    rng = np.random.default_rng(3)
    wave = {"none": None, "longer": rng.uniform(-1.2, 1.2, video_samples + 777), "shorter": rng.uniform(-1.2, 1.2, video_samples - 1501).astype(np.float32),
            "int16": rng.integers(-32768, 32768, video_samples + 5, dtype=np.int16)}[sound]
    path = tmp_path / "take.avi"
    with video.AviWriter(path, 65, 47, fps, wave=wave, wave_sr=sr, quality=90, encoder=restatement_encoder) as w:
        w.write(frames[:2])
        w.write(frames[2:])
    data = path.read_bytes()
    avi = jr.read_avi(data)                                          # RIFF and LIST sizes, idx1 offsets and lengths: asserted inside
    assert avi["frames"] == want_jpg
    assert avi["avih"]["total_frames"] == 5 and avi["avih"]["us_per_frame"] == round(1e6 * scale / rate)
    assert avi["avih"]["width"] == 65 and avi["avih"]["height"] == 47 and avi["avih"]["flags"] & 0x10
    assert avi["avih"]["streams"] == len(avi["streams"]) == (1 if wave is None else 2)
    vh, vf = avi["streams"][0]
    assert vh["type"] == b"vids" and vh["handler"] == b"MJPG" and (vh["rate"], vh["scale"], vh["length"]) == (rate, scale, 5)
    size, width, height, planes, bits, comp = struct.unpack("<IiiHH4s", vf[:20])
    assert (size, width, height, planes, bits, comp) == (40, 65, 47, 1, 24, b"MJPG") and len(vf) == 40
    assert all(flags & 0x10 for name, flags, _, _ in avi["index"] if name == "00dc")
    assert data[avi["movi"]:avi["movi"] + 4] == b"movi"
    if wave is None:
        assert not avi["audio"] and [n for n, _, _, _ in avi["index"]] == ["00dc"] * 5
        return
    ah, af = avi["streams"][1]
    pcm = wave if wave.dtype == np.int16 else np.clip(np.rint(32767.0 * wave.astype(np.float64)), -32768, 32767).astype(np.int16)
    kept = min(len(pcm), video_samples)
    assert ah["type"] == b"auds" and ah["rate"] / ah["scale"] == sr and ah["length"] == kept and ah["sample_size"] == 2
    assert struct.unpack("<HHIIHH", af) == (1, 1, sr, 2 * sr, 2, 16)
    assert np.array_equal(np.frombuffer(b"".join(avi["audio"]), dtype="<i2"), pcm[:kept])
    names = [n for n, _, _, _ in avi["index"]]
    assert names[0] == "00dc" and all(a == "00dc" for a, b in zip(names, names[1:]) if b == "01wb")     # a sound chunk follows its frame
    for k, payload in enumerate(avi["audio"][:-1]):
        assert len(payload) == 2 * ((k + 1) * sr * scale // rate - k * sr * scale // rate)


def test_avi_chunking_does_not_change_the_file(tmp_path):
    frames, wave = avi_frames(5), np.sin(np.arange(4000) / 7.0)
    files = []
    for step in (1, 5):
        path = tmp_path / f"s{step}.avi"
        with video.AviWriter(path, 65, 47, 30, wave=wave, encoder=restatement_encoder) as w:
            for c in range(0, 5, step):
                w.write(frames[c:c + step])
        files.append(path.read_bytes())
    assert files[0] == files[1]
    out = video.write_video(tmp_path / "v.avi", [frames[:3], frames[3:]], 30, wave=wave, encoder=restatement_encoder)
    assert (tmp_path / "v.avi").read_bytes() == files[0] and out == {"frames": 5, "samples": 5 * 16000 // 30, "bytes": len(files[0])}


def test_avi_refuses_to_pass_two_gigabytes(tmp_path, monkeypatch):
    assert video.AviWriter.MAX_BYTES == 2 ** 31 - 2 ** 20
    frames = avi_frames(4)
    sizes = [len(j) for j in restatement_encoder(frames, 90)]
    path = tmp_path / "big.avi"
    w = video.AviWriter(path, 65, 47, 30, encoder=restatement_encoder)
    room = w.file.tell() + sum(s + (s & 1) + 8 for s in sizes[:2]) + 8 + 16 * 2                  # exactly two frames and their index fit
    monkeypatch.setattr(video.AviWriter, "MAX_BYTES", room)
    w.write(frames[:2])
    at = w.file.tell()
    with pytest.raises(ValueError, match="OpenDML"):
        w.write(frames[2:])
    assert w.file.tell() == at and w.frames == 2                                                 # nothing of the offending chunk was written
    w.close()
    data = path.read_bytes()
    assert len(data) == room and len(jr.read_avi(data)["frames"]) == 2


def test_argument_checks_without_a_device():
    good = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    for call in (video.encode_jpeg, video.jpeg_frames):
        with pytest.raises(_lib.SynHipError, match="no CPU fallback"):
            call(good)
        with pytest.raises(ValueError, match="uint8"):
            call(good.float())
        with pytest.raises(ValueError, match="uint8"):
            call(good[0])
        with pytest.raises(ValueError, match="uint8"):
            call(torch.zeros(1, 16, 16, 4, dtype=torch.uint8))
        with pytest.raises(TypeError):
            call(np.zeros((1, 16, 16, 3), np.uint8))
        for quality in (0, 101, 50.5):
            with pytest.raises(ValueError, match="quality"):
                call(good, quality)
    for quality in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            video.quant_tables(quality)
        with pytest.raises(ValueError, match="quality"):
            video.jpeg_header(16, 16, quality)
    for w, h in ((0, 16), (16, 0), (8193, 16)):
        with pytest.raises(ValueError, match="8192"):
            video.jpeg_header(w, h, 90)
    with pytest.raises(ValueError, match="one channel"):
        video.pcm16(np.zeros((10, 2)))
    with pytest.raises(ValueError, match="int16 or float"):
        video.pcm16(np.zeros(10, dtype=np.int32))


def test_avi_writer_argument_checks(tmp_path):
    with pytest.raises(ValueError, match="fps"):
        video.AviWriter(tmp_path / "a.avi", 16, 16, 0)
    with pytest.raises(ValueError, match="quality"):
        video.AviWriter(tmp_path / "a.avi", 16, 16, 30, quality=0)
    with pytest.raises(ValueError, match="8192"):
        video.AviWriter(tmp_path / "a.avi", 0, 16, 30)
    assert not (tmp_path / "a.avi").exists()
    w = video.AviWriter(tmp_path / "b.avi", 16, 16, 30, encoder=restatement_encoder)
    with pytest.raises(ValueError, match="16, 16, 3"):
        w.write(np.zeros((1, 16, 32, 3), np.uint8))
    w.close()
    with pytest.raises(ValueError, match="closed"):
        w.write(np.zeros((1, 16, 16, 3), np.uint8))
    assert jr.read_avi((tmp_path / "b.avi").read_bytes())["frames"] == []


def test_the_header_declares_the_exports_and_the_abi_version_stays():
    for name in ("syn_jpeg_workspace_bytes", "syn_jpeg_transform", "syn_jpeg_measure", "syn_jpeg_write"):
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTS
    assert _lib.PROTOTYPES["syn_jpeg_workspace_bytes"][0] is _lib.i64
    assert _lib.ABI_VERSION == 9
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert "#define SYN_ABI_VERSION 9 " in text and "count first, write second" in text.lower()
    csrc = os.path.join(os.path.dirname(os.path.dirname(_lib.HEADER_PATH)), "syntalker_amd", "csrc")
    with open(os.path.join(csrc, "syn_kernels.hip")) as f:
        assert '#include "syn_jpeg.inc"' in f.read()
    with open(os.path.join(csrc, "syn_jpeg.inc")) as f:
        inc = f.read()
    assert video.MAX_DIM == int(re.search(r"kMaxDim = (\d+)", inc).group(1))
    # the kernel's constants are the restatement's: the basis, the base tables, the scan order
    numbers = lambda name: [int(x) for x in re.search(name + r"[^=]*= \{([^;]*)\};", inc).group(1).replace("{", " ").replace("}", " ").replace(",", " ").split()]
    assert numbers("kM") == jr.dct_matrix().reshape(-1).tolist()
    assert numbers("kBase") == jr.BASE_LUMA + jr.BASE_CHROMA
    assert [numbers("kScanPos").index(k) for k in range(64)] == jr.ZIGZAG.tolist()
