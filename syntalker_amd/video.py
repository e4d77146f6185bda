"""The takes as video with sound: a baseline JPEG encoder on the device (csrc/syn_jpeg.inc) and a Motion-JPEG AVI writer with a PCM
sound track on the host - what the reference gets from ffmpeg in `utils/media.py` (`convert_img_to_mp4`, `add_audio_to_video`), as one playable
file per take and without any library.  H.264 / mp4 and OpenDML (files past 2 GB) stay out; the sound track is written
at its own rate (bringing a file to another rate is `syntalker_amd.audio.load_wave`).

The frames `render.render` left on the device are encoded there, by integer rules stated in include/syn_hip.h and restated in tests/jpeg_ref.py
(JFIF colour in 16-bit fixed point, 4:2:0, a 13-bit integer DCT, the Annex K tables scaled by the IJG quality rule, one restart interval per MCU
row), and cross to the host as files of about a fiftieth of the raw size.  `encode_jpeg` synchronises once: the exact size of the output is known
only after the coder has counted it (count first, write second - nothing is sized by a guess).

Device tensors only, like the rest of the package: a CPU tensor or a missing library raises `SynHipError`."""
from __future__ import annotations

import functools
import os
import struct
from fractions import Fraction

import numpy as np
import torch

from . import _lib

MAX_DIM = 8192             # csrc/syn_jpeg.inc kMaxDim
# scan position -> natural (row-major) index of an 8 x 8 block
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
          15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_BASE = ((16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
         (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)


def _ac_values(head):
    """An Annex K AC value list: its irregular head, then every (run, size) symbol not yet named, in ascending order."""
    seen = set(head)
    return tuple(head) + tuple(s for s in range(0x100) if s not in seen and 1 <= (s & 15) <= 10)


_HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D),
     _ac_values((0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
                 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82))),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     _ac_values((0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
                 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1))),
)


def _check_quality(quality):
    if int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"video: quality is an integer from 1 to 100, got {quality!r}")
    return int(quality)


def _check_size(width, height):
    if int(width) != width or int(height) != height or not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM):
        raise ValueError(f"video: width and height are 1 to {MAX_DIM} pixels, got {width} x {height}")
    return int(width), int(height)


def quant_tables(quality: int = 90) -> np.ndarray:
    """(2, 64) int32, natural order: the luminance and chrominance tables of ITU T.81 Annex K.1 scaled by the IJG rule - s = 5000 // quality below 50,
    else 200 - 2 quality; Q = clamp((base s + 50) // 100, 1, 255).  What libjpeg (and PIL) use at the same `quality`."""
    quality = _check_quality(quality)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(_BASE, dtype=np.int64) * s + 50) // 100, 1, 255).astype(np.int32)


def huffman_tables() -> dict:
    """{(class << 4) | id: (bits, values)}: the four tables of Annex K.3 - 0x00 DC luminance, 0x10 AC luminance, 0x01 DC chrominance, 0x11 AC
    chrominance; bits[k] codes of length k + 1, values in code order: a DHT segment's body behind its first byte."""
    return {key: (bits, vals) for key, bits, vals in _HUFFMAN}


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


@functools.lru_cache(maxsize=64)
def jpeg_header(width: int, height: int, quality: int = 90) -> bytes:
    """Everything in front of the entropy data, constant per shape and quality: SOI, JFIF APP0, two DQT, SOF0 (8 bit, three components 0x22 / 0x11 /
    0x11), four DHT, DRI (one MCU row), SOS."""
    width, height = _check_size(width, height)
    q = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for k in range(2):
        out += _segment(0xDB, bytes([k]) + bytes(int(q[k][i]) for i in ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key, bits, vals in _HUFFMAN:
        out += _segment(0xC4, bytes([key]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", (width + 15) // 16))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


@functools.lru_cache(maxsize=16)
def _header_on(device, width, height, quality):
    return torch.frombuffer(bytearray(jpeg_header(width, height, quality)), dtype=torch.uint8).to(device)


def _encode(rgb: torch.Tensor, quality):
    """-> (data, offsets on the device, offsets on the host)."""
    quality = _check_quality(quality)
    if not torch.is_tensor(rgb):
        raise TypeError(f"video: frames are a torch tensor on the device, got {type(rgb).__name__}")
    if rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.dtype != torch.uint8:
        raise ValueError(f"video: frames are (n, H, W, 3) uint8 RGB, got {tuple(rgb.shape)} {rgb.dtype}")
    if not rgb.is_cuda:
        raise _lib.SynHipError(f"video: the frames are on {rgb.device}: the JPEG encoder runs only on the MI355X HIP kernels (no CPU fallback). Encode the "
                               "frames where render.render left them.")
    n, height, width = (int(d) for d in rgb.shape[:3])
    width, height = _check_size(width, height)
    dev = rgb.device
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), np.zeros(1, dtype=np.int64)
    if tuple(rgb.stride()[1:]) != (3 * width, 3, 1) or (n > 1 and rgb.stride(0) < 3 * width * height):
        rgb = rgb.contiguous()                      # frames may lie any distance apart; inside a frame the bytes are dense
    lib, st = _lib.load(), _lib.current_stream(dev)
    ws = torch.empty(lib.syn_jpeg_workspace_bytes(n, width, height), dtype=torch.uint8, device=dev)
    head = _header_on(dev, width, height, quality)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.check(lib.syn_jpeg_transform(rgb.data_ptr(), int(rgb.stride(0)) if n > 1 else 3 * width * height, n, width, height, quality, ws.data_ptr(), st),
               "syn_jpeg_transform")
    _lib.check(lib.syn_jpeg_measure(n, width, height, int(head.numel()), ws.data_ptr(), offsets.data_ptr(), st), "syn_jpeg_measure")
    host = offsets.cpu().numpy()                    # the one synchronisation: the sizes are known only now
    data = torch.empty(int(host[-1]), dtype=torch.uint8, device=dev)
    _lib.check(lib.syn_jpeg_write(n, width, height, head.data_ptr(), int(head.numel()), ws.data_ptr(), offsets.data_ptr(), data.data_ptr(), int(data.numel()), st),
               "syn_jpeg_write")
    return data, offsets, host


def encode_jpeg(rgb: torch.Tensor, quality: int = 90):
    """rgb (n, H, W, 3) uint8 on the device (the frames any distance apart) -> (data uint8, offsets (n + 1,) int64), both on the device: frame k is
    data[offsets[k]:offsets[k + 1]], a complete JPEG file.  A frame's bytes do not depend on what shares the call."""
    data, offsets, _ = _encode(rgb, quality)
    return data, offsets


def jpeg_frames(rgb: torch.Tensor, quality: int = 90) -> list:
    """The frames as a list of `bytes`, each a complete JPEG file: one synchronisation for the offsets, one copy of exactly the bytes used."""
    data, _, host = _encode(rgb, quality)
    raw = data.cpu().numpy().tobytes()
    return [raw[int(host[k]):int(host[k + 1])] for k in range(len(host) - 1)]


def pcm16(wave) -> np.ndarray:
    """A mono waveform as int16 samples: float -> clip(rint(32767 y)), int16 as it is."""
    if torch.is_tensor(wave):
        wave = wave.detach().cpu().numpy()
    y = np.asarray(wave)
    if y.ndim != 1:
        raise ValueError(f"video: the sound track is one channel of samples, got shape {y.shape}")
    if y.dtype == np.int16:
        return np.ascontiguousarray(y)
    if y.dtype.kind != "f":
        raise ValueError(f"video: int16 or float samples, got {y.dtype}")
    return np.clip(np.rint(32767.0 * y.astype(np.float64)), -32768, 32767).astype(np.int16)


def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


class AviWriter:
    """A Motion-JPEG AVI 1.0 file (`hdrl`, `movi`, `idx1`), written as the frames come.  `write(rgb_chunk)` encodes (n, height, width, 3) uint8 device
    frames and appends one `00dc` chunk each; with `wave` (mono, float or int16, at `wave_sr` - written at its own rate, nothing is resampled) a `01wb`
    chunk follows frame k with samples [k sr scale // rate, (k + 1) sr scale // rate), while there are any: the track is cut at the video's end, as
    `add_audio_to_video`'s `-shortest` does, and a shorter track simply ends.  `fps` becomes the rational rate / scale (30 -> 30 / 1, 7.5 -> 15 / 2).
    `close()` writes the index and patches the counts into the header.  A file that would pass MAX_BYTES raises before the chunk that would do it is
    written (OpenDML is out of scope); what was written before stays a valid file once closed.  `encoder(rgb_chunk, quality) -> [bytes]` replaces
    `jpeg_frames` (the host tests build files without a device)."""

    MAX_BYTES = 2 ** 31 - 2 ** 20

    def __init__(self, path, width: int, height: int, fps, wave=None, wave_sr: int = 16000, quality: int = 90, encoder=None):
        self.width, self.height = _check_size(width, height)
        self.quality = _check_quality(quality)
        if not fps > 0:
            raise ValueError(f"AviWriter: fps must be positive, got {fps!r}")
        frac = Fraction(fps).limit_denominator(1001)
        self.rate, self.scale = frac.numerator, frac.denominator
        self.wave = None if wave is None else pcm16(wave)
        self.wave_sr = int(wave_sr)
        if self.wave is not None and self.wave_sr < 1:
            raise ValueError(f"AviWriter: wave_sr must be positive, got {wave_sr!r}")
        self.encoder = jpeg_frames if encoder is None else encoder
        self.frames, self.samples, self.index, self.largest = 0, 0, [], [0, 0]
        self.movi = self.end = 0                     # offsets of the 'movi' fourcc and of idx1: the sizes that hang on them are patched by close()
        self.path = path
        self.file = open(path, "wb")
        self.file.write(self._header())
        self.movi = self.file.tell() - 4             # of the 'movi' fourcc: idx1 offsets count from here
        self.closed = False

    def _header(self):
        streams = 1 if self.wave is None else 2
        avih = struct.pack("<14I", int(round(1e6 * self.scale / self.rate)), 0, 0, 0x10 | (0x100 if streams == 2 else 0), self.frames, 0, streams, self.largest[0],
                           self.width, self.height, 0, 0, 0, 0)
        vids = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, self.frames, self.largest[0], -1, 0, 0, 0, self.width,
                           self.height)
        bmih = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", 3 * self.width * self.height, 0, 0, 0, 0)
        body = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", vids) + _chunk(b"strf", bmih))
        if streams == 2:
            auds = struct.pack("<4s4sIHHIIIIIIiI4h", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, self.wave_sr, 0, self.samples, self.largest[1], -1, 2, 0, 0, 0, 0)
            fmt = struct.pack("<HHIIHH", 1, 1, self.wave_sr, 2 * self.wave_sr, 2, 16)
            body += _chunk(b"LIST", b"strl" + _chunk(b"strh", auds) + _chunk(b"strf", fmt))
        riff = self.end + 16 * len(self.index) if self.end else 4
        head = b"RIFF" + struct.pack("<I", riff) + b"AVI " + _chunk(b"LIST", body)
        return head + b"LIST" + struct.pack("<I", self.end - self.movi if self.end else 4) + b"movi"

    def _append(self, fourcc, payload, flags, stream):
        size = 8 + len(payload) + (len(payload) & 1)
        if self.file.tell() + size + 8 + 16 * (len(self.index) + 1) > self.MAX_BYTES:
            raise ValueError(f"AviWriter: {self.path} would pass {self.MAX_BYTES} bytes after {self.frames} frames; AVI 1.0 ends there (OpenDML is out of "
                             "scope) - close this file and start another")
        self.index.append(struct.pack("<4sIII", fourcc, flags, self.file.tell() - self.movi, len(payload)))
        self.file.write(_chunk(fourcc, payload))
        self.largest[stream] = max(self.largest[stream], len(payload))

    def write_encoded(self, frames):
        """Appends frames that are JPEG files already."""
        if self.closed:
            raise ValueError("AviWriter: the file is closed")
        for jpg in frames:
            self._append(b"00dc", bytes(jpg), 0x10, 0)           # AVIIF_KEYFRAME: every Motion-JPEG frame is one
            k, self.frames = self.frames, self.frames + 1
            if self.wave is not None:
                lo, hi = (min(len(self.wave), j * self.wave_sr * self.scale // self.rate) for j in (k, k + 1))
                if hi > lo:
                    self._append(b"01wb", self.wave[lo:hi].astype("<i2").tobytes(), 0x10, 1)
                    self.samples = hi

    def write(self, rgb_chunk):
        if self.closed:
            raise ValueError("AviWriter: the file is closed")
        if tuple(rgb_chunk.shape[1:]) != (self.height, self.width, 3):
            raise ValueError(f"AviWriter: frames are (n, {self.height}, {self.width}, 3), got {tuple(rgb_chunk.shape)}")
        self.write_encoded(self.encoder(rgb_chunk, self.quality))

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.end = self.file.tell()
        self.file.write(b"idx1" + struct.pack("<I", 16 * len(self.index)) + b"".join(self.index))
        self.file.seek(0)
        self.file.write(self._header())
        self.file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_video(path, frame_chunks, fps, wave=None, wave_sr: int = 16000, quality: int = 90, encoder=None) -> dict:
    """frame_chunks: an iterable of (n, H, W, 3) uint8 device tensors of one size -> the AVI file at `path`.  Returns dict(frames, samples, bytes)."""
    writer = None
    try:
        for chunk in frame_chunks:
            if writer is None:
                writer = AviWriter(path, int(chunk.shape[2]), int(chunk.shape[1]), fps, wave=wave, wave_sr=wave_sr, quality=quality, encoder=encoder)
            writer.write(chunk)
        if writer is None:
            raise ValueError("write_video: no frames")
    finally:
        if writer is not None:
            writer.close()
    return {"frames": writer.frames, "samples": writer.samples, "bytes": os.path.getsize(path)}
