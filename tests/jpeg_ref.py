"""The baseline JPEG encoder of include/syn_hip.h restated in numpy, a RIFF chunk walker for the AVI files of syntalker_amd/video.py, a
reader of an encoded stream's statistics, and the test pictures.  Not a test file: test_video_host.py pins it (PIL decodes every stream; the tables
are PIL's), test_gpu_video.py holds the device to it byte for byte.

Everything is integer.  `dtype` is the integer type the transform runs in: the rules fit int32 (|S M^T| <= 128 * 23168 < 3.0e6, |T| <= 1448,
|F| <= 1448 * 23168 < 3.4e7, |F| + (Q << 14) < 3.8e7), which the host tests check by running both widths."""
import struct

import numpy as np

# scan position -> natural (row-major) index of an 8 x 8 block
ZIGZAG = np.asarray([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
                     50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (class << 4 | id) -> (BITS: codes of each length 1 .. 16, HUFFVAL), ITU T.81 Annex K.3
HUFFMAN = {
    0x00: ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    0x10: ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], list(_AC_LUMA_VALS)),
    0x01: ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    0x11: ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(_AC_CHROMA_VALS)),
}


def dct_matrix():
    """M[u][x] = rint(8192 * 1/2 * c(u) * cos((2 x + 1) u pi / 16)), int64 (8, 8)."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
    return np.rint(8192.0 * 0.5 * c * np.cos((2 * x + 1) * u * np.pi / 16.0)).astype(np.int64)


def quant_tables(quality):
    """(2, 64) luminance and chrominance divisors in natural order, IJG scaling."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((np.asarray(b, dtype=np.int64) * s + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)])


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of a BITS / HUFFVAL pair (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def header(width, height, quality):
    """SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI, SOS."""
    q = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for k in range(2):
        out += _segment(0xDB, bytes([k]) + bytes(int(v) for v in q[k][ZIGZAG]))
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key in (0x00, 0x10, 0x01, 0x11):
        bits, vals = HUFFMAN[key]
        out += _segment(0xC4, bytes([key]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", (width + 15) // 16))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def _blocks(plane):
    """(h, w) -> (h / 8, w / 8, 8, 8)."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def transform(rgb, quality=90, dtype=np.int64):
    """(H, W, 3) uint8 -> quantised coefficients (mcu_rows, mcu_cols, 6, 64) in scan order: four Y blocks (row-major in the MCU), Cb, Cr."""
    rgb = np.asarray(rgb)
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.dtype == np.uint8
    h, w = rgb.shape[:2]
    p = np.pad(rgb, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge").astype(dtype)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    m = dct_matrix().astype(dtype)
    q = quant_tables(quality).astype(dtype)

    def coefficients(plane, table):
        s = _blocks(plane - 128)
        t = (s @ m.T + 1024) >> 11
        f = m @ t
        assert f.dtype == dtype and t.dtype == dtype
        d = table.reshape(8, 8)
        qf = np.sign(f) * ((np.abs(f) + (d << 14)) // (d << 15))
        return qf.reshape(qf.shape[0], qf.shape[1], 64)[..., ZIGZAG]

    yq, cbq, crq = coefficients(y, q[0]), coefficients(half(cb), q[1]), coefficients(half(cr), q[1])
    rows, cols = p.shape[0] // 16, p.shape[1] // 16
    out = np.empty((rows, cols, 6, 64), dtype=np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, :, k] = yq[dy::2, dx::2]
    out[:, :, 4], out[:, :, 5] = cbq, crq
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    """(category, extra bits) of a non-zero difference or coefficient."""
    size = int(abs(v)).bit_length()
    return size, v if v > 0 else v + (1 << size) - 1


def entropy(coefs):
    """(mcu_rows, mcu_cols, 6, 64) -> the stuffed bytes of each restart interval (one MCU row)."""
    codes = {key: huffman_codes(*HUFFMAN[key]) for key in HUFFMAN}
    out = []
    for row in coefs:
        w, pred = _Bits(), [0, 0, 0]
        for mcu in row:
            for k, block in enumerate(mcu):
                comp = max(0, k - 3)
                dc, ac = codes[0x00 if comp == 0 else 0x01], codes[0x10 if comp == 0 else 0x11]
                d = int(block[0]) - pred[comp]
                pred[comp] = int(block[0])
                if d == 0:
                    w.put(*dc[0])
                else:
                    size, extra = _magnitude(d)
                    w.put(*dc[size])
                    w.put(extra, size)
                run = 0
                for v in block[1:]:
                    v = int(v)
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        w.put(*ac[0xF0])
                        run -= 16
                    size, extra = _magnitude(v)
                    w.put(*ac[(run << 4) | size])
                    w.put(extra, size)
                    run = 0
                if run:
                    w.put(*ac[0x00])
        out.append(w.finish())
    return out


def encode(rgb, quality=90, dtype=np.int64):
    """(H, W, 3) uint8 -> one complete JPEG file."""
    h, w = np.asarray(rgb).shape[:2]
    parts = entropy(transform(rgb, quality, dtype))
    body = b"".join(part + (bytes([0xFF, 0xD0 + (k & 7)]) if k + 1 < len(parts) else b"\xff\xd9") for k, part in enumerate(parts))
    return header(w, h, quality) + body


# ---- what an encoded stream holds -------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, body)] of the file's header up to and including SOS, and the offset of the entropy data."""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF
        marker, (size,) = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])
        out.append((marker, data[pos + 4:pos + 2 + size]))
        pos += 2 + size
        if marker == 0xDA:
            return out, pos


def stream_stats(data):
    """Decodes the symbols of a file made by `encode` (the layout above, the Annex K tables) and returns dict(dc_category, ac_category: the largest
    of each; zero_run: the longest run of zero coefficients in front of a non-zero one; dc_only: blocks with no non-zero AC coefficient; full: blocks whose
    coefficient 63 is non-zero (no EOB); stuffed: 0xFF 0x00 pairs; rst: RST markers, rst_sequence: their numbers in order; blocks)."""
    segs, pos = segments(data)
    sof = [b for m, b in segs if m == 0xC0][0]
    height, width = struct.unpack(">HH", sof[1:5])
    (dri,) = struct.unpack(">H", [b for m, b in segs if m == 0xDD][0])
    rows, cols = (height + 15) // 16, (width + 15) // 16
    assert dri == cols and data[-2:] == b"\xff\xd9"
    decode = {key: {(length, code): sym for sym, (code, length) in huffman_codes(*HUFFMAN[key]).items()} for key in HUFFMAN}
    st = dict(dc_category=0, ac_category=0, zero_run=0, dc_only=0, full=0, stuffed=0, rst=0, rst_sequence=[], blocks=0)
    for row in range(rows):
        end = pos
        while not (data[end] == 0xFF and data[end + 1] != 0):
            end += 2 if data[end] == 0xFF else 1
        raw = data[pos:end]
        st["stuffed"] += raw.count(b"\xff\x00")
        bits = "".join(f"{b:08b}" for b in raw.replace(b"\xff\x00", b"\xff"))
        at = 0

        def symbol(table):
            nonlocal at
            for length in range(1, 17):
                sym = table.get((length, int(bits[at:at + length], 2)))
                if sym is not None:
                    at += length
                    return sym
            raise AssertionError("no Huffman code matches")

        for _ in range(cols):
            for k in range(6):
                size = symbol(decode[0x00 if k < 4 else 0x01])
                at += size
                st["dc_category"] = max(st["dc_category"], size)
                n, zeros, any_ac = 1, 0, False
                while n < 64:
                    rs = symbol(decode[0x10 if k < 4 else 0x11])
                    if rs == 0:
                        break
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        assert rs == 0xF0
                        n, zeros = n + 16, zeros + 16
                        continue
                    st["zero_run"] = max(st["zero_run"], zeros + run)
                    at += size
                    n, zeros, any_ac = n + run + 1, 0, True
                    st["ac_category"] = max(st["ac_category"], size)
                    if n == 64:
                        st["full"] += 1
                assert n <= 64
                st["dc_only"] += not any_ac
                st["blocks"] += 1
        assert len(bits) - at < 8 and set(bits[at:]) <= {"1"}, "an interval ends in 1-bits inside its last byte"
        pos = end + 2
        if row + 1 < rows:
            assert 0xD0 <= data[end + 1] <= 0xD7
            st["rst"] += 1
            st["rst_sequence"].append(data[end + 1] - 0xD0)
        else:
            assert data[end + 1] == 0xD9 and pos == len(data)
    return st


# ---- RIFF ---------------------------------------------------------------------------------------------------------------------------------------
def walk_riff(data):
    """The chunk tree of a RIFF file: [(fourcc, offset of the chunk's header, payload bytes | children)], a LIST / RIFF node being (fourcc + ':' + type,
    offset, [children]).  Asserts that every size stays inside its parent, that odd chunks are padded and that the RIFF size is the file's."""
    def chunks(lo, hi):
        out = []
        while lo < hi:
            assert lo + 8 <= hi, "a chunk header runs past its parent"
            four, (size,) = data[lo:lo + 4], struct.unpack("<I", data[lo + 4:lo + 8])
            assert lo + 8 + size <= hi, (four, lo, size, hi)
            if four in (b"RIFF", b"LIST"):
                out.append((four.decode() + ":" + data[lo + 8:lo + 12].decode(), lo, chunks(lo + 12, lo + 8 + size)))
            else:
                out.append((four.decode(), lo, data[lo + 8:lo + 8 + size]))
            lo += 8 + size + (size & 1)
        assert lo == hi or lo == hi + 1
        return out
    tree = chunks(0, len(data))
    assert len(tree) == 1 and tree[0][0] == "RIFF:AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    return tree[0][2]


def read_avi(data):
    """dict(avih, streams: [(strh, strf)], frames: [bytes], audio: [bytes], index: [(fourcc, flags, offset, size)], movi: offset of the 'movi' fourcc),
    every field unpacked, every index entry checked against the chunk it points to."""
    top = walk_riff(data)
    names = [n for n, _, _ in top]
    assert names == ["LIST:hdrl", "LIST:movi", "idx1"], names
    hdrl, movi, idx = top[0][2], top[1], top[2][2]
    assert hdrl[0][0] == "avih" and len(hdrl[0][2]) == 56
    avih = dict(zip(("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams", "buffer", "width", "height"),
                    struct.unpack("<10I", hdrl[0][2][:40])))
    streams = []
    for name, _, kids in hdrl[1:]:
        assert name == "LIST:strl" and [k[0] for k in kids] == ["strh", "strf"] and len(kids[0][2]) == 56
        h = kids[0][2]
        strh = dict(type=h[0:4], handler=h[4:8], **dict(zip(("flags", "priority", "initial_frames", "scale", "rate", "start", "length", "buffer", "quality",
                                                             "sample_size"), struct.unpack("<IIIIIIIIiI", h[8:48]))))
        streams.append((strh, kids[1][2]))
    movi_at = movi[1] + 8
    frames = [c[2] for c in movi[2] if c[0] == "00dc"]
    audio = [c[2] for c in movi[2] if c[0] == "01wb"]
    assert len(idx) % 16 == 0 and len(idx) // 16 == len(movi[2])
    index = []
    for k, (name, at, payload) in enumerate(movi[2]):
        four, flags, off, size = struct.unpack("<4sIII", idx[16 * k:16 * k + 16])
        assert four.decode() == name and movi_at + off == at and size == len(payload), (k, name, off, at - movi_at, size, len(payload))
        index.append((name, flags, off, size))
    return dict(avih=avih, streams=streams, frames=frames, audio=audio, index=index, movi=movi_at)


# ---- the test pictures ------------------------------------------------------------------------------------------------------------------------------
def ellipse(width, height):
    """A grey ellipse with a smooth shade on white: what a rendered take looks like."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = (x - 0.5 * (width - 1)) / (0.36 * width), (y - 0.5 * (height - 1)) / (0.42 * height)
    shade = np.clip(220.0 * (0.3 + 0.7 * np.sqrt(np.clip(1.0 - u * u - v * v, 0.0, 1.0)) * (0.8 + 0.2 * u)), 0, 255)
    grey = np.where(u * u + v * v < 1.0, np.rint(shade), 255.0).astype(np.uint8)
    return np.repeat(grey[:, :, None], 3, axis=2)


def squares():
    y, x = np.mgrid[0:48, 0:64]
    return np.repeat(((((x // 8) + (y // 8)) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def checkerboard():
    y, x = np.mgrid[0:160, 0:32]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def cos77():
    k = np.arange(32)
    c = np.cos((2 * (k % 8) + 1) * 7 * np.pi / 16.0)
    return np.repeat(np.rint(128.0 + 100.0 * c[:, None] * c[None, :]).astype(np.uint8)[:, :, None], 3, axis=2)


def noise(width=65, height=47, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def colour(width=65, height=47):
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    r = 128 + 100 * np.sin(x / 9.0) * np.cos(y / 13.0)
    g = 40 + 180 * (x + y) / (width + height)
    b = 200 - 150 * np.exp(-((x - width / 3.0) ** 2 + (y - height / 2.0) ** 2) / 300.0)
    return np.rint(np.clip(np.stack([r, g, b], axis=2), 0, 255)).astype(np.uint8)


def pictures():
    """{name: (H, W, 3) uint8}: the set of the issue, each with the condition test_video_host.py asserts on its stream."""
    return {"squares": squares(), "checkerboard": checkerboard(), "cos77": cos77(), "ellipse65x47": ellipse(65, 47), "ellipse130x160": ellipse(130, 160),
            "ellipse16x16": ellipse(16, 16), "noise": noise(), "colour": colour()}


QUALITIES = (50, 90, 100)
