"""A numpy / Python restatement of the stick-figure rasteriser's rules (include/syn_hip.h `syn_plot_*`): the oracle of
tests/test_gpu_plot.py, pinned on hand-counted cases by tests/test_plot_host.py.  It shares no code with syntalker_amd/plot.py beyond the constants it
is handed; fp64 steps are Python floats (IEEE doubles, one rounding per operation), integer steps Python ints or numpy int64."""
import math

import numpy as np

SUB = 16
W_MIN = 0.0625
MAX_R = 4095
GROUND_INTS = 24
EMPTY = (0, 0, 0, 0, -1, 0, 1, 1)


# ---- projection -------------------------------------------------------------------------------------------------------------------------------------
def to_clip(M, p):
    """(x, y, w) of M p: rows 0, 1 and 3, each ((m0 x + m1 y) + m2 z) + m3."""
    x, y, z = (float(c) for c in p)
    return tuple(((float(M[r][0]) * x + float(M[r][1]) * y) + float(M[r][2]) * z) + float(M[r][3]) for r in (0, 1, 3))


def finite(c):
    return all(math.isfinite(v) for v in c)


def cut_w(inside, outside):
    t = _div(inside[2] - W_MIN, inside[2] - outside[2])
    return (inside[0] + t * (outside[0] - inside[0]), inside[1] + t * (outside[1] - inside[1]), W_MIN)


def _div(a, b):
    """IEEE division: inf / nan where Python raises."""
    return float(np.float64(a) / np.float64(b)) if b == 0 or not (math.isfinite(a) and math.isfinite(b)) else a / b


def to_pixel(A, c):
    with np.errstate(all="ignore"):
        u, v = _div(c[0], c[2]), _div(c[1], c[2])
        return (float(A[0][0]) * u + float(A[0][1]) * v) + float(A[0][2]), (float(A[1][0]) * u + float(A[1][1]) * v) + float(A[1][2])


def rint(x):
    return float(np.rint(x))


def pixel_box(xlo, xhi, ylo, yhi, size):
    """The pixels with a sample (16 i + 2 + 4 u) in [lo, hi], clipped to the image: (x0 | x1 << 16, y0 | y1 << 16), (1, 1) when there is none."""
    x0, x1 = max(-((14 - xlo) // 16), 0), min((xhi - 2) // 16, size - 1)
    y0, y1 = max(-((14 - ylo) // 16), 0), min((yhi - 2) // 16, size - 1)
    if x0 > x1 or y0 > y1:
        return 1, 1
    return x0 | x1 << 16, y0 | y1 << 16


def segment_record(M, A, size, p, q, R, layer):
    """The 8 ints of a segment p -> q (3-D points), or EMPTY when it is dropped."""
    if not (1 <= R <= min(MAX_R, SUB * size)):
        return EMPTY
    with np.errstate(all="ignore"):
        ca, cb = to_clip(M, p), to_clip(M, q)
        if not (finite(ca) and finite(cb)) or (ca[2] < W_MIN and cb[2] < W_MIN):
            return EMPTY
        if ca[2] < W_MIN:
            ca = cut_w(cb, ca)
        elif cb[2] < W_MIN:
            cb = cut_w(ca, cb)
        pa, pb = to_pixel(A, ca), to_pixel(A, cb)
        s = [rint(16.0 * v) for v in (*pa, *pb)]
    lo, hi = -SUB * size, 2 * SUB * size
    if not all(lo <= v <= hi for v in s):                               # (a NaN fails)
        return EMPTY
    return snapped_record(*(int(v) for v in s), R, layer, size)


def snapped_record(ax, ay, bx, by, R, layer, size):
    """The record of a segment whose ends are on the grid already: T = isqrt(R^2 L2), -1 for a disc; the pixel box of [min - R, max + R]."""
    L2 = (bx - ax) ** 2 + (by - ay) ** 2
    T = math.isqrt(R * R * L2) if L2 else -1
    box = pixel_box(min(ax, bx) - R, max(ax, bx) + R, min(ay, by) - R, max(ay, by) + R, size)
    return (ax, ay, bx, by, T, R | layer << 16, *box)


def clip_side(pts, axis, bound, keep_above):
    out = []
    for i, a in enumerate(pts):
        b = pts[(i + 1) % len(pts)]
        ia, ib = (a[axis] >= bound, b[axis] >= bound) if keep_above else (a[axis] <= bound, b[axis] <= bound)
        if ia:
            out.append(tuple(a))
        if ia != ib:
            s, e = (a, b) if ia else (b, a)
            t = (bound - s[axis]) / (e[axis] - s[axis])
            other = s[1 - axis] + t * (e[1 - axis] - s[1 - axis])
            out.append((bound, other) if axis == 0 else (other, bound))
    return out


def ground_corners(M, A, size, corners3d):
    """The ground quad (four 3-D corners in order) -> its snapped corners, oriented to a positive doubled area ([] when nothing is left)."""
    with np.errstate(all="ignore"):
        c = [to_clip(M, p) for p in corners3d]
        if not all(finite(v) for v in c):
            return []
        pts = []
        for i in range(4):
            a, b = c[i], c[(i + 1) % 4]
            ia, ib = a[2] >= W_MIN, b[2] >= W_MIN
            if ia:
                pts.append(to_pixel(A, a))
            if ia != ib:
                pts.append(to_pixel(A, cut_w(a, b) if ia else cut_w(b, a)))
    if len(pts) < 3 or not all(math.isfinite(v) for p in pts for v in p):
        return []
    lo, hi = float(-size), float(2 * size)
    for axis in (0, 1):
        pts = clip_side(pts, axis, lo, True)
        if pts:
            pts = clip_side(pts, axis, hi, False)
        if not pts:
            return []
    ilo, ihi = -SUB * size, 2 * SUB * size
    out = []
    for x, y in pts[:9]:
        v = (min(max(int(rint(16.0 * x)), ilo), ihi), min(max(int(rint(16.0 * y)), ilo), ihi))
        if not out or out[-1] != v:
            out.append(v)
    if len(out) > 1 and out[-1] == out[0]:
        out.pop()
    area = sum(out[i][0] * out[(i + 1) % len(out)][1] - out[(i + 1) % len(out)][0] * out[i][1] for i in range(len(out)))
    if len(out) < 3 or area == 0:
        return []
    return out if area > 0 else out[::-1]


def ground_record(M, A, size, corners3d, n_slots_of_frame):
    pts = ground_corners(M, A, size, corners3d) if corners3d is not None else []
    box = (1, 1)
    if pts:
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        box = pixel_box(min(xs), max(xs), min(ys), max(ys), size)
        if box == (1, 1):
            pts = []
    flat = [v for p in pts for v in p]
    return [len(pts), n_slots_of_frame, *box, *flat, *([0] * (GROUND_INTS - 4 - len(flat)))]


def setup_ref(data, trajec, index, bounds, segments, M, A, size, traj_r, n_slots):
    """What syn_plot_setup writes: records (m, n_slots, 8) int32 and grounds (m, 24) int32.  data (m, J, 3) float32 the drawn frames, trajec (n, 2)
    float32, index (m,), bounds (min x, max x, min z, max z) float32, segments (S, 4)."""
    data, trajec, bounds = np.asarray(data, np.float32), np.asarray(trajec, np.float32), np.asarray(bounds, np.float32)
    m, S, J = len(index), len(segments), data.shape[1]
    records = np.empty((m, n_slots, 8), dtype=np.int64)
    records[:] = EMPTY
    grounds = np.zeros((m, GROUND_INTS), dtype=np.int64)
    for f, idx in enumerate(int(k) for k in index):
        if not 0 <= idx < len(trajec):
            grounds[f] = ground_record(M, A, size, None, S)
            ntraj = 0
        else:
            ntraj = min(max(idx - 1, 0), n_slots - S)
            rel = trajec[:ntraj + 1] - trajec[idx]                      # float32, as the reference subtracts
            for w in range(ntraj):
                records[f, w] = segment_record(M, A, size, (rel[w, 0], 0.0, rel[w, 1]), (rel[w + 1, 0], 0.0, rel[w + 1, 1]), traj_r, 1)
            x0, x1, z0, z1 = bounds[0] - trajec[idx, 0], bounds[1] - trajec[idx, 0], bounds[2] - trajec[idx, 1], bounds[3] - trajec[idx, 1]
            grounds[f] = ground_record(M, A, size, [(x0, 0.0, z0), (x0, 0.0, z1), (x1, 0.0, z1), (x1, 0.0, z0)], ntraj + S)
        for k, (ja, jb, layer, R) in enumerate(tuple(int(v) for v in row) for row in segments):
            if 0 <= ja < J and 0 <= jb < J and 2 <= layer < 0x8000:
                records[f, ntraj + k] = segment_record(M, A, size, data[f, ja], data[f, jb], R, layer)
    return records.astype(np.int32), grounds.astype(np.int32)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------
def isqrt(v):
    return math.isqrt(int(v))


def capsule_covers(ax, ay, bx, by, R, T, sx, sy):
    """The rule on arrays (numpy int64) or Python ints: body (0 <= dot <= L2 and |cross| <= T) or a cap."""
    dx, dy, px, py = bx - ax, by - ay, sx - ax, sy - ay
    dot, cross = px * dx + py * dy, dx * py - dy * px
    L2 = dx * dx + dy * dy
    body = (dot >= 0) & (dot <= L2) & (abs(cross) <= T)
    qx, qy = sx - bx, sy - by
    return body | (px * px + py * py <= R * R) | (qx * qx + qy * qy <= R * R)


def _samples(x0, x1, y0, y1):
    """Sample coordinates of the pixels x0 .. x1, y0 .. y1: sx (1, nx, 1, 4), sy (ny, 1, 4, 1) int64."""
    off = 2 + 4 * np.arange(4, dtype=np.int64)
    sx = (SUB * np.arange(x0, x1 + 1, dtype=np.int64))[None, :, None, None] + off[None, None, None, :]
    sy = (SUB * np.arange(y0, y1 + 1, dtype=np.int64))[:, None, None, None] + off[None, None, :, None]
    return sx, sy


def unpack(b):
    return int(b) & 0xffff, int(b) >> 16


def segment_mask(rec, size):
    """(y0, y1, x0, x1, covered (ny, nx, 4, 4) bool) of a record over its pixel box; None for an empty box."""
    ax, ay, bx, by, T, rl, px, py = (int(v) for v in rec)
    (x0, x1), (y0, y1) = unpack(px), unpack(py)
    if x0 > x1:
        return None
    sx, sy = _samples(x0, x1, y0, y1)
    return y0, y1, x0, x1, capsule_covers(ax, ay, bx, by, rl & 0xffff, T, sx, sy)


def edge_threshold(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1


def polygon_covers(pts, sx, sy):
    """A convex polygon with a positive doubled area: every edge value > 0, or = 0 on a top or left edge."""
    inside = np.ones(np.broadcast(sx, sy).shape, dtype=bool)
    for i, (ax, ay) in enumerate(pts):
        bx, by = pts[(i + 1) % len(pts)]
        inside &= (bx - ax) * (sy - ay) - (by - ay) * (sx - ax) >= edge_threshold(ax, ay, bx, by)
    return inside


def draw_ref(records, grounds, colours, size, n_layers=None):
    """What syn_plot_draw paints from the records: (m, size, size, 3) uint8."""
    records, grounds = np.asarray(records), np.asarray(grounds)
    n_layers = len(colours) if n_layers is None else n_layers
    out = np.full((len(records), size, size, 3), 255, dtype=np.int64)
    for f in range(len(records)):
        img = out[f]
        n = int(grounds[f, 0])
        if n >= 3:
            (x0, x1), (y0, y1) = unpack(grounds[f, 2]), unpack(grounds[f, 3])
            pts = [(int(grounds[f, 4 + 2 * i]), int(grounds[f, 5 + 2 * i])) for i in range(n)]
            for ya in range(y0, y1 + 1, 128):                           # in strips: 16 samples a pixel
                yb = min(y1, ya + 127)
                k = polygon_covers(pts, *_samples(x0, x1, ya, yb)).sum(axis=(2, 3))[..., None]
                img[ya:yb + 1, x0:x1 + 1] = (img[ya:yb + 1, x0:x1 + 1] * (32 - k) + 128 * k + 16) >> 5
        mask, layer, touched = np.zeros((size, size, 4, 4), dtype=bool), 0, []

        def flush():
            ya, yb = min(t[0] for t in touched), max(t[1] for t in touched) + 1           # the union of the layer's boxes: nothing else changed
            xa, xb = min(t[2] for t in touched), max(t[3] for t in touched) + 1
            k = mask[ya:yb, xa:xb].sum(axis=(2, 3))[..., None]
            rgb = np.asarray([(int(colours[layer]) >> s) & 255 for s in (0, 8, 16)], dtype=np.int64)
            img[ya:yb, xa:xb] = (img[ya:yb, xa:xb] * (16 - k) + rgb * k + 8) >> 4
            mask[ya:yb, xa:xb] = False
            touched.clear()

        for rec in records[f, :min(int(grounds[f, 1]), records.shape[1])]:
            lay = int(rec[5]) >> 16
            hit = segment_mask(rec, size)
            if hit is None or not 1 <= lay < n_layers:
                continue
            if lay != layer:
                if layer:
                    flush()
                layer = lay
            y0, y1, x0, x1, cov = hit
            mask[y0:y1 + 1, x0:x1 + 1] |= cov
            touched.append((y0, y1, x0, x1))
        if layer:
            flush()
    return out.astype(np.uint8)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def transcribed_prepare(joints):
    """plot_script.py:115-132, line by line."""
    data = joints.copy().reshape(len(joints), -1, 3)
    MINS = data.min(axis=0).min(axis=0)
    MAXS = data.max(axis=0).max(axis=0)
    height_offset = MINS[1]
    data[:, :, 1] -= height_offset
    trajec = data[:, 0, [0, 2]]
    data[..., 0] -= data[:, 0:1, 0]
    data[..., 2] -= data[:, 0:1, 2]
    return data, trajec, MINS, MAXS


def walking_take(n, n_joints, chains, seed=0, step=0.035, turn=0.04, spread=1.0, burst=0):
    """A synthetic take (n, n_joints, 3) float32: a figure whose root walks a turning path (about `step` a frame; a hundred times that in the first
    `burst` frames) while its limbs swing; joints along each chain hang off its first joint, so that every chain is a bent line of plausible length."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    heading = turn * t + 0.3 * np.sin(0.05 * t)
    step = step * np.where(t < burst, 100.0, 1.0)
    root = np.stack([np.cumsum(step * np.sin(heading)), 0.9 + 0.03 * np.sin(0.4 * t), np.cumsum(step * np.cos(heading))], 1)
    j = np.zeros((n, n_joints, 3))
    j[:] = root[:, None]
    for c, chain in enumerate(chains):
        direction = rng.normal(size=3)
        direction[1] = -abs(direction[1]) if c < 2 else abs(direction[1])
        direction /= np.linalg.norm(direction)
        for k in range(1, len(chain)):
            swing = 0.25 * np.sin(0.3 * t + c + 0.5 * k)[:, None] * np.asarray([np.cos(heading), 0 * t, np.sin(heading)]).T
            link = spread * (0.22 if len(chain) > 4 else 0.05) * (direction + swing)
            j[:, chain[k]] = j[:, chain[k - 1]] + link
    return j.astype(np.float32)
