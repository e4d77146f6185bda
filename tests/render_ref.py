"""The renderer restated in numpy, and small meshes, for test_render_host.py, test_gpu_render.py and scripts/bench_render.py.

`pyrender` is not installed, so nothing can execute the reference's renderer; what syntalker_amd/render.py draws is specified rule by rule in
DESIGN.md §22 and csrc/syn_render.inc, and this module is those rules in plain numpy: fp64 projection and normals (`project_ref`; `project_torch32`
is the same chain in fp32 torch on the CPU, whose error against fp64 is the yardstick E of the GPU gate), coverage in int64 with the top-left rule and
depth in np.float32 in the prescribed order (`rasterize_ref`: meant to be fed xy_sub and z as the device snapped them, then bit-equal), fp64 shading
(`shade_ref`).  It never imports syntalker_amd."""
import numpy as np

SUB = 16
SENTINEL = -2 ** 31
SNAP_LIMIT = 2 ** 30


# ---- camera -----------------------------------------------------------------------------------------------------------------------------------------
def rot_x_pose(angle_deg, ty, tz):
    a = angle_deg * np.pi / 180
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a), ty], [0.0, np.sin(a), np.cos(a), tz], [0.0, 0.0, 0.0, 1.0]])


def camera_pose():
    return rot_x_pose(-2.0, 1.0, 5.0)              # fast_render.py create_pose_camera(-2)


def light_pose():
    return rot_x_pose(-30.0, 0.0, 3.0)             # fast_render.py create_pose_light(-30)


def view_of(pose):
    return np.linalg.inv(np.asarray(pose, dtype=np.float64))[:3]


def light_of(pose):
    z = np.asarray(pose, dtype=np.float64)[:3, 2]
    return z / np.linalg.norm(z)


def world_from_pixels(px, py, depth, pose, width, height, ymag=1.0):
    """The world point that lands on pixel coordinates (px, py) (fractions allowed) `depth` in front of the camera: the inverse of the projection."""
    s = ymag / (height / 2)
    cam = np.stack([(np.asarray(px, dtype=np.float64) - width / 2) * s, (height / 2 - np.asarray(py, dtype=np.float64)) * s,
                    -np.asarray(depth, dtype=np.float64) * np.ones_like(px, dtype=np.float64)], -1)
    pose = np.asarray(pose, dtype=np.float64)
    return cam @ pose[:3, :3].T + pose[:3, 3]


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------------------
def uv_sphere(segments=16, rings=10, centre=(0.0, 0.0, 0.0), radius=1.0):
    """A closed UV sphere, poles on the y axis: segments x (rings - 1) + 2 vertices, 2 segments (rings - 1) faces, wound outwards.  16 x 10: 146
    vertices, 288 faces."""
    v = [(0.0, 1.0, 0.0)]
    for r in range(1, rings):
        th = np.pi * r / rings
        for s in range(segments):
            ph = 2 * np.pi * s / segments
            v.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    f = []
    ring = lambda r, s: 1 + (r - 1) * segments + s % segments
    for s in range(segments):
        f.append((0, ring(1, s + 1), ring(1, s)))
        f.append((len(v) - 1, ring(rings - 1, s), ring(rings - 1, s + 1)))
    for r in range(1, rings - 1):
        for s in range(segments):
            f.append((ring(r, s), ring(r, s + 1), ring(r + 1, s + 1)))
            f.append((ring(r, s), ring(r + 1, s + 1), ring(r + 1, s)))
    return np.asarray(v) * radius + np.asarray(centre, dtype=np.float64), np.asarray(f, dtype=np.int32)


def sphere_pair(segments=16, rings=10, centre=(0.0, 1.0, 0.0), radius=0.3, offset=(0.25, 0.05, 0.0)):
    """Two spheres that run through each other (depth ties along the intersection): 2 x the vertices and faces of `uv_sphere`."""
    v0, f0 = uv_sphere(segments, rings, centre, radius)
    v1, f1 = uv_sphere(segments, rings, np.asarray(centre) + np.asarray(offset), radius)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)]).astype(np.int32)


def quad_faces(flip_second=False):
    """Vertices 0 1 / 3 2 at the corners, split along the diagonal 0 - 2."""
    return np.asarray([[0, 1, 2], [0, 3, 2] if flip_second else [0, 2, 3]], dtype=np.int32)


def vertex_faces_csr(faces, n_vertices):
    """offsets (V + 1), incident: a loop, to pin render.vertex_faces_csr."""
    lists = [[] for _ in range(n_vertices)]
    for f, tri in enumerate(np.asarray(faces)):
        for v in sorted(set(int(i) for i in tri)):
            lists[v].append(f)
    off = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    return off, np.asarray([f for l in lists for f in l], dtype=np.int32)


# ---- project ----------------------------------------------------------------------------------------------------------------------------------------
def snap(x_pix):
    """rint(16 x) as the kernel stores it: SENTINEL where not finite, clamped to +-2^30."""
    s = np.rint(16.0 * np.asarray(x_pix, dtype=np.float64))
    ok = np.isfinite(s)
    return np.where(ok, np.clip(np.where(ok, s, 0), -SNAP_LIMIT, SNAP_LIMIT), SENTINEL).astype(np.int64), ok


def project_ref(vertices, faces, view, width, height, ymag=1.0):
    """fp64.  vertices (n, V, 3) -> xy_sub (n, V, 2) int64, z (n, V), normal (n, V, 3)."""
    v = np.asarray(vertices, dtype=np.float64)
    view = np.asarray(view, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cam = v @ view[:, :3].T + view[:, 3]
        scale = (height / 2) / ymag
        sx, okx = snap(width / 2 + cam[..., 0] * scale)
        sy, oky = snap(height / 2 - cam[..., 1] * scale)
        ok = okx & oky & np.isfinite(cam).all(-1)
        xy = np.where(ok[..., None], np.stack([sx, sy], -1), SENTINEL)
        f = np.asarray(faces, dtype=np.int64)
        p0, p1, p2 = v[:, f[:, 0]], v[:, f[:, 1]], v[:, f[:, 2]]
        cr = np.cross(p1 - p0, p2 - p0)
        cr = np.where((np.isfinite(p0).all(-1) & np.isfinite(p1).all(-1) & np.isfinite(p2).all(-1))[..., None], cr, 0.0)
        nsum = np.zeros_like(v)
        for n in range(len(v)):
            for k in range(3):
                np.add.at(nsum[n], f[:, k], cr[n])
        # (a face that names a vertex twice has a zero cross product: listing it once or twice for that vertex is the same sum)
        length = np.linalg.norm(nsum, axis=-1, keepdims=True)
        normal = np.where((length > 0) & np.isfinite(length), nsum / np.where(length > 0, length, 1.0), 0.0)
    return xy, -cam[..., 2], normal


def project_torch32(vertices, faces, view):
    """z and normal of `project_ref` as plain fp32 torch on the CPU computes them: (z (n, V), normal (n, V, 3)) float32 numpy."""
    import torch
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float32))
    m = torch.as_tensor(np.asarray(view, dtype=np.float32))
    z = -(v @ m[2, :3] + m[2, 3])
    f = torch.as_tensor(np.asarray(faces, dtype=np.int64))
    p0, p1, p2 = v[:, f[:, 0]], v[:, f[:, 1]], v[:, f[:, 2]]
    cr = torch.cross(p1 - p0, p2 - p0, dim=-1)
    nsum = torch.zeros_like(v)
    for k in range(3):
        nsum.index_add_(1, f[:, k], cr)
    normal = nsum / nsum.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    return z.numpy(), normal.numpy()


# ---- raster -----------------------------------------------------------------------------------------------------------------------------------------
def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _threshold(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1


def oriented(xy, tri, width, height):
    """The face's screen triangle with a positive doubled area: ((x0, y0), (x1, y1), (x2, y2), area, order) in Python ints, `order` the face's
    vertices in that order; None for a dropped face (sentinel, outside the guard band of 16 max(W, H) units, zero area)."""
    g = SUB * max(width, height)
    pts = [(int(xy[i, 0]), int(xy[i, 1])) for i in tri]
    for x, y in pts:
        if not (-g <= x <= SUB * width + g and -g <= y <= SUB * height + g):
            return None
    (x0, y0), (x1, y1), (x2, y2) = pts
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if area == 0:
        return None
    order = [int(tri[0]), int(tri[1]), int(tri[2])]
    if area < 0:
        pts[1], pts[2] = pts[2], pts[1]
        order[1], order[2] = order[2], order[1]
        area = -area
    return pts[0], pts[1], pts[2], area, order


def _samples(pts, width, height):
    """The pixels whose samples the triangle's bounding box holds, clipped to the image: (i0, i1, j0, j1) inclusive, or None."""
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    i0, i1 = max(-((-(min(xs) - 8)) // SUB), 0), min((max(xs) - 8) // SUB, width - 1)
    j0, j1 = max(-((-(min(ys) - 8)) // SUB), 0), min((max(ys) - 8) // SUB, height - 1)
    return (i0, i1, j0, j1) if i0 <= i1 and j0 <= j1 else None


def _weights(pts, box):
    """(w0, w1, w2) int64 arrays over the box's samples (rows j, columns i) and the covered mask."""
    (x0, y0), (x1, y1), (x2, y2) = pts
    i0, i1, j0, j1 = box
    px = (SUB * np.arange(i0, i1 + 1, dtype=np.int64) + 8)[None, :]
    py = (SUB * np.arange(j0, j1 + 1, dtype=np.int64) + 8)[:, None]
    w0, w1, w2 = _edge(x1, y1, x2, y2, px, py), _edge(x2, y2, x0, y0, px, py), _edge(x0, y0, x1, y1, px, py)
    cover = (w0 >= _threshold(x1, y1, x2, y2)) & (w1 >= _threshold(x2, y2, x0, y0)) & (w2 >= _threshold(x0, y0, x1, y1))
    return w0, w1, w2, cover


def coverage_count(xy, faces, width, height):
    """How many faces cover each sample of one frame: (H, W) int."""
    count = np.zeros((height, width), dtype=np.int64)
    for tri in np.asarray(faces):
        o = oriented(xy, tri, width, height)
        box = o and _samples(o[:3], width, height)
        if not box:
            continue
        count[box[2]:box[3] + 1, box[0]:box[1] + 1] += _weights(o[:3], box)[3]
    return count


def rasterize_ref(xy_sub, z, faces, width, height, znear=0.05, zfar=100.0):
    """xy_sub (n, V, 2) ints, z (n, V) float32 -> face_id (n, H, W) int32, depth (n, H, W) float32: the rules of csrc/syn_render.inc, the depth
    expression in np.float32, one rounding per operation."""
    xy_sub, z = np.asarray(xy_sub), np.asarray(z, dtype=np.float32)
    n = len(xy_sub)
    face_id = np.full((n, height, width), -1, dtype=np.int32)
    depth = np.full((n, height, width), np.inf, dtype=np.float32)
    near, far = np.float32(znear), np.float32(zfar)
    for k in range(n):
        for f, tri in enumerate(np.asarray(faces)):
            o = oriented(xy_sub[k], tri, width, height)
            box = o and _samples(o[:3], width, height)
            if not box:
                continue
            w0, w1, w2, cover = _weights(o[:3], box)
            if not cover.any():
                continue
            z0, z1, z2 = (z[k, i] for i in o[4])
            area = np.float32(np.int64(o[3]))
            with np.errstate(invalid="ignore", over="ignore"):
                d = ((w0.astype(np.float32) * z0 + w1.astype(np.float32) * z1) + w2.astype(np.float32) * z2) / area
            fid, dep = face_id[k, box[2]:box[3] + 1, box[0]:box[1] + 1], depth[k, box[2]:box[3] + 1, box[0]:box[1] + 1]
            take = cover & (d >= near) & (d <= far) & ((d < dep) | ((d == dep) & (f < fid)))
            fid[take], dep[take] = f, d[take]
    return face_id, depth


# ---- shade ------------------------------------------------------------------------------------------------------------------------------------------
def shade_ref(face_id, xy_sub, normal, faces, light, base=(220 / 255,) * 3, background=(255, 255, 255), ambient=0.3, diffuse=0.7):
    """fp64: the unrounded channel values 255 c of every pixel, (n, H, W, 3) float64 (background: the background bytes).  A test compares
    rint of these to the device's bytes."""
    face_id, xy_sub, normal = np.asarray(face_id), np.asarray(xy_sub), np.asarray(normal, dtype=np.float64)
    n, height, width = face_id.shape
    out = np.empty((n, height, width, 3), dtype=np.float64)
    out[...] = np.asarray(background, dtype=np.float64)
    light, base = np.asarray(light, dtype=np.float64), np.asarray(base, dtype=np.float64)
    for k in range(n):
        for f in np.unique(face_id[k][face_id[k] >= 0]):
            o = oriented(xy_sub[k], np.asarray(faces)[f], width, height)
            jj, ii = np.nonzero(face_id[k] == f)
            (x0, y0), (x1, y1), (x2, y2) = o[:3]
            px, py = SUB * ii.astype(np.int64) + 8, SUB * jj.astype(np.int64) + 8
            b = np.stack([_edge(x1, y1, x2, y2, px, py), _edge(x2, y2, x0, y0, px, py), _edge(x0, y0, x1, y1, px, py)], -1) / float(o[3])
            nn = b @ normal[k, o[4]]
            length = np.linalg.norm(nn, axis=-1)
            ndl = np.where(length > 0, np.maximum(0.0, nn @ light) / np.where(length > 0, length, 1.0), 0.0)
            c = np.minimum(1.0, ambient + diffuse * ndl)
            out[k, jj, ii] = np.clip(255.0 * base[None, :] * c[:, None], 0.0, 255.0)
    return out
