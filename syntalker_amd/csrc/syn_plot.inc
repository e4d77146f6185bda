// Stick figures of h3d takes (DESIGN.md §26): the scene of the reference's utils/plot_script.py:86-177 - one perspective camera, one translucent ground
// rectangle, the root's past trajectory and 5 or 15 polylines of given colour and width - as a software rasteriser of thick lines.  fp64 up to the
// 1/16-pixel grid, integers behind it, no atomics of any kind, nothing allocated; a frame's bytes depend on the take's trajectory, that frame's joints
// and its index alone, so they do not depend on which frames share the call.
//
//   setup   k_plot_setup: a thread per (frame, slot) writes a 32-byte record {ax, ay, bx, by, T, R | layer << 16, x0 | x1 << 16, y0 | y1 << 16};
//           k_plot_ground: a thread per frame clips and snaps the ground polygon into a 96-byte record
//   draw    k_plot_draw: a workgroup per 32 x 32 pixel tile and frame walks the frame's records, compacts the hits in ascending slot order into the
//           LDS and runs a wave-uniform loop over them; each lane keeps its 4 pixels' colour and current layer mask in registers
//
// Slots are in paint order: the frame's max(0, index - 1) trajectory segments (layer 1), then the chain segments in table order (layer 2 + chain);
// slots past a frame's own count hold the empty record.  The ground is layer 0 and has a record of its own.
//
// Projection.  clip = M p with every row summed as ((m0 x + m1 y) + m2 z) + m3, (u, v) = (clip.x / clip.w, clip.y / clip.w), col = (a00 u + a01 v) + a02,
// row = (a10 u + a11 v) + a12, snapped as rint(16 col), rint(16 row): fp64, each operation rounded on its own (no contraction).  A segment with an end
// that is not finite is dropped.  A segment crossing w = kWMin is cut there: the end behind becomes in + t (out - in) with t = (in.w - kWMin) /
// (in.w - out.w) and w = kWMin; one wholly behind is dropped.  A segment with a snapped end more than 16 size units (one image side, the guard band)
// outside a border is DROPPED whole (the far end of such a segment is at least one image side away from the picture unless the segment is longer
// than that).  The ground is not dropped but clipped (Sutherland-Hodgman, fp64): against w >= kWMin in clip space, then in pixels against the four
// sides of the guard band, corner = in + t (out - in) with t = (bound - in.c) / (out.c - in.c) and the clipped coordinate set to the bound; up to 9
// corners, snapped and clamped to the band, consecutive duplicates removed, oriented to a positive doubled area.
//
// The bound on the integers.  Images are at most kMaxDim = 4096 pixels a side, so a coordinate lies in [-2^16, 2^17] and a difference of two is at most
// 3 x 2^16: dot and cross products stay below 2^36, L2 = |b - a|^2 below 2^37, and with R <= kMaxR = 4095 the product R^2 L2 is below 2^61 (int64) and
// T = isqrt(R^2 L2) below 2^31 (int32 in the record).  Ground edge values are below 2^37.
namespace {
namespace plot {

constexpr int kSub = 16;              // sub-pixel units per pixel
constexpr int kTile = 32;             // a workgroup's tile is 32 x 32 pixels; wave w draws rows 8 w .. 8 w + 7, a lane 4 pixels (one of each pair of rows)
constexpr int kSlots = 4;
constexpr int kChunk = 256;           // records set up in the LDS at a time; a longer list is drawn in several chunks
constexpr int kWalk = 4;              // records a thread tests per round of a tile's walk over the frame's slots
constexpr int kMaxDim = 4096;
constexpr int kMaxR = 4095;
constexpr int kMaxCorners = 9;        // a quad cut by five lines
constexpr int kGroundInts = 24;       // {corners, slots of the frame, x box, y box, 9 x (x, y), 2 unused}
constexpr double kWMin = 0.0625;
constexpr int kEmptyBox = 1;          // x0 = 1, x1 = 0: no pixel
static_assert(2l * (3l * kSub * kMaxDim) * (3l * kSub * kMaxDim) < (1l << 37), "L2 and every dot / cross product");
static_assert((long)kMaxR * kMaxR < (1l << 24), "R^2 L2 < 2^61");

__device__ __forceinline__ int pack2(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }

struct Clip { double x, y, w; };

__device__ __forceinline__ Clip to_clip(const double* __restrict__ M, double px, double py, double pz) {
#pragma clang fp contract(off)
    Clip c;
    c.x = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3];
    c.y = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7];
    c.w = ((M[12] * px + M[13] * py) + M[14] * pz) + M[15];
    return c;
}
__device__ __forceinline__ bool finite_clip(const Clip& c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.w); }

__device__ __forceinline__ Clip cut_w(const Clip& in, const Clip& out) {              // the point of in -> out on w = kWMin
#pragma clang fp contract(off)
    const double t = (in.w - kWMin) / (in.w - out.w);
    Clip c;
    c.x = in.x + t * (out.x - in.x);
    c.y = in.y + t * (out.y - in.y);
    c.w = kWMin;
    return c;
}

__device__ __forceinline__ void to_pixel(const double* __restrict__ A, const Clip& c, double& col, double& row) {
#pragma clang fp contract(off)
    const double u = c.x / c.w, v = c.y / c.w;
    col = (A[0] * u + A[1] * v) + A[2];
    row = (A[3] * u + A[4] * v) + A[5];
}

__device__ __forceinline__ long isqrt64(long v) {                                      // floor(sqrt(v)), exact, 0 <= v < 2^62
    long r = (long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// the pixels that hold a sample (16 i + 2 + 4 u) of [lo, hi]: ceil((lo - 14) / 16) .. floor((hi - 2) / 16), clipped to the image
__device__ __forceinline__ bool pixel_box(int xlo, int xhi, int ylo, int yhi, int size, int& bx, int& by) {
    const int x0 = max((xlo + 1) >> 4, 0), x1 = min((xhi - 2) >> 4, size - 1);
    const int y0 = max((ylo + 1) >> 4, 0), y1 = min((yhi - 2) >> 4, size - 1);
    bx = by = pack2(kEmptyBox, 0);
    if (x0 > x1 || y0 > y1) return false;
    bx = pack2(x0, x1); by = pack2(y0, y1);
    return true;
}

struct SetupArgs {
    const float* data; const float* trajec; const int* index; const float* bounds; const int* segments; const double* camera;
    int4* records; int* grounds;
    long n_frames, n_take;
    int J, S, P, size, traj_r;
};

__device__ __forceinline__ int frame_trajectory(const SetupArgs& a, long frame, int& idx) {          // the frame's trajectory segments; idx -1: no valid index
    idx = a.index[frame];
    if (idx < 0 || (long)idx >= a.n_take) { idx = -1; return 0; }
    return min(max(idx - 1, 0), a.P - a.S);
}

__global__ __launch_bounds__(256) void k_plot_setup(const SetupArgs a) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_frames * a.P) return;
    const long frame = t / a.P;
    const int w = (int)(t - frame * a.P);
    int idx;
    const int ntraj = frame_trajectory(a, frame, idx);
    int4 r0 = make_int4(0, 0, 0, 0), r1 = make_int4(-1, 0, pack2(kEmptyBox, 0), pack2(kEmptyBox, 0));
    double p[3], q[3];
    int R = 0, layer = 0;
    bool ok = false;
    if (w < ntraj) {                                                   // trajec[w] - trajec[idx] -> trajec[w + 1] - trajec[idx] on y = 0, in fp32 as the reference has them
        const float tx = a.trajec[2 * (long)idx], tz = a.trajec[2 * (long)idx + 1];
        p[0] = (double)(a.trajec[2 * (long)w] - tx); p[1] = 0.0; p[2] = (double)(a.trajec[2 * (long)w + 1] - tz);
        q[0] = (double)(a.trajec[2 * (long)w + 2] - tx); q[1] = 0.0; q[2] = (double)(a.trajec[2 * (long)w + 3] - tz);
        R = a.traj_r; layer = 1; ok = true;
    } else if (w < ntraj + a.S) {
        const int4 s = reinterpret_cast<const int4*>(a.segments)[w - ntraj];           // joint a, joint b, layer, R
        if (s.x >= 0 && s.x < a.J && s.y >= 0 && s.y < a.J && s.z >= 2 && s.z < 0x8000) {
            const float* __restrict__ d = a.data + frame * a.J * 3;
            for (int c = 0; c < 3; ++c) { p[c] = (double)d[3 * s.x + c]; q[c] = (double)d[3 * s.y + c]; }
            R = s.w; layer = s.z; ok = true;
        }
    }
    ok = ok && R >= 1 && R <= kMaxR && R <= kSub * a.size;
    if (ok) {
        Clip ca = to_clip(a.camera, p[0], p[1], p[2]), cb = to_clip(a.camera, q[0], q[1], q[2]);
        ok = finite_clip(ca) && finite_clip(cb) && (ca.w >= kWMin || cb.w >= kWMin);
        if (ok) {
            if (ca.w < kWMin) ca = cut_w(cb, ca);
            else if (cb.w < kWMin) cb = cut_w(ca, cb);
            double c0, r0d, c1, r1d;
            to_pixel(a.camera + 16, ca, c0, r0d);
            to_pixel(a.camera + 16, cb, c1, r1d);
            const double sx0 = rint(16.0 * c0), sy0 = rint(16.0 * r0d), sx1 = rint(16.0 * c1), sy1 = rint(16.0 * r1d);
            const double lo = -(double)(kSub * a.size), hi = (double)(2 * kSub * a.size);
            // (a NaN fails every comparison)
            if (sx0 >= lo && sx0 <= hi && sy0 >= lo && sy0 <= hi && sx1 >= lo && sx1 <= hi && sy1 >= lo && sy1 <= hi) {
                const int ax = (int)sx0, ay = (int)sy0, bx = (int)sx1, by = (int)sy1;
                const long dx = bx - ax, dy = by - ay, L2 = dx * dx + dy * dy;
                const int T = L2 ? (int)isqrt64((long)R * R * L2) : -1;                   // -1: a disc, no sample passes |cross| <= T
                int px, py;
                pixel_box(min(ax, bx) - R, max(ax, bx) + R, min(ay, by) - R, max(ay, by) + R, a.size, px, py);
                r0 = make_int4(ax, ay, bx, by);
                r1 = make_int4(T, R | (layer << 16), px, py);
            }
        }
    }
    a.records[2 * t] = r0;
    a.records[2 * t + 1] = r1;
}

// One clipping pass over a polygon in pixels: keeps c >= bound (keep_above) or c <= bound of coordinate `axis`.
__device__ __forceinline__ int clip_side(const double (&in)[kMaxCorners + 1][2], int n, double (&out)[kMaxCorners + 1][2], int axis, double bound, bool keep_above) {
#pragma clang fp contract(off)
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const double ci = in[i][axis], cj = in[j][axis];
        const bool ii = keep_above ? ci >= bound : ci <= bound, ij = keep_above ? cj >= bound : cj <= bound;
        if (ii && m <= kMaxCorners) { out[m][0] = in[i][0]; out[m][1] = in[i][1]; ++m; }
        if (ii != ij && m <= kMaxCorners) {
            const int s = ii ? i : j, e = ii ? j : i;                  // from the kept corner towards the cut one
            const double t = (bound - in[s][axis]) / (in[e][axis] - in[s][axis]);
            out[m][axis] = bound;
            out[m][1 - axis] = in[s][1 - axis] + t * (in[e][1 - axis] - in[s][1 - axis]);
            ++m;
        }
    }
    return m;
}

__global__ __launch_bounds__(64) void k_plot_ground(const SetupArgs a) {
    const long frame = (long)blockIdx.x * 64 + threadIdx.x;
    if (frame >= a.n_frames) return;
    int idx;
    const int ntraj = frame_trajectory(a, frame, idx);
    int* __restrict__ g = a.grounds + frame * kGroundInts;
    int xs[kMaxCorners + 1], ys[kMaxCorners + 1], n = 0;
    if (idx >= 0) {
        const float tx = a.trajec[2 * (long)idx], tz = a.trajec[2 * (long)idx + 1];
        const float minx = a.bounds[0] - tx, maxx = a.bounds[1] - tx, minz = a.bounds[2] - tz, maxz = a.bounds[3] - tz;
        const Clip c[4] = {to_clip(a.camera, (double)minx, 0.0, (double)minz), to_clip(a.camera, (double)minx, 0.0, (double)maxz),
                           to_clip(a.camera, (double)maxx, 0.0, (double)maxz), to_clip(a.camera, (double)maxx, 0.0, (double)minz)};
        if (finite_clip(c[0]) && finite_clip(c[1]) && finite_clip(c[2]) && finite_clip(c[3])) {
            double pa[kMaxCorners + 1][2], pb[kMaxCorners + 1][2];
            int m = 0;
            bool fin = true;
            for (int i = 0; i < 4; ++i) {                              // w >= kWMin, then to pixels
                const int j = (i + 1) & 3;
                const bool ii = c[i].w >= kWMin, ij = c[j].w >= kWMin;
                if (ii) { to_pixel(a.camera + 16, c[i], pa[m][0], pa[m][1]); ++m; }
                if (ii != ij) { to_pixel(a.camera + 16, ii ? cut_w(c[i], c[j]) : cut_w(c[j], c[i]), pa[m][0], pa[m][1]); ++m; }
            }
            for (int i = 0; i < m; ++i) fin = fin && isfinite(pa[i][0]) && isfinite(pa[i][1]);
            if (fin && m >= 3) {
                const double lo = -(double)a.size, hi = (double)(2 * a.size);
                m = clip_side(pa, m, pb, 0, lo, true);
                m = clip_side(pb, m, pa, 0, hi, false);
                m = clip_side(pa, m, pb, 1, lo, true);
                m = clip_side(pb, m, pa, 1, hi, false);
                const int ilo = -kSub * a.size, ihi = 2 * kSub * a.size;
                for (int i = 0; i < m && i < kMaxCorners; ++i) {
                    const int x = min(max((int)rint(16.0 * pa[i][0]), ilo), ihi), y = min(max((int)rint(16.0 * pa[i][1]), ilo), ihi);
                    if (n && xs[n - 1] == x && ys[n - 1] == y) continue;
                    xs[n] = x; ys[n] = y; ++n;
                }
                if (n > 1 && xs[n - 1] == xs[0] && ys[n - 1] == ys[0]) --n;
            }
        }
    }
    long area = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        area += (long)xs[i] * ys[j] - (long)xs[j] * ys[i];
    }
    int bx = pack2(kEmptyBox, 0), by = bx;
    if (n < 3 || area == 0) n = 0;
    if (n) {
        int xlo = xs[0], xhi = xs[0], ylo = ys[0], yhi = ys[0];
        for (int i = 1; i < n; ++i) { xlo = min(xlo, xs[i]); xhi = max(xhi, xs[i]); ylo = min(ylo, ys[i]); yhi = max(yhi, ys[i]); }
        if (!pixel_box(xlo, xhi, ylo, yhi, a.size, bx, by)) n = 0;
    }
    g[0] = n; g[1] = idx >= 0 ? ntraj + a.S : a.S; g[2] = bx; g[3] = by;
    for (int i = 0; i < kMaxCorners; ++i) {                            // a negative area: the corners in reverse
        const int k = area < 0 ? n - 1 - i : i;
        g[4 + 2 * i] = i < n ? xs[k] : 0;
        g[5 + 2 * i] = i < n ? ys[k] : 0;
    }
    g[22] = g[23] = 0;
}

// ---- draw -------------------------------------------------------------------------------------------------------------------------------------------
struct DrawArgs {
    const int4* records; const int* grounds; const int* colours;
    unsigned char* rgb;
    int P, size, tx, tiles, n_layers;   // tx: tiles per row, tiles: per frame
};

struct DrawLds {
    int list[kChunk + 256 * kWalk];    // the slots whose box meets the tile, ascending; drawn whenever kChunk of them wait
    int wave_hits[kWalk][4];
    int ax[kChunk], ay[kChunk], dx[kChunk], dy[kChunk], T[kChunk], rl[kChunk], bx[kChunk], by[kChunk];
};

__device__ __forceinline__ int blend16(int c, int colour, int k) {     // three bytes of c towards colour by k / 16
    int out = 0;
#pragma unroll
    for (int ch = 0; ch < 24; ch += 8) out |= ((((c >> ch) & 255) * (16 - k) + ((colour >> ch) & 255) * k + 8) >> 4) << ch;
    return out;
}

// the 16 samples (16 x + 2 + 4 u, 16 y + 2 + 4 v) of a pixel against one capsule; (px, py) = sample (0, 0) - a
__device__ __forceinline__ unsigned capsule_mask(int px, int py, int dx, int dy, long L2, long T, long R2) {
    const long dot0 = (long)px * dx + (long)py * dy, cr0 = (long)dx * py - (long)dy * px;
    const int qx = px - dx, qy = py - dy;
    unsigned m = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long dot = dot0 + (long)(4 * u * dx + 4 * v * dy), cr = cr0 + (long)(4 * v * dx - 4 * u * dy);
            const long ex = px + 4 * u, ey = py + 4 * v, fx = qx + 4 * u, fy = qy + 4 * v;
            const bool body = dot >= 0 && dot <= L2 && (cr < 0 ? -cr : cr) <= T;
            const bool caps = ex * ex + ey * ey <= R2 || fx * fx + fy * fy <= R2;
            m |= (unsigned)(body || caps) << (4 * v + u);
        }
    }
    return m;
}

struct Pixels { int c[kSlots]; unsigned mask[kSlots]; int layer; };

__device__ __forceinline__ void flush(Pixels& p, const DrawArgs& a) {                  // the layer is complete: paint it
    const int colour = a.colours[p.layer];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
        const int k = __popc(p.mask[q]);
        if (k) p.c[q] = blend16(p.c[q], colour, k);
        p.mask[q] = 0;
    }
}

__device__ __forceinline__ void draw_chunk(const DrawArgs& a, DrawLds& s, const int* list, long frame, int X0, int Y0, int m, Pixels& p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < m) {
        const long at = 2 * (frame * a.P + list[tid]);
        const int4 r0 = a.records[at], r1 = a.records[at + 1];
        s.ax[tid] = r0.x; s.ay[tid] = r0.y; s.dx[tid] = r0.z - r0.x; s.dy[tid] = r0.w - r0.y;
        s.T[tid] = r1.x; s.rl[tid] = r1.y; s.bx[tid] = r1.z; s.by[tid] = r1.w;
    }
    __syncthreads();
    const int Yw = Y0 + 8 * wave;
    const int x = X0 + (lane & 31), sx = kSub * x + 2;
    for (int k = 0; k < m; ++k) {
        const int bx = __builtin_amdgcn_readfirstlane(s.bx[k]), by = __builtin_amdgcn_readfirstlane(s.by[k]);
        const int rl = __builtin_amdgcn_readfirstlane(s.rl[k]);
        const int layer = rl >> 16, R = rl & 0xffff;
        if (layer < 1 || layer >= a.n_layers) continue;
        if (layer != p.layer) {
            if (p.layer) flush(p, a);
            p.layer = layer;
        }
        const int y0 = by & 0xffff, y1 = by >> 16;
        const int r_lo = max(y0, Yw) - Yw, r_hi = min(y1, Yw + 7) - Yw;
        if (r_lo > r_hi) continue;
        const int ax = s.ax[k], ay = s.ay[k], dx = s.dx[k], dy = s.dy[k];
        const long T = s.T[k], L2 = (long)dx * dx + (long)dy * dy, R2 = (long)R * R;
        const bool xin = x >= (bx & 0xffff) && x <= (bx >> 16);
#pragma unroll
        for (int q = 0; q < kSlots; ++q) {
            if (2 * q + 1 < r_lo || 2 * q > r_hi) continue;
            const int y = Yw + 2 * q + (lane >> 5);
            if (xin && y >= y0 && y <= y1) p.mask[q] |= capsule_mask(sx - ax, kSub * y + 2 - ay, dx, dy, L2, T, R2);
        }
    }
    __syncthreads();                    // (the set-up arrays and the list are rewritten next)
}

__global__ __launch_bounds__(256) void k_plot_draw(const DrawArgs a) {
    __shared__ DrawLds s;
    const long frame = (long)blockIdx.x / a.tiles;
    const int st = (int)((long)blockIdx.x - frame * a.tiles);
    const int X0 = (st % a.tx) * kTile, Y0 = (st / a.tx) * kTile, X1 = X0 + kTile - 1, Y1 = Y0 + kTile - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = X0 + (lane & 31), Yw = Y0 + 8 * wave;
    Pixels p;
#pragma unroll
    for (int q = 0; q < kSlots; ++q) { p.c[q] = 0xffffff; p.mask[q] = 0; }
    p.layer = 0;

    // the ground: a convex polygon of n corners with a positive doubled area; a sample is covered when every edge value is > 0, or = 0 on a top or
    // left edge (render::edge_threshold).  c = (c (32 - k) + 128 k + 16) >> 5
    const int* __restrict__ g = a.grounds + frame * kGroundInts;
    const int gn = g[0], nrec = min(g[1], a.P);
    {
        const int bx = g[2], by = g[3];
        const int bx0 = bx & 0xffff, bx1 = bx >> 16, by0 = by & 0xffff, by1 = by >> 16;
        if (gn >= 3 && bx0 <= bx1 && bx0 <= X1 && bx1 >= X0 && by0 <= Y1 && by1 >= Y0) {           // (uniform)
            unsigned in[kSlots];
#pragma unroll
            for (int q = 0; q < kSlots; ++q) in[q] = 0xffffu;
            for (int e = 0; e < gn; ++e) {
                const int f = e + 1 == gn ? 0 : e + 1;
                const int ex = g[4 + 2 * e], ey = g[5 + 2 * e], fx = g[4 + 2 * f], fy = g[5 + 2 * f];
                const long thr = render::edge_threshold(ex, ey, fx, fy);
                const long A = -(long)(fy - ey), B = fx - ex;
#pragma unroll
                for (int q = 0; q < kSlots; ++q) {
                    const int y = Yw + 2 * q + (lane >> 5);
                    const long e0 = render::edge(ex, ey, fx, fy, kSub * x + 2, kSub * y + 2);
                    unsigned m = 0;
#pragma unroll
                    for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int u = 0; u < 4; ++u) m |= (unsigned)(e0 + 4 * u * A + 4 * v * B >= thr) << (4 * v + u);
                    in[q] &= m;
                }
            }
#pragma unroll
            for (int q = 0; q < kSlots; ++q) {
                const int k = __popc(in[q]);
                const int c = (255 * (32 - k) + 128 * k + 16) >> 5;
                p.c[q] = c | c << 8 | c << 16;
            }
        }
    }

    const int4* __restrict__ rec = a.records + 2 * frame * a.P;
    int count = 0;
    for (int base = 0; base < nrec; base += 256 * kWalk) {
        int2 b[kWalk];
#pragma unroll
        for (int j = 0; j < kWalk; ++j) {
            const int w = base + 256 * j + tid;
            const int4 r = w < nrec ? rec[2 * w + 1] : int4{-1, 0, pack2(kEmptyBox, 0), 0};
            b[j] = int2{r.z, r.w};
        }
        unsigned long long mask[kWalk];
#pragma unroll
        for (int j = 0; j < kWalk; ++j) {
            const int bx0 = b[j].x & 0xffff, bx1 = b[j].x >> 16, by0 = b[j].y & 0xffff, by1 = b[j].y >> 16;
            mask[j] = __ballot(bx0 <= bx1 && bx0 <= X1 && bx1 >= X0 && by0 <= Y1 && by1 >= Y0);
            if (lane == 0) s.wave_hits[j][wave] = __popcll(mask[j]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kWalk; ++j) {                              // slots 256 j + tid of the round, in that order: the list stays ascending
            int before = count;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int h = s.wave_hits[j][w];
                if (w < wave) before += h;
                count += h;
            }
            if ((mask[j] >> lane) & 1ull) s.list[before + __popcll(mask[j] & ((1ull << lane) - 1ull))] = base + 256 * j + tid;       // < kChunk + 256 kWalk
        }
        __syncthreads();
        int head = 0;
        for (; count - head >= kChunk; head += kChunk) draw_chunk(a, s, s.list + head, frame, X0, Y0, kChunk, p);
        if (head) {                                                    // the rest (fewer than kChunk) moves to the front
            const int rest = count - head;
            const int keep = tid < rest ? s.list[head + tid] : 0;
            __syncthreads();
            if (tid < rest) s.list[tid] = keep;
            count = rest;
            __syncthreads();
        }
    }
    if (count > 0) draw_chunk(a, s, s.list, frame, X0, Y0, count, p);
    if (p.layer) flush(p, a);

    if (x < a.size) {
#pragma unroll
        for (int q = 0; q < kSlots; ++q) {
            const int y = Yw + 2 * q + (lane >> 5);
            if (y < a.size) {
                unsigned char* o = a.rgb + ((frame * a.size + y) * a.size + x) * 3;
                o[0] = (unsigned char)(p.c[q] & 255); o[1] = (unsigned char)((p.c[q] >> 8) & 255); o[2] = (unsigned char)((p.c[q] >> 16) & 255);
            }
        }
    }
}

static int64_t record_bytes(int64_t n_frames, int32_t n_slots) { return n_frames * n_slots * 32; }

}  // namespace plot
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t syn_plot_workspace_bytes(int64_t n_frames, int32_t n_slots) {
    if (n_frames < 1 || n_slots < 1) return -1;
    return plot::record_bytes(n_frames, n_slots) + n_frames * plot::kGroundInts * 4;
}

int syn_plot_setup(const float* data, int64_t n_frames, int32_t n_joints, const float* trajec, int64_t n_take, const int32_t* index, const float* bounds,
                   const int32_t* segments, int32_t n_segments, const double* camera, int32_t size, int32_t traj_half_width, int32_t n_slots,
                   void* workspace, void* stream) {
    if (!data || !trajec || !index || !bounds || !segments || !camera || !workspace) return fail_msg("syn_plot_setup: null pointer");
    if (size < 1 || size > plot::kMaxDim) return fail_msg("syn_plot_setup: size is 1 to 4096 pixels");
    if (n_joints < 1 || n_segments < 1 || n_take < 1 || n_frames < 0) return fail_msg("syn_plot_setup: no joints / segments / take, or a negative frame count");
    if (n_slots < n_segments) return fail_msg("syn_plot_setup: n_slots holds the segments and the longest trajectory, so it is at least n_segments");
    if (traj_half_width < 1 || traj_half_width > plot::kMaxR) return fail_msg("syn_plot_setup: half-widths are 1 to 4095 units");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)segments & 15) || ((uintptr_t)camera & 7))
        return fail_msg("syn_plot_setup: the workspace and the segment table must be 16-byte, the camera 8-byte aligned");
    if (n_frames == 0) return 0;
    const int64_t total = n_frames * n_slots;
    if ((total + 255) / 256 > 0x7fffffffLL) return fail_msg("syn_plot_setup: too many slots for one launch");
    plot::SetupArgs a = {};
    a.data = data; a.trajec = trajec; a.index = (const int*)index; a.bounds = bounds; a.segments = (const int*)segments; a.camera = camera;
    a.records = (int4*)workspace; a.grounds = (int*)((char*)workspace + plot::record_bytes(n_frames, n_slots));
    a.n_frames = n_frames; a.n_take = n_take; a.J = n_joints; a.S = n_segments; a.P = n_slots; a.size = size; a.traj_r = traj_half_width;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(plot::k_plot_setup, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(plot::k_plot_ground, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, s, a);
    return launched("k_plot_setup launches");
}

int syn_plot_draw(const void* workspace, int64_t n_frames, int32_t n_slots, const int32_t* colours, int32_t n_layers, int32_t size, uint8_t* rgb,
                  void* stream) {
    if (!workspace || !colours || !rgb) return fail_msg("syn_plot_draw: null pointer");
    if (size < 1 || size > plot::kMaxDim) return fail_msg("syn_plot_draw: size is 1 to 4096 pixels");
    if (n_slots < 1 || n_frames < 0) return fail_msg("syn_plot_draw: no slots, or a negative frame count");
    if (n_layers < 2 || n_layers > 0x8000) return fail_msg("syn_plot_draw: layers are the ground, the trajectory and at least no chain: 2 to 32768");
    if ((uintptr_t)workspace & 15) return fail_msg("syn_plot_draw: the workspace must be 16-byte aligned");
    if (n_frames == 0) return 0;
    const int tx = (size + plot::kTile - 1) / plot::kTile;
    const int64_t blocks = n_frames * tx * tx;
    if (blocks > 0x7fffffffLL) return fail_msg("syn_plot_draw: too many tiles for one launch");
    plot::DrawArgs a = {};
    a.records = (const int4*)workspace; a.grounds = (const int*)((const char*)workspace + plot::record_bytes(n_frames, n_slots)); a.colours = (const int*)colours;
    a.rgb = rgb; a.P = n_slots; a.size = size; a.tx = tx; a.tiles = tx * tx; a.n_layers = n_layers;
    hipLaunchKernelGGL(plot::k_plot_draw, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launched("k_plot_draw launch");
}

}  // extern "C"
