// Drawing the mesh (DESIGN.md §22): the scene of the reference's utils/fast_render.py:16-43 - one mesh, one orthographic camera, one directional
// light, one uniform colour - as a software rasteriser.  Integer and fp32 work only, no atomics of any kind, nothing allocated; every output of a
// frame is a function of that frame's inputs alone, so it does not depend on which frames share the call.
//
//   project   world vertex -> screen position snapped to 1/16 pixel (xy_sub), distance in front of the camera (z), smooth vertex normal
//   raster    xy_sub, z, faces -> face_id, depth per pixel: k_face_boxes (pixel bounding box per face), k_frame_box (their union per frame),
//             k_raster (a workgroup per 64 x 64 supertile bins the boxes into the LDS and draws them chunk by chunk)
//   shade     face_id, xy_sub, normals -> rgb, a Lambert term of the project's own (NOT pyrender's metallic-roughness shader)
//
// Coverage.  The sample of pixel (i, j) is its centre (16 i + 8, 16 j + 8) in sub-pixel units, row 0 on top.  A face is oriented so that its
// doubled area  (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0)  is positive (vertices 1 and 2 swap otherwise), the edge function of the edge a -> b is
// E(p) = (bx - ax)(py - ay) - (by - ay)(px - ax), and with w0 = E_12, w1 = E_20, w2 = E_01 (w0 + w1 + w2 = area) a sample is covered when every
// w > 0, or = 0 on a top edge (dy = 0, dx > 0) or a left edge (dy < 0): two faces that share an edge cover a sample on it exactly once.
//
// The bound on the integers.  Images are at most kMaxDim = 8192 pixels a side and the guard band is g = 16 max(W, H) sub-pixel units beyond each
// border (one image side; a face with a vertex outside it is dropped whole, faces partly outside the image are clipped by the pixel loop).  A kept
// coordinate lies in [-2^17, 2^18], so an edge coefficient A or B (a coordinate difference) is at most 3 x 2^17, and an edge value below 2^39:
// edge values are int64.  Inside a supertile they are  C + A dx + B dy  with the value C at the supertile's first sample in int64 and the offsets
// dx, dy <= 16 (kSuper - 1) = 1008, so the step  A dx + B dy  is at most 3 x 2^17 x 2016 < 2^30 (kMaxStep, asserted below) and is int32.  Where
// |C| < 2^30 as well (kFitsInt: every face near its supertile) the sum is below 2^31 and the whole evaluation runs in int32; otherwise in int64.
//
// Depth at a sample is  ((w0 z0 + w1 z1) + w2 z2) / area  in fp32, each w and the area converted from its integer (round to nearest even), every
// product, sum and the quotient rounded on its own - no contraction - so that a numpy float32 restatement gives the same bits.
namespace {
namespace render {

constexpr int kSub = 16;              // sub-pixel units per pixel
constexpr int kSuper = 64;            // a workgroup's supertile is 64 x 64 pixels; wave w draws the tile of rows 16 w .. 16 w + 15
constexpr int kTileRows = 16;
constexpr int kSlots = 16;            // pixels of a lane: the 4 x 4 blocks (16 x 4 pixels each) of its wave's tile
constexpr int kChunk = 256;           // faces set up in the LDS at a time; a longer list is drawn in several chunks
constexpr int kWalk = 4;              // boxes a thread tests per round of a supertile's walk over the frame's faces
constexpr int kMaxDim = 8192;
constexpr long kMaxCoef = 3l * kSub * kMaxDim;                       // |A|, |B|: two coordinates of [-16 kMaxDim, 32 kMaxDim] apart
constexpr long kMaxStep = kMaxCoef * 2 * (kSub * (kSuper - 1));      // |A dx + B dy| inside a supertile
static_assert(kMaxStep < (1l << 30), "the int32 step inside a supertile, and with |C| < 2^30 the int32 edge value, rely on this");
constexpr int kFitsInt = 8;           // bit of a face's set-up flags: its edge values inside the supertile fit 32 bits
constexpr int kSentinel = INT32_MIN;             // xy_sub of a vertex that is not finite on the screen
constexpr int kSnapLimit = 1 << 30;               // finite positions are clamped here: far outside every guard band, and an int

struct Tri {                          // one oriented face on the screen
    int x0, y0, x1, y1, x2, y2;
    float z0, z1, z2;
    long area;
    bool flip;                        // vertices 1 and 2 are the face's third and second
};

__device__ __forceinline__ long edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long)(bx - ax) * (long)(py - ay) - (long)(by - ay) * (long)(px - ax);
}
__device__ __forceinline__ int edge_threshold(int ax, int ay, int bx, int by) {        // the least covered value: 0 on a top or left edge, else 1
    const int dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

// the three products, the two sums and the quotient, each rounded once (the pragma keeps the compiler from fusing any of them)
__device__ __forceinline__ float depth_at(float w0, float w1, float w2, float z0, float z1, float z2, float area) {
#pragma clang fp contract(off)
    const float a = w0 * z0;
    const float b = w1 * z1;
    const float c = w2 * z2;
    const float s = a + b;
    const float t = s + c;
    return t / area;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---- project ----------------------------------------------------------------------------------------------------------------------------------------
// A thread per (frame, vertex).  The normal is the gather form of trimesh's smooth normals: the vertex's faces through the CSR index in ascending
// face index, each face's (p1 - p0) x (p2 - p0) added in that order - a fixed order and no scatter.  A face with a vertex that is not finite is
// left out of the sum, as it is left out of the picture.
__global__ __launch_bounds__(256) void k_project(const float* __restrict__ verts, const float* __restrict__ view, long total, int V, int W, int H, float ymag,
                                                 const int* __restrict__ faces, int F, const int* __restrict__ vf_off, const int* __restrict__ vf_faces,
                                                 int n_incident, int* __restrict__ xy, float* __restrict__ zout, float* __restrict__ nrm) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long frame = idx / V;
    const int v = (int)(idx - frame * V);
    const float px = verts[idx * 3], py = verts[idx * 3 + 1], pz = verts[idx * 3 + 2];
    const float xc = __fmaf_rn(view[0], px, __fmaf_rn(view[1], py, __fmaf_rn(view[2], pz, view[3])));
    const float yc = __fmaf_rn(view[4], px, __fmaf_rn(view[5], py, __fmaf_rn(view[6], pz, view[7])));
    const float zc = __fmaf_rn(view[8], px, __fmaf_rn(view[9], py, __fmaf_rn(view[10], pz, view[11])));
    const float scale = (0.5f * (float)H) / ymag;                              // pixels per unit: ymag spans half the height, pixels are square
    float sx = rintf(16.0f * __fmaf_rn(xc, scale, 0.5f * (float)W));
    float sy = rintf(16.0f * __fmaf_rn(-yc, scale, 0.5f * (float)H));
    int ix = kSentinel, iy = kSentinel;
    if (finite3(xc, yc, zc) && isfinite(sx) && isfinite(sy)) {
        sx = fminf(fmaxf(sx, -(float)kSnapLimit), (float)kSnapLimit);
        sy = fminf(fmaxf(sy, -(float)kSnapLimit), (float)kSnapLimit);
        ix = (int)sx; iy = (int)sy;
    }
    xy[idx * 2] = ix; xy[idx * 2 + 1] = iy;
    zout[idx] = -zc;

    const float* __restrict__ fv = verts + frame * V * 3;
    int k0 = vf_off[v], k1 = vf_off[v + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > n_incident ? n_incident : k1;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = k0; k < k1; ++k) {
        const int f = vf_faces[k];
        if (f < 0 || f >= F) continue;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;
        const float ax = fv[3 * i0], ay = fv[3 * i0 + 1], az = fv[3 * i0 + 2];
        const float bx = fv[3 * i1], by = fv[3 * i1 + 1], bz = fv[3 * i1 + 2];
        const float cx = fv[3 * i2], cy = fv[3 * i2 + 1], cz = fv[3 * i2 + 2];
        if (!(finite3(ax, ay, az) && finite3(bx, by, bz) && finite3(cx, cy, cz))) continue;
        const float ux = bx - ax, uy = by - ay, uz = bz - az;
        const float wx = cx - ax, wy = cy - ay, wz = cz - az;
        const float c0 = uy * wz, c1 = uz * wy, c2 = uz * wx, c3 = ux * wz, c4 = ux * wy, c5 = uy * wx;
        nx = nx + (c0 - c1);
        ny = ny + (c2 - c3);
        nz = nz + (c4 - c5);
    }
    const float q0 = nx * nx, q1 = ny * ny, q2 = nz * nz;
    const float len = sqrtf((q0 + q1) + q2);
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (len > 0.f && isfinite(len)) { ox = nx / len; oy = ny / len; oz = nz / len; }
    nrm[idx * 3] = ox; nrm[idx * 3 + 1] = oy; nrm[idx * 3 + 2] = oz;
}

// ---- raster: boxes ----------------------------------------------------------------------------------------------------------------------------------
// Loads a face's screen triangle, oriented.  false: a vertex index outside the mesh, a sentinel, a vertex outside the guard band, or zero area.
__device__ __forceinline__ bool load_tri(const int* __restrict__ xy, const float* __restrict__ z, const int* __restrict__ faces, int f, int V, int W, int H,
                                         bool want_z, Tri& t) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    const int2 p0 = reinterpret_cast<const int2*>(xy)[i0], p1 = reinterpret_cast<const int2*>(xy)[i1], p2 = reinterpret_cast<const int2*>(xy)[i2];
    const int g = kSub * (W > H ? W : H);
    const int xlo = -g, xhi = kSub * W + g, ylo = -g, yhi = kSub * H + g;
    if (p0.x < xlo || p0.x > xhi || p1.x < xlo || p1.x > xhi || p2.x < xlo || p2.x > xhi) return false;
    if (p0.y < ylo || p0.y > yhi || p1.y < ylo || p1.y > yhi || p2.y < ylo || p2.y > yhi) return false;
    long area = (long)(p1.x - p0.x) * (long)(p2.y - p0.y) - (long)(p1.y - p0.y) * (long)(p2.x - p0.x);
    if (area == 0) return false;
    t.x0 = p0.x; t.y0 = p0.y;
    const bool flip = area < 0;
    t.x1 = flip ? p2.x : p1.x; t.y1 = flip ? p2.y : p1.y;
    t.x2 = flip ? p1.x : p2.x; t.y2 = flip ? p1.y : p2.y;
    t.area = flip ? -area : area;
    t.flip = flip;
    if (want_z) {
        const float za = z[i0], zb = z[i1], zc = z[i2];
        t.z0 = za; t.z1 = flip ? zc : zb; t.z2 = flip ? zb : zc;
    }
    return true;
}

constexpr int kEmptyBoxX = 1;          // x0 = 1, x1 = 0: no pixel
__device__ __forceinline__ int pack2(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }      // two pixel coordinates (0 .. 8191)

// box (n, F) int2 {x0 | x1 << 16, y0 | y1 << 16}: the pixels whose samples the face's bounding box holds, clipped to the image
__global__ __launch_bounds__(256) void k_face_boxes(const int* __restrict__ xy, const int* __restrict__ faces, long total, int V, int F, int W, int H,
                                                    int2* __restrict__ box) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long frame = idx / F;
    const int f = (int)(idx - frame * F);
    Tri t;
    int2 out = {pack2(kEmptyBoxX, 0), pack2(kEmptyBoxX, 0)};
    if (load_tri(xy + frame * V * 2, nullptr, faces, f, V, W, H, false, t)) {
        const int xmin = min(t.x0, min(t.x1, t.x2)), xmax = max(t.x0, max(t.x1, t.x2));
        const int ymin = min(t.y0, min(t.y1, t.y2)), ymax = max(t.y0, max(t.y1, t.y2));
        const int bx0 = max((xmin + 7) >> 4, 0), bx1 = min((xmax - 8) >> 4, W - 1);          // ceil((xmin - 8) / 16), floor((xmax - 8) / 16)
        const int by0 = max((ymin + 7) >> 4, 0), by1 = min((ymax - 8) >> 4, H - 1);
        if (bx0 <= bx1 && by0 <= by1) out = {pack2(bx0, bx1), pack2(by0, by1)};
    }
    box[idx] = out;
}

// fbox (n) int4 {x0, y0, x1, y1}: the union of a frame's boxes (x0 > x1: nothing to draw).  A workgroup per frame, a fixed tree.
__global__ __launch_bounds__(256) void k_frame_box(const int2* __restrict__ box, int F, int4* __restrict__ fbox) {
    __shared__ int sh[4][256];
    const int2* __restrict__ b = box + (long)blockIdx.x * F;
    int x0 = kMaxDim, y0 = kMaxDim, x1 = -1, y1 = -1;
    for (int f = threadIdx.x; f < F; f += 256) {
        const int2 v = b[f];
        const int ax0 = v.x & 0xffff, ax1 = v.x >> 16;
        if (ax0 > ax1) continue;
        x0 = min(x0, ax0); x1 = max(x1, ax1);
        y0 = min(y0, v.y & 0xffff); y1 = max(y1, v.y >> 16);
    }
    sh[0][threadIdx.x] = x0; sh[1][threadIdx.x] = y0; sh[2][threadIdx.x] = x1; sh[3][threadIdx.x] = y1;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] = min(sh[0][threadIdx.x], sh[0][threadIdx.x + w]);
            sh[1][threadIdx.x] = min(sh[1][threadIdx.x], sh[1][threadIdx.x + w]);
            sh[2][threadIdx.x] = max(sh[2][threadIdx.x], sh[2][threadIdx.x + w]);
            sh[3][threadIdx.x] = max(sh[3][threadIdx.x], sh[3][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) fbox[blockIdx.x] = int4{sh[0][0], sh[1][0], sh[2][0], sh[3][0]};
}

// ---- raster: bin and draw ---------------------------------------------------------------------------------------------------------------------------
struct RasterArgs {
    const int* xy; const float* z; const int* faces; const int2* box; const int4* fbox;
    int* face_id; float* depth;
    int V, F, W, H, sx, supers;        // sx: supertiles per row, supers: per frame
    float znear, zfar;
};

struct RasterLds {
    int list[kChunk + 256 * kWalk];    // the faces whose box meets the supertile, in ascending order; drawn whenever kChunk of them wait
    int wave_hits[kWalk][4];
    int A[3][kChunk], B[3][kChunk];    // edge value = C + A (px - ox) + B (py - oy), (ox, oy) the supertile's first sample
    long C[3][kChunk];
    float z[3][kChunk], area[kChunk];
    int thr[kChunk], face[kChunk], bx[kChunk], by[kChunk];
};

// One face over a wave's tile of 64 x 16 pixels.  The tile is 4 x 4 blocks of 16 x 4 pixels, lane l holds pixel (l & 15, l >> 4) of each block:
// slot 4 rg + cg is the block of columns 16 cg .. 16 cg + 15, rows 4 rg .. 4 rg + 3.  Only the blocks the face's box meets are visited (a small
// face: one or two).  e: the lane's edge values in block (0, 0); a block further right adds 256 A, a block further down 64 B.  T = int when every
// edge value of the face inside the supertile fits 32 bits (kFitsInt: |C| < 2^30, and the steps add up to less than 2^30), else long; the values,
// and their fp32 conversions, are the same.  No test against the box per pixel: a sample outside the box is outside an edge.
template <typename T>
__device__ __forceinline__ void draw_face(T e0, T e1, T e2, int sa0, int sa1, int sa2, int sb0, int sb1, int sb2, int thr, int cg_lo, int cg_hi, int rg_lo,
                                          int rg_hi, float z0, float z1, float z2, float area, int f, float znear, float zfar, float (&best)[kSlots],
                                          int (&bf)[kSlots]) {
    const T t0 = (T)(thr & 1), t1 = (T)((thr >> 1) & 1), t2 = (T)((thr >> 2) & 1);
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        if (rg < rg_lo || rg > rg_hi) continue;
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) {
            if (cg < cg_lo || cg > cg_hi) continue;
            const T w0 = e0 + (T)(sa0 * cg + sb0 * rg), w1 = e1 + (T)(sa1 * cg + sb1 * rg), w2 = e2 + (T)(sa2 * cg + sb2 * rg);
            if (w0 >= t0 && w1 >= t1 && w2 >= t2) {
                const float d = depth_at((float)w0, (float)w1, (float)w2, z0, z1, z2, area);
                const int q = 4 * rg + cg;
                if (d >= znear && d <= zfar && (d < best[q] || (d == best[q] && f < bf[q]))) { best[q] = d; bf[q] = f; }
            }
        }
    }
}

// Sets up the m faces of `list` (a thread each) and draws them: wave w owns the tile of rows 16 w .. 16 w + 15 of the supertile; the 16 pixels of a
// lane live in registers.  The loop over faces is wave-uniform, so are the blocks of the tile that a face's box meets.
__device__ __forceinline__ void draw_chunk(const RasterArgs& a, RasterLds& s, const int* list, long frame, int X0, int Y0, int m, float (&best)[kSlots], int (&bf)[kSlots]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < m) {
        const int f = list[tid];
        Tri t;
        int bx = pack2(kEmptyBoxX, 0), by = bx;
        if (load_tri(a.xy + frame * a.V * 2, a.z + frame * a.V, a.faces, f, a.V, a.W, a.H, true, t)) {
            const int2 b = a.box[frame * a.F + f];
            bx = b.x; by = b.y;
            const int ox = kSub * X0 + 8, oy = kSub * Y0 + 8;
            // w0 = E_12, w1 = E_20, w2 = E_01
            s.A[0][tid] = -(t.y2 - t.y1); s.B[0][tid] = t.x2 - t.x1; s.C[0][tid] = edge(t.x1, t.y1, t.x2, t.y2, ox, oy);
            s.A[1][tid] = -(t.y0 - t.y2); s.B[1][tid] = t.x0 - t.x2; s.C[1][tid] = edge(t.x2, t.y2, t.x0, t.y0, ox, oy);
            s.A[2][tid] = -(t.y1 - t.y0); s.B[2][tid] = t.x1 - t.x0; s.C[2][tid] = edge(t.x0, t.y0, t.x1, t.y1, ox, oy);
            const long lim = 1l << 30;
            const bool fits = s.C[0][tid] > -lim && s.C[0][tid] < lim && s.C[1][tid] > -lim && s.C[1][tid] < lim && s.C[2][tid] > -lim && s.C[2][tid] < lim;
            s.thr[tid] = edge_threshold(t.x1, t.y1, t.x2, t.y2) | edge_threshold(t.x2, t.y2, t.x0, t.y0) << 1 | edge_threshold(t.x0, t.y0, t.x1, t.y1) << 2 |
                         (fits ? kFitsInt : 0);
            s.z[0][tid] = t.z0; s.z[1][tid] = t.z1; s.z[2][tid] = t.z2;
            s.area[tid] = (float)t.area;
            s.face[tid] = f;
        }
        s.bx[tid] = bx; s.by[tid] = by;
    }
    __syncthreads();
    const int Yw = Y0 + kTileRows * wave;
    const int lx = kSub * (lane & 15), ly = kSub * (kTileRows * wave + (lane >> 4));         // the lane's pixel of block (0, 0), from the supertile's first sample
    for (int k = 0; k < m; ++k) {
        const int bx = __builtin_amdgcn_readfirstlane(s.bx[k]), by = __builtin_amdgcn_readfirstlane(s.by[k]);
        const int bx0 = bx & 0xffff, bx1 = bx >> 16;
        if (bx0 > bx1) continue;
        const int r_lo = max(by & 0xffff, Yw) - Yw, r_hi = min(by >> 16, Yw + kTileRows - 1) - Yw;
        if (r_lo > r_hi) continue;
        const int cg_lo = (max(bx0, X0) - X0) >> 4, cg_hi = (min(bx1, X0 + kSuper - 1) - X0) >> 4;
        const int thr = __builtin_amdgcn_readfirstlane(s.thr[k]), f = s.face[k];
        const int A0 = s.A[0][k], A1 = s.A[1][k], A2 = s.A[2][k], B0 = s.B[0][k], B1 = s.B[1][k], B2 = s.B[2][k];
        const int d0 = A0 * lx + B0 * ly, d1 = A1 * lx + B1 * ly, d2 = A2 * lx + B2 * ly;
        const long c0 = s.C[0][k], c1 = s.C[1][k], c2 = s.C[2][k];
        const float z0 = s.z[0][k], z1 = s.z[1][k], z2 = s.z[2][k], area = s.area[k];
        if (thr & kFitsInt)
            draw_face<int>((int)c0 + d0, (int)c1 + d1, (int)c2 + d2, 256 * A0, 256 * A1, 256 * A2, 64 * B0, 64 * B1, 64 * B2, thr, cg_lo, cg_hi, r_lo >> 2, r_hi >> 2,
                           z0, z1, z2, area, f, a.znear, a.zfar, best, bf);
        else
            draw_face<long>(c0 + (long)d0, c1 + (long)d1, c2 + (long)d2, 256 * A0, 256 * A1, 256 * A2, 64 * B0, 64 * B1, 64 * B2, thr, cg_lo, cg_hi, r_lo >> 2,
                            r_hi >> 2, z0, z1, z2, area, f, a.znear, a.zfar, best, bf);
    }
    __syncthreads();                    // (the set-up arrays and the list are rewritten next)
}

__global__ __launch_bounds__(256) void k_raster(const RasterArgs a) {
    __shared__ RasterLds s;
    const long frame = (long)blockIdx.x / a.supers;
    const int st = (int)((long)blockIdx.x - frame * a.supers);
    const int X0 = (st % a.sx) * kSuper, Y0 = (st / a.sx) * kSuper;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float best[kSlots];
    int bf[kSlots];
#pragma unroll
    for (int q = 0; q < kSlots; ++q) { best[q] = __builtin_inff(); bf[q] = -1; }

    const int4 fb = a.fbox[frame];
    const int X1 = X0 + kSuper - 1, Y1 = Y0 + kSuper - 1;
    if (fb.x <= fb.z && fb.x <= X1 && fb.z >= X0 && fb.y <= Y1 && fb.w >= Y0) {          // (uniform: else nothing of the frame is in this supertile)
        const int2* __restrict__ box = a.box + frame * a.F;
        int count = 0;
        for (int base = 0; base < a.F; base += 256 * kWalk) {
            int2 b[kWalk];
#pragma unroll
            for (int j = 0; j < kWalk; ++j) {                          // (kWalk loads in flight, one pair of barriers for all of them)
                const int f = base + 256 * j + tid;
                b[j] = f < a.F ? box[f] : int2{pack2(kEmptyBoxX, 0), 0};
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
            for (int j = 0; j < kWalk; ++j) {                          // faces 256 j + tid of the round, in that order: the list stays ascending
                int before = count;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int h = s.wave_hits[j][w];
                    if (w < wave) before += h;
                    count += h;
                }
                if ((mask[j] >> lane) & 1ull) s.list[before + __popcll(mask[j] & ((1ull << lane) - 1ull))] = base + 256 * j + tid;     // < kChunk + 256 kWalk
            }
            __syncthreads();
            int head = 0;
            for (; count - head >= kChunk; head += kChunk) draw_chunk(a, s, s.list + head, frame, X0, Y0, kChunk, best, bf);
            if (head) {                                                // the rest (fewer than kChunk) moves to the front
                const int rest = count - head;
                const int keep = tid < rest ? s.list[head + tid] : 0;
                __syncthreads();
                if (tid < rest) s.list[tid] = keep;
                count = rest;
                __syncthreads();
            }
        }
        if (count > 0) draw_chunk(a, s, s.list, frame, X0, Y0, count, best, bf);
    }
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {                                 // slot 4 rg + cg: 16 pixels of each of 4 rows
        const int x = X0 + 16 * (q & 3) + (lane & 15), y = Y0 + kTileRows * wave + 4 * (q >> 2) + (lane >> 4);
        if (x < a.W && y < a.H) {
            const long o = (frame * a.H + y) * a.W + x;
            a.face_id[o] = bf[q];
            a.depth[o] = best[q];
        }
    }
}

// ---- shade ------------------------------------------------------------------------------------------------------------------------------------------
struct ShadeArgs {
    const int* face_id; const int* xy; const float* nrm; const int* faces;
    unsigned char* rgb;
    long total;
    int V, F, W, H;
    float lx, ly, lz, base[3], ambient, diffuse;
    int bg[3];
};

// A thread per pixel: the covering face's weights again from xy_sub, b = w / area, n = normalise((b0 n0 + b1 n1) + b2 n2) in the oriented order,
// c = base min(1, ambient + diffuse max(0, n . l)), channel = rint(255 c).  No culling, no normal flip: a face turned away gets the ambient term.
__global__ __launch_bounds__(256) void k_shade(const ShadeArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const long hw = (long)a.H * a.W;
    const long frame = idx / hw;
    const int pix = (int)(idx - frame * hw);
    const int py = pix / a.W, px = pix - py * a.W;
    int c0 = a.bg[0], c1 = a.bg[1], c2 = a.bg[2];
    const int f = a.face_id[idx];
    Tri t;
    if (f >= 0 && f < a.F && load_tri(a.xy + frame * a.V * 2, nullptr, a.faces, f, a.V, a.W, a.H, false, t)) {
        const int sx = kSub * px + 8, sy = kSub * py + 8;
        const float area = (float)t.area;
        const float b0 = (float)edge(t.x1, t.y1, t.x2, t.y2, sx, sy) / area, b1 = (float)edge(t.x2, t.y2, t.x0, t.y0, sx, sy) / area,
                    b2 = (float)edge(t.x0, t.y0, t.x1, t.y1, sx, sy) / area;
        const int i0 = a.faces[3 * f], i1 = a.faces[3 * f + (t.flip ? 2 : 1)], i2 = a.faces[3 * f + (t.flip ? 1 : 2)];
        const float* __restrict__ n = a.nrm + frame * a.V * 3;
        const float nx = b0 * n[3 * i0] + b1 * n[3 * i1] + b2 * n[3 * i2];
        const float ny = b0 * n[3 * i0 + 1] + b1 * n[3 * i1 + 1] + b2 * n[3 * i2 + 1];
        const float nz = b0 * n[3 * i0 + 2] + b1 * n[3 * i1 + 2] + b2 * n[3 * i2 + 2];
        const float len = sqrtf(nx * nx + ny * ny + nz * nz);
        float ndl = 0.f;
        if (len > 0.f && isfinite(len)) ndl = fmaxf(0.f, (nx * a.lx + ny * a.ly + nz * a.lz) / len);
        const float c = fminf(1.f, a.ambient + a.diffuse * ndl);
        c0 = (int)rintf(fminf(fmaxf(255.f * a.base[0] * c, 0.f), 255.f));
        c1 = (int)rintf(fminf(fmaxf(255.f * a.base[1] * c, 0.f), 255.f));
        c2 = (int)rintf(fminf(fmaxf(255.f * a.base[2] * c, 0.f), 255.f));
    }
    unsigned char* o = a.rgb + idx * 3;
    o[0] = (unsigned char)c0; o[1] = (unsigned char)c1; o[2] = (unsigned char)c2;
}

static bool bad_image(int32_t width, int32_t height) { return width < 1 || height < 1 || width > kMaxDim || height > kMaxDim; }
static int64_t box_bytes(int64_t n_frames, int32_t n_faces) { return (n_frames * n_faces * 8 + 15) / 16 * 16; }

}  // namespace render
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t syn_render_workspace_bytes(int64_t n_frames, int32_t n_faces) {
    if (n_frames < 1 || n_faces < 1) return -1;
    return render::box_bytes(n_frames, n_faces) + n_frames * 16;
}

int syn_render_project(const float* vertices, int64_t n_frames, int32_t n_verts, const float* view_3x4, int32_t width, int32_t height, float ymag,
                       const int32_t* faces, int32_t n_faces, const int32_t* vf_offsets, const int32_t* vf_faces, int32_t n_incident, int32_t* xy_sub,
                       float* z, float* normal, void* stream) {
    if (!vertices || !view_3x4 || !faces || !vf_offsets || !vf_faces || !xy_sub || !z || !normal) return fail_msg("syn_render_project: null pointer");
    if (render::bad_image(width, height)) return fail_msg("syn_render_project: width and height are 1 to 8192 pixels");
    if (n_verts < 1 || n_faces < 1 || n_incident < 0 || n_frames < 0) return fail_msg("syn_render_project: no vertices / faces, or a negative count");
    if (!(ymag > 0.f)) return fail_msg("syn_render_project: ymag must be positive");
    if (n_frames == 0) return 0;
    const int64_t total = n_frames * n_verts;
    if ((total + 255) / 256 > 0x7fffffffLL) return fail_msg("syn_render_project: too many vertices for one launch");
    hipLaunchKernelGGL(render::k_project, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices, view_3x4, (long)total, (int)n_verts,
                       (int)width, (int)height, ymag, (const int*)faces, (int)n_faces, (const int*)vf_offsets, (const int*)vf_faces, (int)n_incident, (int*)xy_sub,
                       z, normal);
    return launched("k_project launch");
}

int syn_render_raster(const int32_t* xy_sub, const float* z, int64_t n_frames, int32_t n_verts, const int32_t* faces, int32_t n_faces, int32_t width,
                      int32_t height, float znear, float zfar, void* workspace, int32_t* face_id, float* depth, void* stream) {
    if (!xy_sub || !z || !faces || !workspace || !face_id || !depth) return fail_msg("syn_render_raster: null pointer");
    if (render::bad_image(width, height)) return fail_msg("syn_render_raster: width and height are 1 to 8192 pixels");
    if (n_verts < 1 || n_faces < 1 || n_frames < 0) return fail_msg("syn_render_raster: no vertices / faces, or a negative frame count");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)xy_sub & 7)) return fail_msg("syn_render_raster: the workspace must be 16-byte, xy_sub 8-byte aligned");
    if (n_frames == 0) return 0;
    const int64_t nf = n_frames * n_faces;
    const int sx = (width + render::kSuper - 1) / render::kSuper, sy = (height + render::kSuper - 1) / render::kSuper;
    const int64_t blocks = n_frames * sx * sy;
    if ((nf + 255) / 256 > 0x7fffffffLL || blocks > 0x7fffffffLL) return fail_msg("syn_render_raster: too many faces or supertiles for one launch");
    int2* box = (int2*)workspace;
    int4* fbox = (int4*)((char*)workspace + render::box_bytes(n_frames, n_faces));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(render::k_face_boxes, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, (const int*)xy_sub, (const int*)faces, (long)nf, (int)n_verts,
                       (int)n_faces, (int)width, (int)height, box);
    hipLaunchKernelGGL(render::k_frame_box, dim3((unsigned)n_frames), dim3(256), 0, s, (const int2*)box, (int)n_faces, fbox);
    render::RasterArgs a = {};
    a.xy = (const int*)xy_sub; a.z = z; a.faces = (const int*)faces; a.box = box; a.fbox = fbox; a.face_id = (int*)face_id; a.depth = depth;
    a.V = n_verts; a.F = n_faces; a.W = width; a.H = height; a.sx = sx; a.supers = sx * sy; a.znear = znear; a.zfar = zfar;
    hipLaunchKernelGGL(render::k_raster, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return launched("k_raster launches");
}

int syn_render_shade(const int32_t* face_id, const int32_t* xy_sub, const float* normal, int64_t n_frames, int32_t n_verts, const int32_t* faces,
                     int32_t n_faces, int32_t width, int32_t height, float light_x, float light_y, float light_z, float base_r, float base_g, float base_b,
                     float ambient, float diffuse, int32_t background_r, int32_t background_g, int32_t background_b, uint8_t* rgb, void* stream) {
    if (!face_id || !xy_sub || !normal || !faces || !rgb) return fail_msg("syn_render_shade: null pointer");
    if (render::bad_image(width, height)) return fail_msg("syn_render_shade: width and height are 1 to 8192 pixels");
    if (n_verts < 1 || n_faces < 1 || n_frames < 0) return fail_msg("syn_render_shade: no vertices / faces, or a negative frame count");
    if ((uintptr_t)xy_sub & 7) return fail_msg("syn_render_shade: xy_sub must be 8-byte aligned");
    if ((background_r | background_g | background_b) & ~255) return fail_msg("syn_render_shade: the background is three bytes");
    if (n_frames == 0) return 0;
    render::ShadeArgs a = {};
    a.face_id = (const int*)face_id; a.xy = (const int*)xy_sub; a.nrm = normal; a.faces = (const int*)faces; a.rgb = rgb;
    a.total = (long)n_frames * height * width; a.V = n_verts; a.F = n_faces; a.W = width; a.H = height;
    a.lx = light_x; a.ly = light_y; a.lz = light_z; a.base[0] = base_r; a.base[1] = base_g; a.base[2] = base_b; a.ambient = ambient; a.diffuse = diffuse;
    a.bg[0] = background_r; a.bg[1] = background_g; a.bg[2] = background_b;
    if ((a.total + 255) / 256 > 0x7fffffffL) return fail_msg("syn_render_shade: too many pixels for one launch");
    hipLaunchKernelGGL(render::k_shade, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched("k_shade launch");
}

}  // extern "C"
