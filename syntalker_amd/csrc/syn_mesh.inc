// The SMPL-X mesh (DESIGN.md §21): what `smplx(...)["vertices"]` computes for the reference's `test()` (diffusion_rvqvae_trainer.py:640-675) and its
// renderers (utils/other_tools.py render_one_sequence*), as linear blend skinning in four steps.  fp32 throughout, no floating-point atomics.
//
//   v_shaped  = v_template + shapedirs . betas                         per subject, on the host (mesh.smplx_mesh)
//   J_rest    = J_regressor . v_shaped + joint_dirs . expression       joints::k_fk (the expression moves the rest joints)
//   R, G, A   = Rodrigues, the tree walk, A_j = [G^R | G^t - G^R J_rest,j]                      joints::k_fk in its mesh mode
//   v_posed   = v_shaped + [posedirs | exprdirs] . [R_1 - I .. R_{J-1} - I | expression]        k_mesh_vertices, v_mfma_f32_16x16x4_f32
//   vertex    = sum_j w_vj (A_j^R v_posed + A_j^t) + transl                                     k_mesh_vertices' epilogue
//
// The one large product is frames x (3 V) x Kc, Kc = 9 (J - 1) + E (586 for SMPL-X with 100 expression coefficients); v_posed lives in the MFMA's
// accumulators only, and the per-vertex 4 x 4 that `smplx` materialises (1.2 GB for a 60 s take) never exists.
namespace {
namespace mesh {

constexpr int kFrameTile = 32;        // frames per workgroup of k_mesh_vertices (two MFMA row tiles)
constexpr int kVertexBlock = 64;      // vertices per workgroup (a wave carries 16: one MFMA column tile, three coordinate planes)
constexpr int kGroup = 16;            // contraction indices per packed group: 4 MFMA steps, one 16-byte load per lane and plane
constexpr int kMaxKc = 1024;          // 32 x (1024 + 4) floats of LDS = 128.5 KB
constexpr int kXcds = 8;

static inline int kc_padded(int kc) { return (kc + kGroup - 1) / kGroup * kGroup; }
static inline int lds_stride(int kcp) { return kcp + 4; }                  // = 4 mod 16: the 16 frames of a ds_read_b128 start 4 banks apart

// ---- the packed directions ------------------------------------------------------------------------------------------------------------------------
// out [vertex tile of 16][group g][plane p][lane l][u]: B[k = 16 g + 4 (l >> 4) + u][plane p][vertex 16 tile + (l & 15)], k < 9 (J - 1) a pose
// corrective (posedirs (V, 3, P) as the model file has them), then the E expression directions (exprdirs (V, 3, E)); zero for k >= Kc and for
// vertices >= V.  A lane's 16-byte load is the B operand of the group's four MFMA steps u = 0 .. 3 for one plane, so the three planes' accumulators
// of a lane hold x, y, z of the same (frame, vertex).  (Within a group the contraction runs k = 16 g + 4 q + u over u, then q - a fixed order.)
__global__ __launch_bounds__(256) void k_mesh_pack(const float* __restrict__ posedirs, const float* __restrict__ exprdirs, int V, int P, int E, int G,
                                                   long total, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int u = (int)(idx & 3), l = (int)((idx >> 2) & 63);
    long r = idx >> 8;
    const int p = (int)(r % 3);
    r /= 3;
    const int g = (int)(r % G);
    const long vt = r / G;
    const long v = vt * 16 + (l & 15);
    const int k = kGroup * g + 4 * (l >> 4) + u;
    float x = 0.f;
    if (v < V) {
        if (k < P) x = posedirs[(v * 3 + p) * P + k];
        else if (k - P < E) x = exprdirs[(v * 3 + p) * E + (k - P)];
    }
    out[idx] = x;
}

// ---- joint transforms -----------------------------------------------------------------------------------------------------------------------------
// syn_fk_transforms launches joints::k_fk<true> (syn_joints.inc): syn_fk_joints' kernel with the mesh outputs compiled in.  Per frame n:
//   feat (n, Kcp)      the MFMA's A row: R_j - I of joints 1 .. J - 1 row-major, then the expression, then zeros up to Kcp
//   xf (n, J, 3, 4)    the rows of A_j = [G_j^R | G_j^t - G_j^R J_rest,j]
//   jout (n, J, 3)     G_j^t + transl; without an expression written by joints::k_fk<false>, syn_fk_joints' kernel itself (its bits)

// ---- vertices -------------------------------------------------------------------------------------------------------------------------------------
struct VertArgs {
    const float* dirs; const float* feat; const float* xf; const float* v_shaped;
    const int* skin_idx; const float* skin_w; const float* transl; const int* take_of_frame;
    float* out;
    long N;
    int V, Kcp, G, J, W, n_takes, frames_per_take, ftiles, total, stride;
};

// A workgroup owns kFrameTile frames x kVertexBlock vertices; wave w the 16 vertices 16 w .. 16 w + 15 of the block, for both row tiles and the
// three planes: six independent accumulator tiles, so one wave per SIMD keeps the matrix pipe issuing.  The frames' A rows stay in the LDS for the
// whole loop; the B fragments come from global memory (L2: see the grid order below) three groups ahead of their use.  The epilogue reuses the LDS
// for the joint transforms, one row tile at a time (16 x 55 x 48 B = 42 KB: with 76 KB of A rows two workgroups share a CU's 160 KB), and skins:
// lane l holds x, y, z of vertex l & 15 at frames (l >> 4) 4 + e of either row tile.  Every output element
// is one k-ordered chain of length Kcp followed by the vertex's weight list in order: it does not depend on which frames share the launch.  The
// epilogue's arithmetic is written out in fmaf / fadd for that reason: left to the compiler's contraction, the unrolled (frame) slots of a
// lane were not rounded alike (measured: 2e-7 between a frame in one slot and in another).
//
// Grid order: logical workgroup id = vertex block x frame tiles + frame tile, and hardware block b takes id (b % 8) chunk + b / 8 - blocks b and
// b + 8 share an XCD, so an XCD walks a contiguous range of ids and meets a vertex block's direction slab (Kcp x 3 x 64 x 4 B) in its own L2.
__global__ __launch_bounds__(256) void k_mesh_vertices(const VertArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_mesh[];
    const int chunk = (a.total + kXcds - 1) / kXcds;
    const int id = (int)(blockIdx.x % kXcds) * chunk + (int)(blockIdx.x / kXcds);
    if (id >= a.total) return;
    const int vb = id / a.ftiles, ft = id - vb * a.ftiles;
    const long f0 = (long)ft * kFrameTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k4 = a.Kcp >> 2;
    for (int e = tid; e < kFrameTile * k4; e += 256) {
        const int f = e / k4, c = e - f * k4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (f0 + f < a.N) v = *reinterpret_cast<const f32x4*>(a.feat + (f0 + f) * a.Kcp + 4 * c);
        *reinterpret_cast<f32x4*>(s_mesh + f * a.stride + 4 * c) = v;
    }
    __syncthreads();

    const f32x4* __restrict__ bp = reinterpret_cast<const f32x4*>(a.dirs) + ((long)(vb * 4 + wave) * a.G * 3) * 64 + lane;
    const float* ap = s_mesh + (lane & 15) * a.stride + 4 * (lane >> 4);
    const int astep = 16 * a.stride;
    f32x4 acc[2][3];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int p = 0; p < 3; ++p) acc[m][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 b0[3], b1[3], b2[3];
    auto fetch = [&](f32x4 (&b)[3], int g) {
        if (g < a.G) {
#pragma unroll
            for (int p = 0; p < 3; ++p) b[p] = bp[((long)g * 3 + p) * 64];
        }
    };
    auto group = [&](const f32x4 (&b)[3], int g) {
        if (g < a.G) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap + kGroup * g);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(ap + astep + kGroup * g);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    acc[0][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[u], b[p][u], acc[0][p], 0, 0, 0);
                    acc[1][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[u], b[p][u], acc[1][p], 0, 0, 0);
                }
        }
    };
    fetch(b0, 0);
    fetch(b1, 1);
    for (int g = 0; g < a.G; g += 3) {
        fetch(b2, g + 2);
        group(b0, g);
        fetch(b0, g + 3);
        group(b1, g + 1);
        fetch(b1, g + 4);
        group(b2, g + 2);
    }
    // Epilogue, one row tile (16 frames) at a time so that the transforms fit beside another workgroup's A rows (two workgroups per CU: one's
    // staging and skinning overlap the other's MFMA loop).
    const long left = a.N - f0;
    const int frames = left < kFrameTile ? (int)left : kFrameTile;
    const int v = vb * kVertexBlock + wave * 16 + (lane & 15);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();                                           // (the A rows / the first row tile's transforms are read)
        const int fh = frames - 16 * h < 16 ? frames - 16 * h : 16;        // frames of this row tile (may be <= 0)
        {
            const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.xf + (f0 + 16 * h) * a.J * 12);
            for (int e = tid; e < fh * a.J * 3; e += 256) reinterpret_cast<f32x4*>(s_mesh)[e] = src[e];
        }
        __syncthreads();
        if (v >= a.V || fh <= 0) continue;
        float px[4], py[4], pz[4], ox[4], oy[4], oz[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = (lane >> 4) * 4 + i;                     // row of this tile
            float sx = 0.f, sy = 0.f, sz = 0.f;
            if (f < fh) {
                const long n = f0 + 16 * h + f;
                const int take = a.take_of_frame ? a.take_of_frame[n] : (int)(n / a.frames_per_take);
                if (take < 0 || take >= a.n_takes) {
                    sx = sy = sz = __builtin_nanf("");
                } else {
                    const float* s = a.v_shaped + ((long)take * a.V + v) * 3;
                    sx = s[0]; sy = s[1]; sz = s[2];
                }
            }
            px[i] = __fadd_rn(sx, acc[h][0][i]);
            py[i] = __fadd_rn(sy, acc[h][1][i]);
            pz[i] = __fadd_rn(sz, acc[h][2][i]);
            ox[i] = oy[i] = oz[i] = 0.f;
        }
        for (int w = 0; w < a.W; ++w) {
            const float wt = a.skin_w[(long)v * a.W + w];
            if (wt == 0.f) continue;                               // (the padding of a short list)
            int j = a.skin_idx[(long)v * a.W + w];
            j = j < 0 ? 0 : (j >= a.J ? a.J - 1 : j);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = (lane >> 4) * 4 + i;
                const f32x4* A = reinterpret_cast<const f32x4*>(s_mesh + (f * a.J + j) * 12);
                const f32x4 r0 = A[0], r1 = A[1], r2 = A[2];
                ox[i] = __fmaf_rn(wt, __fmaf_rn(r0[0], px[i], __fmaf_rn(r0[1], py[i], __fmaf_rn(r0[2], pz[i], r0[3]))), ox[i]);
                oy[i] = __fmaf_rn(wt, __fmaf_rn(r1[0], px[i], __fmaf_rn(r1[1], py[i], __fmaf_rn(r1[2], pz[i], r1[3]))), oy[i]);
                oz[i] = __fmaf_rn(wt, __fmaf_rn(r2[0], px[i], __fmaf_rn(r2[1], py[i], __fmaf_rn(r2[2], pz[i], r2[3]))), oz[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = (lane >> 4) * 4 + i;
            if (f >= fh) continue;
            const long n = f0 + 16 * h + f;
            float tx = 0.f, ty = 0.f, tz = 0.f;
            if (a.transl) {
                tx = a.transl[n * 3]; ty = a.transl[n * 3 + 1]; tz = a.transl[n * 3 + 2];
            }
            float* __restrict__ o = a.out + (n * a.V + v) * 3;
            o[0] = __fadd_rn(ox[i], tx); o[1] = __fadd_rn(oy[i], ty); o[2] = __fadd_rn(oz[i], tz);
        }
    }
}

// ---- the face losses of test() (:672-673) -----------------------------------------------------------------------------------------------------------
// l2 = mean (rec - tar)^2; lvel = mean |(rec[1:] - tar[:-1]) - (tar[1:] - tar[:-1])| as the reference writes it, the three differences in fp32.  One
// read of the two (n, C) arrays: rows in chunks of joints::kL1Rows, a thread adds one chunk of one column for both numbers in fp64 (part [2][chunks C]);
// joints::k_l1_columns adds a column's chunks in order, k_vl_total the columns in a fixed tree.  Bitwise the same for every grid.
__global__ __launch_bounds__(256) void k_vl_chunks(const float* __restrict__ rec, const float* __restrict__ tar, long n, int C, double* __restrict__ part) {
    const long chunks = (n + joints::kL1Rows - 1) / joints::kL1Rows, total = chunks * C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long ch = idx / C;
        const int c = (int)(idx - ch * C);
        const long r0 = ch * joints::kL1Rows, r1 = r0 + joints::kL1Rows < n ? r0 + joints::kL1Rows : n;
        double s2 = 0.0, sv = 0.0;
        float prev = r0 > 0 ? tar[(r0 - 1) * C + c] : 0.f;
        for (long r = r0; r < r1; ++r) {
            const float x = rec[r * C + c], t = tar[r * C + c];
            const float d = __fsub_rn(x, t);
            s2 += (double)d * (double)d;
            if (r > 0) sv += fabs((double)__fsub_rn(__fsub_rn(x, prev), __fsub_rn(t, prev)));
            prev = t;
        }
        part[idx] = s2;
        part[total + idx] = sv;
    }
}

__global__ __launch_bounds__(256) void k_vl_total(const double* __restrict__ col, int C, double scale_l2, double scale_vel, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    col += (long)blockIdx.x * C;
    for (int c = threadIdx.x; c < C; c += 256) s += col[c];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0] * (blockIdx.x ? scale_vel : scale_l2);
}

static int64_t packed_floats(int32_t n_verts, int32_t kc) {
    if (n_verts < 1 || kc < 1 || kc > kMaxKc) return -1;
    const int64_t vp = ((int64_t)n_verts + kVertexBlock - 1) / kVertexBlock * kVertexBlock;
    return vp * 3 * kc_padded(kc);
}

}  // namespace mesh
}  // namespace

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int syn_mesh_pack_dirs(const float* posedirs, const float* exprdirs, int32_t n_verts, int32_t n_pose, int32_t n_expr, float* out, void* stream) {
    if (!posedirs || !out || (n_expr > 0 && !exprdirs)) return fail_msg("syn_mesh_pack_dirs: null pointer");
    if (n_verts < 1 || n_pose < 1 || n_expr < 0 || n_pose > mesh::kMaxKc || n_expr > mesh::kMaxKc || n_pose + n_expr > mesh::kMaxKc)
        return fail_msg("syn_mesh_pack_dirs: no vertices / directions, or more than 1024 directions");
    const long total = mesh::packed_floats(n_verts, n_pose + n_expr);
    if ((total + 255) / 256 > 0x7fffffffL) return fail_msg("syn_mesh_pack_dirs: too many elements for one launch");
    hipLaunchKernelGGL(mesh::k_mesh_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, posedirs, exprdirs, (int)n_verts, (int)n_pose,
                       (int)n_expr, mesh::kc_padded(n_pose + n_expr) / mesh::kGroup, total, out);
    return launched("k_mesh_pack launch");
}

int syn_fk_transforms(const int32_t* parents, int32_t n_joints, const float* rest_joints, int32_t n_takes, const float* pose, const float* pose_mean,
                      const float* joint_dirs, const float* expression, int32_t n_expr, int32_t kc, const float* transl, const int32_t* take_of_frame,
                      int32_t frames_per_take, int64_t n_frames, float* feat, float* xforms, float* joints_out, void* stream) {
    if (!parents || !rest_joints || !pose || !feat || !xforms || !joints_out) return fail_msg("syn_fk_transforms: null pointer");
    if (n_joints < 2 || n_joints > joints::kMaxJ) return fail_msg("syn_fk_transforms: a skinned tree has 2 to 64 joints");
    if (n_expr < 0 || kc < 9 * (n_joints - 1) + n_expr || kc > mesh::kMaxKc)
        return fail_msg("syn_fk_transforms: negative expression count, or a row length kc outside 9 (J - 1) + n_expr .. 1024");
    if (n_expr > 0 && (!expression || !joint_dirs)) return fail_msg("syn_fk_transforms: n_expr > 0 needs the expression and joint_dirs");
    if (n_takes < 1 || n_frames < 0) return fail_msg("syn_fk_transforms: no takes / negative frame count");
    if (!take_of_frame && frames_per_take < 1) return fail_msg("syn_fk_transforms: give a frame-to-take index or the frames per take");
    if (!take_of_frame && n_frames > (int64_t)n_takes * frames_per_take) return fail_msg("syn_fk_transforms: more frames than n_takes x frames_per_take");
    if (n_frames == 0) return 0;
    const int64_t blocks = (n_frames + joints::kFkFrames - 1) / joints::kFkFrames;
    if (blocks > 0x7fffffffLL) return fail_msg("syn_fk_transforms: too many frames for one launch");
    joints::FkMesh m = {};
    m.joint_dirs = n_expr > 0 ? joint_dirs : nullptr; m.expr = n_expr > 0 ? expression : nullptr;
    m.feat = feat; m.xf = xforms; m.E = n_expr; m.Kcp = mesh::kc_padded(kc);
    // without an expression the joints are syn_fk_joints' own, bit for bit: its instance of the kernel writes them (transl folded into the root, as there)
    float* const mesh_joints = n_expr > 0 ? joints_out : nullptr;
    hipLaunchKernelGGL(joints::k_fk<true>, dim3((unsigned)blocks), dim3(joints::kFkThreads), 0, (hipStream_t)stream, (const int*)parents, (int)n_joints, rest_joints,
                       (int)n_takes, pose, 0, transl, (const int*)take_of_frame, (int)frames_per_take, (long)n_frames, mesh_joints, pose_mean, m);
    if (n_expr == 0) {
        if (int rc = launched("k_fk launch (mesh outputs)")) return rc;
        hipLaunchKernelGGL(joints::k_fk<false>, dim3((unsigned)blocks), dim3(joints::kFkThreads), 0, (hipStream_t)stream, (const int*)parents, (int)n_joints,
                           rest_joints, (int)n_takes, pose, 0, transl, (const int*)take_of_frame, (int)frames_per_take, (long)n_frames, joints_out, pose_mean,
                           joints::FkMesh{});
    }
    return launched("k_fk launch (mesh outputs)");
}

int syn_mesh_vertices(const float* dirs_packed, int32_t n_verts, int32_t kc, const float* feat, const float* xforms, int32_t n_joints,
                      const float* v_shaped, int32_t n_takes, const int32_t* skin_index, const float* skin_weight, int32_t width, const float* transl,
                      const int32_t* take_of_frame, int32_t frames_per_take, int64_t n_frames, float* vertices_out, void* stream) {
    if (!dirs_packed || !feat || !xforms || !v_shaped || !skin_index || !skin_weight || !vertices_out) return fail_msg("syn_mesh_vertices: null pointer");
    if (n_joints < 1 || n_joints > joints::kMaxJ) return fail_msg("syn_mesh_vertices: 1 to 64 joints");
    if (width < 1 || width > n_joints) return fail_msg("syn_mesh_vertices: the weight lists are 1 to n_joints entries wide");
    if (n_verts < 1 || kc < 1 || kc > mesh::kMaxKc) return fail_msg("syn_mesh_vertices: no vertices, or a contraction length outside 1 .. 1024");
    if (n_takes < 1 || n_frames < 0) return fail_msg("syn_mesh_vertices: no takes / negative frame count");
    if (!take_of_frame && frames_per_take < 1) return fail_msg("syn_mesh_vertices: give a frame-to-take index or the frames per take");
    if (!take_of_frame && n_frames > (int64_t)n_takes * frames_per_take) return fail_msg("syn_mesh_vertices: more frames than n_takes x frames_per_take");
    if (((uintptr_t)dirs_packed | (uintptr_t)feat | (uintptr_t)xforms) & 15) return fail_msg("syn_mesh_vertices: dirs_packed, feat and xforms must be 16-byte aligned");
    if (n_frames == 0) return 0;
    mesh::VertArgs a = {};
    a.dirs = dirs_packed; a.feat = feat; a.xf = xforms; a.v_shaped = v_shaped; a.skin_idx = (const int*)skin_index; a.skin_w = skin_weight;
    a.transl = transl; a.take_of_frame = (const int*)take_of_frame; a.out = vertices_out; a.N = (long)n_frames;
    a.V = n_verts; a.Kcp = mesh::kc_padded(kc); a.G = a.Kcp / mesh::kGroup; a.J = n_joints; a.W = width; a.n_takes = n_takes; a.frames_per_take = frames_per_take;
    const int64_t ftiles = (n_frames + mesh::kFrameTile - 1) / mesh::kFrameTile, vblocks = ((int64_t)n_verts + mesh::kVertexBlock - 1) / mesh::kVertexBlock;
    if (ftiles * vblocks > 0x3fffffffLL) return fail_msg("syn_mesh_vertices: too many frame tiles x vertex blocks for one launch");
    a.ftiles = (int)ftiles; a.total = (int)(ftiles * vblocks); a.stride = mesh::lds_stride(a.Kcp);
    const int feat_floats = mesh::kFrameTile * a.stride, xf_floats = 16 * n_joints * 12;        // (the epilogue stages one row tile of transforms at a time)
    const int lds = 4 * (feat_floats > xf_floats ? feat_floats : xf_floats);
    static OncePerDevice once;
    if (once.first()) allow_lds(mesh::k_mesh_vertices, 4 * mesh::kFrameTile * mesh::lds_stride(mesh::kMaxKc));
    const unsigned grid = (unsigned)((a.total + mesh::kXcds - 1) / mesh::kXcds * mesh::kXcds);
    hipLaunchKernelGGL(mesh::k_mesh_vertices, dim3(grid), dim3(256), (size_t)lds, (hipStream_t)stream, a);
    return launched("k_mesh_vertices launch");
}

int64_t syn_vertex_losses_workspace_bytes(int64_t n, int32_t channels) {
    if (n < 1 || channels < 1) return -1;
    return 2 * (((n + joints::kL1Rows - 1) / joints::kL1Rows) * channels + (int64_t)channels) * (int64_t)sizeof(double);
}

int syn_vertex_losses(const float* rec, const float* tar, int64_t n, int32_t channels, void* workspace, int32_t blocks, double* out, void* stream) {
    if (!rec || !tar || !workspace || !out) return fail_msg("syn_vertex_losses: null pointer");
    if (n < 1 || channels < 1) return fail_msg("syn_vertex_losses: empty input");
    if (((uintptr_t)workspace | (uintptr_t)out) & 7) return fail_msg("syn_vertex_losses: workspace and out must be 8-byte aligned");
    const long chunks = (n + joints::kL1Rows - 1) / joints::kL1Rows, total = chunks * channels;
    long grid = (total + 255) / 256;
    if (blocks > 0) grid = blocks;                         // (a diagnostic: the result does not depend on it)
    if (grid > 65536) grid = 65536;
    double* part = (double*)workspace;
    double* col = part + 2 * total;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh::k_vl_chunks, dim3((unsigned)grid), dim3(256), 0, s, rec, tar, (long)n, (int)channels, part);
    hipLaunchKernelGGL(joints::k_l1_columns, dim3((unsigned)((channels + 255) / 256), 2u), dim3(256), 0, s, (const double*)part, chunks, (int)channels, 1.0, col);
    hipLaunchKernelGGL(mesh::k_vl_total, dim3(2), dim3(256), 0, s, (const double*)col, (int)channels, 1.0 / ((double)n * channels),
                       1.0 / ((double)(n - 1) * channels), out);      // (n = 1: no differences, 0 / 0 = NaN, torch's mean of an empty tensor)
    return launched("k_vertex_losses launches");
}

}  // extern "C"
