// Motion metrics behind the sampler (the reference's `test()`, diffusion_rvqvae_trainer.py:626-684, 722-728; utils/metric.py): SMPL-X skeleton
// joints from joint rotations, their speeds, the motion beats and their alignment with audio onsets (BC), the L1 diversity, and the h3d
// trainer's recover_from_ric (utils/plot_script.py:15-52).  fp32 throughout, except where noted (onset times and the L1 sums are fp64); no
// floating-point atomics: every sum is taken in an order fixed by the problem's shape alone.
//
// What SMPL-X contributes to the metrics is `joints[:, :55]`: forward kinematics over the 55-joint tree from the rest joints of the shaped
// template (the joints are regressed before the pose correctives, and `test()` passes zero expression and zero transl).  The rest joints are
// one host product per subject (joints.smplx_rest_joints); the kernel below is the tree walk.
namespace {
namespace joints {

constexpr int kMaxJ = 64;              // joints of a tree
constexpr int kFkFrames = 8;           // frames per workgroup
constexpr int kFkWaveFrames = 2;       // ... of which each of its four waves carries two
constexpr int kFkThreads = 256;

// rotation_6d_to_matrix (rotation_conversions.py:511-533): the arithmetic of pose::k_rot6d_to_aa's first half; rows b1, b2, b3
__device__ __forceinline__ void rot6d_matrix(const float* p, float (&R)[9]) {
    const float a1[3] = {p[0], p[1], p[2]}, a2[3] = {p[3], p[4], p[5]};
    float b1[3], b2[3];
    const float n1 = fmaxf(sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12f);
#pragma unroll
    for (int e = 0; e < 3; ++e) b1[e] = a1[e] / n1;
    const float dot = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
#pragma unroll
    for (int e = 0; e < 3; ++e) b2[e] = a2[e] - dot * b1[e];
    const float n2 = fmaxf(sqrtf(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]), 1e-12f);
#pragma unroll
    for (int e = 0; e < 3; ++e) b2[e] = b2[e] / n2;
    R[0] = b1[0]; R[1] = b1[1]; R[2] = b1[2];
    R[3] = b2[0]; R[4] = b2[1]; R[5] = b2[2];
    R[6] = b1[1] * b2[2] - b1[2] * b2[1];
    R[7] = b1[2] * b2[0] - b1[0] * b2[2];
    R[8] = b1[0] * b2[1] - b1[1] * b2[0];
}

// Rodrigues: R = I + (sin t / t) K + ((1 - cos t) / t^2) K^2, K the cross-product matrix of the axis-angle vector, t its length.
// 1 - cos t as 2 sin^2(t / 2) (no cancellation); below t = 1e-4 the two factors by their series, which at t = 0 gives I exactly.
__device__ __forceinline__ void axis_angle_matrix(float x, float y, float z, float (&R)[9]) {
    const float t2 = x * x + y * y + z * z;
    float a, b;
    if (t2 < 1e-8f) {
        a = 1.0f - t2 * (1.0f / 6.0f);
        b = 0.5f - t2 * (1.0f / 24.0f);
    } else {
        const float t = sqrtf(t2), sh = sinf(0.5f * t);
        a = sinf(t) / t;
        b = 2.0f * sh * sh / t2;
    }
    R[0] = 1.0f - b * (y * y + z * z); R[1] = b * x * y - a * z;          R[2] = b * x * z + a * y;
    R[3] = b * x * y + a * z;          R[4] = 1.0f - b * (x * x + z * z); R[5] = b * y * z - a * x;
    R[6] = b * x * z - a * y;          R[7] = b * y * z + a * x;          R[8] = 1.0f - b * (x * x + y * y);
}

// Forward kinematics.  A WAVE carries kFkWaveFrames frames, lane l joint l (a tree has at most 64 joints), and everything stays in registers:
// a lane builds its joint's local transform [R_j | rest_j - rest_parent], and the tree is walked by pointer jumping - every lane holds the
// product G of the local transforms from below some ancestor `a` down to its own joint; a round composes it with the ancestor's product and
// jumps to the ancestor's ancestor, G_j <- G_a . G_j, a_j <- a_a, read from the ancestor's lane with wave shuffles - so depth 11 (SMPL-X) takes
// 4 rounds in which every lane does useful work, where a level-by-level walk issues 11 rounds with most lanes idle.  No LDS, no barrier, no
// per-thread ancestor stack, nothing indexed dynamically in registers.  pose_mean [J][3] (or NULL) is added to the axis-angle vectors before
// Rodrigues: SMPL-X's `full_pose += pose_mean`, the hands' mean pose of a model built with flat_hand_mean = False.  A parent that is not an earlier joint is treated as a root, so a malformed tree cannot send a shuffle
// anywhere but to an earlier lane; a take index outside [0, n_takes) gives NaN joints.
//
// The mesh (syn_mesh.inc, syn_fk_transforms) instantiates this kernel with MESH = true.  That instance also writes, per frame, the A row of the
// corrective product m.feat (N, Kcp) = [R_j - I of joints 1 .. J - 1 | expression | 0 ..] and m.xf (N, J, 3, 4), the rows of the skinning transform
// A_j = [G_j^R | G_j^t - G_j^R rest_j]; the rest joints of frame n are the take's plus m.joint_dirs (J, 3, E) . m.expr[n] where m.expr is set;
// transl is not folded into the root but added to the joints written (`out` may be NULL); axis-angle input only.  MESH = false is syn_fk_joints'
// kernel, its code as it was: every `if constexpr (MESH)` below drops out of it.  The two instances are two compilations - hipcc contracts and
// vectorises them differently, and their joints differ in the last bit - so what the mesh instance adds is written out in fmaf / fadd / fsub (the two
// frame slots of a wave must round alike), and where the joints must be syn_fk_joints' bit for bit (no expression) syn_fk_transforms has the
// MESH = false instance write them.
struct FkMesh {
    const float* joint_dirs; const float* expr;
    float* feat; float* xf;
    int E, Kcp;
};

template <bool MESH>
__global__ __launch_bounds__(kFkThreads) void k_fk(const int* __restrict__ parents, int J, const float* __restrict__ rest, int n_takes,
                                                   const float* __restrict__ rot, int six, const float* __restrict__ transl,
                                                   const int* __restrict__ take_of_frame, int frames_per_take, long N, float* __restrict__ out,
                                                   const float* __restrict__ pose_mean, const FkMesh m) {
    [[maybe_unused]] const int P = 9 * (J - 1);
    [[maybe_unused]] float rj[kFkWaveFrames][3];                 // MESH: the frame's rest joint of this lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool live = lane < J;
    int par = live ? parents[lane] : -1;
    if (par < 0 || par >= lane) par = -1;
    const long nw = (long)blockIdx.x * kFkFrames + wave * kFkWaveFrames;
    float G[kFkWaveFrames][12];
#pragma unroll
    for (int f = 0; f < kFkWaveFrames; ++f) {
        const long n = nw + f;
#pragma unroll
        for (int e = 0; e < 12; ++e) G[f][e] = 0.f;
        if constexpr (MESH) {
            rj[f][0] = rj[f][1] = rj[f][2] = 0.f;
            if (n < N) {
            float* __restrict__ frow = m.feat + n * m.Kcp;
            for (int k = P + lane; k < m.Kcp; k += 64) frow[k] = (m.expr && k - P < m.E) ? m.expr[n * m.E + (k - P)] : 0.f;
            }
        }
        if (!live || n >= N) continue;
        float R[9];
        if (six) {
            const float* s = rot + (n * J + lane) * 6;
            const float v[6] = {s[0], s[1], s[2], s[3], s[4], s[5]};
            rot6d_matrix(v, R);
        } else {
            const float* s = rot + (n * J + lane) * 3;
            float x = s[0], y = s[1], z = s[2];
            if (pose_mean) {
                x += pose_mean[lane * 3]; y += pose_mean[lane * 3 + 1]; z += pose_mean[lane * 3 + 2];
            }
            axis_angle_matrix(x, y, z, R);
        }
        if constexpr (MESH) if (lane >= 1) {
            float* __restrict__ frow = m.feat + n * m.Kcp + (lane - 1) * 9;
#pragma unroll
            for (int e = 0; e < 9; ++e) frow[e] = (e == 0 || e == 4 || e == 8) ? __fsub_rn(R[e], 1.0f) : R[e];
        }
        const int take = take_of_frame ? take_of_frame[n] : (int)(n / frames_per_take);
        float t[3];
        if (take < 0 || take >= n_takes) {
            t[0] = t[1] = t[2] = __builtin_nanf("");
            if constexpr (MESH) rj[f][0] = rj[f][1] = rj[f][2] = __builtin_nanf("");
        } else {
            const float* r = rest + ((long)take * J + lane) * 3;
            if (par >= 0) {
                const float* rp = rest + ((long)take * J + par) * 3;
#pragma unroll
                for (int e = 0; e < 3; ++e) t[e] = r[e] - rp[e];
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e) t[e] = (transl && !MESH) ? r[e] + transl[n * 3 + e] : r[e];
            }
            if constexpr (MESH) {
#pragma unroll
                for (int e = 0; e < 3; ++e) rj[f][e] = r[e];
                if (m.expr) {
                    const float* x = m.expr + n * m.E;
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const float* d = m.joint_dirs + ((long)lane * 3 + e) * m.E;
                        float s = 0.f;
                        for (int k = 0; k < m.E; ++k) s = __fmaf_rn(d[k], x[k], s);
                        rj[f][e] = __fadd_rn(rj[f][e], s);
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) G[f][e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) G[f][9 + e] = t[e];
    }
    if constexpr (MESH) if (m.expr) {                            // the offsets between the MOVED rest joints (all 64 lanes are here again)
        const int src = par >= 0 ? par : lane;
#pragma unroll
        for (int f = 0; f < kFkWaveFrames; ++f)
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float rp = __shfl(rj[f][e], src);
                G[f][9 + e] = par >= 0 ? __fsub_rn(rj[f][e], rp) : rj[f][e];
            }
    }
    int anc = par;
    while (__builtin_amdgcn_ballot_w64(anc >= 0)) {               // (all 64 lanes of every wave are here: shuffles read live registers)
        const int src = anc >= 0 ? anc : lane;
        const int next = __shfl(anc, src);
#pragma unroll
        for (int f = 0; f < kFkWaveFrames; ++f) {
            float P[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = __shfl(G[f][e], src);
            if (anc >= 0) {
                float C[12];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) C[3 * r + c] = P[3 * r] * G[f][c] + P[3 * r + 1] * G[f][3 + c] + P[3 * r + 2] * G[f][6 + c];
                    C[9 + r] = P[3 * r] * G[f][9] + P[3 * r + 1] * G[f][10] + P[3 * r + 2] * G[f][11] + P[9 + r];
                }
#pragma unroll
                for (int e = 0; e < 12; ++e) G[f][e] = C[e];
            }
        }
        anc = anc >= 0 ? next : -1;
    }
#pragma unroll
    for (int f = 0; f < kFkWaveFrames; ++f) {
        const long n = nw + f;
        if (!live || n >= N) continue;
        float* __restrict__ dst = out + (n * J + lane) * 3;
        if constexpr (!MESH) {
            dst[0] = G[f][9]; dst[1] = G[f][10]; dst[2] = G[f][11];
        } else {
        float* __restrict__ a = m.xf + (n * J + lane) * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[4 * r] = G[f][3 * r]; a[4 * r + 1] = G[f][3 * r + 1]; a[4 * r + 2] = G[f][3 * r + 2];
            a[4 * r + 3] = __fsub_rn(G[f][9 + r], __fmaf_rn(G[f][3 * r + 2], rj[f][2], __fmaf_rn(G[f][3 * r + 1], rj[f][1], __fmul_rn(G[f][3 * r], rj[f][0]))));
            if (out) dst[r] = transl ? __fadd_rn(G[f][9 + r], transl[n * 3 + r]) : G[f][9 + r];
        }
        }
    }
}

// Joint speeds (metric.py:98-109): forward difference at a take's first frame, central inside, backward at its last, times fps; the
// Euclidean norm per joint; optionally divided by mmae[J].  n_takes takes of n >= 2 frames each; one thread per (frame, joint).
__global__ __launch_bounds__(256) void k_joint_speed(const float* __restrict__ joints, long total, int n, int J, float fps,
                                                     const float* __restrict__ mmae, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % J);
    const long row = idx / J;
    const int fr = (int)(row % n);
    const long lo = fr == 0 ? row : row - 1, hi = fr == n - 1 ? row : row + 1;
    const float scale = hi - lo == 2 ? 0.5f * fps : fps;
    const float* a = joints + (lo * J + j) * 3;
    const float* b = joints + (hi * J + j) * 3;
    const float dx = (b[0] - a[0]) * scale, dy = (b[1] - a[1]) * scale, dz = (b[2] - a[2]) * scale;
    float v = sqrtf(dx * dx + dy * dy + dz * dz);
    if (mmae) v = v / mmae[j];
    out[idx] = v;
}

// Motion beats (metric.py:111-127).  vel (n_takes, n, J); the slice is [t_start, t_start + n_slice) of every take.  Slice index j of joint i
// is a beat where vel[t_start + j, i] is strictly below its `order` neighbours on each side - neighbours outside the slice clipped to its ends,
// scipy's argrelextrema(..., np.less, order) with mode = 'clip', so the slice's first and last index never qualify - and where
// vel[j, i] > threshold: frame j of the WHOLE take, not j + t_start.  The reference tests slice indices for membership in a list of
// whole-take indices, and its numbers are those of this rule.  mask (n_takes, n_slice, J) uint8.
__global__ __launch_bounds__(256) void k_motion_beats(const float* __restrict__ vel, long total, int n, int J, int t_start, int n_slice, int order,
                                                      float threshold, unsigned char* __restrict__ mask) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx % J);
    const long row = idx / J;
    const int j = (int)(row % n_slice);
    const float* v = vel + (row / n_slice) * (long)n * J + i;
    const float c = v[(long)(t_start + j) * J];
    bool ok = v[(long)j * J] > threshold;
    for (int k = 1; k <= order && ok; ++k) {
        const int lo = j - k < 0 ? 0 : j - k, hi = j + k > n_slice - 1 ? n_slice - 1 : j + k;
        ok = c < v[(long)(t_start + lo) * J] && c < v[(long)(t_start + hi) * J];
    }
    mask[idx] = ok ? 1 : 0;
}

// Beat alignment (metric.py:205-241).  One workgroup per (take, upper-body joint): the joint's beat times j / pose_fps go into the LDS (as
// doubles: the reference's times and the onset detector's are float64, and at 60 s an fp32 time is good to 4e-6 s only - the difference is
// taken in fp64, everything after it in fp32), then one thread per audio onset finds the nearest beat and adds exp(-d^2 / 2 sigma^2); the
// workgroup's sum over the onsets, in a fixed order, divided by their number.  A joint without beats: every distance is inf, every term 0.
constexpr int kAlignThreads = 256;
constexpr int kAlignMaxSlice = 16000;          // beats are at least two frames apart: n_slice / 2 + 1 doubles of dynamic LDS, <= 64 KB

__global__ __launch_bounds__(kAlignThreads) void k_beat_align(const unsigned char* __restrict__ mask, int n_slice, int J, const int* __restrict__ upper,
                                                              int U, const double* __restrict__ onsets, const int* __restrict__ onset_off,
                                                              double pose_fps, float sigma, float* __restrict__ per_joint) {
    extern __shared__ __attribute__((aligned(16))) char align_lds[];
    double* const beat_t = reinterpret_cast<double*>(align_lds);      // n_slice / 2 + 1 entries (the launch sizes it)
    const int cap = n_slice / 2 + 1;
    __shared__ int count;
    __shared__ float part[kAlignThreads / 64];
    const int tid = threadIdx.x, take = blockIdx.x / U, joint = upper[blockIdx.x % U];
    if (joint < 0 || joint >= J) {
        if (tid == 0) per_joint[blockIdx.x] = __builtin_nanf("");
        return;
    }
    if (tid == 0) count = 0;
    __syncthreads();
    const unsigned char* m = mask + (long)take * n_slice * J + joint;
    for (int j = tid; j < n_slice; j += kAlignThreads)
        if (m[(long)j * J]) {
            const int k = atomicAdd(&count, 1);               // (the order of the list does not enter the result: a minimum is taken over it)
            if (k < cap) beat_t[k] = (double)j / pose_fps;
        }
    __syncthreads();
    const int nb = count < cap ? count : cap;
    const int o0 = onset_off[take], M = onset_off[take + 1] - o0;
    const float inv = 1.0f / (2.0f * sigma * sigma);
    float sum = 0.f;
    for (int i = tid; i < M; i += kAlignThreads) {
        const double on = onsets[o0 + i];
        float dmin = __builtin_inff();
        for (int b = 0; b < nb; ++b) dmin = fminf(dmin, (float)fabs(beat_t[b] - on));
        sum += expf(-(dmin * dmin) * inv);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) per_joint[blockIdx.x] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)M;
}

__global__ __launch_bounds__(64) void k_beat_mean(const float* __restrict__ per_joint, int n_takes, int U, float* __restrict__ bc) {
    const int take = blockIdx.x * 64 + threadIdx.x;
    if (take >= n_takes) return;
    float s = 0.f;
    for (int u = 0; u < U; ++u) s += per_joint[(long)take * U + u];
    bc[take] = s / (float)U;
}

// L1 diversity (metric.py:12-27): sum over an (n, C) array of |x - mean over the rows|, for n_takes such arrays in one call.  The rows are cut into chunks of kL1Rows whatever
// the launch; a thread adds one chunk of one column in fp64, row by row; the chunk sums of a column are added in chunk order.  Which thread
// meets which (chunk, column) depends on the grid, the order of every addition does not: the result is bitwise the same for every launch
// geometry and every run.  The input is only read (the reference's `run` overwrites its argument with the deviations).
constexpr int kL1Rows = 32;

__global__ __launch_bounds__(256) void k_l1_chunks(const float* __restrict__ x, long n, int C, const double* __restrict__ mean, double* __restrict__ part) {
    const long chunks = (n + kL1Rows - 1) / kL1Rows, total = chunks * C;
    x += (long)blockIdx.y * n * C;                         // blockIdx.y: the take
    part += (long)blockIdx.y * total;
    if (mean) mean += (long)blockIdx.y * C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long ch = idx / C;
        const int c = (int)(idx - ch * C);
        const long r0 = ch * kL1Rows, r1 = r0 + kL1Rows < n ? r0 + kL1Rows : n;
        double s = 0.0;
        if (mean) {
            const double mu = mean[c];
            for (long r = r0; r < r1; ++r) s += fabs((double)x[r * C + c] - mu);
        } else {
            for (long r = r0; r < r1; ++r) s += (double)x[r * C + c];
        }
        part[idx] = s;
    }
}

__global__ __launch_bounds__(256) void k_l1_columns(const double* __restrict__ part, long chunks, int C, double scale, double* __restrict__ col) {
    part += (long)blockIdx.y * chunks * C;
    col += (long)blockIdx.y * C;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < C; c += gridDim.x * 256) {
        double s = 0.0;
        for (long ch = 0; ch < chunks; ++ch) s += part[ch * C + c];
        col[c] = s * scale;
    }
}

__global__ __launch_bounds__(256) void k_l1_total(const double* __restrict__ col, int C, double* __restrict__ out) {     // one workgroup per take
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
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// recover_from_ric (plot_script.py:15-52).  One workgroup per sequence walks its frames in tiles of kRicTile with a workgroup scan per tile
// (wave shuffles, the waves' totals through the LDS, a running carry): the root yaw is the exclusive prefix sum of channel 0; the root xz the
// inclusive prefix sum of the previous frame's velocity (channels 1, 2) rotated by the inverse of the CURRENT frame's yaw quaternion
// (cos a, 0, sin a, 0) - the angle, not its half, as the reference has it; y is channel 3.  Then one lane per (frame, joint) rotates the
// local joint the same way and adds the root xz.  qrot's arithmetic is kept operation for operation (products rounded on their own).
constexpr int kRicTile = 256;

__device__ __forceinline__ float ric_scan(float v, float* sh, float& carry) {       // inclusive scan over the workgroup, plus the carry
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float o = __shfl_up(v, s);
        if (lane >= s) v += o;
    }
    __syncthreads();                                       // (sh is free again)
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    float pre = carry;
    for (int w = 0; w < wave; ++w) pre += sh[w];
    float total = carry;
    for (int w = 0; w < kRicTile / 64; ++w) total += sh[w];
    carry = total;
    return pre + v;
}

// qrot(qinv((c, 0, s, 0)), (x, y, z)): qvec = (0, -s, 0); uv = qvec x v, uuv = qvec x uv, v + 2 (c uv + uuv); y is untouched
__device__ __forceinline__ void ric_rotate(float c, float s, float& x, float& z) {
    const float q = -s;
    const float uvx = __fmul_rn(q, z), uvz = -__fmul_rn(q, x);
    const float uuvx = __fmul_rn(q, uvz), uuvz = -__fmul_rn(q, uvx);
    const float ox = __fadd_rn(x, __fmul_rn(2.0f, __fadd_rn(__fmul_rn(c, uvx), uuvx)));
    const float oz = __fadd_rn(z, __fmul_rn(2.0f, __fadd_rn(__fmul_rn(c, uvz), uuvz)));
    x = ox; z = oz;
}

__global__ __launch_bounds__(kRicTile) void k_recover_from_ric(const float* __restrict__ data, int n, int C, int Jn, float* __restrict__ out,
                                                             float* __restrict__ quat) {
    __shared__ float sh[kRicTile / 64];
    __shared__ float fr[kRicTile][4];                     // per frame of the tile: cos, sin, root x, root z
    const int tid = threadIdx.x;
    const float* __restrict__ d = data + (long)blockIdx.x * n * C;
    float* __restrict__ o = out + (long)blockIdx.x * n * Jn * 3;
    float cy = 0.f, cx = 0.f, cz = 0.f;
    for (int t0 = 0; t0 < n; t0 += kRicTile) {
        const int i = t0 + tid;
        const bool prev = i > 0 && i < n;
        const float* dp = d + (long)(i - 1) * C;
        const float yaw = ric_scan(prev ? dp[0] : 0.f, sh, cy);
        const float c = cosf(yaw), s = sinf(yaw);
        float vx = prev ? dp[1] : 0.f, vz = prev ? dp[2] : 0.f;
        ric_rotate(c, s, vx, vz);
        const float rx = ric_scan(vx, sh, cx), rz = ric_scan(vz, sh, cz);
        __syncthreads();                                  // (the previous tile's readers of fr are done)
        fr[tid][0] = c; fr[tid][1] = s; fr[tid][2] = rx; fr[tid][3] = rz;
        __syncthreads();
        const int frames = n - t0 < kRicTile ? n - t0 : kRicTile;
        for (int e = tid; e < frames * Jn; e += kRicTile) {
            const int f = e / Jn, k = e - f * Jn;
            const float* p = d + (long)(t0 + f) * C;
            float x, y, z;
            if (k == 0) {
                x = fr[f][2]; y = p[3]; z = fr[f][3];
                if (quat) {
                    float* w = quat + ((long)blockIdx.x * n + t0 + f) * 4;
                    w[0] = fr[f][0]; w[1] = 0.f; w[2] = fr[f][1]; w[3] = 0.f;
                }
            } else {
                x = p[4 + 3 * (k - 1)]; y = p[5 + 3 * (k - 1)]; z = p[6 + 3 * (k - 1)];
                ric_rotate(fr[f][0], fr[f][1], x, z);
                x = __fadd_rn(x, fr[f][2]); z = __fadd_rn(z, fr[f][3]);
            }
            float* q = o + ((long)(t0 + f) * Jn + k) * 3;
            q[0] = x; q[1] = y; q[2] = z;
        }
    }
}

}  // namespace joints
}  // namespace

extern "C" {

// ---- entry points ------------------------------------------------------------------------------------------------------------------------
int syn_fk_joints(const int32_t* parents, int32_t n_joints, const float* rest_joints, int32_t n_takes, const float* rot, int32_t rot6d, const float* transl,
                  const int32_t* take_of_frame, int32_t frames_per_take, int64_t n_frames, const float* pose_mean, float* joints_out, void* stream) {
    if (!parents || !rest_joints || !rot || !joints_out) return fail_msg("syn_fk_joints: null pointer");
    if (pose_mean && rot6d) return fail_msg("syn_fk_joints: a mean pose is added to axis-angle vectors; convert 6D rotations first (syn_rot6d_to_axis_angle)");
    if (n_joints < 1 || n_joints > joints::kMaxJ) return fail_msg("syn_fk_joints: a tree has 1 to 64 joints");
    if (n_takes < 1 || n_frames < 0) return fail_msg("syn_fk_joints: no takes / negative frame count");
    if (!take_of_frame && frames_per_take < 1) return fail_msg("syn_fk_joints: give a frame-to-take index or the frames per take");
    if (!take_of_frame && n_frames > (int64_t)n_takes * frames_per_take) return fail_msg("syn_fk_joints: more frames than n_takes x frames_per_take");
    if (n_frames == 0) return 0;
    const int64_t blocks = (n_frames + joints::kFkFrames - 1) / joints::kFkFrames;
    if (blocks > 0x7fffffffLL) return fail_msg("syn_fk_joints: too many frames for one launch");
    hipLaunchKernelGGL(joints::k_fk<false>, dim3((unsigned)blocks), dim3(joints::kFkThreads), 0, (hipStream_t)stream, (const int*)parents, (int)n_joints, rest_joints, (int)n_takes,
                       rot, (int)(rot6d != 0), transl, (const int*)take_of_frame, (int)frames_per_take, (long)n_frames, joints_out, pose_mean, joints::FkMesh{});
    return launched("k_fk launch");
}

int syn_joint_speed(const float* joints_in, int32_t n_takes, int32_t n_frames, int32_t n_joints, float fps, const float* mmae, float* speed, void* stream) {
    if (!joints_in || !speed) return fail_msg("syn_joint_speed: null pointer");
    if (n_takes < 1 || n_frames < 2 || n_joints < 1) return fail_msg("syn_joint_speed: a take needs at least 2 frames and 1 joint");
    const long total = (long)n_takes * n_frames * n_joints;
    if ((total + 255) / 256 > 0x7fffffffL) return fail_msg("syn_joint_speed: too many elements for one launch");
    hipLaunchKernelGGL(joints::k_joint_speed, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, joints_in, total, (int)n_frames, (int)n_joints, fps, mmae, speed);
    return launched("k_joint_speed launch");
}

int syn_motion_beats(const float* vel, int32_t n_takes, int32_t n_frames, int32_t n_joints, int32_t t_start, int32_t t_end, int32_t order, float threshold,
                     uint8_t* mask, void* stream) {
    if (!vel || !mask) return fail_msg("syn_motion_beats: null pointer");
    if (n_takes < 1 || n_frames < 1 || n_joints < 1 || order < 1) return fail_msg("syn_motion_beats: empty input or order < 1");
    if (t_start < 0 || t_end < t_start || t_end > n_frames) return fail_msg("syn_motion_beats: the slice must satisfy 0 <= t_start <= t_end <= n");
    const int n_slice = t_end - t_start;
    const long total = (long)n_takes * n_slice * n_joints;
    if (total == 0) return 0;
    if ((total + 255) / 256 > 0x7fffffffL) return fail_msg("syn_motion_beats: too many elements for one launch");
    hipLaunchKernelGGL(joints::k_motion_beats, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vel, total, (int)n_frames, (int)n_joints, (int)t_start,
                       n_slice, (int)order, threshold, mask);
    return launched("k_motion_beats launch");
}

int syn_beat_align(const uint8_t* mask, int32_t n_takes, int32_t n_slice, int32_t n_joints, const int32_t* upper_body, int32_t n_upper, const double* onsets,
                   const int32_t* onset_offsets, double pose_fps, float sigma, float* per_joint, float* bc, void* stream) {
    if (!mask || !upper_body || !onsets || !onset_offsets || !per_joint || !bc) return fail_msg("syn_beat_align: null pointer");
    if (n_takes < 1 || n_slice < 0 || n_joints < 1 || n_upper < 1) return fail_msg("syn_beat_align: no takes / joints");
    if (n_slice > joints::kAlignMaxSlice) return fail_msg("syn_beat_align: at most 16000 frames per slice");
    if (!(pose_fps > 0.0) || !(sigma > 0.f)) return fail_msg("syn_beat_align: pose_fps and sigma must be positive");
    if ((uintptr_t)onsets & 7) return fail_msg("syn_beat_align: onsets must be 8-byte aligned");
    hipLaunchKernelGGL(joints::k_beat_align, dim3((unsigned)(n_takes * n_upper)), dim3(joints::kAlignThreads), (size_t)(n_slice / 2 + 1) * sizeof(double), (hipStream_t)stream, mask, (int)n_slice, (int)n_joints,
                       (const int*)upper_body, (int)n_upper, onsets, (const int*)onset_offsets, pose_fps, sigma, per_joint);
    if (int rc = launched("k_beat_align launch")) return rc;
    hipLaunchKernelGGL(joints::k_beat_mean, dim3((unsigned)((n_takes + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float*)per_joint, (int)n_takes, (int)n_upper, bc);
    return launched("k_beat_mean launch");
}

int64_t syn_l1div_workspace_bytes(int32_t n_takes, int64_t n, int32_t channels) {
    if (n_takes < 1 || n < 1 || channels < 1) return -1;                 // (no valid call needs 0 bytes: negative = refused, like an error code)
    return (int64_t)n_takes * (((n + joints::kL1Rows - 1) / joints::kL1Rows) * channels + 2 * (int64_t)channels) * (int64_t)sizeof(double);
}

int syn_l1div(const float* x, int32_t n_takes, int64_t n, int32_t channels, void* workspace, int32_t blocks, double* out, void* stream) {
    if (!x || !workspace || !out) return fail_msg("syn_l1div: null pointer");
    if (n_takes < 1 || n_takes > 65535 || n < 1 || channels < 1) return fail_msg("syn_l1div: empty input, or more than 65535 takes");
    if (((uintptr_t)workspace | (uintptr_t)out) & 7) return fail_msg("syn_l1div: workspace and out must be 8-byte aligned");
    const long chunks = (n + joints::kL1Rows - 1) / joints::kL1Rows, total = chunks * channels;
    long grid = (total + 255) / 256;
    if (blocks > 0) grid = blocks;                         // (a diagnostic: the result does not depend on it)
    if (grid > 65536) grid = 65536;
    double* part = (double*)workspace;
    double* mean = part + (long)n_takes * total;
    double* col = mean + (long)n_takes * channels;
    const unsigned cgrid = (unsigned)((channels + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(joints::k_l1_chunks, dim3((unsigned)grid, (unsigned)n_takes), dim3(256), 0, s, x, (long)n, (int)channels, (const double*)nullptr, part);
    hipLaunchKernelGGL(joints::k_l1_columns, dim3(cgrid, (unsigned)n_takes), dim3(256), 0, s, (const double*)part, chunks, (int)channels, 1.0 / (double)n, mean);
    hipLaunchKernelGGL(joints::k_l1_chunks, dim3((unsigned)grid, (unsigned)n_takes), dim3(256), 0, s, x, (long)n, (int)channels, (const double*)mean, part);
    hipLaunchKernelGGL(joints::k_l1_columns, dim3(cgrid, (unsigned)n_takes), dim3(256), 0, s, (const double*)part, chunks, (int)channels, 1.0, col);
    hipLaunchKernelGGL(joints::k_l1_total, dim3((unsigned)n_takes), dim3(256), 0, s, (const double*)col, (int)channels, out);
    return launched("k_l1 launches");
}

int syn_recover_from_ric(const float* data, int32_t n_seq, int32_t n_frames, int32_t channels, int32_t joints_num, float* joints_out, float* root_quat,
                         void* stream) {
    if (!data || !joints_out) return fail_msg("syn_recover_from_ric: null pointer");
    if (n_seq < 1 || n_frames < 1 || joints_num < 1) return fail_msg("syn_recover_from_ric: empty input");
    if (channels < 4 + 3 * (joints_num - 1)) return fail_msg("syn_recover_from_ric: the features need 4 + 3 (joints_num - 1) channels");
    hipLaunchKernelGGL(joints::k_recover_from_ric, dim3((unsigned)n_seq), dim3(joints::kRicTile), 0, (hipStream_t)stream, data, (int)n_frames, (int)channels, (int)joints_num, joints_out, root_quat);
    return launched("k_recover_from_ric launch");
}

}  // extern "C"
