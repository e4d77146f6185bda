// Pose formats either side of the RVQ-VAEs (SURVEY 8 f2 / f3; the reference's `_load_data`, diffusion_rvqvae_trainer.py:257-272, and the tail of
// `_g_test`, :503-531): SMPL-X joint rotations travel as axis-angle vectors, the RVQ-VAEs and the metrics take the 6D representation (first two rows of
// the rotation matrix).  The reference composes four helpers of utils/rotation_conversions.py per direction - a dozen elementwise / masked-scatter
// launches each - here one thread does one joint.  Elementwise fp32 work (36 B per joint): HBM-bound by construction, nothing to tile.
// The arithmetic follows the reference's helpers operation for operation (same small-angle series, same sqrt-of-positive-part + copysign quaternion),
// so that the two agree to fp32 rounding away from the representation's own singularities.
namespace {
namespace pose {

// axis_angle_to_quaternion (rotation_conversions.py:448-477) -> quaternion_to_matrix (:36-64) -> matrix_to_rotation_6d (:535-550)
__global__ __launch_bounds__(256) void k_aa_to_rot6d(const float* __restrict__ aa, long n, float* __restrict__ d6) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = aa[3 * i], y = aa[3 * i + 1], z = aa[3 * i + 2];
    const float angle = sqrtf(x * x + y * y + z * z), half = 0.5f * angle;
    const float s = fabsf(angle) < 1e-6f ? 0.5f - angle * angle / 48.f : sinf(half) / angle;
    const float r = cosf(half), qi = x * s, qj = y * s, qk = z * s;
    const float two_s = 2.0f / (r * r + qi * qi + qj * qj + qk * qk);
    float* o = d6 + 6 * i;
    o[0] = 1.f - two_s * (qj * qj + qk * qk);
    o[1] = two_s * (qi * qj - qk * r);
    o[2] = two_s * (qi * qk + qj * r);
    o[3] = two_s * (qi * qj + qk * r);
    o[4] = 1.f - two_s * (qi * qi + qk * qk);
    o[5] = two_s * (qj * qk - qi * r);
}

__device__ __forceinline__ float sqrt_pos(float v) { return v > 0.f ? sqrtf(v) : 0.f; }                       // _sqrt_positive_part (:85-93)
__device__ __forceinline__ float copysign_ref(float a, float b) { return ((a < 0.f) != (b < 0.f)) ? -a : a; }   // _copysign (:67-82)

// rotation_6d_to_matrix (:511-533: F.normalize, eps 1e-12) -> matrix_to_quaternion (:96-118) -> quaternion_to_axis_angle (:480-508)
__global__ __launch_bounds__(256) void k_rot6d_to_aa(const float* __restrict__ d6, long n, float* __restrict__ aa) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = d6 + 6 * i;
    float a1[3] = {p[0], p[1], p[2]}, a2[3] = {p[3], p[4], p[5]}, b1[3], b2[3], b3[3];
    float n1 = fmaxf(sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12f);
#pragma unroll
    for (int e = 0; e < 3; ++e) b1[e] = a1[e] / n1;
    const float dot = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
#pragma unroll
    for (int e = 0; e < 3; ++e) b2[e] = a2[e] - dot * b1[e];
    float n2 = fmaxf(sqrtf(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]), 1e-12f);
#pragma unroll
    for (int e = 0; e < 3; ++e) b2[e] = b2[e] / n2;
    b3[0] = b1[1] * b2[2] - b1[2] * b2[1];
    b3[1] = b1[2] * b2[0] - b1[0] * b2[2];
    b3[2] = b1[0] * b2[1] - b1[1] * b2[0];
    // rows of the matrix are b1, b2, b3: m[r][c]
    const float m00 = b1[0], m11 = b2[1], m22 = b3[2];
    const float o0 = 0.5f * sqrt_pos(1.f + m00 + m11 + m22);
    const float qx = 0.5f * sqrt_pos(1.f + m00 - m11 - m22), qy = 0.5f * sqrt_pos(1.f - m00 + m11 - m22), qz = 0.5f * sqrt_pos(1.f - m00 - m11 + m22);
    const float o1 = copysign_ref(qx, b3[1] - b2[2]);          // m21 - m12
    const float o2 = copysign_ref(qy, b1[2] - b3[0]);          // m02 - m20
    const float o3 = copysign_ref(qz, b2[0] - b1[1]);          // m10 - m01
    const float norm = sqrtf(o1 * o1 + o2 * o2 + o3 * o3);
    const float half = atan2f(norm, o0), angle = 2.f * half;
    const float s = fabsf(angle) < 1e-6f ? 0.5f - angle * angle / 48.f : sinf(half) / angle;
    aa[3 * i] = o1 / s; aa[3 * i + 1] = o2 / s; aa[3 * i + 2] = o3 / s;
}

}  // namespace pose
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int syn_axis_angle_to_rot6d(const float* axis_angle, int64_t n_joints, float* rot6d, void* stream) {
    if (!axis_angle || !rot6d || n_joints < 0) return fail_msg("syn_axis_angle_to_rot6d: null pointer / negative count");
    if (n_joints == 0) return 0;
    hipLaunchKernelGGL(pose::k_aa_to_rot6d, dim3((unsigned)((n_joints + 255) / 256)), dim3(256), 0, (hipStream_t)stream, axis_angle, (long)n_joints, rot6d);
    return launched("k_aa_to_rot6d launch");
}

int syn_rot6d_to_axis_angle(const float* rot6d, int64_t n_joints, float* axis_angle, void* stream) {
    if (!axis_angle || !rot6d || n_joints < 0) return fail_msg("syn_rot6d_to_axis_angle: null pointer / negative count");
    if (n_joints == 0) return 0;
    hipLaunchKernelGGL(pose::k_rot6d_to_aa, dim3((unsigned)((n_joints + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rot6d, (long)n_joints, axis_angle);
    return launched("k_rot6d_to_aa launch");
}

}  // extern "C"
