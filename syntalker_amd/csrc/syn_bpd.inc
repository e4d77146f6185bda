// The per-timestep terms of the variational bound (diffusion/gaussian_diffusion.py:1201-1234, 1548-1603): per sequence, from
// (x_start, x_t, noise, pred_x0), the three scalars calc_bpd_loop collects - vb, xstart_mse, mse.
//
// No timestep of that loop depends on another, so B clips x T timesteps are B T independent sequences: the step kernels evaluate the model
// on all of them as one batch (one timestep per sequence) and this kernel reduces each to its three numbers, one workgroup per sequence.
// Per element, in fp32, with the row (c1, c2, log_var, r, 1 / m, first) of the sequence's timestep:
//     xstart_mse   (pred - x0)^2
//     mse          (eps - noise)^2,  eps = (r x_t - pred) / m     (the reference recovers eps from pred_xstart the same way)
//     vb, t > 0    normal_kl with the same log-variance on both sides: 0.5 exp(-log_var) (c1 (x0 - pred))^2 - the c2 x_t of the two means
//                  cancels; the common factor 0.5 exp(-log_var) is applied to the sum
//     vb, t == 0   -discretized_gaussian_log_likelihood(x0, mean = c1 pred + c2 x_t, log_scale = 0.5 log_var) of diffusion/losses.py: the
//                  tanh form of the normal cdf, bins of half-width 1/255, clamp(min=1e-12) before every log, the edge branches at
//                  |x0| > 0.999 - with full-precision tanhf / expf / logf: the clamp and the difference of two cdfs amplify last-bit changes
// `first` is uniform over a workgroup: only the t == 0 sequences pay for the transcendentals.
//
// The sum.  The four terms of a 16-byte group are added in fp32 in a fixed order; the group sums of a sequence are then added EXACTLY: a
// non-negative fp32 value below 2^32 is split into four 32-bit limbs of a fixed-point number with 96 fractional bits (trunc, subtract and
// scale by 2^32 are exact in fp32), and the limbs are summed as 64-bit integers (12 288 groups: below 2^46) through the thread, the wave
// (shuffles) and the workgroup (LDS).  Integer addition is associative, so the result does not depend on which thread met which group: no
// atomics, bitwise the same on every run, in every launch and for every order of the groups - token-major and fragment-order latents (the
// same 16-byte groups, permuted) give the same bits.  What lies below 2^-96 is dropped; a group sum of 2^32 or more gives +inf, a NaN NaN.
namespace {
namespace bpd {

constexpr int kSeq4 = 32 * 1536 / 4;          // 16-byte groups per sequence
constexpr int kThreads = 256;
constexpr int kAcc = 13;                      // 3 quantities x 4 limbs + the flags

struct Sum {
    unsigned long long l[4];
};

__device__ __forceinline__ void add(Sum& a, unsigned& flags, int q, float s) {
    if (!(s < 4294967296.f)) {                // (vb's terms are -log of a probability, the others squares: never negative)
        flags |= (s != s ? 2u : 1u) << (2 * q);
        return;
    }
    float f = truncf(s);
    a.l[3] += (unsigned)f;
    s = (s - f) * 4294967296.f;
    f = truncf(s);
    a.l[2] += (unsigned)f;
    s = (s - f) * 4294967296.f;
    f = truncf(s);
    a.l[1] += (unsigned)f;
    s = (s - f) * 4294967296.f;
    a.l[0] += (unsigned)truncf(s);
}

__device__ __forceinline__ float cdf(float x) {            // losses.py approx_standard_normal_cdf
    return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * (x * x * x))));
}

__device__ __forceinline__ float nll(float x0, float mean, float inv_stdv) {
    const float c = x0 - mean;
    const float cp = cdf(inv_stdv * (c + (float)(1.0 / 255.0))), cm = cdf(inv_stdv * (c - (float)(1.0 / 255.0)));
    const float lp = x0 < -0.999f ? logf(fmaxf(cp, 1e-12f)) : x0 > 0.999f ? logf(fmaxf(1.0f - cm, 1e-12f)) : logf(fmaxf(cp - cm, 1e-12f));
    return (cp != cp || cm != cm) ? cp + cm : -lp;          // (fmaxf drops a NaN, torch's clamp keeps it)
}

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int mask) {
    const unsigned lo = __shfl_xor((unsigned)v, mask), hi = __shfl_xor((unsigned)(v >> 32), mask);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ double value(const unsigned long long* l, unsigned flags) {
    if (flags & 2u) return __builtin_nan("");
    if (flags & 1u) return __builtin_inf();
    return (((double)l[0] * 0x1p-32 + (double)l[1]) * 0x1p-32 + (double)l[2]) * 0x1p-32 + (double)l[3];
}

__global__ __launch_bounds__(kThreads) void k_bpd_terms(const syn_bpd_row* __restrict__ table, int n_rows, const int* __restrict__ t_row,
                                                        const int* __restrict__ clip, const f32x4* __restrict__ x_start, int n_clips,
                                                        const f32x4* __restrict__ x_t, const f32x4* __restrict__ noise,
                                                        const f32x4* __restrict__ pred, int n_seq, float* __restrict__ out) {
    __shared__ unsigned long long part[kThreads / 64][kAcc];
    const int seq = blockIdx.x, tid = threadIdx.x;
    if (seq >= n_seq) return;
    const int row_i = t_row[seq], c = clip ? clip[seq] : seq;
    if (row_i < 0 || row_i >= n_rows || c < 0 || c >= n_clips) {      // an index outside its table: nothing is read, the answer is NaN
        if (tid < 3) out[(long)tid * n_seq + seq] = __builtin_nanf("");
        return;
    }
    const syn_bpd_row row = table[row_i];
    const bool first = row.first != 0;
    const float inv_stdv = expf(-(0.5f * row.log_var));
    const f32x4* __restrict__ a = x_start + (long)c * kSeq4;
    const long base = (long)seq * kSeq4;
    Sum sx = {{0, 0, 0, 0}}, se = sx, sv = sx;
    unsigned flags = 0;
#pragma unroll 4
    for (int j = 0; j < kSeq4 / kThreads; ++j) {
        const int i = j * kThreads + tid;
        const f32x4 x0 = a[i], xt = x_t[base + i], nz = noise[base + i], p = pred[base + i];
        float tx[4], te[4], tv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = p[k] - x0[k];
            tx[k] = d * d;
            const float e = (row.r * xt[k] - p[k]) * row.inv_m - nz[k];
            te[k] = e * e;
            if (first) {
                tv[k] = nll(x0[k], row.c1 * p[k] + row.c2 * xt[k], inv_stdv);
            } else {
                const float m = row.c1 * d;
                tv[k] = m * m;
            }
        }
        add(sx, flags, 0, (tx[0] + tx[1]) + (tx[2] + tx[3]));
        add(se, flags, 1, (te[0] + te[1]) + (te[2] + te[3]));
        add(sv, flags, 2, (tv[0] + tv[1]) + (tv[2] + tv[3]));
    }
    unsigned long long v[kAcc];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = sx.l[k];
        v[4 + k] = se.l[k];
        v[8 + k] = sv.l[k];
    }
    v[12] = flags;
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = shfl_xor64(v[k], m);
            v[k] = k == 12 ? (v[k] | o) : (v[k] + o);
        }
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kAcc; ++k) part[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kAcc; ++k) {
            unsigned long long s = part[0][k];
            for (int w = 1; w < kThreads / 64; ++w) s = k == 12 ? (s | part[w][k]) : (s + part[w][k]);
            v[k] = s;
        }
        const unsigned fl = (unsigned)v[12];
        const double n = 4.0 * kSeq4, ln2 = 0.6931471805599453;
        const double scale = first ? 1.0 : 0.5 * exp(-(double)row.log_var);
        out[seq] = (float)(value(v + 8, fl >> 4) * scale / (n * ln2));
        out[(long)n_seq + seq] = (float)(value(v, fl) / n);
        out[2L * n_seq + seq] = (float)(value(v + 4, fl >> 2) / n);
    }
}

}  // namespace bpd
}  // namespace

extern "C" int syn_bpd_terms(const syn_bpd_row* table, int32_t n_rows, const int32_t* t_row, const int32_t* clip, const float* x_start, int32_t n_clips,
                             const float* x_t, const float* noise, const float* pred_x0, int32_t n_seq, float* out, void* stream) {
    if (!table || n_rows <= 0 || !t_row || !x_start || n_clips <= 0 || !x_t || !noise || !pred_x0 || n_seq <= 0 || !out)
        return fail_msg("syn_bpd_terms: null pointer, empty table, or no clips / sequences");
    if (!clip && n_seq > n_clips) return fail_msg("syn_bpd_terms: clip = NULL pairs sequence i with clip i: n_seq must not exceed n_clips");
    if (((uintptr_t)x_start | (uintptr_t)x_t | (uintptr_t)noise | (uintptr_t)pred_x0) & 15)
        return fail_msg("syn_bpd_terms: x_start, x_t, noise and pred_x0 must be 16-byte aligned");
    if (((uintptr_t)table | (uintptr_t)t_row | (uintptr_t)clip | (uintptr_t)out) & 3)
        return fail_msg("syn_bpd_terms: table, t_row, clip and out must be 4-byte aligned");
    hipLaunchKernelGGL(bpd::k_bpd_terms, dim3((unsigned)n_seq), dim3(bpd::kThreads), 0, (hipStream_t)stream, table, (int)n_rows, (const int*)t_row,
                       (const int*)clip, (const f32x4*)x_start, (int)n_clips, (const f32x4*)x_t, (const f32x4*)noise, (const f32x4*)pred_x0,
                       (int)n_seq, out);
    return launched("k_bpd_terms launch");
}
