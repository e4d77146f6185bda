// syn_train.inc — fp32 forward / backward kernels of the non-GEMM pieces of a transformer block, for the
// training path (SURVEY.md §8 a10; reference models/timm_transformer/transformer.py:56-104 Attention,
// :117-151 Mlp, :154-198 Block).  Included by syn_kernels.hip; entry points (syn_ln_*, syn_gelu_*, syn_attn_*,
// syn_bn_*, syn_opt_*, syn_linear_bwd_prep / _wgrad_rows) at the end.  The Linear layers (forward, dgrad, wgrad) already
// run on the MFMA GEMM (syn_linear); these kernels replace the ~40 elementwise / reduction launches per block
// that the PyTorch-ROCm ops cost.  fp32 everywhere: they sit between bf16-operand GEMMs and must not add error.

namespace {
namespace trn {

__device__ __forceinline__ float warp_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- LayerNorm over 512 features, one wave per row (8 features per lane) -----------------------------------
// forward: y = (x - mean) * rstd * g + b; saves mean, rstd
__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                float* __restrict__ y, __bf16* __restrict__ yb, float* __restrict__ mean, float* __restrict__ rstd,
                                                int rows) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xp = x + (size_t)row * SYN_D + lane * 8;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(xp), a1 = *reinterpret_cast<const f32x4*>(xp + 4);
    float s = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a1[0] + a1[1]) + (a1[2] + a1[3]));
    const float m = warp_sum(s) * (1.0f / SYN_D);
    const f32x4 d0 = a0 - m, d1 = a1 - m;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { q = fmaf(d0[e], d0[e], q); q = fmaf(d1[e], d1[e], q); }
    const float r = rsqrtf(warp_sum(q) * (1.0f / SYN_D) + 1e-5f);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(g + lane * 8), g1 = *reinterpret_cast<const f32x4*>(g + lane * 8 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + lane * 8), b1 = *reinterpret_cast<const f32x4*>(b + lane * 8 + 4);
    const f32x4 o0 = d0 * r * g0 + b0, o1 = d1 * r * g1 + b1;
    if (y) {
        float* yp = y + (size_t)row * SYN_D + lane * 8;
        *reinterpret_cast<f32x4*>(yp) = o0;
        *reinterpret_cast<f32x4*>(yp + 4) = o1;
    }
    if (yb) {                                                  // the following Linear's GEMM operand, rounded here instead of by a cast launch
        const bf16x4 h0 = to_bf16x4(o0), h1 = to_bf16x4(o1);
        bf16x8 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h[e] = h0[e]; h[4 + e] = h1[e]; }
        *reinterpret_cast<bf16x8*>(yb + (size_t)row * SYN_D + lane * 8) = h;
    }
    if (lane == 0) { mean[row] = m; rstd[row] = r; }
}

// backward: dx = rstd * (dyg - mean_f(dyg) - xhat * mean_f(dyg * xhat)) [+ add: the gradient that reaches x along the residual
// connection, so that autograd has one gradient for x instead of a copy and an add], dyg = dy * g; per-workgroup partial sums
// of dg = sum_rows dy * xhat and db = sum_rows dy go to part[blockIdx][2][512] (reduced by k_colsum, deterministic)
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ g,
                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                const float* __restrict__ add, float* __restrict__ dx, float* __restrict__ part, int rows,
                                                int rows_per_wg) {
    __shared__ float red[4][2][SYN_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(g + lane * 8), g1 = *reinterpret_cast<const f32x4*>(g + lane * 8 + 4);
    f32x4 dg0 = {0.f, 0.f, 0.f, 0.f}, dg1 = dg0, db0 = dg0, db1 = dg0;
    const int r0 = blockIdx.x * rows_per_wg;
    for (int r = r0 + wave; r < min(rows, r0 + rows_per_wg); r += 4) {
        const size_t o = (size_t)r * SYN_D + lane * 8;
        const f32x4 y0 = *reinterpret_cast<const f32x4*>(dy + o), y1 = *reinterpret_cast<const f32x4*>(dy + o + 4);
        const float m = mean[r], rs = rstd[r];
        const f32x4 h0 = (*reinterpret_cast<const f32x4*>(x + o) - m) * rs, h1 = (*reinterpret_cast<const f32x4*>(x + o + 4) - m) * rs;
        const f32x4 t0 = y0 * g0, t1 = y1 * g1;
        float s1 = ((t0[0] + t0[1]) + (t0[2] + t0[3])) + ((t1[0] + t1[1]) + (t1[2] + t1[3]));
        float s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { s2 = fmaf(t0[e], h0[e], s2); s2 = fmaf(t1[e], h1[e], s2); }
        s1 = warp_sum(s1) * (1.0f / SYN_D);
        s2 = warp_sum(s2) * (1.0f / SYN_D);
        f32x4 o0 = (t0 - s1 - h0 * s2) * rs, o1 = (t1 - s1 - h1 * s2) * rs;
        if (add) { o0 = o0 + *reinterpret_cast<const f32x4*>(add + o); o1 = o1 + *reinterpret_cast<const f32x4*>(add + o + 4); }
        *reinterpret_cast<f32x4*>(dx + o) = o0;
        *reinterpret_cast<f32x4*>(dx + o + 4) = o1;
        dg0 = dg0 + y0 * h0; dg1 = dg1 + y1 * h1; db0 = db0 + y0; db1 = db1 + y1;
    }
    *reinterpret_cast<f32x4*>(&red[wave][0][lane * 8]) = dg0; *reinterpret_cast<f32x4*>(&red[wave][0][lane * 8 + 4]) = dg1;
    *reinterpret_cast<f32x4*>(&red[wave][1][lane * 8]) = db0; *reinterpret_cast<f32x4*>(&red[wave][1][lane * 8 + 4]) = db1;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * SYN_D; i += 256) {
        const int w = i / SYN_D, c = i % SYN_D;
        part[(size_t)blockIdx.x * 2 * SYN_D + i] = (red[0][w][c] + red[1][w][c]) + (red[2][w][c] + red[3][w][c]);
    }
}

// column sums of part[p][cols] in fixed order: columns [0, split) -> out0, [split, cols) -> out1
__global__ void k_colsum(const float* __restrict__ part, int n_part, int cols, int split, float* __restrict__ out0,
                         float* __restrict__ out1) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
#pragma unroll 8
    for (int p = 0; p < n_part; ++p) s += part[(size_t)p * cols + c];   // (loads batched by the unrolling, added in order)
    if (c < split) out0[c] = s; else out1[c - split] = s;
}

// ---- exact-erf GELU (nn.GELU()), elementwise -----------------------------------------------------------------
// ---- BatchNorm1d on batch statistics (+ shortcut) (+ LeakyReLU 0.01) of the audio encoder, channels-last fp32 ------------
// models/utils/layer.py:171-184: act(bn(conv(x)) [+ shortcut]).  Forward: per-chunk (sum, sum of squares) -> finalize (mean,
// rstd, running statistics as nn.BatchNorm1d updates them) -> one elementwise pass.  Backward: with p = the pre-activation,
// dp = dz * (z > 0 ? 1 : 0.01) (the saved output has p's sign), dbeta = sum dp, dgamma = sum dp * xhat,
// dy = gamma rstd (dp - dbeta / M - xhat dgamma / M), dshortcut = dp.  Partial sums are added in a fixed order.
constexpr int kBnRows = 256;        // rows per chunk (a block's threads cover 4-16 rows per pass: many short chunks keep the loads in flight)
// ... halved for short tensors until the statistics launches have ~512 workgroups (the encoder's last blocks: 4 096 rows = 16 chunks of 256)
__host__ __device__ inline int bn_chunk_rows(long rows) {
    int cr = kBnRows;
    while (cr > 32 && rows / cr < 512) cr >>= 1;
    return cr;
}

__global__ __launch_bounds__(256) void k_bn_stats(const float* __restrict__ y, long rows, int C, float* __restrict__ part) {
    __shared__ float red[2][256][4];
    const int tid = threadIdx.x, c4n = C / 4, c4 = tid % c4n, rs = tid / c4n, rstep = 256 / c4n;
    const int cr = bn_chunk_rows(rows);
    const long r0 = (long)blockIdx.x * cr, r1 = min(rows, r0 + cr);
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = s;
#pragma unroll 4
    for (long r = r0 + rs; r < r1; r += rstep) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + r * C + 4 * c4);
        s = s + v; q = q + v * v;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][tid][e] = s[e]; red[1][tid][e] = q[e]; }
    __syncthreads();
    if (tid < c4n) {
        f32x4 ts = {0.f, 0.f, 0.f, 0.f}, tq = ts;
        for (int i = 0; i < rstep; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { ts[e] += red[0][tid + i * c4n][e]; tq[e] += red[1][tid + i * c4n][e]; }
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2) * C + 4 * tid) = ts;
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 1) * C + 4 * tid) = tq;
    }
}

// sum over the chunks of part[chunk][which][c] for one channel per block: 256 partial sums in double, then a tree in LDS
__device__ __forceinline__ void bn_chunk_sums(const float* __restrict__ part, int chunks, int C, int c, double& s, double& q) {
    __shared__ double rs[256], rq[256];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = tid; i < chunks; i += 256) { a += part[((size_t)i * 2) * C + c]; b += part[((size_t)i * 2 + 1) * C + c]; }
    rs[tid] = a; rq[tid] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; rq[tid] += rq[tid + o]; }
        __syncthreads();
    }
    s = rs[0]; q = rq[0];
}

// stats[0][c] = mean, stats[1][c] = rstd; running statistics: momentum update with the UNBIASED variance (torch semantics)
__global__ __launch_bounds__(256) void k_bn_finalize(const float* __restrict__ part, int chunks, int C, long rows, float eps, float momentum,
                              float* __restrict__ stats, float* __restrict__ run_mean, float* __restrict__ run_var,
                              const float* __restrict__ conv_bias) {
    const int c = blockIdx.x;
    double s, q;
    bn_chunk_sums(part, chunks, C, c, s, q);
    if (threadIdx.x) return;
    const double mean = s / rows, var = fmax(q / rows - mean * mean, 0.0);
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(var + eps));
    if (run_mean) {
        // (a per-channel bias of the convolution in front shifts the batch mean and nothing else: it is added here, to the
        // running mean, instead of in a pass of its own over the activations)
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * ((float)mean + (conv_bias ? conv_bias[c] : 0.f));
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(rows > 1 ? var * rows / (rows - 1) : var);
    }
}

__global__ void k_bn_apply(const float* __restrict__ y, const float* __restrict__ shortcut, const float* __restrict__ stats,
                           const float* __restrict__ gamma, const float* __restrict__ beta, int C, long n4, int act, float* __restrict__ z) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    const f32x4 m = *reinterpret_cast<const f32x4*>(stats + c), r = *reinterpret_cast<const f32x4*>(stats + C + c);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), b = *reinterpret_cast<const f32x4*>(beta + c);
    f32x4 p = (v - m) * r * g + b;
    if (shortcut) p = p + *reinterpret_cast<const f32x4*>(shortcut + i * 4);
    if (act) {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = p[e] > 0.f ? p[e] : 0.01f * p[e];
    }
    *reinterpret_cast<f32x4*>(z + i * 4) = p;
}

// part[chunk][0][c] = sum dp, part[chunk][1][c] = sum dp * xhat
// (z == nullptr with act: no shortcut entered the activation, so its sign is that of the normalised y - recomputed from the y this
// pass reads anyway instead of reading z: a third / a quarter fewer bytes in the two passes)
__global__ __launch_bounds__(256) void k_bn_bwd_stats(const float* __restrict__ dz, const float* __restrict__ z, const float* __restrict__ y,
                                                      const float* __restrict__ stats, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, long rows, int C, int act, float* __restrict__ part) {
    __shared__ float red[2][256][4];
    const int tid = threadIdx.x, c4n = C / 4, c4 = tid % c4n, rs = tid / c4n, rstep = 256 / c4n;
    const int cr = bn_chunk_rows(rows);
    const long r0 = (long)blockIdx.x * cr, r1 = min(rows, r0 + cr);
    const f32x4 m = *reinterpret_cast<const f32x4*>(stats + 4 * c4), rr = *reinterpret_cast<const f32x4*>(stats + C + 4 * c4);
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = s;
    f32x4 gm = {0.f, 0.f, 0.f, 0.f}, bt = gm;
    if (act && !z) { gm = *reinterpret_cast<const f32x4*>(gamma + 4 * c4); bt = *reinterpret_cast<const f32x4*>(beta + 4 * c4); }
#pragma unroll 4
    for (long r = r0 + rs; r < r1; r += rstep) {
        f32x4 d = *reinterpret_cast<const f32x4*>(dz + r * C + 4 * c4);
        const f32x4 xh = (*reinterpret_cast<const f32x4*>(y + r * C + 4 * c4) - m) * rr;
        if (act) {
            const f32x4 o = z ? *reinterpret_cast<const f32x4*>(z + r * C + 4 * c4) : xh * gm + bt;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = o[e] > 0.f ? d[e] : 0.01f * d[e];
        }
        s = s + d; q = q + d * xh;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][tid][e] = s[e]; red[1][tid][e] = q[e]; }
    __syncthreads();
    if (tid < c4n) {
        f32x4 ts = {0.f, 0.f, 0.f, 0.f}, tq = ts;
        for (int i = 0; i < rstep; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { ts[e] += red[0][tid + i * c4n][e]; tq[e] += red[1][tid + i * c4n][e]; }
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2) * C + 4 * tid) = ts;
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 1) * C + 4 * tid) = tq;
    }
}

// ---- the same BatchNorm with its statistics reduced over several ranks (nn.SyncBatchNorm, reference train.py:90) --------------
// The per-channel sums leave the device-side reduction as doubles, the caller all-reduces them (RCCL), and the finalising kernels
// take the reduced sums and the global row count.
// sums[0][c], sums[1][c] = the two per-channel sums of part[chunk][2][C] (forward: sum y, sum y^2; backward: sum d, sum d * xhat)
__global__ __launch_bounds__(256) void k_bn_sums64(const float* __restrict__ part, int chunks, int C, double* __restrict__ sums) {
    const int c = blockIdx.x;
    double s, q;
    bn_chunk_sums(part, chunks, C, c, s, q);
    if (threadIdx.x) return;
    sums[c] = s;
    sums[C + c] = q;
}
// k_bn_finalize from reduced sums over rows_total rows
__global__ void k_bn_finalize64(const double* __restrict__ sums, int C, long rows_total, float eps, float momentum, float* __restrict__ stats,
                                float* __restrict__ run_mean, float* __restrict__ run_var, const float* __restrict__ conv_bias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double mean = sums[c] / rows_total, var = fmax(sums[C + c] / rows_total - mean * mean, 0.0);
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(var + eps));
    if (run_mean) {
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * ((float)mean + (conv_bias ? conv_bias[c] : 0.f));
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(rows_total > 1 ? var * rows_total / (rows_total - 1) : var);
    }
}
// dgb[0][c] = dgamma, dgb[1][c] = dbeta of THIS rank (torch: weight / bias gradients stay local, DDP averages them), and the
// reduced sums in the same float layout for k_bn_bwd_apply
__global__ void k_bn_bwd_unpack64(const double* __restrict__ local, const double* __restrict__ total, int C, float* __restrict__ dgb,
                                  float* __restrict__ dgb_total) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    dgb[c] = (float)local[C + c]; dgb[C + c] = (float)local[c]; dgb[2 * C + c] = 0.f;
    dgb_total[c] = (float)total[C + c]; dgb_total[C + c] = (float)total[c];
}

// dgb[0][c] = dgamma, dgb[1][c] = dbeta, dgb[2][c] = 0: the gradient of a convolution bias in front of a batch-statistics BatchNorm (the mean
// subtraction cancels it) - written here so that the caller needs no fill launch for it
__global__ __launch_bounds__(256) void k_bn_bwd_finalize(const float* __restrict__ part, int chunks, int C, float* __restrict__ dgb) {
    const int c = blockIdx.x;
    double s, q;
    bn_chunk_sums(part, chunks, C, c, s, q);
    if (threadIdx.x) return;
    dgb[c] = (float)q;
    dgb[C + c] = (float)s;
    dgb[2 * C + c] = 0.f;
}

__global__ void k_bn_bwd_apply(const float* __restrict__ dz, const float* __restrict__ z, const float* __restrict__ y,
                               const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ dgb, int C, long n4,
                               long rows, int act, float* __restrict__ dy, float* __restrict__ dshort) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    f32x4 d = *reinterpret_cast<const f32x4*>(dz + i * 4);
    const f32x4 m = *reinterpret_cast<const f32x4*>(stats + c), r = *reinterpret_cast<const f32x4*>(stats + C + c);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
    const f32x4 xh = (*reinterpret_cast<const f32x4*>(y + i * 4) - m) * r;
    if (act) {
        const f32x4 o = z ? *reinterpret_cast<const f32x4*>(z + i * 4) : xh * g + *reinterpret_cast<const f32x4*>(beta + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = o[e] > 0.f ? d[e] : 0.01f * d[e];
    }
    if (dshort) *reinterpret_cast<f32x4*>(dshort + i * 4) = d;
    const f32x4 dg = *reinterpret_cast<const f32x4*>(dgb + c), dbv = *reinterpret_cast<const f32x4*>(dgb + C + c);
    const float inv = 1.0f / (float)rows;
    *reinterpret_cast<f32x4*>(dy + i * 4) = g * r * (d - dbv * inv - xh * dg * inv);
}

// ---- fused tail of a BasicBlock (round 5): fewer passes over the block-0-sized tensors -------------------------------------------
// A batch-statistics BatchNorm is an affine map per channel once its statistics exist: a(v) = v * sc + sh, sc = rstd * gamma,
// sh = beta - mean * rstd * gamma.  k_bn_finalize_aff writes (mean, rstd) AND (sc, sh); with them
//   * bn1 + LeakyReLU is applied by conv2 while it stages its input tile (k_conv_train / k_conv_wgrad, `in_aff`): z1 is never written;
//   * the shortcut's BatchNorm is applied inside the block's last elementwise pass (k_bn_apply2): its output is never written;
//   * the backward of bn2 and of the shortcut's BatchNorm share one statistics pass and one apply pass over (dout, y2, y_sc), and the
//     activation's sign comes from the pre-activation recomputed in those passes: the block's output is not read back (nor saved).
__global__ __launch_bounds__(256) void k_bn_finalize_aff(const float* __restrict__ part, int chunks, int C, long rows, float eps, float momentum,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ stats, float* __restrict__ aff, float* __restrict__ run_mean,
                                                         float* __restrict__ run_var, const float* __restrict__ conv_bias) {
    const int c = blockIdx.x;
    double s, q;
    bn_chunk_sums(part, chunks, C, c, s, q);
    if (threadIdx.x) return;
    const double mean = s / rows, var = fmax(q / rows - mean * mean, 0.0);
    const float m = (float)mean, r = (float)(1.0 / sqrt(var + eps));
    stats[c] = m;
    stats[C + c] = r;
    const float sc = r * gamma[c];
    aff[c] = sc;
    aff[C + c] = beta[c] - m * sc;
    if (run_mean) {
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (m + (conv_bias ? conv_bias[c] : 0.f));
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(rows > 1 ? var * rows / (rows - 1) : var);
    }
}

// two finalizations in one launch (bn1 and the shortcut's BatchNorm of a down-sampling block become available together)
struct FinJob { const float* part; int chunks, C; long rows; float eps, momentum; const float* gamma; const float* beta; float* stats; float* aff;
                float* run_mean; float* run_var; const float* conv_bias; };
__global__ __launch_bounds__(256) void k_bn_finalize_aff2(const FinJob ja, const FinJob jb) {
    const bool second = (int)blockIdx.x >= ja.C;
    const FinJob& j = second ? jb : ja;
    const int c = second ? (int)blockIdx.x - ja.C : (int)blockIdx.x, C = j.C;
    double s, q;
    bn_chunk_sums(j.part, j.chunks, C, c, s, q);
    if (threadIdx.x) return;
    const double mean = s / j.rows, var = fmax(q / j.rows - mean * mean, 0.0);
    const float m = (float)mean, r = (float)(1.0 / sqrt(var + j.eps));
    j.stats[c] = m;
    j.stats[C + c] = r;
    const float sc = r * j.gamma[c];
    j.aff[c] = sc;
    j.aff[C + c] = j.beta[c] - m * sc;
    if (j.run_mean) {
        j.run_mean[c] = (1.f - j.momentum) * j.run_mean[c] + j.momentum * (m + (j.conv_bias ? j.conv_bias[c] : 0.f));
        j.run_var[c] = (1.f - j.momentum) * j.run_var[c] + j.momentum * (float)(j.rows > 1 ? var * j.rows / (j.rows - 1) : var);
    }
}

// z = act(a2(y) + (short_aff ? a_s(shortcut) : shortcut)), shortcut may be null
__global__ void k_bn_apply2(const float* __restrict__ y, const float* __restrict__ aff, const float* __restrict__ shortcut,
                            const float* __restrict__ short_aff, int C, long n4, int act, float* __restrict__ z) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(aff + c), sh = *reinterpret_cast<const f32x4*>(aff + C + c);
    f32x4 p;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = fmaf(v[e], sc[e], sh[e]);
    if (shortcut) {
        f32x4 w = *reinterpret_cast<const f32x4*>(shortcut + i * 4);
        if (short_aff) {
            const f32x4 s2 = *reinterpret_cast<const f32x4*>(short_aff + c), h2 = *reinterpret_cast<const f32x4*>(short_aff + C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = fmaf(w[e], s2[e], h2[e]);
        }
        p = p + w;
    }
    if (act) {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = p[e] > 0.f ? p[e] : 0.01f * p[e];
    }
    *reinterpret_cast<f32x4*>(z + i * 4) = p;
}

// backward statistics of the block tail: with p = a2(y) + s (s = a_s(shortcut), the raw shortcut, or nothing), dp = dz * act'(p):
//   part[chunk][0][c] = sum dp, [1][c] = sum dp * xhat2, [2][c] = sum dp * xhat_s (only with short_aff)
__global__ __launch_bounds__(256) void k_bn_bwd_stats2(const float* __restrict__ dz, const float* __restrict__ y, const float* __restrict__ shortcut,
                                                       const float* __restrict__ stats, const float* __restrict__ aff,
                                                       const float* __restrict__ short_stats, const float* __restrict__ short_aff,
                                                       long rows, int C, int act, float* __restrict__ part) {
    __shared__ float red[3][256][4];
    const int tid = threadIdx.x, c4n = C / 4, c4 = tid % c4n, rs = tid / c4n, rstep = 256 / c4n;
    const int cr = bn_chunk_rows(rows);
    const long r0 = (long)blockIdx.x * cr, r1 = min(rows, r0 + cr);
    const f32x4 m = *reinterpret_cast<const f32x4*>(stats + 4 * c4), rr = *reinterpret_cast<const f32x4*>(stats + C + 4 * c4);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(aff + 4 * c4), sh = *reinterpret_cast<const f32x4*>(aff + C + 4 * c4);
    f32x4 ms = {0.f, 0.f, 0.f, 0.f}, rrs = ms, scs = ms, shs = ms;
    if (short_aff) {
        ms = *reinterpret_cast<const f32x4*>(short_stats + 4 * c4); rrs = *reinterpret_cast<const f32x4*>(short_stats + C + 4 * c4);
        scs = *reinterpret_cast<const f32x4*>(short_aff + 4 * c4); shs = *reinterpret_cast<const f32x4*>(short_aff + C + 4 * c4);
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = s, q2 = s;
#pragma unroll 4
    for (long r = r0 + rs; r < r1; r += rstep) {
        f32x4 d = *reinterpret_cast<const f32x4*>(dz + r * C + 4 * c4);
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + r * C + 4 * c4);
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (shortcut) w = *reinterpret_cast<const f32x4*>(shortcut + r * C + 4 * c4);
        if (act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = fmaf(v[e], sc[e], sh[e]) + (short_aff ? fmaf(w[e], scs[e], shs[e]) : w[e]);
                d[e] = p > 0.f ? d[e] : 0.01f * d[e];
            }
        }
        s = s + d; q = q + d * ((v - m) * rr);
        if (short_aff) q2 = q2 + d * ((w - ms) * rrs);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][tid][e] = s[e]; red[1][tid][e] = q[e]; red[2][tid][e] = q2[e]; }
    __syncthreads();
    if (tid < c4n) {
        const int nsum = short_aff ? 3 : 2;
        for (int w = 0; w < nsum; ++w) {
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < rstep; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] += red[w][tid + i * c4n][e];
            *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 3 + w) * C + 4 * tid) = t;
        }
    }
}

// dgb2 = [dgamma2 | dbeta2 | 0], dgbs = [dgamma_s | dbeta_s | 0] from part[chunk][3][C] (one channel per block)
__global__ __launch_bounds__(256) void k_bn_bwd_finalize2(const float* __restrict__ part, int chunks, int C, float* __restrict__ dgb2,
                                                          float* __restrict__ dgbs) {
    __shared__ double r0[256], r1[256], r2[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, b = 0.0, d = 0.0;
    for (int i = tid; i < chunks; i += 256) {
        a += part[((size_t)i * 3) * C + c]; b += part[((size_t)i * 3 + 1) * C + c];
        if (dgbs) d += part[((size_t)i * 3 + 2) * C + c];
    }
    r0[tid] = a; r1[tid] = b; r2[tid] = d;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { r0[tid] += r0[tid + o]; r1[tid] += r1[tid + o]; r2[tid] += r2[tid + o]; }
        __syncthreads();
    }
    if (tid) return;
    dgb2[c] = (float)r1[0]; dgb2[C + c] = (float)r0[0]; dgb2[2 * C + c] = 0.f;
    if (dgbs) { dgbs[c] = (float)r2[0]; dgbs[C + c] = (float)r0[0]; dgbs[2 * C + c] = 0.f; }
}

// dy = gamma2 rstd2 (dp - dbeta / M - xhat2 dgamma2 / M); with a normalised shortcut dshort = the same with its own statistics,
// with a raw shortcut dshort = dp
__global__ void k_bn_bwd_apply2(const float* __restrict__ dz, const float* __restrict__ y, const float* __restrict__ shortcut,
                                const float* __restrict__ stats, const float* __restrict__ aff, const float* __restrict__ short_stats,
                                const float* __restrict__ short_aff, const float* __restrict__ dgb2, const float* __restrict__ dgbs, int C, long n4,
                                long rows, int act, float* __restrict__ dy, float* __restrict__ dshort) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    f32x4 d = *reinterpret_cast<const f32x4*>(dz + i * 4);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    f32x4 w = {0.f, 0.f, 0.f, 0.f};
    if (shortcut) w = *reinterpret_cast<const f32x4*>(shortcut + i * 4);
    const f32x4 m = *reinterpret_cast<const f32x4*>(stats + c), r = *reinterpret_cast<const f32x4*>(stats + C + c);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(aff + c), sh = *reinterpret_cast<const f32x4*>(aff + C + c);
    f32x4 scs = {0.f, 0.f, 0.f, 0.f}, shs = scs;
    if (short_aff) { scs = *reinterpret_cast<const f32x4*>(short_aff + c); shs = *reinterpret_cast<const f32x4*>(short_aff + C + c); }
    if (act) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = fmaf(v[e], sc[e], sh[e]) + (short_aff ? fmaf(w[e], scs[e], shs[e]) : w[e]);
            d[e] = p > 0.f ? d[e] : 0.01f * d[e];
        }
    }
    const float inv = 1.0f / (float)rows;
    const f32x4 dg = *reinterpret_cast<const f32x4*>(dgb2 + c), db = *reinterpret_cast<const f32x4*>(dgb2 + C + c);
    // (sc = gamma rstd)
    *reinterpret_cast<f32x4*>(dy + i * 4) = sc * (d - db * inv - (v - m) * r * dg * inv);
    if (dshort) {
        if (short_aff) {
            const f32x4 ms = *reinterpret_cast<const f32x4*>(short_stats + c), rs = *reinterpret_cast<const f32x4*>(short_stats + C + c);
            const f32x4 dgs = *reinterpret_cast<const f32x4*>(dgbs + c);
            *reinterpret_cast<f32x4*>(dshort + i * 4) = scs * (d - db * inv - (w - ms) * rs * dgs * inv);
        } else
            *reinterpret_cast<f32x4*>(dshort + i * 4) = d;
    }
}

// Everything a Linear's backward needs from dy [M][N] fp32 in one pass: the bf16 copy (operand of the data-gradient GEMM), its
// transpose [N][M] (operand of the weight-gradient GEMM) and per-64-row partial column sums part[M / 64][N] (the bias gradient is
// their sum over the first index - a fixed order) - three PyTorch launches over the full tensor (cast, transposed copy,
// reduction) per layer otherwise.  One block per 64 x 64 tile.  M % 64 == 0, N % 64 == 0.
// dy is read where the producer left it: row r of this Linear's output gradient = row r / row_div of a tensor of pitch `ld` floats (a column
// slice of a wider data gradient - the pieces of a torch.cat -, row_div > 1: the backward of an average pool over row_div consecutive rows,
// with cscale = 1 / row_div), times cscale, times rscale[r / rows_per_scale] (a residual branch's DropPath factor, a loss's per-sample weight).
__global__ __launch_bounds__(256) void k_linear_bwd_prep(const float* __restrict__ dy, int ld, int row_div, float cscale, int M, int N,
                                                         const float* __restrict__ rscale, int rows_per_scale, __bf16* __restrict__ dyb,
                                                         __bf16* __restrict__ dybT, float* __restrict__ part) {
    __shared__ __bf16 tile[64][66];          // [row][col], padded
    __shared__ float red[16][64];
    const int tid = threadIdx.x, c0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
    const int r4 = tid >> 4, q = tid & 15;   // 16 rows per pass x 16 float4 columns
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = p * 16 + r4;
        f32x4 v = *reinterpret_cast<const f32x4*>(dy + (size_t)((m0 + r) / row_div) * ld + c0 + 4 * q);
        float f = cscale;
        if (rscale) f *= rscale[(m0 + r) / rows_per_scale];
        v = v * f;
        sum = sum + v;
        const bf16x4 b = to_bf16x4(v);
        *reinterpret_cast<bf16x4*>(dyb + (size_t)(m0 + r) * N + c0 + 4 * q) = b;
        tile[r][4 * q] = b[0]; tile[r][4 * q + 1] = b[1]; tile[r][4 * q + 2] = b[2]; tile[r][4 * q + 3] = b[3];
    }
    if (part) { red[r4][4 * q] = sum[0]; red[r4][4 * q + 1] = sum[1]; red[r4][4 * q + 2] = sum[2]; red[r4][4 * q + 3] = sum[3]; }
    __syncthreads();
    {   // transposed store: thread -> (column c = tid / 4, 16 rows starting at 16 (tid % 4)): 32 contiguous bytes of dybT
        const int c = tid >> 2, rr = (tid & 3) * 16;
        bf16x8 o0, o1;
#pragma unroll
        for (int e = 0; e < 8; ++e) { o0[e] = tile[rr + e][c]; o1[e] = tile[rr + 8 + e][c]; }
        __bf16* dst = dybT + (size_t)(c0 + c) * M + m0 + rr;
        *reinterpret_cast<bf16x8*>(dst) = o0;
        *reinterpret_cast<bf16x8*>(dst + 8) = o1;
    }
    if (part && tid < 64) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += red[i][tid];
        part[(size_t)blockIdx.y * N + c0 + tid] = s;
    }
}

__global__ void k_gelu_fwd(const float* __restrict__ x, float* __restrict__ y, __bf16* __restrict__ yb, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    if (y) reinterpret_cast<f32x4*>(y)[i] = o;
    if (yb) reinterpret_cast<bf16x4*>(yb)[i] = to_bf16x4(o);
}
// Weight and bias gradient of an nn.Linear that saw only a few rows (the timestep MLP and embed_text: one row per clip, models/denoiser.py:92,
// 231-245): dW[n][k] = sum_m dy[m][n] x[m][k], M <= 64.  On the GEMM kernels this contraction over 32 rows was a chain of pads, transposes and packs
// (~8 launches) around a 97 %-empty MFMA; here a thread owns one k for 16 output features, dy rows ride in LDS, x rows are read coalesced.
__global__ __launch_bounds__(256) void k_linear_wgrad_rows(const float* __restrict__ dy, const __bf16* __restrict__ x, int M, int N, int K,
                                                           float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float dys[64][16];
    const int k = blockIdx.x * 256 + threadIdx.x, n0 = blockIdx.y * 16;
    for (int i = threadIdx.x; i < M * 16; i += 256) dys[i >> 4][i & 15] = dy[(size_t)(i >> 4) * N + n0 + (i & 15)];
    __syncthreads();
    if (db && blockIdx.x == 0 && threadIdx.x < 16) {
        float sacc = 0.f;
        for (int m = 0; m < M; ++m) sacc += dys[m][threadIdx.x];
        db[n0 + threadIdx.x] = sacc;
    }
    if (k >= K) return;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int m = 0; m < M; ++m) {
        const float xv = (float)x[(size_t)m * K + k];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(dys[m][i], xv, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dw[(size_t)(n0 + i) * K + k] = acc[i];
}

// Rotary position embedding on the hidden state (models/denoiser.py:178-186, 324-343): every token's 512 features are 8 groups of 64, a group's
// (u, v) = (first 32, last 32) turns by angle = position x inv_freq[j]: (u cos - v sin, v cos + u sin); inverse = the transposed rotation (its
// backward).  One thread per (token, group, 4 consecutive j): the reference's view / permute / cat / mul / add chain (14 launches each way) as one.
__global__ __launch_bounds__(256) void k_rotary(const float* __restrict__ x, const float* __restrict__ cs, const float* __restrict__ sn, long n_tok,
                                                int inverse, float* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;                  // (token, group, j4): 8 groups x 8 quads per token
    if (i >= n_tok * 64) return;
    const long tok = i >> 6;
    const int g = (int)(i >> 3) & 7, j4 = (int)i & 7, pos = (int)(tok & 31);
    const float* px = x + tok * 512 + g * 64 + 4 * j4;
    const f32x4 u = *reinterpret_cast<const f32x4*>(px), v = *reinterpret_cast<const f32x4*>(px + 32);
    const f32x4 c = *reinterpret_cast<const f32x4*>(cs + pos * 32 + 4 * j4);
    f32x4 s = *reinterpret_cast<const f32x4*>(sn + pos * 32 + 4 * j4);
    if (inverse) s = -s;
    float* py = y + tok * 512 + g * 64 + 4 * j4;
    *reinterpret_cast<f32x4*>(py) = u * c - v * s;
    *reinterpret_cast<f32x4*>(py + 32) = v * c + u * s;
}

__global__ void k_gelu_bwd(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i], d = reinterpret_cast<const f32x4*>(dy)[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float cdf = 0.5f * (1.0f + erff(v[e] * 0.70710678118654752440f));
        const float pdf = 0.3989422804014327f * __expf(-0.5f * v[e] * v[e]);
        o[e] = d[e] * (cdf + v[e] * pdf);
    }
    reinterpret_cast<f32x4*>(dx)[i] = o;
}

// ---- attention of one (sequence, head): 32 x 32 scores over 128 dims, fp32, straight from / to the packed qkv
//      tensor of the qkv Linear ([seq][t][3][4 heads][128]).  256 threads: thread = (query i = tid >> 3, 4 keys).
//      forward: o[seq][t][h*128 + d] = softmax(q k^T / sqrt(128)) v                 (transformer.py:83-104)
//      backward: recomputes p; dv = p^T do, dp = do v^T, ds = p (dp - sum_j dp p), dq = ds k / sqrt(d), dk = ds^T q / sqrt(d)
constexpr int kAT = 32, kAD = 128;
// (the first version read one float per FMA out of LDS and took 34 us per block of the model; the scores / dp loop now reads
// float4 rows - 10 reads per 32 FMAs - and the dq / dk / dv loop keeps 16 tokens x 3 accumulators per thread, its ds / p operands
// arriving as wave-uniform float4 broadcasts - 15 reads per 48 FMAs.)  Rows are padded to 132 / 36 floats: 16-byte aligned.
constexpr int kAPD = kAD + 4, kAPS = kAT + 4;
constexpr int kAttnBwd2Lds = (4 * kAT * kAPD + 3 * kAT * kAPS) * 4;              // 81 408 bytes
__global__ __launch_bounds__(256) void k_attn_bwd2(const float* __restrict__ qkv, const float* __restrict__ d_o, float* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) char smem_attn[];
    float (*q)[kAPD] = reinterpret_cast<float (*)[kAPD]>(smem_attn);
    float (*k)[kAPD] = q + kAT;
    float (*v)[kAPD] = k + kAT;
    float (*go)[kAPD] = v + kAT;
    float (*p)[kAPS] = reinterpret_cast<float (*)[kAPS]>(go + kAT);
    float (*ds)[kAPS] = p + kAT;
    float (*dsT)[kAPS] = ds + kAT;
    const int seq = blockIdx.x >> 2, head = blockIdx.x & 3, tid = threadIdx.x;
    for (int i = tid; i < kAT * (kAD / 4); i += 256) {
        const int t = i / (kAD / 4), d4 = i % (kAD / 4);
        const size_t o = ((size_t)(seq * kAT + t) * 3) * SYN_D + head * kAD + 4 * d4;
        *reinterpret_cast<f32x4*>(&q[t][4 * d4]) = *reinterpret_cast<const f32x4*>(qkv + o);
        *reinterpret_cast<f32x4*>(&k[t][4 * d4]) = *reinterpret_cast<const f32x4*>(qkv + o + SYN_D);
        *reinterpret_cast<f32x4*>(&v[t][4 * d4]) = *reinterpret_cast<const f32x4*>(qkv + o + 2 * SYN_D);
        *reinterpret_cast<f32x4*>(&go[t][4 * d4]) = *reinterpret_cast<const f32x4*>(d_o + (size_t)(seq * kAT + t) * SYN_D + head * kAD + 4 * d4);
    }
    __syncthreads();
    {   // scores and dp of (query i, keys j0 .. j0 + 3) in one sweep over d; softmax and ds over the 8 threads of a query
        const int i = tid >> 3, j0 = (tid & 7) * 4;
        float sc[4] = {0.f, 0.f, 0.f, 0.f}, dp[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d4 = 0; d4 < kAD / 4; ++d4) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(&q[i][4 * d4]), gv = *reinterpret_cast<const f32x4*>(&go[i][4 * d4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(&k[j0 + e][4 * d4]), vv = *reinterpret_cast<const f32x4*>(&v[j0 + e][4 * d4]);
#pragma unroll
                for (int c = 0; c < 4; ++c) { sc[e] = fmaf(qv[c], kv[c], sc[e]); dp[e] = fmaf(gv[c], vv[c], dp[e]); }
            }
        }
        float mx = -3.0e38f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] *= 0.08838834764831845f; mx = fmaxf(mx, sc[e]); }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] = __expf(sc[e] - mx); sum += sc[e]; }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) sum += __shfl_xor(sum, o);
        const float inv = 1.0f / sum;
        float dot = 0.f;
        f32x4 pv, dv4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { pv[e] = sc[e] * inv; dot = fmaf(dp[e], pv[e], dot); }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) dot += __shfl_xor(dot, o);
#pragma unroll
        for (int e = 0; e < 4; ++e) { dv4[e] = pv[e] * (dp[e] - dot) * 0.08838834764831845f; dsT[j0 + e][i] = dv4[e]; }
        *reinterpret_cast<f32x4*>(&p[i][j0]) = pv;
        *reinterpret_cast<f32x4*>(&ds[i][j0]) = dv4;
    }
    __syncthreads();
    {   // dq[t][d] = sum_j ds[t][j] k[j][d], dk[t][d] = sum_j ds[j][t] q[j][d], dv[t][d] = sum_j p[j][t] do[j][d]: thread = (d, 16 tokens)
        const int d = tid & (kAD - 1), t0 = (tid >> 7) * 16;
        float dq[16], dk[16], dv[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) dq[t] = dk[t] = dv[t] = 0.f;
        for (int j = 0; j < kAT; ++j) {
            const float kj = k[j][d], qj = q[j][d], gj = go[j][d];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&dsT[j][t0 + 4 * c]), b = *reinterpret_cast<const f32x4*>(&ds[j][t0 + 4 * c]);
                const f32x4 pc = *reinterpret_cast<const f32x4*>(&p[j][t0 + 4 * c]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dq[4 * c + e] = fmaf(a[e], kj, dq[4 * c + e]);
                    dk[4 * c + e] = fmaf(b[e], qj, dk[4 * c + e]);
                    dv[4 * c + e] = fmaf(pc[e], gj, dv[4 * c + e]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const size_t o = ((size_t)(seq * kAT + t0 + t) * 3) * SYN_D + head * kAD + d;
            dqkv[o] = dq[t]; dqkv[o + SYN_D] = dk[t]; dqkv[o + 2 * SYN_D] = dv[t];
        }
    }
}


// forward in the same style: o[t][d] = sum_j p[t][j] v[j][d] with p^T rows as wave-uniform float4 broadcasts
constexpr int kAttnFwd2Lds = (3 * kAT * kAPD + kAT * kAPS) * 4;                  // 55 296 bytes
__global__ __launch_bounds__(256) void k_attn_fwd2(const float* __restrict__ qkv, float* __restrict__ o, __bf16* __restrict__ ob) {
    extern __shared__ __attribute__((aligned(16))) char smem_attn[];
    float (*q)[kAPD] = reinterpret_cast<float (*)[kAPD]>(smem_attn);
    float (*k)[kAPD] = q + kAT;
    float (*v)[kAPD] = k + kAT;
    float (*pT)[kAPS] = reinterpret_cast<float (*)[kAPS]>(v + kAT);
    const int seq = blockIdx.x >> 2, head = blockIdx.x & 3, tid = threadIdx.x;
    for (int i = tid; i < kAT * (kAD / 4); i += 256) {
        const int t = i / (kAD / 4), d4 = i % (kAD / 4);
        const size_t off = ((size_t)(seq * kAT + t) * 3) * SYN_D + head * kAD + 4 * d4;
        *reinterpret_cast<f32x4*>(&q[t][4 * d4]) = *reinterpret_cast<const f32x4*>(qkv + off);
        *reinterpret_cast<f32x4*>(&k[t][4 * d4]) = *reinterpret_cast<const f32x4*>(qkv + off + SYN_D);
        *reinterpret_cast<f32x4*>(&v[t][4 * d4]) = *reinterpret_cast<const f32x4*>(qkv + off + 2 * SYN_D);
    }
    __syncthreads();
    {
        const int i = tid >> 3, j0 = (tid & 7) * 4;
        float sc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d4 = 0; d4 < kAD / 4; ++d4) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(&q[i][4 * d4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(&k[j0 + e][4 * d4]);
#pragma unroll
                for (int c = 0; c < 4; ++c) sc[e] = fmaf(qv[c], kv[c], sc[e]);
            }
        }
        float mx = -3.0e38f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] *= 0.08838834764831845f; mx = fmaxf(mx, sc[e]); }
#pragma unroll
        for (int s2 = 1; s2 < 8; s2 <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s2));
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] = __expf(sc[e] - mx); sum += sc[e]; }
#pragma unroll
        for (int s2 = 1; s2 < 8; s2 <<= 1) sum += __shfl_xor(sum, s2);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int e = 0; e < 4; ++e) pT[j0 + e][i] = sc[e] * inv;
    }
    __syncthreads();
    {
        const int d = tid & (kAD - 1), t0 = (tid >> 7) * 16;
        float acc[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.f;
        for (int j = 0; j < kAT; ++j) {
            const float vj = v[j][d];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&pT[j][t0 + 4 * c]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * c + e] = fmaf(a[e], vj, acc[4 * c + e]);
            }
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const size_t at = (size_t)(seq * kAT + t0 + t) * SYN_D + head * kAD + d;
            if (o) o[at] = acc[t];
            if (ob) ob[at] = (__bf16)acc[t];
        }
    }
}


// ---- optimizer step: clip_grad_norm_(max_norm) + Adam over a list of tensors (diffusion_rvqvae_trainer.py:351-356) ---------------------------------
// PyTorch runs this as _foreach_norm (2 launches) + stack / norm / clamp / reciprocal glue + _foreach_mul_ on the gradients (118 MB read and written)
// + the fused Adam (5 launches): 0.36 ms of the step at 29.6 M parameters.  Here: per-workgroup partial sums of g^2 (one read of the gradients), one
// workgroup that turns them into the step's scalars (total norm, clip factor, lr / bias corrections; the step count lives on the device), and the
// update with the clip factor applied to g as it is read - the gradients are not rewritten.  Pointers travel as kernel arguments (<= 64 tensors per
// launch), so a captured step holds them by value.  Deterministic: fixed chunking, fixed summation order.
constexpr int kOptMax = 64, kOptChunk = 8192;        // tensors per launch; elements per workgroup (256 threads x 8 float4)
struct OptList { float* p[kOptMax]; const float* g[kOptMax]; float* m[kOptMax]; float* v[kOptMax]; int numel[kOptMax]; int first[kOptMax + 1]; int n; };

__device__ __forceinline__ int opt_tensor_of(const OptList& L, int block) {          // first[t] <= block < first[t + 1]
    int lo = 0, hi = L.n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (L.first[mid] <= block) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(256) void k_opt_sqnorm(const OptList L, float* __restrict__ partials) {
    __shared__ float red[4];
    const int t = opt_tensor_of(L, blockIdx.x), n = L.numel[t];
    const long base = (long)(blockIdx.x - L.first[t]) * kOptChunk;
    const float* g = L.g[t];
    float s = 0.f;
    for (int i = threadIdx.x * 4; i < kOptChunk; i += 1024) {
        const long e = base + i;
        if (e + 3 < n && (reinterpret_cast<uintptr_t>(g + e) & 15) == 0) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(g + e);
            s += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
        } else {
            for (int q = 0; q < 4; ++q) if (e + q < n) s += g[e + q] * g[e + q];
        }
    }
    s = warp_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// scal[0] = clip factor (1 when max_norm <= 0), [1] = lr / (1 - beta1^step), [2] = 1 / sqrt(1 - beta2^step), [3] = total gradient norm; *step += 1 first
__global__ __launch_bounds__(256) void k_opt_scalars(const float* __restrict__ partials, int n_partials, float max_norm, const float* __restrict__ lr_dev,
                                                     float lr, float beta1, float beta2, float* __restrict__ step, float* __restrict__ scal) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x) return;
    const float total = (float)sqrt(red[0]);
    const float st = *step + 1.0f;
    *step = st;
    const float rate = lr_dev ? *lr_dev : lr;
    scal[0] = max_norm > 0.f ? fminf(max_norm / (total + 1e-6f), 1.0f) : 1.0f;        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
    scal[1] = rate / (1.0f - powf(beta1, st));
    scal[2] = 1.0f / sqrtf(1.0f - powf(beta2, st));
    scal[3] = total;
}

__global__ __launch_bounds__(256) void k_opt_adam(const OptList L, const float* __restrict__ scal, float beta1, float beta2, float eps, float wd) {
    const int t = opt_tensor_of(L, blockIdx.x), n = L.numel[t];
    const long base = (long)(blockIdx.x - L.first[t]) * kOptChunk;
    const float clip = scal[0], step_size = scal[1], inv_bc2 = scal[2];
    float* p = L.p[t]; const float* g = L.g[t]; float* m = L.m[t]; float* v = L.v[t];
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    auto one = [&](float pe, float ge, float& me, float& ve) {
        ge = ge * clip;
        if (wd != 0.f) ge = fmaf(wd, pe, ge);
        me = me + (1.0f - beta1) * (ge - me);                     // (torch's lerp form)
        ve = beta2 * ve + (1.0f - beta2) * ge * ge;
        return pe - step_size * me / (sqrtf(ve) * inv_bc2 + eps);
    };
    for (int i = threadIdx.x * 4; i < kOptChunk; i += 1024) {
        const long e = base + i;
        if (e >= n) break;
        if (vec && e + 3 < n) {
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + e), mv = *reinterpret_cast<const f32x4*>(m + e), vv = *reinterpret_cast<const f32x4*>(v + e);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) { float me = mv[q], ve = vv[q]; pv[q] = one(pv[q], gv[q], me, ve); mv[q] = me; vv[q] = ve; }
            *reinterpret_cast<f32x4*>(p + e) = pv; *reinterpret_cast<f32x4*>(m + e) = mv; *reinterpret_cast<f32x4*>(v + e) = vv;
        } else {
            for (int q = 0; q < 4 && e + q < n; ++q) { float me = m[e + q], ve = v[e + q]; p[e + q] = one(p[e + q], g[e + q], me, ve); m[e + q] = me; v[e + q] = ve; }
        }
    }
}

}  // namespace trn
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

// ---- training path: fp32 forward / backward of LayerNorm(512), GELU and the 32-token attention ---------------
int syn_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, void* y_bf16, float* mean, float* rstd, int32_t rows, void* stream) {
    if (!x || !gamma || !beta || (!y && !y_bf16) || !mean || !rstd || rows <= 0) return fail_msg("syn_ln_fwd: bad arguments");
    hipLaunchKernelGGL(trn::k_ln_fwd, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, (__bf16*)y_bf16, mean, rstd, rows);
    return launched("k_ln_fwd launch");
}

int syn_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* add, float* dx,
               float* dgamma, float* dbeta, float* scratch, int32_t rows, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !scratch || rows <= 0) return fail_msg("syn_ln_bwd: bad arguments");
    const int per = 16, nwg = (rows + per - 1) / per;             // scratch: [nwg][2][512] floats (16 rows per workgroup: 1024 rows = 64 workgroups;
                                                                  // with 64 rows the 16 workgroups walked their rows one dependent load after the other, 14 us)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(trn::k_ln_bwd, dim3(nwg), dim3(256), 0, s, dy, x, gamma, mean, rstd, add, dx, scratch, rows, per);
    hipLaunchKernelGGL(trn::k_colsum, dim3(4), dim3(256), 0, s, scratch, nwg, 2 * SYN_D, SYN_D, dgamma, dbeta);   // partials [p][dgamma | dbeta]
    return launched("k_ln_bwd launch");
}

int syn_gelu_fwd(const float* x, float* y, void* y_bf16, int64_t n, void* stream) {
    if (!x || (!y && !y_bf16) || n <= 0 || n % 4) return fail_msg("syn_gelu_fwd: n must be a positive multiple of 4");
    hipLaunchKernelGGL(trn::k_gelu_fwd, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (__bf16*)y_bf16, (size_t)(n / 4));
    return launched("k_gelu_fwd launch");
}

int syn_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream) {
    if (!x || !dy || !dx || n <= 0 || n % 4) return fail_msg("syn_gelu_bwd: n must be a positive multiple of 4");
    hipLaunchKernelGGL(trn::k_gelu_bwd, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, (size_t)(n / 4));
    return launched("k_gelu_bwd launch");
}

int syn_linear_wgrad_rows(const float* dy, const void* x_bf16, int32_t m_rows, int32_t n, int32_t k, float* dw, float* db, void* stream) {
    if (!dy || !x_bf16 || !dw || m_rows <= 0 || m_rows > 64 || n <= 0 || n % 16 || k <= 0)
        return fail_msg("syn_linear_wgrad_rows: 1 .. 64 rows, n a multiple of 16");
    hipLaunchKernelGGL(trn::k_linear_wgrad_rows, dim3((k + 255) / 256, n / 16), dim3(256), 0, (hipStream_t)stream, dy, (const __bf16*)x_bf16, m_rows, n, k, dw, db);
    return launched("k_linear_wgrad_rows launch");
}

int32_t syn_bn_chunks(int64_t rows) { const int cr = trn::bn_chunk_rows((long)rows); return (int32_t)((rows + cr - 1) / cr); }

int syn_bn_act_fwd(const float* y, const float* shortcut, int64_t rows, int32_t channels, const float* gamma, const float* beta, float eps,
                   float momentum, float* run_mean, float* run_var, const float* conv_bias, int32_t act, float* ws, int32_t ws_chunks, float* stats,
                   float* z, void* stream) {
    if (!y || !gamma || !beta || !ws || !stats || !z || rows <= 0 || channels <= 0 || channels % 4 || 256 % (channels / 4) || channels > 1024)
        return fail_msg("syn_bn_act_fwd: need channels in {4 .. 1024} with channels / 4 dividing 256, rows > 0, non-null pointers");
    hipStream_t s = (hipStream_t)stream;
    // ws_chunks > 0: ws already holds that many [2][channels] partial sums (written by the convolution's epilogue, syn_conv1d_train_fwd)
    const int chunks = ws_chunks > 0 ? ws_chunks : syn_bn_chunks(rows);
    if (ws_chunks <= 0) hipLaunchKernelGGL(trn::k_bn_stats, dim3(chunks), dim3(256), 0, s, y, (long)rows, channels, ws);
    hipLaunchKernelGGL(trn::k_bn_finalize, dim3(channels), dim3(256), 0, s, (const float*)ws, chunks, channels, (long)rows, eps, momentum,
                       stats, run_mean, run_var, conv_bias);
    const long n4 = rows * channels / 4;
    hipLaunchKernelGGL(trn::k_bn_apply, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, y, shortcut, (const float*)stats, gamma, beta, channels, n4,
                       act, z);
    return launched("syn_bn_act_fwd");
}

int syn_bn_act_bwd(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta, int64_t rows,
                   int32_t channels, int32_t act, float* ws, float* dgamma_dbeta, float* dy, float* dshortcut, void* stream) {
    if (!dz || !y || !stats || !gamma || !ws || !dgamma_dbeta || !dy || rows <= 0 || channels % 4 || 256 % (channels / 4))
        return fail_msg("syn_bn_act_bwd: bad arguments");
    if (act && !z && (dshortcut || !beta)) return fail_msg("syn_bn_act_bwd: z may only be omitted (with beta given) when no shortcut entered the activation");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = syn_bn_chunks(rows);
    hipLaunchKernelGGL(trn::k_bn_bwd_stats, dim3(chunks), dim3(256), 0, s, dz, z, y, stats, gamma, beta, (long)rows, channels, act, ws);
    hipLaunchKernelGGL(trn::k_bn_bwd_finalize, dim3(channels), dim3(256), 0, s, (const float*)ws, chunks, channels, dgamma_dbeta);
    const long n4 = rows * channels / 4;
    hipLaunchKernelGGL(trn::k_bn_bwd_apply, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dz, z, y, stats, gamma, beta, (const float*)dgamma_dbeta,
                       channels, n4, (long)rows, act, dy, dshortcut);
    return launched("syn_bn_act_bwd");
}

/* ---- the fused tail of a BasicBlock: statistics -> per-channel affine; one elementwise pass per block and direction ---- */
static bool bn_shape_ok(int64_t rows, int32_t channels) { return rows > 0 && channels > 0 && channels % 4 == 0 && 256 % (channels / 4) == 0 && channels <= 1024; }

int syn_bn_finalize(const float* part, int32_t chunks, int64_t rows, int32_t channels, const float* gamma, const float* beta, float eps, float momentum,
                    float* run_mean, float* run_var, const float* conv_bias, float* stats, float* affine, void* stream) {
    if (!part || chunks <= 0 || !gamma || !beta || !stats || !affine || !bn_shape_ok(rows, channels)) return fail_msg("syn_bn_finalize: bad arguments");
    hipLaunchKernelGGL(trn::k_bn_finalize_aff, dim3(channels), dim3(256), 0, (hipStream_t)stream, part, chunks, channels, (long)rows, eps, momentum, gamma, beta,
                       stats, affine, run_mean, run_var, conv_bias);
    return launched("syn_bn_finalize");
}

int syn_bn_finalize_pair(const syn_bn_finalize_job* a, const syn_bn_finalize_job* b, void* stream) {
    if (!a || !b) return fail_msg("syn_bn_finalize_pair: two jobs");
    trn::FinJob j[2];
    const syn_bn_finalize_job* q[2] = {a, b};
    for (int i = 0; i < 2; ++i) {
        if (!q[i]->part || q[i]->chunks <= 0 || !q[i]->gamma || !q[i]->beta || !q[i]->stats || !q[i]->affine || !bn_shape_ok(q[i]->rows, q[i]->channels))
            return fail_msg("syn_bn_finalize_pair: bad arguments");
        j[i].part = q[i]->part; j[i].chunks = q[i]->chunks; j[i].C = q[i]->channels; j[i].rows = (long)q[i]->rows; j[i].eps = q[i]->eps; j[i].momentum = q[i]->momentum;
        j[i].gamma = q[i]->gamma; j[i].beta = q[i]->beta; j[i].stats = q[i]->stats; j[i].aff = q[i]->affine;
        j[i].run_mean = q[i]->run_mean; j[i].run_var = q[i]->run_var; j[i].conv_bias = q[i]->conv_bias;
    }
    hipLaunchKernelGGL(trn::k_bn_finalize_aff2, dim3(j[0].C + j[1].C), dim3(256), 0, (hipStream_t)stream, j[0], j[1]);
    return launched("syn_bn_finalize_pair");
}

int syn_bn_apply2(const float* y, const float* affine, const float* shortcut, const float* short_affine, int64_t rows, int32_t channels, int32_t act,
                  float* z, void* stream) {
    if (!y || !affine || !z || !bn_shape_ok(rows, channels) || (short_affine && !shortcut)) return fail_msg("syn_bn_apply2: bad arguments");
    const long n4 = rows * channels / 4;
    hipLaunchKernelGGL(trn::k_bn_apply2, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, affine, shortcut, short_affine, channels, n4, act, z);
    return launched("syn_bn_apply2");
}

int syn_bn_block_bwd(const float* dz, const float* y, const float* shortcut, const float* stats, const float* affine, const float* short_stats,
                     const float* short_affine, int64_t rows, int32_t channels, int32_t act, float* ws, float* dgb, float* short_dgb, float* dy,
                     float* dshortcut, void* stream) {
    if (!dz || !y || !stats || !affine || !ws || !dgb || !bn_shape_ok(rows, channels)) return fail_msg("syn_bn_block_bwd: bad arguments");
    if (!dy && dshortcut) return fail_msg("syn_bn_block_bwd: dy NULL (statistics and dgamma / dbeta only) takes no dshortcut either");
    if ((short_affine != nullptr) != (short_stats != nullptr) || (short_affine && (!shortcut || !short_dgb || (dy && !dshortcut))))
        return fail_msg("syn_bn_block_bwd: a normalised shortcut needs its tensor, statistics, affine, gradient buffer and dshortcut");
    if (dshortcut && !shortcut) return fail_msg("syn_bn_block_bwd: dshortcut without a shortcut");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = syn_bn_chunks(rows);
    hipLaunchKernelGGL(trn::k_bn_bwd_stats2, dim3(chunks), dim3(256), 0, s, dz, y, shortcut, stats, affine, short_stats, short_affine, (long)rows, channels, act, ws);
    hipLaunchKernelGGL(trn::k_bn_bwd_finalize2, dim3(channels), dim3(256), 0, s, (const float*)ws, chunks, channels, dgb, short_affine ? short_dgb : nullptr);
    const long n4 = rows * channels / 4;
    if (dy)                                                   // (dy NULL: the caller's next kernel forms dy / dshortcut itself - syn_conv1d_first_wgrad_tail)
        hipLaunchKernelGGL(trn::k_bn_bwd_apply2, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dz, y, shortcut, stats, affine, short_stats, short_affine,
                           (const float*)dgb, (const float*)short_dgb, channels, n4, (long)rows, act, dy, dshortcut);
    return launched("syn_bn_block_bwd");
}

/* ---- nn.SyncBatchNorm on the same kernels: sums -> (the caller's all-reduce) -> apply ---- */
int syn_bn_sums(const float* y, int64_t rows, int32_t channels, float* ws, int32_t ws_chunks, double* sums, void* stream) {
    if (!ws || !sums || rows <= 0 || channels <= 0 || channels % 4 || 256 % (channels / 4) || channels > 1024 || (ws_chunks <= 0 && !y))
        return fail_msg("syn_bn_sums: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = ws_chunks > 0 ? ws_chunks : syn_bn_chunks(rows);
    if (ws_chunks <= 0) hipLaunchKernelGGL(trn::k_bn_stats, dim3(chunks), dim3(256), 0, s, y, (long)rows, channels, ws);
    hipLaunchKernelGGL(trn::k_bn_sums64, dim3(channels), dim3(256), 0, s, (const float*)ws, chunks, channels, sums);
    return launched("syn_bn_sums");
}

int syn_bn_act_apply(const float* y, const float* shortcut, int64_t rows, int64_t rows_total, int32_t channels, const float* gamma, const float* beta,
                     float eps, float momentum, float* run_mean, float* run_var, const float* conv_bias, int32_t act, const double* sums_total,
                     float* stats, float* z, void* stream) {
    if (!y || !gamma || !beta || !sums_total || !stats || !z || rows <= 0 || rows_total < rows || channels <= 0 || channels % 4)
        return fail_msg("syn_bn_act_apply: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(trn::k_bn_finalize64, dim3((channels + 255) / 256), dim3(256), 0, s, sums_total, channels, (long)rows_total, eps, momentum, stats,
                       run_mean, run_var, conv_bias);
    const long n4 = rows * channels / 4;
    hipLaunchKernelGGL(trn::k_bn_apply, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, y, shortcut, (const float*)stats, gamma, beta, channels, n4,
                       act, z);
    return launched("syn_bn_act_apply");
}

int syn_bn_bwd_sums(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta, int64_t rows,
                    int32_t channels, int32_t act, float* ws, double* sums, void* stream) {
    if (!dz || !y || !stats || !gamma || !ws || !sums || rows <= 0 || channels % 4 || 256 % (channels / 4))
        return fail_msg("syn_bn_bwd_sums: bad arguments");
    if (act && !z && !beta) return fail_msg("syn_bn_bwd_sums: z may only be omitted with beta given");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = syn_bn_chunks(rows);
    hipLaunchKernelGGL(trn::k_bn_bwd_stats, dim3(chunks), dim3(256), 0, s, dz, z, y, stats, gamma, beta, (long)rows, channels, act, ws);
    hipLaunchKernelGGL(trn::k_bn_sums64, dim3(channels), dim3(256), 0, s, (const float*)ws, chunks, channels, sums);
    return launched("syn_bn_bwd_sums");
}

int syn_bn_act_bwd_apply(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta,
                         const double* sums_local, const double* sums_total, int64_t rows, int64_t rows_total, int32_t channels, int32_t act,
                         float* dgamma_dbeta, float* scratch, float* dy, float* dshortcut, void* stream) {
    if (!dz || !y || !stats || !gamma || !sums_local || !sums_total || !dgamma_dbeta || !scratch || !dy || rows <= 0 || rows_total < rows || channels % 4)
        return fail_msg("syn_bn_act_bwd_apply: bad arguments");
    if (act && !z && (dshortcut || !beta)) return fail_msg("syn_bn_act_bwd_apply: z may only be omitted (with beta given) when no shortcut entered the activation");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(trn::k_bn_bwd_unpack64, dim3((channels + 255) / 256), dim3(256), 0, s, sums_local, sums_total, channels, dgamma_dbeta, scratch);
    const long n4 = rows * channels / 4;
    hipLaunchKernelGGL(trn::k_bn_bwd_apply, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dz, z, y, stats, gamma, beta, (const float*)scratch,
                       channels, n4, (long)rows_total, act, dy, dshortcut);
    return launched("syn_bn_act_bwd_apply");
}

int syn_linear_bwd_prep(const float* dy, int32_t ld, int32_t row_div, float const_scale, int32_t m_rows, int32_t n, const float* row_scale,
                        int32_t rows_per_scale, void* dy_bf16, void* dy_bf16_t, float* colsum_part, void* stream) {
    if (!dy || !dy_bf16 || !dy_bf16_t || m_rows <= 0 || n <= 0 || m_rows % 64 || n % 64 || (row_scale && rows_per_scale <= 0) || ld < n || ld % 4 || row_div < 1)
        return fail_msg("syn_linear_bwd_prep: need m_rows % 64 == 0, n % 64 == 0, ld >= n, ld % 4 == 0, row_div >= 1 and non-null pointers");
    hipLaunchKernelGGL(trn::k_linear_bwd_prep, dim3(n / 64, m_rows / 64), dim3(256), 0, (hipStream_t)stream, dy, ld, row_div, const_scale, m_rows, n, row_scale,
                       rows_per_scale, (__bf16*)dy_bf16, (__bf16*)dy_bf16_t, colsum_part);
    return launched("k_linear_bwd_prep launch");
}

// ---- optimizer step (clip + Adam) over lists of <= 64 tensors ------------------------------------------------------------------------------------
static int opt_fill(trn::OptList& L, const syn_opt_list* l, const char* who) {
    static_assert(SYN_OPT_MAX == trn::kOptMax, "include/syn_hip.h: tensors per optimizer list");
    if (!l || l->n <= 0 || l->n > SYN_OPT_MAX) return fail_msg(who);
    int blocks = 0;
    for (int i = 0; i < l->n; ++i) {
        if (!l->g[i] || l->numel[i] <= 0) return fail_msg(who);
        L.p[i] = l->p[i]; L.g[i] = l->g[i]; L.m[i] = l->m[i]; L.v[i] = l->v[i]; L.numel[i] = l->numel[i];
        L.first[i] = blocks;
        blocks += (l->numel[i] + trn::kOptChunk - 1) / trn::kOptChunk;
    }
    L.first[l->n] = blocks; L.n = l->n;
    return 0;
}

int32_t syn_opt_blocks(const syn_opt_list* l) {
    if (!l || l->n <= 0 || l->n > SYN_OPT_MAX) return -1;
    int blocks = 0;
    for (int i = 0; i < l->n; ++i) blocks += (l->numel[i] + trn::kOptChunk - 1) / trn::kOptChunk;
    return blocks;
}

int syn_opt_sqnorm(const syn_opt_list* l, float* partials, void* stream) {
    trn::OptList L;
    if (!partials) return fail_msg("syn_opt_sqnorm: partials is NULL");
    if (int rc = opt_fill(L, l, "syn_opt_sqnorm: need 1 .. 64 tensors with gradients")) return rc;
    hipLaunchKernelGGL(trn::k_opt_sqnorm, dim3(L.first[L.n]), dim3(256), 0, (hipStream_t)stream, L, partials);
    return launched("k_opt_sqnorm launch");
}

int syn_opt_scalars(const float* partials, int32_t n_partials, float max_norm, const float* lr_dev, float lr, float beta1, float beta2, float* step_dev,
                    float* scal4, void* stream) {
    if ((n_partials > 0 && !partials) || n_partials < 0 || !step_dev || !scal4) return fail_msg("syn_opt_scalars: bad arguments");
    hipLaunchKernelGGL(trn::k_opt_scalars, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, max_norm, lr_dev, lr, beta1, beta2, step_dev, scal4);
    return launched("k_opt_scalars launch");
}

int syn_opt_adam(const syn_opt_list* l, const float* scal4, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    trn::OptList L;
    if (!scal4) return fail_msg("syn_opt_adam: scal4 is NULL");
    if (int rc = opt_fill(L, l, "syn_opt_adam: need 1 .. 64 tensors")) return rc;
    for (int i = 0; i < L.n; ++i) if (!L.p[i] || !L.m[i] || !L.v[i]) return fail_msg("syn_opt_adam: null parameter / moment pointer");
    hipLaunchKernelGGL(trn::k_opt_adam, dim3(L.first[L.n]), dim3(256), 0, (hipStream_t)stream, L, scal4, beta1, beta2, eps, weight_decay);
    return launched("k_opt_adam launch");
}

int syn_attn_fwd(const float* qkv, float* o, void* o_bf16, int32_t n_seq, void* stream) {
    if (!qkv || (!o && !o_bf16) || n_seq <= 0) return fail_msg("syn_attn_fwd: bad arguments");
    hipLaunchKernelGGL(trn::k_attn_fwd2, dim3(n_seq * SYN_HEADS), dim3(256), trn::kAttnFwd2Lds, (hipStream_t)stream, qkv, o, (__bf16*)o_bf16);
    return launched("k_attn_fwd launch");
}

int syn_attn_bwd(const float* qkv, const float* d_o, float* dqkv, int32_t n_seq, void* stream) {
    if (!qkv || !d_o || !dqkv || n_seq <= 0) return fail_msg("syn_attn_bwd: bad arguments");
    static OncePerDevice once;
    if (once.first()) allow_lds(trn::k_attn_bwd2, trn::kAttnBwd2Lds);
    hipLaunchKernelGGL(trn::k_attn_bwd2, dim3(n_seq * SYN_HEADS), dim3(256), trn::kAttnBwd2Lds, (hipStream_t)stream, qkv, d_o, dqkv);
    return launched("k_attn_bwd launch");
}

// backward statistics of a BatchNorm (+ activation) alone - dgamma_dbeta [3][channels] - for a consumer that forms dy itself (syn_conv1d_first_wgrad_bn)
int syn_bn_bwd_stats(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta, int64_t rows,
                     int32_t channels, int32_t act, float* ws, float* dgamma_dbeta, void* stream) {
    if (!dz || !y || !stats || !gamma || !ws || !dgamma_dbeta || rows <= 0 || channels % 4 || 256 % (channels / 4)) return fail_msg("syn_bn_bwd_stats: bad arguments");
    if (act && !z && !beta) return fail_msg("syn_bn_bwd_stats: without z the activation's sign is recomputed and needs beta");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = syn_bn_chunks(rows);
    hipLaunchKernelGGL(trn::k_bn_bwd_stats, dim3(chunks), dim3(256), 0, s, dz, z, y, stats, gamma, beta, (long)rows, channels, act, ws);
    hipLaunchKernelGGL(trn::k_bn_bwd_finalize, dim3(channels), dim3(256), 0, s, (const float*)ws, chunks, channels, dgamma_dbeta);
    return launched("syn_bn_bwd_stats");
}

}  // extern "C"
