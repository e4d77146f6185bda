// Gradient-guided sampling (diffusion/gaussian_diffusion.py:427-503, 549-605, 765-848): the two ends of the denoiser that touch x_t, and the
// update that follows the user's cond_fn.  The eight blocks between them are syn_train_stack_fwd / _bwd (DESIGN.md 19).
//
// x_t enters the model through one affine map, h0 = rotary(x_t^T A^T + cond + TE[t]) (conditioning.fold_input_stage), so
//   k_guide_in_fwd   reads x (B, C, 1, T) fp32 as it lies - the loader transposes and rounds to bf16 into the swizzled LDS image the GEMM loops
//                    of this file read - multiplies by the packed A, starts the accumulators from cond + TE[t] and applies the rotary embedding
//                    in the epilogue (EPI_IN's arithmetic): h0 [32 n_seq][512] fp32, one launch;
//   k_guide_in_bwd   the adjoint: the loader applies the inverse rotation to dh0, the GEMM runs against the packed A^T with the operands swapped,
//                    so that a lane holds four consecutive frames of one channel, and dx (B, C, 1, T) is written (or added to) with 16-byte stores.
// One workgroup per sequence (32 rows) and 512 output columns; the sequence's rows stay in the LDS for the whole K loop: `staged_prime` / `staged_loop`, the
// very loop gemm_mainloop_resident runs, behind loaders of their own.  No atomics: a dx element has one owner, `accumulate` is a read-modify-write by that owner.
namespace {
namespace guide {

constexpr int kRows = 32;                 // rows of a workgroup: one sequence
constexpr int kTile = kRows * 128;        // bytes of one 64-column K tile of the LDS image
constexpr int kFwdLds = (SYN_C / kKT) * kTile, kBwdLds = (kNT / kKT) * kTile;

struct InFwd {
    const float* x; int n_x;              // (n_x, 1536, 1, 32): sequence s reads clip s % n_x (the variants of a clip share its latent)
    const uint4* A;                       // packed A [512][1536]
    const float* cond; const float* te; int n_te; const int* t_model;
    const float* rcos; const float* rsin;
    int n_live;                           // sequences >= n_live are padding: their rows of h0 are zero
    float* h0;
};

__global__ __launch_bounds__(kThreads) void k_guide_in_fwd(const InFwd a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MF = kRows / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    const int s = blockIdx.x, m0 = s * kRows;
    if (s >= a.n_live) {                  // (block-uniform)
        for (int i = tid; i < kRows * kNT / 4; i += kThreads) reinterpret_cast<f32x4*>(a.h0 + (size_t)m0 * kNT)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const uint4* Wq = a.A + ((size_t)(wave * 4) * (SYN_C / 32)) * 64 + lane;
    uint4 w[8][4];
    staged_prime<4, 8>(w, Wq, SYN_C / 32);                      // (the first weight fragments travel while x is staged)
    // x[c][t] -> bf16 rows [t][c]: a thread takes 8 channels of one frame; consecutive lanes take consecutive frames (128-byte runs per channel)
    const float* xs = a.x + (size_t)(s % a.n_x) * (SYN_C * SYN_T);
#pragma unroll 4
    for (int idx = tid; idx < kRows * (SYN_C / 8); idx += kThreads) {
        const int row = idx & 31, slot8 = idx >> 5, kt = slot8 >> 3, slot = slot8 & 7;
        const float* src = xs + (size_t)slot8 * 8 * SYN_T + row;
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (__bf16)src[e * SYN_T];
        *reinterpret_cast<bf16x8*>(smem + kt * kTile + row * 128 + ((slot ^ (row & 7)) << 4)) = v;
    }
    // accumulators start from the additive terms: the clip's conditioning row and the timestep's row of the time table
    f32x4 acc[4][MF];
    int ts = a.t_model[s];
    ts = ts < 0 ? 0 : (ts >= a.n_te ? a.n_te - 1 : ts);
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int m = m0 + mf * 16 + lr;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = wave * 64 + nf * 16 + g * 4;
            acc[nf][mf] = *reinterpret_cast<const f32x4*>(a.cond + (size_t)m * kNT + n) + *reinterpret_cast<const f32x4*>(a.te + (size_t)ts * kNT + n);
        }
    }
    __syncthreads();
    staged_loop<kRows, 4, 8, false>(acc, w, SYN_C / 32, Wq, smem);
    // rotary on the (j, j + 32) pairs of this wave's 64-wide group (models/denoiser.py:178-186): fragments 0, 1 hold j < 32, fragments 2, 3 j + 32
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int pos = mf * 16 + lr, m = m0 + pos;
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
            const int j = nf * 16 + g * 4;
            rotary4(acc[nf][mf], acc[nf + 2][mf], *reinterpret_cast<const f32x4*>(a.rcos + pos * 32 + j), *reinterpret_cast<const f32x4*>(a.rsin + pos * 32 + j));
        }
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) *reinterpret_cast<f32x4*>(a.h0 + (size_t)m * kNT + wave * 64 + nf * 16 + g * 4) = acc[nf][mf];
    }
}

struct InBwd {
    const float* dh0;                     // [32 n_seq][512]
    const uint4* At;                      // packed A^T [1536][512]
    const float* rcos; const float* rsin;
    float* dx; int accumulate;            // (n_seq, 1536, 1, 32)
};

__global__ __launch_bounds__(kThreads) void k_guide_in_bwd(const InBwd a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MF = kRows / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    const int s = blockIdx.x, chunk = blockIdx.y, m0 = s * kRows;
    const uint4* Wq = a.At + ((size_t)(chunk * 32 + wave * 4) * (kNT / 32)) * 64 + lane;
    uint4 wr[8][4];
    staged_prime<4, 8>(wr, Wq, kNT / 32);
    // the rotation's adjoint on the way in: (u, w) <- (u cos + w sin, w cos - u sin), then bf16 into the image
#pragma unroll
    for (int idx = tid; idx < kRows * 64; idx += kThreads) {
        const int j4 = idx & 7, grp = (idx >> 3) & 7, row = idx >> 6;
        const float* src = a.dh0 + (size_t)(m0 + row) * kNT + grp * 64 + j4 * 4;
        const f32x4 u = *reinterpret_cast<const f32x4*>(src), w = *reinterpret_cast<const f32x4*>(src + 32);
        const f32x4 cs = *reinterpret_cast<const f32x4*>(a.rcos + row * 32 + j4 * 4), sn = *reinterpret_cast<const f32x4*>(a.rsin + row * 32 + j4 * 4);
        f32x4 du, dw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            du[e] = __builtin_fmaf(u[e], cs[e], __fmul_rn(w[e], sn[e]));
            dw[e] = __builtin_fmaf(w[e], cs[e], -__fmul_rn(u[e], sn[e]));
        }
        char* base = smem + grp * kTile + row * 128 + (j4 & 1) * 8;
        *reinterpret_cast<bf16x4*>(base + (((j4 >> 1) ^ (row & 7)) << 4)) = to_bf16x4(du);
        *reinterpret_cast<bf16x4*>(base + (((4 + (j4 >> 1)) ^ (row & 7)) << 4)) = to_bf16x4(dw);
    }
    f32x4 acc[4][MF];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    staged_loop<kRows, 4, 8, true>(acc, wr, kNT / 32, Wq, smem);
    // acc[nf][mf] = four consecutive frames 16 mf + 4 g .. + 3 of channel n: one 16-byte store into the channel-major latent
    float* out = a.dx + (size_t)s * (SYN_C * SYN_T);
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
        const int n = chunk * kNT + wave * 64 + nf * 16 + lr;
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            f32x4* p = reinterpret_cast<f32x4*>(out + (size_t)n * SYN_T + mf * 16 + g * 4);
            *p = a.accumulate ? *p + acc[nf][mf] : acc[nf][mf];
        }
    }
}

// The arithmetic behind cond_fn's gradient g, element-wise on (B, C, 1, T).  One row of 8 floats per timestep:
//   mode 0 (condition_mean + p_sample, :427-455, :556)  {variance, exp(0.5 log_variance)}:  sample = a + variance g + [t != 0] sigma noise, a = the posterior mean
//   mode 1 (condition_score + ddim_sample, :457-503, :772-790)  {sqrt(1 - ab), sqrt(1 / ab), sqrt(1 / ab - 1), sqrt(ab_prev), sqrt(1 - ab_prev - sigma^2), sigma}:
//          eps = (r a - x0) / m - sqrt(1 - ab) g;  x0' = r a - m eps;  eps' = (r a - x0') / m;  sample = x0' sqrt(ab_prev) + dir eps' + [t != 0] sigma noise, a = x_t
// Noise: read (channel-major like everything else), or drawn: element (clip b, frame t, channel c) is element ((first_clip + b) 32 + t) 1536 + c of
// syn_randn(seed, stream_id = t_idx[b]) - the step kernels' draw.  A thread owns four consecutive channels of one frame (one randn4) and consecutive
// lanes own consecutive frames: every load and store of a wave is 128-byte runs.  Rows with t == 0, or sigma == 0, neither read nor draw noise.
struct Upd { int mode; const float* a; const float* x0; const float* g; const float* noise; int draw; unsigned long long seed, first_clip;
             const float* coef; int n_rows; const int* t_idx; int n_clips; float* out; };

__global__ __launch_bounds__(256) void k_guide_update(const Upd u) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)u.n_clips * (SYN_C / 4) * SYN_T) return;
    const int t = (int)(idx & 31), c4 = (int)((idx >> 5) % (SYN_C / 4)), b = (int)(idx / ((SYN_C / 4) * SYN_T));
    const size_t off = ((size_t)b * SYN_C + c4 * 4) * SYN_T + t;
    const int ti = u.t_idx[b];
    f32x4 r;
    if (ti < 0 || ti >= u.n_rows) {                       // an index outside the table: NaN, nothing else is read
        const float q = __builtin_nanf("");
        r = f32x4{q, q, q, q};
    } else {
        const float* cf = u.coef + (size_t)ti * 8;
        const float sigma = u.mode == 0 ? cf[1] : cf[5];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const bool noisy = ti != 0 && sigma != 0.f;
        if (noisy) {
            if (u.noise) {
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = u.noise[off + e * SYN_T];
            } else if (u.draw) {
                z = randn4(u.seed, (uint64_t)ti, (((u.first_clip + (uint64_t)b) * SYN_T + t) * (uint64_t)SYN_C + c4 * 4) >> 2);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float av = u.a[off + e * SYN_T], gv = u.g[off + e * SYN_T];
            float v;
            if (u.mode == 0) {
                v = av + nopk(cf[0] * gv);                        // torch's two roundings (condition_mean).  The product passes through an opaque no-op:
                                                                  // hipcc contracts `a + b * c` to an fma, through __fmul_rn as well (it is a plain `*` there)
            } else {
                const float x0 = u.x0[off + e * SYN_T], rx = cf[1] * av;
                const float eps = (rx - x0) / cf[2] - cf[0] * gv;
                const float x0g = rx - cf[2] * eps;
                const float eps2 = (rx - x0g) / cf[2];
                v = x0g * cf[3] + cf[4] * eps2;
            }
            r[e] = noisy ? v + nopk(sigma * z[e]) : v;            // p_sample's `mean + (nonzero sigma) noise`: product and sum rounded apart, as torch's two kernels do
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) u.out[off + e * SYN_T] = r[e];
}

}  // namespace guide
}  // namespace

extern "C" {

int syn_guide_in_fwd(const float* x_bct, int32_t n_x, const void* a_packed, const float* cond, const float* te, int32_t n_te, const int32_t* t_model,
                     const float* rot_cos, const float* rot_sin, int32_t n_live, int32_t n_seq, float* h0, void* stream) {
    if (!x_bct || !a_packed || !cond || !te || !t_model || !rot_cos || !rot_sin || !h0 || n_te <= 0)
        return fail_msg("syn_guide_in_fwd: null pointer or empty time table");
    if (n_seq < 1 || n_seq > 65535 || n_live < 1 || n_live > n_seq || n_x < 1 || n_x > n_live)
        return fail_msg("syn_guide_in_fwd: 1 <= n_x <= n_live <= n_seq <= 65535");
    if (((uintptr_t)x_bct | (uintptr_t)cond | (uintptr_t)te | (uintptr_t)rot_cos | (uintptr_t)rot_sin | (uintptr_t)h0 | (uintptr_t)a_packed) & 15)
        return fail_msg("syn_guide_in_fwd: operands must be 16-byte aligned");
    static OncePerDevice once;
    if (once.first()) { allow_lds(guide::k_guide_in_fwd, guide::kFwdLds); }
    guide::InFwd a;
    a.x = x_bct; a.n_x = n_x; a.A = (const uint4*)a_packed; a.cond = cond; a.te = te; a.n_te = n_te; a.t_model = (const int*)t_model;
    a.rcos = rot_cos; a.rsin = rot_sin; a.n_live = n_live; a.h0 = h0;
    hipLaunchKernelGGL(guide::k_guide_in_fwd, dim3(n_seq), dim3(kThreads), guide::kFwdLds, (hipStream_t)stream, a);
    return launched("k_guide_in_fwd launch");
}

int syn_guide_in_bwd(const float* dh0, const void* at_packed, const float* rot_cos, const float* rot_sin, int32_t n_seq, int32_t accumulate, float* dx_bct,
                     void* stream) {
    if (!dh0 || !at_packed || !rot_cos || !rot_sin || !dx_bct) return fail_msg("syn_guide_in_bwd: null pointer");
    if (n_seq < 1 || n_seq > 65535) return fail_msg("syn_guide_in_bwd: 1 <= n_seq <= 65535");
    if (((uintptr_t)dh0 | (uintptr_t)at_packed | (uintptr_t)rot_cos | (uintptr_t)rot_sin | (uintptr_t)dx_bct) & 15)
        return fail_msg("syn_guide_in_bwd: operands must be 16-byte aligned");
    guide::InBwd a;
    a.dh0 = dh0; a.At = (const uint4*)at_packed; a.rcos = rot_cos; a.rsin = rot_sin; a.dx = dx_bct; a.accumulate = accumulate != 0;
    hipLaunchKernelGGL(guide::k_guide_in_bwd, dim3(n_seq, SYN_C / kNT), dim3(kThreads), guide::kBwdLds, (hipStream_t)stream, a);
    return launched("k_guide_in_bwd launch");
}

int syn_guide_update(int32_t mode, const float* a, const float* pred_x0, const float* grad, const float* noise, int32_t draw, uint64_t seed,
                     uint64_t first_clip, const float* coef, int32_t n_rows, const int32_t* t_idx, int32_t n_clips, float* out, void* stream) {
    if (!a || !grad || !coef || !t_idx || !out || n_rows <= 0 || n_clips <= 0 || mode < 0 || mode > 1 || (mode == 1 && !pred_x0))
        return fail_msg("syn_guide_update: null pointer, empty table or batch, or a mode other than 0 (mean) / 1 (score, which needs pred_x0)");
    guide::Upd u;
    u.mode = mode; u.a = a; u.x0 = pred_x0; u.g = grad; u.noise = noise; u.draw = draw != 0; u.seed = seed; u.first_clip = first_clip;
    u.coef = coef; u.n_rows = n_rows; u.t_idx = (const int*)t_idx; u.n_clips = n_clips; u.out = out;
    const long n = (long)n_clips * (SYN_C / 4) * SYN_T;
    hipLaunchKernelGGL(guide::k_guide_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u);
    return launched("k_guide_update launch");
}

}  // extern "C"
