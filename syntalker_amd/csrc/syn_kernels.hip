// syn_kernels.hip — hand-written CDNA4 (gfx950) kernels for the SynTalker denoising step.
//
// What one step computes (reference models/denoiser.py:132-196 after hoisting the timestep-
// independent conditioning and folding the affine input stage, SURVEY.md §8 a17-a20, followed by the
// posterior update of diffusion/gaussian_diffusion.py:505-557 / :741-791):
//
//   h   = rotary( x_t . A^T + cond[clip] + te[t] )                    k_gemm<EPI_IN>
//   8 x { qkv = LN1(h) . Wqkv^T                                        k_gemm<EPI_QKV>
//         o   = softmax(q k^T / sqrt(128)) v       (4 heads, 32x32)    k_attn
//         h  += o . Wproj^T + b                                        k_gemm<EPI_RESID>  (+ LN2 -> xn)
//         hid = gelu(LN2(h) . W1^T + b1)                               k_gemm<EPI_GELU>
//         h  += hid . W2^T + b2 }                                      k_gemm<EPI_RESID>  (+ LN1' -> xn)
//   x0  = h . Wout^T + bout ;  x_{t-1} = c0*x0 + c1*x_t + sigma*eps    k_gemm<EPI_OUT>
//
// GEMM structure (one template, five epilogues).  A workgroup of 8 waves owns MT rows (whole clips)
// x 512 output columns; wave w owns columns [64w, 64w+64) for ALL MT rows, so
//   * the weight operand is never shared between waves: each wave streams its own MFMA fragments
//     straight from L2 into VGPRs (weights are pre-packed so one fragment = one coalesced 1 KiB read);
//   * the activation operand (MT x 64 bf16 K-tile) is shared by all 8 waves: staged through LDS,
//     double-buffered, 16-byte slots XOR-swizzled by (row & 7) so ds_read_b128 is conflict-free;
//   * a full 512-wide row lives inside one workgroup, so LayerNorm of the NEXT op is an epilogue.
// MFMA orientation: D[n][m] = sum_k W[n][k] X[m][k]  (weights = A operand, tokens = B operand), so a
// lane ends up with 4 CONSECUTIVE output features of one token -> 16 B (fp32) / 8 B (bf16) stores into
// row-major [token][feature] tensors.  v_mfma_f32_16x16x32_bf16 layouts (gfx950):
//   A: lane l holds A[i = l&15][k = 8*(l>>4) .. +7]     B: lane l holds B[k = 8*(l>>4) .. +7][j = l&15]
//   D: lane l, reg r holds D[i = 4*(l>>4) + r][j = l&15]
//
// Files: this one holds the token-resident whole-step kernel k_stack (large batches), the A/B kernels, the small
// kernels and the C-ABI entry points of the step, the packs, the layout converters and syn_linear* (an entry point is
// defined once, in the file that holds the kernels it launches: every other one sits at the end of its .inc); syn_latency.inc the persistent small-batch kernel k_lat; syn_wavenc.inc the
// WavEncoder convolutions (per-clip conditioning); syn_train.inc the fp32 forward / backward kernels of the
// training path; syn_step_plan.inc (plain C++, no HIP) the choice of the kernel that runs a step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "syn_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

namespace {

constexpr int kThreads = 512;   // 8 waves: 2 per SIMD, 256-VGPR budget each
constexpr int kKT = 64;         // K tile staged through LDS (128 B per row)
constexpr int kNT = 512;        // output columns per workgroup (64 per wave)

enum Epi { EPI_PLAIN = 0, EPI_IN = 1, EPI_QKV = 2, EPI_RESID = 3, EPI_GELU = 4, EPI_OUT = 5 };

struct GArgs {
    // operands
    const __bf16* X; long x_chunk_stride; int ldx; int x_rows;   // activation row = m % x_rows
    const uint4* W; int K; int M;
    const float* bias;
    // residual + LayerNorm epilogues
    float* H; __bf16* Y; int ldy; const float* ln_g; const float* ln_b;
    // input epilogue
    const float* cond; const float* te; const int* t_model; const float* rcos; const float* rsin;
    // qkv epilogue
    __bf16* Q; __bf16* Kb; __bf16* Vt;
    // posterior epilogue
    const float* Xt; const float* noise; const float* coef; const int* t_coef;
    float* Xn; __bf16* Xnb; float* X0;
    const unsigned long long* rng;   // {seed, first_clip}: draw the noise in the epilogue, stream id = the clip's t_coef
    // in-painting (syn_denoise_step_edit): x0 = keep ? known : x0 ahead of the update; both token-major like Xt, both NULL = no edit
    const unsigned char* keep; const float* known;
    // plain fp32 output (unit tests)
    float* Yf; int ldyf;
    int ablate;   // diagnostics (syn_test_gemm only): 1 = weights loaded once, 2 = activations staged once, 4 = no store
    int mt128;    // row tile of the 128-column plain GEMM (16 / 32 / 64), chosen by the host per shape
    // plain epilogue of a residual branch's last Linear: Yf = res + rscale[m / rows_per_scale] * (acc + bias) (rscale NULL: factor 1)
    const float* res; const float* rscale; int rows_per_scale;
    int w_ks;     // 128-column GEMM on a K slice (linear_impl: K beyond the resident block): k-steps of the FULL packed weight (its pitch per 16 columns); 0 = K / 32
};

// Rotary pair (models/denoiser.py:178-186) with its roundings pinned: u' = fma(u, cos, -(w sin)), w' = fma(w, cos, u sin), the
// inner products rounded on their own.  Written out because the whole-step kernel and the per-layer kernels must round alike
// (test_fused_layer_kernels_equal_unfused_bitwise) and the compiler's choice of which product to fuse moved with an unrelated edit.
__device__ __forceinline__ void rotary4(f32x4& u, f32x4& w, const f32x4 cs, const f32x4 sn) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ws = __fmul_rn(w[e], sn[e]), us = __fmul_rn(u[e], sn[e]);
        const float a = __builtin_fmaf(u[e], cs[e], -ws), b = __builtin_fmaf(w[e], cs[e], us);
        u[e] = a; w[e] = b;
    }
}

__device__ __forceinline__ bf16x4 to_bf16x4(f32x4 v) {
    bf16x4 r;
    r[0] = (__bf16)v[0]; r[1] = (__bf16)v[1]; r[2] = (__bf16)v[2]; r[3] = (__bf16)v[3];
    return r;
}

// In-painting blend of the reference's p_mean_variance (diffusion/gaussian_diffusion.py:316-320) on four consecutive channels of one
// token: x0 = keep ? known : x0.  Callers test `keep` for null first (wave-uniform), so a step without an edit issues none of these loads.
__device__ __forceinline__ f32x4 edit_x0(const unsigned char* __restrict__ keep, const float* __restrict__ known, const size_t off, f32x4 x0) {
    const uchar4 k = *reinterpret_cast<const uchar4*>(keep + off);
    const f32x4 kn = *reinterpret_cast<const f32x4*>(known + off);
    x0[0] = k.x ? kn[0] : x0[0]; x0[1] = k.y ? kn[1] : x0[1]; x0[2] = k.z ? kn[2] : x0[2]; x0[3] = k.w ? kn[3] : x0[3];
    return x0;
}

// c0 x0 + c1 x_t with the roundings hipcc gives the plain expression `x0 * c0 + xt * c1` in the output stages: fma(x0, c0, xt * c1), the second
// product rounded on its own.  Written out for k_stack's EDIT instances: behind the blend's select the compiler multiplies both arms by c0 first
// and fuses the OTHER product, and the entries that are not kept would differ from the plain step's in the last bit.
// Only this side is pinned: the plain instances keep the expression, so that they compile to what they were.  Their contraction was read from
// the ISA of ROCm 7.2's hipcc (AMD clang 22.0.0git, roc-7.2.0); should a compiler contract it differently, tests/test_gpu_edit.py's bit-equality
// checks fail with no change here, and the fix is to write the plain side with update_pinned's operations too.
__device__ __forceinline__ f32x4 update_pinned(const f32x4 x0, const f32x4 xt, const float c0, const float c1) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(x0[e], c0, __fmul_rn(xt[e], c1));
    return r;
}

// nn.GELU() default = exact erf form 0.5 x (1 + erf(x / sqrt2)).  erf by Abramowitz & Stegun 7.1.26
// (|abs err| <= 1.5e-7, i.e. fp32-roundoff class) with v_rcp_f32 / v_exp_f32: ~16 VALU ops per element.
// The ocml erff() call it replaces measured ~300 cycles per element-wave: 28 % of the fused MLP kernel.
__device__ __forceinline__ float gelu_erf(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);
    const float erf_abs = fmaf(-p * t, e, 1.0f);                 // erf(|x|/sqrt2)
    return 0.5f * x * (1.0f + copysignf(erf_abs, x));
}

// ------------------------------------------------------------------------------------------------
// nn.GELU() of the plain epilogue's value as the bf16 operand of the NEXT Linear (fc1 -> GELU -> fc2, transformer.py:117-151): k_gelu_fwd's
// arithmetic (exact erf form), so the fused MLP branch rounds exactly as the single-op composition does.
__device__ __forceinline__ void plain_gelu_bf16(const GArgs& a, const f32x4 v, int m, int n) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    *reinterpret_cast<bf16x4*>(a.Y + (size_t)m * a.ldyf + n) = to_bf16x4(o);
}

// Main loop: acc[nf][mf] += W-frag(nf) x X-frag(mf) over K (K a multiple of 128).
//   slot nf not in SWAPMASK: acc[nf][mf][r] = out[m = 16mf + (l&15)][n = 16nf' + 4(l>>4) + r]
//   slot nf in SWAPMASK    : acc[nf][mf][r] = out[m = 16mf + 4(l>>4) + r][n = 16nf' + (l&15)]
// Software pipeline (vmcnt retires loads IN ORDER, so every load is issued >= 3 k-steps before its
// consumer and nothing urgent ever queues behind a younger long-latency load):
//   * weight fragments: ring of 4 register slots, loaded 3 k-steps ahead straight from L2/MALL;
//   * activation K-tiles: two register sets in flight (2 tiles ahead of the LDS store), LDS double buffer,
//     one workgroup barrier per K-tile;
//   * __builtin_amdgcn_sched_barrier(0) after each issue block: hipcc otherwise SINKS the prefetch loads
//     down to their consumers (observed: at most 2-3 loads in flight, 76 % of wave cycles parked).
// Wq: this lane's pointer to fragment (slot 0, k-step 0); fragment (nf, ks) is at Wq[((nf*FS)*KS + ks)*64].
template <int MT, int NF, int FS, int SWAPMASK>
__device__ __forceinline__ void gemm_mainloop(f32x4 (&acc)[NF][MT / 16], const __bf16* __restrict__ X, int ldx,
                                              int x_rows, int m0, int M, int K, const uint4* __restrict__ Wq,
                                              char* smem, const int ablate = 0) {
    constexpr int MF = MT / 16;
    constexpr int NLD = (MT * 8 + kThreads - 1) / kThreads;   // 16-byte staging loads per thread per K tile
    constexpr int BUF = MT * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int KS = K / 32, NKT = K / kKT;

    const __bf16* src[NLD];
    int dst[NLD];
    bool live[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int idx = tid + i * kThreads;
        const int row = idx >> 3, slot = idx & 7;
        const int m = m0 + row;
        live[i] = (idx < MT * 8) && (m < M);
        src[i] = X + (size_t)(live[i] ? (m % x_rows) : 0) * ldx + slot * 8;
        dst[i] = row * 128 + ((slot ^ (row & 7)) << 4);
    }
    auto stage_load = [&](uint4 (&st)[NLD], int kt) {
        if (kt < NKT && !((ablate & 2) && kt > 1)) {
#pragma unroll
            for (int i = 0; i < NLD; ++i)
                st[i] = live[i] ? *reinterpret_cast<const uint4*>(src[i] + kt * kKT) : make_uint4(0, 0, 0, 0);
        }
    };
    auto stage_store = [&](const uint4 (&st)[NLD], int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            if (NLD * kThreads == MT * 8 || tid + i * kThreads < MT * 8)
                *reinterpret_cast<uint4*>(smem + buf * BUF + dst[i]) = st[i];
    };
    // fragment read offsets (row = 16mf + (l&15) -> row&7 = l&7; slot = 4ks + (l>>4))
    int xoff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) xoff[ks] = (lane & 15) * 128 + ((((4 * ks) + (lane >> 4)) ^ (lane & 7)) << 4);

    uint4 w0[NF], w1[NF], w2[NF], w3[NF];
    auto w_load = [&](uint4 (&w)[NF], int kstep) {
        if (kstep < KS && !((ablate & 1) && kstep > 3)) {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) w[nf] = Wq[((size_t)(nf * FS) * KS + kstep) * 64];
        }
    };
    auto compute = [&](const uint4 (&w)[NF], int buf, int ks) {
        // activation fragments in groups of <= 4 (16 VGPRs) to stay inside the 256-register budget at MT = 128
        constexpr int G = MF > 4 ? 4 : MF;
#pragma unroll
        for (int h = 0; h < MF / G; ++h) {
            bf16x8 xf[G];
#pragma unroll
            for (int i = 0; i < G; ++i)
                xf[i] = *reinterpret_cast<const bf16x8*>(smem + buf * BUF + (h * G + i) * 2048 + xoff[ks]);
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const bf16x8 wf = __builtin_bit_cast(bf16x8, w[nf]);
#pragma unroll
                for (int i = 0; i < G; ++i)
                    acc[nf][h * G + i] = ((SWAPMASK >> nf) & 1) ? MFMA16(xf[i], wf, acc[nf][h * G + i])
                                                                 : MFMA16(wf, xf[i], acc[nf][h * G + i]);
            }
            if (MF > G) __builtin_amdgcn_sched_barrier(0);
        }
    };

    uint4 sa[NLD], sb[NLD];
    w_load(w0, 0);
    w_load(w1, 1);
    w_load(w2, 2);
    stage_load(sa, 0);
    stage_load(sb, 1);
    stage_store(sa, 0);
    stage_load(sa, 2);
    __syncthreads();
    for (int j = 0; 2 * j < NKT; ++j) {
        const int s4 = 4 * j;
        w_load(w3, s4 + 3);
        __builtin_amdgcn_sched_barrier(0);
        compute(w0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        w_load(w0, s4 + 4);
        __builtin_amdgcn_sched_barrier(0);
        compute(w1, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        stage_store(sb, 1);                 // tile 2j+1 (loaded two tiles ago)
        stage_load(sb, 2 * j + 3);
        w_load(w1, s4 + 5);
        __syncthreads();
        compute(w2, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        w_load(w2, s4 + 6);
        __builtin_amdgcn_sched_barrier(0);
        compute(w3, 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (2 * j + 2 < NKT) stage_store(sa, 0);   // tile 2j+2
        stage_load(sa, 2 * j + 4);
        __syncthreads();
    }
}

// The training step's Linear GEMMs have 512 - 1536 rows: 16-row tiles, 32 - 96 x (n / 512) workgroups, a wave or two per SIMD.  In the
// loop above a k-step is 4 MFMAs of 8 cycles behind weight loads issued 3 k-steps earlier, so at that occupancy every k-step waits for a
// third of an L2 round trip (~350 cycles per k-step: 48 k-steps of a K = 1536 data gradient = 8 us).  Here the workgroup's 16 x K
// activation block goes into the LDS ONCE (K <= 2048: <= 64 KB, the same swizzled 64-column tiles), one barrier, and the loop is
// barrier-free with R k-steps of weight fragments in flight.  Same products in the same order: bitwise the loop above.
#ifndef SYN_GEMM_RING
#define SYN_GEMM_RING 12
#endif
constexpr int kResidentMaxK = 2048;
// The resident loop in two pieces, so that a kernel with a loader of its own (csrc/syn_guide.inc) runs the same K loop: `staged_prime` issues the first
// R - 1 k-steps of weight fragments (before the activation block is staged: the two overlap), `staged_loop` is the barrier-free loop over an LDS image
// [K tile][row 0..MT-1][8 slots of 16 B, slot ^ (row & 7)] that is complete and visible (a barrier lies between).  SWAP: the activation fragment is
// the A operand - acc[nf][mf][r] = out[m = 16 mf + 4 (l >> 4) + r][n = 16 nf + (l & 15)] instead of out[m = 16 mf + (l & 15)][n = 16 nf + 4 (l >> 4) + r].
template <int NF, int R>
__device__ __forceinline__ void staged_w_load(uint4 (&wr)[NF], const uint4* __restrict__ Wq, int KS, int kstep) {
    if (kstep < KS) {
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) wr[nf] = Wq[((size_t)nf * KS + kstep) * 64];
    }
}
template <int NF, int R>
__device__ __forceinline__ void staged_prime(uint4 (&w)[R][NF], const uint4* __restrict__ Wq, int KS) {
    static_assert(R % 2 == 0 && (R - 1) * NF <= 63, "even ring (the k-step's half of its K tile is static), vmcnt has 6 bits");
#pragma unroll
    for (int s = 0; s < R - 1; ++s) staged_w_load<NF, R>(w[s], Wq, KS, s);
    __builtin_amdgcn_sched_barrier(0);
}
template <int MT, int NF, int R, bool SWAP = false>
__device__ __forceinline__ void staged_loop(f32x4 (&acc)[NF][MT / 16], uint4 (&w)[R][NF], int KS, const uint4* __restrict__ Wq, const char* smem) {
    constexpr int MF = MT / 16, TILE = MT * 128;
    const int lane = threadIdx.x & 63;
    int xoff[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) xoff[h] = (lane & 15) * 128 + ((((4 * h) + (lane >> 4)) ^ (lane & 7)) << 4);
    for (int base = 0; base < KS; base += R) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int ks = base + i;
            staged_w_load<NF, R>(w[(i + R - 1) % R], Wq, KS, ks + R - 1);
            __builtin_amdgcn_sched_barrier(0);
            if (ks < KS) {
                bf16x8 xf[MF];
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) xf[mf] = *reinterpret_cast<const bf16x8*>(smem + (ks >> 1) * TILE + mf * 2048 + xoff[i & 1]);
#pragma unroll
                for (int nf = 0; nf < NF; ++nf)
#pragma unroll
                    for (int mf = 0; mf < MF; ++mf) {
                        const bf16x8 wf = __builtin_bit_cast(bf16x8, w[i][nf]);
                        acc[nf][mf] = SWAP ? MFMA16(xf[mf], wf, acc[nf][mf]) : MFMA16(wf, xf[mf], acc[nf][mf]);
                    }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int MT, int NF, int R>
__device__ __forceinline__ void gemm_mainloop_resident(f32x4 (&acc)[NF][MT / 16], const __bf16* __restrict__ X, int ldx, int x_rows, int m0, int M,
                                                       int K, const uint4* __restrict__ Wq, char* smem) {
    constexpr int TILE = MT * 128;
    const int tid = threadIdx.x;
    const int KS = K / 32, total = (K / kKT) * MT * 8;       // 16-byte chunks of the block: [K tile][row 0..MT-1][slot 0..7]
    uint4 w[R][NF];
    staged_prime<NF, R>(w, Wq, KS);
    for (int base = 0; base < total; base += 4 * kThreads) {
        uint4 st[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = base + i * kThreads + tid, row = (idx >> 3) % MT, m = m0 + row;
            st[i] = make_uint4(0, 0, 0, 0);
            if (idx < total && m < M) st[i] = *reinterpret_cast<const uint4*>(X + (size_t)(m % x_rows) * ldx + (idx / (MT * 8)) * kKT + (idx & 7) * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = base + i * kThreads + tid, row = (idx >> 3) % MT, slot = idx & 7;
            if (idx < total) *reinterpret_cast<uint4*>(smem + (idx / (MT * 8)) * TILE + row * 128 + ((slot ^ (row & 7)) << 4)) = st[i];
        }
    }
    __syncthreads();
    staged_loop<MT, NF, R>(acc, w, KS, Wq, smem);
}

// Row mean / rstd over the 512 columns a workgroup owns (8 waves x 64).  One pass (sum and sum of squares,
// fp32), ONE workgroup barrier: every lane then adds the 8 per-wave partials of its own rows (broadcast LDS
// reads).  The cancellation in E[x^2] - mean^2 costs ~6e-8 * (1 + mean^2/var) relative, far below the bf16
// rounding of the normalised output.  v[nf][mf][r] in the non-swapped layout.  red: MT*16 floats of LDS;
// `stat` is unused (kept for the call signature).
template <int MT>
__device__ __forceinline__ void row_stats(const f32x4 (&v)[4][MT / 16], float* red, float* /*stat*/,
                                          float (&mean)[MT / 16], float (&rstd)[MT / 16]) {
    constexpr int MF = MT / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s += v[nf][mf][r];
                q = fmaf(v[nf][mf][r], v[nf][mf][r], q);
            }
        s += __shfl_xor(s, 16); q += __shfl_xor(q, 16);
        s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);
        if (g == 0) *reinterpret_cast<float2*>(red + (mf * 16 + lr) * 16 + wave * 2) = make_float2(s, q);
    }
    __syncthreads();
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const f32x4* p = reinterpret_cast<const f32x4*>(red + (mf * 16 + lr) * 16);
        const f32x4 a = p[0], b = p[1], c = p[2], d = p[3];           // (s0,q0,s1,q1) ...
        const float S = ((a[0] + a[2]) + (b[0] + b[2])) + ((c[0] + c[2]) + (d[0] + d[2]));
        const float Q = ((a[1] + a[3]) + (b[1] + b[3])) + ((c[1] + c[3]) + (d[1] + d[3]));
        mean[mf] = S * (1.0f / 512.0f);
        const float var = fmaxf(Q * (1.0f / 512.0f) - mean[mf] * mean[mf], 0.f);
        rstd[mf] = rsqrtf(var + 1e-5f);                                // nn.LayerNorm: biased variance, eps 1e-5
    }
}

// h (fp32) is final in v; write H, then Y = LN(v)*g + b (or plain bf16(v) when ln_g == nullptr).
template <int MT>
__device__ __forceinline__ void store_h_and_norm(const GArgs& a, f32x4 (&v)[4][MT / 16], int m0, char* smem) {
    constexpr int MF = MT / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int m = m0 + mf * 16 + lr;
        if (m < a.M)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
                *reinterpret_cast<f32x4*>(a.H + (size_t)m * kNT + wave * 64 + nf * 16 + g * 4) = v[nf][mf];
    }
    if (a.Y == nullptr) return;             // residual stream only (the fused stack normalises on chip)
    float mean[MF], rstd[MF];
    if (a.ln_g != nullptr) {
        float* red = reinterpret_cast<float*>(smem);
        row_stats<MT>(v, red, red + MT * 8, mean, rstd);
    }
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
        const int n = wave * 64 + nf * 16 + g * 4;
        f32x4 gg = {1.f, 1.f, 1.f, 1.f}, bb = {0.f, 0.f, 0.f, 0.f};
        if (a.ln_g != nullptr) {
            gg = *reinterpret_cast<const f32x4*>(a.ln_g + n);
            bb = *reinterpret_cast<const f32x4*>(a.ln_b + n);
        }
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int m = m0 + mf * 16 + lr;
            f32x4 y = v[nf][mf];
            if (a.ln_g != nullptr) y = (y - mean[mf]) * rstd[mf] * gg + bb;
            if (m < a.M) *reinterpret_cast<bf16x4*>(a.Y + (size_t)m * a.ldy + n) = to_bf16x4(y);
        }
    }
}

// Beside an MFMA a packed fp32 operation costs ~20 cycles MORE than the two plain ones it replaces (scripts/ubench/seq_issue.hip:
// 35.4 cycles per MFMA with nothing in the gap, 38.2 with two v_fma_f32, 56.5 with one v_pk_fma_f32), and hipcc forms them wherever
// two fp32 values meet in adjacent registers (vector-typed expressions, the SLP vectoriser).  Work that rides in an MFMA's
// shadow is therefore written element by element, every result passed through this opaque no-op.
__device__ __forceinline__ float nopk(float x) { asm("" : "+v"(x)); return x; }

// x + DropPath(branch) (timm_transformer/transformer.py:195-198) in the epilogue of the branch's last Linear: res + factor * (x W^T + b),
// the factor one float per sample (rows_per_scale rows), rounded as torch.addcmul rounds it (product, then sum).
__device__ __forceinline__ f32x4 plain_residual(const GArgs& a, f32x4 v, int m, int n) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(a.res + (size_t)m * a.ldyf + n);
    if (a.rscale) {
        const float sc = a.rscale[m / a.rows_per_scale];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = nopk(v[e] * sc);
    }
    return r + v;
}


// a ^ b ^ c as ONE instruction: gfx950 has no v_xor3_b32, but v_bitop3_b32 evaluates any three-input truth table (0x96: odd parity),
// and hipcc does not form it from the expression (two v_xor_b32).  The generator runs in the shadow of MFMAs, where every vector
// instruction counts: 20 instead of 39 logic operations per four normals.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    if (__builtin_constant_p(b) && b == 0) return a ^ c;            // (the high counter words of round 0 are usually constant zeros)
    return (uint32_t)__builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
// Philox4x32-10 (Salmon et al. 2011), counter = (index/4, stream_id), key = seed; Box-Muller pairs.
// X3 = false: the two-xor form of the same round (same bits).  k_seq's guided drawn-noise instance takes it: with the one-instruction
// form hipcc's register allocation of that instance tips over (41 spilled registers against 18, 14 scratch accesses inside its output
// pair loop against 2).
template <bool X3 = true>
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = X3 ? xor3((uint32_t)(p1 >> 32), c[1], k[0]) : (uint32_t)(p1 >> 32) ^ c[1] ^ k[0];
    const uint32_t n2 = X3 ? xor3((uint32_t)(p0 >> 32), c[3], k[1]) : (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
    c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
    k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
}

// Four N(0,1) values for elements [4*idx4, 4*idx4+3] of the flat noise tensor of step `stream_id`.
template <bool X3 = true>
__device__ __forceinline__ f32x4 randn4(uint64_t seed, uint64_t stream_id, uint64_t idx4) {
    uint32_t c[4] = {(uint32_t)idx4, (uint32_t)(idx4 >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int r = 0; r < 10; ++r) philox_round<X3>(c, k);
    const float inv32 = 2.3283064365386963e-10f;   // 2^-32
    f32x4 z;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = ((float)c[2 * p] + 0.5f) * inv32;           // (0,1)
        const float u2 = ((float)c[2 * p + 1] + 0.5f) * inv32;
        // hardware transcendentals as they are: v_log_f32 is log2 (u1 >= 2^-33 is a normal number, so none of the
        // library's denormal scaling is needed), v_sin/v_cos take their argument in revolutions
        const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1)
        z[2 * p] = nopk(rad * __builtin_amdgcn_cosf(u2));              // (the epilogues call this in the shadow of MFMAs)
        z[2 * p + 1] = nopk(rad * __builtin_amdgcn_sinf(u2));
    }
    return z;
}

template <int MT, int EPI, bool RES = false>
__device__ __forceinline__ void gemm_body(const GArgs& a, const int bx, const int by) {
    static_assert(!RES || (MT == 16 && EPI == EPI_PLAIN), "the activation-resident loop serves the plain 16-row GEMMs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MF = MT / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    const int m0 = bx * MT, chunk = by;
    const int KS = a.K / 32;

    // Accumulators start from the additive epilogue terms (residual + bias, or conditioning + time row):
    // no extra registers after the loop and the loads overlap the pipeline prologue.
    f32x4 acc[4][MF];
    if constexpr (EPI == EPI_RESID) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = wave * 64 + nf * 16 + g * 4;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int m = m0 + mf * 16 + lr;
                f32x4 h = {0.f, 0.f, 0.f, 0.f};
                if (m < a.M) h = *reinterpret_cast<const f32x4*>(a.H + (size_t)m * kNT + n);
                acc[nf][mf] = h + b;
            }
        }
    } else if constexpr (EPI == EPI_IN) {
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int m = m0 + mf * 16 + lr;
            const bool ok = m < a.M;
            const int ts = ok ? a.t_model[m >> 5] : 0;
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const int n = wave * 64 + nf * 16 + g * 4;
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
                if (ok) c = *reinterpret_cast<const f32x4*>(a.cond + (size_t)m * kNT + n);
                acc[nf][mf] = c + *reinterpret_cast<const f32x4*>(a.te + (size_t)ts * kNT + n);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) acc[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const uint4* Wq = a.W + ((size_t)(chunk * 32 + wave * 4) * KS) * 64 + lane;
    const __bf16* X = a.X + (size_t)chunk * a.x_chunk_stride;
    const bool swap = (EPI == EPI_QKV) && (chunk == 2);
    if constexpr (RES)
        gemm_mainloop_resident<16, 4, SYN_GEMM_RING>(acc, X, a.ldx, a.x_rows, m0, a.M, a.K, Wq, smem);
    else if (swap)
        gemm_mainloop<MT, 4, 1, 0xF>(acc, X, a.ldx, a.x_rows, m0, a.M, a.K, Wq, smem);
    else
        gemm_mainloop<MT, 4, 1, 0>(acc, X, a.ldx, a.x_rows, m0, a.M, a.K, Wq, smem, EPI == EPI_PLAIN ? a.ablate : 0);

    const int ncol = chunk * kNT + wave * 64;   // first global output column of this wave

    if constexpr (EPI == EPI_PLAIN) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = ncol + nf * 16 + g * 4;
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) b = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int m = m0 + mf * 16 + lr;
                if (m < a.M && (!(a.ablate & 4) || acc[nf][mf][0] == 12345.678f)) {
                    f32x4 v = acc[nf][mf] + b;
                    if (a.res) v = plain_residual(a, v, m, n);
                    *reinterpret_cast<f32x4*>(a.Yf + (size_t)m * a.ldyf + n) = v;
                    if (a.Y) plain_gelu_bf16(a, v, m, n);
                }
            }
        }
    } else if constexpr (EPI == EPI_IN) {
        // (conditioning + time row were the accumulator's initial value.)  Rotary on the (j, j+32) pairs
        // of this wave's 64-wide group (models/denoiser.py:178-186): frags nf=0,1 hold j<32, nf=2,3 j+32.
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int pos = (m0 + mf * 16 + lr) & 31;
#pragma unroll
            for (int nf = 0; nf < 2; ++nf) {
                const int j = nf * 16 + g * 4;
                const f32x4 cs = *reinterpret_cast<const f32x4*>(a.rcos + pos * 32 + j);
                const f32x4 sn = *reinterpret_cast<const f32x4*>(a.rsin + pos * 32 + j);
                rotary4(acc[nf][mf], acc[nf + 2][mf], cs, sn);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        store_h_and_norm<MT>(a, acc, m0, smem);
    } else if constexpr (EPI == EPI_QKV) {
        if (!swap) {
            __bf16* dst = chunk == 0 ? a.Q : a.Kb;
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int m = m0 + mf * 16 + lr;
                if (m < a.M)
#pragma unroll
                    for (int nf = 0; nf < 4; ++nf)
                        *reinterpret_cast<bf16x4*>(dst + (size_t)m * kNT + wave * 64 + nf * 16 + g * 4) =
                            to_bf16x4(acc[nf][mf]);
            }
        } else {
            // V, transposed per (sequence, head): Vt[((seq*4 + head)*128 + d)*32 + token]
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int mb = m0 + mf * 16;            // 16 rows of one sequence
                const int seq = mb >> 5, tok = (mb & 31) + g * 4;
                if (mb < a.M)
#pragma unroll
                    for (int nf = 0; nf < 4; ++nf) {
                        const int n = wave * 64 + nf * 16 + lr;   // 0..511 = head*128 + d
                        *reinterpret_cast<bf16x4*>(a.Vt + ((size_t)seq * 512 + n) * 32 + tok) = to_bf16x4(acc[nf][mf]);
                    }
            }
        }
    } else if constexpr (EPI == EPI_RESID) {
        store_h_and_norm<MT>(a, acc, m0, smem);
    } else if constexpr (EPI == EPI_GELU) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = ncol + nf * 16 + g * 4;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int m = m0 + mf * 16 + lr;
                f32x4 v = acc[nf][mf] + b;
                v[0] = gelu_erf(v[0]); v[1] = gelu_erf(v[1]); v[2] = gelu_erf(v[2]); v[3] = gelu_erf(v[3]);
                if (m < a.M) *reinterpret_cast<bf16x4*>(a.Y + (size_t)m * a.ldy + n) = to_bf16x4(v);
            }
        }
    } else if constexpr (EPI == EPI_OUT) {
        // x0 = acc + bias;  x_next = c0*x0 + c1*x_t + sigma*eps   (p_sample / ddim_sample)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int m = m0 + mf * 16 + lr;
            if (m >= a.M) continue;
            const int tc = a.t_coef[m >> 5];
            const f32x4 cf = *reinterpret_cast<const f32x4*>(a.coef + (size_t)tc * 4);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const int n = ncol + nf * 16 + g * 4;
                const size_t off = (size_t)m * SYN_C + n;
                f32x4 x0 = acc[nf][mf] + *reinterpret_cast<const f32x4*>(a.bias + n);
                if (a.keep) x0 = edit_x0(a.keep, a.known, off, x0);
                const f32x4 xt = *reinterpret_cast<const f32x4*>(a.Xt + off);
                f32x4 xn = x0 * cf[0] + xt * cf[1];
                if (a.noise) xn = xn + *reinterpret_cast<const f32x4*>(a.noise + off) * cf[2];
                else if (a.rng) xn = xn + randn4(a.rng[0], (uint64_t)tc, (a.rng[1] * (uint64_t)(SYN_T * SYN_C) + off) >> 2) * cf[2];
                *reinterpret_cast<f32x4*>(a.Xn + off) = xn;
                *reinterpret_cast<bf16x4*>(a.Xnb + off) = to_bf16x4(xn);
                if (a.X0) *reinterpret_cast<f32x4*>(a.X0 + off) = x0;
            }
        }
    }
}

template <int MT, int EPI, bool RES = false>
__global__ __launch_bounds__(kThreads) void k_gemm(const GArgs a) { gemm_body<MT, EPI, RES>(a, blockIdx.x, blockIdx.y); }

// Plain GEMM on MT x 128 tiles (8 waves x 16 columns): the training step's shapes (1024 rows, 512 - 1536 columns) on 16 x 512 tiles are 64 - 192
// workgroups that each pull a 512-column slab of W (512 KB at K = 512) through ONE CU's L1 port - ~85 GB/s: 6 us per 512 of K whatever the
// ring depth (measured: 8.8 / 11.9 / 21.1 us at K = 512 / 1024 / 2048).  A quarter of the columns per workgroup = four times the workgroups,
// each pulling (MT + 128) x K x 2 bytes: the same L2 traffic through four times the ports.  Activation block resident in the LDS, deep ring.
template <int MT>
__device__ __forceinline__ void gemm_body_n128(const GArgs& a, const int bx, const int by) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MF = MT / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    const int m0 = bx * MT, KS = a.K / 32;
    f32x4 acc[1][MF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) acc[0][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* Wq = a.W + ((size_t)(by * 8 + wave) * (a.w_ks ? a.w_ks : KS)) * 64 + lane;
    gemm_mainloop_resident<MT, 1, 16>(acc, a.X, a.ldx, a.x_rows, m0, a.M, a.K, Wq, smem);
    const int n = by * 128 + wave * 16 + g * 4;
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) b = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int m = m0 + mf * 16 + lr;
        if (m < a.M) {
            f32x4 v = acc[0][mf] + b;
            if (a.res) v = plain_residual(a, v, m, n);
            *reinterpret_cast<f32x4*>(a.Yf + (size_t)m * a.ldyf + n) = v;
            if (a.Y) plain_gelu_bf16(a, v, m, n);
        }
    }
}
__device__ __forceinline__ void gemm_n128(const GArgs& a, const int bx, const int by) {
    if (a.mt128 == 64) gemm_body_n128<64>(a, bx, by);
    else if (a.mt128 == 32) gemm_body_n128<32>(a, bx, by);
    else gemm_body_n128<16>(a, bx, by);
}
__global__ __launch_bounds__(kThreads) void k_gemm_n128(const GArgs a) { gemm_n128(a, blockIdx.x, blockIdx.y); }

// A handful of rows against a long K (embed_text: 32 clips x 6144 seed values -> 512, models/denoiser.py:100-104): on row tiles this is two
// workgroups walking 192 k-steps one after the other (78 us).  Here a workgroup owns a 16 x 16 output tile and its 8 waves split K - both operands
// straight from L2, eight k-steps of loads in flight per wave - and the partial tiles are added in wave order through the LDS (deterministic).
__global__ __launch_bounds__(kThreads) void k_gemm_skinny(const GArgs a) {
    __shared__ f32x4 red[8][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    const int nf = blockIdx.x, m0 = blockIdx.y * 16, KS = a.K / 32, per = (KS + 7) / 8;
    const int k0 = wave * per, k1 = min(KS, k0 + per);
    const int m = m0 + lr;
    const __bf16* xrow = a.X + (size_t)((m < a.M ? m : 0) % a.x_rows) * a.ldx + 8 * g;
    const uint4* wq = a.W + (size_t)nf * KS * 64 + lane;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kb = k0; kb < k1; kb += 8) {
        uint4 wv[8], xv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ks = kb + i < k1 ? kb + i : k0;
            wv[i] = wq[(size_t)ks * 64];
            xv[i] = *reinterpret_cast<const uint4*>(xrow + ks * 32);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (kb + i < k1) acc = MFMA16(__builtin_bit_cast(bf16x8, wv[i]), __builtin_bit_cast(bf16x8, m < a.M ? xv[i] : make_uint4(0, 0, 0, 0)), acc);
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && m < a.M) {
        f32x4 v = red[0][lane];
#pragma unroll
        for (int w = 1; w < 8; ++w) v = v + red[w][lane];
        const int n = nf * 16 + g * 4;
        if (a.bias) v = v + *reinterpret_cast<const f32x4*>(a.bias + n);
        *reinterpret_cast<f32x4*>(a.Yf + (size_t)m * a.ldyf + n) = v;
    }
}

// Two independent plain GEMMs in one launch (grid z picks; x / y sized for the larger): the data-gradient and weight-gradient GEMMs of
// an nn.Linear's backward are 64 - 128 workgroups each on 256 CUs and do not depend on each other.
struct GPair { GArgs g[2]; int gx[2], gy[2]; const float* bias_parts; float* bias_grad; int part_rows, part_n; };
template <int MT, int MODE>              // MODE 0: 16 x 512 tiles, streaming loop; 1: the same tiles, resident loop; 2: 16 x 128 tiles, resident loop
__global__ __launch_bounds__(kThreads) void k_gemm_pair(const GPair p) {
    const int z = blockIdx.z;
    if (p.bias_grad && blockIdx.x == 0 && blockIdx.y == 0 && z == 0)       // the Linear's bias gradient: the sum of syn_linear_bwd_prep's per-64-row
        for (int n = threadIdx.x; n < p.part_n; n += kThreads) {            // column sums, in row-block order (what `part.sum(0)` cost a launch for)
            float sacc = 0.f;
            for (int i = 0; i < p.part_rows; ++i) sacc += p.bias_parts[(size_t)i * p.part_n + n];
            p.bias_grad[n] = sacc;
        }
    if ((int)blockIdx.x >= p.gx[z] || (int)blockIdx.y >= p.gy[z]) return;
    if constexpr (MODE == 2) gemm_n128(p.g[z], blockIdx.x, blockIdx.y);
    else gemm_body<MT, EPI_PLAIN, MODE == 1>(p.g[z], blockIdx.x, blockIdx.y);
}

// Independent plain GEMMs in one launch on MT x 128 tiles: the four weight gradients of EVERY transformer block (syn_train_stack_wgrad; r5: a launch per block).
// The weight gradients of all eight blocks are open at once when the backward chain kernel
// has finished, and a block's quad launch is one round of ~256 workgroups - eight launches were eight rounds with a tail and a boundary each.  A 1-d grid
// without empty workgroups: id -> (block, GEMM, tile); with a multiple of 8 workgroups the ids are dealt so that an XCD's workgroups are NEIGHBOURS in
// (GEMM, tile) order - tiles along x share their 128-column operand slab in that XCD's L2.
struct GQuadAll { const __bf16* X[SYN_LAYERS][4]; const uint4* W[SYN_LAYERS][4]; float* Y[SYN_LAYERS][4]; int ns[4], ks[4], mt[4], gx[4], cum[5], M, l0; };
__global__ __launch_bounds__(kThreads) void k_gemm_quad_all(const GQuadAll p) {
    const int total = gridDim.x;
    int b = blockIdx.x;
    if (total % 8 == 0) b = (b & 7) * (total >> 3) + (b >> 3);
    const int per = p.cum[4], l = p.l0 + b / per, r = b % per;
    int i = 0;
    while (r >= p.cum[i + 1]) ++i;
    const int loc = r - p.cum[i], bx = loc % p.gx[i], by = loc / p.gx[i];
    GArgs a = {};
    a.X = p.X[l][i]; a.ldx = p.M; a.x_rows = p.ns[i]; a.W = p.W[l][i]; a.K = p.M; a.M = p.ns[i]; a.Yf = p.Y[l][i]; a.ldyf = p.ks[i]; a.mt128 = p.mt[i];
    gemm_n128(a, bx, by);
}

// A forward GEMM of the training step fills a quarter to three quarters of the chip (16-row tiles x n / 512 columns), and the
// backward will need x^T as packed fragments (the weight-gradient GEMM's B operand): grid z = 1 packs them in the GEMM's shadow.
struct GPack { GArgs g; const __bf16* src; uint4* out; int n, k; };          // pack: fragments of W = src^T, src row-major [k][n] (k_pack_t)
template <int MT, int MODE>
__global__ __launch_bounds__(kThreads) void k_gemm_and_pack(const GPack p) {
    if (blockIdx.z == 0) {
        if constexpr (MODE == 2) gemm_n128(p.g, blockIdx.x, blockIdx.y);
        else gemm_body<MT, EPI_PLAIN, MODE == 1>(p.g, blockIdx.x, blockIdx.y);
        return;
    }
    const int KS = p.k / 32, total = (p.n / 16) * KS * 64;
    const int stride = gridDim.x * gridDim.y * kThreads;
    for (int idx = (blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x; idx < total; idx += stride) {
        const int lane = idx & 63, f = idx >> 6, ks = f % KS, nf = f / KS;
        const __bf16* src = p.src + (size_t)(32 * ks + 8 * (lane >> 4)) * p.n + 16 * nf + (lane & 15);
        bf16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = src[(size_t)e * p.n];
        p.out[idx] = __builtin_bit_cast(uint4, r);
    }
}

// ------------------------------------------------------------------------------------------------
// Attention: one wave per (sequence, head); 32 tokens x 128 dims, non-causal
// (models/timm_transformer/transformer.py:89-93).  Everything stays in registers:
//   S^T[key][q] = K Q^T  (A = K rows, B = Q rows)   -> lane owns one q column, 8 keys
//   softmax over keys = 8 in-lane values + 2 xor-shuffles (lanes l, l^16, l^32, l^48)
//   O^T[d][q]   = Vt P^T (A = Vt rows, B = P^T)     -> the S^T accumulator IS the B fragment after
//   permuting the contraction index: slot 8g+e <-> key (e<4 ? 4g+e : 16+4g+e-4), applied to Vt loads.
__global__ __launch_bounds__(256) void k_attn(const __bf16* __restrict__ Q, const __bf16* __restrict__ K,
                                               const __bf16* __restrict__ Vt, __bf16* __restrict__ O, int n_seq) {
    const int lane = threadIdx.x & 63, head = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
    const int seq = blockIdx.x;
    if (seq >= n_seq) return;
    const __bf16* q = Q + (size_t)seq * 32 * 512 + head * 128;
    const __bf16* k = K + (size_t)seq * 32 * 512 + head * 128;
    f32x4 s[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) s[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        bf16x8 kf[2], qf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            kf[f] = *reinterpret_cast<const bf16x8*>(k + (size_t)(16 * f + lr) * 512 + 32 * ks + 8 * g);
            qf[f] = *reinterpret_cast<const bf16x8*>(q + (size_t)(16 * f + lr) * 512 + 32 * ks + 8 * g);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) s[i][j] = MFMA16(kf[i], qf[j], s[i][j]);
    }
    // s[kf][qf][r] = S[q = 16qf + lr][key = 16kf + 4g + r]
    const float sc = 0.08838834764831845f * 1.4426950408889634f;   // 128^-0.5 * log2(e)
    bf16x8 pf[2];
    float inv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float mx = fmaxf(fmaxf(fmaxf(s[0][j][0], s[0][j][1]), fmaxf(s[0][j][2], s[0][j][3])),
                         fmaxf(fmaxf(s[1][j][0], s[1][j][1]), fmaxf(s[1][j][2], s[1][j][3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const __bf16 p = (__bf16)__builtin_amdgcn_exp2f((s[i][j][r] - mx) * sc);
                pf[j][i * 4 + r] = p;
                sum += (float)p;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        inv[j] = 1.0f / sum;
    }
    const __bf16* vt = Vt + (size_t)(seq * 4 + head) * 128 * 32;
    __bf16* o = O + (size_t)seq * 32 * 512 + head * 128;
#pragma unroll
    for (int df = 0; df < 8; ++df) {
        const __bf16* vr = vt + (size_t)(16 * df + lr) * 32 + 4 * g;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr);
        const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vr + 16);
        bf16x8 vf;
        vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
        vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 acc = MFMA16(vf, pf[j], (f32x4{0.f, 0.f, 0.f, 0.f}));
            // acc[r] = O[q = 16j + lr][d = 16df + 4g + r]
            *reinterpret_cast<bf16x4*>(o + (size_t)(16 * j + lr) * 512 + 16 * df + 4 * g) = to_bf16x4(acc * inv[j]);
        }
    }
}

__device__ __forceinline__ void stamp(long long* dbg, int slot) {
    if (dbg != nullptr && threadIdx.x == 0) dbg[(size_t)blockIdx.x * 32 + slot] = (long long)__builtin_readcyclecounter();
}

// ------------------------------------------------------------------------------------------------
// k_stack: the WHOLE 8-block transformer stack for one 64-row tile (2 sequences) in one kernel.
// Rows of different sequences never interact (attention is per sequence), so a workgroup can carry its
// tile through all 8 blocks with no grid-level synchronisation: the fp32 residual rows live in the
// accumulator registers for the entire stack (wave w = columns [64w, 64w+64), 64 VGPRs), every
// intermediate (LayerNorm outputs, q/k/v of one head, attention output, MLP hidden slices) lives in LDS
// as bf16, and the only HBM traffic of the stack is h in (fp32), y out (bf16) and the weight stream,
// which all workgroups walk in the same order so it is served by L2 / the 256 MB Infinity Cache.
// Every GEMM piece is the same barrier-free loop: B operand = activation rows resident in LDS,
// A operand = weight fragments streamed straight from L2 into a register ring D k-steps deep.
//   LDS (130 KB): XN 64x1024 B (LayerNorm output, slots swizzled by row&15)
//                 region B 64 KB: { QS 64x256 | KS 64x256 | VTS 2x128x72 } during attention,
//                                 { HID 2 x 64x512 } during the MLP
//                 RED 2.5 KB LayerNorm scratch
#include "syn_latency.inc"

struct SArgs {
    float* H;             // [M][512] fp32 residual stream: read at entry, final value written back
    __bf16* Y;            // [M][512] bf16(h_final): operand of the output GEMM
    syn_layer layer[SYN_LAYERS];
    int M;
    int write_h;          // also write the final fp32 h (needed only by the guidance combine)
    long long* dbg;
    // tensor-parallel mode (9..128 sequences, MT = 32): tp = 2 or 4 workgroups of ONE XCD share a tile, each computes
    // its heads / MLP slices / output chunks, partial residual streams are exchanged through L2 (see k_stack)
    int tp, tp_tiles;     // members per tile (1 = off), number of tiles
    unsigned* sync;       // [320]: per XCD at +32x: [0] rank allocation, [1] finished workgroups, [2 + g] barrier of group g
    float* xch;           // [tiles][2][4][32 * 512] fp32 exchange slots
    // fused input stage (in.X != nullptr): h = rotary(x_t . A^T + cond + te[t]) instead of reading H
    GArgs in;
    // fused output stage (out.Xn != nullptr; single conditioning variant only): x0 = h . Wout^T + b and the
    // posterior / DDIM update, instead of writing Y
    GArgs out;
};

// Weight ring of a barrier-free GEMM piece: D k-steps x NF fragments.  kloop_prime issues the first D-1
// k-steps (call it EARLY - before the barrier / LayerNorm / softmax that precedes the loop - so the ~1 us
// L2-miss latency of the first fragments is hidden behind that work); kloop_run consumes it.
template <int NF, int FS, int KSTEPS, int D>
__device__ __forceinline__ void kloop_prime(uint4 (&ring)[D][NF], const uint4* __restrict__ Wq, int KS, int kbase) {
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
        if (p < KSTEPS)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) ring[p][nf] = Wq[((size_t)(nf * FS) * KS + kbase + p) * 64];
}

// acc[nf][mf] += W(nf, kbase + s) x LDS-rows, s = 0..KSTEPS-1.  Row r of the operand is at base + r*ROWB,
// 16-byte slot (4s + g) of the row holds k = 32s + 8g .. +7, stored at slot ^ (r & 15).
template <int MF, int NF, int FS, int SWAPMASK, int KSTEPS, int ROWB, int D>
__device__ __forceinline__ void kloop_run(f32x4 (&acc)[NF][MF], uint4 (&ring)[D][NF], const char* base,
                                          const uint4* __restrict__ Wq, int KS, int kbase) {
    const int lane = threadIdx.x & 63, g = lane >> 4, lr = lane & 15;
    const int lane_off = lr * ROWB + (((g ^ lr) & 3) << 4), hi = (lr & 12) << 4;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        if (s + D - 1 < KSTEPS)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) ring[(s + D - 1) % D][nf] = Wq[((size_t)(nf * FS) * KS + kbase + s + D - 1) * 64];
        __builtin_amdgcn_sched_barrier(0);        // keep the prefetch D-1 k-steps ahead (hipcc would sink it)
        // slot (4s+g) ^ lr = ((4s) ^ (lr & 12)) | ((g ^ lr) & 3): one xor + add per k-step; the asm keeps hipcc from
        // hoisting all KSTEPS offsets out of the enclosing loops (16 live VGPRs per call site otherwise)
        int hv = hi;
        asm volatile("" : "+v"(hv));
        const char* xrow = base + lane_off + ((64 * s) ^ hv);
        bf16x8 xf[MF];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) xf[mf] = *reinterpret_cast<const bf16x8*>(xrow + mf * 16 * ROWB);
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            const bf16x8 wf = __builtin_bit_cast(bf16x8, ring[s % D][nf]);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
                acc[nf][mf] = ((SWAPMASK >> nf) & 1) ? MFMA16(xf[mf], wf, acc[nf][mf]) : MFMA16(wf, xf[mf], acc[nf][mf]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// y = LayerNorm(h) * g + b -> bf16 rows in LDS (ROWB = 1024, slots swizzled by row & 15); then h += add[n].
template <int MT>
__device__ __forceinline__ void ln_to_lds(f32x4 (&h)[4][MT / 16], const float* __restrict__ lg, const float* __restrict__ lb,
                                          const float* __restrict__ add, char* XN, float* red) {
    constexpr int MF = MT / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, lr = lane & 15;
    float mean[MF], rstd[MF];
    row_stats<MT>(h, red, red + MT * 8, mean, rstd);
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
        const int n = wave * 64 + nf * 16 + g * 4;
        const f32x4 gg = *reinterpret_cast<const f32x4*>(lg + n), bb = *reinterpret_cast<const f32x4*>(lb + n);
        const f32x4 ad = *reinterpret_cast<const f32x4*>(add + n);
        const int slot = 8 * wave + 2 * nf + (g >> 1);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const f32x4 y = (h[nf][mf] - mean[mf]) * rstd[mf] * gg + bb;
            *reinterpret_cast<bf16x4*>(XN + (mf * 16 + lr) * 1024 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(y);
            h[nf][mf] = h[nf][mf] + ad;
        }
    }
}

// EDIT: the output stage blends the in-painting operands in (out.keep / out.known).  A template flag, not the wave-uniform null test of
// the other output stages: k_stack<64> sits at 256 VGPRs, and the test alone cost it 16 bytes of scratch per lane in steps without an edit.
template <int MT, int TP = 0, bool EDIT = false>       // TP: members per tile in the tile-split mode (0 = off, 2, 4)
__global__ __launch_bounds__(kThreads) void k_stack(const SArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MF = MT / 16;
    constexpr int HC = 256;
    char* const XN = smem;
    char* const RB = smem + MT * 1024;              // region B
    char* const Qs = RB;
    char* const Ks = RB + MT * 256;
    char* const Vts = RB + MT * 512;
    float* const red = reinterpret_cast<float*>(RB + MT * 1024);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    constexpr int KS1 = SYN_D / 32, KS2 = SYN_FF / 32;
    // Tensor-parallel mode: the workgroups of an XCD (hardware XCC id, as in k_lat) take a rank by arrival order; P
    // consecutive ranks form a group = one tile.  The members hold identical copies of the residual stream; after the
    // attention and after the MLP each writes the partial sum of ITS heads / hidden slices (member 0's includes the
    // previous residual) to an L2-resident slot, the group meets at an XCD-local barrier, and everybody adds the P
    // partials in member order - the same bits in every member.
    constexpr int P = TP ? TP : 1;           // 1 in the plain instances: their code is unchanged
    int member = 0, tile = blockIdx.x;
    unsigned* gctr = nullptr;
    unsigned* xbase = nullptr;
    unsigned* const gerr = a.sync ? a.sync + lat::kGroups * 32 : nullptr;
    unsigned gphase = 0;
    if constexpr (TP) {
        __shared__ int s_rank;
        const int xcd = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u) % lat::kGroups;
        xbase = a.sync + xcd * 32;
        if (tid == 0) s_rank = (int)__hip_atomic_fetch_add(xbase, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int rank = s_rank, per_xcd = (int)gridDim.x / lat::kGroups;
        if (rank >= per_xcd) {                                       // the dispatcher did not deal the workgroups evenly
            if (tid == 0) __hip_atomic_store(gerr, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        member = rank % P;
        tile = xcd + lat::kGroups * (rank / P);
        gctr = xbase + 2 + rank / P;
    }
    // (tp) leave the counters zeroed for the next launch: the last workgroup of this XCD to finish resets them
    auto tp_done = [&]() {
        if (TP && tid == 0) {
            const unsigned per_xcd = gridDim.x / lat::kGroups;
            if (__hip_atomic_fetch_add(xbase + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == per_xcd - 1)
                for (int i = 0; i < 32; ++i) __hip_atomic_store(xbase + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (TP && tile >= a.tp_tiles) { tp_done(); return; }           // padding group (tiles are dealt 8 at a time)
    const int m0 = tile * MT;
    float* const xch = TP ? a.xch : nullptr;
    // this member's partial -> sum of all members' partials, in member order (identical bits in every member).  Two slot
    // sets alternate: a member can be at most one exchange ahead of the slowest reader of the previous one.
    auto exchange = [&](f32x4 (&hh)[4][MT / 16], long long* dbg = nullptr) {
        constexpr int MFX = MT / 16;
        stamp(dbg, 21);
        int et = tid;
        asm volatile("" : "+v"(et));              // addresses are rebuilt here, not kept live across the blocks
        float* const set = xch + ((size_t)(tile * 2 + (int)(gphase & 1u)) * 4) * (MT * 512) + et * 4;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MFX; ++mf)
                *reinterpret_cast<f32x4*>(set + (size_t)member * (MT * 512) + (nf * MFX + mf) * 2048) = hh[nf][mf];
        lat::group_release();
        stamp(dbg, 22);
        ++gphase;
        lat::group_wait(gctr, gphase * (unsigned)P, gerr);
        stamp(dbg, 23);
        // the others' partials: all loads of a half (2 x MFX fragments from P - 1 members) are issued before the first add
        // (a dependent chain of 24 L2 round trips measured 5.7 us here); own partial from the register it was stored
        // from (same bits); member order
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[P][2][MFX];
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                    for (int mf = 0; mf < MFX; ++mf)
                        if (j != member)
                            v[j][n2][mf] = lat::ld_xcd(reinterpret_cast<const f32x4*>(set + (size_t)j * (MT * 512) + ((half * 2 + n2) * MFX + mf) * 2048));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                for (int mf = 0; mf < MFX; ++mf) {
                    const f32x4 own = hh[half * 2 + n2][mf];
                    f32x4 sum = member == 0 ? own : v[0][n2][mf];
#pragma unroll
                    for (int j = 1; j < P; ++j) sum = sum + (j == member ? own : v[j][n2][mf]);
                    hh[half * 2 + n2][mf] = sum;
                }
        }
        if (dbg) { __builtin_amdgcn_s_waitcnt(0); stamp(dbg, 24); }
    };
    stamp(a.dbg, 0);

    f32x4 h[4][MF];
    if (a.in.X != nullptr) {
        // ---- input stage: h = rotary(x_t . A^T + cond + te[t]); K = 1536 streamed through region B ----------
        // x_t goes through LDS 512 columns at a time, in the same swizzled row layout LayerNorm writes, alternating
        // between XN and region B, so that the three K pieces run on the barrier-free loop of the blocks (a 64-column
        // tile per barrier, as the stand-alone GEMM does it, spends more time in barriers than in MFMAs here).
        // A wave copies one whole row per instruction: 1 KB contiguous from HBM, 64 distinct LDS slots.
        {
            constexpr int KSI = SYN_C / 32, NCH = SYN_C / 512;
            constexpr int RW = MT / 8;     // rows per wave
            const uint4* wi = a.in.W + ((size_t)(wave * 4) * KSI) * 64 + lane;
            int sl = lane;
            asm volatile("" : "+v"(sl));
            uint4 st[RW];
            auto load = [&](int c) {
#pragma unroll
                for (int i = 0; i < RW; ++i) {
                    const int m = m0 + wave + 8 * i;
                    const int rm = m < a.in.x_rows ? m : m % a.in.x_rows;
                    st[i] = m < a.M ? *reinterpret_cast<const uint4*>(a.in.X + (size_t)rm * a.in.ldx + c * 512 + sl * 8)
                                    : make_uint4(0, 0, 0, 0);
                }
            };
            auto store = [&](char* buf) {
#pragma unroll
                for (int i = 0; i < RW; ++i) {
                    const int r = wave + 8 * i;
                    *reinterpret_cast<uint4*>(buf + r * 1024 + ((sl ^ (r & 15)) << 4)) = st[i];
                }
            };
            uint4 ri[4][4];
            load(0);
            kloop_prime<4, 1, 16, 4>(ri, wi, KSI, 0);
            {
                // h starts as conditioning + time row.  The conditioning tile (128 KB per workgroup) is read with 16
                // lanes on 256 contiguous bytes of a row and turned into the fragment layout through region B (free
                // until the second K piece lands there); read in the fragment layout directly it moves at a third of
                // the rate (16 half cache lines per instruction).
                const int er = sl >> 4, ec = (sl & 15) * 4;
                float* const T = reinterpret_cast<float*>(RB) + wave * (16 * 68);
                f32x4 cq[2][4];
                auto cfetch = [&](int mf, int slot) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = min(m0 + mf * 16 + i * 4 + er, a.M - 1);
                        cq[slot][i] = *reinterpret_cast<const f32x4*>(a.in.cond + (size_t)m * kNT + wave * 64 + ec);
                    }
                };
                cfetch(0, 0);
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    if (mf + 1 < MF) cfetch(mf + 1, (mf + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                    const int ts = a.in.t_model[min(m0 + mf * 16, a.M - 1) >> 5];
#pragma unroll
                    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(T + (i * 4 + er) * 68 + ec) = cq[mf & 1][i];
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int nf = 0; nf < 4; ++nf) {
                        const f32x4 cv = *reinterpret_cast<const f32x4*>(T + lr * 68 + nf * 16 + g * 4);
                        const f32x4 tv = *reinterpret_cast<const f32x4*>(a.in.te + (size_t)ts * kNT + wave * 64 + nf * 16 + g * 4);
                        h[nf][mf] = (m0 + mf * 16 + lr < a.M ? cv : f32x4{0.f, 0.f, 0.f, 0.f}) + tv;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            store(XN);
            load(1);
            __syncthreads();
            if (a.dbg) stamp(a.dbg, 17);
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                char* const cur = (c & 1) ? RB : XN;
                char* const nxt = (c & 1) ? XN : RB;
                kloop_run<MF, 4, 1, 0, 16, 1024, 4>(h, ri, cur, wi, KSI, c * 16);
                if (a.dbg) stamp(a.dbg, 18 + c);
                if (c + 1 < NCH) {
                    kloop_prime<4, 1, 16, 4>(ri, wi, KSI, (c + 1) * 16);
                    store(nxt);
                    if (c + 2 < NCH) load(c + 2);
                    __syncthreads();
                }
            }
        }
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int pos = (m0 + mf * 16 + lr) & 31;
#pragma unroll
            for (int nf = 0; nf < 2; ++nf) {
                const int j = nf * 16 + g * 4;
                const f32x4 cs = *reinterpret_cast<const f32x4*>(a.in.rcos + pos * 32 + j);
                const f32x4 sn = *reinterpret_cast<const f32x4*>(a.in.rsin + pos * 32 + j);
                rotary4(h[nf][mf], h[nf + 2][mf], cs, sn);
            }
        }
    } else {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int m = m0 + mf * 16 + lr;
                h[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (m < a.M) h[nf][mf] = *reinterpret_cast<const f32x4*>(a.H + (size_t)m * kNT + wave * 64 + nf * 16 + g * 4);
            }
    }
    if (a.dbg) stamp(a.dbg, 9);

#ifndef SYN_DQ
#define SYN_DQ 4
#endif
#ifndef SYN_DP
#define SYN_DP 3
#endif
#ifndef SYN_D1
#define SYN_D1 6
#endif
#ifndef SYN_D2
#define SYN_D2 3
#endif
    constexpr int DQ = SYN_DQ, DP = SYN_DP, D1 = SYN_D1, D2 = SYN_D2;   // weight-ring depths (k-steps in flight)
#ifdef SYN_HOTW   /* diagnostic build only: every weight stream aliases block 0 / head 0 / slice 0 (L2-hot) */
#define HOT(x) 0
#else
#define HOT(x) (x)
#endif
    auto wqkv = [&](int l, int head) { return (const uint4*)a.layer[HOT(l)].w_qkv + ((size_t)(HOT(head) * 8 + wave) * KS1) * 64 + lane; };
    for (int l = 0; l < SYN_LAYERS; ++l) {
        const syn_layer& L = a.layer[HOT(l)];
        // Rings are declared per block so they are dead (not loop-carried registers) outside their phase.
        uint4 rq[DQ][3];                           // qkv ring: primed one phase ahead of its loop
        kloop_prime<3, 32, KS1, DQ>(rq, wqkv(l, member), KS1, 0);  // in flight during LayerNorm 1
        const uint4* const wproj = (const uint4*)L.w_proj + ((size_t)(wave * 4) * KS1) * 64 + lane;
        const uint4* const wfc2 = (const uint4*)L.w_fc2 + ((size_t)(wave * 4) * KS2) * 64 + lane;
        // ---- x1 = LN1(h) -> XN;  h += b_proj ------------------------------------------------------------
        ln_to_lds<MT>(h, L.ln1_g, L.ln1_b, L.b_proj, XN, red);
        if (TP && member != 0) {                 // (tp) only member 0's partial carries the residual and the bias
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) h[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        if (l == 3) stamp(a.dbg, 1);
        for (int head = member; head < SYN_HEADS; head += P) {
            // ---- q, k, v fragments of this head for all MT rows ------------------------------------------
            f32x4 acc[3][MF];
#pragma unroll
            for (int sl = 0; sl < 3; ++sl)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) acc[sl][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            kloop_run<MF, 3, 32, 0x4, KS1, 1024, DQ>(acc, rq, XN, wqkv(l, head), KS1, 0);
            uint4 rp[DP][4];                        // proj ring: in flight during the attention
            kloop_prime<4, 1, 4, DP>(rp, wproj, KS1, HOT(head) * 4);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int row = mf * 16 + lr;
                const int off = row * 256 + ((((2 * wave) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8;
                *reinterpret_cast<bf16x4*>(Qs + off) = to_bf16x4(acc[0][mf]);
                *reinterpret_cast<bf16x4*>(Ks + off) = to_bf16x4(acc[1][mf]);
                *reinterpret_cast<bf16x4*>(Vts + (mf >> 1) * (128 * 72) + (wave * 16 + lr) * 72 + ((mf & 1) * 16 + g * 4) * 2) =
                    to_bf16x4(acc[2][mf]);
            }
            __syncthreads();
            if (l == 3 && head == 0) stamp(a.dbg, 2);
            // ---- attention: wave -> (sequence c, 16-query half qh); o overwrites the wave's own q rows ------
            if (wave < MT / 16) {
                const int c = wave >> 1, qh = wave & 1;
                const int qrow = c * 32 + qh * 16 + lr;
                f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int so = (((4 * ks) + g) ^ lr) << 4;
                    const bf16x8 qf = *reinterpret_cast<const bf16x8*>(Qs + qrow * 256 + so);
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (c * 32 + f * 16 + lr) * 256 + so);
                        sc[f] = MFMA16(kf, qf, sc[f]);
                    }
                }
                const float scale = 0.08838834764831845f * 1.4426950408889634f;
                float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),
                                 fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                bf16x8 pf;
                float sum = 0.f;
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const __bf16 pv = (__bf16)__builtin_amdgcn_exp2f((sc[f][r] - mx) * scale);
                        pf[f * 4 + r] = pv;
                        sum += (float)pv;
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
                const char* vt = Vts + c * (128 * 72);
#pragma unroll
                for (int df = 0; df < 8; ++df) {
                    const char* vr = vt + (16 * df + lr) * 72 + 8 * g;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr);
                    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vr + 32);
                    bf16x8 vf;
                    vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
                    vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
                    const f32x4 o = MFMA16(vf, pf, (f32x4{0.f, 0.f, 0.f, 0.f}));
                    // o[r] = O[q = lr][d = 16df + 4g + r] -> row qrow, 16-B slot 2df + (g>>1), swizzled like q/k
                    *reinterpret_cast<bf16x4*>(Qs + qrow * 256 + ((((2 * df) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8) =
                        to_bf16x4(o * inv);
                }
            }
            // next qkv ring (next head, or head 0 of the next block) goes in flight before the proj piece
            if (head + P < SYN_HEADS) kloop_prime<3, 32, KS1, DQ>(rq, wqkv(l, head + P), KS1, 0);
            __syncthreads();
            if (l == 3 && head == 0) stamp(a.dbg, 3);
            // ---- h += o_head . Wproj[:, 128 head .. +128]^T  (K = 128) ---------------------------------------
            kloop_run<MF, 4, 1, 0, 4, 256, DP>(h, rp, Qs, wproj, KS1, HOT(head) * 4);
            __syncthreads();
            if (l == 3 && head == 0) stamp(a.dbg, 4);
        }
        if constexpr (TP) exchange(h, l == 3 ? a.dbg : nullptr);
        if (l == 3) stamp(a.dbg, 5);
        // ---- x2 = LN2(h) -> XN;  h += b_fc2 ------------------------------------------------------------------
        uint4 r1[D1][2];
        auto wfc1 = [&](int c) { return (const uint4*)L.w_fc1 + ((size_t)(HOT(c) * 16 + wave * 2) * KS1) * 64 + lane; };
        kloop_prime<2, 1, KS1, D1>(r1, wfc1(member), KS1, 0);     // in flight during LayerNorm 2
        ln_to_lds<MT>(h, L.ln2_g, L.ln2_b, L.b_fc2, XN, red);
        if (TP && member != 0) {
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) h[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        if (l == 3) stamp(a.dbg, 6);
        int slice_it = 0;
        for (int c = member; c < SYN_FF / HC; c += P, ++slice_it) {
            f32x4 a1[2][MF];
#pragma unroll
            for (int nf = 0; nf < 2; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) a1[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            kloop_run<MF, 2, 1, 0, KS1, 1024, D1>(a1, r1, XN, wfc1(c), KS1, 0);
            uint4 r2[D2][4];
            kloop_prime<4, 1, HC / 32, D2>(r2, wfc2, KS2, HOT(c) * 8);   // in flight during the GELU
            char* const hb = RB + (slice_it & 1) * (MT * 512);
#pragma unroll
            for (int nf = 0; nf < 2; ++nf) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(L.b_fc1 + c * HC + wave * 32 + nf * 16 + g * 4);
                const int slot = 4 * wave + 2 * nf + (g >> 1);
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    f32x4 v = a1[nf][mf] + b;
                    v[0] = gelu_erf(v[0]); v[1] = gelu_erf(v[1]); v[2] = gelu_erf(v[2]); v[3] = gelu_erf(v[3]);
                    *reinterpret_cast<bf16x4*>(hb + (mf * 16 + lr) * 512 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(v);
                }
            }
            if (c + P < SYN_FF / HC) kloop_prime<2, 1, KS1, D1>(r1, wfc1(c + P), KS1, 0);
            __syncthreads();
            kloop_run<MF, 4, 1, 0, HC / 32, 512, D2>(h, r2, hb, wfc2, KS2, HOT(c) * 8);
        }
        __syncthreads();        // region B (hidden slices) becomes q/k/v + LayerNorm scratch of the next block
        if constexpr (TP) exchange(h);
        if (l == 3) stamp(a.dbg, 7);
    }
    if (a.dbg) stamp(a.dbg, 10);
    if (a.out.Xn != nullptr) {
        // ---- output stage: x0 = h . Wout^T + b (there is no final LayerNorm, models/denoiser.py:188-195), then
        //      x_next = c0*x0 + c1*x_t + sigma*eps.  bf16(h) goes to XN with the usual swizzle.
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int slot = 8 * wave + 2 * nf + (g >> 1);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
                *reinterpret_cast<bf16x4*>(XN + (mf * 16 + lr) * 1024 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(h[nf][mf]);
        }
        __syncthreads();
        for (int c = member; c < SYN_C / kNT; c += P) {          // (tp) the output chunks are dealt to the members
            f32x4 acc[4][MF];
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) acc[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            const uint4* wo = a.out.W + ((size_t)(c * 32 + wave * 4) * KS1) * 64 + lane;
            uint4 ro[4][4];
            kloop_prime<4, 1, KS1, 4>(ro, wo, KS1, 0);
            kloop_run<MF, 4, 1, 0, KS1, 1024, 4>(acc, ro, XN, wo, KS1, 0);
            if (a.dbg) stamp(a.dbg, 11 + 2 * c);
            // Epilogue.  An accumulator fragment holds 4 features of 16 tokens per lane, which would touch global
            // memory as 16 half cache lines per instruction; each wave turns its 16 x 64 tile through LDS (region B is
            // free here) so that 16 consecutive lanes cover 256 contiguous bytes of one row.  x_t of a row tile is
            // requested one tile ahead: this is a read-modify-write of 960 KB per workgroup and every workgroup of the
            // chip is in it at the same time.
            int el = lane;
            asm volatile("" : "+v"(el));       // keeps the row addresses below out of the registers live across the GEMM
            const int er = el >> 4, ec = (el & 15) * 4, ncol = c * kNT + wave * 64 + ec;
            float* const T = reinterpret_cast<float*>(RB) + wave * (16 * 68);
            const bool nz_buf = a.out.noise != nullptr, nz_rng = !nz_buf && a.out.rng != nullptr;
            const f32x4 bias = *reinterpret_cast<const f32x4*>(a.out.bias + ncol);
            // (EDIT, 64-row tiles: x_t of a row tile is requested when the tile comes up, not one ahead - the blend's operands take the registers
            //  of the second slot.  One ahead this instance spills 15 VGPRs / 44 B of scratch, this way 9 / 32 B; the plain one 6 / 28 B.)
            constexpr bool AHEAD = !(EDIT && MT == 64);
            f32x4 xt[AHEAD ? 2 : 1][4];
            auto fetch = [&](int mf, int slot) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = min(m0 + mf * 16 + i * 4 + er, a.M - 1);
                    xt[slot][i] = *reinterpret_cast<const f32x4*>(a.out.Xt + (size_t)m * SYN_C + ncol);
                }
            };
            if constexpr (AHEAD) fetch(0, 0);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                if constexpr (!AHEAD) fetch(mf, 0);
                else if (mf + 1 < MF) fetch(mf + 1, (mf + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) *reinterpret_cast<f32x4*>(T + lr * 68 + nf * 16 + g * 4) = acc[nf][mf];
                __builtin_amdgcn_wave_barrier();
                f32x4 av[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(T + (i * 4 + er) * 68 + ec);
                __builtin_amdgcn_wave_barrier();
                const int tc = a.out.t_coef[min(m0 + mf * 16, a.M - 1) >> 5];
                const f32x4 cf = *reinterpret_cast<const f32x4*>(a.out.coef + (size_t)tc * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + mf * 16 + i * 4 + er;
                    const bool ok = m < a.M;
                    const size_t off = (size_t)m * SYN_C + ncol;
                    f32x4 x0 = av[i] + bias;
                    if constexpr (EDIT) x0 = edit_x0(a.out.keep, a.out.known, ok ? off : 0, x0);
                    f32x4 xn;
                    if constexpr (EDIT) xn = update_pinned(x0, xt[AHEAD ? mf & 1 : 0][i], cf[0], cf[1]);
                    else xn = x0 * cf[0] + xt[mf & 1][i] * cf[1];
                    if (nz_buf) xn = xn + *reinterpret_cast<const f32x4*>(a.out.noise + (ok ? off : 0)) * cf[2];
                    else if (nz_rng) xn = xn + randn4(a.out.rng[0], (uint64_t)tc, (a.out.rng[1] * (uint64_t)(SYN_T * SYN_C) + off) >> 2) * cf[2];
                    if (ok) {
                        *reinterpret_cast<f32x4*>(a.out.Xn + off) = xn;
                        *reinterpret_cast<bf16x4*>(a.out.Xnb + off) = to_bf16x4(xn);
                        if (a.out.X0) *reinterpret_cast<f32x4*>(a.out.X0 + off) = x0;
                    }
                }
            }
            if (a.dbg) stamp(a.dbg, 12 + 2 * c);
        }
    } else {
    // ---- out: y = bf16(h) (there is no final LayerNorm, models/denoiser.py:188-195), optionally fp32 h ------
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int m = m0 + mf * 16 + lr;
        if (m < a.M)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const size_t off = (size_t)m * kNT + wave * 64 + nf * 16 + g * 4;
                if (a.write_h) *reinterpret_cast<f32x4*>(a.H + off) = h[nf][mf];
                *reinterpret_cast<bf16x4*>(a.Y + off) = to_bf16x4(h[nf][mf]);
            }
    }
    }
    stamp(a.dbg, 8);
    if constexpr (TP) tp_done();
}

// ------------------------------------------------------------------------------------------------
// Guidance combine: hc[c][m][:] = sum_v w[c][v] * H[v*Mb + m][:]  -> bf16 (operand of the output GEMM)
__global__ void k_combine(const float* __restrict__ H, const float* __restrict__ w, int w_stride, int V, int Mb,
                          __bf16* __restrict__ hc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one float4 each
    const size_t per = (size_t)Mb * kNT / 4;
    if (i >= per * 3) return;
    const int c = (int)(i / per);
    const size_t e = (i % per) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const float* wc = w + (e / ((size_t)SYN_T * kNT)) * w_stride + c * V;                 // (row e / 512 belongs to clip row / 32)
    for (int v = 0; v < V; ++v) s = s + *reinterpret_cast<const f32x4*>(H + (size_t)v * Mb * kNT + e) * wc[v];
    *reinterpret_cast<bf16x4*>(hc + (size_t)c * Mb * kNT + e) = to_bf16x4(s);
}

// Guided small batches (k_lat with per-sequence groups): x0 = sum_v w[blk][v] * x0_v, then the same posterior /
// DDIM update and noise as the fused epilogues.  One float4 per thread.
struct UArgs {
    const float* X0v; const float* w; int w_stride; int V, B;
    const float* Xt; const float* noise; const unsigned long long* rng; const float* coef; const int* t_coef;
    float* Xn; __bf16* Xnb; float* X0;
    const unsigned char* keep; const float* known;      // in-painting, as in GArgs
};
__global__ void k_guided_update(const UArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_clip = (size_t)SYN_T * SYN_C / 4, n4 = (size_t)a.B * per_clip;
    if (i >= n4) return;
    const int clip = (int)(i / per_clip);
    const size_t off = i * 4;                                    // element offset in the [B*32][1536] tensors
    const int blk = (int)((off % SYN_C) / kNT);
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < a.V; ++v)
        x0 = x0 + *reinterpret_cast<const f32x4*>(a.X0v + (size_t)v * a.B * SYN_T * SYN_C + off) * a.w[(size_t)clip * a.w_stride + blk * a.V + v];
    if (a.keep) x0 = edit_x0(a.keep, a.known, off, x0);
    const int tc = a.t_coef[clip];
    const f32x4 cf = *reinterpret_cast<const f32x4*>(a.coef + (size_t)tc * 4);
    f32x4 xn = x0 * cf[0] + *reinterpret_cast<const f32x4*>(a.Xt + off) * cf[1];
    if (a.noise) xn = xn + *reinterpret_cast<const f32x4*>(a.noise + off) * cf[2];
    else if (a.rng) xn = xn + randn4(a.rng[0], (uint64_t)tc, (a.rng[1] * (uint64_t)(SYN_T * SYN_C) + off) >> 2) * cf[2];
    *reinterpret_cast<f32x4*>(a.Xn + off) = xn;
    *reinterpret_cast<bf16x4*>(a.Xnb + off) = to_bf16x4(xn);
    if (a.X0) *reinterpret_cast<f32x4*>(a.X0 + off) = x0;
}

// fp32 W[n][k] -> packed bf16 fragments: out[((nf*KS + ks)*64 + lane)*8 + e] = W[16nf + (lane&15)][32ks + 8(lane>>4) + e]
__global__ void k_pack(const float* __restrict__ W, int N, int K, uint4* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int KS = K / 32;
    if (idx >= (N / 16) * KS * 64) return;
    const int lane = idx & 63, f = idx >> 6, ks = f % KS, nf = f / KS;
    const float* src = W + (size_t)(16 * nf + (lane & 15)) * K + 32 * ks + 8 * (lane >> 4);
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    bf16x8 r;
    r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
    r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    out[idx] = __builtin_bit_cast(uint4, r);
}

// Same fragments for W = S^T, S row-major [K][N] in fp32 or bf16: the training path packs W^T (dgrad) and x^T (wgrad)
// straight from the tensors it already has instead of materialising transposed fp32 copies first.
template <typename T>
__global__ void k_pack_t(const T* __restrict__ S, int N, int K, uint4* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int KS = K / 32;
    if (idx >= (N / 16) * KS * 64) return;
    const int lane = idx & 63, f = idx >> 6, ks = f % KS, nf = f / KS;
    const T* src = S + (size_t)(32 * ks + 8 * (lane >> 4)) * N + 16 * nf + (lane & 15);
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)(float)src[(size_t)e * N];
    out[idx] = __builtin_bit_cast(uint4, r);
}

// The step's weight packs in ONE launch: job j packs src_j (fp32) as k_pack (transposed = 0: src [n][k]) or as k_pack_t
// (transposed = 1: src [k][n]) into out_j.  Grid (blocks of the largest job, jobs).
struct PackJob { const float* src; uint4* out; int n, k, transposed, src_dim; };
// src_dim > 0: the source's real extent along the PADDED dimension - k of a row-major [n][src_dim] source (transposed = 0), n of a row-major
// [k][src_dim] source (transposed = 1); fragments beyond it are zero (text_encoder_body: 300 -> 384 input features).
__global__ void k_pack_many(const PackJob* __restrict__ jobs) {
    const PackJob j = jobs[blockIdx.y];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int KS = j.k / 32;
    if (idx >= (j.n / 16) * KS * 64) return;
    const int lane = idx & 63, f = idx >> 6, ks = f % KS, nf = f / KS;
    bf16x8 r;
    if (j.transposed) {
        const int ld = j.src_dim > 0 ? j.src_dim : j.n, n = 16 * nf + (lane & 15);
        const float* src = j.src + (size_t)(32 * ks + 8 * (lane >> 4)) * ld + n;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = n < ld ? (__bf16)src[(size_t)e * ld] : (__bf16)0.f;
    } else if (j.src_dim > 0) {
        const int k0 = 32 * ks + 8 * (lane >> 4);
        const float* src = j.src + (size_t)(16 * nf + (lane & 15)) * j.src_dim + k0;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = k0 + e < j.src_dim ? (__bf16)src[e] : (__bf16)0.f;
    } else {
        const float* src = j.src + (size_t)(16 * nf + (lane & 15)) * j.k + 32 * ks + 8 * (lane >> 4);
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
        r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
        r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    }
    j.out[idx] = __builtin_bit_cast(uint4, r);
}

// Conv1d(k = 15) weight w[co][ci][15] (fp32) -> the two packed fragment sets (hi, lo bf16 halves) of the training-mode
// GEMM matrix W'[n][tap * cin + c] (taps zero-padded to KT * stride): one launch instead of ten tensor operations per use.
// transposed = 1: the matrix of the data gradient of a stride-1 convolution, n = ci, c = co, tap reversed.
// transposed = 2: the data gradient of a STRIDED, unpadded convolution read as a stride-1 one from dy (cout channels) to rows of
// stride * cin channels: W''[n = r cin + ci][i][co] = w[co][ci][(taps - 1 - i) stride + r], taps = kt_stride (the tap count here).
__device__ __forceinline__ void conv_pack_split(const float* __restrict__ w, int cout, int cin, int kt_stride, int transposed, int stride,
                                                uint4* __restrict__ out_hi, uint4* __restrict__ out_lo, const int idx) {
    const int N = transposed == 2 ? stride * cin : (transposed ? cin : cout), C = transposed ? cout : cin, K = kt_stride * C, KS = K / 32;
    if (idx >= (N / 16) * KS * 64) return;
    const int lane = idx & 63, f = idx >> 6, ks = f % KS, nf = f / KS;
    const int n = 16 * nf + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
    bf16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e, tap = k / C, c = k - tap * C;
        float v = 0.f;
        if (transposed == 2) {
            const int r = n / cin, ci = n - r * cin, t = (kt_stride - 1 - tap) * stride + r;
            if (t < 15) v = w[((size_t)c * cin + ci) * 15 + t];
        } else if (tap < 15) {
            v = transposed ? w[((size_t)c * cin + n) * 15 + (14 - tap)] : w[((size_t)n * cin + c) * 15 + tap];
        }
        h[e] = (__bf16)v;
        l[e] = (__bf16)(v - (float)h[e]);
    }
    out_hi[idx] = __builtin_bit_cast(uint4, h);
    out_lo[idx] = __builtin_bit_cast(uint4, l);
}
__global__ void k_conv_pack_split(const float* __restrict__ w, int cout, int cin, int kt_stride, int transposed, int stride,
                                  uint4* __restrict__ out_hi, uint4* __restrict__ out_lo) {
    conv_pack_split(w, cout, cin, kt_stride, transposed, stride, out_hi, out_lo, blockIdx.x * blockDim.x + threadIdx.x);
}
// every fragment set the training step's convolutions take (forward and data-gradient forms) in ONE launch: the weights only change in
// optimizer.step(); grid y = job, the jobs travel as kernel arguments
constexpr int kConvPackMax = 40;
struct ConvPackJobs { const float* w[kConvPackMax]; uint4* hi[kConvPackMax]; uint4* lo[kConvPackMax]; short cout[kConvPackMax], cin[kConvPackMax];
                      signed char kts[kConvPackMax], mode[kConvPackMax], stride[kConvPackMax]; };
__global__ void k_conv_pack_split_many(const ConvPackJobs j) {
    const int b = blockIdx.y;
    conv_pack_split(j.w[b], j.cout[b], j.cin[b], j.kts[b], j.mode[b], j.stride[b], j.hi[b], j.lo[b], blockIdx.x * blockDim.x + threadIdx.x);
}

// (B,1536,32) <-> (B,32,1536): 64 channels x 32 frames per block through a padded LDS tile.
__global__ __launch_bounds__(256) void k_to_token_major(const float* __restrict__ x, float* __restrict__ of,
                                                         __bf16* __restrict__ ob) {
    __shared__ float tile[64][33];
    const int b = blockIdx.x, c0 = blockIdx.y * 64, tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + i * 256, c = idx >> 5, t = idx & 31;
        tile[c][t] = x[((size_t)b * SYN_C + c0 + c) * 32 + t];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + i * 256, t = idx >> 6, c = idx & 63;
        const float v = tile[c][t];
        const size_t o = ((size_t)b * 32 + t) * SYN_C + c0 + c;
        if (of) of[o] = v;
        if (ob) ob[o] = (__bf16)v;
    }
}

__global__ __launch_bounds__(256) void k_from_token_major(const float* __restrict__ x, float* __restrict__ out) {
    __shared__ float tile[64][33];
    const int b = blockIdx.x, c0 = blockIdx.y * 64, tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + i * 256, t = idx >> 6, c = idx & 63;
        tile[c][t] = x[((size_t)b * 32 + t) * SYN_C + c0 + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = tid + i * 256, c = idx >> 5, t = idx & 31;
        out[((size_t)b * SYN_C + c0 + c) * 32 + t] = tile[c][t];
    }
}

__global__ void k_axpby_rows(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ ab,
                             const int* __restrict__ t_row, long n4, int per_clip4, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int r = t_row[i / per_clip4];
    const float a = ab[2 * r], b = ab[2 * r + 1];
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i], yv = reinterpret_cast<const f32x4*>(y)[i];
    reinterpret_cast<f32x4*>(out)[i] = xv * a + yv * b;
}

// Sampling loops: the timestep vectors of the next step from a device-resident schedule, so that a loop iteration is
// one graph replay and nothing else on the host.  sched[i] = {row of the coefficient table, original timestep};
// *counter is advanced by the kernel (single workgroup).
// n_steps > 1: the vectors of the next n_steps steps at once, row s of t_model [n_steps][n_tm] / t_coef [n_steps][n_tc]
// for step i + s (a graph of n_steps captured steps reads one row each: one of these per replay instead of one per step).
__global__ void k_step_advance(const int* __restrict__ sched, int* __restrict__ counter, int* __restrict__ t_model, int n_tm,
                               int* __restrict__ t_coef, int n_tc, int n_steps) {
    const int i = *counter;
    for (int s = 0; s < n_steps; ++s) {
        const int tc = sched[2 * (i + s)], tm = sched[2 * (i + s) + 1];
        for (int j = threadIdx.x; j < n_tm; j += blockDim.x) t_model[(size_t)s * n_tm + j] = tm;
        for (int j = threadIdx.x; j < n_tc; j += blockDim.x) t_coef[(size_t)s * n_tc + j] = tc;
    }
    __syncthreads();
    if (threadIdx.x == 0) *counter = i + n_steps;
}

__global__ void k_randn(float* __restrict__ out, long n4, uint64_t seed, uint64_t stream_id, long first4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    reinterpret_cast<f32x4*>(out)[i] = randn4(seed, stream_id, (uint64_t)(first4 + i));
}

// ------------------------------------------------------------------------------------------------
thread_local char g_err[256] = "";
long long* g_dbg_attn = nullptr;   // diagnostics only (syn_debug_timing)
long long* g_dbg_mlp = nullptr;

int fail(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}
int fail_msg(const char* what) {
    snprintf(g_err, sizeof(g_err), "%s", what);
    return -2;
}
int launched(const char* what) {     // after a launch: 0, or the launch's error under the label `what`
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(what, e);
}

static int g_gemm_resident = 2;      // 16-row plain GEMMs: 2 = 16 x 128 tiles, activation block resident in the LDS, deep weight ring; 1 = the same loop on
                                     // 16 x 512 tiles; 0 = the streaming loop (syn_debug_gemm_resident: A/B)

#include "syn_step_plan.inc"
static_assert(kPlanT == SYN_T && kPlanXcds == lat::kGroups, "the step planner restates the sequence length and the XCD count");

int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (cus <= 0) cus = 256;
    }
    return cus;
}

// k_lat is written for 8 XCDs x 32 CUs (MI355X in SPX mode): one workgroup per CU, all co-resident.
bool latency_path_ok() {
    static int ok = -1;
    if (ok < 0) {
        int dev = 0, cus = 0;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        ok = cus == lat::kGroups * lat::kP ? 1 : 0;
    }
    return ok == 1;
}

constexpr int kN128Lds = 128 * 1024;
// Row tile of the 128-column plain GEMM: the largest of 64 / 32 / 16 that still gives every CU a workgroup (fewer bytes through each CU's L1
// port: a workgroup pulls (MT + 128) x K x 2) and whose activation block fits the LDS; 0 = the shape does not fit this kernel at all.
int pick_mt128(int M, int N, int K, int chip_parts = 1) {            // chip_parts 2: the GEMM shares the launch (and the chip) with another one
    if (K * 32 > kN128Lds) return 0;
    const int cus = device_cus();
    for (int mt = 64; mt > 16; mt >>= 1)
        if (mt * K * 2 <= kN128Lds && ((M + mt - 1) / mt) * (N / 128) >= cus * 3 / (4 * chip_parts)) return mt;
    return 16;
}
void n128_setup();

template <int EPI>
int launch_gemm(const GArgs& a, int mt, int chunks, hipStream_t s) {
    if (a.K % 128 != 0 || a.M <= 0) return fail_msg("gemm: K must be a multiple of 128 and M > 0");
    dim3 grid((a.M + mt - 1) / mt, chunks), block(kThreads);
    switch (mt) {
        case 128: hipLaunchKernelGGL((k_gemm<128, EPI>), grid, block, 2 * 128 * 128, s, a); break;
        case 64:  hipLaunchKernelGGL((k_gemm<64, EPI>), grid, block, 2 * 64 * 128, s, a); break;
        case 32:  hipLaunchKernelGGL((k_gemm<32, EPI>), grid, block, 2 * 32 * 128 + 1024, s, a); break;
        case 16:
            if constexpr (EPI == EPI_PLAIN) {
                if (const int m128 = (g_gemm_resident == 2 && !a.ablate) ? pick_mt128(a.M, chunks * kNT, a.K) : 0) {
                    GArgs b = a;
                    b.mt128 = m128;
                    n128_setup();
                    hipLaunchKernelGGL(k_gemm_n128, dim3((a.M + m128 - 1) / m128, chunks * 4), block, m128 * a.K * 2, s, b);
                }
                else if (g_gemm_resident == 1 && a.K <= kResidentMaxK && !a.ablate) hipLaunchKernelGGL((k_gemm<16, EPI, true>), grid, block, a.K * 32, s, a);
                else hipLaunchKernelGGL((k_gemm<16, EPI>), grid, block, 2 * 32 * 128 + 1024, s, a);
                break;
            }
            return fail_msg("gemm: 16-row tiles exist for the plain epilogue only");
        default:  return fail_msg("gemm: m_tile must be 16, 32, 64 or 128");
    }
    return launched("k_gemm launch");
}

template <typename K>
void allow_lds(K kernel, int bytes) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// One-time, PER-DEVICE launch setup (hipFuncSetAttribute applies to the current device's copy of the kernel): a process that
// drives several GPUs (nn.DataParallel replicas, one thread each) raises the LDS limit on every one of them.
constexpr int kMaxDevices = 64;
struct OncePerDevice {
    bool done[kMaxDevices] = {};
    bool first() {                                         // true exactly once per device (callers are serialised per device by their stream)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return true;
        if (done[dev]) return false;
        done[dev] = true;
        return true;
    }
};

void n128_setup() {
    static OncePerDevice once;
    if (once.first()) {
        allow_lds(k_gemm_n128, kN128Lds);
        allow_lds(k_gemm_pair<16, 2>, kN128Lds);
        allow_lds(k_gemm_and_pack<16, 2>, kN128Lds);
        allow_lds(k_gemm_quad_all, kN128Lds);
    }
}

// The nine k_stack instances: whole tiles of 64 / 32 rows, 32-row tiles split over 2 / 4 workgroups and 64-row tiles over 2; the in-painting
// (EDIT) form of the whole tiles and of the split 32-row ones.  Each raises its LDS limit on first use, per device.
struct StackInstance {
    int rows, tp;                    // tp: 0 = whole tiles
    bool edit;
    void (*kernel)(SArgs);
    OncePerDevice once;
    int lds() const { return rows * 2048 + 4096; }
};
StackInstance* stack_instance(int rows, int tp, bool edit) {
    static StackInstance table[] = {
        {64, 0, false, k_stack<64>},          {32, 0, false, k_stack<32>},
        {64, 0, true,  k_stack<64, 0, true>}, {32, 0, true,  k_stack<32, 0, true>}, {32, 2, true, k_stack<32, 2, true>}, {32, 4, true, k_stack<32, 4, true>},
        {32, 2, false, k_stack<32, 2>},       {32, 4, false, k_stack<32, 4>},       {64, 2, false, k_stack<64, 2>},
    };
    for (StackInstance& i : table)
        if (i.rows == rows && i.tp == tp && i.edit == edit) return &i;
    return nullptr;
}

int launch_stack(const SArgs& a, int mt, hipStream_t s) {
    const bool edit = a.out.keep != nullptr;           // in-painting
    dim3 grid((a.M + mt - 1) / mt), block(kThreads);
    if (a.tp > 1) {
        if (!(mt == 32 || (mt == 64 && a.tp == 2)) || !a.sync || !a.xch) return fail_msg("stack: the tile-split mode needs 32-row tiles (or 64-row tiles split in two), ws_sync and ws_xch");
        grid.x = lat::kGroups * a.tp * ((a.tp_tiles + lat::kGroups - 1) / lat::kGroups);    // whole groups on every XCD
        if (grid.x > 256) return fail_msg("stack: the tensor-parallel mode needs all its workgroups resident (<= 256)");
        if (edit && mt != 32) return fail_msg("stack: an edit takes split tiles of 32 rows only");
        if (a.tp != 2 && a.tp != 4) return fail_msg("stack: tile split over 2 or 4 workgroups only");
    }
    StackInstance* const k = stack_instance(mt, a.tp > 1 ? a.tp : 0, edit);
    if (!k) return fail_msg("stack: m_tile must be 32 or 64");
    if (k->once.first()) allow_lds(k->kernel, k->lds());
    hipLaunchKernelGGL(k->kernel, grid, block, k->lds(), s, a);
    return launched("k_stack launch");
}

}  // namespace

// One subsystem per file, included at global scope: each puts its kernels and helpers into (anonymous)::<its namespace> - the unnamed namespace
// above, reopened - and defines its C-ABI entry points behind them, at global scope (inside the unnamed namespace an extern "C" function would
// have internal linkage and not be exported).  syn_conv_train.inc is host code only: the training convolutions' launches over wav:: kernels.
#include "syn_stack_train.inc"
#include "syn_seq.inc"
#include "syn_cond.inc"
#include "syn_wavenc.inc"
#include "syn_train.inc"
#include "syn_conv_train.inc"
#include "syn_glue.inc"
#include "syn_rvq.inc"
#include "syn_rvq_train.inc"
#include "syn_pose.inc"
#include "syn_tmr.inc"
#include "syn_bert.inc"
#include "syn_skel.inc"
#include "syn_t2m.inc"
#include "syn_plms.inc"
#include "syn_bpd.inc"
#include "syn_guide.inc"
#include "syn_joints.inc"
#include "syn_mesh.inc"
#include "syn_render.inc"
#include "syn_plot.inc"
#include "syn_audio.inc"
#include "syn_audio_resample.inc"
#include "syn_jpeg.inc"

namespace {

int launch_latency(const lat::LArgs& a, hipStream_t s) {
    static OncePerDevice once;
    if (once.first()) { allow_lds(lat::k_lat, lat::kLds); }
    hipLaunchKernelGGL(lat::k_lat, dim3(lat::kGroups * lat::kP), dim3(kThreads), lat::kLds, s, a);
    return launched("k_lat launch");
}

template <bool G, int NZ>
void launch_seq_as(const seq::QArgs& a, const dim3 grid, hipStream_t s) {
    static OncePerDevice once;
    if (once.first()) { allow_lds(seq::k_seq<G, NZ>, seq::kLds); }
    hipLaunchKernelGGL((seq::k_seq<G, NZ>), grid, dim3(seq::kThreads), seq::kLds, s, a);
}

int launch_seq(const seq::QArgs& a, hipStream_t s) {
    const dim3 grid(a.n_wg > 0 ? a.n_wg : seq_grid(a.R, a.V));
    const int nz = a.noise ? 1 : a.rng ? 2 : 0;                    // (the noise term is part of the instance: no branch per quad)
    if (a.V == 1) {
        if (nz == 2) launch_seq_as<false, 2>(a, grid, s); else if (nz == 1) launch_seq_as<false, 1>(a, grid, s); else launch_seq_as<false, 0>(a, grid, s);
    } else {
        if (nz == 2) launch_seq_as<true, 2>(a, grid, s); else if (nz == 1) launch_seq_as<true, 1>(a, grid, s); else launch_seq_as<true, 0>(a, grid, s);
    }
    return launched("k_seq launch");
}

}  // namespace

extern "C" {

int syn_version(void) { return SYN_ABI_VERSION; }

/* diagnostics (not part of the public header): per-workgroup cycle stamps of layer 3's fused kernels,
 * 32 slots per workgroup; pass NULL to switch off. */
void syn_debug_timing(long long* attn_buf, long long* mlp_buf) { g_dbg_attn = attn_buf; g_dbg_mlp = mlp_buf; }
const char* syn_last_error(void) { return g_err; }

int syn_pack_weight(const float* w, int32_t n, int32_t k, void* out_packed, void* stream) {
    if (!w || !out_packed || n % 16 || k % 32) return fail_msg("syn_pack_weight: need n%16==0, k%32==0, non-null pointers");
    const int total = (n / 16) * (k / 32) * 64;
    hipLaunchKernelGGL(k_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, n, k, (uint4*)out_packed);
    return launched("k_pack launch");
}

int syn_pack_weights(const syn_pack_job* jobs_dev, int32_t n_jobs, int64_t max_fragments, void* stream) {
    static_assert(sizeof(syn_pack_job) == sizeof(PackJob), "syn_pack_job is PackJob");
    if (!jobs_dev || n_jobs <= 0 || max_fragments <= 0) return fail_msg("syn_pack_weights: bad arguments");
    hipLaunchKernelGGL(k_pack_many, dim3((unsigned)((max_fragments * 64 + 255) / 256), n_jobs), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackJob*>(jobs_dev));
    return launched("k_pack_many launch");
}

int syn_pack_weight_t(const void* s_kn, int32_t is_bf16, int32_t n, int32_t k, void* out_packed, void* stream) {
    if (!s_kn || !out_packed || n % 16 || k % 32) return fail_msg("syn_pack_weight_t: need n%16==0, k%32==0, non-null pointers");
    const int total = (n / 16) * (k / 32) * 64;
    if (is_bf16)
        hipLaunchKernelGGL(k_pack_t<__bf16>, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const __bf16*)s_kn, n, k,
                           (uint4*)out_packed);
    else
        hipLaunchKernelGGL(k_pack_t<float>, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)s_kn, n, k,
                           (uint4*)out_packed);
    return launched("k_pack_t launch");
}

int syn_to_token_major(const float* x_bct, int32_t n_clips, float* out_f32, void* out_bf16, void* stream) {
    if (!x_bct || n_clips <= 0) return fail_msg("syn_to_token_major: bad arguments");
    hipLaunchKernelGGL(k_to_token_major, dim3(n_clips, SYN_C / 64), dim3(256), 0, (hipStream_t)stream, x_bct, out_f32,
                       (__bf16*)out_bf16);
    return launched("k_to_token_major launch");
}

int32_t syn_prefers_fragment_order(int32_t n_clips, int32_t n_variants) { return prefers_fragment_order(n_clips, n_variants, device_cus()); }

int syn_x_to_fragment(const float* x_bct, int32_t n_clips, float* out_f32, void* out_bf16, void* stream) {
    if (!x_bct || n_clips <= 0) return fail_msg("syn_x_to_fragment: bad arguments");
    hipLaunchKernelGGL(seq::k_x_to_fragment, dim3(n_clips, SYN_C / 32), dim3(256), 0, (hipStream_t)stream, x_bct, out_f32, (uint4*)out_bf16);
    return launched("k_x_to_fragment launch");
}

int syn_x_from_fragment(const float* x_frag, int32_t n_clips, float* out_bct, void* stream) {
    if (!x_frag || !out_bct || n_clips <= 0) return fail_msg("syn_x_from_fragment: bad arguments");
    hipLaunchKernelGGL(seq::k_x_from_fragment, dim3(n_clips, SYN_C / 32), dim3(256), 0, (hipStream_t)stream, x_frag, out_bct);
    return launched("k_x_from_fragment launch");
}

int syn_from_token_major(const float* x_btc, int32_t n_clips, float* out_bct, void* stream) {
    if (!x_btc || !out_bct || n_clips <= 0) return fail_msg("syn_from_token_major: bad arguments");
    hipLaunchKernelGGL(k_from_token_major, dim3(n_clips, SYN_C / 64), dim3(256), 0, (hipStream_t)stream, x_btc, out_bct);
    return launched("k_from_token_major launch");
}

int syn_axpby_rows(const float* x, const float* y, const float* coef_ab, const int32_t* t_row, int32_t n_clips,
                   int32_t per_clip, float* out, void* stream) {
    if (!x || !y || !coef_ab || !t_row || !out || n_clips <= 0 || per_clip % 4) return fail_msg("syn_axpby_rows: bad arguments");
    const long n4 = (long)n_clips * per_clip / 4;
    hipLaunchKernelGGL(k_axpby_rows, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, coef_ab,
                       t_row, n4, per_clip / 4, out);
    return launched("k_axpby_rows launch");
}

int syn_steps_advance(const int32_t* sched, int32_t* counter, int32_t* t_model, int32_t n_t_model, int32_t* t_coef, int32_t n_t_coef,
                      int32_t n_steps, void* stream) {
    if (!sched || !counter || !t_model || !t_coef || n_t_model <= 0 || n_t_coef <= 0 || n_steps <= 0)
        return fail_msg("syn_steps_advance: bad arguments");
    hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)sched, (int*)counter, (int*)t_model,
                       n_t_model, (int*)t_coef, n_t_coef, n_steps);
    return launched("k_step_advance launch");
}

int syn_step_advance(const int32_t* sched, int32_t* counter, int32_t* t_model, int32_t n_t_model, int32_t* t_coef, int32_t n_t_coef,
                     void* stream) {
    return syn_steps_advance(sched, counter, t_model, n_t_model, t_coef, n_t_coef, 1, stream);
}

int syn_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t first_index, void* stream) {
    if (!out || n <= 0 || n % 4 || first_index % 4) return fail_msg("syn_randn: n and first_index must be multiples of 4");
    const long n4 = n / 4;
    hipLaunchKernelGGL(k_randn, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n4, seed,
                       stream_id, (long)(first_index / 4));
    return launched("k_randn launch");
}

int syn_test_gemm(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k,
                  int32_t m_tile, float* y, void* stream) {
    if (!x_bf16 || !w_packed || !y || n % kNT) return fail_msg("syn_test_gemm: n must be a multiple of 512");
    GArgs a;
    memset(&a, 0, sizeof(a));
    a.X = (const __bf16*)x_bf16; a.ldx = k; a.x_rows = m_rows; a.W = (const uint4*)w_packed; a.K = k; a.M = m_rows;
    a.bias = bias; a.Yf = y; a.ldyf = n;
    a.ablate = m_tile >> 16;              // diagnostics: upper bits of m_tile
    m_tile &= 0xffff;
    return launch_gemm<EPI_PLAIN>(a, m_tile ? m_tile : pick_tile(m_rows, device_cus()), n / kNT, (hipStream_t)stream);
}

static int g_linear_mt = 0;

static int linear_impl(const void* x_bf16, const void* w_packed, const float* bias, const float* res, const float* rscale, int rows_per_scale,
                       int32_t m_rows, int32_t n, int32_t k, float* y, void* xt_packed, void* stream, const char* who, void* gelu_bf16 = nullptr) {
    if (!x_bf16 || !w_packed || !y || n % 128 || k % 128 || m_rows <= 0 || (rscale && (!res || rows_per_scale <= 0)))
        return fail_msg("syn_linear*: need n % 128 == 0 (n % 512 == 0 for the fused epilogues), k % 128 == 0, m_rows > 0, non-null pointers (a row scale needs the residual and rows_per_scale > 0)");
    if (xt_packed && (m_rows % 32 || k % 16)) return fail_msg("syn_linear_and_pack: the x^T pack needs m_rows % 32 == 0");
    GPack p;
    memset(&p, 0, sizeof(p));
    GArgs& a = p.g;
    a.X = (const __bf16*)x_bf16; a.ldx = k; a.x_rows = m_rows; a.W = (const uint4*)w_packed; a.K = k; a.M = m_rows;
    a.bias = bias; a.Yf = y; a.ldyf = n;
    a.res = res; a.rscale = rscale; a.rows_per_scale = rows_per_scale;
    a.Y = (__bf16*)gelu_bf16;
    if (n % kNT) {
        // 128 or 256 output features (mix_audio_text: 512 -> 256): the 128-column tiles only
        if (g_gemm_resident != 2 || res || gelu_bf16) return fail_msg("syn_linear: n % 512 != 0 needs the plain epilogue (128-column tiles)");
        // The kernel keeps its activation block [row tile][K] resident in the LDS: 4096 of K at 16 rows.  A longer K (the weight gradient of a Linear
        // with 128 / 256 / 384 inputs over more than 4096 rows: text_encoder_body beyond 32 clips) goes out as slices of 4096, every slice after the
        // first adding to what the one before it stored (the residual epilogue reading the output in place) - a fixed order, run-to-run identical.
        constexpr int kSlice = kN128Lds / 32;
        static_assert(kSlice * 32 <= kN128Lds, "a slice's activation block fits the LDS at 16-row tiles, so pick_mt128 never answers 0 for it");
        n128_setup();
        for (int k0 = 0; k0 < k; k0 += kSlice) {
            GArgs b = a;
            b.K = k - k0 < kSlice ? k - k0 : kSlice;
            b.X = a.X + k0; b.W = a.W + (size_t)(k0 / 32) * 64; b.w_ks = k / 32;
            if (k0) { b.bias = nullptr; b.res = y; }
            b.mt128 = pick_mt128(m_rows, n, b.K);
            if (!b.mt128) return fail_msg("syn_linear: a K slice does not fit the 128-column kernel's LDS");
            hipLaunchKernelGGL(k_gemm_n128, dim3((m_rows + b.mt128 - 1) / b.mt128, n / 128), dim3(kThreads), b.mt128 * b.K * 2, (hipStream_t)stream, b);
        }
        if (int rc = launched(who)) return rc;
        return xt_packed ? syn_pack_weight_t(x_bf16, 1, k, m_rows, xt_packed, stream) : 0;
    }
    if (!xt_packed && !res && !gelu_bf16 && m_rows <= 64 && k >= 2048 && g_linear_mt == 0 && g_gemm_resident) {       // a few rows, long K: split K over the waves
        hipLaunchKernelGGL(k_gemm_skinny, dim3(n / 16, (m_rows + 15) / 16), dim3(kThreads), 0, (hipStream_t)stream, a);
        return launched("k_gemm_skinny launch");
    }
    if (!xt_packed || m_rows > 2048 || g_linear_mt > 0) {            // no pack, or larger row tiles: the pack is a launch of its own
        // the training step's GEMMs have 512 .. 1536 rows: 16-row tiles give 32 .. 96 x (n / 512) workgroups, twice what 32-row ones do
        const int mt = g_linear_mt > 0 ? g_linear_mt : (m_rows <= 2048 ? 16 : pick_tile(m_rows, device_cus()));
        if (int rc = launch_gemm<EPI_PLAIN>(a, mt, n / kNT, (hipStream_t)stream)) return rc;
        return xt_packed ? syn_pack_weight_t(x_bf16, 1, k, m_rows, xt_packed, stream) : 0;
    }
    p.src = (const __bf16*)x_bf16; p.out = (uint4*)xt_packed; p.n = k; p.k = m_rows;     // x [m][k] is the row-major [k' = m][n' = k] of x^T [k][m]
    if (const int m128 = g_gemm_resident == 2 ? pick_mt128(m_rows, n, k) : 0) {
        a.mt128 = m128;
        n128_setup();
        hipLaunchKernelGGL((k_gemm_and_pack<16, 2>), dim3((m_rows + m128 - 1) / m128, n / 128, 2), dim3(kThreads), m128 * k * 2, (hipStream_t)stream, p);
    } else if (g_gemm_resident == 1 && k <= kResidentMaxK)
        hipLaunchKernelGGL((k_gemm_and_pack<16, 1>), dim3((m_rows + 15) / 16, n / kNT, 2), dim3(kThreads), k * 32, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((k_gemm_and_pack<16, 0>), dim3((m_rows + 15) / 16, n / kNT, 2), dim3(kThreads), 2 * 32 * 128 + 1024, (hipStream_t)stream, p);
    return launched(who);
}

int syn_linear(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k, float* y,
               void* stream) {
    return linear_impl(x_bf16, w_packed, bias, nullptr, nullptr, 0, m_rows, n, k, y, nullptr, stream, "k_gemm launch");
}

int syn_linear_and_pack(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k, float* y,
                        void* xt_packed, void* stream) {
    if (!xt_packed) return fail_msg("syn_linear_and_pack: xt_packed is NULL");
    return linear_impl(x_bf16, w_packed, bias, nullptr, nullptr, 0, m_rows, n, k, y, xt_packed, stream, "k_gemm_and_pack launch");
}

int syn_linear_gelu(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k, float* y, void* y_gelu_bf16,
                    void* xt_packed, void* stream) {
    if (!y_gelu_bf16) return fail_msg("syn_linear_gelu: y_gelu_bf16 is NULL (use syn_linear)");
    return linear_impl(x_bf16, w_packed, bias, nullptr, nullptr, 0, m_rows, n, k, y, xt_packed, stream, "k_gemm (GELU) launch", y_gelu_bf16);
}

int syn_linear_res(const void* x_bf16, const void* w_packed, const float* bias, const float* residual, const float* row_scale,
                   int32_t rows_per_scale, int32_t m_rows, int32_t n, int32_t k, float* y, void* xt_packed, void* stream) {
    if (!residual) return fail_msg("syn_linear_res: residual is NULL (use syn_linear)");
    return linear_impl(x_bf16, w_packed, bias, residual, row_scale, rows_per_scale, m_rows, n, k, y, xt_packed, stream, "k_gemm (residual) launch");
}

int syn_linear_pair(const void* x1_bf16, const void* w1_packed, int32_t m1, int32_t n1, int32_t k1, float* y1,
                    const void* x2_bf16, const void* w2_packed, int32_t m2, int32_t n2, int32_t k2, float* y2,
                    const float* bias_parts, int32_t part_rows, int32_t part_n, float* bias_grad, void* stream) {
    if (bias_grad && (!bias_parts || part_rows <= 0 || part_n <= 0)) return fail_msg("syn_linear_pair: bias_grad needs bias_parts [part_rows][part_n]");
    if (!x1_bf16 || !w1_packed || !y1 || !x2_bf16 || !w2_packed || !y2 || n1 % 128 || n2 % 128 || k1 % 128 || k2 % 128 || m1 <= 0 || m2 <= 0)
        return fail_msg("syn_linear_pair: need n % 128 == 0, k % 128 == 0, m_rows > 0 and non-null pointers");
    const bool n128 = g_gemm_resident == 2 && pick_mt128(m1, n1, k1) && pick_mt128(m2, n2, k2);
    const bool wide = n1 % kNT == 0 && n2 % kNT == 0;
    if (m1 > 2048 || m2 > 2048 || g_linear_mt > 0 || (!n128 && !wide)) {       // larger row tiles, or a shape only one of the tile forms takes: two launches
        if (int rc = syn_linear(x1_bf16, w1_packed, nullptr, m1, n1, k1, y1, stream)) return rc;
        if (int rc = syn_linear(x2_bf16, w2_packed, nullptr, m2, n2, k2, y2, stream)) return rc;
        if (bias_grad) {
            hipLaunchKernelGGL(glu::k_colsum_parts, dim3((part_n + 63) / 64), dim3(64), 0, (hipStream_t)stream, bias_parts, part_rows, part_n, bias_grad);
            if (int rc = launched("k_colsum_parts launch")) return rc;
        }
        return 0;
    }
    GPair p;
    memset(&p, 0, sizeof(p));
    p.bias_parts = bias_parts; p.bias_grad = bias_grad; p.part_rows = part_rows; p.part_n = part_n;
    const void* xs[2] = {x1_bf16, x2_bf16}; const void* ws[2] = {w1_packed, w2_packed};
    const int ms[2] = {m1, m2}, ns[2] = {n1, n2}, ks[2] = {k1, k2}; float* ys[2] = {y1, y2};
    for (int i = 0; i < 2; ++i) {
        GArgs& a = p.g[i];
        a.X = (const __bf16*)xs[i]; a.ldx = ks[i]; a.x_rows = ms[i]; a.W = (const uint4*)ws[i]; a.K = ks[i]; a.M = ms[i];
        a.Yf = ys[i]; a.ldyf = ns[i];
        p.gx[i] = (ms[i] + 15) / 16; p.gy[i] = ns[i] / kNT;
    }
    const bool fits = k1 <= kResidentMaxK && k2 <= kResidentMaxK;
    int lds128 = 0;
    if (n128)                                                                  // 128-column tiles, the row tile per shape (half a chip each)
        for (int i = 0; i < 2; ++i) {
            const int mt = pick_mt128(ms[i], ns[i], ks[i], 2);
            p.g[i].mt128 = mt; p.gx[i] = (ms[i] + mt - 1) / mt; p.gy[i] = ns[i] / 128;
            lds128 = mt * ks[i] * 2 > lds128 ? mt * ks[i] * 2 : lds128;
        }
    const dim3 grid(p.gx[0] > p.gx[1] ? p.gx[0] : p.gx[1], p.gy[0] > p.gy[1] ? p.gy[0] : p.gy[1], 2);
    if (n128) {
        n128_setup();
        hipLaunchKernelGGL((k_gemm_pair<16, 2>), grid, dim3(kThreads), lds128, (hipStream_t)stream, p);
    } else if (g_gemm_resident == 1 && fits)
        hipLaunchKernelGGL((k_gemm_pair<16, 1>), grid, dim3(kThreads), (k1 > k2 ? k1 : k2) * 32, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((k_gemm_pair<16, 0>), grid, dim3(kThreads), 2 * 32 * 128 + 1024, (hipStream_t)stream, p);
    return launched("k_gemm_pair launch");
}

void syn_debug_gemm_resident(int on) { g_gemm_resident = on; }     /* diagnostics: 0 = the streaming loop for the 16-row plain GEMMs too (A/B) */
void syn_debug_linear_tile(int rows) { g_linear_mt = rows; }       /* diagnostics: pin syn_linear's row tile (16 / 32 / 64 / 128), 0 = automatic */

int syn_test_handoff(uint32_t* sync_320_zeroed, uint32_t* buf_8x4096, const float* stream, int64_t stream_n, uint32_t* stale_9_zeroed,
                     int32_t words, int32_t rounds, int32_t mode, void* stream_h) {
    if (!sync_320_zeroed || !buf_8x4096 || !stale_9_zeroed || words <= 0 || words > 4096 || rounds <= 0 || mode < 0 || mode > 4)
        return fail_msg("syn_test_handoff: bad arguments");
    if (!latency_path_ok()) return fail_msg("syn_test_handoff: needs a 256-CU (8 XCD x 32) device");
    static OncePerDevice once;
    if (once.first()) { allow_lds(lat::k_handoff_stress, 96 * 1024); }
    lat::HArgs a;
    a.sync = sync_320_zeroed; a.buf = buf_8x4096; a.stream = stream; a.stream_n = stream_n; a.stale = stale_9_zeroed;
    a.words = words; a.rounds = rounds; a.mode = mode;
    hipLaunchKernelGGL(lat::k_handoff_stress, dim3(256), dim3(512), 96 * 1024, (hipStream_t)stream_h, a);
    return launched("k_handoff_stress launch");
}

int syn_test_mfma_rate(int32_t iters, float* out, int64_t* flops, void* stream) {
    if (iters <= 0 || !out) return fail_msg("syn_test_mfma_rate: bad arguments (out: 256 floats per CU)");
    static OncePerDevice once;
    if (once.first()) { allow_lds(seq::k_mfma_rate, seq::kLds); }
    const int cus = device_cus();
    hipLaunchKernelGGL(seq::k_mfma_rate, dim3(cus), dim3(seq::kThreads), seq::kLds, (hipStream_t)stream, out, iters);
    if (flops) *flops = (int64_t)cus * 4 * (int64_t)iters * 16 * 12 * (2LL * 32 * 32 * 16);
    return launched("k_mfma_rate launch");
}

int syn_test_attention(const void* q, const void* k, const void* vt, int32_t n_seq, void* o, void* stream) {
    if (!q || !k || !vt || !o || n_seq <= 0) return fail_msg("syn_test_attention: bad arguments");
    hipLaunchKernelGGL(k_attn, dim3(n_seq), dim3(256), 0, (hipStream_t)stream, (const __bf16*)q, (const __bf16*)k,
                       (const __bf16*)vt, (__bf16*)o, n_seq);
    return launched("k_attn launch");
}

int syn_rotary(const float* x, const float* cos_t, const float* sin_t, int32_t n_seq, int32_t inverse, float* y, void* stream) {
    if (!x || !cos_t || !sin_t || !y || n_seq <= 0) return fail_msg("syn_rotary: null pointer / empty batch");
    const long n_tok = (long)n_seq * SYN_T;
    hipLaunchKernelGGL(trn::k_rotary, dim3((unsigned)((n_tok * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, cos_t, sin_t, n_tok, inverse, y);
    return launched("k_rotary launch");
}

// Stage classes reported by syn_denoise_step_profile (index into ms[] / count[]).
enum { ST_IN = 0, ST_QKV = 1, ST_ATTN = 2, ST_PROJ = 3, ST_FC1 = 4, ST_FC2 = 5, ST_COMBINE = 6, ST_OUT = 7, ST_N = 8 };

struct StageTimer {          // optional hipEvent after every launch
    bool on = false;
    hipStream_t s = nullptr;
    hipEvent_t ev[64];
    int cls[64];
    int n = 0;
    void begin(hipStream_t st) { on = true; s = st; hipEventCreate(&ev[0]); hipEventRecord(ev[0], s); n = 1; }
    void mark(int c) {
        if (!on || n >= 64) return;
        hipEventCreate(&ev[n]); hipEventRecord(ev[n], s); cls[n] = c; ++n;
    }
};

// Start-delay spread of a multi-step k_seq launch, in units of 64 cycles across the grid (syn_seq.inc); diagnostics only.
static int g_seq_skew = -1, g_seq_dbg_step = 0;

// ---- one denoising step: validate -> plan_step (syn_step_plan.inc) -> run_seq / run_lat / run_stack / run_layers ---------------------
struct StepCall {            // what every path of a step is handed
    const syn_model* md;
    const syn_step* st;
    const syn_edit* ed;      // in-painting, or nullptr: the four token-major output stages blend it in (syn_denoise_step_edit has refused
                             // the wave-per-sequence kernel, which has no such operand)
    hipStream_t s;
    StageTimer* tm;
    void mark(int c) const { if (tm) tm->mark(c); }
    const unsigned char* keep() const { return ed ? ed->keep : nullptr; }
    const float* known() const { return ed ? ed->known : nullptr; }
};

// k_seq: one wave per sequence, weights streamed once per 128 rows (syn_seq.inc); n_steps > 1: the persistent step loop
static int run_seq(const StepCall& c, int n_steps, int tm_stride, int tc_stride) {
    const syn_model* md = c.md; const syn_step* st = c.st;
    if (!md->tape || !md->tape_bias) return fail_msg("syn_denoise_step: syn_model.tape is not set");
    if (md->tape_chunks * seq::kChunkFrags != 36096) return fail_msg("syn_denoise_step: syn_model.tape_chunks must count 16-fragment chunks of the 36096-fragment tape (2256)");
    seq::QArgs q;
    memset(&q, 0, sizeof(q));
    q.tape = (const char*)md->tape; q.tape_chunks = (unsigned)md->tape_chunks; q.bias = md->tape_bias;
    q.te = md->te; q.rcos = md->rot_cos; q.rsin = md->rot_sin; q.cond = st->cond; q.t_model = st->t_model;
    q.xt = st->x_t; q.xb = (const uint4*)st->x_t_bf16; q.noise = st->noise; q.rng = (const unsigned long long*)st->rng;
    q.coef = st->coef; q.t_coef = st->t_coef; q.xn = st->x_next; q.xnb = (uint4*)st->x_next_bf16; q.x0 = st->pred_x0;
    q.R = st->n_clips; q.V = st->n_variants; q.cfg_w = st->cfg_w; q.cfg_stride = st->cfg_w_clip_stride; q.dbg = g_dbg_mlp;
    q.n_steps = n_steps; q.tm_stride = tm_stride; q.tc_stride = tc_stride; q.dbg_step = g_seq_dbg_step;
    if (n_steps > 1 && st->noise) return fail_msg("syn_denoise_steps: injected noise is per step - run such steps one by one");
    // The persistent step loop wants all its workgroups resident at once (one per CU).  A larger batch goes out as
    // CU-filling slices, each carried through ALL the steps by its own launch (slices are independent: a sequence never
    // leaves its wave); run as one launch, a round of workgroups would finish all its steps before the next one starts
    // and the ragged ends of the rounds add up (measured: -1.7 % at 2048 clips, -2.2 % at 4096 against single steps).
    const int total = seq_grid(q.R, q.V), cus = device_cus();
    if (n_steps > 1 && total > cus) {
        for (int w0 = 0; w0 < total; w0 += cus) {
            q.wg0 = w0; q.n_wg = total - w0 < cus ? total - w0 : cus;
            if (int rc = launch_seq(q, c.s)) return rc;
        }
        c.mark(ST_FC2);
        return launched("syn_denoise_steps");
    }
    q.skew = n_steps > 1 && g_seq_skew > 0 ? (unsigned)g_seq_skew : 0u;      // (diagnostics: imposed start delays, see k_seq)
    if (int rc = launch_seq(q, c.s)) return rc;
    c.mark(ST_FC2);
    return launched("syn_denoise_step");
}

// k_lat: one persistent kernel, output features split over the CUs of an XCD (syn_latency.inc); by_seq: the variants of a guided batch
// leave their x0_hat in ws_x0v and k_guided_update combines them
static int run_lat(const StepCall& c, bool by_seq) {
    const syn_model* md = c.md; const syn_step* st = c.st;
    lat::LArgs la;
    memset(&la, 0, sizeof(la));
    la.w_in = (const uint4*)md->w_in; la.te = md->te; la.rcos = md->rot_cos; la.rsin = md->rot_sin;
    for (int l = 0; l < SYN_LAYERS; ++l) la.layer[l] = md->layer[l];
    la.w_out = (const uint4*)md->w_out; la.b_out = md->b_out;
    la.B = st->n_clips; la.V = st->n_variants;
    la.cond = st->cond; la.t_model = st->t_model; la.cfg_w = st->cfg_w; la.cfg_stride = st->cfg_w_clip_stride;
    la.xb = (const __bf16*)st->x_t_bf16; la.xt = st->x_t; la.noise = st->noise;
    la.rng = (const unsigned long long*)st->rng; la.coef = st->coef; la.t_coef = st->t_coef;
    la.xn = st->x_next; la.xnb = (__bf16*)st->x_next_bf16; la.x0 = st->pred_x0;
    la.keep = c.keep(); la.known = c.known();
    la.H = st->ws_h; la.Q = (__bf16*)st->ws_q; la.Kb = (__bf16*)st->ws_k; la.Vt = (__bf16*)st->ws_vt;
    la.HID = (__bf16*)st->ws_hid; la.sync = st->ws_sync; la.dbg = g_dbg_mlp;
    la.X0v = by_seq ? st->ws_x0v : nullptr;
    if (int rc = launch_latency(la, c.s)) return rc;
    c.mark(ST_FC2);
    if (by_seq) {
        UArgs u;
        u.X0v = st->ws_x0v; u.w = st->cfg_w; u.w_stride = st->cfg_w_clip_stride; u.V = st->n_variants; u.B = st->n_clips; u.Xt = st->x_t; u.noise = st->noise;
        u.rng = (const unsigned long long*)st->rng; u.coef = st->coef; u.t_coef = st->t_coef;
        u.Xn = st->x_next; u.Xnb = (__bf16*)st->x_next_bf16; u.X0 = st->pred_x0;
        u.keep = c.keep(); u.known = c.known();
        const size_t n4 = (size_t)st->n_clips * SYN_T * SYN_C / 4;
        hipLaunchKernelGGL(k_guided_update, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, c.s, u);
        c.mark(ST_OUT);
    }
    return launched("syn_denoise_step");
}

// input stage of the token-major paths: h = rotary(x_t A^T + cond + te[t])
static GArgs step_in_args(const StepCall& c) {
    const syn_model* md = c.md; const syn_step* st = c.st;
    const int Mb = st->n_clips * SYN_T;
    GArgs ain;
    memset(&ain, 0, sizeof(ain));
    ain.X = (const __bf16*)st->x_t_bf16; ain.ldx = SYN_C; ain.x_rows = Mb; ain.W = (const uint4*)md->w_in; ain.K = SYN_C; ain.M = st->n_variants * Mb;
    ain.cond = st->cond; ain.te = md->te; ain.t_model = st->t_model; ain.rcos = md->rot_cos; ain.rsin = md->rot_sin;
    ain.H = st->ws_h; ain.ldy = SYN_D;
    return ain;
}

// output stage of the token-major paths (its input X is set by whoever runs it: k_stack itself, or step_out_stage)
static GArgs step_out_args(const StepCall& c) {
    const syn_model* md = c.md; const syn_step* st = c.st;
    const int Mb = st->n_clips * SYN_T;
    GArgs aout;
    memset(&aout, 0, sizeof(aout));
    aout.ldx = SYN_D; aout.x_rows = Mb; aout.W = (const uint4*)md->w_out; aout.K = SYN_D; aout.M = Mb; aout.bias = md->b_out;
    aout.Xt = st->x_t; aout.noise = st->noise; aout.rng = (const unsigned long long*)st->rng; aout.coef = st->coef;
    aout.t_coef = st->t_coef; aout.Xn = st->x_next; aout.Xnb = (__bf16*)st->x_next_bf16; aout.X0 = st->pred_x0;
    aout.keep = c.keep(); aout.known = c.known();
    return aout;
}

static int step_out_stage(const StepCall& c, int out_tile);

// k_stack: the whole stack in one kernel (production), the output stage inside it when there is a single conditioning variant
static int run_stack(const StepCall& c, const StepPlan& p) {
    const syn_step* st = c.st;
    SArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.H = st->ws_h; sa.Y = (__bf16*)st->ws_xn; sa.M = st->n_variants * st->n_clips * SYN_T; sa.write_h = st->n_variants > 1; sa.dbg = g_dbg_mlp;
    for (int l = 0; l < SYN_LAYERS; ++l) sa.layer[l] = c.md->layer[l];
    sa.in = step_in_args(c);
    if (p.fuse_out) sa.out = step_out_args(c);
    sa.tp = p.tp;
    if (p.tp > 1) { sa.tp_tiles = st->n_variants * st->n_clips; sa.sync = st->ws_sync; sa.xch = st->ws_xch; }
    if (int rc = launch_stack(sa, p.tile_rows, c.s)) return rc;
    c.mark(ST_FC2);
    return p.fuse_out ? launched("syn_denoise_step") : step_out_stage(c, p.out_tile);
}

// five kernels per block, kept as the plain restatement the whole-stack kernel is checked against bit for bit (tests) and for the h8 tap
// it leaves in ws_xn
static int run_layers(const StepCall& c, const StepPlan& p) {
    const syn_model* md = c.md; const syn_step* st = c.st;
    hipStream_t s = c.s;
    const int R = st->n_variants * st->n_clips * SYN_T, mt = p.tile_rows;
    int rc;
    GArgs a = step_in_args(c);           // [; xn = LN1_0(h)]
    a.Y = (__bf16*)st->ws_xn; a.ln_g = md->layer[0].ln1_g; a.ln_b = md->layer[0].ln1_b;
    if ((rc = launch_gemm<EPI_IN>(a, mt, 1, s))) return rc;
    c.mark(ST_IN);
    for (int l = 0; l < SYN_LAYERS; ++l) {
        const syn_layer& L = md->layer[l];
        // qkv
        memset(&a, 0, sizeof(a));
        a.X = (const __bf16*)st->ws_xn; a.ldx = SYN_D; a.x_rows = R; a.W = (const uint4*)L.w_qkv; a.K = SYN_D; a.M = R;
        a.Q = (__bf16*)st->ws_q; a.Kb = (__bf16*)st->ws_k; a.Vt = (__bf16*)st->ws_vt;
        if ((rc = launch_gemm<EPI_QKV>(a, mt, 3, s))) return rc;
        c.mark(ST_QKV);
        // attention
        hipLaunchKernelGGL(k_attn, dim3(R / SYN_T), dim3(256), 0, s, (const __bf16*)st->ws_q, (const __bf16*)st->ws_k,
                           (const __bf16*)st->ws_vt, (__bf16*)st->ws_o, R / SYN_T);
        c.mark(ST_ATTN);
        // proj + residual, LN2 -> xn
        memset(&a, 0, sizeof(a));
        a.X = (const __bf16*)st->ws_o; a.ldx = SYN_D; a.x_rows = R; a.W = (const uint4*)L.w_proj; a.K = SYN_D; a.M = R;
        a.bias = L.b_proj; a.H = st->ws_h; a.Y = (__bf16*)st->ws_xn; a.ldy = SYN_D; a.ln_g = L.ln2_g; a.ln_b = L.ln2_b;
        if ((rc = launch_gemm<EPI_RESID>(a, mt, 1, s))) return rc;
        c.mark(ST_PROJ);
        // fc1 + gelu
        memset(&a, 0, sizeof(a));
        a.X = (const __bf16*)st->ws_xn; a.ldx = SYN_D; a.x_rows = R; a.W = (const uint4*)L.w_fc1; a.K = SYN_D; a.M = R;
        a.bias = L.b_fc1; a.Y = (__bf16*)st->ws_hid; a.ldy = SYN_FF;
        if ((rc = launch_gemm<EPI_GELU>(a, mt, 2, s))) return rc;
        c.mark(ST_FC1);
        // fc2 + residual, next block's LN1 -> xn (last block: plain bf16 copy, there is no final norm)
        memset(&a, 0, sizeof(a));
        a.X = (const __bf16*)st->ws_hid; a.ldx = SYN_FF; a.x_rows = R; a.W = (const uint4*)L.w_fc2; a.K = SYN_FF; a.M = R;
        a.bias = L.b_fc2; a.H = st->ws_h; a.Y = (__bf16*)st->ws_xn; a.ldy = SYN_D;
        if (l + 1 < SYN_LAYERS) { a.ln_g = md->layer[l + 1].ln1_g; a.ln_b = md->layer[l + 1].ln1_b; }
        if ((rc = launch_gemm<EPI_RESID>(a, mt, 1, s))) return rc;
        c.mark(ST_FC2);
    }
    return step_out_stage(c, p.out_tile);
}

// the separate output stage (+ guidance combination of the variants, linear so it commutes with the GEMM)
static int step_out_stage(const StepCall& c, int out_tile) {
    const syn_step* st = c.st;
    const int Mb = st->n_clips * SYN_T;
    GArgs aout = step_out_args(c);
    if (st->n_variants > 1) {
        const size_t n4 = (size_t)3 * Mb * kNT / 4;
        hipLaunchKernelGGL(k_combine, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, c.s, st->ws_h, st->cfg_w, st->cfg_w_clip_stride, st->n_variants, Mb,
                           (__bf16*)st->ws_hc);
        c.mark(ST_COMBINE);
        aout.X = (const __bf16*)st->ws_hc; aout.x_chunk_stride = (long)Mb * kNT;
    } else {
        aout.X = (const __bf16*)st->ws_xn;
    }
    if (int rc = launch_gemm<EPI_OUT>(aout, out_tile, 3, c.s)) return rc;
    c.mark(ST_OUT);
    return launched("syn_denoise_step");
}

static int step_impl(const syn_model* md, const syn_step* st, hipStream_t s, StageTimer* tm, int n_steps = 1, int tm_stride = 0,
                     int tc_stride = 0, const syn_edit* ed = nullptr) {
    if (!md || !st) return fail_msg("syn_denoise_step: null model/step");
    const int B = st->n_clips, V = st->n_variants;
    if (B <= 0 || V <= 0) return fail_msg("syn_denoise_step: n_clips and n_variants must be positive");
    if (V > 1 && (!st->cfg_w || (!st->ws_hc && !st->x_fragment_order))) return fail_msg("syn_denoise_step: n_variants > 1 needs cfg_w and ws_hc");
    if (st->cfg_w_clip_stride != 0 && st->cfg_w_clip_stride != 3 * V) return fail_msg("syn_denoise_step: cfg_w_clip_stride is 0 (one weight table) or 3 * n_variants (one per clip)");
    if (!st->cond || !st->t_model || !st->x_t || !st->x_t_bf16 || !st->coef || !st->t_coef || !st->x_next ||
        !st->x_next_bf16 || !st->ws_h || !st->ws_xn || !st->ws_q || !st->ws_k || !st->ws_vt || !st->ws_o || !st->ws_hid)
        return fail_msg("syn_denoise_step: null state/workspace pointer");
    const StepPlan p = plan_step({B, V, st->m_tile, st->reserved, st->x_fragment_order, st->ws_sync != nullptr, st->ws_xch != nullptr,
                                  st->ws_x0v != nullptr, device_cus(), latency_path_ok()});
    const StepCall c{md, st, ed, s, tm};
    switch (p.path) {
        case STEP_SEQ:    return run_seq(c, n_steps, tm_stride, tc_stride);
        case STEP_LAT:    return run_lat(c, p.by_seq);
        case STEP_STACK:  return run_stack(c, p);
        case STEP_LAYERS: return run_layers(c, p);
        case STEP_ERROR:  break;
    }
    return fail_msg(p.error);
}

int syn_denoise_step(const syn_model* md, const syn_step* st, void* stream) {
    return step_impl(md, st, (hipStream_t)stream, nullptr);
}

int syn_denoise_step_edit(const syn_model* md, const syn_step* st, const syn_edit* ed, void* stream) {
    if (ed && st) {
        if (!ed->keep != !ed->known)
            return fail_msg("syn_denoise_step_edit: syn_edit.keep and syn_edit.known go together (exactly one of them is NULL)");
        if (ed->keep && st->x_fragment_order)
            return fail_msg("syn_denoise_step_edit: x_fragment_order = 1: an edit needs the latent, keep and known token-major (the wave-per-sequence kernel takes no edit)");
        if (ed->keep && (st->reserved & 7) == 5)
            return fail_msg("syn_denoise_step_edit: reserved = 5 pins the wave-per-sequence kernel, which takes no edit");
    }
    return step_impl(md, st, (hipStream_t)stream, nullptr, 1, 0, 0, ed);
}

void syn_debug_seq_skew(int units_of_64_cycles) { g_seq_skew = units_of_64_cycles; }
void syn_debug_seq_step(int step) { g_seq_dbg_step = step; }

int syn_denoise_steps(const syn_model* md, const syn_step* st, int32_t n_steps, int32_t t_model_stride, int32_t t_coef_stride,
                      void* stream) {
    if (!md || !st) return fail_msg("syn_denoise_steps: null model/step");
    if (n_steps <= 0 || t_model_stride < 0 || t_coef_stride < 0) return fail_msg("syn_denoise_steps: n_steps must be positive, strides non-negative");
    if (n_steps > 1 && (st->x_next != st->x_t || st->x_next_bf16 != st->x_t_bf16))
        return fail_msg("syn_denoise_steps: consecutive steps run in place (x_next = x_t, x_next_bf16 = x_t_bf16)");
    if (st->x_fragment_order) return step_impl(md, st, (hipStream_t)stream, nullptr, n_steps, t_model_stride, t_coef_stride);
    // token-major latents: one launch (set) per step, the same kernels syn_denoise_step picks
    syn_step one = *st;
    for (int j = 0; j < n_steps; ++j) {
        one.t_model = st->t_model + (size_t)j * t_model_stride;
        one.t_coef = st->t_coef + (size_t)j * t_coef_stride;
        const int rc = step_impl(md, &one, (hipStream_t)stream, nullptr);
        if (rc) return rc;
    }
    return 0;
}

int syn_denoise_step_profile(const syn_model* md, const syn_step* st, void* stream, float* ms_out, int32_t* count_out) {
    if (!ms_out || !count_out) return fail_msg("syn_denoise_step_profile: null output");
    StageTimer tm;
    tm.begin((hipStream_t)stream);
    const int rc = step_impl(md, st, (hipStream_t)stream, &tm);
    for (int c = 0; c < ST_N; ++c) { ms_out[c] = 0.f; count_out[c] = 0; }
    if (tm.n > 1) hipEventSynchronize(tm.ev[tm.n - 1]);
    for (int i = 1; i < tm.n; ++i) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, tm.ev[i - 1], tm.ev[i]);
        ms_out[tm.cls[i]] += ms;
        count_out[tm.cls[i]] += 1;
    }
    for (int i = 0; i < tm.n; ++i) hipEventDestroy(tm.ev[i]);
    return rc;
}

}  // extern "C"
