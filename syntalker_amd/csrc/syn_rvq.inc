// syn_rvq.inc — RVQ-VAE either side of the denoising loop (SURVEY.md §8 f2; reference models/vq/model.py:53-109,
// encdec.py:4-67, resnet.py:12-83, residual_vq.py:91-165, quantizer.py:62-69,143-171), eval mode.  Included by
// syn_kernels.hip; entry points syn_vq_* at the end.  Once per clip (map2latent before training, latent2origin after sampling): ≈ 1.2 GMAC per body part,
// about three denoising steps' worth for the three parts — this file is about being the reference's callers' drop-in
// on the device, not about peak rate.
//
// Conv1d stack: activations are channels-last [clip][position][channel], kept as fp32 (residual chain, final output)
// with a bf16 shadow that is the MFMA operand.  One kernel covers every convolution of the encoder and decoder:
//   out[t][co] = bias[co] + sum_{tap, ci} W[co][ci][tap] * in[(t*stride + tap*dil - pad) >> up][ci]
// `up` = 1 folds nn.Upsample(scale 2, nearest) into the read of the conv that follows it (encdec.py:55-57); the ReLU
// in front of a conv is applied while its input window is copied to LDS, the one behind it in the epilogue.  Weights
// are the MFMA A operand (fragments [tap][co/16][ci/32][lane] packed on the host, read straight from L2), positions the
// B operand, read from the LDS window: no im2col.
//
// Residual quantiser: fp32 throughout — the index is a discrete decision, a bf16 distance would flip codes.  One
// workgroup owns 16 latent rows (4 when there are few) for all 6 layers: residual rows in LDS, distances against the TRANSPOSED codebook
// (lanes = consecutive codes: coalesced), argmin by wave shuffles, then the reference's straight-through expression
// r + (c - r) so that the rounding of the quantised sum is the reference's.

namespace {
namespace rvq {

struct CvArgs {
    const __bf16* X;        // [clips][t_in][cin] bf16
    const uint4* W;         // fragments [taps][cout/16][cin/32][64]
    const float* bias;      // [cout]
    const float* R;         // residual fp32 [clips][t_out][cout] or null
    float* Yf;              // fp32 out [clips][t_out][ldy] or null
    __bf16* Yb;             // bf16 out [clips][t_out][cout] or null
    int t_in, t_out, cin, cout, cout_valid, ldy;
    int taps, stride, dil, pad, up, relu_in, relu_out;
};

constexpr int kCvThreads = 256;

// workgroup: MF*16 output positions of one clip x 128 output channels; wave = 32 channels x all positions
template <int MF>
__global__ __launch_bounds__(kCvThreads) void k_conv1d(const CvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MT = MF * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, lr = lane & 15;
    const int clip = blockIdx.z, t0 = blockIdx.x * MT, co0 = blockIdx.y * 128 + wave * 32;
    const int KS = a.cin / 32, pitch = a.cin * 2 + 16;
    const int u0 = t0 * a.stride - a.pad;                               // first input coordinate (upsampled frame)
    const int base = u0 >> a.up;                                        // arithmetic shift = floor, also for u0 < 0
    const int nrows = ((u0 + (MT - 1) * a.stride + (a.taps - 1) * a.dil) >> a.up) - base + 1;
    // ---- input window -> LDS (zero rows where the conv pads; optional ReLU) -------------------------------------
    const __bf16* const X = a.X + (size_t)clip * a.t_in * a.cin;
    const int cpr = a.cin / 8;
    for (int c = tid; c < nrows * cpr; c += kCvThreads) {
        const int row = c / cpr, col = c - row * cpr, src = base + row;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (src >= 0 && src < a.t_in) {
            v = *reinterpret_cast<const uint4*>(X + (size_t)src * a.cin + col * 8);
            if (a.relu_in) {
                // bf16 pairs: clear every half whose sign bit is set
                auto relu2 = [](unsigned w) { return w & ~(((w >> 15) & 1u) * 0xFFFFu) & ~(((w >> 31) & 1u) * 0xFFFF0000u); };
                v.x = relu2(v.x); v.y = relu2(v.y); v.z = relu2(v.z); v.w = relu2(v.w);
            }
        }
        *reinterpret_cast<uint4*>(smem + row * pitch + col * 16) = v;
    }
    __syncthreads();

    f32x4 acc[2][MF];
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
    // K loop over (tap, 32-channel step), flattened; weight fragments run 7 steps ahead in a register ring (at one clip
    // the loop is a chain of L2 round trips otherwise)
    const int nco16 = a.cout / 16, total = a.taps * KS;
    auto wptr = [&](int kk) {
        const int tap = kk / KS, ks = kk - tap * KS;
        return a.W + ((size_t)(tap * nco16 + co0 / 16) * KS + ks) * 64 + lane;
    };
    constexpr int RD = 8;                                                // ring depth: RD - 1 K-steps of weights in flight
    uint4 r0[RD], r1[RD];
#pragma unroll
    for (int p = 0; p < RD - 1; ++p)
        if (p < total) { const uint4* q = wptr(p); r0[p] = q[0]; r1[p] = q[(size_t)KS * 64]; }
    for (int kk0 = 0; kk0 < total; kk0 += RD) {
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int kk = kk0 + j;
            if (kk >= total) break;
            if (kk + RD - 1 < total) {
                const uint4* q = wptr(kk + RD - 1);
                r0[(j + RD - 1) % RD] = q[0]; r1[(j + RD - 1) % RD] = q[(size_t)KS * 64];
            }
            const int tap = kk / KS, ks = kk - tap * KS;
            bf16x8 xf[MF];
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int row = ((u0 + (mf * 16 + lr) * a.stride + tap * a.dil) >> a.up) - base;
                xf[mf] = *reinterpret_cast<const bf16x8*>(smem + row * pitch + g * 16 + ks * 64);
            }
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                acc[0][mf] = MFMA16(__builtin_bit_cast(bf16x8, r0[j]), xf[mf], acc[0][mf]);
                acc[1][mf] = MFMA16(__builtin_bit_cast(bf16x8, r1[j]), xf[mf], acc[1][mf]);
            }
        }
    }
    // ---- epilogue: lane holds channels co0 + nf*16 + 4g .. +3 of position t0 + mf*16 + lr -------------------------
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
        const int co = co0 + nf * 16 + g * 4;
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + co);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const int t = t0 + mf * 16 + lr;
            if (t >= a.t_out) continue;
            const size_t row = (size_t)clip * a.t_out + t;
            f32x4 v = acc[nf][mf] + b;
            if (a.R) v = v + *reinterpret_cast<const f32x4*>(a.R + row * a.cout + co);
            if (a.relu_out) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
            if (a.Yf) {
                if (a.cout_valid == a.cout && (a.ldy & 3) == 0) *reinterpret_cast<f32x4*>(a.Yf + row * a.ldy + co) = v;
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (co + r < a.cout_valid) a.Yf[row * a.ldy + co + r] = v[r];
            }
            if (a.Yb) *reinterpret_cast<bf16x4*>(a.Yb + row * a.cout + co) = to_bf16x4(v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int kQ = 6, kCodes = 512, kDim = 512, kQThreads = 256;
// rows per workgroup: 16 amortises the codebook stream; 4 when there are few rows (one clip = 32 rows) so that more CUs work
__host__ __device__ constexpr int q_rows(int rows) { return rows <= 1024 ? 4 : 16; }

struct QArgs {
    const float* X;         // [rows][512] latent rows (token-major: (N, T/4, 512) as latent2origin receives it)
    const float* CB;        // [6][512 codes][512] codebooks (gather)
    const float* CBT;       // [6][512 dims][512 codes] transposed (distance)
    const float* CC;        // [6][512] |c|^2
    float* Qf;              // [rows][512] quantised sum, fp32
    __bf16* Qb;             // same, bf16 (decoder input) or null
    int32_t* idx;           // [rows][6]
    float* sqerr;           // [workgroups][6] sum over this workgroup's rows of |r - c|^2 (commit loss numerators)
    int32_t* hist;          // [6][512] code usage (perplexity), zeroed by the caller
    int rows;
};

template <int kQRows>
__global__ __launch_bounds__(kQThreads) void k_quantize(const QArgs a) {
    __shared__ __attribute__((aligned(16))) float R[kQRows][kDim];      // residual rows
    __shared__ float best_d[4][kQRows];
    __shared__ int best_i[4][kQRows];
    __shared__ int pick[kQRows];
    __shared__ float xx[kQRows];
    __shared__ float err_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * kQRows;
    float out[kQRows][2];                                                // this thread's dims tid, tid + 256 of every row
#pragma unroll
    for (int t = 0; t < kQRows; ++t) {
        const int row = min(r0 + t, a.rows - 1);
        R[t][tid] = a.X[(size_t)row * kDim + tid];
        R[t][tid + 256] = a.X[(size_t)row * kDim + tid + 256];
        out[t][0] = out[t][1] = 0.f;
    }
    __syncthreads();
    for (int q = 0; q < kQ; ++q) {
        // |x|^2 per row: wave w reduces rows w, w + 4, ...
#pragma unroll
        for (int i = 0; i < kQRows / 4; ++i) {
            const int t = wave + 4 * i;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float v = R[t][lane + 64 * k]; s = fmaf(v, v, s); }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) xx[t] = s;
        }
      if constexpr (kQRows == 16) {
        // 16 rows x 512 codes x 512 dims on the fp32 matrix pipe: v_mfma_f32_16x16x4_f32 accumulates its four k in order with
        // one rounding each - the same fmaf chain over d = 0 .. 511 the vector version runs (the index is a discrete decision:
        // test_gpu_rvq holds the reference's indices) - at the packed-vector rate, without a broadcast LDS read per 8 FMAs.
        // A[i][k] = R[i][4 s + k] in lane 16 k + i; B[k][j] in lane 16 k + j: one 16-byte load of codebook row 4 s + k, codes
        // 64 blk + 4 j .. + 3, feeds FOUR MFMAs (column j of tile e is code 64 blk + 4 j + e); a wave owns blocks 2 w, 2 w + 1.
        const int kk = lane >> 4, j = lane & 15;
        const float* ct = a.CBT + (size_t)q * kDim * kCodes + (size_t)kk * kCodes + 128 * wave + 4 * j;
        f32x4 acc[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[b][e] = f32x4{0.f, 0.f, 0.f, 0.f};
        constexpr int PF = 8;                                          // k-steps of codebook rows in flight (L2 latency)
        f32x4 ring[PF][2];
#pragma unroll
        for (int p = 0; p < PF; ++p)
#pragma unroll
            for (int b = 0; b < 2; ++b) ring[p][b] = *reinterpret_cast<const f32x4*>(ct + (size_t)(4 * p) * kCodes + 64 * b);
#pragma unroll 1
        for (int s0 = 0; s0 < kDim / 4; s0 += PF) {
#pragma unroll
            for (int p = 0; p < PF; ++p) {
                const int st = s0 + p;
                const float av = R[j][4 * st + kk];
                const f32x4 b0 = ring[p][0], b1 = ring[p][1];
                const int nx = min(st + PF, kDim / 4 - 1);             // (the tail re-reads the last rows)
#pragma unroll
                for (int b = 0; b < 2; ++b) ring[p][b] = *reinterpret_cast<const f32x4*>(ct + (size_t)(4 * nx) * kCodes + 64 * b);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[0][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0[e], acc[0][e], 0, 0, 0);
                    acc[1][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1[e], acc[1][e], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                                 // xx visible
        // D[i][jj] sits in lane 16 (i / 4) + jj, register i % 4: this lane holds rows 4 kk + r against codes 128 w + 64 b + 4 j + e
        float cc[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.CC + q * kCodes + 128 * wave + 64 * b + 4 * j);
            cc[b][0] = v[0]; cc[b][1] = v[1]; cc[b][2] = v[2]; cc[b][3] = v[3];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = 4 * kk + r;
            const float x2 = xx[t];
            float bd = 0.f; int bi = 0;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 4; ++e) {                           // ascending code index: the first minimum stays
                    const float d = (x2 - 2.f * acc[b][e][r]) + cc[b][e];
                    const int ci = 128 * wave + 64 * b + 4 * j + e;
                    if ((b == 0 && e == 0) || d < bd) { bd = d; bi = ci; }
                }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {                           // the 16 lanes of this row group
                const float od = __shfl_xor(bd, o); const int oi = __shfl_xor(bi, o);
                if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            }
            if (j == 0) { best_d[wave][t] = bd; best_i[wave][t] = bi; }
        }
      } else {
        // dot products of the 16 rows with codes tid and tid + 256
        float dot[kQRows][2];
#pragma unroll
        for (int t = 0; t < kQRows; ++t) dot[t][0] = dot[t][1] = 0.f;
        // codebook columns stream through two register sets, one chunk of CH dims ahead of the FMAs (one wave per SIMD:
        // nothing else hides the L2 latency; deeper for the 4-row variant, whose chunks compute for less time)
        const float* ct = a.CBT + (size_t)q * kDim * kCodes + tid;
        constexpr int CH = kQRows == 4 ? 32 : 16;
        float ca[CH][2], cn[CH][2];
        auto load = [&](float (&c)[CH][2], int d0) {
#pragma unroll
            for (int e = 0; e < CH; ++e) { c[e][0] = ct[(size_t)(d0 + e) * kCodes]; c[e][1] = ct[(size_t)(d0 + e) * kCodes + 256]; }
        };
        auto fma_chunk = [&](const float (&c)[CH][2], int d0) {
#pragma unroll
            for (int e4 = 0; e4 < CH; e4 += 4)
#pragma unroll
                for (int t = 0; t < kQRows; ++t) {
                    const f32x4 r = *reinterpret_cast<const f32x4*>(&R[t][d0 + e4]);      // broadcast read
#pragma unroll
                    for (int e = 0; e < 4; ++e) { dot[t][0] = fmaf(r[e], c[e4 + e][0], dot[t][0]); dot[t][1] = fmaf(r[e], c[e4 + e][1], dot[t][1]); }
                }
        };
        load(ca, 0);
        for (int d = 0; d < kDim; d += 2 * CH) {
            load(cn, d + CH);
            __builtin_amdgcn_sched_barrier(0);
            fma_chunk(ca, d);
            __builtin_amdgcn_sched_barrier(0);
            if (d + 2 * CH < kDim) load(ca, d + 2 * CH);
            __builtin_amdgcn_sched_barrier(0);
            fma_chunk(cn, d + CH);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                                 // xx visible
        const float cc0 = a.CC[q * kCodes + tid], cc1 = a.CC[q * kCodes + tid + 256];
#pragma unroll
        for (int t = 0; t < kQRows; ++t) {
            // quantizer.py:64-66: (|x|^2 - 2 x.c) + |c|^2, smallest distance wins, lowest index on ties (argmax of -d)
            const float d0 = (xx[t] - 2.f * dot[t][0]) + cc0, d1 = (xx[t] - 2.f * dot[t][1]) + cc1;
            float bd = d0; int bi = tid;
            if (d1 < bd) { bd = d1; bi = tid + 256; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float od = __shfl_xor(bd, o); const int oi = __shfl_xor(bi, o);
                if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            }
            if (lane == 0) { best_d[wave][t] = bd; best_i[wave][t] = bi; }
        }
      }
        __syncthreads();
        if (tid < kQRows) {
            float bd = best_d[0][tid]; int bi = best_i[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (best_d[w][tid] < bd || (best_d[w][tid] == bd && best_i[w][tid] < bi)) { bd = best_d[w][tid]; bi = best_i[w][tid]; }
            pick[tid] = bi;
            if (r0 + tid < a.rows) {
                a.idx[(size_t)(r0 + tid) * kQ + q] = bi;
                atomicAdd(a.hist + q * kCodes + bi, 1);
            }
        }
        __syncthreads();
        float err = 0.f;
#pragma unroll
        for (int t = 0; t < kQRows; ++t) {
            const float* c = a.CB + ((size_t)q * kCodes + pick[t]) * kDim;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int d = tid + 256 * h;
                const float r = R[t][d], cv = c[d];
                const float qd = r + (cv - r);                          // quantizer.py:163
                if (r0 + t < a.rows) err = fmaf(r - cv, r - cv, err);
                R[t][d] = r - qd;                                       // residual_vq.py:125
                out[t][h] += qd;                                        // :126
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) err += __shfl_xor(err, o);
        if (lane == 0) err_part[wave] = err;
        __syncthreads();
        if (tid == 0) a.sqerr[(size_t)blockIdx.x * kQ + q] = (err_part[0] + err_part[1]) + (err_part[2] + err_part[3]);
    }
#pragma unroll
    for (int t = 0; t < kQRows; ++t) {
        if (r0 + t >= a.rows) break;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const size_t o = (size_t)(r0 + t) * kDim + tid + 256 * h;
            a.Qf[o] = out[t][h];
            if (a.Qb) a.Qb[o] = (__bf16)out[t][h];
        }
    }
}

// summed codes of given indices (forward_decoder, models/vq/model.py:86-89; residual_vq.py:54-70): rows x 6 -> rows x 512
__global__ void k_codes(const int32_t* idx, const float* CB, float* Qf, __bf16* Qb, int rows, int nq) {
    const int row = blockIdx.x, d = threadIdx.x;                         // 512 threads
    if (row >= rows) return;
    float s = 0.f;
    for (int q = 0; q < nq; ++q) {
        const int i = idx[(size_t)row * nq + q];
        if (i >= 0) s += CB[((size_t)q * kCodes + i) * kDim + d];        // -1 = dropped layer (masked out, :66-68)
    }
    Qf[(size_t)row * kDim + d] = s;
    if (Qb) Qb[(size_t)row * kDim + d] = (__bf16)s;
}

}  // namespace rvq
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int syn_vq_conv1d(const syn_vq_conv* cv, const void* x_bf16, const float* resid, float* y_f32, int32_t ldy, void* y_bf16,
                  int32_t clips, int32_t t_in, int32_t t_out, void* stream) {
    if (!cv || !cv->w_packed || !cv->bias || !x_bf16 || (!y_f32 && !y_bf16) || clips <= 0 || t_in <= 0 || t_out <= 0)
        return fail_msg("syn_vq_conv1d: bad arguments");
    if (cv->cin % 32 || cv->cout % 128 || cv->taps < 1 || cv->stride < 1 || cv->dil < 1 || cv->up < 0 || cv->up > 1)
        return fail_msg("syn_vq_conv1d: cin must be a multiple of 32, cout of 128, up 0 or 1");
    rvq::CvArgs a;
    a.X = (const __bf16*)x_bf16; a.W = (const uint4*)cv->w_packed; a.bias = cv->bias; a.R = resid; a.Yf = y_f32; a.Yb = (__bf16*)y_bf16;
    a.t_in = t_in; a.t_out = t_out; a.cin = cv->cin; a.cout = cv->cout; a.cout_valid = cv->cout_valid; a.ldy = ldy;
    a.taps = cv->taps; a.stride = cv->stride; a.dil = cv->dil; a.pad = cv->pad; a.up = cv->up; a.relu_in = cv->relu_in; a.relu_out = cv->relu_out;
    // 32 output positions per workgroup: its window (34-66 rows, <= 69 KB) lets 2-4 workgroups share a CU; 64-position
    // tiles (one workgroup per CU, half the weight re-reads) measured 5 % slower at 256 clips
    constexpr int mf = 2, mt = mf * 16;
    const int rows = (((mt - 1) * cv->stride + (cv->taps - 1) * cv->dil) >> cv->up) + 2;
    const int lds = rows * (cv->cin * 2 + 16);
    if (lds > 160 * 1024) return fail_msg("syn_vq_conv1d: input window does not fit LDS");
    static OncePerDevice once;
    if (once.first()) { allow_lds(rvq::k_conv1d<2>, 160 * 1024); }
    const dim3 grid((t_out + mt - 1) / mt, cv->cout / 128, clips);
    hipLaunchKernelGGL(rvq::k_conv1d<mf>, grid, dim3(rvq::kCvThreads), lds, (hipStream_t)stream, a);
    return launched("k_conv1d launch");
}

namespace {
int vq_conv(const syn_vq_conv& base, int up, int relu_in, int relu_out, const void* x, const float* resid, float* yf, int ldy, void* yb,
            int clips, int t_in, int t_out, void* stream) {
    syn_vq_conv cv = base;
    cv.up = up; cv.relu_in = relu_in; cv.relu_out = relu_out;
    return syn_vq_conv1d(&cv, x, resid, yf, ldy, yb, clips, t_in, t_out, stream);
}

struct VqWs { float* af; __bf16* ab; float* bf; __bf16* bb; __bf16* hb; __bf16* in; };
VqWs vq_ws(void* ws, int clips, int t_max, int cin_p) {
    const size_t n = (size_t)clips * t_max * rvq::kDim;
    char* p = (char*)ws;
    VqWs w;
    w.af = (float*)p; p += n * 4;
    w.bf = (float*)p; p += n * 4;
    w.ab = (__bf16*)p; p += n * 2;
    w.bb = (__bf16*)p; p += n * 2;
    w.hb = (__bf16*)p; p += n * 2;
    w.in = (__bf16*)p;
    (void)cin_p;
    return w;
}

// Resnet1D (models/vq/resnet.py:71-83): 3 x { x += conv2(relu(conv1(relu(x)))) }, dilations 9, 3, 1, on (af, ab) in place
int vq_resnet(const syn_vq_conv* c, VqWs& w, int clips, int t, void* stream) {
    for (int j = 0; j < 3; ++j) {
        int rc = vq_conv(c[2 * j], 0, 1, 0, w.ab, nullptr, nullptr, 0, w.hb, clips, t, t, stream);
        if (rc) return rc;
        if ((rc = vq_conv(c[2 * j + 1], 0, 1, 0, w.hb, w.af, w.af, rvq::kDim, w.ab, clips, t, t, stream))) return rc;
    }
    return 0;
}

__global__ void k_vq_pose_in(const float* pose, __bf16* out, long rows, int d, int dp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * dp) return;
    const long r = i / dp; const int c = (int)(i - r * dp);
    out[i] = c < d ? (__bf16)pose[r * d + c] : (__bf16)0.f;
}
}  // namespace

int64_t syn_vq_workspace_bytes(int32_t clips, int32_t t_pose, int32_t pose_dim) {
    if (clips <= 0 || t_pose <= 0 || pose_dim <= 0) return -1;
    const int64_t n = (int64_t)clips * t_pose * rvq::kDim;
    const int64_t in_row = ((pose_dim + 31) / 32 * 32) * 2;            // padded bf16 pose row; also holds the quantised rows (256 B per pose frame)
    return n * 14 + (int64_t)clips * t_pose * (in_row > 256 ? in_row : 256) + 256;
}

int syn_vq_map2latent(const syn_vq_model* m, const float* pose, int32_t clips, int32_t t_pose, void* workspace, float* latent,
                      void* stream) {
    if (!m || !pose || !workspace || !latent || clips <= 0 || t_pose <= 0 || t_pose % 4) return fail_msg("syn_vq_map2latent: bad arguments (frames % 4 == 0)");
    const int dp = m->enc[0].cin;
    VqWs w = vq_ws(workspace, clips, t_pose, dp);
    const long rows = (long)clips * t_pose;
    hipLaunchKernelGGL(k_vq_pose_in, dim3((unsigned)((rows * dp + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pose, w.in, rows, m->pose_dim, dp);
    int rc, t = t_pose;
    if ((rc = vq_conv(m->enc[0], 0, 0, 1, w.in, nullptr, w.af, rvq::kDim, w.ab, clips, t, t, stream))) return rc;     // conv + ReLU (encdec.py:23-24)
    for (int i = 0; i < 2; ++i) {
        if ((rc = vq_conv(m->enc[1 + 7 * i], 0, 0, 0, w.ab, nullptr, w.bf, rvq::kDim, w.bb, clips, t, t / 2, stream))) return rc;   // k4 s2 (:27-29)
        t /= 2;
        { float* f = w.af; w.af = w.bf; w.bf = f; __bf16* b = w.ab; w.ab = w.bb; w.bb = b; }
        if ((rc = vq_resnet(m->enc + 2 + 7 * i, w, clips, t, stream))) return rc;
    }
    return vq_conv(m->enc[15], 0, 0, 0, w.ab, nullptr, latent, rvq::kDim, nullptr, clips, t, t, stream);           // (:33)
}

namespace {
int vq_decode(const syn_vq_model* m, VqWs& w, const __bf16* qb, int clips, int t, float* pose_out, void* stream) {
    int rc;
    if ((rc = vq_conv(m->dec[0], 0, 0, 1, qb, nullptr, w.af, rvq::kDim, w.ab, clips, t, t, stream))) return rc;        // conv + ReLU (encdec.py:50-51)
    for (int i = 0; i < 2; ++i) {
        if ((rc = vq_resnet(m->dec + 1 + 7 * i, w, clips, t, stream))) return rc;
        if ((rc = vq_conv(m->dec[7 + 7 * i], 1, 0, 0, w.ab, nullptr, w.bf, rvq::kDim, w.bb, clips, t, 2 * t, stream))) return rc;   // Upsample x2 + conv (:55-57)
        t *= 2;
        { float* f = w.af; w.af = w.bf; w.bf = f; __bf16* b = w.ab; w.ab = w.bb; w.bb = b; }
    }
    if ((rc = vq_conv(m->dec[15], 0, 0, 1, w.ab, nullptr, nullptr, 0, w.hb, clips, t, t, stream))) return rc;          // conv + ReLU (:60-61)
    return vq_conv(m->dec[16], 0, 0, 0, w.hb, nullptr, pose_out, m->pose_dim, nullptr, clips, t, t, stream);          // (:62), (N, T, D)
}
}  // namespace

int syn_vq_latent2origin(const syn_vq_model* m, const float* latent, int32_t clips, int32_t t_lat, void* workspace, float* pose_out,
                         int32_t* idx, float* sqerr, int32_t* hist, void* stream) {
    if (!m || !latent || !workspace || !pose_out || !idx || !sqerr || !hist || clips <= 0 || t_lat <= 0) return fail_msg("syn_vq_latent2origin: bad arguments");
    VqWs w = vq_ws(workspace, clips, 4 * t_lat, m->enc[0].cin);
    // quantised rows: fp32 into bf (free until the first up-conv), bf16 into the input region (the decoder's operand)
    int rc = syn_vq_quantize(latent, m->codebooks, m->codebooks_t, m->code_sq, w.bf, w.in, idx, sqerr, hist, clips * t_lat, stream);
    if (rc) return rc;
    return vq_decode(m, w, w.in, clips, t_lat, pose_out, stream);
}

int syn_vq_forward_decoder(const syn_vq_model* m, const int32_t* idx, int32_t n_q, int32_t clips, int32_t t_lat, void* workspace,
                           float* pose_out, void* stream) {
    if (!m || !idx || !workspace || !pose_out || clips <= 0 || t_lat <= 0) return fail_msg("syn_vq_forward_decoder: bad arguments");
    VqWs w = vq_ws(workspace, clips, 4 * t_lat, m->enc[0].cin);
    int rc = syn_vq_codes(idx, m->codebooks, w.bf, w.in, clips * t_lat, n_q, stream);
    if (rc) return rc;
    return vq_decode(m, w, w.in, clips, t_lat, pose_out, stream);
}

int32_t syn_vq_quantize_groups(int32_t rows) { return (rows + rvq::q_rows(rows) - 1) / rvq::q_rows(rows); }

int syn_vq_quantize(const float* x, const float* codebooks, const float* codebooks_t, const float* code_sq, float* q_f32,
                    void* q_bf16, int32_t* idx, float* sqerr, int32_t* hist, int32_t rows, void* stream) {
    if (!x || !codebooks || !codebooks_t || !code_sq || !q_f32 || !idx || !sqerr || !hist || rows <= 0)
        return fail_msg("syn_vq_quantize: bad arguments");
    rvq::QArgs a;
    a.X = x; a.CB = codebooks; a.CBT = codebooks_t; a.CC = code_sq; a.Qf = q_f32; a.Qb = (__bf16*)q_bf16; a.idx = idx;
    a.sqerr = sqerr; a.hist = hist; a.rows = rows;
    if (rvq::q_rows(rows) == 4) hipLaunchKernelGGL(rvq::k_quantize<4>, dim3(syn_vq_quantize_groups(rows)), dim3(rvq::kQThreads), 0, (hipStream_t)stream, a);
    else                        hipLaunchKernelGGL(rvq::k_quantize<16>, dim3(syn_vq_quantize_groups(rows)), dim3(rvq::kQThreads), 0, (hipStream_t)stream, a);
    return launched("k_quantize launch");
}

int syn_vq_codes(const int32_t* idx, const float* codebooks, float* q_f32, void* q_bf16, int32_t rows, int32_t n_q, void* stream) {
    if (!idx || !codebooks || !q_f32 || rows <= 0 || n_q < 1 || n_q > rvq::kQ) return fail_msg("syn_vq_codes: bad arguments");
    hipLaunchKernelGGL(rvq::k_codes, dim3(rows), dim3(rvq::kDim), 0, (hipStream_t)stream, idx, codebooks, q_f32, (__bf16*)q_bf16, rows, n_q);
    return launched("k_codes launch");
}

}  // extern "C"
