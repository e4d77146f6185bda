// syn_rvq_train.inc — training the body-part RVQ-VAEs (reference rvq_beatx_train.py over models/vq/{model,encdec,resnet,residual_vq,
// quantizer}.py in train mode; DESIGN.md §16).  Included by syn_kernels.hip behind syn_rvq.inc; entry points syn_vq_train_* at the end.
//
// The convolutions of the step run on the eval path's kernel, rvq::k_conv1d, untouched (syn_vq_conv1d): the forward with the bf16 input of
// every convolution kept, the data gradients as the same convolution over tap-flipped, transposed weights (k_pack_jobs below writes both
// fragment sets from the fp32 master weights each step).  What that kernel does not do lives here:
//   k_ew            out = sr * resid + sv * [relu_src > 0] * keep * v      the Dropout(0.2) + residual add behind conv2 (resnet.py:66-67), the ReLU
//                                                                          masks of the backward, the gradient that enters the encoder
//   k_pairsum / k_stuff   the two resampling steps of the backward: nearest-x2 upsample (sum of the two frames a source frame fed) and the
//                         stride-2 convolutions (dy with zeros between its frames, so that their data gradient is a stride-1 convolution)
//   k_wgrad         dW[co][ci][tap] = sum_{n,t} dy[n,t,co] * x[n, (t*s + tap*d - p) >> up, ci] on the bf16 MFMA, fp32 accumulation
//   k_colsum        the bias gradients
//   k_quantize_train / k_tile_init / k_code_update / k_cb_t / k_cb_sq      QuantizeEMAReset.forward in training, one layer per launch
//   k_recons / k_scalars    the reconstruction loss, its gradient and the four numbers a step reports
// Everything is a fixed-order sum: no floating-point atomics, two runs on the same inputs are bit-equal.

namespace {
namespace rvqt {

using rvq::kCodes;
using rvq::kDim;
using rvq::kQ;

// ---- fragment packing from the fp32 master weights ------------------------------------------------------------------------------
// kind 0: conv weight W[cout][cin][taps] -> fragments [taps][cout_p/16][cin_p/32][lane = g*16 + r][8] bf16 (rvqvae.pack_conv)
// kind 1: the data gradient's operand W'[ci][co][taps - 1 - tap] = W[co][ci][tap], same fragment order with (cout_p, cin_p) those of W'
// kind 2: fp32 vector of `cout` entries -> `cout_p` entries, zero padded (the bias of a convolution whose cout is no multiple of 128)
// kind 3: as kind 0, of the part bf16 rounding dropped: bf16(w - float(bf16(w))) - the forward's second weight operand (see k_ew)
struct PackJob { const float* w; void* out; int cout, cin, taps, cout_p, cin_p, kind; };

__global__ __launch_bounds__(256) void k_pack_jobs(const PackJob* __restrict__ jobs) {
    const PackJob j = jobs[blockIdx.y];
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (j.kind == 2) {
        if (u < j.cout_p) reinterpret_cast<float*>(j.out)[u] = u < j.cout ? j.w[u] : 0.f;
        return;
    }
    const int KS = j.cin_p / 32, NF = j.cout_p / 16;
    if (u >= j.taps * NF * KS * 64) return;
    const int lane = u & 63, ks = (u >> 6) % KS, f = ((u >> 6) / KS) % NF, tap = (u >> 6) / (KS * NF);
    const int r = lane & 15, g = lane >> 4, co = 16 * f + r, ci = 32 * ks + 8 * g;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float x = 0.f;
        if (j.kind != 1) { if (co < j.cout && ci + e < j.cin) x = j.w[((size_t)co * j.cin + ci + e) * j.taps + tap]; }
        else             { if (co < j.cin && ci + e < j.cout) x = j.w[((size_t)(ci + e) * j.cin + co) * j.taps + (j.taps - 1 - tap)]; }
        if (j.kind == 3) x -= (float)(__bf16)x;
        v[e] = (__bf16)x;
    }
    reinterpret_cast<bf16x8*>(j.out)[u] = v;
}

// pose fp32 [rows][d] -> bf16 [rows][dp], zero padded; out_lo (optional): what the rounding dropped, bf16(x - float(bf16(x)))
__global__ __launch_bounds__(256) void k_cast_pad(const float* __restrict__ x, __bf16* __restrict__ out, __bf16* __restrict__ out_lo, long n, int d, int dp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long r = i / dp; const int c = (int)(i - r * dp);
    const float v = c < d ? x[r * d + c] : 0.f;
    const __bf16 hi = (__bf16)v;
    out[i] = hi;
    if (out_lo) out_lo[i] = (__bf16)(v - (float)hi);
}

// out = sr * resid + sv * [relu_src > 0] * keep * v, four elements per thread; every operand but v optional.
// out_lo (optional) = bf16(out - float(bf16(out))), the part of out its bf16 copy drops: the training FORWARD feeds each convolution both parts
// (three products W_hi x_hi + W_lo x_hi + W_hi x_lo, DESIGN.md 16.3), so that the ReLU masks of the backward are those of an fp32 forward.
// lo_relu: the consumer applies ReLU to its input - it does so by the SIGN OF THE HIGH PART, so the low part is stored as zero where out <= 0.
__global__ __launch_bounds__(256) void k_ew(const float* __restrict__ v, const float* __restrict__ resid, const __bf16* __restrict__ relu_src,
                                            const unsigned char* __restrict__ keep, float sv, float sr, float* __restrict__ out_f,
                                            __bf16* __restrict__ out_b, __bf16* __restrict__ out_lo, int lo_relu, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 x = *reinterpret_cast<const f32x4*>(v + 4 * i);
    if (relu_src) {
        const bf16x4 m = *reinterpret_cast<const bf16x4*>(relu_src + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) if (!((float)m[e] > 0.f)) x[e] = 0.f;
    }
    if (keep) {
        const unsigned k = *reinterpret_cast<const unsigned*>(keep + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) if (!((k >> (8 * e)) & 0xFFu)) x[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = __fmul_rn(sv, x[e]);
    if (resid) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(resid + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = __fadd_rn(__fmul_rn(sr, r[e]), x[e]);
    }
    if (out_f) *reinterpret_cast<f32x4*>(out_f + 4 * i) = x;
    const bf16x4 hi = to_bf16x4(x);
    if (out_b) *reinterpret_cast<bf16x4*>(out_b + 4 * i) = hi;
    if (out_lo) {
        f32x4 lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) lo[e] = (lo_relu && !((float)hi[e] > 0.f)) ? 0.f : x[e] - (float)hi[e];
        *reinterpret_cast<bf16x4*>(out_lo + 4 * i) = to_bf16x4(lo);
    }
}

// nn.Upsample(x2, nearest) backward: out[r] = du[2 r] + du[2 r + 1] (clips hold an even number of upsampled frames)
__global__ __launch_bounds__(256) void k_pairsum(const float* __restrict__ du, float* __restrict__ out, long n4, int c4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long r = i / c4; const int c = (int)(i - r * c4);
    const f32x4 a = *reinterpret_cast<const f32x4*>(du + ((2 * r) * c4 + c) * 4), b = *reinterpret_cast<const f32x4*>(du + ((2 * r + 1) * c4 + c) * 4);
    *reinterpret_cast<f32x4*>(out + 4 * i) = a + b;
}

// out[2 r] = dy[r], out[2 r + 1] = 0 (bf16 rows of c8 * 8 channels)
__global__ __launch_bounds__(256) void k_stuff(const uint4* __restrict__ dy, uint4* __restrict__ out, long n8, int c8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const long r = i / c8; const int c = (int)(i - r * c8);
    out[(2 * r) * c8 + c] = dy[i];
    out[(2 * r + 1) * c8 + c] = make_uint4(0, 0, 0, 0);
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------------
// One workgroup = 64 output channels x 64 input channels of one tap, the whole sum over K = clips * t_out positions, in chunks of 64.
// Both operands are K-major in memory ([position][channel]) and the MFMA wants 8 consecutive k per lane, so a chunk goes through the LDS
// transposed: a thread loads 8 channels of two neighbouring positions (2 x 16 B, coalesced over channels) and writes 8 dwords, each the
// (k, k + 1) pair of one channel; an image row is one channel's 64 positions (128 B), its 16-byte slots XOR-swizzled with
// s(row) = (row ^ row >> 3) & 7 so that both the transposing ds_write_b32 (8 channel groups x 4 pairs per half wave) and the
// ds_read_b128 of the fragments (16 rows x one slot) touch every bank once.  The next chunk's loads are in flight during the MFMAs.
// Shifted reads (tap * dil - pad) are BOUNDS-CHECKED per position against the clip's own frames: outside them the operand is zero, never
// the neighbouring clip.  Channels past ldy / ldx and positions past K read as zero; stores are masked to cout x cin.
struct WgArgs {
    const __bf16* DY; const __bf16* X; float* dW;
    int ldy, ldx, clips, t_in, t_out, cout, cin, taps, stride, dil, pad, up, relu_in;
};
constexpr int kWgKC = 64, kWgTile = 64;

__device__ __forceinline__ int wg_off(int row, int kdw) {       // byte offset of dword kdw (positions 2 kdw, 2 kdw + 1) of image row `row`
    return row * 128 + ((((kdw >> 2) ^ (row ^ (row >> 3))) & 7) << 4) + ((kdw & 3) << 2);
}

__global__ __launch_bounds__(256) void k_wgrad(const WgArgs a) {
    __shared__ __attribute__((aligned(16))) char sA[kWgTile * 128];     // dy^T [co][k]
    __shared__ __attribute__((aligned(16))) char sB[kWgTile * 128];     // x^T  [ci][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const int co0 = blockIdx.x * kWgTile, ci0 = blockIdx.y * kWgTile, tap = blockIdx.z;
    const int K = a.clips * a.t_out;
    const int kp = tid >> 3, cg = tid & 7;                              // staging role: positions 2 kp, 2 kp + 1 of the chunk, channels 8 cg .. + 7
    const int shift = tap * a.dil - a.pad, t_up = a.t_in << a.up;
    auto load_dy = [&](int k) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < K && co0 + 8 * cg < a.ldy) v = *reinterpret_cast<const uint4*>(a.DY + (size_t)k * a.ldy + co0 + 8 * cg);
        return v;
    };
    auto load_x = [&](int k) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < K && ci0 + 8 * cg < a.ldx) {
            const int n = k / a.t_out, t = k - n * a.t_out, u = t * a.stride + shift;
            if (u >= 0 && u < t_up) {
                v = *reinterpret_cast<const uint4*>(a.X + ((size_t)n * a.t_in + (u >> a.up)) * a.ldx + ci0 + 8 * cg);
                if (a.relu_in) {
                    auto relu2 = [](unsigned w) { return w & ~(((w >> 15) & 1u) * 0xFFFFu) & ~(((w >> 31) & 1u) * 0xFFFF0000u); };
                    v.x = relu2(v.x); v.y = relu2(v.y); v.z = relu2(v.z); v.w = relu2(v.w);
                }
            }
        }
        return v;
    };
    auto stage = [&](char* img, const uint4 lo, const uint4 hi) {       // lo: position 2 kp, hi: 2 kp + 1
        const unsigned l[4] = {lo.x, lo.y, lo.z, lo.w}, h[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<unsigned*>(img + wg_off(8 * cg + 2 * j, kp)) = (l[j] & 0xFFFFu) | (h[j] << 16);
            *reinterpret_cast<unsigned*>(img + wg_off(8 * cg + 2 * j + 1, kp)) = (l[j] >> 16) | (h[j] & 0xFFFF0000u);
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wco = (wave & 1) * 32, wci = (wave >> 1) * 32;
    uint4 d0 = load_dy(2 * kp), d1 = load_dy(2 * kp + 1), x0 = load_x(2 * kp), x1 = load_x(2 * kp + 1);
    for (int k0 = 0; k0 < K; k0 += kWgKC) {
        stage(sA, d0, d1);
        stage(sB, x0, x1);
        __syncthreads();
        if (k0 + kWgKC < K) {
            const int kn = k0 + kWgKC + 2 * kp;
            d0 = load_dy(kn); d1 = load_dy(kn + 1); x0 = load_x(kn); x1 = load_x(kn + 1);
        }
#pragma unroll
        for (int ks = 0; ks < kWgKC / 32; ++ks) {
            bf16x8 af[2], bfr[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = *reinterpret_cast<const bf16x8*>(sA + wg_off(wco + 16 * i + r, 16 * ks + 4 * g));
                bfr[i] = *reinterpret_cast<const bf16x8*>(sB + wg_off(wci + 16 * i + r, 16 * ks + 4 * g));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = MFMA16(af[i], bfr[j], acc[i][j]);
        }
        __syncthreads();
    }
    // D[row = co 4 g + e][col = ci r]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = ci0 + wci + 16 * j + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co0 + wco + 16 * i + 4 * g + e;
                if (co < a.cout && ci < a.cin) a.dW[((size_t)co * a.cin + ci) * a.taps + tap] = acc[i][j][e];
            }
        }
}

// db[c] = sum_k dy[k][c]: 64 channels per workgroup, 16 interleaved partial sums per channel added in order
__global__ __launch_bounds__(1024) void k_colsum(const __bf16* __restrict__ dy, int ld, int K, int cout, float* __restrict__ db) {
    __shared__ float part[16][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), slot = threadIdx.x >> 6;
    float s = 0.f;
    if (c < cout)
        for (int k = slot; k < K; k += 16) s += (float)dy[(size_t)k * ld + c];
    part[slot][threadIdx.x & 63] = s;
    __syncthreads();
    if (slot == 0 && c < cout) {
        float t = part[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < 16; ++i) t += part[i][threadIdx.x];
        db[c] = t;
    }
}

// ---- the quantiser in training -------------------------------------------------------------------------------------------------
// `_tile(x)[:512]` (quantizer.py:49-58 and its callers): row c of x when there are at least 512, else row c % rows plus noise[c] * std
__device__ __forceinline__ float tile_at(const float* __restrict__ x, int rows, const float* __restrict__ noise, float stdv, int c, int d) {
    if (rows >= kCodes) return x[(size_t)c * kDim + d];
    return __fadd_rn(x[(size_t)(c % rows) * kDim + d], __fmul_rn(noise[(size_t)c * kDim + d], stdv));
}

// init_codebook (quantizer.py:60-65): codebook = code_sum = _tile(x)[:512], code_count = 1
__global__ __launch_bounds__(256) void k_tile_init(const float* __restrict__ x, int rows, const float* __restrict__ noise, float stdv,
                                                   float* __restrict__ cb, float* __restrict__ code_sum, float* __restrict__ code_count) {
    const int c = blockIdx.x;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int d = threadIdx.x + 256 * h;
        const float v = tile_at(x, rows, noise, stdv, c, d);
        cb[(size_t)c * kDim + d] = v;
        code_sum[(size_t)c * kDim + d] = v;
    }
    if (threadIdx.x == 0) code_count[c] = 1.f;
}

// codebook [code][dim] -> [dim][code]
__global__ __launch_bounds__(256) void k_cb_t(const float* __restrict__ cb, float* __restrict__ cbt) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, d0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = cb[(size_t)(c0 + ty + 8 * i) * kDim + d0 + tx];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) cbt[(size_t)(d0 + ty + 8 * i) * kCodes + c0 + tx] = tile[tx][ty + 8 * i];
}

// |code|^2 (quantizer.py:73: sum(k_w ** 2, dim = 0)), dims in ascending order
__global__ __launch_bounds__(256) void k_cb_sq(const float* __restrict__ cbt, float* __restrict__ cc) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    for (int d = 0; d < kDim; ++d) { const float v = cbt[(size_t)d * kCodes + c]; s = __fadd_rn(s, __fmul_rn(v, v)); }
    cc[c] = s;
}

// One layer of ResidualVQ.forward in training (residual_vq.py:139-152 over quantizer.py:132-158 without the codebook update): the eval
// kernel's fp32 distances (rvq::k_quantize, vector form), index = argmax(-distance / temperature + gumbel), lowest index on ties.
struct QtArgs {
    const float* Xin;       // [rows][512] this layer's input rows (the residual)
    const float* CB; const float* CBT; const float* CC;     // this layer's codebook, its transpose, |code|^2
    const float* G;         // [rows][512 codes] Gumbel noise, or null (plain argmin)
    float temperature;
    float* Xout;            // [rows][512] residual behind this layer (may not alias Xin: the codebook update reads Xin afterwards)
    float* Qacc;            // [rows][512] sum of the straight-through outputs, accumulated over the layers (`first`: starts it)
    __bf16* Qb;             // the same in bf16 (the decoder's operand), or null
    float* Rsum;            // [rows][512] sum over the layers of (x - x_d): what the commit loss sends back into the encoder
    int32_t* idx;           // [rows][6], column `layer`
    float* sqerr;           // [workgroups] sums of |x - x_d|^2 over the workgroup's rows
    int layer, first, rows;
};

template <int kQRows>
__global__ __launch_bounds__(256) void k_quantize_train(const QtArgs a) {
    __shared__ __attribute__((aligned(16))) float R[kQRows][kDim];
    __shared__ float best_s[4][kQRows];
    __shared__ int best_i[4][kQRows];
    __shared__ int pick[kQRows];
    __shared__ float xx[kQRows];
    __shared__ float err_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * kQRows;
#pragma unroll
    for (int t = 0; t < kQRows; ++t) {
        const int row = min(r0 + t, a.rows - 1);
        R[t][tid] = a.Xin[(size_t)row * kDim + tid];
        R[t][tid + 256] = a.Xin[(size_t)row * kDim + tid + 256];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kQRows / 4; ++i) {                               // |x|^2: wave w reduces rows w, w + 4, ...
        const int t = wave + 4 * i;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float v = R[t][lane + 64 * k]; s = fmaf(v, v, s); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) xx[t] = s;
    }
    float dot[kQRows][2];                                                // rows x codes tid, tid + 256
#pragma unroll
    for (int t = 0; t < kQRows; ++t) dot[t][0] = dot[t][1] = 0.f;
    const float* ct = a.CBT + tid;
    constexpr int CH = 16;
    for (int d0 = 0; d0 < kDim; d0 += CH) {
        float c[CH][2];
#pragma unroll
        for (int e = 0; e < CH; ++e) { c[e][0] = ct[(size_t)(d0 + e) * kCodes]; c[e][1] = ct[(size_t)(d0 + e) * kCodes + 256]; }
#pragma unroll
        for (int e4 = 0; e4 < CH; e4 += 4)
#pragma unroll
            for (int t = 0; t < kQRows; ++t) {
                const f32x4 rv = *reinterpret_cast<const f32x4*>(&R[t][d0 + e4]);       // broadcast read
#pragma unroll
                for (int e = 0; e < 4; ++e) { dot[t][0] = fmaf(rv[e], c[e4 + e][0], dot[t][0]); dot[t][1] = fmaf(rv[e], c[e4 + e][1], dot[t][1]); }
            }
    }
    __syncthreads();                                                     // xx visible
    const float cc0 = a.CC[tid], cc1 = a.CC[tid + 256];
#pragma unroll
    for (int t = 0; t < kQRows; ++t) {
        const int row = min(r0 + t, a.rows - 1);
        // quantizer.py:69-73 then :27: (|x|^2 - 2 x.c) + |c|^2; logits = -distance / temperature + noise; the largest wins
        float s0 = -((xx[t] - 2.f * dot[t][0]) + cc0), s1 = -((xx[t] - 2.f * dot[t][1]) + cc1);
        if (a.G) {
            s0 = __fadd_rn(__fdiv_rn(s0, a.temperature), a.G[(size_t)row * kCodes + tid]);
            s1 = __fadd_rn(__fdiv_rn(s1, a.temperature), a.G[(size_t)row * kCodes + tid + 256]);
        }
        float bs = s0; int bi = tid;
        if (s1 > bs) { bs = s1; bi = tid + 256; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o); const int oi = __shfl_xor(bi, o);
            if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) { best_s[wave][t] = bs; best_i[wave][t] = bi; }
    }
    __syncthreads();
    if (tid < kQRows) {
        float bs = best_s[0][tid]; int bi = best_i[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (best_s[w][tid] > bs || (best_s[w][tid] == bs && best_i[w][tid] < bi)) { bs = best_s[w][tid]; bi = best_i[w][tid]; }
        pick[tid] = bi;
        if (r0 + tid < a.rows) a.idx[(size_t)(r0 + tid) * kQ + a.layer] = bi;
    }
    __syncthreads();
    float err = 0.f;
#pragma unroll
    for (int t = 0; t < kQRows; ++t) {
        if (r0 + t >= a.rows) break;
        const float* c = a.CB + (size_t)pick[t] * kDim;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int d = tid + 256 * h;
            const size_t o = (size_t)(r0 + t) * kDim + d;
            const float r = R[t][d], cv = c[d];
            const float diff = __fadd_rn(r, -cv);
            const float qd = __fadd_rn(r, __fadd_rn(cv, -r));            // quantizer.py:148: x + (x_d - x)
            err = fmaf(diff, diff, err);
            a.Xout[o] = __fadd_rn(r, -qd);                               // residual_vq.py:146
            const float q = a.first ? qd : __fadd_rn(a.Qacc[o], qd);     // :147
            a.Qacc[o] = q;
            if (a.Qb) a.Qb[o] = (__bf16)q;
            a.Rsum[o] = a.first ? diff : __fadd_rn(a.Rsum[o], diff);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) err += __shfl_xor(err, o);
    if (lane == 0) err_part[wave] = err;
    __syncthreads();
    if (tid == 0) a.sqerr[blockIdx.x] = (err_part[0] + err_part[1]) + (err_part[2] + err_part[3]);
}

// update_codebook (quantizer.py:107-130) for code blockIdx.x: this batch's sum of the rows that chose it (ascending row order) and their
// count, the EMA of both, usage = count >= 1, and the codebook entry - the EMA mean, or `_tile(x)` for an unused code.
__global__ __launch_bounds__(256) void k_code_update(const float* __restrict__ x, const int32_t* __restrict__ idx, int layer, int rows,
                                                     const float* __restrict__ noise, float stdv, float mu, float one_minus_mu,
                                                     float* __restrict__ cb, float* __restrict__ code_sum, float* __restrict__ code_count,
                                                     float* __restrict__ batch_count) {
    __shared__ unsigned char match[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    float s0 = 0.f, s1 = 0.f;
    int cnt = 0;
    for (int base = 0; base < rows; base += 256) {
        const int row = base + tid;
        match[tid] = row < rows && idx[(size_t)row * kQ + layer] == c;
        __syncthreads();
        const int m = min(256, rows - base);
        for (int t = 0; t < m; ++t)
            if (match[t]) {
                s0 = __fadd_rn(s0, x[(size_t)(base + t) * kDim + tid]);
                s1 = __fadd_rn(s1, x[(size_t)(base + t) * kDim + tid + 256]);
                ++cnt;
            }
        __syncthreads();
    }
    const float n_new = __fadd_rn(__fmul_rn(mu, code_count[c]), __fmul_rn(one_minus_mu, (float)cnt));
    const float usage = n_new >= 1.f ? 1.f : 0.f;
    __syncthreads();                                                     // every thread has read the old count
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int d = tid + 256 * h;
        const size_t o = (size_t)c * kDim + d;
        const float s_new = __fadd_rn(__fmul_rn(mu, code_sum[o]), __fmul_rn(one_minus_mu, h ? s1 : s0));
        code_sum[o] = s_new;
        const float rnd = tile_at(x, rows, noise, stdv, c, d);
        cb[o] = __fadd_rn(__fmul_rn(usage, __fdiv_rn(s_new, n_new)), __fmul_rn(1.f - usage, rnd));
    }
    if (tid == 0) { code_count[c] = n_new; batch_count[c] = (float)cnt; }
}

// ---- loss ------------------------------------------------------------------------------------------------------------------------
// kind 0: MSE, 1: L1, 2: SmoothL1 (beta = 1), mean over rows x dim (rvq_beatx_train.py:53-62, :80 with the mask of every channel).
// d_rec bf16 [rows][dp] = d loss / d rec, zero in the padded channels; part[block] = the block's sum of the per-element losses.
constexpr int kLossPer = 16;
__global__ __launch_bounds__(256) void k_recons(const float* __restrict__ rec, const float* __restrict__ gt, long n, int dim, int dp, int kind,
                                                float inv_count, __bf16* __restrict__ d_rec, float* __restrict__ part) {
    __shared__ float wsum[4];
    float s = 0.f;
    const long base = (long)blockIdx.x * 256 * kLossPer;
#pragma unroll
    for (int j = 0; j < kLossPer; ++j) {
        const long i = base + (long)j * 256 + threadIdx.x;
        if (i >= n) continue;
        const long r = i / dp; const int c = (int)(i - r * dp);
        float gr = 0.f;
        if (c < dim) {
            const float d = rec[r * dim + c] - gt[r * dim + c], ad = fabsf(d), sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            if (kind == 0)      { s += d * d; gr = 2.f * d; }
            else if (kind == 1) { s += ad; gr = sg; }
            else                { s += ad < 1.f ? 0.5f * d * d : ad - 0.5f; gr = ad < 1.f ? d : sg; }
        }
        d_rec[i] = (__bf16)(gr * inv_count);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// out[4] = {loss, recons, commit, perplexity}: recons = sum(part) / count; commit = mean over the active layers of sqerr / (rows * 512)
// (quantizer.py:144, residual_vq.py:157); perplexity = mean of exp(-sum p log(p + 1e-7)), p = batch_count / rows (quantizer.py:126-127, :158)
__global__ __launch_bounds__(512) void k_scalars(const float* __restrict__ part, int n_part, float inv_count, const float* __restrict__ sqerr,
                                                 int groups, const float* __restrict__ batch_count, int n_active, int rows, float commit_w,
                                                 float* __restrict__ out) {
    __shared__ float red[512];
    __shared__ float perp[kQ];
    const int tid = threadIdx.x;
    for (int q = 0; q < n_active; ++q) {
        const float p = batch_count[q * kCodes + tid] / (float)rows;
        red[tid] = p * logf(p + 1e-7f);
        __syncthreads();
        for (int o = 256; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) perp[q] = expf(-red[0]);
        __syncthreads();
    }
    if (tid == 0) {
        float rs = 0.f;
        for (int i = 0; i < n_part; ++i) rs += part[i];
        const float recons = rs * inv_count;
        float commit = 0.f, pp = 0.f;
        for (int q = 0; q < n_active; ++q) {
            float e = 0.f;
            for (int gidx = 0; gidx < groups; ++gidx) e += sqerr[(size_t)q * groups + gidx];
            commit += e / ((float)rows * (float)kDim);
            pp += perp[q];
        }
        commit /= (float)n_active; pp /= (float)n_active;
        out[0] = recons + commit_w * commit; out[1] = recons; out[2] = commit; out[3] = pp;
    }
}

}  // namespace rvqt
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int syn_vq_train_pack(const void* jobs_dev, int32_t n_jobs, int32_t max_units, void* stream) {
    if (!jobs_dev || n_jobs <= 0 || max_units <= 0) return fail_msg("syn_vq_train_pack: bad arguments");
    hipLaunchKernelGGL(rvqt::k_pack_jobs, dim3((max_units + 255) / 256, n_jobs), dim3(256), 0, (hipStream_t)stream, (const rvqt::PackJob*)jobs_dev);
    return launched("k_pack_jobs launch");
}

int syn_vq_train_cast(const float* x, int64_t rows, int32_t dim, int32_t dim_padded, void* out_bf16, void* out_lo_bf16, void* stream) {
    if (!x || !out_bf16 || rows <= 0 || dim <= 0 || dim_padded < dim) return fail_msg("syn_vq_train_cast: bad arguments");
    const long n = (long)rows * dim_padded;
    hipLaunchKernelGGL(rvqt::k_cast_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (__bf16*)out_bf16, (__bf16*)out_lo_bf16, n, dim, dim_padded);
    return launched("k_cast_pad launch");
}

int syn_vq_train_ew(const float* v, const float* resid, const void* relu_src_bf16, const uint8_t* keep, float scale_v, float scale_resid,
                    float* out_f32, void* out_bf16, void* out_lo_bf16, int32_t lo_relu, int64_t n, void* stream) {
    if (!v || (!out_f32 && !out_bf16 && !out_lo_bf16) || n <= 0 || n % 4) return fail_msg("syn_vq_train_ew: bad arguments (n % 4 == 0)");
    hipLaunchKernelGGL(rvqt::k_ew, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, resid, (const __bf16*)relu_src_bf16, keep,
                       scale_v, scale_resid, out_f32, (__bf16*)out_bf16, (__bf16*)out_lo_bf16, lo_relu, (long)(n / 4));
    return launched("k_ew launch");
}

int syn_vq_train_pairsum(const float* du, float* out, int64_t rows_out, int32_t channels, void* stream) {
    if (!du || !out || rows_out <= 0 || channels <= 0 || channels % 4) return fail_msg("syn_vq_train_pairsum: bad arguments (channels % 4 == 0)");
    const long n4 = (long)rows_out * (channels / 4);
    hipLaunchKernelGGL(rvqt::k_pairsum, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, du, out, n4, channels / 4);
    return launched("k_pairsum launch");
}

int syn_vq_train_stuff(const void* dy_bf16, void* out_bf16, int64_t rows_in, int32_t channels, void* stream) {
    if (!dy_bf16 || !out_bf16 || rows_in <= 0 || channels <= 0 || channels % 8) return fail_msg("syn_vq_train_stuff: bad arguments (channels % 8 == 0)");
    const long n8 = (long)rows_in * (channels / 8);
    hipLaunchKernelGGL(rvqt::k_stuff, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)dy_bf16, (uint4*)out_bf16, n8, channels / 8);
    return launched("k_stuff launch");
}

int syn_vq_train_wgrad(const void* dy_bf16, int32_t ldy, const void* x_bf16, int32_t ldx, float* dw, float* db, int32_t clips, int32_t t_in,
                       int32_t t_out, int32_t cout, int32_t cin, int32_t taps, int32_t stride, int32_t dil, int32_t pad, int32_t up, int32_t relu_in,
                       void* stream) {
    if (!dy_bf16 || !x_bf16 || !dw || clips <= 0 || t_in <= 0 || t_out <= 0 || cout <= 0 || cin <= 0 || taps <= 0 || stride <= 0 || dil <= 0 || pad < 0 ||
        up < 0 || up > 1 || ldy < cout || ldx < cin || ldy % 8 || ldx % 8 || (int64_t)clips * t_out >= (1ll << 30) || (int64_t)clips * t_in >= (1ll << 30))
        return fail_msg("syn_vq_train_wgrad: bad arguments (row pitches: multiples of 8 channels that hold cout / cin)");
    rvqt::WgArgs a;
    a.DY = (const __bf16*)dy_bf16; a.X = (const __bf16*)x_bf16; a.dW = dw; a.ldy = ldy; a.ldx = ldx; a.clips = clips; a.t_in = t_in; a.t_out = t_out;
    a.cout = cout; a.cin = cin; a.taps = taps; a.stride = stride; a.dil = dil; a.pad = pad; a.up = up; a.relu_in = relu_in;
    hipLaunchKernelGGL(rvqt::k_wgrad, dim3((cout + 63) / 64, (cin + 63) / 64, taps), dim3(256), 0, (hipStream_t)stream, a);
    int rc = launched("k_wgrad launch");
    if (rc || !db) return rc;
    hipLaunchKernelGGL(rvqt::k_colsum, dim3((cout + 63) / 64), dim3(1024), 0, (hipStream_t)stream, (const __bf16*)dy_bf16, ldy, clips * t_out, cout, db);
    return launched("k_colsum launch");
}

int syn_vq_train_codebook_prep(const float* codebook, float* codebook_t, float* code_sq, void* stream) {
    if (!codebook || !codebook_t || !code_sq) return fail_msg("syn_vq_train_codebook_prep: bad arguments");
    hipLaunchKernelGGL(rvqt::k_cb_t, dim3(rvq::kCodes / 32, rvq::kDim / 32), dim3(256), 0, (hipStream_t)stream, codebook, codebook_t);
    hipLaunchKernelGGL(rvqt::k_cb_sq, dim3(rvq::kCodes / 256), dim3(256), 0, (hipStream_t)stream, (const float*)codebook_t, code_sq);
    return launched("k_cb_t / k_cb_sq launch");
}

int syn_vq_train_tile(const float* x, int32_t rows, const float* noise, float* codebook, float* code_sum, float* code_count, void* stream) {
    if (!x || rows <= 0 || (rows < rvq::kCodes && !noise) || !codebook || !code_sum || !code_count) return fail_msg("syn_vq_train_tile: bad arguments (fewer rows than codes need the noise)");
    hipLaunchKernelGGL(rvqt::k_tile_init, dim3(rvq::kCodes), dim3(256), 0, (hipStream_t)stream, x, rows, noise, (float)(0.01 / sqrt((double)rvq::kDim)), codebook, code_sum, code_count);
    return launched("k_tile_init launch");
}

int syn_vq_train_quantize(const float* x_in, const float* codebook, const float* codebook_t, const float* code_sq, const float* gumbel, float temperature,
                          float* x_out, float* q_acc, void* q_bf16, float* resid_sum, int32_t* idx, float* sqerr, int32_t layer, int32_t first, int32_t rows,
                          void* stream) {
    if (!x_in || !codebook || !codebook_t || !code_sq || !x_out || x_out == x_in || !q_acc || !resid_sum || !idx || !sqerr || layer < 0 || layer >= rvq::kQ ||
        rows <= 0 || (gumbel && !(temperature > 0.f)))
        return fail_msg("syn_vq_train_quantize: bad arguments");
    rvqt::QtArgs a;
    a.Xin = x_in; a.CB = codebook; a.CBT = codebook_t; a.CC = code_sq; a.G = gumbel; a.temperature = temperature; a.Xout = x_out; a.Qacc = q_acc;
    a.Qb = (__bf16*)q_bf16; a.Rsum = resid_sum; a.idx = idx; a.sqerr = sqerr; a.layer = layer; a.first = first; a.rows = rows;
    const int groups = syn_vq_quantize_groups(rows);
    if (rvq::q_rows(rows) == 4) hipLaunchKernelGGL(rvqt::k_quantize_train<4>, dim3(groups), dim3(256), 0, (hipStream_t)stream, a);
    else                        hipLaunchKernelGGL(rvqt::k_quantize_train<16>, dim3(groups), dim3(256), 0, (hipStream_t)stream, a);
    return launched("k_quantize_train launch");
}

int syn_vq_train_codebook_update(const float* x_in, const int32_t* idx, int32_t layer, int32_t rows, const float* noise, float mu, float one_minus_mu,
                                 float* codebook, float* code_sum, float* code_count, float* batch_count, void* stream) {
    if (!x_in || !idx || layer < 0 || layer >= rvq::kQ || rows <= 0 || (rows < rvq::kCodes && !noise) || !codebook || !code_sum || !code_count || !batch_count)
        return fail_msg("syn_vq_train_codebook_update: bad arguments (fewer rows than codes need the noise)");
    hipLaunchKernelGGL(rvqt::k_code_update, dim3(rvq::kCodes), dim3(256), 0, (hipStream_t)stream, x_in, idx, layer, rows, noise,
                       (float)(0.01 / sqrt((double)rvq::kDim)), mu, one_minus_mu, codebook, code_sum, code_count, batch_count);
    return launched("k_code_update launch");
}

int32_t syn_vq_train_loss_parts(int64_t rows, int32_t dim_padded) {
    if (rows <= 0 || dim_padded <= 0) return -1;
    return (int32_t)((rows * dim_padded + 256 * rvqt::kLossPer - 1) / (256 * rvqt::kLossPer));
}

int syn_vq_train_loss(const float* rec, const float* gt, int64_t rows, int32_t dim, int32_t dim_padded, int32_t kind, void* d_rec_bf16, float* parts,
                      void* stream) {
    if (!rec || !gt || !d_rec_bf16 || !parts || rows <= 0 || dim <= 0 || dim_padded < dim || kind < 0 || kind > 2) return fail_msg("syn_vq_train_loss: bad arguments");
    hipLaunchKernelGGL(rvqt::k_recons, dim3(syn_vq_train_loss_parts(rows, dim_padded)), dim3(256), 0, (hipStream_t)stream, rec, gt, (long)rows * dim_padded, dim,
                       dim_padded, kind, (float)(1.0 / ((double)rows * dim)), (__bf16*)d_rec_bf16, parts);
    return launched("k_recons launch");
}

int syn_vq_train_scalars(const float* parts, int32_t n_parts, int64_t count, const float* sqerr, int32_t groups, const float* batch_count, int32_t n_active,
                         int32_t rows, float commit_weight, float* out4, void* stream) {
    if (!parts || n_parts <= 0 || count <= 0 || !sqerr || groups <= 0 || !batch_count || n_active < 1 || n_active > rvq::kQ || rows <= 0 || !out4)
        return fail_msg("syn_vq_train_scalars: bad arguments");
    hipLaunchKernelGGL(rvqt::k_scalars, dim3(1), dim3(512), 0, (hipStream_t)stream, parts, n_parts, (float)(1.0 / (double)count), sqerr, groups, batch_count,
                       n_active, rows, commit_weight, out4);
    return launched("k_scalars launch");
}

}  // extern "C"
