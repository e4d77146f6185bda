// syn_wavenc.inc — WavEncoder forward (SURVEY.md §8 f1; reference models/denoiser.py:304-322, BasicBlock
// models/utils/layer.py:144-184), eval mode with BatchNorm folded into the convolutions.  Included by
// syn_kernels.hip; entry points syn_wav_* at the end (the training convolutions' are in syn_conv_train.inc).  Once per clip, outside the denoising loop: 2.31 GMAC per clip, which on the PyTorch-ROCm /
// MIOpen path (naive kernels for the unusual first layers) costs as much as ~70 denoising steps.
//
// Every Conv1d(k = 15) of the encoder becomes ONE kind of MFMA GEMM by two layout choices:
//   * activations are channels-last bf16 [clip][position][channel]: the im2col row of output position l is the
//     CONTIGUOUS window of 15 input rows starting at row l (plus a zero halo of 7 rows where the conv pads), so
//     no im2col is ever materialised - the B operand fragments are read straight out of an LDS copy of the tile;
//   * a stride-s conv reads rows l*s .. l*s+14 = the s-row groups l .. l+ceil(15/s)-1: viewing s consecutive rows
//     as one row of s*Cin channels (free in this layout) turns it into a stride-1 conv with KT = ceil(15/s) taps
//     and Cin' = s*Cin channels (weights re-ordered on the host, taps >= 15 zero).
//   GEMM: D[co][l] = sum_{tap, c} W'[co][tap][c] * X[l + tap][c],  K = KT * Cin', weights = MFMA A operand
//   (packed fragments, streamed L2 -> VGPR through a 3-deep ring like k_stack), positions = B operand, so a lane
//   ends with 4 consecutive output channels of one position: 8-byte channels-last stores.
// The shortcut conv of a down-sampling block has the same input and geometry as conv1: the two run as one GEMM
// with the output channels concatenated (epilogue C1SC).  conv2's epilogue adds the shortcut, applies
// LeakyReLU(0.01) and writes the next block's input.  Block 0 (1 or 2 input channels, stride 5, padding 1700) is one
// kernel of its own, k_block0 below.

namespace {
namespace wav {

enum Epi { E_C1 = 0, E_C1SC = 1, E_C2 = 2 };

struct CArgs {
    const __bf16* X; long x_clip_stride; int x_off; int x_rows;     // input: row r of the clip at X + clip*stride + x_off + r*CINP; rows >= x_rows read as 0
    int L_out;
    const uint4* W; const float* bias;                               // packed [N/16][K/32] fragments; bias[N]
    __bf16* Z; long z_clip_stride; int z_off;                        // E_C1 / E_C1SC first half / E_C2: lrelu output, row pitch = its channel count
    __bf16* S; long s_clip_stride;                                   // E_C1SC second half (shortcut, no activation)
    const __bf16* R; long r_clip_stride; int r_off;                  // E_C2: residual, same pitch as Z
    float* Yf; long yf_clip_stride;                                  // E_C2 final layer: fp32 output instead of Z
};

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : 0.01f * v; }

// WN x WM waves per workgroup (4 or 8): with 4 waves and a 39-52 KB tile, three workgroups share a CU (12 waves, 170
// VGPRs each) and one's tile staging / epilogue overlaps the others' MFMA loops.  (Two 8-wave workgroups per CU were
// tried via launch bounds: 128 VGPRs -> 24-364 spills, 2x slower.)
template <int CINP, int KT, int WN, int WM, int RF, int EPI>
__global__ __launch_bounds__(WN * WM * 64)
void k_conv(const CArgs a) {
    constexpr int KSB = CINP / 32, KS = KT * KSB, MW = WM * RF * 16, ROWS = MW + KT - 1, PITCH = CINP * 2 + 16;
    constexpr int N = WN * 64, NZ = EPI == E_C1SC ? N / 2 : N;
    static_assert((WN * WM == 8 || WN * WM == 4) && KS % 3 == 0, "4 or 8 waves; the weight ring is unrolled by 3");
    constexpr int NTHR = WN * WM * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, lr = lane & 15;
    const int wn = wave % WN, wm = wave / WN;
    const int clip = blockIdx.y, l0 = blockIdx.x * MW;
    const __bf16* const X = a.X + (size_t)clip * a.x_clip_stride + a.x_off;
    const uint4* const Wq = a.W + ((size_t)(wn * 4) * KS) * 64 + lane;        // fragment (nf, ks) at Wq[(nf*KS + ks)*64]
    uint4 ring[3][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) ring[p][nf] = Wq[((size_t)nf * KS + p) * 64];
    // ---- stage the input tile: rows l0 .. l0 + ROWS - 1, 16 bytes per thread and pass --------------------------
    for (int c = tid; c < ROWS * (CINP / 8); c += NTHR) {
        const int row = c / (CINP / 8), col = c - row * (CINP / 8);
        uint4 v = {0u, 0u, 0u, 0u};
        if (l0 + row < a.x_rows) v = *reinterpret_cast<const uint4*>(X + (size_t)(l0 + row) * CINP + col * 8);
        *reinterpret_cast<uint4*>(smem + row * PITCH + col * 16) = v;
    }
    __syncthreads();
    f32x4 acc[4][RF];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* xb = smem + (wm * RF * 16 + lr) * PITCH + 16 * g;
    int xoff = 0, cb = 0;
    for (int ks0 = 0; ks0 < KS; ks0 += 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int ks = ks0 + u;
            if (ks + 2 < KS)
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) ring[(u + 2) % 3][nf] = Wq[((size_t)nf * KS + ks + 2) * 64];
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 xf[RF];
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) xf[rf] = *reinterpret_cast<const bf16x8*>(xb + rf * 16 * PITCH + xoff);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const bf16x8 wf = __builtin_bit_cast(bf16x8, ring[u][nf]);
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(wf, xf[rf], acc[nf][rf]);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (++cb == KSB) { cb = 0; xoff += PITCH - (KSB - 1) * 64; } else xoff += 64;   // next 32 channels / next tap
        }
    }
    // ---- epilogue ----------------------------------------------------------------------------------------------
#pragma unroll
    for (int rf = 0; rf < RF; ++rf) {
        const int m = l0 + (wm * RF + rf) * 16 + lr;
        if (m >= a.L_out) continue;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = wn * 64 + nf * 16 + 4 * g;
            f32x4 v = acc[nf][rf] + *reinterpret_cast<const f32x4*>(a.bias + n);
            if (EPI == E_C1SC && n >= NZ) {
                *reinterpret_cast<bf16x4*>(a.S + (size_t)clip * a.s_clip_stride + (size_t)m * NZ + (n - NZ)) = to_bf16x4(v);
                continue;
            }
            if (EPI == E_C2) {
                const bf16x4 r = *reinterpret_cast<const bf16x4*>(a.R + (size_t)clip * a.r_clip_stride + a.r_off + (size_t)m * NZ + n);
                v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
            }
            v[0] = lrelu(v[0]); v[1] = lrelu(v[1]); v[2] = lrelu(v[2]); v[3] = lrelu(v[3]);
            if (EPI == E_C2 && a.Yf) *reinterpret_cast<f32x4*>(a.Yf + (size_t)clip * a.yf_clip_stride + (size_t)m * NZ + n) = v;
            else *reinterpret_cast<bf16x4*>(a.Z + (size_t)clip * a.z_clip_stride + a.z_off + (size_t)m * NZ + n) = to_bf16x4(v);
        }
    }
}

// Block 0 in one kernel: conv1 (Conv1d(cin, 64, 15, stride 5, padding 1700)) -> LeakyReLU -> conv2 (64 -> 64, k 15,
// padding 7) + shortcut conv (same geometry as conv1) -> LeakyReLU, BatchNorms folded.  conv1 and the shortcut are
// 1 % of the FLOPs but their outputs are the two largest tensors of the encoder (2 x 1.8 MB per clip): instead of a
// round trip through HBM, a workgroup recomputes the conv1 rows its conv2 tile needs (512 + 14 halo rows, one
// K = 32 MFMA step each: 15 taps x cin <= 30 values) straight into the LDS tile, and the shortcut becomes the initial
// value of the conv2 accumulators.  wav fp32 [clip][L][cin] -> X1 bf16 [clip][L1][64].
struct B0Args {
    const float* wav; long wav_clip_stride; int L, cin, L1;
    const float* w_first;          // [2][15*cin][64] fp32 (conv1, shortcut; k = tap*cin + c) then bias [2][64]
    const uint4* W2; const float* bias2;
    __bf16* X1; long x1_clip_stride;
};
#ifndef SYN_B0_WAVES      /* waves per workgroup of k_block0, 64 output positions each.  8: one 86 KB workgroup per CU.  Measured at 64 clips: 4 waves (44 KB
                             tiles, three workgroups per CU) 0.601 ms, 2 waves 0.608 ms against 0.587 ms - overlapping the phases of several
                             workgroups is not what holds this kernel at a fifth of the matrix rate */
#define SYN_B0_WAVES 8
#endif
#ifndef SYN_B0_RING
#define SYN_B0_RING 5      /* 64 clips: 0.602 ms with 3 (two k-steps ahead), 0.577 with 5, 0.582 with 6 */
#endif
constexpr int kB0Waves = SYN_B0_WAVES, kB0Tile = kB0Waves * 64;
constexpr int kB0Rows = kB0Tile + 14, kB0Pitch = 64 * 2 + 16;
constexpr int kB0Win = ((kB0Rows - 1) * 5 + 15 + 8) * 2;        // samples x channels the tile's windows touch (+ tail for k = 30, 31)
constexpr int kB0Lds = kB0Rows * kB0Pitch + kB0Win * 2;

__global__ __launch_bounds__(kB0Waves * 64) void k_block0(const B0Args a) {
    constexpr int CINP = 64, KT = 15, KSB = 2, KS = 30, RF = 4, PITCH = kB0Pitch, kThreads = kB0Waves * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* const win = reinterpret_cast<__bf16*>(smem + kB0Rows * PITCH);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, lr = lane & 15;
    const int clip = blockIdx.y, l0 = blockIdx.x * kB0Tile, cin = a.cin, kk = 15 * cin;
    const uint4* const Wq = a.W2 + lane;                         // conv2 fragment (nf, ks) at Wq[(nf*KS + ks)*64]
    constexpr int RD = SYN_B0_RING;                               // weight ring: RD - 1 k-steps in flight ahead of the MFMAs
    static_assert(KS % RD == 0, "ring depth must divide the 30 k-steps");
    uint4 ring[RD][4];
#pragma unroll
    for (int p = 0; p < RD - 1; ++p)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) ring[p][nf] = Wq[((size_t)nf * KS + p) * 64];
    // ---- waveform window of the tile -> LDS (bf16), zero outside the clip (the conv's own zero padding) ---------
    const long first = ((long)l0 - 7) * 5 - 1700;                // sample of tap 0 of tile row 0
    const float* const wv = a.wav + (size_t)clip * a.wav_clip_stride;
    for (int i = tid; i < kB0Win; i += kThreads) {
        const long smp = first + i / cin;
        win[i] = (__bf16)((cin * (kB0Win / 2) > i && smp >= 0 && smp < a.L) ? wv[smp * cin + (i % cin)] : 0.f);
    }
    // conv1 / shortcut weights as MFMA A fragments: lane (co = 16 nf + lr, k = 8 g .. 8 g + 7), zero for k >= 15 cin
    bf16x8 w1[4], wsc[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 8 * g + e, co = 16 * nf + lr;
            w1[nf][e] = (__bf16)(k < kk ? a.w_first[(size_t)k * 64 + co] : 0.f);
            wsc[nf][e] = (__bf16)(k < kk ? a.w_first[(size_t)(kk + k) * 64 + co] : 0.f);
        }
    __syncthreads();
    auto window = [&](int row) {                                 // B fragment of tile row `row`: 8 consecutive window values
        const __bf16* p = win + (size_t)row * 5 * cin + 8 * g;
        bf16x8 x;
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = p[e];
        return x;
    };
    // ---- conv1 rows of the tile -> LDS (zero where the position is outside [0, L1): conv2 pads with zeros) ---------
    const float* const bias1 = a.w_first + (size_t)2 * kk * 64;
    for (int rt = wave; rt * 16 < kB0Rows; rt += kB0Waves) {
        const int row = rt * 16 + lr;
        const bf16x8 x = window(min(row, kB0Rows - 1));
        const long pos = (long)l0 - 7 + row;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            f32x4 z = MFMA16(w1[nf], x, (f32x4{0.f, 0.f, 0.f, 0.f})) + *reinterpret_cast<const f32x4*>(bias1 + 16 * nf + 4 * g);
            z[0] = lrelu(z[0]); z[1] = lrelu(z[1]); z[2] = lrelu(z[2]); z[3] = lrelu(z[3]);
            if (pos < 0 || pos >= a.L1) z = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < kB0Rows) *reinterpret_cast<bf16x4*>(smem + row * PITCH + (16 * nf + 4 * g) * 2) = to_bf16x4(z);
        }
    }
    // ---- accumulators start from the shortcut conv of their own output rows (tile row = output row + 7) ------------
    f32x4 acc[4][RF];
#pragma unroll
    for (int rf = 0; rf < RF; ++rf) {
        const bf16x8 x = window((wave * RF + rf) * 16 + lr + 7);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
            acc[nf][rf] = MFMA16(wsc[nf], x, (f32x4{0.f, 0.f, 0.f, 0.f})) + *reinterpret_cast<const f32x4*>(bias1 + 64 + 16 * nf + 4 * g);
    }
    __syncthreads();
    // ---- conv2 over the LDS tile (same loop as k_conv<64, 15, 1, 8, 4>) ----------------------------------------------
    const char* xb = smem + (wave * RF * 16 + lr) * PITCH + 16 * g;
    int xoff = 0, cb = 0;
    for (int ks0 = 0; ks0 < KS; ks0 += RD) {
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            const int ks = ks0 + u;
            if (ks + RD - 1 < KS)
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) ring[(u + RD - 1) % RD][nf] = Wq[((size_t)nf * KS + ks + RD - 1) * 64];
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 xf[RF];
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) xf[rf] = *reinterpret_cast<const bf16x8*>(xb + rf * 16 * PITCH + xoff);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const bf16x8 wf = __builtin_bit_cast(bf16x8, ring[u][nf]);
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(wf, xf[rf], acc[nf][rf]);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (++cb == KSB) { cb = 0; xoff += PITCH - (KSB - 1) * 64; } else xoff += 64;
        }
    }
#pragma unroll
    for (int rf = 0; rf < RF; ++rf) {
        const int m = l0 + (wave * RF + rf) * 16 + lr;
        if (m >= a.L1) continue;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = nf * 16 + 4 * g;
            f32x4 v = acc[nf][rf] + *reinterpret_cast<const f32x4*>(a.bias2 + n);
            v[0] = lrelu(v[0]); v[1] = lrelu(v[1]); v[2] = lrelu(v[2]); v[3] = lrelu(v[3]);
            *reinterpret_cast<bf16x4*>(a.X1 + (size_t)clip * a.x1_clip_stride + (size_t)m * 64 + n) = to_bf16x4(v);
        }
    }
}

// ---- training-mode forward (SURVEY.md 8 a10 / f1): the same implicit GEMM on fp32-equivalent operands ------------------
// BatchNorm runs on batch statistics in training, so nothing is folded, the output is the fp32 pre-normalisation tensor, and
// bf16 operands are not enough: rounding the forward activations to bf16 moves the gradients of the first encoder blocks
// by 14 % (DESIGN.md 8).  Activations and weights are therefore split x = hi + lo (two bf16 each, 16 mantissa bits) and
// every product is three MFMAs, hi.hi + lo.hi + hi.lo (the lo.lo term is below fp32 rounding): fp32-grade results at a
// third of the bf16 matrix rate, which is still 5 x the fp32 matrix pipe MIOpen's kernels use.
// Input: fp32 channels-last [clip][row][CINP] exactly as PyTorch lays out an (N, C, 1, L) channels_last tensor (a stride-s
// conv reads it as rows of s * Cin channels, see above); rows before 0 or past the clip read as zero (the conv's padding).
struct TArgs {
    const float* X; long x_clip_stride; long x_elems;      // floats per clip that exist; element index >= x_elems or < 0 reads 0
    int row0;                                               // input row (of CINP floats) under tap 0 of output position 0: -padding / stride
    int L_out;
    const uint4* Whi; const uint4* Wlo; const float* bias;  // packed [N/16][K/32] fragments of the hi / lo halves; bias[N] or null
    float* Y; long y_clip_stride;                           // fp32 [clip][L_out][N]
    int y_pitch, y_col0; long y_elems;                      // row pitch of Y in floats (0: N), first column of this launch's N-slice, floats per clip that exist (0: all)
    float* bn_part;                                         // null, or [workgroup][2][N]: per-channel sum and sum of squares of this workgroup's outputs
    int terms;                                              // bit 0: the W_lo . x_hi product, bit 1: the W_hi . x_lo product (3 = fp32-grade; set by the launcher)
    const float* in_aff;                                    // null, or [2][CINP]: the input is read as act(x * scale[c] + shift[c]) - the BatchNorm (+ LeakyReLU) of the
    int in_act;                                             // convolution in front, applied while the tile is staged (positions outside the clip stay zero: the padding)
    const float* X2; const uint4* Whi2; const uint4* Wlo2;  // null, or a second input / weight pair of the same geometry accumulated into the same output
    const float* R;                                         // null, or a tensor laid out like Y that is added to the result (k_conv_train only)
    const uint4* WhiB; const uint4* WloB; float* YB; float* bn_partB;   // DUAL instances: a second convolution of the same geometry on the SAME input tile (a
                                                            // down-sampling block's shortcut convolution beside its conv1: the tile is staged once), laid out like Y / bn_part
    long long* dbg;                                         // diagnostics (syn_debug_timing's first buffer): 8 cycle stamps per workgroup, or null
};

// Row padding of the training kernels' LDS tiles: 32 bytes.  A ds_read_b128 is served in four groups of 16 lanes over 64 banks; the
// fragment read (16 rows x 4 chunks of 16 B) is conflict-free when the row pitch is 32 B more than a multiple of 256 B - with the
// 16-byte padding of the eval-mode kernel every read took 8 LDS cycles instead of 4 (bank model: MI355X_MICROARCH.md, LDS).
constexpr int kTrainPad = 32;

// Staging of a training-mode input tile: ROWS rows of CINP fp32 channels -> two bf16 planes (hi, lo = x - hi) in LDS.  The
// global loads go out in batches of up to 6 per thread BEFORE anything waits for them (a loop of load -> wait -> convert ->
// ds_write paid one memory latency per 1 KB a wave fetched: 17-19 dependent round trips per tile, more than the tile's MFMA
// phase takes - the kernels were bound by it, DESIGN.md 4.4 r5b).  Element index of chunk c (four floats) = e_base + 4 c;
// indices < 0 or >= x_elems read as zero (the convolution's padding).  AFF (stride-1 layers, NTHR % (CINP / 4) == 0: a thread
// keeps its four channels for all its rows): the input is read as act(x * scale[c] + shift[c]).
template <int CINP, int ROWS, int NTHR, int PITCH, bool AFF>
__device__ __forceinline__ void stage_split_tile(const float* __restrict__ X, long e_base, long x_elems, const float* in_aff, int in_act,
                                                 char* smem, int tid) {
    constexpr int CQ = CINP / 4, TOT = ROWS * CQ, NIT = (TOT + NTHR - 1) / NTHR, NB = (NIT + 5) / 6, UB = (NIT + NB - 1) / NB, PLANE = ROWS * PITCH;
    f32x4 isc = {1.f, 1.f, 1.f, 1.f}, ish = {0.f, 0.f, 0.f, 0.f};
    bool aff = false;
    if constexpr (AFF) {
        static_assert(NTHR % CQ == 0, "a thread keeps its channels");
        if (in_aff) { aff = true; isc = *reinterpret_cast<const f32x4*>(in_aff + (tid % CQ) * 4); ish = *reinterpret_cast<const f32x4*>(in_aff + CINP + (tid % CQ) * 4); }
    }
#pragma unroll 1
    for (int b = 0; b < NB; ++b) {
        f32x4 v[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = tid + (b * UB + u) * NTHR;
            const long e = e_base + 4 * (long)c;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < TOT && e >= 0 && e + 3 < x_elems) v[u] = *reinterpret_cast<const f32x4*>(X + e);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = tid + (b * UB + u) * NTHR;
            if (c >= TOT) continue;
            const long e = e_base + 4 * (long)c;
            bool live[4] = {true, true, true, true};
            if (!(e >= 0 && e + 3 < x_elems)) {              // outside the clip, or (x_elems % 4 != 0) the clip's last, partial chunk
#pragma unroll
                for (int i = 0; i < 4; ++i) { live[i] = e + i >= 0 && e + i < x_elems; if (live[i]) v[u][i] = X[e + i]; }
            }
            if constexpr (AFF) {
                if (aff) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float t = fmaf(v[u][i], isc[i], ish[i]);
                        if (in_act) t = lrelu(t);
                        v[u][i] = live[i] ? t : 0.f;
                    }
                }
            }
            const int row = c / CQ, col = c - row * CQ;
            const bf16x4 h = to_bf16x4(v[u]);
            const f32x4 r = {v[u][0] - (float)h[0], v[u][1] - (float)h[1], v[u][2] - (float)h[2], v[u][3] - (float)h[3]};
            *reinterpret_cast<bf16x4*>(smem + row * PITCH + col * 8) = h;
            *reinterpret_cast<bf16x4*>(smem + PLANE + row * PITCH + col * 8) = to_bf16x4(r);
        }
    }
}

// Decomposition (r5b): a workgroup computes MW = WM x RF x 16 positions of NT = WN x NF x 16 output channels (grid z: the layer's channel
// blocks).  What bounds these kernels is the CU's L1 port, not the matrix pipe: every wave streams the weight fragments of ITS
// channels (hi + lo, NF KB each per k-step) L2 -> VGPR, and the port delivers ~42 B/clk in practice - with NF = 4 (64 channels per
// wave, the first version) the eight waves of a CU asked for 64 KB per k-step round = 1.5 k cycles beside 0.4 - 1.5 k cycles of
// MFMAs (profiles/r04_ab_conv_terms.txt: a third of the MFMAs bought 16 %).  Fewer channels and more positions per wave move
// that traffic to the LDS (input fragments, 256 B/clk): per wave and k-step NF x 2 KB of weights, RF x 2 KB of LDS reads,
// 3 x NF x RF MFMAs.
template <int CINP, int KT, int WN, int WM, int RF, int NF = 4, bool DUAL = false>
__global__ __launch_bounds__(WN * WM * 64, 2)                    // (two waves per SIMD: two 4-wave workgroups per CU, one staging while the other multiplies)
void k_conv_train(const TArgs a) {
    constexpr int KSB = CINP / 32, KS = KT * KSB, MW = WM * RF * 16, ROWS = MW + KT - 1, PITCH = CINP * 2 + kTrainPad;
    constexpr int NT = WN * NF * 16, PLANE = ROWS * PITCH, H = (NF + 1) / 2;
    static_assert((WN * WM == 8 || WN * WM == 4) && KS % 6 == 0, "4 or 8 waves; the k loop is unrolled by 6 (weight ring of 3, x_hi fragments of 2)");
    constexpr int NTHR = WN * WM * 64;
    constexpr bool XDB = RF <= 4;                            // the next step's x_hi fragments are read a step ahead (RF x 4 more registers)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, lr = lane & 15;
    const int wn = wave % WN, wm = wave / WN;
    const int clip = blockIdx.y, l0 = blockIdx.x * MW, zc = blockIdx.z * NT, n_all = gridDim.z * NT;
    long long* const dbg = a.dbg ? a.dbg + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 : nullptr;
    if (dbg && tid == 0) { dbg[0] = (long long)__builtin_readcyclecounter(); dbg[5] = (long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); }   // HW_ID
    constexpr int NC = DUAL ? 2 : 1;                         // DUAL: two convolutions (WhiB / WloB -> YB) over the one staged tile
    f32x4 accs[NC][NF][RF];
#pragma unroll
    for (int cv = 0; cv < NC; ++cv)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) accs[cv][nf][rf] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (X2: a second (input, weights) pair of the same geometry accumulated into the same tile - the data gradient of a down-sampling block's
    // input, conv1^T dy1 + shortcut^T dy_sc, written once instead of two tensors and an add)
    const int npass = a.X2 ? 2 : 1;
    // one pass: (input, weights) -> the accumulators `acc`; restage = false: the tile in LDS is this pass's input already (DUAL's second convolution)
    auto run_pass = [&](const float* Xp, const uint4* Whp, const uint4* Wlp, f32x4 (&acc)[NF][RF], const bool restage, const bool first) {
    const float* const X = Xp + (size_t)clip * a.x_clip_stride;
    const uint4* const Wh = Whp + ((size_t)(zc / 16 + wn * NF) * KS) * 64 + lane;
    const uint4* const Wl = Wlp + ((size_t)(zc / 16 + wn * NF) * KS) * 64 + lane;
    uint4 rh[3][NF], rl[3][NF];
    if (restage && !first) __syncthreads();                 // everybody is done with the first tile
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) { rh[p][nf] = Wh[((size_t)nf * KS + p) * 64]; rl[p][nf] = Wl[((size_t)nf * KS + p) * 64]; }
    // ---- stage the input tile as two bf16 planes (hi, lo): rows l0 + row0 .. + ROWS - 1 (batched loads: stage_split_tile) --
    // (the strided layers' 384-channel rows take no input affine: launcher-checked)
    if (restage) {
        stage_split_tile<CINP, ROWS, NTHR, PITCH, NTHR % (CINP / 4) == 0>(X, ((long)l0 + a.row0) * CINP, a.x_elems, a.in_aff, a.in_act, smem, tid);
        if (dbg && tid == 0 && first) dbg[1] = (long long)__builtin_readcyclecounter();
        __syncthreads();
        if (dbg && tid == 0 && first) dbg[2] = (long long)__builtin_readcyclecounter();
    }
    const char* xb = smem + (wm * RF * 16 + lr) * PITCH + 16 * g;
    int xoff = 0, cb = 0;
    // The k loop: the weight fragments of k-step ks + 2 and the input fragments are requested in two halves BETWEEN the three product
    // sweeps of a step instead of in one clump in front of them.
    bf16x8 xh[XDB ? 2 : 1][RF], xl[RF];
    if constexpr (XDB)
#pragma unroll
        for (int rf = 0; rf < RF; ++rf) xh[0][rf] = *reinterpret_cast<const bf16x8*>(xb + rf * 16 * PITCH);
#pragma unroll 1
    for (int ks0 = 0; ks0 < KS; ks0 += 6) {
#pragma unroll
        for (int u = 0; u < 6; ++u) {
            const int ks = ks0 + u, w = u % 3, wn2 = (u + 2) % 3, xc = XDB ? (u & 1) : 0, xn = XDB ? (xc ^ 1) : 0;
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 2 < KS)
#pragma unroll
                for (int nf = 0; nf < H; ++nf) {
                    rh[wn2][nf] = Wh[((size_t)nf * KS + ks + 2) * 64];
                    rl[wn2][nf] = Wl[((size_t)nf * KS + ks + 2) * 64];
                }
            if constexpr (!XDB)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) xh[0][rf] = *reinterpret_cast<const bf16x8*>(xb + rf * 16 * PITCH + xoff);
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) xl[rf] = *reinterpret_cast<const bf16x8*>(xb + PLANE + rf * 16 * PITCH + xoff);   // needed by the second sweep
            // small terms first; the three products of an accumulator are issued a whole (nf, rf) sweep apart, so that no MFMA waits
            // for the one before it
            if (a.terms & 1)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(__builtin_bit_cast(bf16x8, rl[w][nf]), xh[xc][rf], acc[nf][rf]);
            __builtin_amdgcn_sched_barrier(0);
            if (++cb == KSB) { cb = 0; xoff += PITCH - (KSB - 1) * 64; } else xoff += 64;   // next 32 channels / next tap: step ks + 1
            if (ks + 2 < KS)
#pragma unroll
                for (int nf = H; nf < NF; ++nf) {
                    rh[wn2][nf] = Wh[((size_t)nf * KS + ks + 2) * 64];
                    rl[wn2][nf] = Wl[((size_t)nf * KS + ks + 2) * 64];
                }
            if constexpr (XDB)
                if (ks + 1 < KS)
#pragma unroll
                    for (int rf = 0; rf < RF; ++rf) xh[xn][rf] = *reinterpret_cast<const bf16x8*>(xb + rf * 16 * PITCH + xoff);       // the next step's first sweep
            if (a.terms & 2)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(__builtin_bit_cast(bf16x8, rh[w][nf]), xl[rf], acc[nf][rf]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nf = 0; nf < NF; ++nf)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(__builtin_bit_cast(bf16x8, rh[w][nf]), xh[xc][rf], acc[nf][rf]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    };  // run_pass
    if constexpr (DUAL) {
        run_pass(a.X, a.Whi, a.Wlo, accs[0], true, true);
        run_pass(a.X, a.WhiB, a.WloB, accs[NC - 1], false, false);
    } else {
#pragma unroll 1
        for (int pass = 0; pass < npass; ++pass)
            run_pass(pass ? a.X2 : a.X, pass ? a.Whi2 : a.Whi, pass ? a.Wlo2 : a.Wlo, accs[0], true, pass == 0);
    }
    if (dbg && tid == 0) dbg[3] = (long long)__builtin_readcyclecounter();
#pragma unroll
    for (int cv = 0; cv < NC; ++cv) {
    f32x4 (&acc)[NF][RF] = accs[cv];
    float* const bn_part_cv = cv ? a.bn_partB : a.bn_part;
    float* const Y_cv = cv ? a.YB : a.Y;
    if (bn_part_cv) {
        // BatchNorm's batch statistics start here: the per-channel sum and sum of squares of this workgroup's tile, from the
        // accumulators (one pass over the 117 MB block-0 tensors fewer than a statistics kernel reading y back)
        f32x4 s[NF], q[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            s[nf] = q[nf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rf = 0; rf < RF; ++rf)
                if (l0 + (wm * RF + rf) * 16 + lr < a.L_out) { s[nf] = s[nf] + acc[nf][rf]; q[nf] = q[nf] + acc[nf][rf] * acc[nf][rf]; }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
#pragma unroll
                for (int e = 0; e < 4; ++e) { s[nf][e] += __shfl_xor(s[nf][e], off); q[nf][e] += __shfl_xor(q[nf][e], off); }
        }
        __syncthreads();                                     // the input tile is dead: the waves' sums meet in its place
        float* const red = reinterpret_cast<float*>(smem);   // [WM][2][NT]
        if (lr == 0)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                *reinterpret_cast<f32x4*>(red + (wm * 2 + 0) * NT + (wn * NF + nf) * 16 + 4 * g) = s[nf];
                *reinterpret_cast<f32x4*>(red + (wm * 2 + 1) * NT + (wn * NF + nf) * 16 + 4 * g) = q[nf];
            }
        __syncthreads();
        float* const out = bn_part_cv + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * n_all;   // [tile][2][all channels]
        for (int i = tid; i < 2 * NT; i += NTHR) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) t += red[w * 2 * NT + i];
            out[(i / NT) * n_all + zc + (i % NT)] = t;
        }
    }
#pragma unroll
    for (int rf = 0; rf < RF; ++rf) {
        const int m = l0 + (wm * RF + rf) * 16 + lr;
        if (m >= a.L_out) continue;
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            const int n = zc + (wn * NF + nf) * 16 + 4 * g;
            f32x4 v = acc[nf][rf];
            if (a.bias) v = v + *reinterpret_cast<const f32x4*>(a.bias + n);
            const long at = (long)m * (a.y_pitch ? a.y_pitch : n_all) + a.y_col0 + n;
            if (a.y_elems == 0 || at + 3 < a.y_elems) {
                if (a.R) v = v + *reinterpret_cast<const f32x4*>(a.R + (size_t)clip * a.y_clip_stride + at);
                *reinterpret_cast<f32x4*>(Y_cv + (size_t)clip * a.y_clip_stride + at) = v;
            }
        }
    }
    if (DUAL && cv == 0 && a.bn_partB) __syncthreads();    // (the statistics scratch of the first convolution is read before the second one's is written)
    }   // cv
    if (dbg && tid == 0) dbg[4] = (long long)__builtin_readcyclecounter();
}

// The same GEMM for the 64-output-channel strided layers (rows of 384 channels, 3 taps), with the four waves splitting K instead
// of the positions.  With k_conv_train<384, 3, 1, 4, 1> every wave streamed all 288 KB of weight fragments for its own 16
// positions - one fragment load per MFMA triple, the L1 port's limit - because a 64-position tile of two 384-channel planes is
// all the LDS holds.  Here a wave streams a quarter of K (72 KB) for all 64 positions (four MFMA triples per fragment pair), and the
// waves' partial accumulators are added in wave order through the LDS the input tile has left: run-to-run identical.
template <int CINP, int KT, int RF>
__global__ __launch_bounds__(256)
void k_conv_train_ks(const TArgs a) {
    static_assert(RF >= 1 && RF <= 4, "a wave finishes one row fragment");
    constexpr int KSB = CINP / 32, KS = KT * KSB, KQ = KS / 4, MW = RF * 16, ROWS = MW + KT - 1, PITCH = CINP * 2 + kTrainPad;
    constexpr int N = 64, PLANE = ROWS * PITCH, NTHR = 256;
    static_assert(KS % 4 == 0 && KQ % 3 == 0, "four K quarters; the weight ring is unrolled by 3");
    static_assert(4 * 4 * RF * 64 * 16 <= 2 * PLANE, "the partial accumulators reuse the input tile's LDS");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, lr = lane & 15;
    const int clip = blockIdx.y, l0 = blockIdx.x * MW;
    const float* const X = a.X + (size_t)clip * a.x_clip_stride;
    const int ks_first = wave * KQ;
    const uint4* const Wh = a.Whi + (size_t)ks_first * 64 + lane;
    const uint4* const Wl = a.Wlo + (size_t)ks_first * 64 + lane;
    uint4 rh[3][4], rl[3][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) { rh[p][nf] = Wh[((size_t)nf * KS + p) * 64]; rl[p][nf] = Wl[((size_t)nf * KS + p) * 64]; }
    stage_split_tile<CINP, ROWS, NTHR, PITCH, false>(X, ((long)l0 + a.row0) * CINP, a.x_elems, nullptr, 0, smem, tid);
    __syncthreads();
    f32x4 acc[4][RF];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* xb = smem + lr * PITCH + 16 * g;
    int cb = ks_first % KSB, xoff = (ks_first / KSB) * PITCH + cb * 64;
    for (int ks0 = 0; ks0 < KQ; ks0 += 3) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int ks = ks0 + u;
            if (ks + 2 < KQ)
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) {
                    rh[(u + 2) % 3][nf] = Wh[((size_t)nf * KS + ks + 2) * 64];
                    rl[(u + 2) % 3][nf] = Wl[((size_t)nf * KS + ks + 2) * 64];
                }
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 xh[RF], xl[RF];
#pragma unroll
            for (int rf = 0; rf < RF; ++rf) {
                xh[rf] = *reinterpret_cast<const bf16x8*>(xb + rf * 16 * PITCH + xoff);
                xl[rf] = *reinterpret_cast<const bf16x8*>(xb + PLANE + rf * 16 * PITCH + xoff);
            }
            if (a.terms & 1)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(__builtin_bit_cast(bf16x8, rl[u][nf]), xh[rf], acc[nf][rf]);
            if (a.terms & 2)
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(__builtin_bit_cast(bf16x8, rh[u][nf]), xl[rf], acc[nf][rf]);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int rf = 0; rf < RF; ++rf) acc[nf][rf] = MFMA16(__builtin_bit_cast(bf16x8, rh[u][nf]), xh[rf], acc[nf][rf]);
            __builtin_amdgcn_sched_barrier(0);
            if (++cb == KSB) { cb = 0; xoff += PITCH - (KSB - 1) * 64; } else xoff += 64;
        }
    }
    __syncthreads();                                         // the input tile is dead
    f32x4* const red = reinterpret_cast<f32x4*>(smem);        // [wave][nf][rf][lane]
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int rf = 0; rf < RF; ++rf) red[((wave * 4 + nf) * RF + rf) * 64 + lane] = acc[nf][rf];
    __syncthreads();
    // wave w finishes row fragment rf = w: the four partial sums in wave order, the statistics, the store
    const int rf = wave < RF ? wave : 0, m = wave < RF ? l0 + rf * 16 + lr : a.L_out;      // (RF < 4: the last waves have no fragment)
    f32x4 out[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
        out[nf] = red[((0 * 4 + nf) * RF + rf) * 64 + lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) out[nf] = out[nf] + red[((w * 4 + nf) * RF + rf) * 64 + lane];
    }
    if (a.bn_part) {
        __syncthreads();                                     // everybody has read the partial accumulators
        float* const st = reinterpret_cast<float*>(smem);     // [wave][2][N]
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = s;
            if (m < a.L_out) { s = out[nf]; q = out[nf] * out[nf]; }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1)
#pragma unroll
                for (int e = 0; e < 4; ++e) { s[e] += __shfl_xor(s[e], off); q[e] += __shfl_xor(q[e], off); }
            if (lr == 0) {
                *reinterpret_cast<f32x4*>(st + (wave * 2 + 0) * N + nf * 16 + 4 * g) = s;
                *reinterpret_cast<f32x4*>(st + (wave * 2 + 1) * N + nf * 16 + 4 * g) = q;
            }
        }
        __syncthreads();
        float* const o = a.bn_part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * N;
        for (int i = tid; i < 2 * N; i += NTHR) o[i] = (st[i] + st[2 * N + i]) + (st[4 * N + i] + st[6 * N + i]);
    }
    if (m < a.L_out)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = nf * 16 + 4 * g;
            f32x4 v = out[nf];
            if (a.bias) v = v + *reinterpret_cast<const f32x4*>(a.bias + n);
            const long at = (long)m * (a.y_pitch ? a.y_pitch : N) + a.y_col0 + n;
            if (a.y_elems == 0 || at + 3 < a.y_elems) *reinterpret_cast<f32x4*>(a.Y + (size_t)clip * a.y_clip_stride + at) = v;
        }
}

// ---- training-mode weight gradient of a stride-1 Conv1d(k = 15) ----------------------------------------------------------
// dW[co][t][c] = sum over clips and positions l of dy[l][co] * x[l + t - 7][c]: a GEMM whose contraction runs over POSITIONS,
// while both tensors are channels-last.  A workgroup takes one block of 16 input channels and a share of the position
// chunks (128 output positions each), transposes the chunk's dy tile and x rows into LDS on the way in (hi / lo bf16 planes,
// positions contiguous), and its 8 waves take two taps each: the B fragment of tap t is the x row shifted by t elements -
// read as five aligned dwords and funnelled by 16 bits when t is odd.  Three MFMAs per product as in the forward kernel.
// Partial sums per workgroup share go to `part` and are added up by k_conv_wgrad_sum (no atomics: run-to-run identical).
struct WArgs {
    const float* GY; long gy_clip_stride; int L_out;         // dy fp32 [clip][L_out][CO]
    const float* X; long x_clip_stride; long x_elems;        // x fp32 [clip][L_in][cin]
    int cin, n_clips, chunks_per_clip, shares;               // cin: channels of a row of X as the kernel sees it (stride * Cin for a strided conv)
    int co_n;                                                // output channels of the layer (row pitch of GY)
    int row0;                                                // X row under tap 0 of output position 0 (-7: stride-1 'same'; 0: strided, unpadded)
    float* part;                                             // [shares][CO][TAPS][cin]
    int terms;                                               // bit 0: the dy_lo . x_hi product, bit 1: the dy_hi . x_lo product (3 = fp32-grade; set by the launcher)
    long long* dbg;                                          // diagnostics (syn_debug_timing's first buffer), or null: per workgroup the cycles spent in the tile stores, in the k loop, in all
    const float* GY2;                                        // k_conv_wgrad_s<128, TAPS, true>: a SECOND convolution's dy (same geometry, same input: conv1 and the shortcut
                                                             // convolution of a down-sampling block) - the tile's rows 64 .. 127; both of co_n = 64 channels
    const float* in_aff; int in_act;                         // null, or [2][cin]: x is read as act(x * scale[c] + shift[c]) (stride-1 layers: the BatchNorm + LeakyReLU
                                                             // in front of conv2 recomputed from its input y1, the tensor z1 is never stored); rows outside the clip stay zero
};
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2w __attribute__((ext_vector_type(2)));
// LDS geometry (r5b, against the bank model of MI355X_MICROARCH.md: ds_write_b32 / ds_read_b32 32 banks in two groups of 32 lanes,
// ds_read_b128 64 banks in four groups of 16 lanes):
//  * a lane group lg of an MFMA takes the 32-position block lg of a chunk, the k loop steps 8 positions inside the blocks (position
//    32 lg + 8 kk + j instead of 32 kk + 8 lg + j - a sum over positions, any order): the tap-shifted dword reads of the x rows, 16
//    rows x 2 lane groups per LDS cycle, then fall on 32 different banks with the odd pitch (they were 2-way conflicted: lane groups
//    4 dwords apart collide for rows 12 apart whatever the pitch);
//  * the dy tile [co][position] has NO row padding (256 B) and its 16-byte columns are XOR-swizzled by the row,
//    column' = column ^ ((row >> 2) ^ (row << 2)) & 15: the transposed stores (16 channels x 4 positions per instruction) were 8-way
//    conflicted with the padded pitch and the fragment reads 2-way; both run at their nominal rate now (CO 128 / 256: stores 2-way).
constexpr int kWgP = 128, kWgAP = kWgP, kWgBP = kWgP + 26;
__device__ __forceinline__ int wg_a_swz(int row) { return ((row >> 2) ^ (row << 2)) & 15; }
// element (row, position p) of the dy tile, p even (a dword = positions p, p + 1)
__device__ __forceinline__ int wg_a_at(int row, int p) { return row * kWgAP + 8 * ((p >> 3) ^ wg_a_swz(row)) + (p & 7); }
static_assert(kWgBP % 2 == 0, "rows start on a dword");   // B pitch 77 dwords (odd): the tap-shifted dword reads of 16 rows hit 16 banks (76: 8 banks, 4-way conflicts on every read)
constexpr int wgrad_cb(int co) { return co >= 256 ? 1 : 256 / co; }     // channel blocks per workgroup
constexpr int wgrad_lds2(int co_t, int cb) { return (2 * co_t * kWgAP + 2 * 16 * cb * kWgBP) * 2; }
constexpr int wgrad_lds(int co) { return wgrad_lds2(co, wgrad_cb(co)); }

// TAPS = 15 (stride 1), or ceil(15 / stride) for a strided convolution read as a stride-1 one over rows of stride * Cin channels
// CB: blocks of 16 input channels per workgroup (CB x CO = 256: the accumulators of a wave's two taps fill half its registers) -
// the dy tile, the expensive one to stage (transposed, split), then serves CB x 16 channels.  CO is the TILE of output channels a
// workgroup owns (grid z walks the tiles of a layer with a.co_n channels): the 128- / 256-channel layers run as <64, 15, 2> - more slices
// of the gradient per position share = fewer shares = fewer full-size partial gradients through HBM (launch_wgrad_tiled)
template <int CO, int TAPS, int CB>
__global__ __launch_bounds__(512) void k_conv_wgrad(const WArgs a) {
    constexpr int TPW = (TAPS + 7) / 8;                      // taps per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* const Ah = reinterpret_cast<__bf16*>(smem);
    __bf16* const Al = Ah + CO * kWgAP;
    __bf16* const Bh = Al + CO * kWgAP;
    __bf16* const Bl = Bh + 16 * CB * kWgBP;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lg = lane >> 4, lr = lane & 15;
    const int cb0 = blockIdx.x * CB, share = blockIdx.y;
    const int co0 = blockIdx.z * CO;                         // CO = the tile of output channels this workgroup owns (grid z: tiles of a wider layer, a.co_n channels)
    f32x4 acc[TPW][CB][CO / 16];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int m = 0; m < CO / 16; ++m) acc[ti][b][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto split2 = [](float v0, float v1, unsigned& hi, unsigned& lo) {          // two values -> packed {hi0, hi1}, {lo0, lo1}
        const __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
        const __bf16 l0 = (__bf16)(v0 - (float)h0), l1 = (__bf16)(v1 - (float)h1);
        hi = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
        lo = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    };
    // staging, software-pipelined over the chunks: the global loads of chunk c + 1 are issued before the MFMA phase of chunk c and
    // sit in registers across it (a workgroup is alone on its CU: without this every chunk paid a full memory latency)
    constexpr int NA = (kWgP / 2) * (CO / 4), AI = NA / 512, NX = ((kWgP + 16) / 2) * 4 * CB, XI = (NX + 511) / 512;
    static_assert(NA % 512 == 0, "staging trip counts");
    f32x4 av[AI][2], xv[XI][2];
    auto load_tiles = [&](int c) {
        const int clip = c / a.chunks_per_clip, l0 = (c - clip * a.chunks_per_clip) * kWgP;
        const float* const gy = a.GY + (size_t)clip * a.gy_clip_stride;
        const float* const x = a.X + (size_t)clip * a.x_clip_stride;
#pragma unroll
        for (int it = 0; it < AI; ++it) {
            const int i = tid + 512 * it, pp = i / (CO / 4), c4 = i - pp * (CO / 4), l = l0 + 2 * pp;
            av[it][0] = av[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (l < a.L_out) av[it][0] = *reinterpret_cast<const f32x4*>(gy + (size_t)l * a.co_n + co0 + 4 * c4);
            if (l + 1 < a.L_out) av[it][1] = *reinterpret_cast<const f32x4*>(gy + (size_t)(l + 1) * a.co_n + co0 + 4 * c4);
        }
#pragma unroll
        for (int it = 0; it < XI; ++it) {
            const int i = tid + 512 * it, pp = i / (4 * CB), c4 = i - pp * (4 * CB);
            const long r0 = (long)l0 + a.row0 + 2 * pp;
            const long e0 = r0 * a.cin + 16 * cb0 + 4 * c4, e1 = e0 + a.cin;
            xv[it][0] = xv[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            const bool ok0 = i < NX && r0 >= 0 && e0 + 3 < a.x_elems, ok1 = i < NX && r0 + 1 >= 0 && e1 + 3 < a.x_elems;
            if (ok0) xv[it][0] = *reinterpret_cast<const f32x4*>(x + e0);
            if (ok1) xv[it][1] = *reinterpret_cast<const f32x4*>(x + e1);
            if (a.in_aff) {
                const f32x4 isc = *reinterpret_cast<const f32x4*>(a.in_aff + 16 * cb0 + 4 * c4), ish = *reinterpret_cast<const f32x4*>(a.in_aff + a.cin + 16 * cb0 + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v0 = fmaf(xv[it][0][e], isc[e], ish[e]), v1 = fmaf(xv[it][1][e], isc[e], ish[e]);
                    if (a.in_act) { v0 = lrelu(v0); v1 = lrelu(v1); }
                    xv[it][0][e] = ok0 ? v0 : 0.f; xv[it][1][e] = ok1 ? v1 : 0.f;
                }
            }
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int it = 0; it < AI; ++it) {                                       // dy tile, transposed: [co][position]
            const int i = tid + 512 * it, pp = i / (CO / 4), c4 = i - pp * (CO / 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned hi, lo;
                split2(av[it][0][e], av[it][1][e], hi, lo);
                // (= wg_a_at(4 c4 + e, 2 pp) in bytes: the row's swizzle is (c4 ^ 4 e) & 15, so e only flips bits 6-7 of the byte offset)
                const unsigned sa = ((unsigned)(1024 * c4 + 4 * (pp & 3)) | (16u * (((pp >> 2) ^ c4) & 15))) ^ (64u * e);
                *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(Ah) + sa + 256 * e) = hi;
                *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(Al) + sa + 256 * e) = lo;
            }
        }
#pragma unroll
        for (int it = 0; it < XI; ++it) {                                       // x rows l0 + row0 .. + P + 15 of these channel blocks
            const int i = tid + 512 * it, pp = i / (4 * CB), c4 = i - pp * (4 * CB);
            if (i < NX) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned hi, lo;
                    split2(xv[it][0][e], xv[it][1][e], hi, lo);
                    *reinterpret_cast<unsigned*>(Bh + (4 * c4 + e) * kWgBP + 2 * pp) = hi;
                    *reinterpret_cast<unsigned*>(Bl + (4 * c4 + e) * kWgBP + 2 * pp) = lo;
                }
            }
        }
    };
    const int total = a.n_clips * a.chunks_per_clip;
    long long t_store = 0, t_loop = 0, t_begin = a.dbg ? (long long)__builtin_readcyclecounter() : 0, t0 = 0;
    if (share < total) load_tiles(share);
    for (int c = share; c < total; c += a.shares) {
        __syncthreads();                                                         // everybody is done with the previous tiles
        if (a.dbg) t0 = (long long)__builtin_readcyclecounter();
        store_tiles();
        __syncthreads();
        if (a.dbg) { const long long t1 = (long long)__builtin_readcyclecounter(); t_store += t1 - t0; t0 = t1; }
        if (c + a.shares < total) load_tiles(c + a.shares);
#pragma unroll 1
        for (int kk = 0; kk < kWgP / 32; ++kk) {
            const unsigned la_k = (unsigned)(256 * lr + 16 * (((4 * lg) ^ wg_a_swz(lr)) & 15)) ^ (16u * kk);
            if constexpr (TPW == 2 && CO == 64) {
                // 64 output channels: the dy fragments of all four channel blocks stay in registers for the k step and the x rows are
                // STREAMED block by block, one block's ten dwords read ahead while the previous block's 16 - 24 MFMAs run (r5b: with all
                // of a step's 48 LDS reads in front of its 64 MFMAs a wave spent ~40 % of the loop waiting for the LDS)
                bf16x8 ahm[4], alm[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const unsigned a_at = (la_k ^ (64u * m)) + 4096u * m;
                    ahm[m] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Ah) + a_at);
                    alm[m] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Al) + a_at);
                }
                unsigned dh[2][5], dl[2][5];
                auto rd = [&](int b, int buf) {
                    const int base = (16 * b + lr) * kWgBP + 32 * lg + 8 * kk + 2 * wave;
                    const unsigned* ph = reinterpret_cast<const unsigned*>(Bh) + (base >> 1);
                    const unsigned* pl = reinterpret_cast<const unsigned*>(Bl) + (base >> 1);
#pragma unroll
                    for (int i = 0; i < 5; ++i) { dh[buf][i] = ph[i]; dl[buf][i] = pl[i]; }
                };
                rd(0, 0);
#pragma unroll
                for (int b = 0; b < CB; ++b) {
                    if (b + 1 < CB) rd(b + 1, (b + 1) & 1);
                    u32x4 f0h, f0l, f1h, f1l;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f0h[i] = dh[b & 1][i]; f0l[i] = dl[b & 1][i];
                        f1h[i] = __builtin_amdgcn_alignbit(dh[b & 1][i + 1], dh[b & 1][i], 16);
                        f1l[i] = __builtin_amdgcn_alignbit(dl[b & 1][i + 1], dl[b & 1][i], 16);
                    }
                    const bf16x8 bh0 = __builtin_bit_cast(bf16x8, f0h), bl0 = __builtin_bit_cast(bf16x8, f0l);
                    const bf16x8 bh1 = __builtin_bit_cast(bf16x8, f1h), bl1 = __builtin_bit_cast(bf16x8, f1l);
                    if (a.terms & 1)
#pragma unroll
                    for (int m = 0; m < 4; ++m) { acc[0][b][m] = MFMA16(alm[m], bh0, acc[0][b][m]); acc[1][b][m] = MFMA16(alm[m], bh1, acc[1][b][m]); }
                    if (a.terms & 2)
#pragma unroll
                    for (int m = 0; m < 4; ++m) { acc[0][b][m] = MFMA16(ahm[m], bl0, acc[0][b][m]); acc[1][b][m] = MFMA16(ahm[m], bl1, acc[1][b][m]); }
#pragma unroll
                    for (int m = 0; m < 4; ++m) { acc[0][b][m] = MFMA16(ahm[m], bh0, acc[0][b][m]); acc[1][b][m] = MFMA16(ahm[m], bh1, acc[1][b][m]); }
                }
                continue;
            }
            bf16x8 bh[TPW][CB], bl[TPW][CB];
            if constexpr (TPW == 2) {
                // a wave's two taps (2 wave, 2 wave + 1) come out of the same five dwords per plane: the even one as they are, the
                // odd one funnelled by 16 bits (the LDS pipe, shared by the 8 waves, is what this loop is bound by)
#pragma unroll
                for (int b = 0; b < CB; ++b) {
                    const int base = (16 * b + lr) * kWgBP + 32 * lg + 8 * kk + 2 * wave;   // even: kWgBP is
                    const unsigned* ph = reinterpret_cast<const unsigned*>(Bh) + (base >> 1);
                    const unsigned* pl = reinterpret_cast<const unsigned*>(Bl) + (base >> 1);
                    unsigned dh[5], dl[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) { dh[i] = ph[i]; dl[i] = pl[i]; }
                    u32x4 f0h, f0l, f1h, f1l;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f0h[i] = dh[i]; f0l[i] = dl[i];
                        f1h[i] = __builtin_amdgcn_alignbit(dh[i + 1], dh[i], 16);
                        f1l[i] = __builtin_amdgcn_alignbit(dl[i + 1], dl[i], 16);
                    }
                    bh[0][b] = __builtin_bit_cast(bf16x8, f0h); bl[0][b] = __builtin_bit_cast(bf16x8, f0l);
                    bh[1][b] = __builtin_bit_cast(bf16x8, f1h); bl[1][b] = __builtin_bit_cast(bf16x8, f1l);
                }
            } else
#pragma unroll
            for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
                for (int b = 0; b < CB; ++b) {
                    const int t = min(TPW * wave + ti, TAPS - 1);
                    const int base = (16 * b + lr) * kWgBP + 32 * lg + 8 * kk + t;   // first of this lane's 8 positions, shifted by the tap
                    const unsigned sh = (base & 1) * 16;
                    const unsigned* ph = reinterpret_cast<const unsigned*>(Bh) + (base >> 1);
                    const unsigned* pl = reinterpret_cast<const unsigned*>(Bl) + (base >> 1);
                    unsigned dh[5], dl[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) { dh[i] = ph[i]; dl[i] = pl[i]; }
                    u32x4 fh, fl;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        fh[i] = __builtin_amdgcn_alignbit(dh[i + 1], dh[i], sh);
                        fl[i] = __builtin_amdgcn_alignbit(dl[i + 1], dl[i], sh);
                    }
                    bh[ti][b] = __builtin_bit_cast(bf16x8, fh);
                    bl[ti][b] = __builtin_bit_cast(bf16x8, fl);
                }
#pragma unroll
            for (int m = 0; m < CO / 16; ++m) {
                // (= wg_a_at(16 m + lr, 32 lg + 8 kk) in bytes: one XOR with a constant on the lane's per-kk offset)
                const unsigned a_at = (la_k ^ (64u * (m & 3))) + 4096u * m;
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Ah) + a_at);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Al) + a_at);
                // (the three products of an accumulator a (tap, block) sweep apart)
                if (a.terms & 1)
#pragma unroll
                for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
                    for (int b = 0; b < CB; ++b) acc[ti][b][m] = MFMA16(al, bh[ti][b], acc[ti][b][m]);
                if (a.terms & 2)
#pragma unroll
                for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
                    for (int b = 0; b < CB; ++b) acc[ti][b][m] = MFMA16(ah, bl[ti][b], acc[ti][b][m]);
#pragma unroll
                for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
                    for (int b = 0; b < CB; ++b) acc[ti][b][m] = MFMA16(ah, bh[ti][b], acc[ti][b][m]);
            }
        }
        if (a.dbg) t_loop += (long long)__builtin_readcyclecounter() - t0;
    }
    if (a.dbg && tid == 0) {
        long long* const d = a.dbg + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8;
        d[0] = t_store; d[1] = t_loop; d[2] = (long long)__builtin_readcyclecounter() - t_begin; d[3] = (total - share + a.shares - 1) / a.shares;
    }
    // D[i = co][j = channel]: lane holds channel lr, rows 4 lg + r
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int t = TPW * wave + ti;
        if (t >= TAPS) continue;
#pragma unroll
        for (int b = 0; b < CB; ++b)
#pragma unroll
            for (int m = 0; m < CO / 16; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + 16 * m + 4 * lg + r;
                    a.part[(((size_t)share * a.co_n + co) * TAPS + t) * a.cin + 16 * (cb0 + b) + lr] = acc[ti][b][m][r];
                }
    }
}

// ---- weight gradient of the STRIDED convolutions ---------------------------------------------------------------------------
// Read as a stride-1 convolution over rows of stride * Cin = 384 channels with TAPS = ceil(15 / stride) = 3 / 5 taps, the GEMM
// has many channels and few taps: the decomposition above (waves = taps, workgroup = 16 channels) would leave most waves
// idle and re-stage the dy tile 24 times.  Here a workgroup takes 128 of the 384 row channels (grid x), a block of CO_T
// output channels (grid z) and a share of the position chunks (grid y); each of its 8 waves owns 16 row channels and keeps
// all TAPS x CO_T / 16 accumulator tiles.  Staging, split operands, tap shift by funnelled dwords and the deterministic
// partial sums are those of k_conv_wgrad.
constexpr int kWsJ = 128, kWsBP = kWgP + 26;                  // row channels per workgroup; B row pitch (77 dwords: odd)
constexpr int kWsRows = kWgP + 8;                            // x' rows staged per chunk (taps <= 5, + the funnel's look-ahead)
constexpr int wgrad_s_lds(int co_t) { return (2 * co_t * kWgAP + 2 * kWsJ * kWsBP) * 2; }

// DUAL (CO_T = 128): the tile's two halves are the dy of TWO convolutions over the same input (a.GY, a.GY2; 64 channels each) - conv1 and the shortcut convolution
// of block 1 stage their 117 MB input once instead of twice; part [share][128][TAPS][cin] holds both gradients (rows 0 - 63 / 64 - 127 of a share)
template <int CO_T, int TAPS, bool DUAL = false>
__global__ __launch_bounds__(512) void k_conv_wgrad_s(const WArgs a) {
    static_assert(TAPS <= 5, "x' rows staged per chunk");
    static_assert(!DUAL || CO_T == 128, "two 64-channel gradients per tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __bf16* const Ah = reinterpret_cast<__bf16*>(smem);
    __bf16* const Al = Ah + CO_T * kWgAP;
    __bf16* const Bh = Al + CO_T * kWgAP;
    __bf16* const Bl = Bh + kWsJ * kWsBP;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lg = lane >> 4, lr = lane & 15;
    const int jb = blockIdx.x, share = blockIdx.y, co0 = CO_T * blockIdx.z;
    f32x4 acc[TAPS][CO_T / 16];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int m = 0; m < CO_T / 16; ++m) acc[t][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto split2 = [](float v0, float v1, unsigned& hi, unsigned& lo) {
        const __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
        const __bf16 l0 = (__bf16)(v0 - (float)h0), l1 = (__bf16)(v1 - (float)h1);
        hi = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
        lo = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    };
    // staging as in k_conv_wgrad: loads first, conversion after; where the accumulators leave room (PRE), the loads of the next chunk
    // are issued before the MFMA phase of this one
    constexpr int NA = (kWgP / 2) * (CO_T / 4), AI = NA / 512, NX = (kWsRows / 2) * (kWsJ / 4), XI = (NX + 511) / 512;
    constexpr bool PRE = TAPS * (CO_T / 16) <= 24;
    static_assert(NA % 512 == 0, "staging trip counts");
    f32x4 av[AI][2], xv[XI][2];
    auto load_x = [&](int c) {
        const int clip = c / a.chunks_per_clip, l0 = (c - clip * a.chunks_per_clip) * kWgP;
        const float* const x = a.X + (size_t)clip * a.x_clip_stride;
#pragma unroll
        for (int it = 0; it < XI; ++it) {
            const int i = tid + 512 * it, pp = i / (kWsJ / 4), c4 = i - pp * (kWsJ / 4);
            const long r0 = (long)l0 + a.row0 + 2 * pp;
            const long e0 = r0 * a.cin + kWsJ * jb + 4 * c4, e1 = e0 + a.cin;
            xv[it][0] = xv[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < NX && r0 >= 0 && e0 + 3 < a.x_elems) xv[it][0] = *reinterpret_cast<const f32x4*>(x + e0);
            if (i < NX && r0 + 1 >= 0 && e1 + 3 < a.x_elems) xv[it][1] = *reinterpret_cast<const f32x4*>(x + e1);
        }
    };
    auto load_a = [&](int c) {
        const int clip = c / a.chunks_per_clip, l0 = (c - clip * a.chunks_per_clip) * kWgP;
        const float* const gy = a.GY + (size_t)clip * a.gy_clip_stride + co0;
        const float* const gy2 = DUAL ? a.GY2 + (size_t)clip * a.gy_clip_stride : nullptr;
#pragma unroll
        for (int it = 0; it < AI; ++it) {
            const int i = tid + 512 * it, pp = i / (CO_T / 4), c4 = i - pp * (CO_T / 4), l = l0 + 2 * pp;
            av[it][0] = av[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* const src = (DUAL && c4 >= 16) ? gy2 + 4 * (c4 - 16) : gy + 4 * c4;        // (DUAL: two tensors of pitch co_n = 64)
            if (l < a.L_out) av[it][0] = *reinterpret_cast<const f32x4*>(src + (size_t)l * a.co_n);
            if (l + 1 < a.L_out) av[it][1] = *reinterpret_cast<const f32x4*>(src + (size_t)(l + 1) * a.co_n);
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int it = 0; it < XI; ++it) {                                       // x' rows of this workgroup's 128 row channels, transposed
            const int i = tid + 512 * it, pp = i / (kWsJ / 4), c4 = i - pp * (kWsJ / 4);
            if (i < NX) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned hi, lo;
                    split2(xv[it][0][e], xv[it][1][e], hi, lo);
                    *reinterpret_cast<unsigned*>(Bh + (4 * c4 + e) * kWsBP + 2 * pp) = hi;
                    *reinterpret_cast<unsigned*>(Bl + (4 * c4 + e) * kWsBP + 2 * pp) = lo;
                }
            }
        }
    };
    auto store_a = [&]() {
#pragma unroll
        for (int it = 0; it < AI; ++it) {                                       // dy tile of this output-channel block, transposed
            const int i = tid + 512 * it, pp = i / (CO_T / 4), c4 = i - pp * (CO_T / 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned hi, lo;
                split2(av[it][0][e], av[it][1][e], hi, lo);
                // (= wg_a_at(4 c4 + e, 2 pp) in bytes: the row's swizzle is (c4 ^ 4 e) & 15, so e only flips bits 6-7 of the byte offset)
                const unsigned sa = ((unsigned)(1024 * c4 + 4 * (pp & 3)) | (16u * (((pp >> 2) ^ c4) & 15))) ^ (64u * e);
                *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(Ah) + sa + 256 * e) = hi;
                *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(Al) + sa + 256 * e) = lo;
            }
        }
    };
    const int total = a.n_clips * a.chunks_per_clip;
    long long t_store = 0, t_loop = 0, t_begin = a.dbg ? (long long)__builtin_readcyclecounter() : 0, t0 = 0;
    if (PRE && share < total) { load_x(share); load_a(share); }
    for (int c = share; c < total; c += a.shares) {
        __syncthreads();
        if (a.dbg) t0 = (long long)__builtin_readcyclecounter();
        if (PRE) { store_x(); store_a(); }
        else { load_x(c); store_x(); load_a(c); store_a(); }                     // (two rounds: the registers do not hold both tiles)
        __syncthreads();
        if (a.dbg) { const long long t1 = (long long)__builtin_readcyclecounter(); t_store += t1 - t0; t0 = t1; }
        if (PRE && c + a.shares < total) { load_x(c + a.shares); load_a(c + a.shares); }
#pragma unroll 1
        for (int kk = 0; kk < kWgP / 32; ++kk) {
            const unsigned la_k = (unsigned)(256 * lr + 16 * (((4 * lg) ^ wg_a_swz(lr)) & 15)) ^ (16u * kk);
            bf16x8 bh[TAPS], bl[TAPS];
            {
                // the TAPS tap-shifted fragments of a lane overlap: its 8 + TAPS - 1 positions are NDW consecutive dwords of the row (the first position is
                // even: the pitch and every term of `base` are), read ONCE per plane and funnelled per tap (r6: 10 dwords per tap and plane before - 30 / 50
                // ds_read_b32 per k step against 12 / 14 now; the loop is bound by the LDS pipe its 8 waves share)
                constexpr int NDW = ((TAPS - 1) >> 1) + 5;
                const int base = (16 * wave + lr) * kWsBP + 32 * lg + 8 * kk;
                const unsigned* ph = reinterpret_cast<const unsigned*>(Bh) + (base >> 1);
                const unsigned* pl = reinterpret_cast<const unsigned*>(Bl) + (base >> 1);
                unsigned dh[NDW], dl[NDW];
#pragma unroll
                for (int i = 0; i < NDW; ++i) { dh[i] = ph[i]; dl[i] = pl[i]; }
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    u32x4 fh, fl;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        fh[i] = __builtin_amdgcn_alignbit(dh[(t >> 1) + i + 1], dh[(t >> 1) + i], (t & 1) * 16);
                        fl[i] = __builtin_amdgcn_alignbit(dl[(t >> 1) + i + 1], dl[(t >> 1) + i], (t & 1) * 16);
                    }
                    bh[t] = __builtin_bit_cast(bf16x8, fh);
                    bl[t] = __builtin_bit_cast(bf16x8, fl);
                }
            }
#pragma unroll
            for (int m = 0; m < CO_T / 16; ++m) {
                // (= wg_a_at(16 m + lr, 32 lg + 8 kk) in bytes: one XOR with a constant on the lane's per-kk offset)
                const unsigned a_at = (la_k ^ (64u * (m & 3))) + 4096u * m;
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Ah) + a_at);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Al) + a_at);
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    if (a.terms & 1) acc[t][m] = MFMA16(al, bh[t], acc[t][m]);
                    if (a.terms & 2) acc[t][m] = MFMA16(ah, bl[t], acc[t][m]);
                    acc[t][m] = MFMA16(ah, bh[t], acc[t][m]);
                }
            }
        }
        if (a.dbg) t_loop += (long long)__builtin_readcyclecounter() - t0;
    }
    const long long t_epi = a.dbg ? (long long)__builtin_readcyclecounter() : 0;
    // D[i = co][j = row channel]: lane holds row channel lr of its wave's 16, output channels 4 lg + r
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int m = 0; m < CO_T / 16; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 16 * m + 4 * lg + r;
                a.part[(((size_t)share * (DUAL ? CO_T : a.co_n) + co) * TAPS + t) * a.cin + kWsJ * jb + 16 * wave + lr] = acc[t][m][r];
            }
    if (a.dbg && tid == 0) {                                                     // diagnostics (syn_debug_timing): cycles in the tile stores, the k loops, in all, chunks, before the epilogue
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        long long* const d = a.dbg + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8;
        d[0] = t_store; d[1] = t_loop; d[2] = (long long)__builtin_readcyclecounter() - t_begin; d[3] = (total - share + a.shares - 1) / a.shares; d[4] = t_epi - t_begin;
    }
}

// dW[co][ci][t] (the module's weight layout) = sum over the shares of part[share][co][j][r * cin + ci], t = j * stride + r.
// The partial sums are the traffic (up to 63 MB, read once).  A workgroup takes 32 quads of consecutive elements; its 8 lane-groups of 32 take
// the shares g, g + 8, g + 16, ... (a lane-group reads 512 contiguous bytes of a share), and the 8 sub-sums meet in LDS in group order: a fixed
// order, run-to-run identical.  (r5b: one thread per quad over ALL shares was 60 workgroups of 256 dependent loads for the 64-channel layers -
// 15-20 us for what the memory system moves in 3.)  The 4-byte scatter into the module's layout happens once per output.
constexpr int kWsumGroups = 8;
__global__ __launch_bounds__(256) void k_conv_wgrad_sum(const float* __restrict__ part, int shares, int co_n, int cin, int stride, int taps, float* __restrict__ dw) {
    __shared__ f32x4 red[kWsumGroups][32];
    const int cinp = stride * cin, per = co_n * taps * cinp;
    const int e = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int s4 = (blockIdx.x * 32 + e) * 4;                                      // over (co, j, r * cin + ci), four consecutive ci
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s4 < per)
#pragma unroll 4
        for (int g = grp; g < shares; g += kWsumGroups) acc = acc + *reinterpret_cast<const f32x4*>(part + (size_t)g * per + s4);
    red[grp][e] = acc;
    __syncthreads();
    if (grp != 0 || s4 >= per) return;
#pragma unroll
    for (int g = 1; g < kWsumGroups; ++g) acc = acc + red[g][e];
    const int c = s4 % cinp, j = (s4 / cinp) % taps, co = s4 / (cinp * taps);
    const int r = c / cin, ci = c - r * cin, t = j * stride + r;
    if (t < 15)
#pragma unroll
        for (int q = 0; q < 4; ++q) dw[((size_t)co * cin + ci + q) * 15 + t] = acc[q];
}

// ---- training mode, the encoder's FIRST layer: Conv1d(1 | 2 -> 64, k 15, stride 5, padding 1700) ------------------------------
// (block 0's conv1 and its shortcut convolution, models/denoiser.py:308 / models/utils/layer.py:150,158).  15 x cin <= 30
// products per output: not a matrix problem but a streaming one - the output (and, backward, dy) is the largest tensor of the
// encoder (1.9 MB per clip) - so plain fp32 FMAs: exact fp32, no operand split.  A thread owns one output channel; the window
// of the waveform a tile needs sits in LDS and is read as broadcasts.
struct FArgs {
    const float* X; int L_in; int n_clips;                    // waveform fp32 [clip][L_in][CIN]
    const float* W;                                           // module layout [64][CIN][15]
    float* Y; const float* DY; int L_out;                     // [clip][L_out][64]
    int stride, pad;
    float* part; int chunks_per_clip;                         // weight gradient: partial sums [clip * chunks_per_clip][64][CIN * 15]
    // weight gradient with the BatchNorm + LeakyReLU backward of THIS convolution's output folded in (k_conv_first_wgrad5): DY is then dz, the
    // gradient at the activation's output, BY the convolution's raw output y; dy = scale (dp - dbeta / M - xhat dgamma / M), dp = dz act'(a(y)),
    // is formed as the values are loaded - the tensor dy is never written (nor read back)
    const float* BY; const float* bn_stats; const float* bn_aff; const float* bn_dgb; float bn_inv_rows; int bn_act;
    // forward of two convolutions over the same window (block 0's conv1 and its shortcut convolution): second weight / output / statistics
    const float* W2; float* Y2; float* part2;
    // weight gradient of block 0's SHORTCUT convolution with the block tail's backward folded in (k_conv_first_wgrad_m, T_y2 != null): DY is dout, the
    // gradient at the block's output; BY the shortcut convolution's raw output with bn_stats / bn_aff / bn_dgb of ITS BatchNorm; T_y2 conv2's raw output
    // with t_stats / t_aff / t_dgb of bn2.  With p = a2(y2) + a_s(y_s), d = dout act'(p): the shortcut's dy_s = BatchNorm backward of d (never written: it
    // feeds the matrix pipe), and dy2 = bn2's backward of d is WRITTEN to T_dy2 - the apply pass of syn_bn_block_bwd and the tensor dy_s are gone
    const float* T_y2; const float* t_stats; const float* t_aff; const float* t_dgb; float* T_dy2;
};
constexpr int kF1Tile = 256;                                 // output positions per workgroup (forward): 4 x fewer partial sums for the BatchNorm finalize than 64
constexpr int kF1Chunk = 1024;                               // output positions per workgroup (weight gradient)

template <int CIN>
__global__ __launch_bounds__(256) void k_conv_first_fwd(const FArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const win = reinterpret_cast<float*>(smem);       // [(kF1Tile - 1) * stride + 15][CIN]
    const int tid = threadIdx.x, co = tid & 63, pg = tid >> 6, clip = blockIdx.y, l0 = blockIdx.x * kF1Tile;
    const int rows = (kF1Tile - 1) * a.stride + 15;
    const long p0 = (long)l0 * a.stride - a.pad;
    const float* const x = a.X + (size_t)clip * a.L_in * CIN;
    for (int i = tid; i < rows * CIN; i += 256) {
        const long p = p0 + i / CIN;
        win[i] = (p >= 0 && p < a.L_in) ? x[p * CIN + (i % CIN)] : 0.f;
    }
    float w[CIN][15];
#pragma unroll
    for (int c = 0; c < CIN; ++c)
#pragma unroll
        for (int t = 0; t < 15; ++t) w[c][t] = a.W[(co * CIN + c) * 15 + t];
    __syncthreads();
    float* const y = a.Y + (size_t)clip * a.L_out * 64;
    float bs = 0.f, bq = 0.f;
    for (int i = pg; i < kF1Tile; i += 4) {
        const int l = l0 + i;
        if (l >= a.L_out) break;
        const float* const r = win + i * a.stride * CIN;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 15; ++t)
#pragma unroll
            for (int c = 0; c < CIN; ++c) acc = fmaf(w[c][t], r[t * CIN + c], acc);
        y[(size_t)l * 64 + co] = acc;
        bs += acc; bq = fmaf(acc, acc, bq);
    }
    if (a.part) {
        // BatchNorm's batch statistics start here (as in k_conv_train): per-channel sum and sum of squares of this workgroup's tile,
        // the four position groups added in a fixed order -> part[workgroup][2][64]
        __syncthreads();                                      // the window is dead
        float* const red = win;                               // [4][2][64]
        red[(pg * 2 + 0) * 64 + co] = bs; red[(pg * 2 + 1) * 64 + co] = bq;
        __syncthreads();
        if (tid < 128)
            a.part[((size_t)clip * gridDim.x + blockIdx.x) * 128 + tid] = (red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid]);
    }
}


// The first layer's weight gradient as a persistent stream on the fp32 matrix pipe (r5b).  dW[co][k] = sum over positions of dy[pos][co] * window[pos][k],
// where the k = tap * CIN + c <= 30 window values of a position are CONTIGUOUS in the waveform (x[(pos * stride - pad) * CIN + k]).  v_mfma_f32_32x32x2_f32 takes
// one A and one B value per lane: A[m = co][kk = position] = lane (co = l % 32, position p + l / 32) - consecutive lanes read consecutive channels of a position,
// coalesced, no transposition of dy anywhere - and B[kk = position][n = k] = lane (k = l % 32, the same position): a coalesced read of the waveform itself, no LDS
// window.  Two MFMAs (channels 0-31 / 32-63) per two positions; exact fp32 products and accumulation like the FMA kernels above.  The BatchNorm + LeakyReLU
// backward of the convolution's output folds into the loaded value (a lane's channel is fixed: its constants sit in registers).
// What the FMA kernels lacked was not arithmetic but a stream: a workgroup per 1024 positions staged a window, reduced eight waves through LDS and wrote 7.7 KB of
// partial sums for 0.25 - 0.5 MB of input - 2.6 TB/s where a grid-stride read of the same tensors runs at 6.5 (scripts/ubench/hbm_width.hip).  Here every wave
// walks position pairs across the whole batch with kF1mAhead steps of loads in flight and keeps its 64 x 32 partial gradient in registers until the end.
typedef float f32x16w __attribute__((ext_vector_type(16)));
constexpr int kF1mWaves = 4, kF1mAhead = 8, kF1mAheadTail = 5;
// TAIL: the block tail's backward folded in (FArgs::T_y2 ...): an instance of its own - three tensors per position instead of two and a store want their
// own register budget (as one kernel the plain calls fell from four waves per SIMD to three: the grid's fourth workgroup per CU then runs in a second round)
template <int CIN, bool TAIL = false>
__global__ __launch_bounds__(kF1mWaves * 64) void k_conv_first_wgrad_m(const FArgs a) {
    constexpr int KK = CIN * 15, NW = kF1mWaves, D = TAIL ? kF1mAheadTail : kF1mAhead;
    __shared__ float red[NW][64][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, half = lane >> 5;
    float sc[2] = {0.f, 0.f}, sh[2] = {0.f, 0.f}, mu[2] = {0.f, 0.f}, rs[2] = {0.f, 0.f}, dgm[2] = {0.f, 0.f}, dbm[2] = {0.f, 0.f};
    float sc2[2] = {0.f, 0.f}, sh2[2] = {0.f, 0.f}, mu2[2] = {0.f, 0.f}, rs2[2] = {0.f, 0.f}, dgm2[2] = {0.f, 0.f};
    constexpr bool tail = TAIL;
    if (a.BY)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int co = ln + 32 * h;
            mu[h] = a.bn_stats[co]; rs[h] = a.bn_stats[64 + co]; sc[h] = a.bn_aff[co]; sh[h] = a.bn_aff[64 + co];
            dgm[h] = a.bn_dgb[co] * a.bn_inv_rows; dbm[h] = a.bn_dgb[64 + co] * a.bn_inv_rows;
            if (tail) {
                mu2[h] = a.t_stats[co]; rs2[h] = a.t_stats[64 + co]; sc2[h] = a.t_aff[co]; sh2[h] = a.t_aff[64 + co];
                dgm2[h] = a.t_dgb[co] * a.bn_inv_rows;                     // (dbeta is the same sum for both BatchNorms: sum of d)
            }
        }
    f32x16w acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    // work item q = a pair of positions (2 pp, 2 pp + 1) of one clip; wave w of workgroup b takes q = b NW + w, then strides by the grid's waves
    const int ppc = (a.L_out + 1) / 2;                         // pairs per clip
    const long n_items = (long)a.n_clips * ppc, stride_q = (long)gridDim.x * NW;
    const long q0 = (long)blockIdx.x * NW + wave;
    const int n_steps = q0 < n_items ? (int)((n_items - q0 + stride_q - 1) / stride_q) : 0;
    float gd[D][2], gy[D][2], g2[TAIL ? D : 1][2], gb[D];
    unsigned gat[TAIL ? D : 1];                              // (element offset of the slot's values: the launcher keeps n_clips x L_out x 64 below 2^32 for a TAIL launch)
    bool live[D];
    auto fetch = [&](int j, int slot) {
        const long q = q0 + (long)j * stride_q;
        const int clip = (int)(q / ppc), pos = 2 * (int)(q - (long)clip * ppc) + half;
        const bool ok = pos < a.L_out;
        live[slot] = ok;
        const size_t at = ((size_t)clip * a.L_out + pos) * 64 + ln;
        if constexpr (TAIL) gat[slot] = (unsigned)at;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            gd[slot][h] = ok ? a.DY[at + 32 * h] : 0.f;
            gy[slot][h] = (a.BY && ok) ? a.BY[at + 32 * h] : 0.f;
            if constexpr (TAIL) g2[slot][h] = ok ? a.T_y2[at + 32 * h] : 0.f;
        }
        const long e = ((long)pos * a.stride - a.pad) * CIN + ln;             // element of the clip's waveform under (position, k = ln)
        gb[slot] = (ok && ln < KK && e >= 0 && e < (long)a.L_in * CIN) ? a.X[(size_t)clip * a.L_in * CIN + e] : 0.f;
    };
#pragma unroll
    for (int j = 0; j < D - 1; ++j) if (j < n_steps) fetch(j, j);
    for (int j0 = 0; j0 < n_steps; j0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int j = j0 + u;
            if (j >= n_steps) break;
            if (j + D - 1 < n_steps) fetch(j + D - 1, (u + D - 1) % D);
            float d[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float v = gd[u][h];
                if constexpr (TAIL) {
                    const float yv = gy[u][h], y2v = g2[u][h];
                    if (a.bn_act && fmaf(y2v, sc2[h], sh2[h]) + fmaf(yv, sc[h], sh[h]) <= 0.f) v *= 0.01f;
                    if (live[u]) a.T_dy2[(size_t)gat[u] + 32 * h] = sc2[h] * (v - dbm[h] - (y2v - mu2[h]) * rs2[h] * dgm2[h]);
                    v = sc[h] * (v - dbm[h] - (yv - mu[h]) * rs[h] * dgm[h]);
                    if (!live[u]) v = 0.f;
                } else if (a.BY) {
                    const float yv = gy[u][h];
                    if (a.bn_act && fmaf(yv, sc[h], sh[h]) <= 0.f) v *= 0.01f;
                    v = sc[h] * (v - dbm[h] - (yv - mu[h]) * rs[h] * dgm[h]);
                    if (!live[u]) v = 0.f;
                }
                d[h] = v;
            }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d[0], gb[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d[1], gb[u], acc1, 0, 0, 0);
        }
    }
    // the waves' partial gradients meet in LDS in wave order (run-to-run identical); the workgroups' partial sums are added by k_conv_first_wsum
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int co = 8 * (i >> 2) + 4 * half + (i & 3);      // D[row = channel][column = k]: lane holds column ln, rows 8 (i / 4) + 4 half + i % 4
        red[wave][co][ln] = acc0[i];
        red[wave][32 + co][ln] = acc1[i];
    }
    __syncthreads();
    float* const out = a.part + (size_t)blockIdx.x * 64 * KK;
    for (int i = tid; i < 64 * KK; i += NW * 64) {
        const int co = i / KK, n = i - co * KK, t = n / CIN, c = n - t * CIN;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += red[w][co][n];
        out[co * KK + c * 15 + t] = v;
    }
}

// conv1 of block 0 (r6, last session): its weight gradient AND the backward statistics of bn1 in ONE pass over (dz, y).  The BatchNorm backward
//   dy = scale (dp - dbeta / M - xhat dgamma / M),  dp = dz act'(a(y)),  dbeta = sum dp,  dgamma = sum dp xhat
// is linear in the two sums, and nothing but a REDUCTION consumes dy here (the waveform takes no gradient):
//   dW[co][k] = sum_pos dy win = scale (S1 - dbeta / M S2 - dgamma / M S3),  S1[co][k] = sum dp win,  S2[k] = sum win,  S3[co][k] = sum xhat win.
// So the statistics pass (k_bn_bwd_stats: 234 MB read, 51 us) and its finalize launch go: this kernel accumulates S1 and S3 on the fp32 matrix pipe (four MFMAs per
// position pair instead of two - the kernel is bound by HBM), S2 / dbeta / dgamma in lane registers, and k_conv_first_wgrad_lin_fin combines the workgroups' partial
// sums (in double) into dW and [dgamma | dbeta | 0].  Partial sums of a workgroup: [S1: 64 KK][S3: 64 KK][S2: 32][dbeta: 64][dgamma: 64] floats.
constexpr int kF1lAhead = 6;
constexpr int first_lin_part(int cin) { return 2 * 64 * cin * 15 + 32 + 128; }
template <int CIN>
__global__ __launch_bounds__(kF1mWaves * 64) void k_conv_first_wgrad_lin(const FArgs a) {
    constexpr int KK = CIN * 15, NW = kF1mWaves, D = kF1lAhead;
    __shared__ float red[NW][64][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), ln = lane & 31, half = lane >> 5;
    float sc[2], sh[2], mu[2], rs[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int co = ln + 32 * h;
        mu[h] = a.bn_stats[co]; rs[h] = a.bn_stats[64 + co]; sc[h] = a.bn_aff[co]; sh[h] = a.bn_aff[64 + co];
    }
    f32x16w acc[4];                                            // S1 (channels 0-31, 32-63), S3 (likewise)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    float s2 = 0.f, dbl[2] = {0.f, 0.f}, dgl[2] = {0.f, 0.f};
    const int ppc = (a.L_out + 1) / 2;
    const long n_items = (long)a.n_clips * ppc, stride_q = (long)gridDim.x * NW;
    const long q0 = (long)blockIdx.x * NW + wave;
    const int n_steps = q0 < n_items ? (int)((n_items - q0 + stride_q - 1) / stride_q) : 0;
    float gd[D][2], gy[D][2], gb[D];
    bool live[D];
    auto fetch = [&](int j, int slot) {
        const long q = q0 + (long)j * stride_q;
        const int clip = (int)(q / ppc), pos = 2 * (int)(q - (long)clip * ppc) + half;
        const bool ok = pos < a.L_out;
        live[slot] = ok;
        const size_t at = ((size_t)clip * a.L_out + pos) * 64 + ln;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            gd[slot][h] = ok ? a.DY[at + 32 * h] : 0.f;
            gy[slot][h] = ok ? a.BY[at + 32 * h] : 0.f;
        }
        const long e = ((long)pos * a.stride - a.pad) * CIN + ln;
        gb[slot] = (ok && ln < KK && e >= 0 && e < (long)a.L_in * CIN) ? a.X[(size_t)clip * a.L_in * CIN + e] : 0.f;
    };
#pragma unroll
    for (int j = 0; j < D - 1; ++j) if (j < n_steps) fetch(j, j);
    for (int j0 = 0; j0 < n_steps; j0 += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int j = j0 + u;
            if (j >= n_steps) break;
            if (j + D - 1 < n_steps) fetch(j + D - 1, (u + D - 1) % D);
            float dp[2], xh[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float yv = gy[u][h];
                float v = gd[u][h];
                if (a.bn_act && fmaf(yv, sc[h], sh[h]) <= 0.f) v *= 0.01f;
                dp[h] = live[u] ? v : 0.f;
                xh[h] = live[u] ? (yv - mu[h]) * rs[h] : 0.f;
                dbl[h] += dp[h]; dgl[h] = fmaf(dp[h], xh[h], dgl[h]);
            }
            s2 += gb[u];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[0], gb[u], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[1], gb[u], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(xh[0], gb[u], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(xh[1], gb[u], acc[3], 0, 0, 0);
        }
    }
    float* const out = a.part + (size_t)blockIdx.x * first_lin_part(CIN);
    // S1, then S3: the waves' partial matrices meet in LDS in wave order, [co][k = t CIN + c] as the finalize reads them
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        if (which) __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = 8 * (i >> 2) + 4 * half + (i & 3);
            red[wave][co][ln] = acc[2 * which][i];
            red[wave][32 + co][ln] = acc[2 * which + 1][i];
        }
        __syncthreads();
        for (int i = tid; i < 64 * KK; i += NW * 64) {
            const int co = i / KK, k = i - co * KK;
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) v += red[w][co][k];
            out[which * 64 * KK + i] = v;
        }
    }
    __syncthreads();
    // S2 [k = ln], dbeta / dgamma [co = ln + 32 h]: the two position halves of a lane pair, then the waves in order
    float* const r1 = &red[0][0][0];                           // [wave][5][32]
    r1[(wave * 5 + 0) * 32 + ln] = s2 + __shfl_xor(s2, 32);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float b = dbl[h] + __shfl_xor(dbl[h], 32), g = dgl[h] + __shfl_xor(dgl[h], 32);
        if (half == 0) { r1[(wave * 5 + 1 + h) * 32 + ln] = b; r1[(wave * 5 + 3 + h) * 32 + ln] = g; }
    }
    __syncthreads();
    if (tid < 160) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += r1[w * 160 + tid];
        out[2 * 64 * KK + tid] = v;                            // [S2: 32][dbeta: 64][dgamma: 64]
    }
}

// dW (module layout) and [dgamma | dbeta | 0] from k_conv_first_wgrad_lin's partial sums: one workgroup per output channel, everything summed in part order in double
template <int CIN>
__global__ __launch_bounds__(1024) void k_conv_first_wgrad_lin_fin(const float* __restrict__ part, int n_part, const float* __restrict__ aff, float inv_rows,
                                                                    float* __restrict__ dw, float* __restrict__ dgb) {
    constexpr int KK = CIN * 15, PER = first_lin_part(CIN), SL = 32;
    __shared__ double red[SL][32][3];
    __shared__ double rb[1024], rg[1024];
    const int co = blockIdx.x, tid = threadIdx.x, k = tid & 31, sl = tid >> 5;
    // dbeta, dgamma of this channel
    double b = 0.0, g = 0.0;
    for (int p = tid; p < n_part; p += 1024) { const float* q = part + (size_t)p * PER + 2 * 64 * KK + 32; b += q[co]; g += q[64 + co]; }
    rb[tid] = b; rg[tid] = g;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (k < KK)
#pragma unroll 4
        for (int p = sl; p < n_part; p += SL) {
            const float* q = part + (size_t)p * PER;
            s1 += q[co * KK + k]; s3 += q[64 * KK + co * KK + k]; s2 += q[2 * 64 * KK + k];
        }
    red[sl][k][0] = s1; red[sl][k][1] = s2; red[sl][k][2] = s3;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) { if (tid < o) { rb[tid] += rb[tid + o]; rg[tid] += rg[tid + o]; } __syncthreads(); }
    const double sdb = rb[0], sdg = rg[0];
    if (tid < KK) {
        double t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
        for (int gi = 0; gi < SL; ++gi) { t1 += red[gi][tid][0]; t2 += red[gi][tid][1]; t3 += red[gi][tid][2]; }
        const int t = tid / CIN, c = tid - t * CIN;
        dw[(co * CIN + c) * 15 + t] = (float)((double)aff[co] * (t1 - sdb * (double)inv_rows * t2 - sdg * (double)inv_rows * t3));
    }
    if (tid == 0) { dgb[co] = (float)sdg; dgb[64 + co] = (float)sdb; dgb[128 + co] = 0.f; }
}

// Forward of TWO first-layer convolutions over the same waveform window - block 0's conv1 and its shortcut convolution (models/utils/layer.py:150,158:
// same input, kernel, stride and padding) - in one launch: a window value read from the LDS feeds both, the window is staged once.  Statistics of both
// outputs as in k_conv_first_fwd.
template <int CIN>
__global__ __launch_bounds__(256) void k_conv_first_fwd2(const FArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const win = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, co = tid & 63, pg = tid >> 6, clip = blockIdx.y, l0 = blockIdx.x * kF1Tile;
    const int rows = (kF1Tile - 1) * a.stride + 15;
    const long p0 = (long)l0 * a.stride - a.pad;
    const float* const x = a.X + (size_t)clip * a.L_in * CIN;
    for (int i = tid; i < rows * CIN; i += 256) {
        const long p = p0 + i / CIN;
        win[i] = (p >= 0 && p < a.L_in) ? x[p * CIN + (i % CIN)] : 0.f;
    }
    float w[CIN][15], w2[CIN][15];
#pragma unroll
    for (int c = 0; c < CIN; ++c)
#pragma unroll
        for (int t = 0; t < 15; ++t) { w[c][t] = a.W[(co * CIN + c) * 15 + t]; w2[c][t] = a.W2[(co * CIN + c) * 15 + t]; }
    __syncthreads();
    float* const y = a.Y + (size_t)clip * a.L_out * 64;
    float* const y2 = a.Y2 + (size_t)clip * a.L_out * 64;
    float bs = 0.f, bq = 0.f, bs2 = 0.f, bq2 = 0.f;
    for (int i = pg; i < kF1Tile; i += 4) {
        const int l = l0 + i;
        if (l >= a.L_out) break;
        const float* const r = win + i * a.stride * CIN;
        float acc = 0.f, acc2 = 0.f;
#pragma unroll
        for (int t = 0; t < 15; ++t)
#pragma unroll
            for (int c = 0; c < CIN; ++c) { const float v = r[t * CIN + c]; acc = fmaf(w[c][t], v, acc); acc2 = fmaf(w2[c][t], v, acc2); }
        y[(size_t)l * 64 + co] = acc;
        y2[(size_t)l * 64 + co] = acc2;
        bs += acc; bq = fmaf(acc, acc, bq); bs2 += acc2; bq2 = fmaf(acc2, acc2, bq2);
    }
    if (a.part) {
        __syncthreads();
        float* const red = win;                               // [2 convolutions][4][2][64]
        red[(pg * 2 + 0) * 64 + co] = bs; red[(pg * 2 + 1) * 64 + co] = bq;
        red[512 + (pg * 2 + 0) * 64 + co] = bs2; red[512 + (pg * 2 + 1) * 64 + co] = bq2;
        __syncthreads();
        const size_t at = ((size_t)clip * gridDim.x + blockIdx.x) * 128;
        if (tid < 128) a.part[at + tid] = (red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid]);
        else a.part2[at + tid - 128] = (red[512 + tid - 128] + red[640 + tid - 128]) + (red[768 + tid - 128] + red[896 + tid - 128]);
    }
}

// dw[i] = sum over the parts, in part order within 16 interleaved groups and then over the groups: fixed order, run-to-run identical
__global__ __launch_bounds__(1024) void k_conv_first_wsum(const float* __restrict__ part, int n_part, int n, float* __restrict__ dw) {
    __shared__ float red[16][64];
    const int o = threadIdx.x & 63, g = threadIdx.x >> 6, idx = blockIdx.x * 64 + o;
    float s = 0.f;
    if (idx < n)
#pragma unroll 4
        for (int p = g; p < n_part; p += 16) s += part[(size_t)p * n + idx];
    red[g][o] = s;
    __syncthreads();
    if (g == 0 && idx < n) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) v += red[k][o];
        dw[idx] = v;
    }
}

// The partial-sum reductions of up to four weight gradients in ONE launch (the three convolutions of a BasicBlock: as launches of their own they were
// 14 + 2 launches of 6 - 15 us per step, most of them too small to reach the memory rate).  kind 0: k_conv_wgrad_sum's reduction + scatter into the
// module's layout; kind 1: the first layer's plain sum over its workgroups' partial gradients (k_conv_first_wsum's job; here 8 lane-groups of 32
// quads instead of 16 x 64 scalars - the same fixed order every run).
constexpr int kWsumJobs = 4;
struct WSumJob { const float* part; float* dw; int shares, co_n, cin, stride, taps, kind, first_block, per, pitch; };   // pitch: elements between the shares (per, or more: a share that holds two gradients)
struct WSumJobs { WSumJob j[kWsumJobs]; int n; };
__global__ __launch_bounds__(256) void k_conv_wgrad_sums(const WSumJobs a) {
    __shared__ f32x4 red[kWsumGroups][32];
    int k = a.n - 1;
    while (k > 0 && (int)blockIdx.x < a.j[k].first_block) --k;
    const WSumJob J = a.j[k];
    const int lb = (int)blockIdx.x - J.first_block;
    const int e = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int s4 = (lb * 32 + e) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s4 < J.per)
#pragma unroll 4
        for (int g = grp; g < J.shares; g += kWsumGroups) acc = acc + *reinterpret_cast<const f32x4*>(J.part + (size_t)g * J.pitch + s4);
    red[grp][e] = acc;
    __syncthreads();
    if (grp != 0 || s4 >= J.per) return;
#pragma unroll
    for (int g = 1; g < kWsumGroups; ++g) acc = acc + red[g][e];
    if (J.kind == 1) { *reinterpret_cast<f32x4*>(J.dw + s4) = acc; return; }
    const int cinp = J.stride * J.cin;
    const int c = s4 % cinp, j = (s4 / cinp) % J.taps, co = s4 / (cinp * J.taps);
    const int r = c / J.cin, ci = c - r * J.cin, t = j * J.stride + r;
    if (t < 15)
#pragma unroll
        for (int q = 0; q < 4; ++q) J.dw[((size_t)co * J.cin + ci + q) * 15 + t] = acc[q];
}

}  // namespace wav

// ---- WavEncoder forward: lengths, workspace layout and the 12 launches ----------------------------------------
struct WavPlan {
    int L1, L2, L3, L4;                 // positions after blocks 0, 1(=2), 3(=4), 5
    long z0, s0, x1, z1, s1, x2, z2, x3, z3, s3, x4, z4, x5, z5, s5, per_clip;   // element (bf16) offsets inside a clip's workspace
};
constexpr int kHalo = 7, kSlack = 16;   // zero rows in front of / behind padded tensors; zero tail rows of the grouped ones
WavPlan wav_plan(int L) {
    WavPlan p;
    p.L1 = (L + 2 * 1700 - 15) / 5 + 1;
    p.L2 = (p.L1 - 15) / 6 + 1;
    p.L3 = (p.L2 - 15) / 6 + 1;
    p.L4 = (p.L3 - 15) / 3 + 1;
    long o = 0;
    auto take = [&](long rows, int ch) { const long at = o; o += rows * ch; o = (o + 63) & ~63L; return at; };
    const long h2 = p.L2 + 2 * kHalo + kSlack, h3 = p.L3 + 2 * kHalo + kSlack, h4 = p.L4 + 2 * kHalo + kSlack;
    p.z0 = p.s0 = 0;      /* block 0's intermediates never leave the chip (k_block0) */  p.x1 = take(p.L1 + kSlack, 64);
    p.z1 = take(h2, 64);  p.s1 = take(p.L2, 64);  p.x2 = take(h2, 64);
    p.z2 = take(h2, 64);  p.x3 = take(p.L2 + kSlack, 64);
    p.z3 = take(h3, 128); p.s3 = take(p.L3, 128); p.x4 = take(h3, 128);
    p.z4 = take(h3, 128); p.x5 = take(p.L3 + kSlack, 128);
    p.z5 = take(h4, 256); p.s5 = take(p.L4, 256);
    p.per_clip = o;
    return p;
}

template <int CINP, int KT, int WN, int WM, int RF, int EPI>
int launch_conv(const wav::CArgs& a, int n_clips, hipStream_t s) {
    constexpr int MW = WM * RF * 16, lds = (MW + KT - 1) * (CINP * 2 + 16);
    static OncePerDevice once;
    if (once.first()) { allow_lds(wav::k_conv<CINP, KT, WN, WM, RF, EPI>, lds); }
    hipLaunchKernelGGL((wav::k_conv<CINP, KT, WN, WM, RF, EPI>), dim3((a.L_out + MW - 1) / MW, n_clips), dim3(WN * WM * 64), lds, s, a);
    return launched("k_conv launch");
}

}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int32_t syn_wav_out_frames(int32_t n_samples) { return n_samples >= 15 ? wav_plan(n_samples).L4 : 0; }

int64_t syn_wav_workspace_bytes(int32_t n_clips, int32_t n_samples) {
    if (n_clips <= 0 || n_samples < 15) return 0;
    return (int64_t)wav_plan(n_samples).per_clip * n_clips * 2;
}

// Where syn_wav_encode keeps what inside a clip's workspace (host only, no launch): the WavPlan it runs from, word for word.
int syn_wav_layout(int32_t n_samples, int64_t* out) {
    if (!out) return fail_msg("syn_wav_layout: null argument");
    if (n_samples < 15) return fail_msg("syn_wav_layout: clip too short");
    const WavPlan p = wav_plan(n_samples);
    const int64_t words[] = {p.L1, p.L2, p.L3, p.L4, p.per_clip, p.x1, p.z1, p.s1, p.x2, p.z2, p.x3, p.z3, p.s3, p.x4, p.z4, p.x5, p.z5, p.s5, kHalo, kSlack};
    static_assert(sizeof(words) == SYN_WAV_LAYOUT_WORDS * sizeof(int64_t), "include/syn_hip.h: SYN_WAV_LAYOUT_WORDS");
    memcpy(out, words, sizeof(words));
    return 0;
}

int syn_wav_encode(const syn_wavenc* enc, const float* wav_in, int32_t n_clips, int32_t n_samples, void* workspace, float* out,
                   void* stream) {
    if (!enc || !wav_in || !workspace || !out || n_clips <= 0) return fail_msg("syn_wav_encode: null argument");
    if (enc->cin != 1 && enc->cin != 2) return fail_msg("syn_wav_encode: 1 or 2 input channels");
    const WavPlan p = wav_plan(n_samples);
    if (p.L4 <= 0) return fail_msg("syn_wav_encode: clip too short");
    hipStream_t s = (hipStream_t)stream;
    __bf16* const ws = (__bf16*)workspace;
    const long cs = p.per_clip;
    int rc;
    {   // block 0 in one kernel: conv1 recomputed into the LDS tile, shortcut as the accumulators' initial value
        static OncePerDevice once;
        if (once.first()) { allow_lds(wav::k_block0, wav::kB0Lds); }
        wav::B0Args b;
        b.wav = wav_in; b.wav_clip_stride = (long)n_samples * enc->cin; b.L = n_samples; b.cin = enc->cin; b.L1 = p.L1;
        b.w_first = enc->w_first; b.W2 = (const uint4*)enc->conv[0].w; b.bias2 = enc->conv[0].bias;
        b.X1 = ws + p.x1; b.x1_clip_stride = cs;
        hipLaunchKernelGGL(wav::k_block0, dim3((p.L1 + wav::kB0Tile - 1) / wav::kB0Tile, n_clips), dim3(wav::kB0Waves * 64), wav::kB0Lds, s, b);
    }
    auto base = [&](int i) {
        wav::CArgs a;
        memset(&a, 0, sizeof(a));
        a.W = (const uint4*)enc->conv[i].w; a.bias = enc->conv[i].bias;
        a.x_clip_stride = a.z_clip_stride = a.s_clip_stride = a.r_clip_stride = cs;
        return a;
    };
    wav::CArgs a;
    // block 1: conv1 | shortcut (stride 6 = 3 taps over 6-row groups), conv2 -> x2 (halo: block 2 pads by 7)
    a = base(1); a.X = ws + p.x1; a.x_rows = (p.L1 + 5) / 6; a.L_out = p.L2; a.Z = ws + p.z1; a.z_off = kHalo * 64; a.S = ws + p.s1;
    if ((rc = launch_conv<384, 3, 2, 2, 2, wav::E_C1SC>(a, n_clips, s))) return rc;
    a = base(2); a.X = ws + p.z1; a.x_rows = p.L2 + 2 * kHalo; a.L_out = p.L2; a.Z = ws + p.x2; a.z_off = kHalo * 64; a.R = ws + p.s1;
    if ((rc = launch_conv<64, 15, 1, 4, 4, wav::E_C2>(a, n_clips, s))) return rc;
    // block 2 (identity shortcut): conv1, conv2 + x2 -> x3
    a = base(3); a.X = ws + p.x2; a.x_rows = p.L2 + 2 * kHalo; a.L_out = p.L2; a.Z = ws + p.z2; a.z_off = kHalo * 64;
    if ((rc = launch_conv<64, 15, 1, 4, 4, wav::E_C1>(a, n_clips, s))) return rc;
    a = base(4); a.X = ws + p.z2; a.x_rows = p.L2 + 2 * kHalo; a.L_out = p.L2; a.Z = ws + p.x3; a.R = ws + p.x2; a.r_off = kHalo * 64;
    if ((rc = launch_conv<64, 15, 1, 4, 4, wav::E_C2>(a, n_clips, s))) return rc;
    // block 3: 64 -> 128, stride 6
    a = base(5); a.X = ws + p.x3; a.x_rows = (p.L2 + 5) / 6; a.L_out = p.L3; a.Z = ws + p.z3; a.z_off = kHalo * 128; a.S = ws + p.s3;
    if ((rc = launch_conv<384, 3, 4, 1, 4, wav::E_C1SC>(a, n_clips, s))) return rc;
    a = base(6); a.X = ws + p.z3; a.x_rows = p.L3 + 2 * kHalo; a.L_out = p.L3; a.Z = ws + p.x4; a.z_off = kHalo * 128; a.R = ws + p.s3;
    if ((rc = launch_conv<128, 15, 2, 2, 4, wav::E_C2>(a, n_clips, s))) return rc;
    // block 4 (identity shortcut)
    a = base(7); a.X = ws + p.x4; a.x_rows = p.L3 + 2 * kHalo; a.L_out = p.L3; a.Z = ws + p.z4; a.z_off = kHalo * 128;
    if ((rc = launch_conv<128, 15, 2, 2, 4, wav::E_C1>(a, n_clips, s))) return rc;
    a = base(8); a.X = ws + p.z4; a.x_rows = p.L3 + 2 * kHalo; a.L_out = p.L3; a.Z = ws + p.x5; a.R = ws + p.x4; a.r_off = kHalo * 128;
    if ((rc = launch_conv<128, 15, 2, 2, 4, wav::E_C2>(a, n_clips, s))) return rc;
    // block 5: 128 -> 256, stride 3 (5 taps over 3-row groups); conv2 writes the fp32 result
    a = base(9); a.X = ws + p.x5; a.x_rows = (p.L3 + 2) / 3; a.L_out = p.L4; a.Z = ws + p.z5; a.z_off = kHalo * 256; a.S = ws + p.s5;
    if ((rc = launch_conv<384, 5, 8, 1, 4, wav::E_C1SC>(a, n_clips, s))) return rc;
    a = base(10); a.X = ws + p.z5; a.x_rows = p.L4 + 2 * kHalo; a.L_out = p.L4; a.R = ws + p.s5; a.Yf = out; a.yf_clip_stride = (long)p.L4 * 256;
    if ((rc = launch_conv<256, 15, 4, 1, 4, wav::E_C2>(a, n_clips, s))) return rc;
    return launched("syn_wav_encode");
}

}  // extern "C"
