// The T2M text-motion co-embedding evaluator (utils/t2m_eval_tools.py:332-351, 564-639): MovementConvEncoder, MotionEncoderBiGRUCo and
// TextEncoderBiGRUCo in eval mode, fp32 (DESIGN.md §13).  Everything is fp32 operands on v_mfma_f32_16x16x4_f32 (exact fp32 products,
// fp32 accumulation): the co-embeddings feed a ranking (R-precision), and the split-bf16 scheme of syn_tmr.inc is not accurate enough.
//
// k_t2m_gemm  C = epi(A' W^T + b): one family for every non-recurrent product.  A' is a plain row-major matrix, the stride-2 four-tap
//             window of a Conv1d(k4, s2, p1) (implicit GEMM, k = tap * cin + c, zero rows outside the take) or LeakyReLU(LayerNorm(row)).
//             64 x 128 tile per workgroup of 4 waves; A staged through the LDS 64 columns of K at a time, W read as packed fragments.
// k_t2m_gru   the recurrence.  A workgroup owns 16 sequences and one direction for all their steps: h lives in the LDS as fp32, each of
//             the 8 waves owns H / 8 hidden units for all three gates (r, z, n and h' of a unit meet in one lane), W_hh streams from the
//             packed copy every step.  Sequences are independent: no inter-workgroup traffic, two workgroup barriers per step.
// Every output row is a k-ordered fma chain that does not depend on which rows share its tile: bitwise reproducible, and a sequence's
// embedding does not depend on its batch.
namespace {
namespace t2m {

constexpr int kBM = 64, kBN = 128, kKC = 64, kLdA = kKC + 4;       // row stride = 4 mod 64 words: the 16 x 4 float4 A reads spread over the banks
constexpr int kRows = 16;                                         // sequences per recurrent workgroup (the MFMA's M)
constexpr int kGruWaves = 8;
constexpr float kSlope = 0.2f, kLnEps = 1e-5f;

enum { A_PLAIN = 0, A_CONV = 1, A_LN = 2 };
enum { E_BIAS = 0, E_LEAKY = 1, E_ADD = 2 };

static inline long round_up(long v, long m) { return (v + m - 1) / m * m; }
static inline int conv_len(int t) { return (t - 2) / 2 + 1; }      // Conv1d(k4, s2, p1)
static inline long packed_floats(int n, int k) { return round_up(n, kBN) / 16 * round_up(k, 16) / 16 * 256; }

struct GemmArgs {
    const float* a; long lda; int m, k, n;
    int cin, t_in, t_out;                       // A_CONV: row = (sequence, output frame); a [seq][t_in][lda], cin channels used
    const float* ln_g; const float* ln_b;       // A_LN: k <= 1024
    const float* w; const float* bias; int kq;  // packed fragments, kq = ceil(k / 16)
    int epi; const float* res; long ldr;        // E_ADD: + res[row][col]
    float* c; long ldc;
};

template <int AMODE>
__global__ __launch_bounds__(256) void k_t2m_gemm(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float s_a[kBM * kLdA];
    __shared__ long s_off[kBM];                 // A_CONV: offset of the row's window frame 0 (2 j - 1) in a; A_PLAIN / A_LN: of the row
    __shared__ int s_f0[kBM];                   // A_CONV: 2 j - 1, or t_in for rows past m (every tap fails the bounds test)
    __shared__ float s_mean[kBM], s_rstd[kBM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long r0 = (long)blockIdx.x * kBM;
    if (tid < kBM) {
        const long row = r0 + tid;
        if (AMODE == A_CONV) {
            const long seq = row / g.t_out;
            const int j = (int)(row - seq * g.t_out);
            s_f0[tid] = row < g.m ? 2 * j - 1 : g.t_in;
            s_off[tid] = row < g.m ? (seq * g.t_in + (2 * j - 1)) * g.lda : 0;
        } else {
            s_f0[tid] = row < g.m ? 0 : 1;
            s_off[tid] = row < g.m ? row * g.lda : 0;
        }
    }
    __syncthreads();
    if (AMODE == A_LN) {                        // per row: mean, then the variance about it (two passes), as LayerNorm
        for (int i = 0; i < kBM / 4; ++i) {
            const int r = wave * (kBM / 4) + i;
            const float* p = g.a + s_off[r];
            float s = 0.f;
            if (s_f0[r] == 0)
                for (int k = lane; k < g.k; k += 64) s += p[k];
            for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
            const float mean = s / (float)g.k;
            float q = 0.f;
            if (s_f0[r] == 0)
                for (int k = lane; k < g.k; k += 64) { const float d = p[k] - mean; q += d * d; }
            for (int o = 32; o; o >>= 1) q += __shfl_xor(q, o);
            if (lane == 0) { s_mean[r] = mean; s_rstd[r] = 1.f / sqrtf(q / (float)g.k + kLnEps); }
        }
        __syncthreads();
    }
    const int nt0 = (blockIdx.y * 4 + wave) * 2;               // this wave's two 16-column tiles
    const f32x4* w0 = reinterpret_cast<const f32x4*>(g.w) + (long)nt0 * g.kq * 64 + lane;
    const f32x4* w1 = w0 + (long)g.kq * 64;
    f32x4 acc[2][4];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[c][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kk = tid & 63, rb = tid >> 6;                    // staging: this thread's column of the K block, rows rb + 4 i
    const int kend = g.kq * 16;
    for (int k0 = 0; k0 < kend; k0 += kKC) {
        const int k = k0 + kk;
        int tap = 0, c = k;
        if (AMODE == A_CONV) { tap = k / g.cin; c = k - tap * g.cin; }
        float lg = 0.f, lb = 0.f;
        if (AMODE == A_LN && k < g.k) { lg = g.ln_g[k]; lb = g.ln_b[k]; }
#pragma unroll 4
        for (int i = 0; i < kBM / 4; ++i) {
            const int r = rb + 4 * i;
            float v = 0.f;
            if (k < g.k) {
                if (AMODE == A_CONV) {
                    const int f = s_f0[r] + tap;
                    if (f >= 0 && f < g.t_in) v = g.a[s_off[r] + (long)tap * g.lda + c];
                } else if (s_f0[r] == 0) {
                    v = g.a[s_off[r] + k];
                    if (AMODE == A_LN) {
                        v = (v - s_mean[r]) * s_rstd[r] * lg + lb;
                        v = v > 0.f ? v : kSlope * v;
                    }
                }
            }
            s_a[r * kLdA + kk] = v;
        }
        __syncthreads();
        const int nq = min(kKC / 16, g.kq - k0 / 16);
        for (int q = 0; q < nq; ++q) {
            const f32x4 b0 = w0[(long)(k0 / 16 + q) * 64], b1 = w1[(long)(k0 / 16 + q) * 64];
            f32x4 av[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) av[r] = *reinterpret_cast<const f32x4*>(&s_a[(r * 16 + (lane & 15)) * kLdA + 16 * q + 4 * (lane >> 4)]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc[0][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][j], b0[j], acc[0][r], 0, 0, 0);
                    acc[1][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][j], b1[j], acc[1][r], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    // D: row (l >> 4) * 4 + e, column l & 15
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int col = (nt0 + ct) * 16 + (lane & 15);
        if (col >= g.n) continue;
        const float bias = g.bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long row = r0 + r * 16 + (lane >> 4) * 4 + e;
                if (row >= g.m) continue;
                float v = acc[ct][r][e] + bias;
                if (g.epi == E_ADD) v += g.res[row * g.ldr + col];
                if (g.epi == E_LEAKY) v = v > 0.f ? v : kSlope * v;
                g.c[row * g.ldc + col] = v;
            }
    }
}

struct GruArgs {
    const float* gx;            // W_ih x + b_ih of every step: [n_seq][max_len][2][3 H] (direction, then gates r | z | n)
    const float* whh[2];        // packed fragments per direction
    const float* bhh;           // [2][3 H]
    const float* hidden;        // [2][H]
    const int32_t* lengths; const int32_t* order;
    int n_seq, max_len;
    float* hcat;                // [n_seq][2 H]: final state, forward | reverse
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

template <int H>
__global__ __launch_bounds__(64 * kGruWaves) void k_t2m_gru(const GruArgs g) {
    constexpr int UPW = H / kGruWaves, TPW = UPW / 16, NCT = 3 * TPW, KQ = H / 16, LD = H + 4;
    extern __shared__ __attribute__((aligned(16))) float s_h[];            // [kRows][LD]
    __shared__ int s_seq[kRows], s_len[kRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, dir = blockIdx.y;
    if (tid < kRows) {
        const int slot = blockIdx.x * kRows + tid;
        int seq = -1, len = 0;
        if (slot < g.n_seq) {
            seq = g.order[slot];
            if (seq < 0 || seq >= g.n_seq) seq = -1;
            else len = min(max(g.lengths[seq], 0), g.max_len);
        }
        s_seq[tid] = seq;
        s_len[tid] = len;
    }
    for (int e = tid; e < kRows * H; e += 64 * kGruWaves) s_h[(e / H) * LD + (e % H)] = g.hidden[dir * H + (e % H)];
    __syncthreads();
    int steps = 0;
#pragma unroll
    for (int i = 0; i < kRows; ++i) steps = max(steps, s_len[i]);
    // wave w streams its fragments in consumption order: [q][gate * TPW + tile][lane] float4
    const f32x4* wp = reinterpret_cast<const f32x4*>(g.whh[dir]) + (long)wave * KQ * NCT * 64 + lane;
    const float* bhh = g.bhh + dir * 3 * H;
    const float* ap = &s_h[(lane & 15) * LD + 4 * (lane >> 4)];
    for (int s = 0; s < steps; ++s) {
        f32x4 acc[NCT];
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < KQ; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 16 * q);
            f32x4 b[NCT];
#pragma unroll
            for (int c = 0; c < NCT; ++c) b[c] = wp[((long)q * NCT + c) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < NCT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[c][j], acc[c], 0, 0, 0);
        }
        __syncthreads();                                       // every wave has read this step's h
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = (lane >> 4) * 4 + e;
            const int len = s_len[row];
            if (s >= len) continue;                            // a finished (or absent) row keeps its state
            const int t = dir ? len - 1 - s : s;
            const float* gx = g.gx + (((long)s_seq[row] * g.max_len + t) * 2 + dir) * 3 * H;
#pragma unroll
            for (int tl = 0; tl < TPW; ++tl) {
                const int u = wave * UPW + tl * 16 + (lane & 15);
                const float r = sigmoidf_(gx[u] + (acc[tl][e] + bhh[u]));
                const float z = sigmoidf_(gx[H + u] + (acc[TPW + tl][e] + bhh[H + u]));
                const float n = tanhf(gx[2 * H + u] + r * (acc[2 * TPW + tl][e] + bhh[2 * H + u]));
                const float h = s_h[row * LD + u];
                s_h[row * LD + u] = n + z * (h - n);
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < kRows * H; e += 64 * kGruWaves) {
        const int row = e / H, u = e % H;
        if (s_seq[row] >= 0) g.hcat[(long)s_seq[row] * 2 * H + dir * H + u] = s_h[row * LD + u];
    }
}

// w [n][k] (Linear) or [n][conv_cin][4] (Conv1d, k = tap * conv_cin + c) -> float4 fragments: element j of lane l of fragment (tile, q) is
// B[k = 16 q + 4 (l >> 4) + j][column 16 tile + (l & 15)], zero outside n x k.
// layout 0 (GEMM): fragment index tile * kq + q, tiles 0 .. roundup(n, 128) / 16.
// layout H (recurrent, n = 3 H, k = H): wave w of 8 owns units w H/8 ..; index (w * kq + q) * NCT + gate * TPW + tile-in-wave.
__global__ __launch_bounds__(256) void k_t2m_pack(const float* __restrict__ w, int n, int k, int conv_cin, int layout, long frags, int kq,
                                                  float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;       // one float4 per thread
    if (i >= frags * 64) return;
    const int lane = (int)(i & 63);
    const long f = i >> 6;
    int q, col;
    if (layout == 0) {
        q = (int)(f % kq);
        col = (int)(f / kq) * 16 + (lane & 15);
    } else {
        const int h = layout, upw = h / kGruWaves, tpw = upw / 16, nct = 3 * tpw;
        const int c = (int)(f % nct);
        q = (int)(f / nct % kq);
        const int wv = (int)(f / nct / kq);
        col = (c / tpw) * h + wv * upw + (c % tpw) * 16 + (lane & 15);
    }
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kk = 16 * q + 4 * (lane >> 4) + j;
        float x = 0.f;
        if (col < n && kk < k) {
            if (conv_cin > 0) { const int tap = kk / conv_cin, c = kk - tap * conv_cin; x = w[((long)col * conv_cin + c) * 4 + tap]; }
            else x = w[(long)col * k + kk];
        }
        v[j] = x;
    }
    reinterpret_cast<f32x4*>(out)[i] = v;
}

static int gemm(hipStream_t st, int amode, GemmArgs g) {
    g.kq = (int)(round_up(g.k, 16) / 16);
    const dim3 grid((unsigned)((g.m + kBM - 1) / kBM), (unsigned)(round_up(g.n, kBN) / kBN));
    if (amode == A_CONV)     hipLaunchKernelGGL(k_t2m_gemm<A_CONV>, grid, dim3(256), 0, st, g);
    else if (amode == A_LN)  hipLaunchKernelGGL(k_t2m_gemm<A_LN>, grid, dim3(256), 0, st, g);
    else                     hipLaunchKernelGGL(k_t2m_gemm<A_PLAIN>, grid, dim3(256), 0, st, g);
    return launched("k_t2m_gemm launch");
}

static int linear(hipStream_t st, const float* a, long lda, long m, int k, int n, const float* w, const float* bias, int epi, float* c, long ldc,
                  const float* res = nullptr, long ldr = 0) {
    GemmArgs g = {};
    g.a = a; g.lda = lda; g.m = (int)m; g.k = k; g.n = n; g.w = w; g.bias = bias; g.epi = epi; g.res = res; g.ldr = ldr; g.c = c; g.ldc = ldc;
    return gemm(st, A_PLAIN, g);
}

static bool gru_ok(const syn_t2m_gru& r) { return r.w_ih && r.b_ih && r.w_hh[0] && r.w_hh[1] && r.b_hh && r.hidden; }
static bool head_ok(const syn_t2m_head& h) { return h.w1 && h.b1 && h.ln_g && h.ln_b && h.w2 && h.b2; }

struct Carve {
    char* p;
    float* take(long floats) { float* r = (float*)p; p += round_up(floats * 4, 256); return r; }
};

// gx -> final states -> Linear, LayerNorm + LeakyReLU (applied by the last GEMM's A load), Linear
template <int H>
static int recur_and_head(hipStream_t st, const syn_t2m_gru& r, const syn_t2m_head& hd, const float* gx, int n_seq, int max_len,
                          const int32_t* lengths, const int32_t* order, float* hcat, float* y1, float* out) {
    GruArgs a = {};
    a.gx = gx; a.whh[0] = r.w_hh[0]; a.whh[1] = r.w_hh[1]; a.bhh = r.b_hh; a.hidden = r.hidden; a.lengths = lengths; a.order = order;
    a.n_seq = n_seq; a.max_len = max_len; a.hcat = hcat;
    const size_t lds = (size_t)kRows * (H + 4) * sizeof(float);
    static OncePerDevice once;                                 // > 64 KB of dynamic LDS needs the opt-in (H = 1024: 64.25 KB)
    if (once.first()) allow_lds(k_t2m_gru<H>, (int)lds);
    hipLaunchKernelGGL(k_t2m_gru<H>, dim3((unsigned)((n_seq + kRows - 1) / kRows), 2), dim3(64 * kGruWaves), lds, st, a);
    if (int rc = launched("k_t2m_gru launch")) return rc;
    if (int rc = linear(st, hcat, 2 * H, n_seq, 2 * H, H, hd.w1, hd.b1, E_BIAS, y1, H)) return rc;
    GemmArgs g = {};
    g.a = y1; g.lda = H; g.m = n_seq; g.k = H; g.n = SYN_T2M_EMB; g.ln_g = hd.ln_g; g.ln_b = hd.ln_b; g.w = hd.w2; g.bias = hd.b2; g.epi = E_BIAS;
    g.c = out; g.ldc = SYN_T2M_EMB;
    return gemm(st, A_LN, g);
}

}  // namespace t2m
}  // namespace

extern "C" {

int syn_t2m_pack_weight(const float* w, int32_t n, int32_t k, int32_t conv_cin, int32_t layout, float* out, void* stream) {
    if (!w || !out) return fail_msg("syn_t2m_pack_weight: null pointer");
    if (n < 1 || k < 1 || n > (1 << 16) || k > (1 << 16) || conv_cin < 0 || (conv_cin > 0 && k != 4 * conv_cin))
        return fail_msg("syn_t2m_pack_weight: n, k outside 1 .. 65536, or a convolution whose k is not 4 conv_cin");
    if (layout != 0 && !((layout == SYN_T2M_TEXT_H || layout == SYN_T2M_MOTION_H) && n == 3 * layout && k == layout && conv_cin == 0))
        return fail_msg("syn_t2m_pack_weight: layout is 0 (GEMM) or the GRU width H (512 / 1024) of a 3 H x H weight_hh");
    const int kq = (int)(t2m::round_up(k, 16) / 16);
    const long frags = layout == 0 ? t2m::round_up(n, t2m::kBN) / 16 * kq : (long)3 * layout / 16 * kq;
    hipLaunchKernelGGL(t2m::k_t2m_pack, dim3((unsigned)((frags * 64 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (int)n, (int)k, (int)conv_cin,
                       (int)layout, frags, kq, out);
    return launched("k_t2m_pack launch");
}

int64_t syn_t2m_workspace_bytes(int32_t n_seq, int32_t max_len, int32_t kind) {
    if (n_seq < 1 || n_seq > SYN_T2M_MAX_SEQ || (kind != SYN_T2M_MOTION && kind != SYN_T2M_TEXT)) return -1;
    if (max_len < (kind == SYN_T2M_MOTION ? 4 : 1) || max_len > SYN_T2M_MAX_FRAMES) return -1;
    t2m::Carve c = {nullptr};
    const long n = n_seq;
    if (kind == SYN_T2M_MOTION) {
        const long t1 = t2m::conv_len(max_len), t2 = t2m::conv_len((int)t1);
        c.take(n * t1 * SYN_T2M_MOVE); c.take(n * t2 * SYN_T2M_MOVE); c.take(n * t2 * SYN_T2M_MOVE);
        c.take(n * t2 * SYN_T2M_MOTION_H); c.take(n * t2 * 6 * SYN_T2M_MOTION_H); c.take(n * 2 * SYN_T2M_MOTION_H); c.take(n * SYN_T2M_MOTION_H);
    } else {
        const long l = max_len;
        c.take(n * l * SYN_T2M_WORD); c.take(n * l * SYN_T2M_TEXT_H); c.take(n * l * 6 * SYN_T2M_TEXT_H); c.take(n * 2 * SYN_T2M_TEXT_H);
        c.take(n * SYN_T2M_TEXT_H);
    }
    return (long)(c.p - (char*)nullptr);
}

int syn_t2m_encode_motion(const syn_t2m_model* m, const float* motions, int32_t n_seq, int32_t n_frames, int32_t ld, const int32_t* lengths_dev,
                          const int32_t* order_dev, void* workspace, float* out, void* stream) {
    using namespace t2m;
    if (!m || !motions || !lengths_dev || !order_dev || !workspace || !out) return fail_msg("syn_t2m_encode_motion: null pointer");
    if (n_seq < 1 || n_seq > SYN_T2M_MAX_SEQ || n_frames < 4 || n_frames > SYN_T2M_MAX_FRAMES || ld < SYN_T2M_POSE)
        return fail_msg("syn_t2m_encode_motion: n_seq outside 1 .. SYN_T2M_MAX_SEQ, n_frames outside 4 .. SYN_T2M_MAX_FRAMES, or ld < 619");
    if (!m->conv1_w || !m->conv1_b || !m->conv2_w || !m->conv2_b || !m->out_w || !m->out_b || !m->motion_in_w || !m->motion_in_b ||
        !gru_ok(m->motion_gru) || !head_ok(m->motion_head))
        return fail_msg("syn_t2m_encode_motion: model with a null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int t1 = conv_len(n_frames), t2 = conv_len(t1);
    const long n = n_seq;
    constexpr int H = SYN_T2M_MOTION_H, C = SYN_T2M_MOVE;
    Carve ws = {(char*)workspace};                              // the order of syn_t2m_workspace_bytes
    float* c1 = ws.take(n * t1 * C); float* c2 = ws.take(n * t2 * C); float* mv = ws.take(n * t2 * C);
    float* emb = ws.take(n * t2 * H); float* gx = ws.take(n * t2 * 6 * H); float* hcat = ws.take(n * 2 * H); float* y1 = ws.take(n * H);
    GemmArgs g = {};
    g.a = motions; g.lda = ld; g.m = (int)(n * t1); g.k = 4 * SYN_T2M_POSE; g.n = C; g.cin = SYN_T2M_POSE; g.t_in = n_frames; g.t_out = t1;
    g.w = m->conv1_w; g.bias = m->conv1_b; g.epi = E_LEAKY; g.c = c1; g.ldc = C;
    if (int rc = gemm(st, A_CONV, g)) return rc;
    g.a = c1; g.lda = C; g.m = (int)(n * t2); g.k = 4 * C; g.cin = C; g.t_in = t1; g.t_out = t2; g.w = m->conv2_w; g.bias = m->conv2_b; g.c = c2;
    if (int rc = gemm(st, A_CONV, g)) return rc;
    if (int rc = linear(st, c2, C, n * t2, C, C, m->out_w, m->out_b, E_BIAS, mv, C)) return rc;
    if (int rc = linear(st, mv, C, n * t2, C, H, m->motion_in_w, m->motion_in_b, E_BIAS, emb, H)) return rc;
    if (int rc = linear(st, emb, H, n * t2, H, 6 * H, m->motion_gru.w_ih, m->motion_gru.b_ih, E_BIAS, gx, 6 * H)) return rc;
    return recur_and_head<H>(st, m->motion_gru, m->motion_head, gx, n_seq, t2, lengths_dev, order_dev, hcat, y1, out);
}

int syn_t2m_encode_text(const syn_t2m_model* m, const float* word_embs, const float* pos_onehot, int32_t n_seq, int32_t max_len,
                        const int32_t* lengths_dev, const int32_t* order_dev, void* workspace, float* out, void* stream) {
    using namespace t2m;
    if (!m || !word_embs || !pos_onehot || !lengths_dev || !order_dev || !workspace || !out) return fail_msg("syn_t2m_encode_text: null pointer");
    if (n_seq < 1 || n_seq > SYN_T2M_MAX_SEQ || max_len < 1 || max_len > SYN_T2M_MAX_FRAMES)
        return fail_msg("syn_t2m_encode_text: n_seq outside 1 .. SYN_T2M_MAX_SEQ or max_len outside 1 .. SYN_T2M_MAX_FRAMES");
    if (!m->pos_w || !m->pos_b || !m->text_in_w || !m->text_in_b || !gru_ok(m->text_gru) || !head_ok(m->text_head))
        return fail_msg("syn_t2m_encode_text: model with a null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long n = n_seq, rows = n * max_len;
    constexpr int H = SYN_T2M_TEXT_H, W = SYN_T2M_WORD;
    Carve ws = {(char*)workspace};
    float* x0 = ws.take(rows * W); float* emb = ws.take(rows * H); float* gx = ws.take(rows * 6 * H); float* hcat = ws.take(n * 2 * H);
    float* y1 = ws.take(n * H);
    if (int rc = linear(st, pos_onehot, SYN_T2M_POS, rows, SYN_T2M_POS, W, m->pos_w, m->pos_b, E_ADD, x0, W, word_embs, W)) return rc;
    if (int rc = linear(st, x0, W, rows, W, H, m->text_in_w, m->text_in_b, E_BIAS, emb, H)) return rc;
    if (int rc = linear(st, emb, H, rows, H, 6 * H, m->text_gru.w_ih, m->text_gru.b_ih, E_BIAS, gx, 6 * H)) return rc;
    return recur_and_head<H>(st, m->text_gru, m->text_head, gx, n_seq, max_len, lengths_dev, order_dev, hcat, y1, out);
}

}  // extern "C"
