// TMR's ACTOR-style encoders (models/temos/motionencoder/actor.py, textencoder/distillbert_actor.py): a 4-layer, 256-wide post-norm
// nn.TransformerEncoder over [mu_token, logvar_token, Linear(features)] + pe, read at rows 0 and 1 (DESIGN.md §10).
// Layout: the residual stream x is fp32 [n_seq][S = max_len + 2][256] in a caller's workspace; every Linear is one launch of k_tmr_gemm
// (64 rows x 256 output columns per workgroup, hi + lo bf16 split of both operands: three MFMAs per product) with its epilogue
// (embedding + pe + tokens, bias, GELU, or bias + residual + LayerNorm); attention is k_tmr_attn (a workgroup per sequence, head and 64 queries).
// The last layer runs its queries, out_proj, FFN and both LayerNorms on rows 0-1 of each sequence only ("head rows").
// syn_bert.inc uses this file's tile constants, split8 / load8, the packed-weight layout (k_tmr_pack) and `launched`.
namespace {
namespace tmr {

constexpr int kD = 256, kQKV = 768, kFF = 1024, kHeads = 4, kHd = 64, kMaxS = 256;
constexpr int kBM = 64, kBN = 256, kKC = 32;                   // GEMM tile: rows x output columns, k per staged chunk
constexpr int kArow = 80;                                      // LDS bytes per staged A row: 4 x 16 B of k + 16 B pad (ds_read_b128 rows off the same banks)

enum { EPI_EMBED = 0, EPI_BIAS_BF16 = 1, EPI_GELU = 2, EPI_LN = 3 };
enum { ROWS_ALL = 0, ROWS_EMBED = 1, ROWS_HEAD = 2 };

struct GemmArgs {
    const float* a; int lda; int K; int M;                     // A rows of the product: row a_row(i) of `a`, K valid columns (zero beyond)
    int a_mapped; int relu_in; int rows; int S; int L;         // a_mapped: A row = mapped row r (else logical row i); rows: ROWS_*
    const bf16x8* w; int KS; int n_frag_cols;                  // packed hi fragments [n/16][KS][64]; lo fragments follow the hi ones
    int col0;                                                  // first output column of this launch (multiple of 256)
    const float* bias;
    // epilogue
    const float* res; float* out_f; int ld_out; __bf16* out_h;
    const float* ln_g; const float* ln_b; const float* pe; const float* tok_mu; const float* tok_lv;
    float* head_mu; float* head_lv;                            // last LayerNorm: rows 0 / 1 of each sequence also go here
};

__device__ __forceinline__ int map_row(const GemmArgs& a, int i) {
    if (a.rows == ROWS_EMBED) return (i / a.L) * a.S + 2 + i % a.L;
    if (a.rows == ROWS_HEAD) return (i >> 1) * a.S + (i & 1);
    return i;
}

__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];
        hi[j] = h;
        lo[j] = (__bf16)(v[j] - (float)h);
    }
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// 256 threads; wave w owns output columns [64 w, 64 w + 64) of the tile, all 64 rows: acc[m tile][n tile].
template <int EPI>
__global__ __launch_bounds__(256) void k_tmr_gemm(const GemmArgs a) {
    __shared__ __attribute__((aligned(16))) char s_a[2][kBM * kArow];     // hi, lo
    __shared__ float s_red[4][kBM];
    __shared__ float s_stat[2][kBM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kBM;
    const int col_tile0 = a.col0 + blockIdx.y * kBN;
    // this thread's staging slot: row sr of the tile, k group sg (8 columns)
    const int sr = tid >> 2, sg = tid & 3;
    const int si = m0 + sr;
    const float* arow = nullptr;
    if (si < a.M) arow = a.a + (long)(a.a_mapped ? map_row(a, si) : si) * a.lda;
    const bool vec = (a.lda % 4) == 0 && ((uintptr_t)a.a & 15) == 0 && (a.K % kKC) == 0;

    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const long lo_off = (long)a.n_frag_cols * a.KS * 64;
    const int ntile0 = col_tile0 / 16 + wave * 4;
    float av[8];
    auto load_a = [&](int k0) {
        const int k = k0 + sg * 8;
        if (arow && vec) load8(arow + k, av);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = (arow && k + j < a.K) ? arow[k + j] : 0.f;
        }
        if (a.relu_in) {
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = fmaxf(av[j], 0.f);
        }
    };
    load_a(0);
    for (int ks = 0; ks < a.KS; ++ks) {
        bf16x8 bh[4], bl[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const long f = ((long)(ntile0 + nt) * a.KS + ks) * 64 + lane;
            bh[nt] = a.w[f];
            bl[nt] = a.w[lo_off + f];
        }
        bf16x8 hi, lo;
        split8(av, hi, lo);
        __syncthreads();                                       // the previous chunk's fragments have been read
        *reinterpret_cast<bf16x8*>(s_a[0] + sr * kArow + sg * 16) = hi;
        *reinterpret_cast<bf16x8*>(s_a[1] + sr * kArow + sg * 16) = lo;
        __syncthreads();
        if (ks + 1 < a.KS) load_a((ks + 1) * kKC);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int off = (mt * 16 + (lane & 15)) * kArow + (lane >> 4) * 16;
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(s_a[0] + off);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(s_a[1] + off);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                acc[mt][nt] = MFMA16(al, bh[nt], acc[mt][nt]);
                acc[mt][nt] = MFMA16(ah, bl[nt], acc[mt][nt]);
                acc[mt][nt] = MFMA16(ah, bh[nt], acc[mt][nt]);
            }
        }
    }

    // epilogue: acc[mt][nt][e] is row mt*16 + (lane>>4)*4 + e, column col_tile0 + wave*64 + nt*16 + (lane&15)
    const int cl = wave * 64 + (lane & 15);
    float bias[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bias[nt] = a.bias[col_tile0 + cl + nt * 16];
    if constexpr (EPI == EPI_LN) {
        // v = acc + bias + res; two-pass mean / variance over the 256 columns of a row (4 waves x 4 n tiles x 16 lanes)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = m0 + mt * 16 + (lane >> 4) * 4 + e;
                const float* rr = i < a.M ? a.res + (long)map_row(a, i) * kD : nullptr;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt][e] += bias[nt] + (rr ? rr[cl + nt * 16] : 0.f);
            }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int rt = mt * 16 + (lane >> 4) * 4 + e;
                    float s = 0.f;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        const float v = acc[mt][nt][e];
                        s += pass == 0 ? v : (v - s_stat[0][rt]) * (v - s_stat[0][rt]);
                    }
                    s += __shfl_xor(s, 1);
                    s += __shfl_xor(s, 2);
                    s += __shfl_xor(s, 4);
                    s += __shfl_xor(s, 8);
                    if ((lane & 15) == 0) s_red[wave][rt] = s;
                }
            __syncthreads();
            if (tid < kBM) {
                const float t = (s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]) * (1.f / kD);
                if (pass == 0) s_stat[0][tid] = t;
                else s_stat[1][tid] = rsqrtf(t + 1e-5f);
            }
            __syncthreads();
        }
        float g[4], b[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) { g[nt] = a.ln_g[cl + nt * 16]; b[nt] = a.ln_b[cl + nt * 16]; }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int rt = mt * 16 + (lane >> 4) * 4 + e, i = m0 + rt;
                if (i >= a.M) continue;
                const int r = map_row(a, i);
                const float mean = s_stat[0][rt], rstd = s_stat[1][rt];
                float* o = a.out_f + (long)r * kD;
                float* h = nullptr;
                if (a.head_mu && a.rows == ROWS_HEAD) h = ((i & 1) ? a.head_lv : a.head_mu) + (long)(i >> 1) * kD;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const float y = (acc[mt][nt][e] - mean) * rstd * g[nt] + b[nt];
                    o[cl + nt * 16] = y;
                    if (h) h[cl + nt * 16] = y;
                }
            }
    } else {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = m0 + mt * 16 + (lane >> 4) * 4 + e;
                if (i >= a.M) continue;
                const int r = map_row(a, i);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const int c = col_tile0 + cl + nt * 16;
                    const float v = acc[mt][nt][e] + bias[nt];
                    if constexpr (EPI == EPI_EMBED) {
                        const int s = r % a.S;
                        a.out_f[(long)r * kD + c] = v + a.pe[s * kD + c];
                        if (s == 2) {                          // the sequence's distribution tokens, rows 0 / 1 (+ pe[0], pe[1])
                            a.out_f[(long)(r - 2) * kD + c] = a.tok_mu[c] + a.pe[c];
                            a.out_f[(long)(r - 1) * kD + c] = a.tok_lv[c] + a.pe[kD + c];
                        }
                    } else if constexpr (EPI == EPI_BIAS_BF16) {
                        a.out_h[(long)r * a.ld_out + c] = (__bf16)v;
                    } else {
                        a.out_f[(long)i * a.ld_out + c] = gelu_erf(v);
                    }
                }
            }
    }
}

// Self-attention of one head over one sequence for 64 queries (4 waves x 16): S = QK^T / 8 with keys >= 2 + n masked, fp32 softmax,
// O = P V.  Q, K, V are the bf16 qkv rows; P goes through the LDS as bf16, V is staged transposed (the B operand wants 8 keys per lane).
__global__ __launch_bounds__(256) void k_tmr_attn(const __bf16* __restrict__ qkv, const int32_t* __restrict__ lengths, int S, int L,
                                                  int q_rows, float* __restrict__ o) {
    __shared__ __attribute__((aligned(16))) __bf16 s_vt[kHd][kMaxS + 8];
    __shared__ __attribute__((aligned(16))) __bf16 s_p[4][16][kMaxS + 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    int n = lengths ? lengths[b] : L;
    n = n < 0 ? 0 : (n > L ? L : n);
    const int valid = 2 + n;                                   // keys 0 .. valid-1 attend (the two tokens always)
    const int kt_n = (valid + 15) / 16;
    const __bf16* base = qkv + (long)b * S * kQKV;
    // V^T of the valid keys (zero to the next 32 so that the last k step reads defined values)
    const int kpad = (valid + 31) & ~31;
    for (int t = tid; t < kpad * 8; t += 256) {
        const int key = t >> 3, dg = (t & 7) * 8;
        bf16x8 v = {};
        if (key < valid) v = *reinterpret_cast<const bf16x8*>(base + (long)key * kQKV + 2 * kD + h * kHd + dg);
#pragma unroll
        for (int j = 0; j < 8; ++j) s_vt[dg + j][key] = v[j];
    }
    const int q0 = qt * 64 + wave * 16;
    const bool active = q0 < q_rows;
    f32x4 sc[kMaxS / 16];
    if (active) {
        // Q fragments (A operand): row q0 + (lane & 15), d = 32 ks + 8 (lane >> 4) + j
        const int qr = q0 + (lane & 15);
        bf16x8 qa[2] = {};
        if (qr < S) {
            qa[0] = *reinterpret_cast<const bf16x8*>(base + (long)qr * kQKV + h * kHd + (lane >> 4) * 8);
            qa[1] = *reinterpret_cast<const bf16x8*>(base + (long)qr * kQKV + h * kHd + 32 + (lane >> 4) * 8);
        }
#pragma unroll
        for (int kt = 0; kt < kMaxS / 16; ++kt) {
            sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kt < kt_n) {
                const int key = kt * 16 + (lane & 15);
                bf16x8 k0 = {}, k1 = {};
                if (key < valid) {
                    k0 = *reinterpret_cast<const bf16x8*>(base + (long)key * kQKV + kD + h * kHd + (lane >> 4) * 8);
                    k1 = *reinterpret_cast<const bf16x8*>(base + (long)key * kQKV + kD + h * kHd + 32 + (lane >> 4) * 8);
                }
                sc[kt] = MFMA16(qa[0], k0, sc[kt]);
                sc[kt] = MFMA16(qa[1], k1, sc[kt]);
            }
        }
    }
    float inv_sum[4];
    if (active) {
        // softmax along a query row: its keys are the 16 lanes of a lane group x the key tiles
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < kMaxS / 16; ++kt)
                if (kt < kt_n && kt * 16 + (lane & 15) < valid) m = fmaxf(m, sc[kt][e] * 0.125f);
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));
            m = fmaxf(m, __shfl_xor(m, 4));
            m = fmaxf(m, __shfl_xor(m, 8));
            float s = 0.f;
            const int qrow = (lane >> 4) * 4 + e;
#pragma unroll
            for (int kt = 0; kt < kMaxS / 16; ++kt) {
                if (kt * 16 >= kpad) break;
                const int key = kt * 16 + (lane & 15);
                float p = 0.f;
                if (kt < kt_n && key < valid) p = __expf(sc[kt][e] * 0.125f - m);
                const __bf16 pb = (__bf16)p;
                s += (float)pb;                                // the row sum of exactly the weights P V uses
                s_p[wave][qrow][key] = pb;
            }
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 8);
            inv_sum[e] = 1.f / s;
        }
    }
    __syncthreads();                                           // V^T staged, P written
    if (!active) return;
    f32x4 oa[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) oa[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < kpad / 32; ++ks) {
        const bf16x8 pa = *reinterpret_cast<const bf16x8*>(&s_p[wave][lane & 15][ks * 32 + (lane >> 4) * 8]);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const bf16x8 vb = *reinterpret_cast<const bf16x8*>(&s_vt[nt * 16 + (lane & 15)][ks * 32 + (lane >> 4) * 8]);
            oa[nt] = MFMA16(pa, vb, oa[nt]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = q0 + (lane >> 4) * 4 + e;
        if (q >= q_rows || q >= S) continue;
        float* orow = o + ((long)b * S + q) * kD + h * kHd;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) orow[nt * 16 + (lane & 15)] = oa[nt][e] * inv_sum[e];
    }
}

// fp32 W [n][k] -> hi and lo bf16 fragments of the 16x16x32 MFMA's B operand: [n/16][kp/32][64 lanes][8], lane l holding
// W[16 nt + (l & 15)][32 ks + 8 (l >> 4) + j]; columns k .. kp-1 are zero.  The lo fragments follow all hi ones.
__global__ __launch_bounds__(256) void k_tmr_pack(const float* __restrict__ w, int n, int k, int ks_n, bf16x8* __restrict__ out) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x, total = (long)n / 16 * ks_n * 64;
    if (g >= total) return;
    const int lane = (int)(g & 63);
    const long f = g >> 6;
    const int ks = (int)(f % ks_n), nt = (int)(f / ks_n);
    const int row = nt * 16 + (lane & 15), c0 = ks * 32 + (lane >> 4) * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = c0 + j < k ? w[(long)row * k + c0 + j] : 0.f;
    bf16x8 hi, lo;
    split8(v, hi, lo);
    out[g] = hi;
    out[total + g] = lo;
}

template <int EPI>
int gemm(const GemmArgs& a, int n_cols, hipStream_t st) {
    dim3 grid((unsigned)((a.M + kBM - 1) / kBM), (unsigned)(n_cols / kBN));
    hipLaunchKernelGGL(k_tmr_gemm<EPI>, grid, dim3(256), 0, st, a);
    return launched("k_tmr_gemm launch");
}

}  // namespace tmr
}  // namespace

extern "C" {

int syn_tmr_pack_weight(const float* w, int32_t n, int32_t k, void* out, void* stream) {
    if (!w || !out || n < 16 || n % 16 || k < 1 || k > SYN_TMR_MAX_FEATS)
        return fail_msg("syn_tmr_pack_weight: null pointer, rows not a positive multiple of 16, or columns outside 1 .. SYN_TMR_MAX_FEATS");
    const int ks = (k + 31) / 32;
    const long total = (long)n / 16 * ks * 64;
    hipLaunchKernelGGL(tmr::k_tmr_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (int)n, (int)k, ks, (bf16x8*)out);
    return launched("k_tmr_pack launch");
}

int syn_tmr_encode(const syn_tmr_model* m, const float* features, int32_t n_seq, int32_t max_len, const int32_t* lengths, void* workspace,
                   float* mu, float* logvar, void* stream) {
    using namespace tmr;
    if (!m || !features || !workspace || !mu || !logvar) return fail_msg("syn_tmr_encode: null pointer");
    if (n_seq < 1 || n_seq > SYN_TMR_MAX_SEQ || max_len < 1 || max_len > SYN_TMR_MAX_LEN)
        return fail_msg("syn_tmr_encode: n_seq outside 1 .. SYN_TMR_MAX_SEQ or max_len outside 1 .. SYN_TMR_MAX_LEN");
    if (m->nfeats < 1 || m->nfeats > SYN_TMR_MAX_FEATS || !m->w_in || !m->b_in || !m->mu_token || !m->logvar_token || !m->pe)
        return fail_msg("syn_tmr_encode: model has nfeats outside 1 .. SYN_TMR_MAX_FEATS or a null input weight / token / pe");
    for (int l = 0; l < SYN_TMR_LAYERS; ++l) {
        const syn_tmr_layer& y = m->layer[l];
        if (!y.w_qkv || !y.b_qkv || !y.w_out || !y.b_out || !y.ln1_g || !y.ln1_b || !y.w_fc1 || !y.b_fc1 || !y.w_fc2 || !y.b_fc2 || !y.ln2_g || !y.ln2_b)
            return fail_msg("syn_tmr_encode: model layer with a null weight");
    }
    hipStream_t st = (hipStream_t)stream;
    const int S = max_len + 2, R = n_seq * S;
    char* ws = (char*)workspace;                                // layout: syn_tmr_encode's comment in the header (tmr.workspace_bytes)
    float* x = (float*)ws;                       ws += (size_t)R * kD * 4;
    __bf16* qkv = (__bf16*)ws;                   ws += (size_t)R * kQKV * 2;
    float* o = (float*)ws;                       ws += (size_t)R * kD * 4;
    float* hid = (float*)ws;

    GemmArgs base = {};                                         // what every Linear of the stack shares: a 256-wide, row-mapped A
    base.S = S; base.L = max_len; base.lda = kD; base.K = kD; base.KS = kD / 32; base.n_frag_cols = kD / 16; base.a_mapped = 1;
    GemmArgs g = base;                                          // input Linear (+ ReLU for text) + pe, and the two distribution tokens
    g.a = features; g.lda = m->nfeats; g.K = m->nfeats; g.M = n_seq * max_len; g.a_mapped = 0; g.relu_in = m->relu_in ? 1 : 0; g.rows = ROWS_EMBED;
    g.w = (const bf16x8*)m->w_in; g.KS = (m->nfeats + 31) / 32; g.bias = m->b_in;
    g.out_f = x; g.pe = m->pe; g.tok_mu = m->mu_token; g.tok_lv = m->logvar_token;
    int rc = gemm<EPI_EMBED>(g, kD, st);
    for (int l = 0; l < SYN_TMR_LAYERS && !rc; ++l) {
        const syn_tmr_layer& y = m->layer[l];
        const bool last = l == SYN_TMR_LAYERS - 1;
        GemmArgs q = base;                                     // in_proj of every row
        q.a = x; q.M = R; q.rows = ROWS_ALL; q.w = (const bf16x8*)y.w_qkv; q.n_frag_cols = kQKV / 16; q.bias = y.b_qkv; q.out_h = qkv; q.ld_out = kQKV;
        if (!last) {
            rc = gemm<EPI_BIAS_BF16>(q, kQKV, st);
        } else {                                               // keys / values of every row, queries of rows 0-1
            q.col0 = kD;
            rc = gemm<EPI_BIAS_BF16>(q, 2 * kD, st);
            q.M = 2 * n_seq; q.rows = ROWS_HEAD; q.col0 = 0;
            if (!rc) rc = gemm<EPI_BIAS_BF16>(q, kD, st);
        }
        if (rc) return rc;
        const int q_rows = last ? 2 : S;
        hipLaunchKernelGGL(k_tmr_attn, dim3((unsigned)((q_rows + 63) / 64), kHeads, (unsigned)n_seq), dim3(256), 0, st, qkv, lengths, S, max_len, q_rows, o);
        if ((rc = launched("k_tmr_attn launch"))) return rc;
        GemmArgs t = base;                                     // from here on the last layer runs its head rows only
        t.rows = last ? ROWS_HEAD : ROWS_ALL; t.M = last ? 2 * n_seq : R;
        GemmArgs p = t;                                        // out_proj + residual + norm1
        p.a = o; p.w = (const bf16x8*)y.w_out; p.bias = y.b_out; p.res = x; p.out_f = x; p.ln_g = y.ln1_g; p.ln_b = y.ln1_b;
        if ((rc = gemm<EPI_LN>(p, kD, st))) return rc;
        GemmArgs f = t;                                        // linear1 + GELU
        f.a = x; f.w = (const bf16x8*)y.w_fc1; f.n_frag_cols = kFF / 16; f.bias = y.b_fc1; f.out_f = hid; f.ld_out = kFF;
        if ((rc = gemm<tmr::EPI_GELU>(f, kFF, st))) return rc;
        GemmArgs s = t;                                        // linear2 + residual + norm2 (the last layer's rows 0 / 1 are mu / logvar)
        s.a = hid; s.lda = kFF; s.K = kFF; s.KS = kFF / 32; s.a_mapped = 0; s.w = (const bf16x8*)y.w_fc2; s.bias = y.b_fc2;
        s.res = x; s.out_f = x; s.ln_g = y.ln2_g; s.ln_b = y.ln2_b;
        if (last) { s.head_mu = mu; s.head_lv = logvar; }
        rc = gemm<EPI_LN>(s, kD, st);
    }
    return rc;
}

}  // extern "C"
