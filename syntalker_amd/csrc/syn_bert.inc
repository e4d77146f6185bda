// DistilBERT's forward in front of TMR's text encoder (transformers' DistilBertModel: embeddings + n post-norm TransformerBlocks, 768 wide,
// 12 heads x 64, FF 3072, erf GELU, LayerNorm eps 1e-12; DESIGN.md §14): token ids -> last_hidden_state.
// Layout: rows are padded, row i = sequence i / L, position i % L; the residual stream x IS the caller's `hidden` [n_seq][L][768] fp32, rows at
// or beyond a sequence's length are zero and are never computed: a GEMM tile without a valid row returns, a GEMM reads zeros for an invalid
// row of A and writes no invalid row.  Every Linear is one launch of k_bert_gemm (k_tmr_gemm's tile and hi + lo bf16 split: 64 rows x 256
// columns, three MFMAs per product) with bias, bias + GELU or bias + residual; a LayerNorm is its own launch (k_bert_ln, a wave per row);
// attention is k_bert_attn (a workgroup per sequence, head and 64 queries) with hi + lo bf16 splits of Q, K, P and V as well.
namespace {
namespace bert {

using tmr::kArow;
using tmr::kBM;
using tmr::kBN;
using tmr::kKC;
using tmr::load8;
using tmr::split8;

constexpr int kD = SYN_BERT_D, kQKV = 3 * SYN_BERT_D, kFF = SYN_BERT_FF, kHeads = SYN_BERT_HEADS, kHd = 64;
static_assert(kHeads * kHd == kD && kD % kBN == 0 && kQKV % kBN == 0 && kFF % kBN == 0 && kD % kKC == 0 && kFF % kKC == 0, "tile shapes");

enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RES = 2 };

struct GemmArgs {
    const float* a; int lda; int KS; int M; int L;             // A: M = n_seq L rows of KS x 32 columns, 16-byte aligned rows
    const int32_t* lengths;
    const bf16x8* w; int n_frag_cols;                          // packed hi fragments [n/16][KS][64]; lo fragments follow the hi ones
    const float* bias; const float* res; float* out; int ld_out;
};

__device__ __forceinline__ bool row_valid(const int32_t* lengths, int L, int M, int i) {
    if (i >= M) return false;
    return lengths ? i % L < lengths[i / L] : true;
}

// 256 threads; wave w owns output columns [64 w, 64 w + 64) of the tile, all 64 rows: acc[m tile][n tile] (k_tmr_gemm's main loop).
template <int EPI>
__global__ __launch_bounds__(256) void k_bert_gemm(const GemmArgs a) {
    __shared__ __attribute__((aligned(16))) char s_a[2][kBM * kArow];     // hi, lo
    __shared__ int s_valid[kBM];
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kBM;
    const int col_tile0 = blockIdx.y * kBN;
    // this thread's staging slot: row sr of the tile, k group sg (8 columns)
    const int sr = tid >> 2, sg = tid & 3;
    const int si = m0 + sr;
    const bool ok = row_valid(a.lengths, a.L, a.M, si);
    if (tid == 0) s_any = 0;
    __syncthreads();
    if (sg == 0) {
        s_valid[sr] = ok;
        if (ok) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;                                        // a tile of padding rows only
    const float* arow = ok ? a.a + (long)si * a.lda : nullptr;

    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const long lo_off = (long)a.n_frag_cols * a.KS * 64;
    const int ntile0 = col_tile0 / 16 + wave * 4;
    float av[8];
    auto load_a = [&](int k0) {
        if (arow) load8(arow + k0 + sg * 8, av);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = 0.f;
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
    const int c0 = col_tile0 + wave * 64 + (lane & 15);
    float bias[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bias[nt] = a.bias[c0 + nt * 16];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rt = mt * 16 + (lane >> 4) * 4 + e;
            if (!s_valid[rt]) continue;
            const long i = m0 + rt;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int c = c0 + nt * 16;
                float v = acc[mt][nt][e] + bias[nt];
                if constexpr (EPI == EPI_GELU) v = gelu_erf(v);
                if constexpr (EPI == EPI_RES) v += a.res[i * kD + c];
                a.out[i * a.ld_out + c] = v;
            }
        }
}

// A wave per row of 768: EMBED: word[id] + pos[position] (ids clamped into the table), else src's row; LayerNorm with eps 1e-12 in fp32, the
// variance in a second pass over the registers.  Rows at or beyond the sequence's length are written as zeros.
template <bool EMBED>
__global__ __launch_bounds__(256) void k_bert_ln(const float* __restrict__ src, const int32_t* __restrict__ ids, const float* __restrict__ word,
                                                 const float* __restrict__ pos, int vocab, const int32_t* __restrict__ lengths, int L, int M,
                                                 const float* __restrict__ g, const float* __restrict__ b, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 4 + wave;
    if (i >= M) return;
    float* o = out + i * kD;
    if (!row_valid(lengths, L, M, (int)i)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) *reinterpret_cast<float4*>(o + j * 256 + lane * 4) = float4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    float4 v[3];
    if constexpr (EMBED) {
        int id = ids[i];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const float* wr = word + (long)id * kD;
        const float* pr = pos + (long)(i % L) * kD;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 p = *reinterpret_cast<const float4*>(wr + j * 256 + lane * 4), q = *reinterpret_cast<const float4*>(pr + j * 256 + lane * 4);
            v[j] = float4{p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w};
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = *reinterpret_cast<const float4*>(src + i * kD + j * 256 + lane * 4);
    }
    auto wave_sum = [](float s) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
        return s;
    };
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    const float mean = wave_sum(s) * (1.f / kD);
    s = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float dx = v[j].x - mean, dy = v[j].y - mean, dz = v[j].z - mean, dw = v[j].w - mean;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = rsqrtf(wave_sum(s) * (1.f / kD) + 1e-12f);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float4 gg = *reinterpret_cast<const float4*>(g + j * 256 + lane * 4), bb = *reinterpret_cast<const float4*>(b + j * 256 + lane * 4);
        *reinterpret_cast<float4*>(o + j * 256 + lane * 4) = float4{(v[j].x - mean) * rstd * gg.x + bb.x, (v[j].y - mean) * rstd * gg.y + bb.y,
                                                                    (v[j].z - mean) * rstd * gg.z + bb.z, (v[j].w - mean) * rstd * gg.w + bb.w};
    }
}

// Self-attention of one head over one sequence for 64 queries (4 waves x 16), k_tmr_attn's structure on split operands: S = QK^T / 8 over the
// n valid keys, fp32 softmax, O = P V, each product as three MFMAs on hi + lo bf16 halves of both sides.  Q, K, V are the fp32 qkv rows;
// P goes through the LDS, V is staged transposed.  LDS: [V^T hi | V^T lo](64 rows) [P hi | P lo](4 waves x 16 rows), `stride` bf16 per row
// (roundup(L, 32) + 8).  NKT: key tiles of 16 held in registers (4: L <= 64, 16: L <= 256).
template <int NKT>
__global__ __launch_bounds__(256) void k_bert_attn(const float* __restrict__ qkv, const int32_t* __restrict__ lengths, int L, int stride,
                                                   float* __restrict__ o) {
    extern __shared__ __attribute__((aligned(16))) char smem_bert[];
    __bf16* s_vh = reinterpret_cast<__bf16*>(smem_bert);
    __bf16* s_vl = s_vh + 64 * stride;
    __bf16* s_ph = s_vl + 64 * stride;
    __bf16* s_pl = s_ph + 64 * stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, h = blockIdx.y, qt = blockIdx.z;
    int n = lengths ? lengths[b] : L;
    n = n < 0 ? 0 : (n > L ? L : n);
    if (qt * 64 >= n) return;                                  // no valid query in this tile (the whole workgroup)
    const int kt_n = (n + 15) / 16;
    const int kpad = (n + 31) & ~31;                           // <= roundup(L, 32) <= NKT * 16
    const float* base = qkv + (long)b * L * kQKV;
    // V^T of the valid keys (zero to the next 32 so that the last k step reads defined values)
    for (int t = tid; t < kpad * 8; t += 256) {
        const int key = t >> 3, dg = (t & 7) * 8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (key < n) load8(base + (long)key * kQKV + 2 * kD + h * kHd + dg, v);
        bf16x8 hi, lo;
        split8(v, hi, lo);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s_vh[(dg + j) * stride + key] = hi[j];
            s_vl[(dg + j) * stride + key] = lo[j];
        }
    }
    const int q0 = qt * 64 + wave * 16;
    const bool active = q0 < n;
    f32x4 sc[NKT];
    float inv_sum[4];
    if (active) {
        // Q fragments (A operand): row q0 + (lane & 15), d = 32 ks + 8 (lane >> 4) + j
        const int qr = q0 + (lane & 15);
        bf16x8 qh[2], ql[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (qr < n) load8(base + (long)qr * kQKV + h * kHd + ks * 32 + (lane >> 4) * 8, v);
            split8(v, qh[ks], ql[ks]);
        }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kt < kt_n) {
                const int key = kt * 16 + (lane & 15);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (key < n) load8(base + (long)key * kQKV + kD + h * kHd + ks * 32 + (lane >> 4) * 8, v);
                    bf16x8 kh, kl;
                    split8(v, kh, kl);
                    sc[kt] = MFMA16(ql[ks], kh, sc[kt]);
                    sc[kt] = MFMA16(qh[ks], kl, sc[kt]);
                    sc[kt] = MFMA16(qh[ks], kh, sc[kt]);
                }
            }
        }
        // softmax along a query row: its keys are the 16 lanes of a lane group x the key tiles
        __bf16* ph = s_ph + wave * 16 * stride;
        __bf16* pl = s_pl + wave * 16 * stride;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
                if (kt < kt_n && kt * 16 + (lane & 15) < n) m = fmaxf(m, sc[kt][e] * 0.125f);
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));
            m = fmaxf(m, __shfl_xor(m, 4));
            m = fmaxf(m, __shfl_xor(m, 8));
            float s = 0.f;
            const int qrow = (lane >> 4) * 4 + e;
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                if (kt * 16 >= kpad) break;
                const int key = kt * 16 + (lane & 15);
                float p = 0.f;
                if (kt < kt_n && key < n) p = __expf(sc[kt][e] * 0.125f - m);
                const __bf16 hi = (__bf16)p, lo = (__bf16)(p - (float)hi);
                s += (float)hi + (float)lo;                    // the row sum of exactly the weights P V uses
                ph[qrow * stride + key] = hi;
                pl[qrow * stride + key] = lo;
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
        const int pof = (wave * 16 + (lane & 15)) * stride + ks * 32 + (lane >> 4) * 8;
        const bf16x8 pah = *reinterpret_cast<const bf16x8*>(s_ph + pof), pal = *reinterpret_cast<const bf16x8*>(s_pl + pof);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int vof = (nt * 16 + (lane & 15)) * stride + ks * 32 + (lane >> 4) * 8;
            const bf16x8 vbh = *reinterpret_cast<const bf16x8*>(s_vh + vof), vbl = *reinterpret_cast<const bf16x8*>(s_vl + vof);
            oa[nt] = MFMA16(pal, vbh, oa[nt]);
            oa[nt] = MFMA16(pah, vbl, oa[nt]);
            oa[nt] = MFMA16(pah, vbh, oa[nt]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = q0 + (lane >> 4) * 4 + e;
        if (q >= n) continue;
        float* orow = o + ((long)b * L + q) * kD + h * kHd;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) orow[nt * 16 + (lane & 15)] = oa[nt][e] * inv_sum[e];
    }
}

template <int EPI>
int gemm(const GemmArgs& a, int n_cols, hipStream_t st) {
    dim3 grid((unsigned)((a.M + kBM - 1) / kBM), (unsigned)(n_cols / kBN));
    hipLaunchKernelGGL(k_bert_gemm<EPI>, grid, dim3(256), 0, st, a);
    return launched("k_bert_gemm launch");
}

}  // namespace bert
}  // namespace

extern "C" int syn_bert_encode(const syn_bert_model* m, const int32_t* ids, int32_t n_seq, int32_t max_len, const int32_t* lengths, void* workspace,
                    float* hidden, void* stream) {
    using namespace bert;
    if (!m || !ids || !workspace || !hidden) return fail_msg("syn_bert_encode: null pointer");
    if (n_seq < 1 || n_seq > SYN_TMR_MAX_SEQ || max_len < 1 || max_len > SYN_TMR_MAX_LEN)
        return fail_msg("syn_bert_encode: n_seq outside 1 .. SYN_TMR_MAX_SEQ or max_len outside 1 .. SYN_TMR_MAX_LEN");
    if (m->n_layers < 1 || m->n_layers > SYN_BERT_MAX_LAYERS) return fail_msg("syn_bert_encode: model n_layers outside 1 .. SYN_BERT_MAX_LAYERS");
    if (m->vocab < 1 || m->n_pos < max_len) return fail_msg("syn_bert_encode: model vocab < 1 or fewer position rows (n_pos) than max_len");
    if (!m->word || !m->pos || !m->emb_ln_g || !m->emb_ln_b) return fail_msg("syn_bert_encode: model with a null embedding table or LayerNorm");
    for (int l = 0; l < m->n_layers; ++l) {
        const syn_bert_layer& y = m->layer[l];
        if (!y.w_qkv || !y.b_qkv || !y.w_out || !y.b_out || !y.ln1_g || !y.ln1_b || !y.w_fc1 || !y.b_fc1 || !y.w_fc2 || !y.b_fc2 || !y.ln2_g || !y.ln2_b)
            return fail_msg("syn_bert_encode: model layer with a null weight");
    }
    if (((uintptr_t)workspace | (uintptr_t)hidden | (uintptr_t)m->word | (uintptr_t)m->pos) & 15)
        return fail_msg("syn_bert_encode: workspace, hidden and the embedding tables must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int R = n_seq * max_len;
    float* x = hidden;
    float* qkv = (float*)workspace;                             // layout: syn_bert_encode's comment in the header (tmr.bert_workspace_bytes)
    float* tmp = qkv;                                           // a Linear's output before its LayerNorm: the qkv rows are dead by then
    float* o = qkv + (size_t)R * kQKV;
    float* hid = o + (size_t)R * kD;
    const int stride = ((max_len + 31) & ~31) + 8;
    const int lds = 256 * stride * 2;
    static OncePerDevice once;
    if (once.first()) { allow_lds(k_bert_attn<4>, 160 * 1024); allow_lds(k_bert_attn<16>, 160 * 1024); }

    const unsigned ln_grid = (unsigned)((R + 3) / 4);
    hipLaunchKernelGGL(k_bert_ln<true>, dim3(ln_grid), dim3(256), 0, st, (const float*)nullptr, ids, m->word, m->pos, (int)m->vocab, lengths,
                       (int)max_len, R, m->emb_ln_g, m->emb_ln_b, x);
    int rc = launched("k_bert_ln launch");
    if (rc) return rc;
    for (int l = 0; l < m->n_layers; ++l) {
        const syn_bert_layer& y = m->layer[l];
        GemmArgs g = {};
        g.M = R; g.L = max_len; g.lengths = lengths;
        g.a = x; g.lda = kD; g.KS = kD / kKC; g.w = (const bf16x8*)y.w_qkv; g.n_frag_cols = kQKV / 16; g.bias = y.b_qkv; g.out = qkv; g.ld_out = kQKV;
        if ((rc = gemm<EPI_BIAS>(g, kQKV, st))) return rc;
        const dim3 agrid((unsigned)n_seq, kHeads, (unsigned)((max_len + 63) / 64));
        if (max_len <= 64) hipLaunchKernelGGL(k_bert_attn<4>, agrid, dim3(256), lds, st, (const float*)qkv, lengths, (int)max_len, stride, o);
        else hipLaunchKernelGGL(k_bert_attn<16>, agrid, dim3(256), lds, st, (const float*)qkv, lengths, (int)max_len, stride, o);
        if ((rc = launched("k_bert_attn launch"))) return rc;
        g.a = o; g.w = (const bf16x8*)y.w_out; g.n_frag_cols = kD / 16; g.bias = y.b_out; g.res = x; g.out = tmp; g.ld_out = kD;   // out_lin + residual
        if ((rc = gemm<EPI_RES>(g, kD, st))) return rc;
        hipLaunchKernelGGL(k_bert_ln<false>, dim3(ln_grid), dim3(256), 0, st, (const float*)tmp, (const int32_t*)nullptr, (const float*)nullptr,
                           (const float*)nullptr, 0, lengths, (int)max_len, R, y.ln1_g, y.ln1_b, x);
        if ((rc = launched("k_bert_ln launch"))) return rc;
        g.a = x; g.w = (const bf16x8*)y.w_fc1; g.n_frag_cols = kFF / 16; g.bias = y.b_fc1; g.res = nullptr; g.out = hid; g.ld_out = kFF;  // lin1 + GELU
        if ((rc = gemm<bert::EPI_GELU>(g, kFF, st))) return rc;
        g.a = hid; g.lda = kFF; g.KS = kFF / kKC; g.w = (const bf16x8*)y.w_fc2; g.n_frag_cols = kD / 16; g.bias = y.b_fc2; g.res = x; g.out = tmp;
        g.ld_out = kD;                                          // lin2 + residual
        if ((rc = gemm<EPI_RES>(g, kD, st))) return rc;
        hipLaunchKernelGGL(k_bert_ln<false>, dim3(ln_grid), dim3(256), 0, st, (const float*)tmp, (const int32_t*)nullptr, (const float*)nullptr,
                           (const float*)nullptr, 0, lengths, (int)max_len, R, y.ln2_g, y.ln2_b, x);
        if ((rc = launched("k_bert_ln launch"))) return rc;
    }
    return 0;
}
