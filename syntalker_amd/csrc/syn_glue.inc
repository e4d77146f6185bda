// syn_glue.inc — the seams of the training step (SURVEY.md §8 a10): what sits BETWEEN the GEMMs, convolutions and block kernels of
// `training_losses` forward + backward.  In the reference these are torch.cat / avg_pool1d / permute / .to() / embedding / masked_l2
// (models/denoiser.py:147-176, diffusion/gaussian_diffusion.py:202-215, 1307-1314); as PyTorch ops around hand-written kernels they were
// ~90 launches of 2-15 us per step (0.36 ms of a 4.6 ms step, profiles/r05_train_step_split.txt).  Every kernel here writes a GEMM
// operand in the form the GEMM takes it (bf16 rows, zero-padded to the 128-column granularity) or reads a gradient where the GEMM left it
// (a column slice of a wider fp32 tensor), so no cast, cat, pad, slice copy or transpose launch is left.  All HBM-bound elementwise work:
// one pass, coalesced 16-byte accesses.  Included by syn_kernels.hip; entry points at the end.

namespace {
namespace glu {

// ---- bf16 GEMM operand [M][out_ld] = the concatenation of up to 4 fp32 sources along the columns (+ zero padding) ---------------------------
// Source s contributes `width` columns; row r of the operand reads source row r / row_div (a per-clip vector broadcast over the clip's
// frames: denoiser.py:160-174 `emb.repeat`, denoiser_h3d.py:196) or the MEAN of source rows r * pool .. + pool - 1 (F.avg_pool1d over the frame
// axis, denoiser.py:157); p2: a second tensor of the same shape added first (emb_seed + emb_t).
constexpr int kCatMax = 4;
struct CatSrc { const float* p; const float* p2; int width, ld, row_div, pool; };
struct CatArgs { CatSrc s[kCatMax]; int n_src, M, out_ld; __bf16* out; };
__global__ __launch_bounds__(256) void k_rows_concat_bf16(const CatArgs a) {
    const int q4 = a.out_ld / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.M * q4) return;
    const int r = (int)(i / q4);
    int c = (int)(i - (long)r * q4) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    int col = c;
#pragma unroll
    for (int s = 0; s < kCatMax; ++s) {
        if (s >= a.n_src) break;
        const CatSrc& S = a.s[s];
        if (col >= 0 && col < S.width) {
            if (S.pool > 1) {
                for (int j = 0; j < S.pool; ++j) v = v + *reinterpret_cast<const f32x4*>(S.p + ((size_t)r * S.pool + j) * S.ld + col);
                v = v * (1.0f / (float)S.pool);
            } else {
                const size_t at = (size_t)(r / S.row_div) * S.ld + col;
                v = *reinterpret_cast<const f32x4*>(S.p + at);
                if (S.p2) v = v + *reinterpret_cast<const f32x4*>(S.p2 + at);
            }
        }
        col -= S.width;
    }
    *reinterpret_cast<bf16x4*>(a.out + (size_t)r * a.out_ld + c) = to_bf16x4(v);
}

// ---- nn.Embedding lookup straight into the following Linear's operand: out[r][0:D] = bf16(table[ids[r]]), columns D .. out_ld zero ------
// (models/denoiser.py:72,152: text_pre_encoder_body in front of text_encoder_body, D = 300 -> 384 columns.)
__global__ __launch_bounds__(256) void k_embed_rows_bf16(const long* __restrict__ ids, const float* __restrict__ table, int V, int D, int M, int out_ld,
                                                         __bf16* __restrict__ out) {
    const int q4 = out_ld / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)M * q4) return;
    const int r = (int)(i / q4), c = (int)(i - (long)r * q4) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const long id = ids[r];
    if (c < D && id >= 0 && id < V) v = *reinterpret_cast<const f32x4*>(table + (size_t)id * D + c);
    *reinterpret_cast<bf16x4*>(out + (size_t)r * out_ld + c) = to_bf16x4(v);
}

// ---- (B, C, 1, T) fp32 latent -> bf16 rows [B * T][C] (the permute of denoiser.py:160 + the operand rounding), T = 32 --------------------------
// A block takes 64 channels of one clip: 64 x 32 floats contiguous in, 32 row segments of 128 B out, transposed through the LDS.
__global__ __launch_bounds__(256) void k_bct_to_rows_bf16(const float* __restrict__ x, int C, __bf16* __restrict__ out) {
    __shared__ float tile[64][33];
    const int b = blockIdx.y, c0 = blockIdx.x * 64, tid = threadIdx.x;
    const float* src = x + ((size_t)b * C + c0) * 32;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = (p * 256 + tid) * 4, c = e >> 5, t = e & 31;
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + e);
        tile[c][t] = v[0]; tile[c][t + 1] = v[1]; tile[c][t + 2] = v[2]; tile[c][t + 3] = v[3];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = p * 256 + tid, t = e >> 4, c = (e & 15) * 4;                 // 32 rows x 16 quads
        bf16x4 o;
        o[0] = (__bf16)tile[c][t]; o[1] = (__bf16)tile[c + 1][t]; o[2] = (__bf16)tile[c + 2][t]; o[3] = (__bf16)tile[c + 3][t];
        *reinterpret_cast<bf16x4*>(out + ((size_t)b * 32 + t) * C + c0 + c) = o;
    }
}

// ---- out[g][c] = sum over the `group` rows of group g of src[row][c] (rows of pitch ld), in row order: the gradient of a per-clip vector that the
// forward broadcast over the clip's frames, read out of a column slice of the input stage's data gradient --------------------------------------
__global__ __launch_bounds__(256) void k_rows_group_sum(const float* __restrict__ src, int ld, int width, int group, int n_groups, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_groups * width) return;
    const int g = i / width, c = i - g * width;
    const float* p = src + (size_t)g * group * ld + c;
    float acc = 0.f;
    int r = 0;
    for (; r + 8 <= group; r += 8) {                          // (eight loads in flight: a chain of dependent round trips otherwise)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u) * ld];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; r < group; ++r) acc += p[(size_t)r * ld];
    out[i] = acc;
}

// ---- out[r][0:width] = scale * src[r / row_div][0:width] (fp32, src rows of pitch ld): the backward of an average pool over row_div consecutive rows
// (scale = 1 / row_div) read out of a column slice of a wider data gradient ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_expand(const float* __restrict__ src, int ld, int width, int row_div, float scale, int M, float* __restrict__ out) {
    const int q4 = width / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)M * q4) return;
    const int r = (int)(i / q4), c = (int)(i - (long)r * q4) * 4;
    *reinterpret_cast<f32x4*>(out + (size_t)r * width + c) = *reinterpret_cast<const f32x4*>(src + (size_t)(r / row_div) * ld + c) * scale;
}

// ---- sum of a Linear's per-64-row bias-gradient partial sums (syn_linear_bwd_prep), in row-block order -----------------------------------------
__global__ __launch_bounds__(64) void k_colsum_parts(const float* __restrict__ part, int rows, int n, float* __restrict__ out) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n) return;
    float acc = 0.f;
    int i = 0;
    for (; i + 8 <= rows; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(i + u) * n + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; i < rows; ++i) acc += part[(size_t)i * n + c];
    out[c] = acc;
}

// ---- one read pass over a buffer (a dword per 64-byte line): whatever the memory-side cache has evicted comes back before a latency-bound
// consumer asks for it line by line (the transposed block weights in front of the backward chain) ---------------------------------------------------
__global__ __launch_bounds__(256) void k_touch(const unsigned* __restrict__ p, long lines, unsigned* __restrict__ sink) {
    unsigned acc = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < lines; i += (long)gridDim.x * 256) acc += p[i * 16];
    if (acc == 0x9e3779b9u && sink) *sink = acc;            // (never in practice: keeps the loads)
}

// ---- masked SmoothL1 of training_losses (gaussian_diffusion.py:202-215 `masked_l2`, :1307-1314) ------------------------------------------------------
// loss[b] = sum_{c,t} sl1(out - target) mask[b][t] / (sum_t mask[b][t] * C).  target is (B, C, 1, T) as the reference lays it out; `out` / `dout`
// either the same, or (rows = 1) the output Linear's own [B][T][C] rows - what `out.permute(0, 2, 1).unsqueeze(2)` is a view of, so that neither the
// forward nor the backward has to materialise the permuted tensor.  A block takes 64 channels of one clip (the target tile transposed through the
// LDS for the rows layout); the per-block partial sums are added in block order by k_sl1_final; the gradient is a pass of its own in the backward
// with the upstream per-sample factor folded in (the forward neither writes nor keeps it).
template <bool GRAD>
__global__ __launch_bounds__(256) void k_sl1_tiles(const float* __restrict__ target, const float* __restrict__ out, const unsigned char* __restrict__ mask,
                                                   int C, int T, int rows, const float* __restrict__ gscale, float* __restrict__ part, float* __restrict__ dout) {
    __shared__ float tt[64][65];
    __shared__ float msk[64];
    __shared__ float red[256];
    const int b = blockIdx.y, c0 = blockIdx.x * 64, tid = threadIdx.x;
    if (tid < T) msk[tid] = mask[(size_t)b * T + tid] ? 1.f : 0.f;
    const float* tg = target + ((size_t)b * C + c0) * T;
    for (int e = tid; e < 64 * T; e += 256) tt[e / T][e % T] = tg[e];
    __syncthreads();
    float inv = 0.f;
    if constexpr (GRAD) {
        float cnt = 0.f;
        for (int t = 0; t < T; ++t) cnt += msk[t];
        inv = (gscale ? gscale[b] : 1.0f) / (cnt * (float)C);
    }
    float acc = 0.f;
    for (int e = tid; e < 64 * T; e += 256) {
        int c, t;
        size_t at;
        if (rows) { t = e >> 6; c = e & 63; at = ((size_t)b * T + t) * C + c0 + c; }
        else { c = e / T; t = e % T; at = ((size_t)b * C + c0 + c) * T + t; }
        const float d = out[at] - tt[c][t], ad = fabsf(d), m = msk[t];
        if constexpr (GRAD) dout[at] = (ad < 1.f ? d : (d > 0.f ? 1.f : -1.f)) * m * inv;
        else acc += (ad < 1.f ? 0.5f * d * d : ad - 0.5f) * m;
    }
    if constexpr (!GRAD) {
        red[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = red[0];
    }
}
// poison: NULL, or a device flag that turns every loss into NaN while it is nonzero (the persistent block kernels' barrier-timeout flag: a step whose
// activations may be wrong must not look like a step).
__global__ __launch_bounds__(256) void k_sl1_final(const float* __restrict__ part, const unsigned char* __restrict__ mask, int B, int chunks, int C, int T,
                                                   const int* __restrict__ poison, float* __restrict__ loss) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float acc = 0.f, cnt = 0.f;
    for (int i = 0; i < chunks; ++i) acc += part[(size_t)b * chunks + i];
    for (int t = 0; t < T; ++t) cnt += mask[(size_t)b * T + t] ? 1.f : 0.f;
    loss[b] = (poison && *poison) ? __builtin_nanf("") : acc / (cnt * (float)C);
}

// ---- gradient of an nn.Embedding table (models/denoiser.py:72 text_pre_encoder_body, 11 195 x 300) --------------------------------------------------
// dW[v] = sum over the positions whose id is v of dy[position], positions in increasing order: no atomics on the result, no sort (PyTorch-ROCm's
// embedding_dense_backward is a chain of ~15 sort / scan / segment kernels, and the one op of the step that does not survive being replayed from
// a hipGraph).  Every row of dW is written by this ONE launch: a block first zeroes its slice of the rows no id names (a bitmap of the ids in LDS) -
// not a memset node in front: inside the captured training step a 13 MB hipMemsetAsync node was not reliably ordered against this kernel on replay
// (rows came back zeroed after the kernel had run, or not zeroed at all; scripts/diag_ddp_determinism.py) - then a wave takes one position p: if an
// EARLIER position carries the same id the wave retires (that position's wave owns the row), else it walks the later positions with a ballot per 64
// and adds the matching rows of dy in position order.
// (The first version gave every 16 table rows a block that scanned all the ids: 700 blocks x 4096 ids, 52 us; this one 17 us.)
constexpr int kEmbMaxPos = 8192, kEmbWaves = 8, kEmbMaxD = 512, kEmbMaxV = 65536;
__global__ __launch_bounds__(kEmbWaves * 64) void k_embedding_wgrad(const long* __restrict__ ids, const float* __restrict__ dy, int ld, int n_pos, int V, int D,
                                                                  float* __restrict__ dw) {
    __shared__ int sid[kEmbMaxPos];
    __shared__ unsigned seen[kEmbMaxV / 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < (V + 31) / 32; i += kEmbWaves * 64) seen[i] = 0u;
    for (int i = tid; i < n_pos; i += kEmbWaves * 64) sid[i] = (int)ids[i];
    __syncthreads();
    for (int i = tid; i < n_pos; i += kEmbWaves * 64) {
        const int v = sid[i];
        if (v >= 0 && v < V) atomicOr(&seen[v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    {   // this block's slice of the table: rows nobody names are zero
        const int per = (V + (int)gridDim.x - 1) / (int)gridDim.x, r0 = (int)blockIdx.x * per, r1 = min(V, r0 + per);
        for (int r = r0 + wave; r < r1; r += kEmbWaves) {
            if (seen[r >> 5] >> (r & 31) & 1u) continue;
            for (int f = lane; f < D; f += 64) dw[(size_t)r * D + f] = 0.f;
        }
    }
    const int p = blockIdx.x * kEmbWaves + wave;
    if (p >= n_pos) return;
    const int v = sid[p];
    if (v < 0 || v >= V) return;
    for (int base = 0; base < p; base += 64) {
        const int j = base + lane;
        if (__ballot(j < p && sid[j] == v)) return;                  // an earlier position owns this row
    }
    float acc[kEmbMaxD / 64];
#pragma unroll
    for (int e = 0; e < kEmbMaxD / 64; ++e) acc[e] = 0.f;
    for (int base = p & ~63; base < n_pos; base += 64) {
        const int j = base + lane;
        unsigned long long hit = __ballot(j >= p && j < n_pos && sid[j] == v);
        while (hit) {
            const int q = base + __builtin_ctzll(hit);
            hit &= hit - 1;
            const float* row = dy + (size_t)q * ld;
#pragma unroll
            for (int e = 0; e < kEmbMaxD / 64; ++e)
                if (lane + 64 * e < D) acc[e] += row[lane + 64 * e];
        }
    }
#pragma unroll
    for (int e = 0; e < kEmbMaxD / 64; ++e)
        if (lane + 64 * e < D) dw[(size_t)v * D + lane + 64 * e] = acc[e];
}

}  // namespace glu
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int syn_masked_smooth_l1(const float* target, const float* out, const uint8_t* mask, int32_t batch, int32_t channels, int32_t t_len, int32_t out_rows,
                         float* part, const int32_t* poison_flag, float* loss, void* stream) {
    if (!target || !out || !mask || !loss || !part || batch <= 0 || channels <= 0 || channels % 64 || t_len <= 0 || t_len > 64)
        return fail_msg("syn_masked_smooth_l1: channels must be a multiple of 64, t_len <= 64, part [batch][channels / 64]");
    const int chunks = channels / 64;
    hipLaunchKernelGGL(glu::k_sl1_tiles<false>, dim3(chunks, batch), dim3(256), 0, (hipStream_t)stream, target, out, mask, channels, t_len, out_rows,
                       (const float*)nullptr, part, (float*)nullptr);
    hipLaunchKernelGGL(glu::k_sl1_final, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, mask, batch, chunks, channels, t_len, poison_flag, loss);
    return launched("k_sl1_tiles launch");
}

int syn_masked_smooth_l1_grad(const float* target, const float* out, const uint8_t* mask, int32_t batch, int32_t channels, int32_t t_len, int32_t out_rows,
                              const float* sample_scale, float* dout, void* stream) {
    if (!target || !out || !mask || !dout || batch <= 0 || channels <= 0 || channels % 64 || t_len <= 0 || t_len > 64)
        return fail_msg("syn_masked_smooth_l1_grad: channels must be a multiple of 64, t_len <= 64");
    hipLaunchKernelGGL(glu::k_sl1_tiles<true>, dim3(channels / 64, batch), dim3(256), 0, (hipStream_t)stream, target, out, mask, channels, t_len, out_rows,
                       sample_scale, (float*)nullptr, dout);
    return launched("k_sl1_tiles (gradient) launch");
}

int syn_rows_concat_bf16(const syn_concat_src* srcs, int32_t n_src, int32_t m_rows, int32_t out_ld, void* out_bf16, void* stream) {
    if (!srcs || n_src < 1 || n_src > SYN_CONCAT_MAX || m_rows <= 0 || out_ld <= 0 || out_ld % 4 || !out_bf16) return fail_msg("syn_rows_concat_bf16: 1 .. 4 sources, out_ld % 4 == 0");
    glu::CatArgs a;
    memset(&a, 0, sizeof(a));
    int total = 0;
    for (int i = 0; i < n_src; ++i) {
        const syn_concat_src& c = srcs[i];
        if (!c.p || c.width <= 0 || c.width % 4 || c.ld % 4 || c.ld < c.width || c.row_div < 1 || c.pool < 1 || (c.pool > 1 && (c.row_div != 1 || c.p2)))
            return fail_msg("syn_rows_concat_bf16: a source needs width % 4 == 0, ld % 4 == 0, ld >= width, row_div >= 1, pool >= 1 (a pooled source: row_div 1, no addend)");
        a.s[i].p = c.p; a.s[i].p2 = c.p2; a.s[i].width = c.width; a.s[i].ld = c.ld; a.s[i].row_div = c.row_div; a.s[i].pool = c.pool;
        total += c.width;
    }
    if (total > out_ld) return fail_msg("syn_rows_concat_bf16: the sources are wider than out_ld");
    a.n_src = n_src; a.M = m_rows; a.out_ld = out_ld; a.out = (__bf16*)out_bf16;
    const long n = (long)m_rows * (out_ld / 4);
    hipLaunchKernelGGL(glu::k_rows_concat_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched("k_rows_concat_bf16 launch");
}

int syn_embed_rows_bf16(const int64_t* ids, const float* table, int32_t vocab, int32_t dim, int32_t m_rows, int32_t out_ld, void* out_bf16, void* stream) {
    if (!ids || !table || !out_bf16 || vocab <= 0 || dim <= 0 || dim % 4 || m_rows <= 0 || out_ld < dim || out_ld % 4) return fail_msg("syn_embed_rows_bf16: dim % 4 == 0, out_ld >= dim, out_ld % 4 == 0");
    const long n = (long)m_rows * (out_ld / 4);
    hipLaunchKernelGGL(glu::k_embed_rows_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long*>(ids), table, vocab,
                       dim, m_rows, out_ld, (__bf16*)out_bf16);
    return launched("k_embed_rows_bf16 launch");
}

int syn_bct_to_rows_bf16(const float* x_bct, int32_t n_clips, int32_t channels, int32_t t_len, void* out_bf16, void* stream) {
    if (!x_bct || !out_bf16 || n_clips <= 0 || channels <= 0 || channels % 64 || t_len != 32) return fail_msg("syn_bct_to_rows_bf16: channels % 64 == 0, t_len == 32");
    hipLaunchKernelGGL(glu::k_bct_to_rows_bf16, dim3(channels / 64, n_clips), dim3(256), 0, (hipStream_t)stream, x_bct, channels, (__bf16*)out_bf16);
    return launched("k_bct_to_rows_bf16 launch");
}

int syn_rows_group_sum(const float* src, int32_t ld, int32_t width, int32_t group, int32_t n_groups, float* out, void* stream) {
    if (!src || !out || ld < width || width <= 0 || group <= 0 || n_groups <= 0) return fail_msg("syn_rows_group_sum: bad arguments");
    hipLaunchKernelGGL(glu::k_rows_group_sum, dim3((n_groups * width + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, ld, width, group, n_groups, out);
    return launched("k_rows_group_sum launch");
}

int syn_rows_expand(const float* src, int32_t ld, int32_t width, int32_t row_div, float scale, int32_t m_rows, float* out, void* stream) {
    if (!src || !out || width <= 0 || width % 4 || ld < width || ld % 4 || row_div < 1 || m_rows <= 0) return fail_msg("syn_rows_expand: width % 4 == 0, ld >= width, ld % 4 == 0, row_div >= 1");
    const long n = (long)m_rows * (width / 4);
    hipLaunchKernelGGL(glu::k_rows_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, ld, width, row_div, scale, m_rows, out);
    return launched("k_rows_expand launch");
}

int syn_colsum_parts(const float* part, int32_t rows, int32_t n, float* out, void* stream) {
    if (!part || !out || rows <= 0 || n <= 0) return fail_msg("syn_colsum_parts: bad arguments");
    hipLaunchKernelGGL(glu::k_colsum_parts, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, part, rows, n, out);
    return launched("k_colsum_parts launch");
}

int syn_touch(const void* p, int64_t bytes, void* stream) {
    if (!p || bytes < 64) return fail_msg("syn_touch: at least one 64-byte line");
    const long lines = bytes / 64;
    const long blocks = (lines + 255) / 256;
    hipLaunchKernelGGL(glu::k_touch, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)p, lines, (unsigned*)nullptr);
    return launched("k_touch launch");
}

int syn_embedding_wgrad(const int64_t* ids, const float* dy, int32_t ld, int32_t n_pos, int32_t vocab, int32_t dim, float* dw, void* stream) {
    if (!ids || !dy || !dw || n_pos <= 0 || n_pos > glu::kEmbMaxPos || vocab <= 0 || vocab > glu::kEmbMaxV || dim <= 0 || dim > glu::kEmbMaxD || ld < dim)
        return fail_msg("syn_embedding_wgrad: bad arguments (at most 8192 positions per call, vocab <= 65536, dim <= 512, ld >= dim)");
    hipLaunchKernelGGL(glu::k_embedding_wgrad, dim3((n_pos + glu::kEmbWaves - 1) / glu::kEmbWaves), dim3(glu::kEmbWaves * 64), 0, (hipStream_t)stream,
                       reinterpret_cast<const long*>(ids), dy, ld, n_pos, vocab, dim, dw);
    return launched("k_embedding_wgrad launch");
}

}  // extern "C"
