// syn_cond.inc — per-clip conditioning behind the audio encoder (SURVEY 8 f1; models/denoiser.py:147-157, 160-174):
//   word embedding gather -> Linear 300->256, concat with the audio features -> Linear 512->256 (mix_audio_text),
//   avg_pool1d(4), . W2c^T, plus embed_text(seed) . W2a^T [+ style . W3s^T] + every bias
// = the additive tensor `cond` [clip][32][512] of the step kernels, once per clip.  Everything between the audio features
// and `cond` is affine, so the host folds it (fp64, conditioning.py:CondWeights) into
//   cond[b][f][n] = sum_k pool4(audio)[b][f][k] GT[k][n] + 1/4 sum_{i<4} TW[word[b][4f+i]][n] + d[b][n]
//   d[b][n]       = sum_k seed[b][k] ST[k][n] (+ sum_k style[b][k] ST[6144 + k][n]) + c0[n]
// with GT = (W2c Wm_a)^T (256 x 512), TW = word_embedding (W2c Wm_w Wt)^T (vocabulary x 512: the whole word path is a
// table lookup), ST = [W2a W_embed_text | W3s]^T.  fp32 FMA kernels (15 MFLOP per clip; the result feeds every step, so it
// keeps fp32), weights read coalesced along n, activations broadcast from LDS.
namespace {
namespace cnd {

// d[b][n] as kClipSplit partial sums over K: 32 clips x 64 features x one K share per workgroup (a thread = one feature x 8 clips:
// eight FMAs per weight it reads), K streamed in chunks of 64 through LDS.  Round 2 ran the whole K = 6144 in one workgroup per
// 16 clips x 64 features - 128 workgroups, 96 dependent chunk loads each, 535 us per 256 clips, a third of the per-clip conditioning
// time; the K split fills the chip.  The partial sums are added in a fixed order by k_cond_frames (no atomics: bitwise reproducible).
constexpr int kClipSplit = 8;
__global__ __launch_bounds__(256) void k_cond_clip(const float* __restrict__ seed, int k1, const float* __restrict__ style, int k2,
                                                   const float* __restrict__ ST, int n_clips, float* __restrict__ dpart /*[kClipSplit][n_clips][512]*/) {
    __shared__ float xs[32][65];
    const int tid = threadIdx.x, n = blockIdx.x * 64 + (tid & 63), cg = tid >> 6, b0 = blockIdx.y * 32;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int K = k1 + k2, chunks = (K + 63) / 64, per = (chunks + kClipSplit - 1) / kClipSplit;
    const int c_lo = blockIdx.z * per, c_hi = min(chunks, c_lo + per);
    for (int ch = c_lo; ch < c_hi; ++ch) {
        const int kb = ch * 64;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + i * 256, r = idx >> 6, c = idx & 63, k = kb + c, b = b0 + r;
            float v = 0.f;
            if (b < n_clips && k < K) v = k < k1 ? seed[(size_t)b * k1 + k] : style[(size_t)b * k2 + (k - k1)];
            xs[r][c] = v;
        }
        __syncthreads();
        const int kn = min(64, K - kb);
#pragma unroll 4
        for (int c = 0; c < kn; ++c) {
            const float w = ST[(size_t)(kb + c) * SYN_D + n];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(xs[cg * 8 + j][c], w, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = b0 + cg * 8 + j;
        if (b < n_clips) dpart[((size_t)blockIdx.z * n_clips + b) * SYN_D + n] = acc[j];
    }
}

// cond[b][f][n]: one clip x 128 features per workgroup; the pooled audio features (32 x 256) live in LDS
__global__ __launch_bounds__(256) void k_cond_frames(const float* __restrict__ audio /*[B][128][256]*/, const long long* __restrict__ word /*[B][128]*/,
                                                     const float* __restrict__ GT, const float* __restrict__ TW, int vocab,
                                                     const float* __restrict__ dpart, const float* __restrict__ c0, int n_clips,
                                                     float* __restrict__ cond) {
    __shared__ float ap[32][256];
    __shared__ int wd[128];
    const int tid = threadIdx.x, b = blockIdx.y, n = blockIdx.x * 128 + (tid & 127), fg = tid >> 7;
    const float* a = audio + (size_t)b * 128 * 256;
    for (int i = tid; i < 32 * 256; i += 256) {
        const int f = i >> 8, k = i & 255;
        ap[f][k] = 0.25f * ((a[(4 * f) * 256 + k] + a[(4 * f + 1) * 256 + k]) + (a[(4 * f + 2) * 256 + k] + a[(4 * f + 3) * 256 + k]));
    }
    if (tid < 128) {
        const long long w = word[(size_t)b * 128 + tid];
        wd[tid] = (int)(w < 0 ? 0 : (w >= vocab ? vocab - 1 : w));
    }
    __syncthreads();
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int k = 0; k < 256; ++k) {
        const float g = GT[(size_t)k * SYN_D + n];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(ap[fg * 16 + j][k], g, acc[j]);
    }
    float dn = c0[n];                                               // + the clip's seed / style term: K shares in order
#pragma unroll
    for (int z = 0; z < kClipSplit; ++z) dn += dpart[((size_t)z * n_clips + b) * SYN_D + n];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int f = fg * 16 + j;
        const float t = (TW[(size_t)wd[4 * f] * SYN_D + n] + TW[(size_t)wd[4 * f + 1] * SYN_D + n]) +
                        (TW[(size_t)wd[4 * f + 2] * SYN_D + n] + TW[(size_t)wd[4 * f + 3] * SYN_D + n]);
        cond[((size_t)b * 32 + f) * SYN_D + n] = acc[j] + 0.25f * t + dn;
    }
}

}  // namespace cnd
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int syn_cond_encode(const syn_cond_weights* w, const float* audio_feat, const int64_t* word, const float* seed, const float* style,
                    int32_t n_clips, float* d_scratch, float* cond, void* stream) {
    if (!w || !w->gt || !w->tw || !w->st || !w->c0 || !audio_feat || !word || !seed || !d_scratch || !cond || n_clips <= 0)
        return fail_msg("syn_cond_encode: null argument");
    if (w->seed_dim <= 0 || w->style_dim < 0 || w->vocab <= 0 || (w->style_dim > 0 && !style))
        return fail_msg("syn_cond_encode: bad dimensions (a model with a style projection needs the style vectors)");
    hipStream_t s = (hipStream_t)stream;
    static_assert(cnd::kClipSplit == SYN_COND_SCRATCH_ROWS, "include/syn_hip.h: d_scratch rows per clip");
    hipLaunchKernelGGL(cnd::k_cond_clip, dim3(SYN_D / 64, (n_clips + 31) / 32, cnd::kClipSplit), dim3(256), 0, s, seed, w->seed_dim, style,
                       w->style_dim, w->st, n_clips, d_scratch);
    hipLaunchKernelGGL(cnd::k_cond_frames, dim3(SYN_D / 128, n_clips), dim3(256), 0, s, audio_feat, (const long long*)word, w->gt, w->tw,
                       w->vocab, d_scratch, w->c0, n_clips, cond);
    return launched("syn_cond_encode");
}

}  // extern "C"
