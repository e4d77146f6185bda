// The FGD motion embedder, VAESKConv.map2latent = LocalEncoder (models/motion_encoder.py:698-787): four SkeletonResidual layers
// (models/utils/skeleton.py:547-586) over the SMPL-X edge graph (DESIGN.md §12).
// One GEMM per layer covers both branches: output frame t reads the window x[2t-1 .. 2t+2] (zero outside the take), the main conv all
// four taps, the shortcut tap 1 (x[2t]).  Columns 0 .. cout_p are the main conv's channels, cout_p .. 2 cout_p the shortcut's; rows are
// k = tap * cin_p + c.  The masked weights are packed per 16-column tile as the chunks of 4 rows that hold a nonzero of W*M only, and a
// workgroup (one clip, 16 output frames) loops over those on v_mfma_f32_16x16x4_f32 (fp32 operands, exact fp32 products).
// GroupNorm needs the whole take: layer i writes its pre-norm r | s and, per 16-frame tile and group, the fp64 sum and sum of squares;
// layer i + 1 reduces those in tile order, then applies the affine, the shortcut add, the pooling and tanh while staging its window.
// k_skel_out does the same for the last layer and writes the embedding.  No atomics: bitwise reproducible, clips independent.
namespace {
namespace skel {

constexpr int kTile = 16;                        // output frames per workgroup (the MFMA's M)
constexpr int kWin = 2 * kTile + 2;              // input frames a tile reads
constexpr int kBatch = 8;                        // kept chunks whose fragments are loaded together
constexpr int kGroups = 10, kPoolMax = SYN_SKEL_POOL_MAX, kMaxC = SYN_SKEL_MAX_C;
constexpr double kEps = 1e-5;

// what the consumer of a layer's output needs to turn r | s into the next layer's input: tanh(P (GroupNorm(r) + s))
struct Src {
    const float* y;              // pre-norm r | s [clips][t][2 cout_p]
    const double* st;            // partial sums [clips][tiles][10][2]
    const float* gn_g; const float* gn_b;
    const int32_t* pool_src; const float* pool_w;
    int cout, cout_p, t, tiles, width;
};

struct ConvArgs {
    const float* x;              // layer 0: the input [clips][t_in][cin]
    Src in;                      // later layers: the previous layer's output
    int cin, cin_p, stride, t_in, t_out, tiles;
    const float* w; const int32_t* chunk_off; const int32_t* chunk_k; const float* bias;
    int cout, cout_p, n_ctiles;
    float* y; double* st;
};

struct Norm {                    // LDS: the GroupNorm of the source layer, per channel
    float mean[kMaxC], scale[kMaxC], beta[kMaxC];
    double g[2 * kGroups];
};

// GroupNorm statistics of clip b of `s`, reduced over its tiles in order (every workgroup of the clip computes the same values)
__device__ void norm_prepare(const Src& s, int b, Norm& n) {
    const int tid = threadIdx.x;
    if (tid < 2 * kGroups) {
        const double* p = s.st + (long)b * s.tiles * 2 * kGroups + tid;
        double acc = 0.0;
        for (int k = 0; k < s.tiles; ++k) acc += p[(long)k * 2 * kGroups];
        n.g[tid] = acc;
    }
    __syncthreads();
    const int gs = s.cout / kGroups;
    const double cnt = (double)gs * s.t;
    for (int j = tid; j < s.cout; j += blockDim.x) {
        const int g = j / gs;
        const double mean = n.g[2 * g] / cnt;
        double var = n.g[2 * g + 1] / cnt - mean * mean;
        var = var > 0.0 ? var : 0.0;
        n.mean[j] = (float)mean;
        n.scale[j] = (float)(1.0 / sqrt(var + kEps)) * s.gn_g[j];
        n.beta[j] = s.gn_b[j];
    }
    __syncthreads();
}

// channel c of the source layer's output at frame t of clip b: tanh(sum_k w_k (GroupNorm(r)[j_k] + s[j_k]))
__device__ __forceinline__ float src_value(const Src& s, const Norm& n, int b, int t, int c) {
    const float* row = s.y + ((long)b * s.t + t) * 2 * s.cout_p;
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < kPoolMax; ++k) {
        const int j = s.pool_src[c * kPoolMax + k];
        if (j < 0 || j >= s.cout) continue;
        v += s.pool_w[c * kPoolMax + k] * ((row[j] - n.mean[j]) * n.scale[j] + n.beta[j] + row[s.cout_p + j]);
    }
    return tanhf(v);
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_skel_conv(const ConvArgs a) {
    extern __shared__ float s_win[];                           // [kWin][a.stride]
    __shared__ Norm s_norm;
    __shared__ double s_csum[kMaxC], s_csq[kMaxC];             // per r column of this tile: sum, sum of squares over its frames
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int t0 = tile * kTile;
    if (!FIRST) norm_prepare(a.in, b, s_norm);
    for (int e = tid; e < kWin * a.cin_p; e += 256) {
        const int f = e / a.cin_p, c = e - f * a.cin_p;
        const int t = 2 * t0 - 1 + f;
        float v = 0.f;
        if (t >= 0 && t < a.t_in && c < a.cin) v = FIRST ? a.x[((long)b * a.t_in + t) * a.cin + c] : src_value(a.in, s_norm, b, t, c);
        s_win[f * a.stride + c] = v;
    }
    __syncthreads();
    // A operand of lane l: output frame t0 + (l & 15), row 4 chunk + (l >> 4) = window frame 2 (l & 15) + tap, channel c0 + (l >> 4)
    const int arow = 2 * (lane & 15) * a.stride + (lane >> 4);
    const int ldy = 2 * a.cout_p;
    for (int nt = wave; nt < a.n_ctiles; nt += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int q1 = a.chunk_off[nt + 1];
        int q = a.chunk_off[nt];
        for (; q + kBatch <= q1; q += kBatch) {               // kBatch independent fragment loads in flight, then their MFMAs in order
            float av[kBatch], bv[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int ck = a.chunk_k[q + u];
                const int tap = ck >> 16, c0 = ck & 0xffff;
                av[u] = (tap < 4 && c0 + 4 <= a.cin_p) ? s_win[arow + tap * a.stride + c0] : 0.f;
                bv[u] = a.w[(long)(q + u) * 64 + lane];
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
        }
        for (; q < q1; ++q) {
            const int ck = a.chunk_k[q];
            const int tap = ck >> 16, c0 = ck & 0xffff;
            const float av = (tap < 4 && c0 + 4 <= a.cin_p) ? s_win[arow + tap * a.stride + c0] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, a.w[(long)q * 64 + lane], acc, 0, 0, 0);
        }
        // D: row (l >> 4) * 4 + e, column l & 15
        const int col = nt * kTile + (lane & 15);
        const float bias = a.bias[col];
        double cs = 0.0, cq = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = t0 + (lane >> 4) * 4 + e;
            if (t < a.t_out) {
                const float v = acc[e] + bias;
                a.y[((long)b * a.t_out + t) * ldy + col] = v;
                cs += v;
                cq += (double)v * v;
            }
        }
        cs += __shfl_xor(cs, 16);
        cq += __shfl_xor(cq, 16);
        cs += __shfl_xor(cs, 32);
        cq += __shfl_xor(cq, 32);
        if (lane < 16 && col < a.cout) {
            s_csum[col] = cs;
            s_csq[col] = cq;
        }
    }
    __syncthreads();
    if (tid < 2 * kGroups) {
        const int g = tid >> 1, gs = a.cout / kGroups;
        const double* src = (tid & 1) ? s_csq : s_csum;
        double acc = 0.0;
        for (int c = g * gs; c < (g + 1) * gs; ++c) acc += src[c];
        a.st[((long)b * a.tiles + tile) * 2 * kGroups + tid] = acc;
    }
}

// the last layer's output: out [clips][t][width]
__global__ __launch_bounds__(256) void k_skel_out(const Src s, int tiles, float* __restrict__ out) {
    __shared__ Norm s_norm;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    norm_prepare(s, b, s_norm);
    for (int e = threadIdx.x; e < kTile * s.width; e += 256) {
        const int i = e / s.width, c = e - i * s.width;
        const int t = tile * kTile + i;
        if (t < s.t) out[((long)b * s.t + t) * s.width + c] = src_value(s, s_norm, b, t, c);
    }
}

// one workgroup of 64 per 16-column tile: its kept chunks, lane l = B[row 4 chunk + (l >> 4)][column 16 tile + (l & 15)]
__global__ __launch_bounds__(64) void k_skel_pack(const float* __restrict__ w, const float* __restrict__ mask, const float* __restrict__ ws,
                                                  const float* __restrict__ ms, int cout, int cin, int cout_p, const int32_t* __restrict__ chunk_off,
                                                  const int32_t* __restrict__ chunk_k, float* __restrict__ out) {
    const int nt = blockIdx.x, lane = threadIdx.x;
    const int n = nt * kTile + (lane & 15);
    for (int q = chunk_off[nt]; q < chunk_off[nt + 1]; ++q) {
        const int ck = chunk_k[q];
        const int tap = ck >> 16, c = (ck & 0xffff) + (lane >> 4);
        float v = 0.f;
        if (n < cout_p) {
            if (n < cout && c < cin && tap < 4) {
                const long i = ((long)n * cin + c) * 4 + tap;
                v = w[i] * mask[i];
            }
        } else if (n - cout_p < cout && c < cin && tap == 1) {
            const long i = (long)(n - cout_p) * cin + c;
            v = ws[i] * ms[i];
        }
        out[(long)q * 64 + lane] = v;
    }
}

static inline long round_up(long v, long m) { return (v + m - 1) / m * m; }
static inline int cin_pad(int cin) { return (int)round_up(cin, 4); }
static inline int lds_stride(int cin_p) { return cin_p + (int)((34 - cin_p % 32) % 32); }     // = 2 mod 32: the 16 x 4 A reads hit 64 banks

}  // namespace skel
}  // namespace

extern "C" {

int syn_skel_pack_weight(const float* w, const float* mask, const float* ws, const float* ms, int32_t cout, int32_t cin, const int32_t* chunk_off,
                         const int32_t* chunk_k, float* out, void* stream) {
    if (!w || !mask || !ws || !ms || !chunk_off || !chunk_k || !out || cout < 1 || cout > skel::kMaxC || cin < 1 || cin > skel::kMaxC)
        return fail_msg("syn_skel_pack_weight: null pointer, or channels outside 1 .. SYN_SKEL_MAX_C");
    const int cout_p = (int)skel::round_up(cout, skel::kTile);
    hipLaunchKernelGGL(skel::k_skel_pack, dim3((unsigned)(2 * cout_p / skel::kTile)), dim3(64), 0, (hipStream_t)stream, w, mask, ws, ms, (int)cout, (int)cin,
                       cout_p, chunk_off, chunk_k, out);
    return launched("k_skel_pack launch");
}

int syn_skel_encode(const syn_skel_model* m, const float* x, int32_t n_clips, int32_t n_frames, void* workspace, float* out, void* stream) {
    using namespace skel;
    if (!m || !x || !workspace || !out) return fail_msg("syn_skel_encode: null pointer");
    if (n_clips < 1 || n_clips > SYN_SKEL_MAX_CLIPS || n_frames < 16 || n_frames % 16 || n_frames > (1 << 24))
        return fail_msg("syn_skel_encode: n_clips outside 1 .. SYN_SKEL_MAX_CLIPS or n_frames not a positive multiple of 16 (at most 2^24)");
    for (int l = 0; l < SYN_SKEL_LAYERS; ++l) {
        const syn_skel_layer& y = m->layer[l];
        if (!y.w || !y.chunk_off || !y.chunk_k || !y.bias || !y.gn_g || !y.gn_b || !y.pool_src || !y.pool_w)
            return fail_msg("syn_skel_encode: model layer with a null pointer");
        if (y.cin < 1 || y.cin > kMaxC || y.cout < kGroups || y.cout > kMaxC || y.cout % kGroups || y.out_width < 1 || y.out_width > kMaxC ||
            (l > 0 && y.cin != m->layer[l - 1].out_width))
            return fail_msg("syn_skel_encode: layer widths outside 1 .. SYN_SKEL_MAX_C, a GroupNorm width not a multiple of 10, or a layer whose "
                            "input is not the previous layer's output");
    }
    if ((long)n_clips * ((n_frames / 2 + kTile - 1) / kTile) > (1L << 24)) return fail_msg("syn_skel_encode: too many clip x frame tiles");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;                                // layout: syn_skel_encode's comment in the header (evaluator.workspace_bytes)
    Src src = {};
    for (int l = 0; l < SYN_SKEL_LAYERS; ++l) {
        const syn_skel_layer& y = m->layer[l];
        ConvArgs a = {};
        a.x = x;
        a.in = src;
        a.cin = y.cin; a.cin_p = cin_pad(y.cin); a.stride = lds_stride(a.cin_p);
        a.t_in = n_frames >> l; a.t_out = n_frames >> (l + 1); a.tiles = (a.t_out + kTile - 1) / kTile;
        a.w = y.w; a.chunk_off = y.chunk_off; a.chunk_k = y.chunk_k; a.bias = y.bias;
        a.cout = y.cout; a.cout_p = (int)round_up(y.cout, kTile); a.n_ctiles = 2 * a.cout_p / kTile;
        a.y = (float*)ws;    ws += round_up((long)n_clips * a.t_out * 2 * a.cout_p * 4, 256);
        a.st = (double*)ws;  ws += round_up((long)n_clips * a.tiles * 2 * kGroups * 8, 256);
        const size_t lds = (size_t)kWin * a.stride * sizeof(float);
        const dim3 grid((unsigned)((long)n_clips * a.tiles));
        if (l == 0) hipLaunchKernelGGL(k_skel_conv<true>, grid, dim3(256), lds, st, a);
        else        hipLaunchKernelGGL(k_skel_conv<false>, grid, dim3(256), lds, st, a);
        if (int rc = launched("k_skel_conv launch")) return rc;
        src.y = a.y; src.st = a.st; src.gn_g = y.gn_g; src.gn_b = y.gn_b; src.pool_src = y.pool_src; src.pool_w = y.pool_w;
        src.cout = a.cout; src.cout_p = a.cout_p; src.t = a.t_out; src.tiles = a.tiles; src.width = y.out_width;
    }
    hipLaunchKernelGGL(k_skel_out, dim3((unsigned)((long)n_clips * src.tiles)), dim3(256), 0, st, src, src.tiles, out);
    return launched("k_skel_out launch");
}

}  // extern "C"
