// syn_conv_train.inc — host side of the WavEncoder's convolutions in TRAINING mode (syn_conv1d_*): the launch of every kernel instance and the
// entry points.  No kernels of its own: it launches wav:: kernels (syn_wavenc.inc) and the weight packs of syn_kernels.hip, and is included
// behind syn_wavenc.inc and syn_train.inc.
namespace {

// diagnostics (syn_debug_conv_terms): which of the two cross products of the split-operand convolutions are issued (3 = both)
// Default (-1): forward and data gradient issue both cross products (fp32-grade: the forward activations feed batch statistics, and rounding them to bf16
// moved the first blocks' gradients by 14 %, DESIGN.md); the WEIGHT gradient drops the dy_hi . x_lo product, i.e. reads x rounded to bf16 - a sum over
// 10^4 - 10^5 positions per element averages that rounding out (r4 A/B, profiles/r04_ab_conv_terms.txt: every gradient within the same error as with
// the third product, -0.08 ms per step).
static int g_conv_terms = -1;
static inline int conv_terms(bool wgrad) { return g_conv_terms >= 0 ? g_conv_terms : (wgrad ? 1 : 3); }

template <int CINP, int KT, int RF>
int launch_conv_train_ks(const wav::TArgs& a0, int n_clips, hipStream_t s) {
    wav::TArgs a = a0; a.terms = conv_terms(false); a.dbg = nullptr;
    constexpr int MW = RF * 16, lds = 2 * (MW + KT - 1) * (CINP * 2 + wav::kTrainPad);
    static_assert(lds <= 160 * 1024, "two bf16 planes of the input tile must fit the LDS");
    static OncePerDevice once;
    if (once.first()) { allow_lds(wav::k_conv_train_ks<CINP, KT, RF>, lds); }
    hipLaunchKernelGGL((wav::k_conv_train_ks<CINP, KT, RF>), dim3((a.L_out + MW - 1) / MW, n_clips), dim3(256), lds, s, a);
    return launched("k_conv_train_ks launch");
}

// n_out: output channels this launch covers (a multiple of the instance's WN x NF x 16 channels per workgroup: grid z)
template <int CINP, int KT, int WN, int WM, int RF, int NF = 4, bool DUAL = false>
int launch_conv_train(const wav::TArgs& a0, int n_clips, hipStream_t s, int n_out = WN * NF * 16) {
    wav::TArgs a = a0; a.terms = conv_terms(false); a.dbg = g_dbg_attn;
    constexpr int MW = WM * RF * 16, lds = 2 * (MW + KT - 1) * (CINP * 2 + wav::kTrainPad), NT = WN * NF * 16;
    static_assert(lds <= 160 * 1024, "two bf16 planes of the input tile must fit the LDS");
    if (n_out % NT) return fail_msg("k_conv_train: the launch's channels are not a multiple of the instance's channel block");
    static OncePerDevice once;
    if (once.first()) { allow_lds(wav::k_conv_train<CINP, KT, WN, WM, RF, NF, DUAL>, lds); }
    hipLaunchKernelGGL((wav::k_conv_train<CINP, KT, WN, WM, RF, NF, DUAL>), dim3((a.L_out + MW - 1) / MW, n_clips, n_out / NT), dim3(WN * WM * 64), lds, s, a);
    return launched("k_conv_train launch");
}

template <int CO_T, int TAPS, bool DUAL = false>
int launch_wgrad_s(const wav::WArgs& a0, hipStream_t s) {
    wav::WArgs a = a0; a.terms = conv_terms(true); a.dbg = g_dbg_attn;
    static_assert(wav::wgrad_s_lds(CO_T) <= 160 * 1024, "dy and x' tiles must fit the LDS");
    static OncePerDevice once;
    if (once.first()) { allow_lds(wav::k_conv_wgrad_s<CO_T, TAPS, DUAL>, wav::wgrad_s_lds(CO_T)); }
    hipLaunchKernelGGL((wav::k_conv_wgrad_s<CO_T, TAPS, DUAL>), dim3(a.cin / wav::kWsJ, a.shares, DUAL ? 1 : a.co_n / CO_T), dim3(512), wav::wgrad_s_lds(CO_T), s, a);
    return launched("k_conv_wgrad_s launch");
}

// The 128- / 256-channel stride-1 layers on 64-channel output tiles (grid z) with 32 input channels per workgroup: the gradient is cut in cout / 64 x cin / 32 slices
// (8 / 32) instead of cin / 32 (4) or cin / 16 (16), so the same number of workgroups needs that many fewer position shares - and every share is a full-size partial
// gradient written here and read back by syn_conv1d_wgrad_sums (r6: 87 MB -> 22 MB per 128-channel layer, 126 -> 31 MB for the 256-channel one; the three launches
// 104 + 49 -> 120 us, the sums 159 -> 137 us per step; 16 input channels per workgroup measured 134 us - the dy fragments are then re-read from the LDS per 24 MFMAs)
constexpr int kWgradWideCb = 2;
// The short 64-channel layers (blocks 1 - 2: 18 chunks per clip) likewise on two slices of 32 input channels (186 -> 93 shares of 245 KB: the three launches 134 -> 103 us);
// block 0's conv2 (105 chunks per clip, dy = 117 MB) stays on one slice: staging its dy tiles twice costs what the smaller partial sums save (166 -> 174 us)
static bool wgrad64_two_slices(int l_out) { return (l_out + wav::kWgP - 1) / wav::kWgP < 50; }
template <int CO_T, int TAPS, int CB>
int launch_wgrad_tiled(const wav::WArgs& a0, hipStream_t s) {
    wav::WArgs a = a0; a.terms = conv_terms(true); a.dbg = g_dbg_attn;
    static OncePerDevice once;
    if (once.first()) { allow_lds(wav::k_conv_wgrad<CO_T, TAPS, CB>, wav::wgrad_lds2(CO_T, CB)); }
    hipLaunchKernelGGL((wav::k_conv_wgrad<CO_T, TAPS, CB>), dim3(a.cin / (16 * CB), a.shares, a.co_n / CO_T), dim3(512), wav::wgrad_lds2(CO_T, CB), s, a);
    return launched("k_conv_wgrad (tiled) launch");
}

template <int CO, int TAPS>
int launch_wgrad(const wav::WArgs& a0, hipStream_t s) {
    wav::WArgs a = a0; a.terms = conv_terms(true); a.dbg = g_dbg_attn;
    static OncePerDevice once;
    constexpr int CB = wav::wgrad_cb(CO);
    if (once.first()) { allow_lds(wav::k_conv_wgrad<CO, TAPS, CB>, wav::wgrad_lds(CO)); }
    hipLaunchKernelGGL((wav::k_conv_wgrad<CO, TAPS, CB>), dim3(a.cin / (16 * CB), a.shares), dim3(512), wav::wgrad_lds(CO), s, a);
    return launched("k_conv_wgrad launch");
}

}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

// output-channel tile of the strided layers' weight gradient (k_conv_wgrad_s<CO_T, TAPS>; conv_train_wgrad_impl launches what this says)
static int wgrad_s_tile(int cout) { return cout >= 64 ? 64 : 0; }   // (128-channel tiles for block 3 meant 3 slices x 85 shares of 590 KB; 64: 6 x 42)

int32_t syn_conv1d_wgrad_shares(int32_t n_clips, int32_t l_out, int32_t cin_rows, int32_t cout) {
    if (n_clips <= 0 || l_out <= 0 || cin_rows < 16 || cout < 64 || cout % 64) return 0;   // (a size query: 0 for a geometry no kernel takes, as the other queries answer)
    const int chunks = n_clips * ((l_out + wav::kWgP - 1) / wav::kWgP);
    const bool strided = cin_rows == 384;                           // (the stride-1 layers have 64 / 128 / 256 row channels)
    // slices of the gradient = workgroups per position share (stride-1 layers: cout = cin; 64 channels: one 64 x 64 slice)
    int blocks = strided ? (cin_rows / wav::kWsJ) * (cout / wgrad_s_tile(cout)) : cin_rows / (16 * wav::wgrad_cb(cin_rows));
    if (!strided && cin_rows >= 128) blocks = (cin_rows / (16 * kWgradWideCb)) * (cin_rows / 64);   // (64-channel output tiles: launch_wgrad_tiled)
    if (!strided && cin_rows == 64 && wgrad64_two_slices(l_out)) blocks = 2;
    if (blocks < 1) return 0;
    int shares = strided ? device_cus() / blocks : (device_cus() + blocks - 1) / blocks;   // one workgroup per CU in total (the partial sums are read back once per share)
    if (shares > chunks) shares = chunks;
    // every share writes a partial sum of the whole gradient block and k_conv_wgrad_sum reads them all back: with few chunks per
    // share that traffic outweighs the parallelism (time ~ chunks / shares x t_chunk + shares x t_partial, t_chunk / t_partial ~ 60)
    // (r5b: 21 -> 60 - the chunk got 1.4 x faster (streamed x rows), the partial sums did not: 608 chunks on 112 shares 57 us, on 155 - 220 shares 47 - 48 us)
    const int balanced = (int)sqrtf(60.f * (float)chunks);
    if (!strided && shares > balanced) shares = balanced;
    return shares < 1 ? 1 : shares;
}

static int conv_train_wgrad_impl(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                                 int32_t cout, const float* in_affine, int32_t in_act, float* ws, float* dw, void* stream) {
    if (!x || !dy || !ws || n_clips <= 0 || l_in <= 0 || cin % 16 || stride < 1) return fail_msg("syn_conv1d_train_wgrad: bad arguments");
    if (in_affine && stride != 1) return fail_msg("syn_conv1d_train_wgrad_norm: the input affine is for the stride-1 layers (conv2 of a block)");
    if (!((stride == 1 && pad == 7) || (pad == 0 && stride * cin == 384 && (stride == 3 || stride == 6))))
        return fail_msg("syn_conv1d_train_wgrad: stride 1 with padding 7, or the encoder's unpadded strided layers (stride x cin = 384)");
    const int l_out = (l_in + 2 * pad - 15) / stride + 1, taps = (15 + stride - 1) / stride, cinp = stride * cin;
    if (l_out <= 0) return fail_msg("syn_conv1d_train_wgrad: input shorter than the kernel");
    wav::WArgs a;
    a.GY = dy; a.gy_clip_stride = (long)l_out * cout; a.L_out = l_out; a.X = x; a.x_clip_stride = (long)l_in * cin; a.x_elems = (long)l_in * cin;
    a.cin = cinp; a.co_n = cout; a.n_clips = n_clips; a.chunks_per_clip = (l_out + wav::kWgP - 1) / wav::kWgP; a.row0 = stride == 1 ? -7 : 0;
    a.shares = syn_conv1d_wgrad_shares(n_clips, l_out, cinp, cout); a.part = ws;
    a.in_aff = in_affine; a.in_act = in_act; a.GY2 = nullptr;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (cout == 64 && taps == 15 && wgrad64_two_slices(l_out)) rc = launch_wgrad_tiled<64, 15, 2>(a, s);
    else if (cout == 64 && taps == 15) rc = launch_wgrad<64, 15>(a, s);
    else if ((cout == 128 || cout == 256) && taps == 15) rc = launch_wgrad_tiled<64, 15, kWgradWideCb>(a, s);
    // the strided layers, read as stride-1 ones over rows of stride * Cin = 384 channels: waves = row channels, not taps
    else if (cout == 64 && taps == 3) rc = launch_wgrad_s<64, 3>(a, s);
    else if (cout == 128 && taps == 3) rc = launch_wgrad_s<64, 3>(a, s);      // (two 64-channel tiles: twice the slices, half the shares)
    else if (cout == 256 && taps == 5) rc = launch_wgrad_s<64, 5>(a, s);     // (128-channel blocks spill: 20 accumulator tiles per wave is the limit)
    else return fail_msg("syn_conv1d_train_wgrad: 64 / 128 / 256 output channels; strided: (64 | 128, stride 6), (256, stride 3)");
    if (rc || !dw) return rc;                                    // (dw NULL: the partial sums only - syn_conv1d_wgrad_sums adds several gradients' up in one launch)
    const int total4 = cout * taps * cinp / 4;                   // (cin % 16 == 0: four consecutive channels share r)
    hipLaunchKernelGGL(wav::k_conv_wgrad_sum, dim3((total4 + 31) / 32), dim3(256), 0, s, (const float*)ws, a.shares, cout, cin, stride, taps, dw);
    return launched("k_conv_wgrad_sum launch");
}

int syn_conv1d_train_wgrad(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                           int32_t cout, float* ws, float* dw, void* stream) {
    return conv_train_wgrad_impl(x, dy, n_clips, l_in, cin, stride, pad, cout, nullptr, 0, ws, dw, stream);
}

int syn_conv1d_train_wgrad_norm(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                                int32_t cout, const float* in_affine, int32_t in_act, float* ws, float* dw, void* stream) {
    if (!in_affine) return fail_msg("syn_conv1d_train_wgrad_norm: in_affine is NULL (use syn_conv1d_train_wgrad)");
    return conv_train_wgrad_impl(x, dy, n_clips, l_in, cin, stride, pad, cout, in_affine, in_act, ws, dw, stream);
}

/* conv1 and the shortcut convolution of a down-sampling block (same input, same geometry): both weight gradients' partial sums from ONE launch that stages the
 * input once (k_conv_wgrad_s<128, 3, true>: the tile's two halves are the two dy).  (64, 6, 64) only - block 1, whose input is the encoder's largest tensor. */
int syn_conv1d_train_wgrad_pair(const float* x, const float* dy_a, const float* dy_b, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                                int32_t cout, float* ws, void* stream) {
    if (!x || !dy_a || !dy_b || !ws || n_clips <= 0 || l_in <= 0) return fail_msg("syn_conv1d_train_wgrad_pair: bad arguments");
    if (!(cin == 64 && stride == 6 && pad == 0 && cout == 64)) return fail_msg("syn_conv1d_train_wgrad_pair: the (64, stride 6, 64) layer pair only (block 1 of the audio encoder)");
    const int l_out = (l_in - 15) / stride + 1, cinp = stride * cin;
    if (l_out <= 0) return fail_msg("syn_conv1d_train_wgrad_pair: input shorter than the kernel");
    wav::WArgs a;
    a.GY = dy_a; a.GY2 = dy_b; a.gy_clip_stride = (long)l_out * cout; a.L_out = l_out; a.X = x; a.x_clip_stride = (long)l_in * cin; a.x_elems = (long)l_in * cin;
    a.cin = cinp; a.co_n = cout; a.n_clips = n_clips; a.chunks_per_clip = (l_out + wav::kWgP - 1) / wav::kWgP; a.row0 = 0;
    a.shares = syn_conv1d_wgrad_shares(n_clips, l_out, cinp, cout); a.part = ws;          // (3 slices, as for one of the two: ws holds shares x 2 gradients)
    a.in_aff = nullptr; a.in_act = 0;
    return launch_wgrad_s<128, 3, true>(a, (hipStream_t)stream);
}

// workgroups of the persistent first-layer weight gradient (k_conv_first_wgrad_m): four per CU once there is that much work, never more than there are
// 64-pair work items per workgroup
static int first_wgrad_groups(int n_clips, int l_out, int per_cu = 4) {
    const long pairs = (long)n_clips * ((l_out + 1) / 2);
    const long want = (long)per_cu * device_cus(), by_work = (pairs + 255) / 256;      // (1 / 2 / 4 / 8 per CU at the bench shape: 190 / 123 / 108 / 107 us for the two launches)
    return (int)(by_work < 1 ? 1 : by_work < want ? by_work : want);
}
int32_t syn_conv1d_first_parts(int32_t n_clips, int32_t l_out) {
    return n_clips > 0 && l_out > 0 ? first_wgrad_groups(n_clips, l_out) : 0;        // one partial gradient per workgroup
}
int32_t syn_conv1d_first_tiles(int32_t n_clips, int32_t l_out) { return n_clips > 0 && l_out > 0 ? n_clips * ((l_out + wav::kF1Tile - 1) / wav::kF1Tile) : 0; }

static int first_layer_args(wav::FArgs& a, const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const char* who) {
    if (!x || n_clips <= 0 || l_in <= 0 || (cin != 1 && cin != 2) || stride < 1 || stride > 8 || pad < 0) return fail_msg(who);
    a.X = x; a.L_in = l_in; a.n_clips = n_clips; a.stride = stride; a.pad = pad;
    a.L_out = (l_in + 2 * pad - 15) / stride + 1;
    if (a.L_out <= 0) return fail_msg(who);
    a.W = nullptr; a.Y = nullptr; a.DY = nullptr; a.part = nullptr; a.chunks_per_clip = (a.L_out + wav::kF1Chunk - 1) / wav::kF1Chunk;
    a.BY = nullptr; a.bn_stats = a.bn_aff = a.bn_dgb = nullptr; a.bn_inv_rows = 0.f; a.bn_act = 0; a.W2 = nullptr; a.Y2 = nullptr; a.part2 = nullptr;
    a.T_y2 = nullptr; a.t_stats = a.t_aff = a.t_dgb = nullptr; a.T_dy2 = nullptr;
    return 0;
}

int syn_conv1d_first_fwd_stats(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const float* w, float* y,
                               float* bn_part, void* stream) {
    wav::FArgs a;
    if (!w || !y) return fail_msg("syn_conv1d_first_fwd: bad arguments");
    if (int rc = first_layer_args(a, x, n_clips, l_in, cin, stride, pad, "syn_conv1d_first_fwd: bad arguments (cin 1 | 2, 64 output channels)")) return rc;
    a.W = w; a.Y = y; a.part = bn_part;
    const dim3 grid((a.L_out + wav::kF1Tile - 1) / wav::kF1Tile, n_clips);
    size_t lds = (size_t)((wav::kF1Tile - 1) * stride + 15) * cin * sizeof(float);
    if (lds < 4 * 2 * 64 * sizeof(float)) lds = 4 * 2 * 64 * sizeof(float);       // (the statistics of the four position groups meet in the window's place)
    if (cin == 1) hipLaunchKernelGGL(wav::k_conv_first_fwd<1>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(wav::k_conv_first_fwd<2>, grid, dim3(256), lds, (hipStream_t)stream, a);
    return launched("k_conv_first_fwd launch");
}

int syn_conv1d_first_fwd(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const float* w, float* y,
                         void* stream) {
    return syn_conv1d_first_fwd_stats(x, n_clips, l_in, cin, stride, pad, w, y, nullptr, stream);
}

struct FirstTail { const float* y2; const float* stats2; const float* aff2; const float* dgb2; float* dy2; };
static int first_wgrad_impl(const float* x, const float* dy, const float* bn_y, const float* bn_stats, const float* bn_aff, const float* bn_dgb,
                            int32_t bn_act, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dw, void* stream,
                            const FirstTail* tail = nullptr) {
    wav::FArgs a;
    if (!dy || !ws) return fail_msg("syn_conv1d_first_wgrad: bad arguments");
    if (int rc = first_layer_args(a, x, n_clips, l_in, cin, stride, pad, "syn_conv1d_first_wgrad: bad arguments (cin 1 | 2, 64 output channels)")) return rc;
    a.DY = dy; a.part = ws;
    if (bn_y) {
        if (stride != 5 || !bn_stats || !bn_aff || !bn_dgb) return fail_msg("syn_conv1d_first_wgrad_bn: stride 5 (the encoder's), statistics, affine and dgamma / dbeta");
        a.BY = bn_y; a.bn_stats = bn_stats; a.bn_aff = bn_aff; a.bn_dgb = bn_dgb; a.bn_inv_rows = 1.0f / ((float)n_clips * (float)a.L_out); a.bn_act = bn_act;
    }
    if (tail) {
        if (!bn_y || !tail->y2 || !tail->stats2 || !tail->aff2 || !tail->dgb2 || !tail->dy2) return fail_msg("syn_conv1d_first_wgrad_tail: null pointer");
        a.T_y2 = tail->y2; a.t_stats = tail->stats2; a.t_aff = tail->aff2; a.t_dgb = tail->dgb2; a.T_dy2 = tail->dy2;
    }
    hipStream_t s = (hipStream_t)stream;
    const int groups = first_wgrad_groups(n_clips, a.L_out);
    if (tail) {
        if ((long)n_clips * a.L_out * 64 >= (1L << 32)) return fail_msg("syn_conv1d_first_wgrad_tail: n_clips x l_out x 64 must stay below 2^32 elements");
        if (cin == 1) hipLaunchKernelGGL((wav::k_conv_first_wgrad_m<1, true>), dim3(groups), dim3(wav::kF1mWaves * 64), 0, s, a);
        else hipLaunchKernelGGL((wav::k_conv_first_wgrad_m<2, true>), dim3(groups), dim3(wav::kF1mWaves * 64), 0, s, a);
    }
    else if (cin == 1) hipLaunchKernelGGL((wav::k_conv_first_wgrad_m<1>), dim3(groups), dim3(wav::kF1mWaves * 64), 0, s, a);
    else hipLaunchKernelGGL((wav::k_conv_first_wgrad_m<2>), dim3(groups), dim3(wav::kF1mWaves * 64), 0, s, a);
    const int n = 64 * cin * 15;
    if (dw) hipLaunchKernelGGL(wav::k_conv_first_wsum, dim3((n + 63) / 64), dim3(1024), 0, s, (const float*)ws, groups, n, dw);
    return launched("k_conv_first_wgrad_m launch");
}

int syn_conv1d_wgrad_sums(const syn_wgrad_sum_job* jobs, int32_t n_jobs, void* stream) {
    static_assert(SYN_WGRAD_SUM_MAX == wav::kWsumJobs, "include/syn_hip.h: jobs per syn_conv1d_wgrad_sums call");
    if (!jobs || n_jobs < 1 || n_jobs > SYN_WGRAD_SUM_MAX) return fail_msg("syn_conv1d_wgrad_sums: 1 .. 4 jobs");
    wav::WSumJobs a;
    memset(&a, 0, sizeof(a));
    int blocks = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const syn_wgrad_sum_job& q = jobs[i];
        wav::WSumJob& J = a.j[i];
        if (!q.part || !q.dw || q.n_clips <= 0 || q.l_out <= 0) return fail_msg("syn_conv1d_wgrad_sums: null pointer / empty job");
        J.part = q.part; J.dw = q.dw; J.cin = q.cin; J.stride = q.stride; J.co_n = q.cout; J.first_block = blocks;
        if (q.first_layer) {
            if ((q.cin != 1 && q.cin != 2) || q.cout != 64) return fail_msg("syn_conv1d_wgrad_sums: a first-layer job has 1 | 2 input and 64 output channels");
            J.kind = 1; J.shares = first_wgrad_groups(q.n_clips, q.l_out); J.per = 64 * q.cin * 15; J.taps = 15;
        } else {
            if (q.cin % 16 || q.stride < 1) return fail_msg("syn_conv1d_wgrad_sums: cin must be a multiple of 16");
            J.kind = 0; J.taps = (15 + q.stride - 1) / q.stride; J.shares = syn_conv1d_wgrad_shares(q.n_clips, q.l_out, q.stride * q.cin, q.cout);
            J.per = q.cout * J.taps * q.stride * q.cin;
        }
        J.pitch = q.share_pitch > 0 ? q.share_pitch : J.per;
        if (J.pitch < J.per || J.pitch % 4) return fail_msg("syn_conv1d_wgrad_sums: share_pitch must be 0 or a multiple of 4 not below the gradient's size");
        blocks += (J.per / 4 + 31) / 32;
    }
    a.n = n_jobs;
    hipLaunchKernelGGL(wav::k_conv_wgrad_sums, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launched("k_conv_wgrad_sums launch");
}

int syn_conv1d_first_wgrad(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws,
                           float* dw, void* stream) {
    return first_wgrad_impl(x, dy, nullptr, nullptr, nullptr, nullptr, 0, n_clips, l_in, cin, stride, pad, ws, dw, stream);
}

int syn_conv1d_first_wgrad_bn(const float* x, const float* dz, const float* y, const float* stats, const float* affine, const float* dgamma_dbeta,
                              int32_t act, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dw, void* stream) {
    if (!y) return fail_msg("syn_conv1d_first_wgrad_bn: y is NULL (use syn_conv1d_first_wgrad)");
    return first_wgrad_impl(x, dz, y, stats, affine, dgamma_dbeta, act, n_clips, l_in, cin, stride, pad, ws, dw, stream);
}

int syn_conv1d_first_wgrad_bn_lin(const float* x, const float* dz, const float* y, const float* stats, const float* affine, int32_t act,
                                  int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dw, float* dgamma_dbeta, void* stream) {
    wav::FArgs a;
    if (!dz || !y || !stats || !affine || !ws || !dw || !dgamma_dbeta) return fail_msg("syn_conv1d_first_wgrad_bn_lin: null pointer");
    if (int rc = first_layer_args(a, x, n_clips, l_in, cin, stride, pad, "syn_conv1d_first_wgrad_bn_lin: bad arguments (cin 1 | 2, 64 output channels)")) return rc;
    if (stride != 5) return fail_msg("syn_conv1d_first_wgrad_bn_lin: stride 5 (the encoder's)");
    a.DY = dz; a.BY = y; a.bn_stats = stats; a.bn_aff = affine; a.bn_act = act; a.part = ws;
    hipStream_t s = (hipStream_t)stream;
    const int groups = first_wgrad_groups(n_clips, a.L_out, 3);      // (64 accumulator + 73 other registers: three waves per SIMD - a fourth workgroup per CU would run in a second round)
    const float inv_rows = 1.0f / ((float)n_clips * (float)a.L_out);
    if (cin == 1) {
        hipLaunchKernelGGL(wav::k_conv_first_wgrad_lin<1>, dim3(groups), dim3(wav::kF1mWaves * 64), 0, s, a);
        hipLaunchKernelGGL(wav::k_conv_first_wgrad_lin_fin<1>, dim3(64), dim3(1024), 0, s, (const float*)ws, groups, affine, inv_rows, dw, dgamma_dbeta);
    } else {
        hipLaunchKernelGGL(wav::k_conv_first_wgrad_lin<2>, dim3(groups), dim3(wav::kF1mWaves * 64), 0, s, a);
        hipLaunchKernelGGL(wav::k_conv_first_wgrad_lin_fin<2>, dim3(64), dim3(1024), 0, s, (const float*)ws, groups, affine, inv_rows, dw, dgamma_dbeta);
    }
    return launched("k_conv_first_wgrad_lin launch");
}

int syn_conv1d_first_wgrad_tail(const float* x, const float* dout, const float* y2, const float* y_short, const float* stats2, const float* affine2,
                                const float* short_stats, const float* short_affine, const float* dgb2, const float* short_dgb, int32_t act,
                                int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dy2, void* stream) {
    const FirstTail t = {y2, stats2, affine2, dgb2, dy2};
    return first_wgrad_impl(x, dout, y_short, short_stats, short_affine, short_dgb, act, n_clips, l_in, cin, stride, pad, ws, nullptr, stream, &t);
}

int syn_conv1d_first_fwd2(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const float* w_a, const float* w_b,
                          float* y_a, float* y_b, float* bn_part_a, float* bn_part_b, void* stream) {
    wav::FArgs a;
    if (!w_a || !w_b || !y_a || !y_b || ((bn_part_a == nullptr) != (bn_part_b == nullptr))) return fail_msg("syn_conv1d_first_fwd2: bad arguments");
    if (int rc = first_layer_args(a, x, n_clips, l_in, cin, stride, pad, "syn_conv1d_first_fwd2: bad arguments (cin 1 | 2, 64 output channels)")) return rc;
    a.W = w_a; a.W2 = w_b; a.Y = y_a; a.Y2 = y_b; a.part = bn_part_a; a.part2 = bn_part_b;
    const dim3 grid((a.L_out + wav::kF1Tile - 1) / wav::kF1Tile, n_clips);
    size_t lds = (size_t)((wav::kF1Tile - 1) * stride + 15) * cin * sizeof(float);
    if (lds < 2 * 4 * 2 * 64 * sizeof(float)) lds = 2 * 4 * 2 * 64 * sizeof(float);
    if (cin == 1) hipLaunchKernelGGL(wav::k_conv_first_fwd2<1>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(wav::k_conv_first_fwd2<2>, grid, dim3(256), lds, (hipStream_t)stream, a);
    return launched("k_conv_first_fwd2 launch");
}

// taps of the strided data-gradient GEMM, padded so that taps * cout / 32 is a multiple of the weight ring's 3
static int dgrad_taps(int stride, int cout) {
    int kt = (15 + stride - 1) / stride;
    while ((kt * cout / 32) % 3) ++kt;
    return kt;
}

// geometry of one pack: taps (padded), kernel mode, fragments x 64; < 0: not a shape the kernels take
static int conv_pack_geometry(int cout, int cin, int stride, int transposed, int& kts, int& mode) {
    if (cout % 16 || cin % 16 || stride < 1 || cout <= 0 || cin <= 0) return -1;
    int N, C;
    mode = transposed ? 1 : 0;
    if (transposed && stride > 1) { mode = 2; kts = dgrad_taps(stride, cout); N = stride * cin; C = cout; }
    else { kts = (15 + stride - 1) / stride * stride; N = transposed ? cin : cout; C = transposed ? cout : cin; }
    if ((kts * C) % 32) return -1;
    return (N / 16) * (kts * C / 32) * 64;
}

int syn_conv1d_pack_split_many(const syn_conv_pack_req* reqs, int32_t n_reqs, void* stream) {
    static_assert(SYN_CONV_PACK_MAX == kConvPackMax, "include/syn_hip.h: packs per launch");
    if (!reqs || n_reqs <= 0 || n_reqs > kConvPackMax) return fail_msg("syn_conv1d_pack_split_many: 1 .. 40 requests");
    ConvPackJobs j;
    memset(&j, 0, sizeof(j));
    int most = 0;
    for (int i = 0; i < n_reqs; ++i) {
        const syn_conv_pack_req& r = reqs[i];
        int kts, mode;
        const int total = (r.w && r.out_hi && r.out_lo) ? conv_pack_geometry(r.cout, r.cin, r.stride, r.transposed, kts, mode) : -1;
        if (total < 0) return fail_msg("syn_conv1d_pack_split_many: bad request (as syn_conv1d_pack_split)");
        j.w[i] = r.w; j.hi[i] = (uint4*)r.out_hi; j.lo[i] = (uint4*)r.out_lo; j.cout[i] = (short)r.cout; j.cin[i] = (short)r.cin;
        j.kts[i] = (signed char)kts; j.mode[i] = (signed char)mode; j.stride[i] = (signed char)r.stride;
        most = total > most ? total : most;
    }
    hipLaunchKernelGGL(k_conv_pack_split_many, dim3((most + 255) / 256, n_reqs), dim3(256), 0, (hipStream_t)stream, j);
    return launched("k_conv_pack_split_many launch");
}

int syn_conv1d_pack_split(const float* w, int32_t cout, int32_t cin, int32_t stride, int32_t transposed, void* out_hi, void* out_lo,
                          void* stream) {
    if (!w || !out_hi || !out_lo) return fail_msg("syn_conv1d_pack_split: bad arguments");
    int kts, mode;
    const int total = conv_pack_geometry(cout, cin, stride, transposed, kts, mode);
    if (total < 0) return fail_msg("syn_conv1d_pack_split: channels must be multiples of 16 and taps x channels a multiple of 32");
    hipLaunchKernelGGL(k_conv_pack_split, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, cout, cin, kts, mode, stride,
                       (uint4*)out_hi, (uint4*)out_lo);
    return launched("k_conv_pack_split launch");
}

int64_t syn_conv1d_pack_bytes(int32_t cout, int32_t cin, int32_t stride, int32_t transposed) {
    if (cout <= 0 || cin <= 0 || stride < 1) return 0;
    if (transposed && stride > 1) return (int64_t)stride * cin * dgrad_taps(stride, cout) * cout * 2;
    const int kts = (15 + stride - 1) / stride * stride;
    return (int64_t)cout * kts * cin * 2;
}

// Data gradient of a strided, unpadded Conv1d(k = 15) of the encoder: dx [n][l_in][cin] from dy [n][l_out][cout] - a stride-1
// convolution over dy whose output rows are stride consecutive positions x cin channels: ONE launch over all stride x cin columns, 64 per
// workgroup (grid z), a wave 16 channels x 128 / 64 / 32 positions (the decompositions measured in round 5: profiles/r05_ubench_conv_variants.txt).
static int dgrad_strided_impl(const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t cout,
                              const void* w_hi, const void* w_lo, const float* dy2, const void* w2_hi, const void* w2_lo, float* dx, void* stream) {
    if (!dy || !w_hi || !w_lo || !dx || n_clips <= 0 || l_in < 15 || stride < 2) return fail_msg("syn_conv1d_train_dgrad_strided: bad arguments");
    if (dy2 && (!w2_hi || !w2_lo)) return fail_msg("syn_conv1d_train_dgrad_sum: the second gradient needs its fragment sets");
    const int l_out = (l_in - 15) / stride + 1, kt = dgrad_taps(stride, cout), q_rows = (l_in + stride - 1) / stride, np = stride * cin;
    if (np % 128) return fail_msg("syn_conv1d_train_dgrad_strided: stride * cin must be a multiple of 128");
    hipStream_t s = (hipStream_t)stream;
    wav::TArgs a;
    a.X = dy; a.x_clip_stride = (long)l_out * cout; a.x_elems = (long)l_out * cout; a.row0 = -(kt - 1); a.L_out = q_rows;
    a.Whi = (const uint4*)w_hi; a.Wlo = (const uint4*)w_lo; a.bias = nullptr;
    a.Y = dx; a.y_clip_stride = (long)l_in * cin; a.y_pitch = np; a.y_col0 = 0; a.y_elems = (long)l_in * cin; a.bn_part = nullptr;
    a.in_aff = nullptr; a.in_act = 0; a.R = nullptr;
    a.X2 = dy2; a.Whi2 = dy2 ? (const uint4*)w2_hi : nullptr; a.Wlo2 = dy2 ? (const uint4*)w2_lo : nullptr;
    if (cout == 64 && kt == 3) return launch_conv_train<64, 3, 4, 1, 8, 1>(a, n_clips, s, np);
    if (cout == 128 && kt == 3) return launch_conv_train<128, 3, 4, 1, 4, 1>(a, n_clips, s, np);
    if (cout == 256 && kt == 6) return launch_conv_train<256, 6, 4, 1, 2, 1>(a, n_clips, s, np);
    return fail_msg("syn_conv1d_train_dgrad_strided: (cout, stride) must be (64, 6), (128, 6) or (256, 3)");
}

// row fragments (16 positions) per tile of the K-split kernel: 3 = 48 positions, 78 KB of LDS, so two workgroups share a CU and
// one's staging overlaps the other's MFMA phase (4 = 64 positions, 103 KB: one workgroup per CU)
constexpr int kKsRf = 3;
// positions per workgroup tile of syn_conv1d_train_fwd's kernel instance (0: not one of the encoder's layers).  The decomposition of every layer
// class - channels and positions per wave, channel blocks on grid z - is the one that won round 5's comparison (profiles/r05_ubench_conv_variants.txt;
// the other variants live in the lab notebook, not here): what bounds these kernels is the CU's L1 port (weight fragments), so a wave takes few
// channels and many positions.
static int conv_train_tile(int cinp, int stride, int cout, int n_clips, int l_out) {
    if (cinp == 384 && stride == 6 && cout == 64) return 16 * kKsRf;
    // (224 positions - two planes of 238 rows x 160 B = 76 KB, two workgroups per CU with the 32-byte row padding; short layers: 128, so that the
    // launch still fills the chip and the last tile of a clip wastes less)
    if (cinp == 64 && stride == 1 && cout == 64) return (long)n_clips * ((l_out + 255) / 256) < 2 * device_cus() ? 128 : 224;
    if (cinp == 128 && stride == 1 && cout == 128) return 64;
    if (cinp == 256 && stride == 1 && cout == 256) return 32;
    if (cinp == 384 && stride == 6) return 64;
    if (cinp == 384 && stride == 3) return 32;
    return 0;
}

int32_t syn_conv1d_train_fwd_tiles(int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, int32_t cout) {
    if (stride < 1) return 0;
    const int l_out = (l_in + 2 * pad - 15) / stride + 1, mw = l_out > 0 && n_clips > 0 ? conv_train_tile(stride * cin, stride, cout, n_clips, l_out) : 0;
    return mw ? n_clips * ((l_out + mw - 1) / mw) : 0;
}

struct ConvDual { const void* w_hi; const void* w_lo; float* y; float* bn_part; };     // a second convolution of the same geometry on the same input

static int conv_train_fwd_impl(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                               const void* w_hi, const void* w_lo, const float* bias, int32_t cout, const float* in_affine, int32_t in_act,
                               float* y, float* bn_part, void* stream, const float* residual = nullptr, const ConvDual* dual = nullptr) {
    if (residual && !(stride == 1 && cin * stride != 384)) return fail_msg("syn_conv1d_train_dgrad_sum: the residual rides the stride-1 kernel");
    if (!x || !w_hi || !w_lo || !y || n_clips <= 0 || l_in <= 0) return fail_msg("syn_conv1d_train_fwd: null pointer / empty batch");
    if (in_affine && stride != 1) return fail_msg("syn_conv1d_train_fwd_norm: the input affine is for the stride-1 layers (conv2 of a block)");
    if (stride < 1 || pad < 0 || pad % stride) return fail_msg("syn_conv1d_train_fwd: padding must be a multiple of the stride");
    const int l_out = (l_in + 2 * pad - 15) / stride + 1;
    if (l_out <= 0) return fail_msg("syn_conv1d_train_fwd: input shorter than the kernel");
    wav::TArgs a;
    a.X = x; a.x_clip_stride = (long)l_in * cin; a.x_elems = (long)l_in * cin; a.row0 = -pad / stride; a.L_out = l_out;
    a.Whi = (const uint4*)w_hi; a.Wlo = (const uint4*)w_lo; a.bias = bias; a.Y = y; a.y_clip_stride = (long)l_out * cout;
    a.y_pitch = 0; a.y_col0 = 0; a.y_elems = 0; a.bn_part = bn_part;
    a.in_aff = in_affine; a.in_act = in_act;
    a.X2 = nullptr; a.Whi2 = a.Wlo2 = nullptr; a.R = residual;
    a.WhiB = a.WloB = nullptr; a.YB = nullptr; a.bn_partB = nullptr;
    if (dual) {
        if (stride == 1 || bias || !dual->w_hi || !dual->w_lo || !dual->y || ((dual->bn_part == nullptr) != (bn_part == nullptr)))
            return fail_msg("syn_conv1d_train_fwd_pair: the encoder's strided layers, no bias, both or neither with statistics");
        a.WhiB = (const uint4*)dual->w_hi; a.WloB = (const uint4*)dual->w_lo; a.YB = dual->y; a.bn_partB = dual->bn_part;
    }
    if (bn_part && bias) return fail_msg("syn_conv1d_train_fwd: the statistics are those of the convolution without its bias (pass bias = NULL)");
    hipStream_t s = (hipStream_t)stream;
    const int cinp = stride * cin;
    // (rows of stride * cin floats, ceil(15 / stride) taps; tiles as the eval-mode encoder picks them, halved where two planes
    // of a 384-channel tile would not fit the LDS)
    // (short layers: smaller tiles, so that the launch still fills the chip and the last tile of a clip wastes less)
    if (cinp == 64 && stride == 1 && cout == 64)               // a wave: 32 channels x 112 / 64 positions
        return conv_train_tile(cinp, stride, cout, n_clips, l_out) > 128 ? launch_conv_train<64, 15, 2, 2, 7, 2>(a, n_clips, s, 64)
                                                                         : launch_conv_train<64, 15, 2, 2, 4, 2>(a, n_clips, s, 64);
    if (cinp == 128 && stride == 1 && cout == 128) return launch_conv_train<128, 15, 4, 1, 4, 1>(a, n_clips, s, 128);   // 64 positions x 64 channels per workgroup (z: 2), a wave: 16 channels x 64 positions
    if (cinp == 256 && stride == 1 && cout == 256) return launch_conv_train<256, 15, 4, 1, 2, 1>(a, n_clips, s, 256);   // 32 positions x 64 channels (z: 4)
    if (cinp == 384 && stride == 6 && cout == 64) {            // the four waves split K
        // (a pair goes out as two launches: on this kernel - 48-position tiles, bound by its fixed costs, not by staging - sharing the tile measured
        //  145 us against 2 x 66)
        if (int rc = launch_conv_train_ks<384, 3, kKsRf>(a, n_clips, s)) return rc;
        if (!dual) return 0;
        a.Whi = a.WhiB; a.Wlo = a.WloB; a.Y = a.YB; a.bn_part = a.bn_partB;
        return launch_conv_train_ks<384, 3, kKsRf>(a, n_clips, s);
    }
    if (cinp == 384 && stride == 6 && cout == 128) return dual ? launch_conv_train<384, 3, 2, 2, 2, 4, true>(a, n_clips, s) : launch_conv_train<384, 3, 2, 2, 2>(a, n_clips, s);   // 64-position tiles
    if (cinp == 384 && stride == 3 && cout == 256) return dual ? launch_conv_train<384, 5, 4, 1, 2, 1, true>(a, n_clips, s, 256) : launch_conv_train<384, 5, 4, 1, 2, 1>(a, n_clips, s, 256);   // 32 positions x 64 channels (z: 4)
    return fail_msg("syn_conv1d_train_fwd: not one of the WavEncoder's convolutions (cin x stride -> cout: 64x1->64, 128x1->128, 256x1->256, 64x6->64, 64x6->128, 128x3->256)");
}

int syn_conv1d_train_fwd(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                         const void* w_hi, const void* w_lo, const float* bias, int32_t cout, float* y, float* bn_part, void* stream) {
    return conv_train_fwd_impl(x, n_clips, l_in, cin, stride, pad, w_hi, w_lo, bias, cout, nullptr, 0, y, bn_part, stream);
}

int syn_conv1d_train_fwd_pair(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, int32_t cout,
                              const void* wa_hi, const void* wa_lo, float* y_a, float* bn_part_a,
                              const void* wb_hi, const void* wb_lo, float* y_b, float* bn_part_b, void* stream) {
    const ConvDual d{wb_hi, wb_lo, y_b, bn_part_b};
    return conv_train_fwd_impl(x, n_clips, l_in, cin, stride, pad, wa_hi, wa_lo, nullptr, cout, nullptr, 0, y_a, bn_part_a, stream, nullptr, &d);
}

int syn_conv1d_train_fwd_norm(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                              const void* w_hi, const void* w_lo, int32_t cout, const float* in_affine, int32_t in_act, float* y, float* bn_part,
                              void* stream) {
    if (!in_affine) return fail_msg("syn_conv1d_train_fwd_norm: in_affine is NULL (use syn_conv1d_train_fwd)");
    return conv_train_fwd_impl(x, n_clips, l_in, cin, stride, pad, w_hi, w_lo, nullptr, cout, in_affine, in_act, y, bn_part, stream);
}

int syn_conv1d_train_dgrad_sum(const float* dy, const void* w_hi, const void* w_lo, const float* dy2, const void* w2_hi, const void* w2_lo,
                               const float* residual, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, int32_t cout, float* dx,
                               void* stream) {
    if (stride == 1) {
        if (dy2) return fail_msg("syn_conv1d_train_dgrad_sum: two gradients are summed for the strided layers (a down-sampling block); stride 1 takes a residual");
        if (pad != 7) return fail_msg("syn_conv1d_train_dgrad_sum: stride 1 means the padding-7 layers");
        return conv_train_fwd_impl(dy, n_clips, l_in, cout, 1, 7, w_hi, w_lo, nullptr, cin, nullptr, 0, dx, nullptr, stream, residual);
    }
    if (residual || pad != 0) return fail_msg("syn_conv1d_train_dgrad_sum: the strided layers are unpadded and take no residual");
    return dgrad_strided_impl(dy, n_clips, l_in, cin, stride, cout, w_hi, w_lo, dy2, w2_hi, w2_lo, dx, stream);
}

void syn_debug_conv_terms(int mask) { g_conv_terms = mask < 0 ? -1 : (mask & 3); }   /* diagnostics: cross products of the split-operand training convolutions (3 = all) */

}  // extern "C"
