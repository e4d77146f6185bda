// syn_stack_train.inc — the 8 transformer blocks of the TRAINING forward as one persistent kernel (round 5; SURVEY.md §8 a10 / a19;
// reference models/timm_transformer/transformer.py:154-198 Block, :83-104 Attention, :145-151 Mlp, :21-38 DropPath).
// Included by syn_kernels.hip behind k_stack, whose tile-split mode it is built on; entry points syn_train_stack_* at the end.
//
// Why.  Issued as one launch per operation the forward of the blocks is 56 launches of 6-10 us for 38 GFLOP (profiles/r04_train_step_split.txt:
// 0.55 ms, every launch at its latency floor).  k_stack already runs this arithmetic for sampling as ONE launch: a 32-row tile (one sequence)
// split over the 4 workgroups of one XCD - member j takes head j and MLP slice j, the members' partial sums meet in an L2-resident exchange
// (two per block).  This kernel is that loop plus what a backward needs:
//   * DropPath (one factor per sequence and branch): a branch is accumulated on its own, starting from its bias in member 0 and from zero in
//     the others, and after the exchange h = h_in + factor * branch.  h_in is not kept in registers (the kernel sits at 236 of 256): it is the
//     tensor the backward needs anyway, written by member 0 before the branch and read back by everybody (L2, past the L1) after the exchange;
//   * saved for the backward, in the layouts training.AttnBranchFn / MlpBranchFn.backward take: the branch inputs h (fp32), LayerNorm mean / rstd,
//     qkv and the fc1 pre-activation (fp32), and the four operand transposes of the weight-gradient GEMMs as packed MFMA fragments
//     (LayerNorm outputs, attention output, GELU output: gathered out of the LDS tiles the forward GEMMs read).
// Arithmetic = k_stack's (bf16 operands incl. q / k / v / p, fp32 accumulate, fp32 residual / LayerNorm / softmax).
namespace {
namespace stk {

constexpr int kTrainLds = 72 * 1024 + 64 * 1024;       // k_stack<32>'s tiles (68 KB, rounded) + the branch input's fp32 copy

struct TrainSave {       // one block's saved tensors; M = 32 x sequences rows
    float* hA; float* meanA; float* rstdA;      // attention branch: input [M][512], LayerNorm statistics [M]
    float* qkv;                                 // [M][1536] fp32 (no bias: the reference's qkv Linear has none)
    uint4* xt_ln1; uint4* xt_o;                 // fragments of LN1(h)^T and of the attention output^T: [512 / 16][M / 32][64] x 16 B
    float* hM; float* meanM; float* rstdM;      // MLP branch
    float* pre;                                 // [M][1024] fc1 output + bias, before the GELU
    uint4* xt_ln2; uint4* xt_a;                 // fragments of LN2(h)^T [512/16][M/32][64], of GELU(pre)^T [1024/16][M/32][64]
};

struct TArgsS {
    const float* H;       // [M][512] input
    float* Hout;          // [M][512] output
    syn_layer layer[SYN_LAYERS];
    TrainSave save[SYN_LAYERS];
    const float* dp;      // null, or DropPath factors [2 * SYN_LAYERS][tiles]: row 2 l = attention branch of block l, 2 l + 1 = its MLP branch
    int M, tiles;
    int flags;            // diagnostics (timing only, wrong results): 1 no fp32 saves, 2 no transposed fragments, 4 unused
    unsigned* sync;       // [320] zeroed (k_stack's layout)
    float* xch;           // [tiles][2][4][32 * 512] exchange slots
};

// fragment (nf, ks = tile) of X^T for the 32 rows of a tile held in LDS as swizzled bf16 rows: lane (g, lr) takes X[8 g + e][16 nf + lr], e = 0..7
__device__ __forceinline__ uint4 xt_frag(const char* base, int rowb, int col0) {
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));                 // rebuilt here: hoisted out of the block loop these eight addresses per call site end up in scratch
    const int g = lane >> 4, col = col0 + (lane & 15);
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int r = 8 * g + e;
        v[e] = *reinterpret_cast<const unsigned short*>(base + r * rowb + ((((col >> 3) ^ (r & 15))) << 4) + (col & 7) * 2);
    }
    uint4 o;
    o.x = (unsigned)v[0] | ((unsigned)v[1] << 16); o.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
    o.z = (unsigned)v[4] | ((unsigned)v[5] << 16); o.w = (unsigned)v[6] | ((unsigned)v[7] << 16);
    return o;
}

__global__ __launch_bounds__(kThreads) void k_stack_train(const TArgsS a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MT = 32, MF = 2, P = 4, HC = 256;
    constexpr int KS1 = SYN_D / 32, KS2 = SYN_FF / 32;
    char* const XN = smem;
    char* const RB = smem + MT * 1024;
    char* const Qs = RB;
    char* const Ks = RB + MT * 256;
    char* const Vts = RB + MT * 512;
    float* const red = reinterpret_cast<float*>(RB + MT * 1024);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    // membership: as in k_stack's tile-split mode (hardware XCC id, rank by arrival)
    __shared__ int s_rank;
    const int xcd = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u) % lat::kGroups;
    unsigned* const xbase = a.sync + xcd * 32;
    unsigned* const gerr = a.sync + lat::kGroups * 32;
    if (tid == 0) s_rank = (int)__hip_atomic_fetch_add(xbase, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int rank = s_rank, per_xcd = (int)gridDim.x / lat::kGroups;
    if (rank >= per_xcd) {
        if (tid == 0) __hip_atomic_store(gerr, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int member = rank % P, tile = xcd + lat::kGroups * (rank / P);
    unsigned* const gctr = xbase + 2 + rank / P;
    unsigned gphase = 0;
    auto tp_done = [&]() {
        if (tid == 0) {
            if (__hip_atomic_fetch_add(xbase + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)per_xcd - 1)
                for (int i = 0; i < 32; ++i) __hip_atomic_store(xbase + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (tile >= a.tiles) { tp_done(); return; }
    const int m0 = tile * MT;
    const int KSM = a.M / 32;                                  // k-steps (32-row tiles) of the transposed operands
    // this member's partial -> the sum of the four, in member order (k_stack's exchange)
    auto exchange = [&](f32x4 (&hh)[4][MF]) {
        int et = tid;
        asm volatile("" : "+v"(et));
        float* const set = a.xch + ((size_t)(tile * 2 + (int)(gphase & 1u)) * 4) * (MT * 512) + et * 4;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
                *reinterpret_cast<f32x4*>(set + (size_t)member * (MT * 512) + (nf * MF + mf) * 2048) = hh[nf][mf];
        lat::group_release();
        ++gphase;
        lat::group_wait(gctr, gphase * (unsigned)P, gerr);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[P][2][MF];
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                    for (int mf = 0; mf < MF; ++mf)
                        if (j != member)
                            v[j][n2][mf] = lat::ld_xcd(reinterpret_cast<const f32x4*>(set + (size_t)j * (MT * 512) + ((half * 2 + n2) * MF + mf) * 2048));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    const f32x4 own = hh[half * 2 + n2][mf];
                    f32x4 sum = member == 0 ? own : v[0][n2][mf];
#pragma unroll
                    for (int j = 1; j < P; ++j) sum = sum + (j == member ? own : v[j][n2][mf]);
                    hh[half * 2 + n2][mf] = sum;
                }
        }
    };
    // row / column of this lane's h fragments: h[nf][mf] = rows m0 + 16 mf + lr, columns 64 wave + 16 nf + 4 g .. + 3
    auto hoff = [&](int nf, int mf) { return (size_t)(m0 + mf * 16 + lr) * kNT + wave * 64 + nf * 16 + g * 4; };
    // (b) the branch input also stays on chip: 64 KB of LDS behind the tiles (one workgroup per CU: the LDS has the room), so that the residual after the
    // exchange is an LDS read, not an L2 round trip on the critical path
    float* const HS = reinterpret_cast<float*>(smem + 72 * 1024);
    auto hs_at = [&](int nf, int mf) { int t = threadIdx.x; asm volatile("" : "+v"(t)); return HS + ((nf * MF + mf) * kThreads + t) * 4; };
    f32x4 h[4][MF];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) h[nf][mf] = *reinterpret_cast<const f32x4*>(a.H + hoff(nf, mf));
    // LayerNorm of h -> XN (bf16, swizzled); statistics out; then h = the branch's starting value (member 0: its bias; the others: 0)
    auto ln_branch_start = [&](const float* lg, const float* lb, const float* bias, float* save_h, float* save_mean, float* save_rstd) {
        if (member == 0 && !(a.flags & 1)) {
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) *reinterpret_cast<f32x4*>(save_h + hoff(nf, mf)) = h[nf][mf];
        }
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) *reinterpret_cast<f32x4*>(hs_at(nf, mf)) = h[nf][mf];
        float mean[MF], rstd[MF];
        row_stats<MT>(h, red, red + MT * 8, mean, rstd);
        if (member == 0 && wave == 0 && g == 0) {
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) { save_mean[m0 + mf * 16 + lr] = mean[mf]; save_rstd[m0 + mf * 16 + lr] = rstd[mf]; }
        }
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int n = wave * 64 + nf * 16 + g * 4;
            const f32x4 gg = *reinterpret_cast<const f32x4*>(lg + n), bb = *reinterpret_cast<const f32x4*>(lb + n);
            const f32x4 ad = member == 0 ? *reinterpret_cast<const f32x4*>(bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            const int slot = 8 * wave + 2 * nf + (g >> 1);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const f32x4 y = (h[nf][mf] - mean[mf]) * rstd[mf] * gg + bb;
                *reinterpret_cast<bf16x4*>(XN + (mf * 16 + lr) * 1024 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(y);
                h[nf][mf] = ad;
            }
        }
    };
    // after the exchange: h = h_in + factor * branch, h_in read back from where member 0 saved it (stores drained before the group barrier)
    auto residual = [&](const float* /*saved_h*/, float f) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(hs_at(nf, mf));       // (this lane's own values: no barrier needed)
                h[nf][mf] = o + h[nf][mf] * f;
            }
    };
    constexpr int DQ = 4, DP = 3, D1 = 6, D2 = 3;
    for (int l = 0; l < SYN_LAYERS; ++l) {
        const syn_layer& L = a.layer[l];
        const TrainSave& S = a.save[l];
        const float fa = a.dp ? a.dp[(size_t)(2 * l) * a.tiles + tile] : 1.0f, fm = a.dp ? a.dp[(size_t)(2 * l + 1) * a.tiles + tile] : 1.0f;
        // ---- attention branch: member = head -----------------------------------------------------------------------------------------
        const int head = member;
        const uint4* const wq = (const uint4*)L.w_qkv + ((size_t)(head * 8 + wave) * KS1) * 64 + lane;
        const uint4* const wproj = (const uint4*)L.w_proj + ((size_t)(wave * 4) * KS1) * 64 + lane;
        uint4 rq[DQ][3];
        kloop_prime<3, 32, KS1, DQ>(rq, wq, KS1, 0);
        ln_branch_start(L.ln1_g, L.ln1_b, L.b_proj, S.hA, S.meanA, S.rstdA);
        __syncthreads();
        if (member == 0 && !(a.flags & 2)) {                // LN1(h)^T fragments: 32 of them, four per wave
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nf = wave * 4 + j;
                S.xt_ln1[((size_t)nf * KSM + tile) * 64 + lane] = xt_frag(XN, 1024, 16 * nf);
            }
        }
        {
            f32x4 acc[3][MF];
#pragma unroll
            for (int sl = 0; sl < 3; ++sl)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) acc[sl][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            kloop_run<MF, 3, 32, 0x4, KS1, 1024, DQ>(acc, rq, XN, wq, KS1, 0);
            uint4 rp[DP][4];
            kloop_prime<4, 1, 4, DP>(rp, wproj, KS1, head * 4);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int row = mf * 16 + lr;
                const int off = row * 256 + ((((2 * wave) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8;
                *reinterpret_cast<bf16x4*>(Qs + off) = to_bf16x4(acc[0][mf]);
                *reinterpret_cast<bf16x4*>(Ks + off) = to_bf16x4(acc[1][mf]);
                *reinterpret_cast<bf16x4*>(Vts + (mf >> 1) * (128 * 72) + (wave * 16 + lr) * 72 + ((mf & 1) * 16 + g * 4) * 2) = to_bf16x4(acc[2][mf]);
                if (a.flags & 1) continue;
                // the fp32 q / k / v of this head for the backward: [M][3][4 heads][128]
                float* const qrow = S.qkv + (size_t)(m0 + row) * (3 * SYN_D) + head * 128 + wave * 16 + g * 4;
                *reinterpret_cast<f32x4*>(qrow) = acc[0][mf];
                *reinterpret_cast<f32x4*>(qrow + SYN_D) = acc[1][mf];
                // v is held swapped: acc[2][mf][r] = v[row 16 mf + 4 g + r][feature 16 wave + lr]
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    S.qkv[(size_t)(m0 + mf * 16 + 4 * g + r) * (3 * SYN_D) + 2 * SYN_D + head * 128 + wave * 16 + lr] = acc[2][mf][r];
            }
            __syncthreads();
            if (wave < MT / 16) {
                const int qh = wave & 1;
                const int qrow = qh * 16 + lr;
                f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int so = (((4 * ks) + g) ^ lr) << 4;
                    const bf16x8 qf = *reinterpret_cast<const bf16x8*>(Qs + qrow * 256 + so);
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (f * 16 + lr) * 256 + so);
                        sc[f] = MFMA16(kf, qf, sc[f]);
                    }
                }
                const float scale = 0.08838834764831845f * 1.4426950408889634f;
                float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                bf16x8 pf;
                float sum = 0.f;
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const __bf16 pv = (__bf16)__builtin_amdgcn_exp2f((sc[f][r] - mx) * scale);
                        pf[f * 4 + r] = pv;
                        sum += (float)pv;
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int df = 0; df < 8; ++df) {
                    const char* vr = Vts + (16 * df + lr) * 72 + 8 * g;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr);
                    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vr + 32);
                    bf16x8 vf;
                    vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
                    vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
                    const f32x4 o = MFMA16(vf, pf, (f32x4{0.f, 0.f, 0.f, 0.f}));
                    *reinterpret_cast<bf16x4*>(Qs + qrow * 256 + ((((2 * df) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(o * inv);
                }
            }
            __syncthreads();
            // attention output^T fragments of this head: nf = 8 head + wave
            if (!(a.flags & 2)) S.xt_o[((size_t)(head * 8 + wave) * KSM + tile) * 64 + lane] = xt_frag(Qs, 256, 16 * wave);
            kloop_run<MF, 4, 1, 0, 4, 256, DP>(h, rp, Qs, wproj, KS1, head * 4);
            __syncthreads();
        }
        exchange(h);
        residual(S.hA, fa);
        // ---- MLP branch: member = hidden slice of 256 --------------------------------------------------------------------------------------
        const int c = member;
        const uint4* const wfc1 = (const uint4*)L.w_fc1 + ((size_t)(c * 16 + wave * 2) * KS1) * 64 + lane;
        const uint4* const wfc2 = (const uint4*)L.w_fc2 + ((size_t)(wave * 4) * KS2) * 64 + lane;
        uint4 r1[D1][2];
        kloop_prime<2, 1, KS1, D1>(r1, wfc1, KS1, 0);
        ln_branch_start(L.ln2_g, L.ln2_b, L.b_fc2, S.hM, S.meanM, S.rstdM);
        __syncthreads();
        if (member == 0 && !(a.flags & 2)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nf = wave * 4 + j;
                S.xt_ln2[((size_t)nf * KSM + tile) * 64 + lane] = xt_frag(XN, 1024, 16 * nf);
            }
        }
        {
            f32x4 a1[2][MF];
#pragma unroll
            for (int nf = 0; nf < 2; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) a1[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            kloop_run<MF, 2, 1, 0, KS1, 1024, D1>(a1, r1, XN, wfc1, KS1, 0);
            uint4 r2[D2][4];
            kloop_prime<4, 1, HC / 32, D2>(r2, wfc2, KS2, c * 8);
            char* const hb = RB;
#pragma unroll
            for (int nf = 0; nf < 2; ++nf) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(L.b_fc1 + c * HC + wave * 32 + nf * 16 + g * 4);
                const int slot = 4 * wave + 2 * nf + (g >> 1);
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    f32x4 v = a1[nf][mf] + b;
                    if (!(a.flags & 1)) *reinterpret_cast<f32x4*>(S.pre + (size_t)(m0 + mf * 16 + lr) * SYN_FF + c * HC + wave * 32 + nf * 16 + g * 4) = v;
                    v[0] = gelu_erf(v[0]); v[1] = gelu_erf(v[1]); v[2] = gelu_erf(v[2]); v[3] = gelu_erf(v[3]);
                    *reinterpret_cast<bf16x4*>(hb + (mf * 16 + lr) * 512 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(v);
                }
            }
            __syncthreads();
            // GELU output^T fragments of this slice: nf = 16 c + 2 wave + j
            if (!(a.flags & 2))
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nfl = 2 * wave + j;
                S.xt_a[((size_t)(c * 16 + nfl) * KSM + tile) * 64 + lane] = xt_frag(hb, 512, 16 * nfl);
            }
            kloop_run<MF, 4, 1, 0, HC / 32, 512, D2>(h, r2, hb, wfc2, KS2, c * 8);
        }
        __syncthreads();
        exchange(h);
        residual(S.hM, fm);
    }
    if (member == 0) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) *reinterpret_cast<f32x4*>(a.Hout + hoff(nf, mf)) = h[nf][mf];
    }
    tp_done();
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The data-gradient chain of the eight blocks as ONE persistent launch (round 5): the mirror image of k_stack_train.  Per block, backwards:
//   MLP branch   d = dh; da = (f d) . W2 (member c: its 256 hidden units) | dpre = da GELU'(pre) | dz = dpre . W1 (partial over the member's units)
//                | exchange | dh += LayerNorm2-backward(dz)
//   attention    do = (f d) . Wproj (member = head) | softmax-attention backward on the saved q, k, v (MFMA, both orientations of the 32 x 32
//                score matrix so that no register tile is ever transposed) | dz = dqkv . Wqkv (partial) | exchange | dh += LayerNorm1-backward(dz)
// Weights: the TRANSPOSED fragment sets (fragments of W^T), i.e. what `syn_linear_pair`'s data-gradient GEMM takes.
// The weight gradients are NOT formed here (their contraction runs over all rows of the batch): the kernel writes their left operands - the four
// gradients of a block as transposed bf16 matrices [features][M] - and syn_train_stack_wgrad runs the 32 GEMMs afterwards, four per launch.
// Bias / LayerNorm parameter gradients leave as per-sequence partial sums (fp32), added up over the sequences by k_colsum.
// dh between the branches lives in registers; across a branch it is parked in a per-lane slot of global memory and fetched back while the group
// barrier of the exchange is waited for (its own lane wrote it: visible once that lane's stores have drained, which the barrier's release does).
struct TrainGrad {       // one block's outputs of the backward chain
    __bf16* dyt_fc2; __bf16* dyt_fc1; __bf16* dyt_proj; __bf16* dyt_qkv;      // [512][M], [1024][M], [512][M], [1536][M]: (gradient at the Linear's output)^T
    float* part;                                                              // [tiles][kPartCols]: see kP* below
};
constexpr int kPLn2G = 0, kPLn2B = 512, kPFc2B = 1024, kPFc1B = 1536, kPLn1G = 2560, kPLn1B = 3072, kPProjB = 3584, kPartCols = 4096;
// sums of `part` over the sequences, in sequence order, each of the seven segments into its own tensor (the gradients autograd adopts without a copy)
struct SmallOut { const float* part[SYN_LAYERS]; float* p[SYN_LAYERS][7]; };
__global__ void k_part_sums(int n_part, int l0, SmallOut o) {    // grid (16, blocks): one launch for the blocks l0 .. l0 + gridDim.y - 1
    const int c = blockIdx.x * blockDim.x + threadIdx.x, l = l0 + blockIdx.y;
    if (c >= kPartCols) return;
    const float* const part = o.part[l];
    float s = 0.f;
#pragma unroll 8
    for (int p = 0; p < n_part; ++p) s += part[(size_t)p * kPartCols + c];
    const int seg = c < 1536 ? c >> 9 : (c < 2560 ? 3 : 4 + ((c - 2560) >> 9)), base = c < 1536 ? (c >> 9) << 9 : (c < 2560 ? 1536 : 2560 + (((c - 2560) >> 9) << 9));
    o.p[l][seg][c - base] = s;
}

struct TArgsB {
    const float* dH;      // [M][512] gradient at the output of the last block
    float* dHin;          // [M][512] gradient at the input of the first
    syn_layer layer[SYN_LAYERS];          // w_* = fragments of W^T (w_qkv: [512][1536], w_proj: [512][512], w_fc1: [512][1024], w_fc2: [1024][512]); ln*_g as in the forward
    TrainSave save[SYN_LAYERS];           // what the forward wrote (read-only here)
    TrainGrad grad[SYN_LAYERS];
    const float* dp;
    int M, tiles;
    unsigned* sync; float* xch;
    float* stash;         // [tiles][4 members][32 * 512] fp32: dh parked across a branch
    int flags;            // diagnostics (timing only, wrong results): 1 no transposed-gradient stores, 2 no attention mathematics, 4 no bias / LayerNorm partial sums
    int l_first, l_last;  // blocks of this launch, walked downwards: l_first >= l_last (a chain cut in pieces lets the weight-gradient GEMMs of the finished
                          // blocks run on the idle half of the chip beside the next piece)
};

__device__ __forceinline__ float gelu_grad(float x) {            // d/dx [x Phi(x)] = Phi(x) + x phi(x), erf by Abramowitz & Stegun 7.1.26 as gelu_erf
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-z * z * 1.4426950408889634f);          // exp(-x^2 / 2)
    const float erf_abs = fmaf(-p * t, e, 1.0f);
    return 0.5f * (1.0f + copysignf(erf_abs, x)) + x * e * 0.3989422804014327f;
}

// (rows 8 q .. 8 q + 7 of column col) of a swizzled bf16 row tile -> one 16-byte piece of a transposed row
__device__ __forceinline__ uint4 col8(const char* base, int rowb, int col, int q) {
    unsigned short v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int r = 8 * q + e;
        v[e] = *reinterpret_cast<const unsigned short*>(base + r * rowb + ((((col >> 3) ^ (r & 15))) << 4) + (col & 7) * 2);
    }
    uint4 o;
    o.x = (unsigned)v[0] | ((unsigned)v[1] << 16); o.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
    o.z = (unsigned)v[4] | ((unsigned)v[5] << 16); o.w = (unsigned)v[6] | ((unsigned)v[7] << 16);
    return o;
}

__global__ __launch_bounds__(kThreads) void k_stack_train_bwd(const TArgsB a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MT = 32, MF = 2, P = 4, HC = 256;
    constexpr int KS1 = SYN_D / 32, KS2 = SYN_FF / 32, KS3 = 3 * SYN_D / 32;
    // LDS: DB = the branch's (f d) as bf16 rows (B operand of the first GEMM), later the attention's dq / dk / dv row tiles;
    //      RB = MLP: dpre rows [32][256]; attention: Q, K, V, dO row tiles + Q^T, K^T, dO^T
    char* const DB = smem;                                  // 32 KB
    char* const RB = smem + 32 * 1024;
    char* const Qs = RB, * const Ks = RB + 8192, * const Vs = RB + 16384, * const Os = RB + 24576;       // [32][128] bf16, swizzled 16-byte slots
    char* const QT = RB + 32768, * const KT = QT + 128 * 72, * const OT = KT + 128 * 72;                   // [128][36] bf16
    float* const stat = reinterpret_cast<float*>(OT + 128 * 72);                                           // [32 queries][4]: max, 1 / sum, dot
    float* const red = stat + 128;                                                                           // row reductions: 32 x 16 floats
    char* const DQs = DB, * const DKs = DB + 8192, * const DVs = DB + 16384;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, lr = lane & 15;
    __shared__ int s_rank;
    const int xcd = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u) % lat::kGroups;
    unsigned* const xbase = a.sync + xcd * 32;
    unsigned* const gerr = a.sync + lat::kGroups * 32;
    if (tid == 0) s_rank = (int)__hip_atomic_fetch_add(xbase, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int rank = s_rank, per_xcd = (int)gridDim.x / lat::kGroups;
    if (rank >= per_xcd) {
        if (tid == 0) __hip_atomic_store(gerr, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int member = rank % P, tile = xcd + lat::kGroups * (rank / P);
    unsigned* const gctr = xbase + 2 + rank / P;
    unsigned gphase = 0;
    auto tp_done = [&]() {
        if (tid == 0) {
            if (__hip_atomic_fetch_add(xbase + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)per_xcd - 1)
                for (int i = 0; i < 32; ++i) __hip_atomic_store(xbase + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (tile >= a.tiles) { tp_done(); return; }
    const int m0 = tile * MT;
    const int M = a.M;
    float* const park = a.stash + ((size_t)(tile * P + member) * kThreads) * 32;      // 8 x f32x4 per thread
    auto hoff = [&](int nf, int mf) { return (size_t)(m0 + mf * 16 + lr) * kNT + wave * 64 + nf * 16 + g * 4; };
    // partial sums of the four members in member order
    // `hx` (the LayerNorm input of this lane's fragments, read-only data of the forward) is requested while the group barrier is waited for;
    // `keep` (this lane's parked dh) once the partials' registers are free again - its latency hides behind the LayerNorm backward's row reductions
    auto exchange = [&](f32x4 (&hh)[4][MF], f32x4 (&keep)[4][MF], f32x4 (&hx)[4][MF], const float* hsrc) {
        int et = tid;
        asm volatile("" : "+v"(et));
        float* const set = a.xch + ((size_t)(tile * 2 + (int)(gphase & 1u)) * 4) * (MT * 512) + et * 4;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
                *reinterpret_cast<f32x4*>(set + (size_t)member * (MT * 512) + (nf * MF + mf) * 2048) = hh[nf][mf];
        lat::group_release();                     // (vmcnt(0): the parked dh of this lane is in L2 as well)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) hx[nf][mf] = *reinterpret_cast<const f32x4*>(hsrc + hoff(nf, mf));
        __builtin_amdgcn_sched_barrier(0);
        ++gphase;
        lat::group_wait(gctr, gphase * (unsigned)P, gerr);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[P][2][MF];
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                    for (int mf = 0; mf < MF; ++mf)
                        if (j != member)
                            v[j][n2][mf] = lat::ld_xcd(reinterpret_cast<const f32x4*>(set + (size_t)j * (MT * 512) + ((half * 2 + n2) * MF + mf) * 2048));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    const f32x4 own = hh[half * 2 + n2][mf];
                    f32x4 sum = member == 0 ? own : v[0][n2][mf];
#pragma unroll
                    for (int j = 1; j < P; ++j) sum = sum + (j == member ? own : v[j][n2][mf]);
                    hh[half * 2 + n2][mf] = sum;
                }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) keep[nf][mf] = lat::ld_xcd(reinterpret_cast<const f32x4*>(park + ((nf * MF + mf) * kThreads + et) * 4));
        __builtin_amdgcn_sched_barrier(0);
    };
    // column sums over the tile's 32 rows of a [4][MF] fragment set -> out[64 wave + 16 nf + 4 g + e] (this wave's 64 columns)
    auto col_sums = [&](const f32x4 (&v)[4][MF], float* out) {
        if (a.flags & 4) return;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            f32x4 s = v[nf][0] + v[nf][1];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += __shfl_xor(s[e], o);
            if (lr == 0) *reinterpret_cast<f32x4*>(out + wave * 64 + nf * 16 + g * 4) = s;
        }
    };
    // start of a branch: park dh, DB = bf16(f dh) rows, its transpose -> the weight-gradient operand of the branch's LAST Linear, bias gradient partial
    auto branch_start = [&](f32x4 (&dh)[4][MF], float f, __bf16* dyt, float* bias_part) {
        int et = tid;
        asm volatile("" : "+v"(et));
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int slot = 8 * wave + 2 * nf + (g >> 1);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                *reinterpret_cast<f32x4*>(park + ((nf * MF + mf) * kThreads + et) * 4) = dh[nf][mf];
                dh[nf][mf] = dh[nf][mf] * f;
                *reinterpret_cast<bf16x4*>(DB + (mf * 16 + lr) * 1024 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(dh[nf][mf]);
            }
        }
        if (member == 3) col_sums(dh, bias_part);               // (identical in every member: one of them writes)
        __syncthreads();
        if (!(a.flags & 1)) {   // (f d)^T: member j writes feature rows 128 j .. + 127, a thread 8 of the tile's 32 columns of one row
            const int col = 128 * member + (et & 127), q = et >> 7;
            *reinterpret_cast<uint4*>(dyt + (size_t)col * M + m0 + 8 * q) = col8(DB, 1024, col, q);
        }
    };
    // LayerNorm backward over the exchanged dz: dh = keep + rstd (t - mean(t) - xhat mean(t xhat)), t = dz gamma; parameter gradient partials
    auto ln_backward = [&](f32x4 (&dz)[4][MF], const f32x4 (&keep)[4][MF], const f32x4 (&hx)[4][MF], const float* mean_p, const float* rstd_p,
                           const float* gamma, float* pg, float* pb) {
        float mean[MF], rstd[MF];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) { mean[mf] = mean_p[m0 + mf * 16 + lr]; rstd[mf] = rstd_p[m0 + mf * 16 + lr]; }
        f32x4 xh[4][MF];
        float s1[MF] = {0.f, 0.f}, s2[MF] = {0.f, 0.f};
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const f32x4 gg = *reinterpret_cast<const f32x4*>(gamma + wave * 64 + nf * 16 + g * 4);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                xh[nf][mf] = (hx[nf][mf] - mean[mf]) * rstd[mf];
                const f32x4 t = dz[nf][mf] * gg;
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1[mf] += t[e]; s2[mf] = fmaf(t[e], xh[nf][mf][e], s2[mf]); }
            }
        }
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            s1[mf] += __shfl_xor(s1[mf], 16); s2[mf] += __shfl_xor(s2[mf], 16);
            s1[mf] += __shfl_xor(s1[mf], 32); s2[mf] += __shfl_xor(s2[mf], 32);
            if (g == 0) *reinterpret_cast<float2*>(red + (mf * 16 + lr) * 16 + wave * 2) = make_float2(s1[mf], s2[mf]);
        }
        __syncthreads();
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const f32x4* p = reinterpret_cast<const f32x4*>(red + (mf * 16 + lr) * 16);
            const f32x4 c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3];
            s1[mf] = (((c0[0] + c0[2]) + (c1[0] + c1[2])) + ((c2[0] + c2[2]) + (c3[0] + c3[2]))) * (1.0f / 512.0f);
            s2[mf] = (((c0[1] + c0[3]) + (c1[1] + c1[3])) + ((c2[1] + c2[3]) + (c3[1] + c3[3]))) * (1.0f / 512.0f);
        }
        if (member == 1) {                                      // dgamma = sum_rows dz xhat
            f32x4 pr[4][MF];
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) pr[nf][mf] = dz[nf][mf] * xh[nf][mf];
            col_sums(pr, pg);
        }
        if (member == 2) col_sums(dz, pb);                      // dbeta = sum_rows dz
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const f32x4 gg = *reinterpret_cast<const f32x4*>(gamma + wave * 64 + nf * 16 + g * 4);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
                dz[nf][mf] = keep[nf][mf] + (dz[nf][mf] * gg - s1[mf] - xh[nf][mf] * s2[mf]) * rstd[mf];
        }
        __syncthreads();                                        // (red is reused by the next reduction)
    };
    f32x4 dh[4][MF];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) dh[nf][mf] = *reinterpret_cast<const f32x4*>(a.dH + hoff(nf, mf));
    constexpr int D1 = 6, D2 = 3, DO = 6, DP = 3;
    for (int l = a.l_first; l >= a.l_last; --l) {
        const syn_layer& L = a.layer[l];
        const TrainSave& S = a.save[l];
        const TrainGrad& G = a.grad[l];
        float* const part = G.part + (size_t)tile * kPartCols;
        const float fa = a.dp ? a.dp[(size_t)(2 * l) * a.tiles + tile] : 1.0f, fm = a.dp ? a.dp[(size_t)(2 * l + 1) * a.tiles + tile] : 1.0f;
        // ================================ MLP branch ================================
        {
            const int c = member;
            // W2^T [1024][512]: this member's hidden units c 256 + wave 32 + {0, 16}; W1^T [512][1024]: all 512 rows, k = the member's units
            const uint4* const w2t = (const uint4*)L.w_fc2 + ((size_t)(c * 16 + wave * 2) * KS1) * 64 + lane;
            const uint4* const w1t = (const uint4*)L.w_fc1 + ((size_t)(wave * 4) * KS2) * 64 + lane;
            uint4 r1[D1][2];
            kloop_prime<2, 1, KS1, D1>(r1, w2t, KS1, 0);
            f32x4 pre[2][MF];                                   // fc1's pre-activation of this member's units (in flight during the first GEMM)
#pragma unroll
            for (int nf = 0; nf < 2; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf)
                    pre[nf][mf] = *reinterpret_cast<const f32x4*>(S.pre + (size_t)(m0 + mf * 16 + lr) * SYN_FF + c * HC + wave * 32 + nf * 16 + g * 4);
            branch_start(dh, fm, G.dyt_fc2, part + kPFc2B);
            f32x4 a1[2][MF];
#pragma unroll
            for (int nf = 0; nf < 2; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) a1[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            kloop_run<MF, 2, 1, 0, KS1, 1024, D1>(a1, r1, DB, w2t, KS1, 0);          // da = (f d) . W2
            uint4 r2[D2][4];
            kloop_prime<4, 1, HC / 32, D2>(r2, w1t, KS2, c * 8);
            char* const hb = RB;
            f32x4 bs[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int nf = 0; nf < 2; ++nf) {
                const int slot = 4 * wave + 2 * nf + (g >> 1);
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = a1[nf][mf][e] * gelu_grad(pre[nf][mf][e]);
                    bs[nf] = bs[nf] + v;
                    *reinterpret_cast<bf16x4*>(hb + (mf * 16 + lr) * 512 + ((slot ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(v);
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1)
#pragma unroll
                    for (int e = 0; e < 4; ++e) bs[nf][e] += __shfl_xor(bs[nf][e], o);
                if (lr == 0) *reinterpret_cast<f32x4*>(part + kPFc1B + c * HC + wave * 32 + nf * 16 + g * 4) = bs[nf];       // fc1 bias gradient partial
            }
            __syncthreads();
            if (!(a.flags & 1)) {   // dpre^T rows c 256 .. + 255: thread -> (unit, 16 of the 32 columns)
                int et = tid;
                asm volatile("" : "+v"(et));
                const int col = et & 255, q2 = et >> 8;
                __bf16* const dst = G.dyt_fc1 + (size_t)(c * HC + col) * M + m0 + 16 * q2;
                *reinterpret_cast<uint4*>(dst) = col8(hb, 512, col, 2 * q2);
                *reinterpret_cast<uint4*>(dst + 8) = col8(hb, 512, col, 2 * q2 + 1);
            }
            f32x4 dz[4][MF];
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) dz[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            kloop_run<MF, 4, 1, 0, HC / 32, 512, D2>(dz, r2, hb, w1t, KS2, c * 8);    // dz (partial) = dpre . W1[units of c, :]
            __syncthreads();
            f32x4 hx[4][MF];
            exchange(dz, dh, hx, S.hM);
            ln_backward(dz, dh, hx, S.meanM, S.rstdM, L.ln2_g, part + kPLn2G, part + kPLn2B);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) dh[nf][mf] = dz[nf][mf];
        }
        // ================================ attention branch ================================
        {
            const int head = member;
            // Wproj^T [512][512]: rows (attention features) of this head, 16 per wave; Wqkv^T [512][1536]: all 512 rows, k = this head's q, k, v columns
            const uint4* const wpt = (const uint4*)L.w_proj + ((size_t)(head * 8 + wave) * KS1) * 64 + lane;
            const uint4* const wqt = (const uint4*)L.w_qkv + ((size_t)(wave * 4) * KS3) * 64 + lane;
            uint4 ro[DO][1];
            kloop_prime<1, 1, KS1, DO>(ro, wpt, KS1, 0);
            // q, k, v of this head, this wave's 16 features: fp32 from the forward
            f32x4 qv[3][MF];
#pragma unroll
            for (int w3 = 0; w3 < 3; ++w3)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf)
                    qv[w3][mf] = *reinterpret_cast<const f32x4*>(S.qkv + (size_t)(m0 + mf * 16 + lr) * (3 * SYN_D) + w3 * SYN_D + head * 128 + wave * 16 + g * 4);
            branch_start(dh, fa, G.dyt_proj, part + kPProjB);
            f32x4 a1[1][MF] = {{f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}};
            kloop_run<MF, 1, 1, 0, KS1, 1024, DO>(a1, ro, DB, wpt, KS1, 0);           // do = (f d) . Wproj[:, head]
            uint4 rp[DP][4];
            kloop_prime<4, 1, 4, DP>(rp, wqt, KS3, head * 4);
            // row tiles (token rows, 16-byte slots swizzled by the row) and the transposes the products over tokens take
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int row = mf * 16 + lr;
                const int off = row * 256 + ((((2 * wave) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8;
                const bf16x4 qb = to_bf16x4(qv[0][mf]), kb = to_bf16x4(qv[1][mf]), vb = to_bf16x4(qv[2][mf]), ob = to_bf16x4(a1[0][mf]);
                *reinterpret_cast<bf16x4*>(Qs + off) = qb; *reinterpret_cast<bf16x4*>(Ks + off) = kb;
                *reinterpret_cast<bf16x4*>(Vs + off) = vb; *reinterpret_cast<bf16x4*>(Os + off) = ob;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int at = (wave * 16 + g * 4 + e) * 72 + row * 2;
                    *reinterpret_cast<__bf16*>(QT + at) = qb[e]; *reinterpret_cast<__bf16*>(KT + at) = kb[e]; *reinterpret_cast<__bf16*>(OT + at) = ob[e];
                }
            }
            __syncthreads();                                    // (everybody is also past the first GEMM: DB may take dq / dk / dv now)
            const float scl = 0.08838834764831845f, scale = scl * 1.4426950408889634f;
            f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            const int half = wave & 1;
            if (a.flags & 2) {
            } else if (wave < 2) {
                // S^T[key][query] = K Q^T, dP^T = V dO^T for the queries 16 half .. + 15 (a lane: query lr, keys 16 f + 4 g + r)
                const int qrow = half * 16 + lr;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int so = (((4 * ks) + g) ^ lr) << 4;
                    const bf16x8 qf = *reinterpret_cast<const bf16x8*>(Qs + qrow * 256 + so), of = *reinterpret_cast<const bf16x8*>(Os + qrow * 256 + so);
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        sc[f] = MFMA16(*reinterpret_cast<const bf16x8*>(Ks + (f * 16 + lr) * 256 + so), qf, sc[f]);
                        dp[f] = MFMA16(*reinterpret_cast<const bf16x8*>(Vs + (f * 16 + lr) * 256 + so), of, dp[f]);
                    }
                }
                float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                float pv[2][4], sum = 0.f;
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pv[f][r] = (float)(__bf16)__builtin_amdgcn_exp2f((sc[f][r] - mx) * scale);      // (rounded as the forward's numerators were)
                        sum += pv[f][r];
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
                float dot = 0.f;
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pv[f][r] *= inv; dot = fmaf(dp[f][r], pv[f][r], dot); }
                dot += __shfl_xor(dot, 16);
                dot += __shfl_xor(dot, 32);
                if (g == 0) *reinterpret_cast<f32x4*>(stat + qrow * 4) = f32x4{mx, inv, dot, 0.f};
                bf16x8 dsT;                                      // dS^T as the B operand over keys: slot 4 f + r = key 16 f + 4 g + r
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dsT[f * 4 + r] = (__bf16)(pv[f][r] * (dp[f][r] - dot) * scl);
                // dQ^T[d][query] = sum_key K^T[d][key] dS^T[key][query] -> dq rows
#pragma unroll
                for (int df = 0; df < 8; ++df) {
                    const char* kr = KT + (16 * df + lr) * 72 + 8 * g;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(kr), hi = *reinterpret_cast<const bf16x4*>(kr + 32);
                    bf16x8 kf;
                    kf[0] = lo[0]; kf[1] = lo[1]; kf[2] = lo[2]; kf[3] = lo[3]; kf[4] = hi[0]; kf[5] = hi[1]; kf[6] = hi[2]; kf[7] = hi[3];
                    const f32x4 o = MFMA16(kf, dsT, (f32x4{0.f, 0.f, 0.f, 0.f}));
                    *reinterpret_cast<bf16x4*>(DQs + qrow * 256 + ((((2 * df) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8) = to_bf16x4(o);
                }
            } else if (wave < 4) {
                // S[query][key] = Q K^T, dP = dO V^T for the keys 16 half .. + 15 (a lane: key lr, queries 16 f + 4 g + r)
                const int krow = half * 16 + lr;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int so = (((4 * ks) + g) ^ lr) << 4;
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + krow * 256 + so), vf = *reinterpret_cast<const bf16x8*>(Vs + krow * 256 + so);
#pragma unroll
                    for (int f = 0; f < 2; ++f) {
                        sc[f] = MFMA16(*reinterpret_cast<const bf16x8*>(Qs + (f * 16 + lr) * 256 + so), kf, sc[f]);
                        dp[f] = MFMA16(*reinterpret_cast<const bf16x8*>(Os + (f * 16 + lr) * 256 + so), vf, dp[f]);
                    }
                }
            }
            __syncthreads();                                    // the queries' max / sum / dot are in `stat`
            if (!(a.flags & 2) && wave >= 2 && wave < 4) {
                const int krow = half * 16 + lr;
                bf16x8 pB, dsB;                                  // B operands over queries: slot 4 f + r = query 16 f + 4 g + r
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x4 st = *reinterpret_cast<const f32x4*>(stat + (16 * f + 4 * g + r) * 4);
                        const float pq = (float)(__bf16)__builtin_amdgcn_exp2f((sc[f][r] - st[0]) * scale) * st[1];
                        pB[f * 4 + r] = (__bf16)pq;
                        dsB[f * 4 + r] = (__bf16)(pq * (dp[f][r] - st[2]) * scl);
                    }
#pragma unroll
                for (int df = 0; df < 8; ++df) {
                    const char* orow = OT + (16 * df + lr) * 72 + 8 * g;
                    const char* qrw = QT + (16 * df + lr) * 72 + 8 * g;
                    const bf16x4 olo = *reinterpret_cast<const bf16x4*>(orow), ohi = *reinterpret_cast<const bf16x4*>(orow + 32);
                    const bf16x4 qlo = *reinterpret_cast<const bf16x4*>(qrw), qhi = *reinterpret_cast<const bf16x4*>(qrw + 32);
                    bf16x8 of, qf;
                    of[0] = olo[0]; of[1] = olo[1]; of[2] = olo[2]; of[3] = olo[3]; of[4] = ohi[0]; of[5] = ohi[1]; of[6] = ohi[2]; of[7] = ohi[3];
                    qf[0] = qlo[0]; qf[1] = qlo[1]; qf[2] = qlo[2]; qf[3] = qlo[3]; qf[4] = qhi[0]; qf[5] = qhi[1]; qf[6] = qhi[2]; qf[7] = qhi[3];
                    const f32x4 dv = MFMA16(of, pB, (f32x4{0.f, 0.f, 0.f, 0.f}));        // dV^T[d][key] = sum_query dO^T[d][query] P[query][key]
                    const f32x4 dk = MFMA16(qf, dsB, (f32x4{0.f, 0.f, 0.f, 0.f}));       // dK^T[d][key] = sum_query Q^T[d][query] dS[query][key]
                    const int off = krow * 256 + ((((2 * df) + (g >> 1)) ^ lr) << 4) + (g & 1) * 8;
                    *reinterpret_cast<bf16x4*>(DVs + off) = to_bf16x4(dv);
                    *reinterpret_cast<bf16x4*>(DKs + off) = to_bf16x4(dk);
                }
            }
            __syncthreads();
            if (!(a.flags & 1)) {   // dqkv^T rows of this head: thread -> (which of q / k / v, feature, 32 columns); 384 of the 512 threads
                int et = tid;
                asm volatile("" : "+v"(et));
                if (et < 384) {
                    const int w3 = et >> 7, col = et & 127;
                    const char* const src = DB + w3 * 8192;
                    __bf16* const dst = G.dyt_qkv + (size_t)(w3 * SYN_D + head * 128 + col) * M + m0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4*>(dst + 8 * q) = col8(src, 256, col, q);
                }
            }
            f32x4 dz[4][MF];
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) dz[nf][mf] = f32x4{0.f, 0.f, 0.f, 0.f};
            // dz (partial) = dq . Wq[head rows, :] + dk . Wk[...] + dv . Wv[...]: three K pieces of 128
            kloop_run<MF, 4, 1, 0, 4, 256, DP>(dz, rp, DQs, wqt, KS3, head * 4);
            kloop_prime<4, 1, 4, DP>(rp, wqt, KS3, 16 + head * 4);
            kloop_run<MF, 4, 1, 0, 4, 256, DP>(dz, rp, DKs, wqt, KS3, 16 + head * 4);
            kloop_prime<4, 1, 4, DP>(rp, wqt, KS3, 32 + head * 4);
            kloop_run<MF, 4, 1, 0, 4, 256, DP>(dz, rp, DVs, wqt, KS3, 32 + head * 4);
            __syncthreads();
            f32x4 hx[4][MF];
            exchange(dz, dh, hx, S.hA);
            ln_backward(dz, dh, hx, S.meanA, S.rstdA, L.ln1_g, part + kPLn1G, part + kPLn1B);
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) dh[nf][mf] = dz[nf][mf];
        }
    }
    if (member == 0) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) *reinterpret_cast<f32x4*>(a.dHin + hoff(nf, mf)) = dh[nf][mf];
    }
    tp_done();
}

constexpr int kTrainBwdLds = 32 * 1024 + 32768 + 3 * 128 * 72 + 512 + 32 * 16 * 4 + 64;

}  // namespace stk
}  // namespace

// ---- entry points (include/syn_hip.h) ----------------------------------------------------------------------------------------------------
extern "C" {

int syn_train_stack_fwd(const syn_train_stack* t, void* stream) {
    if (!t || !t->h_in || !t->h_out || !t->sync || !t->xch || t->n_seq < 1 || t->n_seq > 64) return fail_msg("syn_train_stack_fwd: 1 .. 64 sequences, non-null pointers");
    if (!latency_path_ok()) return fail_msg("syn_train_stack_fwd: needs a 256-CU (8 XCD x 32) device");
    stk::TArgsS a;
    memset(&a, 0, sizeof(a));
    a.H = t->h_in; a.Hout = t->h_out; a.dp = t->drop_path; a.M = 32 * t->n_seq; a.tiles = t->n_seq; a.sync = t->sync; a.xch = t->xch; a.flags = t->reserved;
    for (int l = 0; l < SYN_LAYERS; ++l) {
        const syn_layer& L = t->layer[l];
        const syn_train_block_save& S = t->save[l];
        if (!L.ln1_g || !L.ln1_b || !L.w_qkv || !L.w_proj || !L.b_proj || !L.ln2_g || !L.ln2_b || !L.w_fc1 || !L.b_fc1 || !L.w_fc2 || !L.b_fc2)
            return fail_msg("syn_train_stack_fwd: a block's weights are incomplete");
        if (!S.h_attn || !S.mean_attn || !S.rstd_attn || !S.qkv || !S.xt_ln1 || !S.xt_attn || !S.h_mlp || !S.mean_mlp || !S.rstd_mlp || !S.pre || !S.xt_ln2 || !S.xt_gelu)
            return fail_msg("syn_train_stack_fwd: a block's saved tensors are incomplete");
        a.layer[l] = L;
        stk::TrainSave& d = a.save[l];
        d.hA = S.h_attn; d.meanA = S.mean_attn; d.rstdA = S.rstd_attn; d.qkv = S.qkv; d.xt_ln1 = (uint4*)S.xt_ln1; d.xt_o = (uint4*)S.xt_attn;
        d.hM = S.h_mlp; d.meanM = S.mean_mlp; d.rstdM = S.rstd_mlp; d.pre = S.pre; d.xt_ln2 = (uint4*)S.xt_ln2; d.xt_a = (uint4*)S.xt_gelu;
    }
    static OncePerDevice once;
    if (once.first()) { allow_lds(stk::k_stack_train, stk::kTrainLds); }
    const int grid = lat::kGroups * 4 * ((t->n_seq + lat::kGroups - 1) / lat::kGroups);
    hipLaunchKernelGGL(stk::k_stack_train, dim3(grid), dim3(kThreads), stk::kTrainLds, (hipStream_t)stream, a);
    return launched("k_stack_train launch");
}

int syn_train_stack_bwd(const syn_train_stack_grad* t, void* stream) {
    if (!t || !t->fwd || !t->dh_out || !t->dh_in || !t->stash) return fail_msg("syn_train_stack_bwd: null argument");
    const syn_train_stack& f = *t->fwd;
    if (f.n_seq < 1 || f.n_seq > 64 || !f.sync || !f.xch) return fail_msg("syn_train_stack_bwd: 1 .. 64 sequences, the forward's sync / xch");
    if (!latency_path_ok()) return fail_msg("syn_train_stack_bwd: needs a 256-CU (8 XCD x 32) device");
    stk::TArgsB a;
    memset(&a, 0, sizeof(a));
    a.dH = t->dh_out; a.dHin = t->dh_in; a.dp = f.drop_path; a.M = 32 * f.n_seq; a.tiles = f.n_seq; a.sync = f.sync; a.xch = f.xch; a.stash = t->stash;
    a.l_first = t->first_block; a.l_last = t->last_block; a.flags = f.reserved;
    if (a.l_first < a.l_last || a.l_last < 0 || a.l_first >= SYN_LAYERS) return fail_msg("syn_train_stack_bwd: blocks are walked downwards: SYN_LAYERS > first_block >= last_block >= 0");
    for (int l = 0; l < SYN_LAYERS; ++l) {
        const syn_layer& L = t->layer_t[l];
        const syn_train_block_save& S = f.save[l];
        const syn_train_block_grad& G = t->grad[l];
        if (!L.ln1_g || !L.w_qkv || !L.w_proj || !L.ln2_g || !L.w_fc1 || !L.w_fc2) return fail_msg("syn_train_stack_bwd: a block's transposed weights / LayerNorm gains are incomplete");
        if (!G.dyt_fc2 || !G.dyt_fc1 || !G.dyt_proj || !G.dyt_qkv || !G.part) return fail_msg("syn_train_stack_bwd: a block's outputs are incomplete");
        a.layer[l] = L;
        stk::TrainSave& d = a.save[l];
        d.hA = S.h_attn; d.meanA = S.mean_attn; d.rstdA = S.rstd_attn; d.qkv = S.qkv; d.xt_ln1 = (uint4*)S.xt_ln1; d.xt_o = (uint4*)S.xt_attn;
        d.hM = S.h_mlp; d.meanM = S.mean_mlp; d.rstdM = S.rstd_mlp; d.pre = S.pre; d.xt_ln2 = (uint4*)S.xt_ln2; d.xt_a = (uint4*)S.xt_gelu;
        stk::TrainGrad& o = a.grad[l];
        o.dyt_fc2 = (__bf16*)G.dyt_fc2; o.dyt_fc1 = (__bf16*)G.dyt_fc1; o.dyt_proj = (__bf16*)G.dyt_proj; o.dyt_qkv = (__bf16*)G.dyt_qkv; o.part = G.part;
    }
    static OncePerDevice once;
    if (once.first()) { allow_lds(stk::k_stack_train_bwd, stk::kTrainBwdLds); }
    const int grid = lat::kGroups * 4 * ((f.n_seq + lat::kGroups - 1) / lat::kGroups);
    hipLaunchKernelGGL(stk::k_stack_train_bwd, dim3(grid), dim3(kThreads), stk::kTrainBwdLds, (hipStream_t)stream, a);
    return launched("k_stack_train_bwd launch");
}

// The weight gradients the backward chain left open: per block dW = dY^T . X for its four Linears - dY^T from syn_train_stack_bwd ([features][M] bf16),
// X^T fragments from the forward - four GEMMs per launch; then the per-sequence partial sums of the bias / LayerNorm gradients added up.
int syn_train_stack_wgrad(const syn_train_stack_grad* t, void* stream) {
    if (!t || !t->fwd) return fail_msg("syn_train_stack_wgrad: null argument");
    const syn_train_stack& f = *t->fwd;
    const int M = 32 * f.n_seq;
    if (f.n_seq < 1 || f.n_seq > 64 || M % 128) return fail_msg("syn_train_stack_wgrad: the row count must be a multiple of 128 (4 sequences)");
    n128_setup();
    hipStream_t s = (hipStream_t)stream;
    stk::SmallOut so;
    memset(&so, 0, sizeof(so));
    if (t->first_block < t->last_block || t->last_block < 0 || t->first_block >= SYN_LAYERS) return fail_msg("syn_train_stack_wgrad: SYN_LAYERS > first_block >= last_block >= 0");
    GQuadAll q;
    memset(&q, 0, sizeof(q));
    const int ns[4] = {512, 1024, 512, 1536}, ks[4] = {1024, 512, 512, 512};           // dW [n][k]: fc2, fc1, proj, qkv
    int lds = 0;
    for (int i = 0; i < 4; ++i) {
        const int mt = pick_mt128(ns[i], ks[i], M, 8);                // (64-row tiles for all four: 126 us for 8 launches against 182 with proj on 32-row tiles)
        if (!mt) return fail_msg("syn_train_stack_wgrad: row count too large for the resident GEMM");
        q.ns[i] = ns[i]; q.ks[i] = ks[i]; q.mt[i] = mt; q.gx[i] = (ns[i] + mt - 1) / mt;
        q.cum[i + 1] = q.cum[i] + q.gx[i] * (ks[i] / 128);
        lds = mt * M * 2 > lds ? mt * M * 2 : lds;
    }
    q.M = M; q.l0 = t->last_block;
    for (int l = t->last_block; l <= t->first_block; ++l) {
        const syn_train_block_save& S = f.save[l];
        const syn_train_block_grad& G = t->grad[l];
        if (!G.dw_fc2 || !G.dw_fc1 || !G.dw_proj || !G.dw_qkv || !G.d_ln2_g || !G.d_ln2_b || !G.d_fc2_b || !G.d_fc1_b || !G.d_ln1_g || !G.d_ln1_b || !G.d_proj_b) return fail_msg("syn_train_stack_wgrad: a block's gradient buffers are incomplete");
        const void* xs[4] = {G.dyt_fc2, G.dyt_fc1, G.dyt_proj, G.dyt_qkv};
        const void* ws[4] = {S.xt_gelu, S.xt_ln2, S.xt_attn, S.xt_ln1};
        float* ys[4] = {G.dw_fc2, G.dw_fc1, G.dw_proj, G.dw_qkv};
        for (int i = 0; i < 4; ++i) { q.X[l][i] = (const __bf16*)xs[i]; q.W[l][i] = (const uint4*)ws[i]; q.Y[l][i] = ys[i]; }
        // bias / LayerNorm gradients: column sums over the sequences, in sequence order
        float* const outs[7] = {G.d_ln2_g, G.d_ln2_b, G.d_fc2_b, G.d_fc1_b, G.d_ln1_g, G.d_ln1_b, G.d_proj_b};
        so.part[l] = G.part;
        for (int i = 0; i < 7; ++i) so.p[l][i] = outs[i];
    }
    // every block's four weight-gradient GEMMs in ONE launch (k_gemm_quad_all)
    hipLaunchKernelGGL(k_gemm_quad_all, dim3(q.cum[4] * (t->first_block - t->last_block + 1)), dim3(kThreads), lds, s, q);
    hipLaunchKernelGGL(stk::k_part_sums, dim3((stk::kPartCols + 255) / 256, t->first_block - t->last_block + 1), dim3(256), 0, s, f.n_seq, t->last_block, so);
    return launched("syn_train_stack_wgrad");
}

}  // extern "C"
