// syn_latency.inc — small-batch (latency) path of the denoising step.  Included by syn_kernels.hip.
//
// k_stack keeps a 32/64-row tile of tokens resident in one CU and streams ALL weights (38 MB per step)
// through that CU: perfect when there are >= 256 tiles, but at B = 1 (the reference's real sampling case:
// test.py / demo.py denoise one 128-frame window at a time, diffusion_rvqvae_trainer.py:413-531) one CU
// works and 255 idle, and the step takes as long as one CU needs to pull 38 MB through its 64 B/clk L1.
//
// k_lat turns the decomposition around for few rows: the OUTPUT FEATURES of every GEMM are split over the
// 32 CUs of an XCD, the (few) token rows are shared.  One persistent kernel, 8 groups x 32 workgroups:
//   * group = blockIdx % 8.  Workgroups are dispatched round-robin over the 8 XCDs, so a group sits on ONE
//     XCD: the activations it exchanges between phases (h, q/k/v, MLP hidden: a few hundred KB) never leave
//     that XCD's L2, and the group barrier is an atomic in that L2.  Group g owns clips [B g/8, B (g+1)/8)
//     with all their guidance variants - no traffic between groups at all (B = 8 uses all 8 XCDs).
//   * phase = one GEMM (plus what can be fused on its input/output side); workgroup p owns 16-feature MFMA
//     tiles {p, p+32, ..} of that GEMM for ALL rows of the group, so every weight byte is read by exactly
//     one CU per XCD.  Row-wise operations that need a whole 512-wide row (LayerNorm, attention) are
//     recomputed redundantly by every workgroup from the L2-resident activations: that is ~2 MFLOP per
//     sequence and removes two barriers per block.
//       in : h = rotary(x_t.A^T + cond + te[t])                 | 8 x { qkv = LN1(h).Wqkv^T
//       | h += attention(q,k,v).Wproj^T + b | hid = gelu(LN2(h).W1^T + b1) | h += hid.W2^T + b2 }
//       | out: x0 = (sum_v w_v h_v).Wout^T + b; posterior / DDIM update; Philox noise
//     = 34 phases, 33 group barriers per step.
//   * inside a phase, a wave computes units (feature tile, 16-token tile, K part); K is split over waves so
//     that all 8 waves work even with a single sequence, partial sums are reduced through LDS in a FIXED
//     order (results do not depend on how many sequences the group holds: batch rows stay independent
//     bit for bit).  Weight fragments and activation fragments are loaded straight into MFMA operand
//     registers (global -> VGPR); only LayerNorm / attention outputs go through LDS.
// Arithmetic is the same as k_stack's (bf16 operands, fp32 accumulate, fp32 residual stream / LayerNorm /
// softmax, q, k, v, p and o rounded to bf16): the two paths agree to fp32-reassociation level, not bitwise.
//
// Co-residency: the group barrier needs all 32 workgroups of a group running.  256 workgroups x 80 KB LDS
// fit the 256 CUs when the device runs nothing else; the wait is bounded (kSpinLimit) and raises a sticky
// error flag (sync[kGroups*32]) instead of hanging if that assumption is broken.

namespace lat {

constexpr int kGroups = 8;
constexpr int kP = 32;                 // workgroups per group (= CUs per XCD)
constexpr int kSpinLimit = 1 << 21;
constexpr int kXnBytes = 64 * 1024;    // 64 rows x 1024 B
constexpr int kRedBytes = 64 * 1024;   // 8 waves x 2 accumulators x 4 token tiles x 64 lanes x 16 B
constexpr int kLds = kXnBytes + kRedBytes;

struct LArgs {
    const uint4* w_in; const float* te; const float* rcos; const float* rsin;
    syn_layer layer[SYN_LAYERS];
    const uint4* w_out; const float* b_out;
    int B, V;
    const float* cond; const int* t_model; const float* cfg_w; int cfg_stride;
    const __bf16* xb; const float* xt; const float* noise; const unsigned long long* rng;
    const float* coef; const int* t_coef;
    float* xn; __bf16* xnb; float* x0;
    const unsigned char* keep; const float* known;      // in-painting (syn_denoise_step_edit): x0 = keep ? known : x0, or both NULL
    float* H; __bf16* Q; __bf16* Kb; __bf16* Vt; __bf16* HID;
    float* X0v;                        // != nullptr: per-sequence groups; the output stage writes x0_hat of every variant here
                                       // ([V*B*32][1536] fp32) and k_guided_update combines them and applies the step
    unsigned* sync;                    // [kGroups][32] u32: {arrivals, finished, ranks}; [kGroups*32] = sticky error flag
    long long* dbg;
};

// threadIdx.x behind an opaque asm: everything derived from it (lane offsets, fragment addresses) is recomputed where
// it is used instead of being hoisted out of the 8-block loop by hipcc and parked in scratch for the whole kernel
// NB: wave-level control flow must stay SCALAR (readfirstlane of tid >> 6).  With the wave index left in a VGPR
// hipcc treats `if (wave < units)` / the A-B operand swap as divergent and predicates the MFMAs through EXEC;
// that build produced wrong token tiles 2-3 (observed, bisected) whenever the weights were not waited for
// right before the MFMAs.
__device__ __forceinline__ int opaque_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// Loads of data another workgroup of the group wrote earlier in this launch.  A CU's vector L1 is never refreshed by another
// CU's stores and `buffer_inv sc0` does not drop it (tests/test_gpu_kernels.py::test_group_barrier_acquire_under_adversarial_
// reuse: 100 % stale on an L1-resident hand-off, exactly like no instruction at all), while the agent-scope invalidate costs
// ~14 us per barrier here.  So these loads simply do not use the L1: non-temporal loads are served by the XCD's L2, which
// is where the producers' stores are once their vmcnt has drained (0 stale words in the same test).
template <typename T>
__device__ __forceinline__ T ld_xcd(const T* p) { return __builtin_nontemporal_load(p); }

struct Grp {
    int c0, nc, ns, B;                 // first clip, clips, sequences of this group; total clips
    int n0;                            // >= 0: the group owns the sequences n0 .. n0 + ns - 1 of the V*B (guided batches,
                                       // one variant of one clip = one unit of work; nc = 0); < 0: whole clips c0 .. c0 + nc - 1
    // index of local sequence s in the [V*B] sequence tensors (sequence v*B + clip)
    __device__ __forceinline__ int seq(int s) const {
        if (n0 >= 0) return n0 + s;
        const int v = s / nc;
        return v * B + c0 + (s - v * nc);
    }
};

// Barrier of the workgroups of ONE XCD.  They share that XCD's L2, which is the coherence point for everything
// they exchange: a store is visible to the group once it is acknowledged by L2 (vmcnt == 0), and readers fetch the
// exchanged tensors past their CU's L1 (ld_xcd).  No L2 write-back / invalidate as an agent-scope fence would do
// (buffer_wbl2 + buffer_inv sc1 measured ~15 us per barrier here and evict the weights besides).  Membership of
// the group is the hardware XCC id, not an assumption about the dispatcher (see k_lat).
// Split in two so that loads which do not depend on the other workgroups (the NEXT phase's weights, LayerNorm
// parameters, biases: all cold, HBM latency) are issued between release and wait and fly during the wait.
__device__ __forceinline__ void group_release() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // compiler ordering; the hardware part is the wait below
    __builtin_amdgcn_s_waitcnt(0);                               // vmcnt(0): this wave's stores are in L2
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void group_wait(unsigned* ctr, unsigned target, unsigned* err) {
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    if (threadIdx.x == 0) {
        // vmcnt retires in order, so the first poll also waits out this wave's own prefetched (HBM-latency) loads:
        // the barriers that prefetch most show ~2k cycles more wait.  Tried and rejected: polling through the
        // scalar path (s_load glc: ~3x slower per poll), letting wave 0 prefetch after the wait (its loads then sit
        // on the critical path), prefetching a whole phase ahead (SYN_LAT_EARLY: the phase's own L2 loads queue
        // behind the cold ones, 176 -> 184..205 us).
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int n = 0;
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if ((++n & 255) == 0 &&
                (n > kSpinLimit || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
    // no cache maintenance here: everything the members exchange is read with L1-bypassing loads (ld_xcd), the weights and
    // parameters they share are read-only for the whole launch
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- adversarial check of the group's hand-off ---------------------------------------------------------------------------
// What a consumer CU must do to see what another CU of its XCD published ("stores acknowledged by L2, then a flag"), measured
// in the form /opt/skills/guides/MI355X_MICROARCH.md prescribes: consumer L1-WARM (it re-reads the same <= 16 KB every round),
// every word checked, uneven load (the other workgroups of the XCD stream from HBM), a new payload every round, one producer /
// consumer pair per XCD.  mode 0: plain loads, no invalidate; 1: `buffer_inv sc0` (what round 1's barrier relied on);
// 2: `buffer_inv sc1`; 3: non-temporal loads, no invalidate (what ld_xcd does); 4: sc1 loads through a buffer descriptor.
// Result on MI355X: modes 0 and 1 read 100 % stale words after the first round, modes 2, 3 and 4 never read one.
// stale[xcd] = words that were read with an older round's value.
struct HArgs { unsigned* sync; unsigned* buf; const float* stream; long stream_n; unsigned* stale; int words, rounds, mode; };

__global__ __launch_bounds__(512) void k_handoff_stress(const HArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // sized to force one workgroup per CU
    __shared__ int s_rank;
    const int tid = threadIdx.x;
    const int xcd = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u) % kGroups;
    unsigned* const st = a.sync + xcd * 32;          // [0] rank allocation, [1] flag (round published), [2] ack (round consumed), [3] done
    if (tid == 0) s_rank = (int)__hip_atomic_fetch_add(st, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int rank = s_rank;
    unsigned* const buf = a.buf + (size_t)xcd * 4096;
    auto value = [](unsigned r, unsigned i) { return r * 2654435761u + i * 40503u + 17u; };
    auto spin = [&](unsigned* w, unsigned target) {
        int n = 0;
        while (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target && ++n < kSpinLimit) __builtin_amdgcn_s_sleep(1);
        return n < kSpinLimit;
    };
    if (rank == 0) {                                 // producer
        for (int r = 1; r <= a.rounds; ++r) {
            for (int i = tid; i < a.words; i += 512) buf[i] = value((unsigned)r, (unsigned)i);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_waitcnt(0);           // stores acknowledged by L2 (group_release)
            __syncthreads();
            if (tid == 0) {
                __hip_atomic_store(st + 1, (unsigned)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!spin(st + 2, (unsigned)r)) break;
            }
            __syncthreads();
        }
        if (tid == 0) __hip_atomic_store(st + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (rank == 1) {                          // consumer: the same addresses every round -> L1-resident
        unsigned bad = 0;
        for (int r = 1; r <= a.rounds; ++r) {
            if (tid == 0) spin(st + 1, (unsigned)r);
            __syncthreads();
            if (a.mode == 1) asm volatile("buffer_inv sc0" ::: "memory");
            if (a.mode == 2) asm volatile("buffer_inv sc1" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (a.mode == 3) {          // no invalidate, loads that bypass L1: non-temporal
                for (int i = tid; i < a.words; i += 512) bad += __builtin_nontemporal_load(buf + i) != value((unsigned)r, (unsigned)i);
            } else if (a.mode == 4) {   // no invalidate, sc1 loads through a buffer descriptor
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(buf, 0, 4096 * 4, 0x00020000);
                for (int i = tid; i < a.words; i += 512)
                    bad += (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rs, i * 4, 0, 16) != value((unsigned)r, (unsigned)i);
            } else
            for (int i = tid; i < a.words; i += 512) bad += buf[i] != value((unsigned)r, (unsigned)i);
            __syncthreads();
            if (tid == 0) __hip_atomic_store(st + 2, (unsigned)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (bad) atomicAdd(a.stale + xcd, bad);
    } else if (a.stream) {                           // everybody else: HBM streaming load on this XCD until the pair is done
        float acc = 0.f;
        long i = ((long)blockIdx.x * 512 + tid) * 4;
        while (__hip_atomic_load(st + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            for (int k = 0; k < 64; ++k) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(a.stream + (i % (a.stream_n - 4)));
                acc += v[0] + v[3];
                i += 256L * 512 * 4;
            }
        }
        if (acc == 12345.678f) a.stale[8] = 1;       // keeps the loads alive
    }
    (void)smem;
}

// ---- staging into LDS: bf16 rows of 1024 B, 16-byte slot s of row r stored at slot ^ (r & 15) ---------------
// all-reduce over the 16 lanes of a DPP row; every lane ends with the bitwise identical sum (each step adds the
// two halves' values, a + b == b + a)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);     // row_half_mirror: the other quad of the 8-lane half
    v += dpp_mov<0x140>(v);     // row_mirror: the other half of the row
    return v;
}

// LayerNorm parameters of this lane: features 4j + 64i .. +3, j = lane & 15 (prefetched before the barrier)
struct LnParams { f32x4 g[8], b[8]; };
__device__ __forceinline__ void ln_prefetch(LnParams& P, const float* __restrict__ gam, const float* __restrict__ bet) {
    const int j = opaque_tid() & 15;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        P.g[i] = *reinterpret_cast<const f32x4*>(gam + 4 * j + 64 * i);
        P.b[i] = *reinterpret_cast<const f32x4*>(bet + 4 * j + 64 * i);
    }
    __builtin_amdgcn_sched_barrier(0);          // issue here, not where hipcc would sink them (next to their use)
}

// LayerNorm of the rows of local sequences [s0, s0 + NSQ): 16 lanes per row (4 rows per wave and pass), so the
// row statistics need 4 DPP steps instead of a 6-level LDS butterfly; all loads go out back to back.
template <int NSQ>
__device__ __forceinline__ void stage_ln_rows(const float* H, const Grp& G, int s0, const LnParams& P, char* XN) {
    const int tid = opaque_tid(), lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 15, rg = lane >> 4;
    f32x4 x[NSQ][8];
#pragma unroll
    for (int q = 0; q < NSQ; ++q) {
        const float* hp = H + ((size_t)G.seq(s0 + q) * 32 + 4 * wave + rg) * SYN_D + 4 * j;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[q][i] = ld_xcd(reinterpret_cast<const f32x4*>(hp + 64 * i));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < NSQ; ++q) {
        float s = 0.f, sq = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) { s += x[q][i][e]; sq = fmaf(x[q][i][e], x[q][i][e], sq); }
        s = row16_sum(s);
        sq = row16_sum(sq);
        const float mean = s * (1.0f / 512.0f);
        const float var = fmaxf(sq * (1.0f / 512.0f) - mean * mean, 0.f);
        const float rstd = rsqrtf(var + 1e-5f);                     // nn.LayerNorm: biased variance, eps 1e-5
        const int r = 32 * q + 4 * wave + rg;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 y = (x[q][i] - mean) * rstd * P.g[i] + P.b[i];
            *reinterpret_cast<bf16x4*>(XN + r * 1024 + (((8 * i + (j >> 1)) ^ (r & 15)) << 4) + (j & 1) * 8) = to_bf16x4(y);
        }
    }
}
__device__ __forceinline__ void stage_ln(const float* H, const Grp& G, int s0, int nsq, const LnParams& P, char* XN) {
    if (nsq == 2) stage_ln_rows<2>(H, G, s0, P, XN);
    else stage_ln_rows<1>(H, G, s0, P, XN);
}

// bf16(sum_v w[v] * h_v) of the rows of local clips [cl0, cl0 + ncl) (w == nullptr: single variant, plain copy).
__device__ __forceinline__ void stage_combine(const float* H, const Grp& G, int V, int cl0, int ncl, const float* w, int w_stride, char* XN) {
    const int tid = opaque_tid(), lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int r = wave; r < ncl * 32; r += 8) {
        const int clip = G.c0 + cl0 + (r >> 5);
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        for (int v = 0; v < V; ++v) {
            const float* hp = H + ((size_t)(v * G.B + clip) * 32 + (r & 31)) * SYN_D + lane * 8;
            const float wv = w ? w[(size_t)clip * w_stride + v] : 1.0f;
            a0 = a0 + ld_xcd(reinterpret_cast<const f32x4*>(hp)) * wv;
            a1 = a1 + ld_xcd(reinterpret_cast<const f32x4*>(hp + 4)) * wv;
        }
        bf16x8 o8;
        o8[0] = (__bf16)a0[0]; o8[1] = (__bf16)a0[1]; o8[2] = (__bf16)a0[2]; o8[3] = (__bf16)a0[3];
        o8[4] = (__bf16)a1[0]; o8[5] = (__bf16)a1[1]; o8[6] = (__bf16)a1[2]; o8[7] = (__bf16)a1[3];
        *reinterpret_cast<bf16x8*>(XN + r * 1024 + ((lane ^ (r & 15)) << 4)) = o8;
    }
}

// ---- activation-fragment sources (B operand: lane (g, lr) needs row lr, k = 32 ks + 8 g .. +7) ---------------
struct LdsTile {                       // token tile tt of the staged chunk
    const char* row;                   // XN + (16 tt + lr) * 1024
    int g, lr;
    __device__ __forceinline__ bf16x8 operator()(int ks) const {
        return *reinterpret_cast<const bf16x8*>(row + (((4 * ks + g) ^ lr) << 4));
    }
};
struct GlobalTile {                    // row-major bf16 tensor in global memory (L2)
    const __bf16* row;                 // this lane's row + 8 g
    __device__ __forceinline__ bf16x8 operator()(int ks) const { return *reinterpret_cast<const bf16x8*>(row + 32 * ks); }
};

struct XcdTile {                       // the same for a tensor other workgroups of the group wrote in this launch (hidden layer)
    const __bf16* row;
    __device__ __forceinline__ bf16x8 operator()(int ks) const {
        return __builtin_bit_cast(bf16x8, ld_xcd(reinterpret_cast<const f32x4*>(row + 32 * ks)));
    }
};

template <typename T> struct BMk_is_global { static constexpr bool value = false; };
template <> struct BMk_is_global<GlobalTile> { static constexpr bool value = true; };
template <> struct BMk_is_global<XcdTile> { static constexpr bool value = true; };

// One GEMM of a phase for a chunk of n_tt <= NTT (4: two sequences) token tiles.  Unit = (feature tile ft, K part kp):
// wave w is unit w (ft = w / KP, kp = w % KP; NFT * KP <= 8), holds its K part of the tile's weights in
// registers - loaded ONCE per phase, ahead of the group barrier, and reused for every chunk - and multiplies it
// with all token tiles of the chunk.  Partial sums go through LDS; output (ft, tt) is then summed over kp in
// fixed order and finished by wave (ft * n_tt + tt) % 8, so the epilogue work is spread over the waves too.
//   bsrc(tt): fragment source; swap(ft): tokens as the A operand (D = [token][feature], used for V so that it
//   can be written transposed); pre(ft, tt): epilogue operands (bias, residual) loaded with the GEMM operands.
template <int KS, int KP, int NACC> struct WRegs { uint4 w[NACC][KS / KP]; };

struct WTile {                          // packed weight tiles {first + stride * ft (+ acc_stride * acc)} of a matrix
    const uint4* w; int first, stride, acc_stride, ks;
    __device__ __forceinline__ const uint4* operator()(int ft, int acc) const {
        return w + (size_t)(first + stride * ft + acc_stride * acc) * ks * 64;
    }
};

template <int KS, int KP, int NFT, int NACC>
__device__ __forceinline__ void prefetch_w(WRegs<KS, KP, NACC>& R, const WTile& wt) {
    constexpr int KSU = KS / KP;
    static_assert(KS % KP == 0 && NFT * KP <= 8, "one unit per wave");
    const int tid = opaque_tid(), lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave < NFT * KP) {
        const int ft = wave / KP, kp = wave % KP;
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const uint4* W = wt(ft, a) + (size_t)(kp * KSU) * 64 + lane;
#pragma unroll
            for (int i = 0; i < KSU; ++i) R.w[a][i] = W[i * 64];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int KS, int KP, int NFT, int NACC, int NTT = 4, typename BMk, typename SwapF, typename PreF, typename Epi>
__device__ __forceinline__ void gemm_chunk(const WRegs<KS, KP, NACC>& R, int n_tt, const BMk& bsrc, const SwapF& swapf,
                                           const PreF& pre, const Epi& epi, float* RED) {
    constexpr int KSU = KS / KP;
    const int tid = opaque_tid(), lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_out = NFT * n_tt;
    // epilogue operands of this wave's first output (cold biases / L2-resident residual): in flight during the MFMAs
    decltype(pre(0, 0)) pv{};
    if (wave < n_out) pv = pre(wave / n_tt, wave % n_tt);
    if (wave < NFT * KP) {
        const int ft = wave / KP, kp = wave % KP;
        const bool sw = swapf(ft);
        f32x4 acc[NACC][NTT];
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int t = 0; t < NTT; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BMk_is_global<decltype(bsrc(0))>::value) {
            // fragments from global memory (L2): every load of the unit in flight before the first MFMA waits
            bf16x8 xf[NTT][KSU];
#pragma unroll
            for (int t = 0; t < NTT; ++t)
                if (t < n_tt) {
                    const auto b = bsrc(t);
#pragma unroll
                    for (int i = 0; i < KSU; ++i) xf[t][i] = b(kp * KSU + i);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < KSU; ++i)
#pragma unroll
                for (int t = 0; t < NTT; ++t)
                    if (t < n_tt)
#pragma unroll
                        for (int a = 0; a < NACC; ++a) {
                            const bf16x8 wf = __builtin_bit_cast(bf16x8, R.w[a][i]);
                            acc[a][t] = sw ? MFMA16(xf[t][i], wf, acc[a][t]) : MFMA16(wf, xf[t][i], acc[a][t]);
                        }
        } else {
            // fragments from LDS: read k-step by k-step (short latency, keeps the register footprint small)
#pragma unroll
            for (int i = 0; i < KSU; ++i) {
                bf16x8 xf[NTT];
#pragma unroll
                for (int t = 0; t < NTT; ++t)
                    if (t < n_tt) xf[t] = bsrc(t)(kp * KSU + i);
#pragma unroll
                for (int t = 0; t < NTT; ++t)
                    if (t < n_tt)
#pragma unroll
                        for (int a = 0; a < NACC; ++a) {
                            const bf16x8 wf = __builtin_bit_cast(bf16x8, R.w[a][i]);
                            acc[a][t] = sw ? MFMA16(xf[t], wf, acc[a][t]) : MFMA16(wf, xf[t], acc[a][t]);
                        }
            }
        }
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int t = 0; t < NTT; ++t)
                if (t < n_tt) *reinterpret_cast<f32x4*>(RED + (((wave * NACC + a) * 4 + t) * 64 + lane) * 4) = acc[a][t];
    }
    __syncthreads();
    for (int o = wave; o < n_out; o += 8) {
        const int ft = o / n_tt, tt = o - ft * n_tt;
        f32x4 r[NACC];
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            r[a] = *reinterpret_cast<const f32x4*>(RED + ((((ft * KP) * NACC + a) * 4 + tt) * 64 + lane) * 4);
#pragma unroll
            for (int kp = 1; kp < KP; ++kp)
                r[a] = r[a] + *reinterpret_cast<const f32x4*>(RED + ((((ft * KP + kp) * NACC + a) * 4 + tt) * 64 + lane) * 4);
        }
        if (o >= 8) pv = pre(ft, tt);
        epi(ft, tt, r[0], r[NACC - 1], pv);
    }
}

struct NoSwap { __device__ __forceinline__ bool operator()(int) const { return false; } };
struct NoPre { __device__ __forceinline__ int operator()(int, int) const { return 0; } };
struct Pre2 { f32x4 a, b; };

__global__ __launch_bounds__(kThreads) void k_lat(const LArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const XN = smem;
    float* const RED = reinterpret_cast<float*>(smem + kXnBytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, lr = lane & 15;
    // group = the XCD this workgroup really runs on (HW_REG_XCC_ID, bits 3:0); rank p = arrival order on that XCD.
    // The dispatcher places workgroup i on XCD i % 8, so every XCD receives exactly kP of the 8 kP workgroups;
    // if it ever does not, the surplus workgroups leave and the short group's barrier wait runs out (error flag).
    __shared__ int s_rank;
    const int grp = (int)(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 15u) % kGroups;
    unsigned* const ctr = a.sync + grp * 32;
    unsigned* const err = a.sync + kGroups * 32;
    if (tid == 0) s_rank = (int)__hip_atomic_fetch_add(ctr + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int p = s_rank;
    if (p >= kP) {
        if (tid == 0) __hip_atomic_store(err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    Grp G;
    G.B = a.B;
    if (a.X0v) {                       // guided small batch: sequences, not clips, are dealt to the XCDs
        const long nseq = (long)a.B * a.V;
        G.n0 = (int)((nseq * grp) / kGroups);
        G.ns = (int)((nseq * (grp + 1)) / kGroups) - G.n0;
        G.c0 = 0; G.nc = 0;
    } else {
        G.n0 = -1;
        G.c0 = (int)(((long)a.B * grp) / kGroups);
        G.nc = (int)(((long)a.B * (grp + 1)) / kGroups) - G.c0;
        G.ns = G.nc * a.V;
    }
    if (G.ns == 0) {                                            // fewer clips than groups: this XCD has no work
        if (tid == 0 && __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kP - 1) {
            __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    unsigned phase = 0;
    constexpr int KS1 = SYN_D / 32, KS2 = SYN_FF / 32, KSI = SYN_C / 32;
#define LSTAMP(slot) do { if (a.dbg && tid == 0) a.dbg[blockIdx.x * 64 + (slot)] = __builtin_readcyclecounter(); } while (0)
    LSTAMP(0);

    // Cold operands (weights, LayerNorm parameters: HBM latency) are requested one whole phase before their use.
    LnParams lnp;
    WRegs<KS1, 2, 1> rq;                                        // qkv: tiles p, p + 32, p + 64; 2 K parts

    // ---- in: h_v = rotary(x_t . A^T + cond_v + te[t_v]).  The product is shared by the variants of a clip.
    //      Workgroup p: feature-tile pair (u, v = u + 2 tiles) number p & 15, token tiles of parity p >> 4;
    //      8 K parts of 6 k-steps.
    {
        const int pair = p & 15, par = p >> 4;
        const int tu = 4 * (pair >> 1) + (pair & 1);            // u tile; its rotary partner is tile tu + 2
        WRegs<KSI, 8, 2> ri;
        prefetch_w<KSI, 8, 1, 2>(ri, WTile{a.w_in, tu, 0, 2, KSI});
        const __bf16* const xb = a.xb;
        const float* const cond = a.cond; const float* const te = a.te; const int* const t_model = a.t_model;
        const float* const rcos = a.rcos; const float* const rsin = a.rsin;
        float* const H = a.H;
        const int V = a.V, B = a.B;
        constexpr int INC = 2;                                  // clips per pass (register budget: 2 x 6 fragments each)
        const Grp Gc = G;
        const int n_items = G.n0 >= 0 ? G.ns : G.nc;            // sequences (each with its own clip's x_t) or clips (all variants)
        for (int cl0 = 0; cl0 < n_items; cl0 += INC) {
            const int c0 = G.c0 + cl0;
            auto clip_of = [=](int tt) { return Gc.n0 >= 0 ? (Gc.n0 + cl0 + tt) % B : c0 + tt; };
            auto bsrc = [=](int tt) {                           // rows clip * 32 + par * 16 + lr of x_t
                return GlobalTile{xb + ((size_t)clip_of(tt) * 32 + par * 16 + lr) * SYN_C + 8 * g};
            };
            auto epi = [=](int, int tt, f32x4 au, f32x4 av, int) {
                const int pos = par * 16 + lr, j = 16 * (pair & 1) + 4 * g, nu = 64 * (pair >> 1) + j;
                const f32x4 cs = *reinterpret_cast<const f32x4*>(rcos + pos * 32 + j);
                const f32x4 sn = *reinterpret_cast<const f32x4*>(rsin + pos * 32 + j);
                const int v_lo = Gc.n0 >= 0 ? 0 : 0, v_hi = Gc.n0 >= 0 ? 1 : V;
                for (int v = v_lo; v < v_hi; ++v) {
                    const int sq = Gc.n0 >= 0 ? Gc.n0 + cl0 + tt : v * B + c0 + tt;
                    const size_t row = (size_t)sq * 32 + pos;
                    const float* tp = te + (size_t)t_model[sq] * SYN_D;
                    const f32x4 u = au + *reinterpret_cast<const f32x4*>(cond + row * SYN_D + nu) + *reinterpret_cast<const f32x4*>(tp + nu);
                    const f32x4 w = av + *reinterpret_cast<const f32x4*>(cond + row * SYN_D + nu + 32) +
                                    *reinterpret_cast<const f32x4*>(tp + nu + 32);
                    *reinterpret_cast<f32x4*>(H + row * SYN_D + nu) = u * cs - w * sn;
                    *reinterpret_cast<f32x4*>(H + row * SYN_D + nu + 32) = w * cs + u * sn;
                }
            };
            gemm_chunk<KSI, 8, 1, 2, INC>(ri, min(INC, n_items - cl0), bsrc, NoSwap{}, NoPre{}, epi, RED);
            if (cl0 + INC < n_items) __syncthreads();
        }
    }
    LSTAMP(20);
#ifndef SYN_LAT_EARLY
#define SYN_LAT_EARLY 0          /* experiment knob, bit s: prefetch site s a whole phase ahead instead of before the wait */
#endif
#define PF_SITE(site, when_early, ...) do { if (((SYN_LAT_EARLY >> (site)) & 1) == (when_early)) { __VA_ARGS__ } } while (0)
#define GROUP_BARRIER(site, ...) do { group_release(); PF_SITE(site, 0, __VA_ARGS__); group_wait(ctr, ++phase * kP, err); } while (0)
#define PF_EARLY(site, ...) PF_SITE(site, 1, __VA_ARGS__)
    group_release();
    ln_prefetch(lnp, a.layer[0].ln1_g, a.layer[0].ln1_b);
    prefetch_w<KS1, 2, 3, 1>(rq, WTile{(const uint4*)a.layer[0].w_qkv, p, 32, 0, KS1});
    group_wait(ctr, ++phase * kP, err);
    LSTAMP(1);

    for (int l = 0; l < SYN_LAYERS; ++l) {
        const syn_layer L = a.layer[l];
        const int lane = opaque_tid() & 63, g = lane >> 4, lr = lane & 15;    // shadow: not hoistable out of the loop
        if (l == 3) LSTAMP(7);
        WRegs<KS1, 8, 1> rp;                                    // proj: tile p; 8 K parts of 2 k-steps
        PF_EARLY(0, prefetch_w<KS1, 8, 1, 1>(rp, WTile{(const uint4*)L.w_proj, p, 0, 0, KS1}););
        // ---- qkv = LN1(h) . Wqkv^T: tiles p (q), p + 32 (k), p + 64 (v, written transposed per sequence) ----
        for (int s0 = 0; s0 < G.ns; s0 += 2) {
            const int nsq = min(2, G.ns - s0);
            stage_ln(a.H, G, s0, nsq, lnp, XN);
            if (l == 3) LSTAMP(30);
            __syncthreads();
            if (l == 3) LSTAMP(31);
            auto bsrc = [=](int tt) { return LdsTile{XN + (16 * tt + lr) * 1024, g, lr}; };
            auto swapf = [](int ft) { return ft == 2; };
            __bf16* const Q = a.Q; __bf16* const Kb = a.Kb; __bf16* const Vt = a.Vt;
            const Grp Gc = G;
            auto epi = [=](int ft, int tt, f32x4 acc, f32x4, int) {
                const int sq = Gc.seq(s0 + (tt >> 1)), half = tt & 1;
                if (ft < 2) {
                    __bf16* dst = (ft == 0 ? Q : Kb) + ((size_t)sq * 32 + half * 16 + lr) * SYN_D + 16 * p + 4 * g;
                    *reinterpret_cast<bf16x4*>(dst) = to_bf16x4(acc);
                } else {    // acc[r] = v[token 16 half + 4g + r][feature lr]; token t of a row is stored at
                            // 8 ((t & 15) >> 2) + 4 (t >> 4) + (t & 3): the PV fragment of a lane is one 16-B load
                    *reinterpret_cast<bf16x4*>(Vt + ((size_t)sq * SYN_D + 16 * p + lr) * 32 + 8 * g + 4 * half) = to_bf16x4(acc);
                }
            };
            gemm_chunk<KS1, 2, 3, 1>(rq, 2 * nsq, bsrc, swapf, NoPre{}, epi, RED);
            if (s0 + 2 < G.ns) __syncthreads();
        }
        if (l == 3) LSTAMP(12);
        GROUP_BARRIER(0, prefetch_w<KS1, 8, 1, 1>(rp, WTile{(const uint4*)L.w_proj, p, 0, 0, KS1}););
        if (l == 3) LSTAMP(2);
        WRegs<KS1, 4, 1> r1;                                    // fc1: tiles p, p + 32; 4 K parts of 4 k-steps
        PF_EARLY(1, ln_prefetch(lnp, L.ln2_g, L.ln2_b);
                 prefetch_w<KS1, 4, 2, 1>(r1, WTile{(const uint4*)L.w_fc1, p, 32, 0, KS1}););

        // ---- h += softmax(q k^T / sqrt(128)) v . Wproj^T + b: attention of the chunk's sequences (all heads)
        //      into LDS, then projection tile p ------------------------------------------------------------
        for (int s0 = 0; s0 < G.ns; s0 += 2) {
            const int nsq = min(2, G.ns - s0);
            // q, k, v of one sequence (96 KB) are copied to LDS by all 8 waves with fully coalesced 16-byte loads
            // (q into the rows of XN that the attention output will overwrite, k and v^T into the reduction region),
            // then wave (head, query half) works out of LDS.  The L1 path (~40-64 B/clk per CU) bounds this phase:
            // per-wave global fragment loads with (head, query-half) units re-read k and v (160 KB, +4k cycles), and
            // (sequence, head) units on 4 waves read 96 KB but serialise both query halves on half of the waves.
            char* const KL = reinterpret_cast<char*>(RED);
            char* const VL = reinterpret_cast<char*>(RED) + 32 * 1024;
            for (int sl = 0; sl < nsq; ++sl) {
                const size_t sq = (size_t)G.seq(s0 + sl);
                if (sl > 0) __syncthreads();                      // k / v^T of the previous sequence are still being read
                {
                    const int t = opaque_tid();
                    uint4 qv[4], kv[4], vv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = t + kThreads * i, row = c >> 6, slot = c & 63;
                        qv[i] = __builtin_bit_cast(uint4, ld_xcd(reinterpret_cast<const f32x4*>(a.Q + (sq * 32 + row) * SYN_D + slot * 8)));
                        kv[i] = __builtin_bit_cast(uint4, ld_xcd(reinterpret_cast<const f32x4*>(a.Kb + (sq * 32 + row) * SYN_D + slot * 8)));
                        vv[i] = __builtin_bit_cast(uint4, ld_xcd(reinterpret_cast<const f32x4*>(a.Vt + sq * SYN_D * 32 + (size_t)c * 8)));
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = t + kThreads * i, row = c >> 6, slot = c & 63;
                        *reinterpret_cast<uint4*>(XN + (sl * 32 + row) * 1024 + ((slot ^ (row & 15)) << 4)) = qv[i];
                        *reinterpret_cast<uint4*>(KL + row * 1024 + ((slot ^ (row & 15)) << 4)) = kv[i];
                        *reinterpret_cast<uint4*>(VL + c * 16) = vv[i];
                    }
                }
                __syncthreads();
                {
                    const int head = wave >> 1, qh = wave & 1;
                    const int row = sl * 32 + qh * 16 + lr;
                    f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const int so = ((head * 16 + 4 * ks + g) ^ lr) << 4;
                        const bf16x8 qf = *reinterpret_cast<const bf16x8*>(XN + row * 1024 + so);
#pragma unroll
                        for (int f = 0; f < 2; ++f)
                            sc[f] = MFMA16(*reinterpret_cast<const bf16x8*>(KL + (f * 16 + lr) * 1024 + so), qf, sc[f]);
                    }
                    const float scale = 0.08838834764831845f * 1.4426950408889634f;
                    float mx = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])),
                                     fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
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
                        const bf16x8 vf = *reinterpret_cast<const bf16x8*>(VL + (head * 128 + 16 * df + lr) * 64 + 16 * g);
                        const f32x4 o = MFMA16(vf, pf, (f32x4{0.f, 0.f, 0.f, 0.f}));
                        // o overwrites this wave's own q rows / columns (all its q reads are complete: they feed the MFMAs above)
                        *reinterpret_cast<bf16x4*>(XN + row * 1024 + (((head * 16 + 2 * df + (g >> 1)) ^ lr) << 4) + (g & 1) * 8) =
                            to_bf16x4(o * inv);
                    }
                }
            }
            if (l == 3) LSTAMP(32);
            __syncthreads();
            if (l == 3) LSTAMP(33);
            auto bsrc = [=](int tt) { return LdsTile{XN + (16 * tt + lr) * 1024, g, lr}; };
            float* const H = a.H;
            const float* const bp = L.b_proj;
            const Grp Gc = G;
            auto pre = [=](int, int tt) {
                const float* hp = H + ((size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr) * SYN_D + 16 * p + 4 * g;
                return ld_xcd(reinterpret_cast<const f32x4*>(hp)) + *reinterpret_cast<const f32x4*>(bp + 16 * p + 4 * g);
            };
            auto epi = [=](int, int tt, f32x4 acc, f32x4, f32x4 res) {
                float* hp = H + ((size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr) * SYN_D + 16 * p + 4 * g;
                *reinterpret_cast<f32x4*>(hp) = res + acc;
            };
            gemm_chunk<KS1, 8, 1, 1>(rp, 2 * nsq, bsrc, NoSwap{}, pre, epi, RED);
            if (s0 + 2 < G.ns) __syncthreads();
        }
        if (l == 3) LSTAMP(13);
        GROUP_BARRIER(1, ln_prefetch(lnp, L.ln2_g, L.ln2_b);
                      prefetch_w<KS1, 4, 2, 1>(r1, WTile{(const uint4*)L.w_fc1, p, 32, 0, KS1}););
        if (l == 3) LSTAMP(3);
        WRegs<KS2, 8, 1> r2;                                    // fc2: tile p; 8 K parts of 4 k-steps
        PF_EARLY(2, prefetch_w<KS2, 8, 1, 1>(r2, WTile{(const uint4*)L.w_fc2, p, 0, 0, KS2}););

        // ---- hid = gelu(LN2(h) . W1^T + b1): tiles p, p + 32 ----------------------------------------------
        for (int s0 = 0; s0 < G.ns; s0 += 2) {
            const int nsq = min(2, G.ns - s0);
            stage_ln(a.H, G, s0, nsq, lnp, XN);
            __syncthreads();
            auto bsrc = [=](int tt) { return LdsTile{XN + (16 * tt + lr) * 1024, g, lr}; };
            __bf16* const HID = a.HID;
            const float* const b1 = L.b_fc1;
            const Grp Gc = G;
            auto pre = [=](int ft, int) { return *reinterpret_cast<const f32x4*>(b1 + 16 * (p + 32 * ft) + 4 * g); };
            auto epi = [=](int ft, int tt, f32x4 acc, f32x4, f32x4 bias) {
                const int n = 16 * (p + 32 * ft) + 4 * g;
                f32x4 v = acc + bias;
                v[0] = gelu_erf(v[0]); v[1] = gelu_erf(v[1]); v[2] = gelu_erf(v[2]); v[3] = gelu_erf(v[3]);
                *reinterpret_cast<bf16x4*>(HID + ((size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr) * SYN_FF + n) = to_bf16x4(v);
            };
            gemm_chunk<KS1, 4, 2, 1>(r1, 2 * nsq, bsrc, NoSwap{}, pre, epi, RED);
            if (s0 + 2 < G.ns) __syncthreads();
        }
        if (l == 3) LSTAMP(14);
        GROUP_BARRIER(2, prefetch_w<KS2, 8, 1, 1>(r2, WTile{(const uint4*)L.w_fc2, p, 0, 0, KS2}););
        if (l == 3) LSTAMP(4);
        PF_EARLY(3, if (l + 1 < SYN_LAYERS) {
                     ln_prefetch(lnp, a.layer[l + 1].ln1_g, a.layer[l + 1].ln1_b);
                     prefetch_w<KS1, 2, 3, 1>(rq, WTile{(const uint4*)a.layer[l + 1].w_qkv, p, 32, 0, KS1});
                 });


        // ---- h += hid . W2^T + b2: tile p, K = 1024 straight from the L2-resident hidden tensor ------------
        for (int s0 = 0; s0 < G.ns; s0 += 2) {
            const int nsq = min(2, G.ns - s0);
            const __bf16* const HID = a.HID;
            const Grp Gc = G;
            auto bsrc = [=](int tt) {
                return XcdTile{HID + ((size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr) * SYN_FF + 8 * g};
            };
            float* const H = a.H;
            const float* const b2 = L.b_fc2;
            auto pre = [=](int, int tt) {
                const float* hp = H + ((size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr) * SYN_D + 16 * p + 4 * g;
                return ld_xcd(reinterpret_cast<const f32x4*>(hp)) + *reinterpret_cast<const f32x4*>(b2 + 16 * p + 4 * g);
            };
            auto epi = [=](int, int tt, f32x4 acc, f32x4, f32x4 res) {
                float* hp = H + ((size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr) * SYN_D + 16 * p + 4 * g;
                *reinterpret_cast<f32x4*>(hp) = res + acc;
            };
            gemm_chunk<KS2, 8, 1, 1>(r2, 2 * nsq, bsrc, NoSwap{}, pre, epi, RED);
            if (s0 + 2 < G.ns) __syncthreads();
        }
        if (l == 3) LSTAMP(15);
        GROUP_BARRIER(3, if (l + 1 < SYN_LAYERS) {
                          ln_prefetch(lnp, a.layer[l + 1].ln1_g, a.layer[l + 1].ln1_b);
                          prefetch_w<KS1, 2, 3, 1>(rq, WTile{(const uint4*)a.layer[l + 1].w_qkv, p, 32, 0, KS1});
                      });
        if (l == 3) LSTAMP(5);
    }

    LSTAMP(8);
    // ---- out: x0 = (sum_v w[blk][v] h_v) . Wout^T + b, x_next = c0 x0 + c1 x_t + sigma eps.  Tiles p + 32 blk,
    //      blk = 512-channel block (body part) of the guidance weights (there is no final LayerNorm) --------
    if (G.n0 >= 0) {
        // guided small batch: x0_hat of every sequence (variant) on its own XCD; k_guided_update forms
        // sum_v w[blk][v] x0_v (the guidance weights sum to 1 per block, so the bias is counted once) and the step
        WRegs<KS1, 2, 1> ro;
        prefetch_w<KS1, 2, 3, 1>(ro, WTile{a.w_out, p, 32, 0, KS1});
        const float* const b_out = a.b_out;
        float* const X0v = a.X0v;
        const Grp Gc = G;
        for (int s0 = 0; s0 < G.ns; s0 += 2) {
            const int nsq = min(2, G.ns - s0);
            if (s0 > 0) __syncthreads();
            for (int r = wave; r < nsq * 32; r += 8) {            // bf16(h) rows of the chunk -> LDS
                const float* hp = a.H + ((size_t)G.seq(s0 + (r >> 5)) * 32 + (r & 31)) * SYN_D + lane * 8;
                const f32x4 a0 = ld_xcd(reinterpret_cast<const f32x4*>(hp)), a1 = ld_xcd(reinterpret_cast<const f32x4*>(hp + 4));
                bf16x8 o8;
                o8[0] = (__bf16)a0[0]; o8[1] = (__bf16)a0[1]; o8[2] = (__bf16)a0[2]; o8[3] = (__bf16)a0[3];
                o8[4] = (__bf16)a1[0]; o8[5] = (__bf16)a1[1]; o8[6] = (__bf16)a1[2]; o8[7] = (__bf16)a1[3];
                *reinterpret_cast<bf16x8*>(XN + r * 1024 + ((lane ^ (r & 15)) << 4)) = o8;
            }
            __syncthreads();
            auto bsrc = [=](int tt) { return LdsTile{XN + (16 * tt + lr) * 1024, g, lr}; };
            auto pre = [=](int ft, int) { return *reinterpret_cast<const f32x4*>(b_out + 16 * (p + 32 * ft) + 4 * g); };
            auto epi = [=](int ft, int tt, f32x4 acc, f32x4, f32x4 bias) {
                const size_t row = (size_t)Gc.seq(s0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr;
                *reinterpret_cast<f32x4*>(X0v + row * SYN_C + 16 * (p + 32 * ft) + 4 * g) = acc + bias;
            };
            gemm_chunk<KS1, 2, 3, 1>(ro, 2 * nsq, bsrc, NoSwap{}, pre, epi, RED);
        }
    } else {
        WRegs<KS1, 2, 1> ro;                                    // single variant: the three blocks in one pass
        if (a.V == 1) prefetch_w<KS1, 2, 3, 1>(ro, WTile{a.w_out, p, 32, 0, KS1});
        const int c0 = G.c0;
        const int* const t_coef = a.t_coef; const float* const coef = a.coef; const float* const b_out = a.b_out;
        const float* const xt_p = a.xt; const float* const noise = a.noise; const unsigned long long* const rng = a.rng;
        float* const xn_p = a.xn; __bf16* const xnb = a.xnb; float* const x0_p = a.x0;
        const unsigned char* const keep = a.keep; const float* const known = a.known;
        for (int cl0 = 0; cl0 < G.nc; cl0 += 2) {
            const int ncl = min(2, G.nc - cl0);
            for (int blk = 0; blk < (a.V > 1 ? 3 : 1); ++blk) {
                if (cl0 > 0 || blk > 0) __syncthreads();
                stage_combine(a.H, G, a.V, cl0, ncl, a.V > 1 ? a.cfg_w + blk * a.V : nullptr, a.cfg_stride, XN);
                __syncthreads();
                auto bsrc = [=](int tt) { return LdsTile{XN + (16 * tt + lr) * 1024, g, lr}; };
                auto pre = [=](int ft, int tt) {
                    const int m = (c0 + cl0 + (tt >> 1)) * 32 + (tt & 1) * 16 + lr, n = 16 * (p + 32 * (blk + ft)) + 4 * g;
                    return Pre2{*reinterpret_cast<const f32x4*>(b_out + n), *reinterpret_cast<const f32x4*>(xt_p + (size_t)m * SYN_C + n)};
                };
                auto epi = [=](int ft, int tt, f32x4 acc, f32x4, Pre2 pv) {
                    const int clip = c0 + cl0 + (tt >> 1);
                    const int m = clip * 32 + (tt & 1) * 16 + lr, n = 16 * (p + 32 * (blk + ft)) + 4 * g;
                    const int tc = t_coef[clip];
                    const f32x4 cf = *reinterpret_cast<const f32x4*>(coef + (size_t)tc * 4);
                    const size_t off = (size_t)m * SYN_C + n;
                    f32x4 x0 = acc + pv.a;
                    if (keep) x0 = edit_x0(keep, known, off, x0);
                    f32x4 xn = x0 * cf[0] + pv.b * cf[1];
                    if (noise) xn = xn + *reinterpret_cast<const f32x4*>(noise + off) * cf[2];
                    else if (rng) xn = xn + randn4(rng[0], (uint64_t)tc, (rng[1] * (uint64_t)(SYN_T * SYN_C) + off) >> 2) * cf[2];
                    *reinterpret_cast<f32x4*>(xn_p + off) = xn;
                    *reinterpret_cast<bf16x4*>(xnb + off) = to_bf16x4(xn);
                    if (x0_p) *reinterpret_cast<f32x4*>(x0_p + off) = x0;
                };
                if (a.V == 1) {
                    gemm_chunk<KS1, 2, 3, 1>(ro, 2 * ncl, bsrc, NoSwap{}, pre, epi, RED);
                } else {                                          // guidance: one block (its own combination) at a time
                    WRegs<KS1, 8, 1> rb;
                    prefetch_w<KS1, 8, 1, 1>(rb, WTile{a.w_out, p + 32 * blk, 0, 0, KS1});
                    gemm_chunk<KS1, 8, 1, 1>(rb, 2 * ncl, bsrc, NoSwap{}, pre, epi, RED);
                }
            }
        }
    }
    LSTAMP(6);

    // ---- leave the counters zeroed for the next launch: the last workgroup of the group to finish resets them
    if (tid == 0) {
        const unsigned done = __hip_atomic_fetch_add(ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done == kP - 1) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace lat
