// syn_seq.inc — k_seq: the whole denoising step, one WAVE per sequence, four sequences per workgroup (large batches).
// (Included by syn_kernels.hip; its entry points - the step and the fragment-order converters - are there.)
//
// Why a second whole-step kernel.  k_stack keeps 64 rows (2 sequences) per CU: its LayerNorm output (64 KB) and the
// q/k/v / hidden staging (64 KB) fill the LDS, and every workgroup pulls the 38 MB weight set through its CU's 64 B/clk
// L2 port once per 64 rows - at MFMA speed a 64-row tile needs all of that bandwidth, so the step is weight-stream-bound
// (measured 40-55 B/clk per CU, 0.37 of the bf16 MFMA peak, DESIGN.md 4.1).  Rows per CU per weight byte is the only lever,
// and 128 rows of bf16 activations do not fit the LDS.  k_seq turns the decomposition around:
//   * a workgroup is 4 waves (one per SIMD, 512 registers each); a wave owns ONE sequence: 32 tokens x 512 features.
//     Its fp32 residual stream (256 registers), the LayerNorm output as bf16 MFMA operands (128 registers) and every
//     attention / MLP intermediate live in that wave's registers.  Activations never touch the LDS, rows of different
//     waves never meet, and there is no activation barrier anywhere in the step.
//   * the LDS (160 KB) holds nothing but WEIGHTS: the step's weights are pre-packed into one contiguous "tape" of 1 KB
//     MFMA fragments in consumption order (syntalker_amd/tape.py); the four waves DMA it into a 5 x 16 KB ring
//     (global_load_lds, 4 chunks = ~2 k cycles ahead of use; kSlots / kLook below) and every wave reads every fragment with one
//     ds_read_b128: 128 rows share each weight byte, the L2 port sees half the bytes per row that k_stack needs.
//   * v_mfma_f32_32x32x16_bf16, weights as the A operand: D[feature][token].  A lane ends up with features
//     {8q + 4hi + r} of token lane&31 - and that register image is, as it stands, the B operand of the next MFMA for
//     the K chunk 16c..16c+15 (registers of quads 2c, 2c+1) once the weights' K index is permuted the same way (done in
//     the tape).  q.k^T, softmax, P.V therefore run on accumulator registers exactly like the GEMMs: S^T = K.Q^T (k tile
//     as A, q tile as B), P^T is S^T's register image, V is produced in the swapped orientation so that it is the A
//     operand of O^T = V^T.P^T.  LayerNorm and softmax reduce over a lane's registers + ONE lane^32 exchange.
//   * LayerNorm gain / shift are folded into the qkv / fc1 weights and biases on the host, the k bias cancels in the
//     softmax, the v bias moves into the proj bias: inside the step biases are only accumulator initial values, read
//     from a 16 KB per-block set that rides along in the LDS.
//   * the latent lives in HBM in "fragment order" (what a lane holds): every global access of the step is a fully
//     coalesced 1 KB wave access; the reference layout exists only at loop entry / exit (syn_x_to_fragment / _from_).
// Every layout decision here is executed lane by lane by tests/kseq_model.py against the oracle on the CPU.
//
// Reference semantics: models/denoiser.py:132-196 (hoisted + folded, SURVEY 8 a17-a20), timm_transformer/transformer.py:
// 83-104,145-151,195-198, gaussian_diffusion.py:505-557 / :741-791 for the update.
namespace {
namespace seq {

typedef __attribute__((ext_vector_type(16))) float f32x16;
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

#ifndef SEQ_ABL      /* diagnostic builds only (timing ablations, results are garbage): 1 no DMA in the steady state,
                        2 no chunk barrier / wait, 4 no LDS fragment reads, 8 no MFMAs in the pieces */
#define SEQ_ABL 0
#endif
#ifndef SEQ_ABL2     /* more timing ablations (garbage results): 1 GELU = identity, 2 LayerNorm without statistics, 16 no LayerNorm at all (constant operands) */
#define SEQ_ABL2 0
#endif
constexpr int kThreads = 256;
constexpr int kFragBytes = 1024;
#ifndef SEQ_CHUNK
#define SEQ_CHUNK 16
#endif
#ifndef SEQ_WIN      /* LDS fragment reads in flight ahead of their MFMA (power of two, <= chunk size) */
#define SEQ_WIN 4
#endif
#ifndef SEQ_SPREAD   /* 1: a chunk's DMAs are issued one by one between MFMAs instead of together at the chunk boundary */
#define SEQ_SPREAD 1
#endif
#ifndef SEQ_SCHED    /* 0: fence after every fragment (nothing moves across an MFMA); n: up to n vector instructions per MFMA */
#define SEQ_SCHED 0
#endif
constexpr int kChunkFrags = SEQ_CHUNK, kChunkBytes = kChunkFrags * kFragBytes;     // ring granule: 16 (8) fragments, 4 (2) per wave
constexpr int kPerWave = kChunkFrags / 4;
constexpr int kSlots = 80 / kChunkFrags, kLook = kSlots - 1;   // ring slots; chunks issued ahead of the one being consumed
constexpr int kRingBytes = kSlots * kChunkBytes;            // 80 KB
constexpr int kBiasSet = 2048;                              // floats per bias set (8 KB, DMA'd like a chunk)
// (Biases and slabs BELOW the ring, where ds_read reaches them with a 16-bit immediate instead of a vector add per access - 700
// per block - was measured slower: 243 k cycles per block against 234 k, the register allocation moved again.)
constexpr int kRingBase = 0;
constexpr int kBiasBase = kRingBytes;                       // two sets
constexpr int kSlabBase = kBiasBase + 2 * kBiasSet * 4;     // per wave: residual tiles 12..15, fp32, 16 KB
constexpr int kSlabBytes = 4 * 4096;
constexpr int kLds = kSlabBase + 4 * kSlabBytes;            // 160 KB
// s_waitcnt vmcnt(N) of the ring: DMAs of this wave that are younger than the chunk waited for (2 per chunk)
#if SEQ_CHUNK == 16
#define SEQ_WAIT_STEADY "s_waitcnt vmcnt(8)"                /* chunks k+2, k+3 (4 DMAs each) */
#define SEQ_WAIT_FIRST "s_waitcnt vmcnt(12)"                /* chunks 1 .. 3 */
#else
#define SEQ_WAIT_STEADY "s_waitcnt vmcnt(14)"               /* chunks k+2 .. k+8 */
#define SEQ_WAIT_FIRST "s_waitcnt vmcnt(16)"                /* chunks 1 .. 8 */
#endif

struct QArgs {
    const char* tape; unsigned tape_chunks;                 // 2256 chunks of kChunkFrags = 16 fragments, followed by the first kLook chunks once more
    const float* bias;                                      // [9][2048]
    const float* te; const float* rcos; const float* rsin;
    const float* cond; const int* t_model;
    const float* xt;            // fragment order fp32 [R][48][4][64][4]
    const uint4* xb;            // fragment order bf16 [R][48][2][64] x 16 B
    const float* noise;         // fragment order, or null
    const unsigned long long* rng; const float* coef; const int* t_coef;
    float* xn; uint4* xnb; float* x0;
    int R;                      // clips (= sequences when V == 1)
    int V;                      // variants per clip (classifier-free guidance as one fused batch); k_seq<true> when > 1
    const float* cfg_w;         // [3][V] weights of the variants for output channels 0:512, 512:1024, 1024:1536 ...
    int cfg_stride;             // ... of clip 0; clip c's table starts cfg_stride floats x c further (0: one table for all clips, 3 V: per-clip scales)
    int n_steps;                // consecutive steps in this launch (>= 1); step j reads t_model + j tm_stride, t_coef + j tc_stride
    int tm_stride, tc_stride;
    int wg0, n_wg;              // this launch covers workgroups wg0 .. wg0 + n_wg - 1 of the batch (multi-step launches of batches
                                // with more workgroups than CUs go out one CU-filling slice after the other)
    int dbg_step;               // which step of the launch the per-stage cycle stamps describe
    unsigned skew;              // start delay of the last workgroup, in units of 64 cycles (spread linearly over the grid)
    long long* dbg;
};

// One LDS-DMA of 1 KB: lane l copies 16 B from src + 16 l to LDS byte address lds_dst + 16 l.  hipcc neither counts this
// load (the ring's own s_waitcnt does) nor preserves M0 around it (cdna_hip_programming.md 5.7).
__device__ __forceinline__ void dma_frag(const char* src, unsigned lds_dst, unsigned lane16) {
    // "s" operands must be wave-uniform for the compiler (kernel arguments, the wave index and chunk counters that are kept
    // in SGPRs by the readfirstlanes at their updates).
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %3\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane16), "s"(lds_dst), "s"(src) : "memory");
}

// The steady-state form: M0 is left pointing at the destination (nothing hipcc emits in this kernel reads M0 - checked in
// the -S output), and OFF is added to BOTH addresses, so the four fragments a wave copies per chunk share one source and
// one destination base: -9 % cycles per block against per-fragment address arithmetic with M0 saved and restored.
template <int OFF>
__device__ __forceinline__ void dma_frag_at(const char* src, unsigned lds_dst, unsigned lane16) {
    asm volatile("s_mov_b32 m0, %1\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %2 offset:%c3"
                 :: "v"(lane16), "s"(lds_dst), "s"(src), "i"(OFF) : "memory");
}

// The ring's bookkeeping.  Everything a chunk period needs is kept incrementally and every update is ONE pinned instruction
// group placed in an MFMA gap of take() (asm volatile: hipcc otherwise gathers the scalar arithmetic into a clump of ~17
// instructions in front of the chunk barrier, and with one wave per SIMD every scalar instruction that does not sit in an
// MFMA's shadow is matrix-pipe idle time - scripts/ubench/seq_issue.hip: 40.3 cycles per MFMA with the clump, 35.4 without):
//   * source: a constant scalar base (the tape) + a 32-bit vector offset that grows by one chunk per period (one v_add); the
//     tape carries its first kLook chunks again at its end, so the look-ahead across a step boundary needs no wrap test - the
//     offset is simply reset when a step begins;
//   * destination: slot base in a scalar register, wrapped by add / compare / conditional move (3 scalar instructions),
//     M0 = slot base + this wave's quarter is formed by the s_add that writes M0;
//   * LDS read bases of the current / next chunk in two vector registers.
#ifndef SEQ_DMA_POL      /* cache policy of the tape DMA (A/B): 0 default, 1 nt, 2 sc1, 3 sc0 */
#define SEQ_DMA_POL 0
#endif
#if SEQ_DMA_POL == 1
#define SEQ_DMA_POLICY " nt"
#elif SEQ_DMA_POL == 2
#define SEQ_DMA_POLICY " sc1"
#elif SEQ_DMA_POL == 3
#define SEQ_DMA_POLICY " sc0"
#else
#define SEQ_DMA_POLICY ""
#endif
struct Ring {
    const char* tape;      // scalar, constant
    unsigned voff;         // vector: 16 lane + 4 KB wave + 16 KB x (chunk this wave issues next)
    unsigned dst;          // scalar: LDS base of the slot the DMAs of this chunk period fill (the one chunk k-1 left)
    unsigned wq;           // scalar: this wave's quarter of a chunk, 4 KB wave
    unsigned voff0;        // vector: 16 lane + 4 KB wave (step boundary: voff = voff0 + kLook chunks)
    unsigned lane16;
    unsigned cur, nxt;     // this lane's LDS byte address inside the current / next chunk
    bf16x8 win[SEQ_WIN];   // the next fragments of the tape (they may belong to the next chunk)
};
static_assert(SEQ_CHUNK == 16 && kPerWave == 4, "the pinned ring arithmetic below is written for 16-fragment chunks");

// One of this wave's four DMAs of the chunk period: 1 KB from tape + voff + OFF to LDS dst + wq + OFF (+ 16 lane).  M0 is left
// pointing at the destination (nothing hipcc emits in this kernel reads M0 - checked in the -S output).
template <int OFF>
__device__ __forceinline__ void ring_dma(const Ring& r) {
    asm volatile("s_add_u32 m0, %1, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %3 offset:%c4" SEQ_DMA_POLICY
                 :: "v"(r.voff), "s"(r.dst), "s"(r.wq), "s"(r.tape), "i"(OFF) : "memory", "scc");
}
__device__ __forceinline__ void ring_dma_i(const Ring& r, int i) {
    switch (i) {
        case 0: ring_dma<0>(r); break;
        case 1: ring_dma<1024>(r); break;
        case 2: ring_dma<2048>(r); break;
        default: ring_dma<3072>(r); break;
    }
}
// next chunk period: the slot after this one, the tape one chunk on
__device__ __forceinline__ void ring_advance_dma(Ring& r) {
    // (plain expressions: the scheduling fences of take() keep them in the gap they are written in; as inline asm with an SGPR
    // in/out operand the same three instructions made hipcc lose the value's uniformity in some builds - "illegal VGPR to SGPR copy")
    const unsigned d = r.dst + kChunkBytes;
    r.dst = d == (unsigned)kRingBytes ? 0u : d;
    r.voff += kChunkBytes;
}
// read base of chunk k+1, the "next" chunk of period k (first used by the look-ahead at fragment 12): two slots on from the one this
// period's DMAs fill (the slot of chunk k-1)
__device__ __forceinline__ void ring_next_base(Ring& r) {
    static_assert(kSlots == 5 && kRingBase == 0, "slot arithmetic");
    // (plain expressions: the scheduling fences of take() keep them in the gap they are written in)
    unsigned t = r.dst + 2 * kChunkBytes;
    t = t >= (unsigned)kRingBytes ? t - kRingBytes : t;
    r.nxt = r.lane16 + t;
}

__device__ __forceinline__ void bias_issue(const float* bias, const Ring& r, int set) {
    const char* src = reinterpret_cast<const char*>(bias + (size_t)set * kBiasSet) + r.wq / 2;
    const unsigned dst = kBiasBase + (set & 1) * (kBiasSet * 4) + r.wq / 2;
    dma_frag(src, dst, r.lane16);
    dma_frag(src + kFragBytes, dst + kFragBytes, r.lane16);
}

// Start of chunk k: chunk k+1 must have landed before anybody reads ahead into it (every wave waits for ITS quarter, the
// barrier makes it everybody's); after the barrier all waves are done with chunk k-1, whose slot takes chunk k+4.
// The DMAs of chunks k+2, k+3 are younger than the ones waited for; any other vector memory operation in flight only
// makes the wait longer, never shorter (the counter retires in order).
__device__ __forceinline__ void ring_boundary(Ring& r) {
    if (!(SEQ_ABL & 2)) {
        if (!(SEQ_ABL & 64)) asm volatile(SEQ_WAIT_STEADY ::: "memory");
        if (!(SEQ_ABL & 128)) __builtin_amdgcn_s_barrier();
    }
    r.cur = r.nxt;                     // (the chunk that was "next" is the current one now)
}

// Next fragment of the tape.  f = position inside the chunk: a compile-time constant at every call site (pieces
// are multiples of 16 fragments and fully unrolled), so the branches fold.  The window keeps the LDS reads four fragments
// (= 128 cycles of MFMA issue) ahead of their use; hipcc would otherwise sink every read down to its consumer.
__device__ __forceinline__ bf16x8 take(Ring& r, const char* lds, int& f) {
    if (f == 0) {
        // The read this call owes the window - fragment SEQ_WIN of the chunk that starts here - goes out BEFORE the barrier:
        // that chunk has been everybody's since the previous barrier, and its address is the old "next" one.  What follows
        // the barrier release is then the MFMA itself.
        const bf16x8 a = r.win[0];
        if (!(SEQ_ABL & 4)) r.win[0] = *reinterpret_cast<const bf16x8*>(lds + r.nxt + SEQ_WIN * kFragBytes);
        ring_boundary(r);
        __builtin_amdgcn_sched_barrier(0);
        f = 1;
        return a;
    }
    // the DMAs of chunk k+4 (into the slot chunk k-1 just left), one at a time behind MFMAs 2, 6, 10, 14 of this chunk (not 1: the
    // instructions that follow a barrier release closely cost more - 215.4 k -> 212.4 k cycles per block): a DMA
    // instruction occupies the wave for ~46 cycles; issued back to back after the barrier all of that is matrix-pipe idle time,
    // issued right behind an MFMA 32 of the 46 cycles are the MFMA's own
    if (!(SEQ_ABL & 1) && (f & 3) == 2) ring_dma_i(r, f >> 2);
    // the bookkeeping, one group per gap: the read base of chunk k+2 (first used by the look-ahead at fragment 12) ...
    if (f == 6) ring_next_base(r);
    // ... and, behind the period's last DMA, the next period's slot and tape position
    if (f == 15) ring_advance_dma(r);
    const bf16x8 a = r.win[f & (SEQ_WIN - 1)];
    const int g = f + SEQ_WIN;
    if (!(SEQ_ABL & 4))
        r.win[f & (SEQ_WIN - 1)] = *reinterpret_cast<const bf16x8*>(lds + (g < kChunkFrags ? r.cur + g * kFragBytes : r.nxt + (g - kChunkFrags) * kFragBytes));
#if SEQ_SCHED == 0
    __builtin_amdgcn_sched_barrier(0);
#else
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, SEQ_SCHED, 0);
#endif
    f = (f + 1) & (kChunkFrags - 1);
    return a;
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& t, int c) {      // registers of quads 2c, 2c+1 -> bf16 operand
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)t[8 * c + e];
    return o;
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int v = 0; v < 16; ++v) z[v] = 0.f;
    return z;
}

// accumulator initial value of a (non-swapped) 32-feature tile: bias[32 tile + 8q + 4hi + r], from the LDS-resident set
__device__ __forceinline__ f32x16 bias_tile(const char* lds, int set, int off, int tile, int hi) {
    // the bias sets sit above 64 KB, beyond a ds_read's 16-bit immediate: left to itself hipcc adds the constant to a register
    // once per read (700 vector adds per block); with the sum hidden behind an empty asm it is made once per tile
    unsigned at = (unsigned)(kBiasBase + (set & 1) * (kBiasSet * 4) + (off + 32 * tile + 4 * hi) * 4);
    asm volatile("" : "+v"(at));
    const float* b = reinterpret_cast<const float*>(lds + at);
    f32x16 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(b + 8 * q);
        o[4 * q] = v[0]; o[4 * q + 1] = v[1]; o[4 * q + 2] = v[2]; o[4 * q + 3] = v[3];
    }
    return o;
}

// residual tiles 12..15 of this wave: private LDS slab, [tile][quad][lane] x 16 B
__device__ __forceinline__ f32x16 slab_load(const char* slab, int t) {
    f32x16 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(slab + (t * 4 + q) * 1024);
        o[4 * q] = v[0]; o[4 * q + 1] = v[1]; o[4 * q + 2] = v[2]; o[4 * q + 3] = v[3];
    }
    return o;
}
__device__ __forceinline__ void slab_store(char* slab, int t, const f32x16& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(slab + (t * 4 + q) * 1024) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
}

__device__ __forceinline__ float xor32(float v) { return __shfl_xor(v, 32); }

// nn.GELU() = x Phi(x).  Phi(x) = sigmoid(x (c0 + c1 x^2 + c2 x^4)) with minimax-fitted coefficients: |error| <= 2.6e-5
// (the plain tanh form: 4.7e-4), i.e. 80 x below the bf16 rounding of the value it feeds; 10 vector operations (2 transcendental)
// against 15 for the erf series of gelu_erf.  The fit holds on |x| <= 10.5 only: the quartic turns over at x^2 = 123.7 (at 11.2 it
// returns 1.27, at -12 it returns -12), so x^2 is clamped at 64 - beyond |x| = 8 the exponent is -4.98 x, monotone, and the sigmoid
// saturates to 1 / 0 on both sides like Phi (there Phi is within 1e-15 of them); a NaN still comes out as a NaN, through x.
// This kernel has one wave per SIMD: every vector instruction that does not fit an MFMA's shadow is wall time.
__device__ __forceinline__ float gelu_fast(float x) {
    if (SEQ_ABL2 & 1) return x;
    const float x2 = fminf(x * x, 64.0f);
    float t = fmaf(1.0142633e-3f, x2, -1.0677573e-1f);        // -log2(e) * (c2 x^2 + c1)
    t = fmaf(t, x2, -2.3011213f);                              // -log2(e) * c0
    const float e = __builtin_amdgcn_exp2f(x * t);             // exp(-u)
    return nopk(x * __builtin_amdgcn_rcpf(1.0f + e));
}

// "wide" piece: residual += W(:, kc) . B[kc] over all 16 tiles of the residual stream
struct NoFill { __device__ __forceinline__ void operator()(int) const {} };

// The slab tiles (residual tiles 12..15, LDS-resident between the pieces) make ONE round trip per wide piece, overlapped with
// its MFMAs: all four are loaded into accumulator registers in the gaps of eight early MFMAs (the q / k / v / fc1 accumulators
// are dead inside a wide piece, which is exactly the room four tiles need - the accumulator file holds 256 registers, 192 of them
// the register tiles), take part in the piece like the other twelve, and in the last k chunk they come FIRST, so that their
// sixteen stores ride in the gaps of the twelve MFMAs that follow.  (Round 2 loaded, accumulated and stored them two at a time
// AFTER the twelve register tiles: two load - MFMA - store phases per piece with nothing to hide the LDS latency behind, 700
// cycles each, 20 k of a block's 203 k cycles - measured by running the same MFMAs on register copies.)
// Fragment order of a piece (tape.py `wide`):  [kc < SPLIT][tile 0..11], [kc < SPLIT][tile 12..15], then for kc >= SPLIT
// [tile 0..15], the last k chunk as [tile 12..15][tile 0..11] (KC > 1).  SPLIT > 0 defers the slab tiles of the first k chunks: the
// MLP's fc2 piece starts while the second fc1 tile pair is still being put through GELU in accumulator registers (until MFMA 35; the slab
// tiles arrive in gaps 36..43).
// fill(i), i = 0 .. 16 KC - 1: vector work the caller wants issued in the shadow of the i-th MFMA (the fences in take() keep it there).
__device__ __forceinline__ void slab_load_half(const char* slab, int t, int half, f32x16& o) {
#pragma unroll
    for (int q = 2 * half; q < 2 * half + 2; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(slab + (t * 4 + q) * 1024);
        o[4 * q] = v[0]; o[4 * q + 1] = v[1]; o[4 * q + 2] = v[2]; o[4 * q + 3] = v[3];
    }
}
__device__ __forceinline__ void slab_store_quad(char* slab, int t, int q, const f32x16& v) {
    *reinterpret_cast<f32x4*>(slab + (t * 4 + q) * 1024) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
}

template <int KC, int SPLIT = 0, typename Opnd, typename Fill = NoFill>
__device__ __forceinline__ void wide_of(Ring& r, const char* lds, f32x16 (&h)[12], char* slab, Opnd opnd, Fill fill = Fill()) {
    static_assert(SPLIT >= 0 && SPLIT < KC && (SPLIT == 0 || 12 * SPLIT >= 20), "slab loads must fit in front of their first use");
    constexpr int kLoad0 = SPLIT ? 12 * SPLIT - 12 : 0;              // the eight MFMAs whose gaps carry the sixteen slab reads
    constexpr int kStore0 = KC > 1 ? 16 * (KC - 1) + 4 : 16 * KC;    // first MFMA whose gap carries slab stores (none if KC == 1)
    f32x16 s[4];
    int f = 0, n = 0;
    auto mm = [&](f32x16& acc, int kc) {
        acc = MFMA32(take(r, lds, f), opnd(kc), acc);
        if (n >= kLoad0 && n < kLoad0 + 8) slab_load_half(slab, (n - kLoad0) >> 1, (n - kLoad0) & 1, s[(n - kLoad0) >> 1]);
        if (n >= kStore0 && n < kStore0 + 12) {                       // 16 stores over 12 gaps: two in each of the first four
            const int j = n - kStore0, first = j < 4 ? 2 * j : 4 + j, cnt = j < 4 ? 2 : 1;
#pragma unroll
            for (int w = first; w < first + cnt; ++w) slab_store_quad(slab, w >> 2, w & 3, s[w >> 2]);
        }
        fill(n);
        ++n;
    };
    if constexpr (SPLIT > 0) {
#pragma unroll
        for (int kc = 0; kc < SPLIT; ++kc)
#pragma unroll
            for (int t = 0; t < 12; ++t) mm(h[t], kc);
#pragma unroll
        for (int kc = 0; kc < SPLIT; ++kc)
#pragma unroll
            for (int t = 0; t < 4; ++t) mm(s[t], kc);
    }
#pragma unroll
    for (int kc = SPLIT; kc < KC; ++kc) {
        if (KC > 1 && kc == KC - 1) {
#pragma unroll
            for (int t = 0; t < 4; ++t) mm(s[t], kc);
#pragma unroll
            for (int t = 0; t < 12; ++t) mm(h[t], kc);
        } else {
#pragma unroll
            for (int t = 0; t < 12; ++t) mm(h[t], kc);
#pragma unroll
            for (int t = 0; t < 4; ++t) mm(s[t], kc);
        }
    }
    if constexpr (KC == 1) {                                          // (the rank-1 bias pieces: nothing left to hide the stores behind)
#pragma unroll
        for (int t = 0; t < 4; ++t) slab_store(slab, t, s[t]);
    }
}

template <int KC, typename Fill = NoFill>
__device__ __forceinline__ void wide(Ring& r, const char* lds, f32x16 (&h)[12], char* slab, bf16x8 (&B)[KC], Fill fill = Fill()) {
    wide_of<KC, 0>(r, lds, h, slab, [&](int kc) { return B[kc]; }, fill);
}

// "pair" piece over K = 512: two tiles in flight, fragments [kc][u]; SWAP: the activation is the A operand
template <bool SWAP, typename Fill = NoFill>
__device__ __forceinline__ void pair512(Ring& r, const char* lds, const bf16x8 (&B)[32], f32x16& a0, f32x16& a1, Fill fill = Fill()) {
    int f = 0;
#pragma unroll
    for (int kc = 0; kc < 32; ++kc) {
        const bf16x8 w0 = take(r, lds, f);
        a0 = SWAP ? MFMA32(B[kc], w0, a0) : MFMA32(w0, B[kc], a0);
        const bf16x8 w1 = take(r, lds, f);
        a1 = SWAP ? MFMA32(B[kc], w1, a1) : MFMA32(w1, B[kc], a1);
        fill(kc);                      // vector work issued in the shadow of these two MFMAs
    }
}

// mean / rstd of every token over its 512 features, then XN = (h - mean) * rstd as bf16 operands (gain / shift live in the tape)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) { return a + b; }                 // v_pk_add_f32 / v_pk_fma_f32: fine where no MFMA is in flight
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return a * b + c; }
// (nopk: syn_kernels.hip - work that rides in an MFMA's shadow is written element by element, packed fp32 operations stall there)

__device__ __forceinline__ void norm_to_operands(const f32x16 (&h)[12], const char* slab, bf16x8 (&xn)[32]) {
    if (SEQ_ABL2 & 16) {                                            // (timing: what the whole function costs)
#pragma unroll
        for (int i = 0; i < 32; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) xn[i][e] = (__bf16)0.01f;
        return;
    }
    // No MFMA is in flight here, so packed fp32 operations cost what a scalar one does (beside MFMAs they do not): sums and
    // normalisation two values per instruction - a third of this function's ~1460 vector instructions, two of them per block.
    f32x2 s2 = {0.f, 0.f}, q2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x16 v = t < 12 ? h[t] : slab_load(slab, t - 12);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x2 p = {v[2 * i], v[2 * i + 1]};
            s2 = pk_add(s2, p);
            q2 = pk_fma(p, p, q2);
        }
    }
    float s = s2[0] + s2[1], q = q2[0] + q2[1];
    if (SEQ_ABL2 & 2) { s = 1.f; q = 600.f; }
    s += xor32(s); q += xor32(q);
    const float mean = s * (1.0f / 512.0f);
    const float var = fmaxf(q * (1.0f / 512.0f) - mean * mean, 0.f);
    const float rstd = rsqrtf(var + 1e-5f);                          // nn.LayerNorm: biased variance, eps 1e-5
    const float nm = -mean * rstd;
    const f32x2 r2 = {rstd, rstd}, n2 = {nm, nm};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x16 v = t < 12 ? h[t] : slab_load(slab, t - 12);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x2 y = pk_fma(f32x2{v[8 * c + 2 * e], v[8 * c + 2 * e + 1]}, r2, n2);
                o[2 * e] = (__bf16)y[0]; o[2 * e + 1] = (__bf16)y[1];
            }
            xn[2 * t + c] = o;
        }
    }
}

// The arguments are read from the kernarg segment where they are needed, through a pointer hipcc cannot see through
// (KARGS): taken by value they are all live for the whole step loop - 34 scalar registers of pointers, the scalar file
// spills into vector lanes and the vector allocation, a few registers from 512 as it is, tips over (89 spilled registers
// against 16).
using KArgs = const __attribute__((address_space(4))) QArgs;
#define KARGS(name) KArgs* name = reinterpret_cast<KArgs*>(reinterpret_cast<unsigned long long>(__builtin_amdgcn_kernarg_segment_ptr())); asm volatile("" : "+s"(name))

// G (guided batches, cfg_sampler.py:10-167): the V <= 4 variants of a clip are the waves of ONE workgroup (two clips per
// workgroup at V = 2).  They share x_t, run the blocks independently under their own conditioning, and meet in the output
// stage: every wave projects its own stream (all of them consume the same weight fragments), publishes its x0 tiles in its
// LDS slab (dead by then), and the posterior update of a tile pair - x0 = sum_v w[c][v] x0_v - is dealt out to the V
// waves by quad pairs, so each wave draws 1 / V of the noise.
// NZ: the noise term of the update - 0 none (DDIM with eta = 0, a bare model evaluation), 1 read from QArgs::noise, 2 drawn here.
template <bool G, int NZ>
__global__ __launch_bounds__(kThreads) void k_seq(const QArgs) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    KARGS(a0);
    const int lane0 = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int seq, cseq, var = 0, group0 = 0;          // clip (latent, coefficients, noise), row of cond / t_model, variant, first wave of the clip
    bool live;
    if constexpr (!G) {
        seq = (a0->wg0 + (int)blockIdx.x) * 4 + wave;
        live = seq < a0->R;
        seq = live ? seq : a0->R - 1;                           // idle waves shadow the last sequence (stores masked)
        cseq = seq;
    } else {
        const int V = a0->V, cpw = 4 / V;                       // clips per workgroup: 2, 1, 1 at V = 2, 3, 4
        const int g = wave / V;
        seq = (a0->wg0 + (int)blockIdx.x) * cpw + g;
        live = g < cpw && seq < a0->R;
        var = live ? wave - g * V : -1;                         // (-1: takes no part in the posterior update)
        group0 = live ? g * V : 0;
        seq = live ? seq : a0->R - 1;
        cseq = (live ? var : 0) * a0->R + seq;
    }

    Ring r;
    r.tape = a0->tape; r.lane16 = (unsigned)lane0 * 16;
    r.wq = (unsigned)__builtin_amdgcn_readfirstlane(wave * (kPerWave * kFragBytes));
    r.voff0 = r.lane16 + r.wq;
    // prologue: bias set 0 first (older than every chunk: landed by the first wait), then chunks 0 .. kLook-1 into slots 0 .. kLook-1
    bias_issue(a0->bias, r, 0);
    r.voff = r.voff0; r.dst = kRingBase;
#pragma unroll 1
    for (int c = 0; c < kLook; ++c) {
#pragma unroll
        for (int i = 0; i < kPerWave; ++i) ring_dma_i(r, i);
        ring_advance_dma(r);
    }                                                                // (now: chunk kLook into slot kLook, the period-0 DMAs)
    asm volatile(SEQ_WAIT_FIRST ::: "memory");
    __builtin_amdgcn_s_barrier();
    r.cur = r.lane16 + kRingBase;                                    // slot 0
    r.nxt = r.cur;                                                   // (the first take() opens chunk 0: its look-ahead read and cur = nxt expect slot 0 here)
#pragma unroll
    for (int i = 0; i < SEQ_WIN; ++i) r.win[i] = *reinterpret_cast<const bf16x8*>(lds + kRingBase + r.lane16 + i * kFragBytes);
    // Several steps per launch: every workgroup keeps ITS four sequences for all of them (a sequence never leaves its wave:
    // the x_next this wave stores is the x_t it loads one step later), so there is no launch boundary, no refill of the ring
    // and no common finishing line between steps: -5 % per step at 10 steps per launch.  The workgroups start in lock-step and
    // drift apart by themselves (std of the phase: 13 k cycles in step 0, 336 k = 15 % of a step in step 9); an imposed start
    // delay (skew > 0, diagnostics) only adds its own length - the input / output stages are bound by instruction issue, not
    // by the HBM burst of 256 workgroups storing at once (measured with the stores and loads ablated, DESIGN.md 4.0).
    if (a0->skew) {
        const unsigned n = (unsigned)(((unsigned long long)a0->skew * blockIdx.x) / gridDim.x);
        for (unsigned i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_s_barrier();
    }
    if (a0->dbg && wave == 0 && lane0 == 0) a0->dbg[(size_t)blockIdx.x * 32 + 0] = (long long)__builtin_readcyclecounter();

#pragma unroll 1
  for (int step = 0; step < a0->n_steps; ++step) {
    KARGS(a);
    if (step) {
        // every wave is past the previous step's output stage (its biases sit in slot 0, where set 0 goes now)
        // (G: the x_next of this clip was stored by all waves of its group and every one of them loads all of it next)
        if constexpr (G) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        bias_issue(a->bias, r, 0);
        // the ring already holds the next step's first kLook chunks (the tape repeats them at its end): go on behind them
        r.voff = r.voff0 + kLook * kChunkBytes;
        asm volatile("" : "+v"(r.voff));
    }
    // everything a lane derives from its index is derived again in every step: hoisted out of the step loop, the addresses
    // of a dozen tensors would sit in registers this kernel does not have (167 spilled registers instead of 16)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int hi = lane >> 5, tok = lane & 31;
    char* const slab = lds + kSlabBase + wave * kSlabBytes + lane * 16;
    const bool stamp = a->dbg && wave == 0 && lane == 0 && step == a->dbg_step;
    f32x16 h[12];
    // ---- input stage: h = rotary(x_t . A^T + cond + te[t]); all 16 tiles in registers here ----------------------------
    {
        f32x16 g[16];
        const int ts = a->t_model[(size_t)step * a->tm_stride + cseq];
        const float* cp = a->cond + ((size_t)cseq * 32 + tok) * SYN_D + 4 * hi;
        const float* tp = a->te + (size_t)ts * SYN_D + 4 * hi;
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 c = *reinterpret_cast<const f32x4*>(cp + 32 * t + 8 * q);
                const f32x4 e = *reinterpret_cast<const f32x4*>(tp + 32 * t + 8 * q);
                g[t][4 * q] = c[0] + e[0]; g[t][4 * q + 1] = c[1] + e[1]; g[t][4 * q + 2] = c[2] + e[2]; g[t][4 * q + 3] = c[3] + e[3];
            }
        // x_t operands: one coalesced 1 KB load per k-chunk, 8 chunks ahead
        const uint4* xp = a->xb + (size_t)seq * (96 * 64) + lane;
        uint4 xq[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xq[u] = xp[u * 64];
#ifndef SEQ_IN_UNROLL
#define SEQ_IN_UNROLL 1
#endif
#pragma unroll SEQ_IN_UNROLL
        for (int j = 0; j < 12; ++j) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bf16x8 b = __builtin_bit_cast(bf16x8, xq[u]);
                // (unconditional: around a load that depends on a runtime condition hipcc branches and waits vmcnt(0), which
                // also drains the ring's DMAs - the tail re-reads the last chunk instead)
                const int kn = min(j * 8 + u + 8, 95);
                if (!(SEQ_ABL & 32)) xq[u] = xp[(size_t)kn * 64];
                int f = 0;
#pragma unroll
                for (int t = 0; t < 16; ++t) g[t] = MFMA32(take(r, lds, f), b, g[t]);
            }
        }
        // rotary on the (j, j + 32) pairs of every 64-wide group = tiles 2g, 2g + 1, same register (denoiser.py:178-186)
        f32x4 cs[4], sn[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cs[q] = *reinterpret_cast<const f32x4*>(a->rcos + tok * 32 + 8 * q + 4 * hi);
            sn[q] = *reinterpret_cast<const f32x4*>(a->rsin + tok * 32 + 8 * q + 4 * hi);
        }
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float u = g[2 * p][v], w = g[2 * p + 1][v], c = cs[v >> 2][v & 3], s = sn[v >> 2][v & 3];
                g[2 * p][v] = u * c - w * s;
                g[2 * p + 1][v] = w * c + u * s;
            }
#pragma unroll
        for (int t = 0; t < 12; ++t) h[t] = g[t];
#pragma unroll
        for (int t = 0; t < 4; ++t) slab_store(slab, t, g[12 + t]);
    }
    if (stamp) a->dbg[(size_t)blockIdx.x * 32 + 1] = (long long)__builtin_readcyclecounter();

    const float scale = 0.08838834764831845f * 1.4426950408889634f;   // 128^-0.5 * log2(e)
    // B operand of the rank-1 bias updates: 1.0 in the slots k = 0, 1.  Rebuilt at each use (two moves) instead of living in
    // four registers across the whole block loop: the allocator is within a few registers of the 512 it has.
    auto make_ones = [&](bf16x8 (&o)[1]) {
        int hz = hi;
        asm volatile("" : "+v"(hz));
#pragma unroll
        for (int e = 0; e < 8; ++e) o[0][e] = (__bf16)((hz == 0 && e < 2) ? 1.0f : 0.0f);
    };
#pragma unroll 1
    for (int l = 0; l < SYN_LAYERS; ++l) {
        bf16x8 xn[32];
        // ---- attention half ------------------------------------------------------------------------------------
        norm_to_operands(h, slab, xn);
        {
            bf16x8 ones[1];
            make_ones(ones);
            wide<1>(r, lds, h, slab, ones);                          // h += proj bias (+ folded v bias)
        }
#pragma unroll 1
        for (int head = 0; head < SYN_HEADS; ++head) {
            bf16x8 qb[4][2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                f32x16 a0 = bias_tile(lds, l, 128 * head, 2 * p, hi), a1 = bias_tile(lds, l, 128 * head, 2 * p + 1, hi);
                pair512<false>(r, lds, xn, a0, a1);
                qb[2 * p][0] = pack8(a0, 0); qb[2 * p][1] = pack8(a0, 1);
                qb[2 * p + 1][0] = pack8(a1, 0); qb[2 * p + 1][1] = pack8(a1, 1);
            }
            // S^T[key][query] = sum_d K[key][d] Q[query][d]: the k tile is the A operand, the q tile the B operand
            f32x16 s = zero16();
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                f32x16 a0 = zero16(), a1 = zero16();
                pair512<false>(r, lds, xn, a0, a1);
                s = MFMA32(pack8(a0, 0), qb[2 * p][0], s);
                s = MFMA32(pack8(a0, 1), qb[2 * p][1], s);
                s = MFMA32(pack8(a1, 0), qb[2 * p + 1][0], s);
                s = MFMA32(pack8(a1, 1), qb[2 * p + 1][1], s);
            }
            float mx = s[0];
#pragma unroll
            for (int v = 1; v < 16; ++v) mx = fmaxf(mx, s[v]);
            mx = fmaxf(mx, xor32(mx));
            bf16x8 pb[2];
            float sum = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const __bf16 pv = (__bf16)__builtin_amdgcn_exp2f((s[v] - mx) * scale);
                pb[v >> 3][v & 7] = pv;
                sum += (float)pv;
            }
            sum += xor32(sum);
            const float inv = 1.0f / sum;
            // O^T[d][query] = sum_key V^T[d][key] P^T[key][query]: v comes out [key][d] (swapped), i.e. as the A operand
            bf16x8 ob[8];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                f32x16 a0 = zero16(), a1 = zero16();
                pair512<true>(r, lds, xn, a0, a1);
                f32x16 o0 = MFMA32(pack8(a0, 0), pb[0], zero16());
                o0 = MFMA32(pack8(a0, 1), pb[1], o0);
                f32x16 o1 = MFMA32(pack8(a1, 0), pb[0], zero16());
                o1 = MFMA32(pack8(a1, 1), pb[1], o1);
                o0 = o0 * inv; o1 = o1 * inv;
                ob[4 * p] = pack8(o0, 0); ob[4 * p + 1] = pack8(o0, 1);
                ob[4 * p + 2] = pack8(o1, 0); ob[4 * p + 3] = pack8(o1, 1);
            }
            wide<8>(r, lds, h, slab, ob);                            // h += o_head . Wproj[:, 128 head ..]^T
        }
        // ---- MLP half ------------------------------------------------------------------------------------------
        bias_issue(a->bias, r, l + 1);       // next block's (or the output stage's) biases into the other slot: every wave is past
                                       // block l-1 (we all met at this block's chunk barriers)
        norm_to_operands(h, slab, xn);
        {
            bf16x8 ones[1];
            make_ones(ones);
            wide<1>(r, lds, h, slab, ones);                          // h += fc2 bias
        }
#pragma unroll 1
        for (int sl = 0; sl < SYN_FF / 128; ++sl) {
            // fc1 of the slice as two tile pairs; the GELU of pair 0 runs in the shadow of pair 1's MFMAs, the GELU of pair 1
            // in the shadow of the first fc2 MFMAs (k chunks 0..3 of fc2 read only pair 0's tiles)
            bf16x8 hb[8];
            f32x16 a0 = bias_tile(lds, l, 512 + 128 * sl, 0, hi), a1 = bias_tile(lds, l, 512 + 128 * sl, 1, hi);
            pair512<false>(r, lds, xn, a0, a1);
            f32x16 b0 = bias_tile(lds, l, 512 + 128 * sl, 2, hi), b1 = bias_tile(lds, l, 512 + 128 * sl, 3, hi);
            // one GELU per k chunk: 9 vector instructions behind 2 MFMAs
            pair512<false>(r, lds, xn, b0, b1, [&](int kc) {
                if (kc < 16) a0[kc] = gelu_fast(a0[kc]); else a1[kc - 16] = gelu_fast(a1[kc - 16]);
            });
            hb[0] = pack8(a0, 0); hb[1] = pack8(a0, 1); hb[2] = pack8(a1, 0); hb[3] = pack8(a1, 1);
            // fc2 k chunks 0..3 (MFMAs 0..47) read hb[0..3]; pair 1's GELU and conversion ride on MFMAs 0..35
            wide_of<8, 4>(r, lds, h, slab, [&](int kc) { return hb[kc]; }, [&](int i) {
                if (i < 16) b0[i] = gelu_fast(b0[i]);
                else if (i < 32) b1[i - 16] = gelu_fast(b1[i - 16]);
                else if (i == 32) hb[4] = pack8(b0, 0);
                else if (i == 33) hb[5] = pack8(b0, 1);
                else if (i == 34) hb[6] = pack8(b1, 0);
                else if (i == 35) hb[7] = pack8(b1, 1);
            });                                                      // h += gelu(slice) . W2[:, 128 sl ..]^T
        }
        if (stamp) a->dbg[(size_t)blockIdx.x * 32 + 2 + l] = (long long)__builtin_readcyclecounter();
    }

    // ---- output stage: x0 = h . Wout^T + b (no final LayerNorm, denoiser.py:188-195), x_next = c0 x0 + c1 x_t + sigma eps
    {
        KARGS(a);                                                    // (shadows the step's pointer: nothing of the input stage stays live)
        bf16x8 hb[32];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const f32x16 v = t < 12 ? h[t] : slab_load(slab, t - 12);
            hb[2 * t] = pack8(v, 0); hb[2 * t + 1] = pack8(v, 1);
        }
        const int tc = a->t_coef[(size_t)step * a->tc_stride + seq];
        const f32x4 cf = *reinterpret_cast<const f32x4*>(a->coef + (size_t)tc * 4);
        // This sequence's rows of every tensor: a scalar base each, and ONE 32-bit lane offset that moves on by a tile pair
        // (8 KB of fp32, 4 KB of bf16 operands) per iteration - all that the 16 loads / stores of a pair add is an immediate.
        const size_t seq_f32 = (size_t)seq * (SYN_T * SYN_C * 4), seq_b16 = (size_t)seq * (SYN_T * SYN_C * 2);
        const char* const xt_s = reinterpret_cast<const char*>(a->xt) + seq_f32;
        char* const xn_s = reinterpret_cast<char*>(a->xn) + seq_f32;
        char* const xnb_s = reinterpret_cast<char*>(a->xnb) + seq_b16;
        char* const x0_s = a->x0 ? reinterpret_cast<char*>(a->x0) + seq_f32 : nullptr;
        [[maybe_unused]] const char* const nz_s = NZ == 1 ? reinterpret_cast<const char*>(a->noise) + seq_f32 : nullptr;
        [[maybe_unused]] unsigned long long seed = 0ull;
        // counter of this lane's first Philox block: token-major element index / 4 - what keys the noise (same values as k_stack);
        // tile nf, quad q add 8 nf + 2 q
        [[maybe_unused]] unsigned long long idx4 = 0ull;
        if constexpr (NZ == 2) {
            seed = a->rng[0];
            idx4 = (a->rng[1] + (unsigned long long)seq) * (unsigned long long)(SYN_T * SYN_C / 4) + (unsigned long long)(tok * (SYN_C / 4) + hi);
        }
        int off_f = lane * 16, off_b = lane * 16;                    // byte offsets of the pair whose update is being issued (pr - 1)
        // Software pipeline over the 24 tile pairs: the posterior update of pair p-1 (Philox + Box-Muller + the fused multiply-
        // adds: ~110 vector instructions per 4 channels of 32 tokens) is issued one quad per 4 k-chunks in the shadow of pair p's
        // MFMAs, its x_t was requested one pair earlier, its stores go out as they are produced.
        // (defined before the pair loop: left undefined, hipcc carries their registers around the whole step loop - 40 spilled)
        // Two sets of accumulators and x_t registers, taken in turn: the update of pair p-1 reads the set that pair p does not
        // write, so nothing is copied between pairs (one set handed on to a "previous pair" copy cost 64 v_accvgpr_mov and 32 v_mov
        // per pair).  The odd pairs' set is carried around the loop (and read after it), so it is the one defined here.
        f32x16 acc_odd[2] = {zero16(), zero16()};
        f32x4 xt_odd[2][4], xo;
        // G: this wave's two 8 KB exchange buffers (its slab), and the slabs of its clip's variants
        [[maybe_unused]] const int nvar = G ? a->V : 1;
        [[maybe_unused]] unsigned gat = (unsigned)(kSlabBase + group0 * kSlabBytes + lane * 16);
        if constexpr (G) asm volatile("" : "+v"(gat));
        xo = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) xt_odd[u][q] = xo;
        auto fetch = [&](int off, f32x4 (&xt)[2][4]) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    xt[u][q] = (SEQ_ABL & 16) ? f32x4{1.f, 2.f, 3.f, 4.f} : *reinterpret_cast<const f32x4*>(xt_s + off + (u * 4 + q) * 1024);
        };
        // channels 32 nf + 8 q + 4 hi .. + 3 of the pair whose offsets are off_f / off_b; pr: that pair's index (G only);
        // pacc / pxt: that pair's accumulators and x_t
        auto quad = [&](int pr, int u, int q, const f32x16 (&pacc)[2], const f32x4 (&pxt)[2][4]) {
            const int at_f = off_f + (u * 4 + q) * 1024;
            f32x4 x0;
            if constexpr (!G) {
                x0 = f32x4{pacc[u][4 * q], pacc[u][4 * q + 1], pacc[u][4 * q + 2], pacc[u][4 * q + 3]};
            } else {
                // (every variant's tile started from the output bias: the weights of a guidance formula sum to 1)
                const float* wc = a->cfg_w + (size_t)seq * a->cfg_stride + ((2 * pr + u) >> 4) * nvar;
                const unsigned at = gat + (unsigned)((pr & 1) * 8192 + (u * 4 + q) * 1024);
                x0 = *reinterpret_cast<const f32x4*>(lds + at) * wc[0];
#pragma unroll
                for (int v = 1; v < 4; ++v)
                    if (v < nvar) x0 = x0 + *reinterpret_cast<const f32x4*>(lds + at + v * kSlabBytes) * wc[v];
            }
            f32x4 xv;
            [[maybe_unused]] f32x4 z;
            if constexpr (NZ == 1) z = *reinterpret_cast<const f32x4*>(nz_s + at_f);
            if constexpr (NZ == 2) z = randn4<!G>(seed, (uint64_t)tc, idx4 + (unsigned long long)(8 * u + 2 * q));
#pragma unroll
            for (int e = 0; e < 4; ++e) {                            // (element by element: see nopk)
                float v = fmaf(x0[e], cf[0], nopk(pxt[u][q][e] * cf[1]));
                if constexpr (NZ != 0) v = fmaf(z[e], cf[2], v);
                xv[e] = nopk(v);
            }
            if (live && (!(SEQ_ABL & 8) || a->R < 0)) {
                *reinterpret_cast<f32x4*>(xn_s + at_f) = xv;
                if (x0_s) *reinterpret_cast<f32x4*>(x0_s + at_f) = x0;
                if (q & 1) {                                         // quads 2c, 2c+1 -> one bf16 operand fragment of the next step
                    bf16x8 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { o[e] = (__bf16)xo[e]; o[4 + e] = (__bf16)xv[e]; }
                    *reinterpret_cast<uint4*>(xnb_s + off_b + (u * 2 + (q >> 1)) * 1024) = __builtin_bit_cast(uint4, o);
                }
            }
            xo = xv;
        };
        auto advance = [&]() {                                       // the pair behind the one in the matrix pipe moves on
            off_f += 8192; off_b += 4096;
            if constexpr (NZ == 2) idx4 += 16;
        };
        if constexpr (!G) {
            // pair pr into acc / cxt, the update of pair pr - 1 out of pacc / pxt
            auto pair = [&](int pr, bool first, f32x16 (&acc)[2], f32x4 (&cxt)[2][4], const f32x16 (&pacc)[2], const f32x4 (&pxt)[2][4]) {
                acc[0] = bias_tile(lds, SYN_LAYERS, 0, 2 * pr, hi); acc[1] = bias_tile(lds, SYN_LAYERS, 0, 2 * pr + 1, hi);
                fetch(first ? off_f : off_f + 8192, cxt);            // consumed during the NEXT pair's MFMAs
                if (first) {
                    pair512<false>(r, lds, hb, acc[0], acc[1]);
                } else {
                    pair512<false>(r, lds, hb, acc[0], acc[1], [&](int kc) {
                        if ((kc & 3) == 0) quad(pr - 1, kc >> 4, (kc >> 2) & 3, pacc, pxt);
                    });
                    advance();
                }
            };
#pragma unroll 1
            for (int pp = 0; pp < 12; ++pp) {
                f32x16 acc_even[2];
                f32x4 xt_even[2][4];
                pair(2 * pp, pp == 0, acc_even, xt_even, acc_odd, xt_odd);
                pair(2 * pp + 1, false, acc_odd, xt_odd, acc_even, xt_even);
            }
        } else {
            // The variants' tiles pass through the LDS; all that is handed from pair to pair in registers is x_t (32 moves), and the
            // two-set form of the loop tips the guided instances' register allocation over (46 spilled registers against 22): one
            // pair per iteration, x_t handed on through xt_odd.
#pragma unroll 1
            for (int pr = 0; pr < 24; ++pr) {
                f32x16 acc0 = bias_tile(lds, SYN_LAYERS, 0, 2 * pr, hi), acc1 = bias_tile(lds, SYN_LAYERS, 0, 2 * pr + 1, hi);
                f32x4 cxt[2][4];
                fetch(pr == 0 ? off_f : off_f + 8192, cxt);          // consumed during the NEXT pair's MFMAs
                if (pr == 0) {
                    pair512<false>(r, lds, hb, acc0, acc1);
                } else {
                    pair512<false>(r, lds, hb, acc0, acc1, [&](int kc) {
                        if ((kc & 3) == 0 && ((kc >> 3) % nvar) == var) quad(pr - 1, kc >> 4, (kc >> 2) & 3, acc_odd, xt_odd);   // quad pair kc >> 3 is this wave's
                    });
                    advance();
                }
                // publish: the chunk barrier that opens the next pair (or the one below, after the last) makes it everybody's;
                // the buffer written now was last read during pair pr - 1, i.e. before every wave's latest barrier
                char* const mine = slab + (pr & 1) * 8192;
                slab_store(mine, 0, acc0);
                slab_store(mine, 1, acc1);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int q = 0; q < 4; ++q) xt_odd[u][q] = cxt[u][q];
            }
        }
        if constexpr (G) __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < 8; ++i)                                  // the last pair's update has nobody to hide behind
            if (!G || ((i >> 1) % nvar) == var) quad(23, i >> 2, i & 3, acc_odd, xt_odd);
    }
    if (stamp) a->dbg[(size_t)blockIdx.x * 32 + 10] = (long long)__builtin_readcyclecounter();
  }
    if (a0->dbg && wave == 0 && lane0 == 0) a0->dbg[(size_t)blockIdx.x * 32 + 11] = (long long)__builtin_readcyclecounter();
    // drain: the look-ahead DMAs still in flight target this workgroup's LDS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// (B,1536,1,32) fp32 <-> fragment order.  One block per (clip, 32-channel tile): 32 channels x 32 frames through LDS.
__global__ __launch_bounds__(256) void k_x_to_fragment(const float* __restrict__ x, float* __restrict__ of, uint4* __restrict__ ob) {
    __shared__ float tile[32][33];          // [channel][frame]
    const int b = blockIdx.x, nf = blockIdx.y, tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256, c = idx >> 5, t = idx & 31;
        tile[c][t] = x[((size_t)b * SYN_C + 32 * nf + c) * 32 + t];
    }
    __syncthreads();
    // fp32: [b][nf][q][lane][r], channel 8q + 4hi + r of token lane & 31; thread = (q, lane)
    {
        const int q = tid >> 6, lane = tid & 63, hi = lane >> 5, tk = lane & 31;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = tile[8 * q + 4 * hi + r][tk];
        if (of) *reinterpret_cast<f32x4*>(of + (((size_t)b * 48 + nf) * 4 + q) * 256 + lane * 4) = v;
    }
    // bf16: [b][nf][c][lane][e], channel 16c + 8(e>>2) + 4hi + (e&3); threads 0..127 = (c, lane)
    if (ob && tid < 128) {
        const int c = tid >> 6, lane = tid & 63, hi = lane >> 5, tk = lane & 31;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)tile[16 * c + 8 * (e >> 2) + 4 * hi + (e & 3)][tk];
        ob[((size_t)b * 48 + nf) * 128 + c * 64 + lane] = __builtin_bit_cast(uint4, o);
    }
}

__global__ __launch_bounds__(256) void k_x_from_fragment(const float* __restrict__ xf, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int b = blockIdx.x, nf = blockIdx.y, tid = threadIdx.x;
    {
        const int q = tid >> 6, lane = tid & 63, hi = lane >> 5, tk = lane & 31;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xf + (((size_t)b * 48 + nf) * 4 + q) * 256 + lane * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[8 * q + 4 * hi + r][tk] = v[r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256, c = idx >> 5, t = idx & 31;
        out[((size_t)b * SYN_C + 32 * nf + c) * 32 + t] = tile[c][t];
    }
}

// The matrix pipe alone, in k_seq's occupancy: one wave per SIMD (the 160 KB of LDS keep a CU to one workgroup), 12 independent 32x32x16 bf16
// accumulators, operands in registers, nothing else in the instruction stream.  What this loop reaches on a box - its clock under the power cap
// included - is the practical ceiling of any kernel built on this MFMA (bench.py: roofline.practical_peak; scripts/ubench/seq_issue.hip is the
// study this comes from).
__global__ __launch_bounds__(kThreads) void k_mfma_rate(float* __restrict__ out, int iters) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63;
    f32x16 acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = zero16();
    // four A and four B operand images of pseudo-random values, taken in turn: the operand buses toggle as they do on real data (one constant
    // operand pair runs ~25 % faster on the same box - the power cap is what sets the clock, and switching activity is what draws the power)
    bf16x8 a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned ha = (unsigned)(lane * 8 + e + 977 * j) * 2654435761u, hb = (unsigned)(lane * 8 + e + 131 * j + 7) * 2246822519u;
            a[j][e] = (__bf16)(((float)(ha >> 16) - 32768.f) * (1.0f / 65536.f));
            b[j][e] = (__bf16)(((float)(hb >> 16) - 32768.f) * (1.0f / 65536.f));
        }
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int rep = 0; rep < 16; ++rep)
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] = MFMA32(a[(i + rep) & 3], b[i & 3], acc[i]);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) sum += acc[i][v];
    if (iters < 0) lds[threadIdx.x] = (char)sum;              // (never: keeps the LDS allocation referenced)
    out[(size_t)blockIdx.x * kThreads + threadIdx.x] = sum;
}

}  // namespace seq
}  // namespace
