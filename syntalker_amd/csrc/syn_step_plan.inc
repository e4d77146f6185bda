// Which kernel runs a denoising step: pure host arithmetic over (batch, flags, device shape).  Plain C++17 with no HIP, no globals and no
// device query, so it compiles and is tested on its own (tests/native/step_plan_host.cpp); syn_kernels.hip includes it inside its
// anonymous namespace and feeds it device_cus() / latency_path_ok().  A new step path is a new StepPath and a new line in plan_step.

constexpr int kPlanT = 32;         // rows (latent frames) of a sequence: SYN_T
constexpr int kPlanXcds = 8;       // XCDs the small-batch kernel deals sequences to: lat::kGroups

// workgroups of a k_seq launch: 4 sequences each; a guided clip's V variants never straddle a workgroup
inline int seq_grid(int n_clips, int n_variants) {
    const int cpw = n_variants == 1 ? 4 : 4 / n_variants;
    return (n_clips + cpw - 1) / cpw;
}

inline int pick_tile(int rows, int cus) {
    // enough workgroups to cover the 256 CUs first, then the larger tile (weight reuse per L2 byte).
    // 128-row tiles exist for the A/B paths only: with the 4-slot weight ring they exceed 256 VGPRs.
    if (rows / 64 >= 192) return 64;
    // more 32-row tiles than CUs would mean a second, mostly empty round of workgroups (257..383 sequences: 0.84 ms per step against
    // 0.52 ms on 64-row tiles, `profiles/r02_diag_batch_sweep.txt`); up to one tile per CU the smaller tile wins (0.41-0.46 against 0.52 ms)
    if ((rows + 31) / 32 > cus) return 64;
    return 32;
}

inline int prefers_fragment_order(int n_clips, int n_variants, int cus) {
    // k_seq runs 4 sequences per CU and pass, k_stack 2; measured per pass at full occupancy (profiles/r02_diag_seq.txt):
    // 1.26 ms against 0.66 ms.  Both quantise to whole passes over the 256 CUs, so the choice follows the pass counts:
    // 1024 / 2048 / 3072 clips -> k_seq, 1280 or 1536 -> k_stack (a second, mostly empty k_seq pass would cost more).
    // Guided batches: the V variants of a clip are the waves of one workgroup (2 clips per workgroup at V = 2, one at V = 3
    // - a wave idles - and 4); k_stack sees V * n_clips sequences.
    if (n_variants < 1 || n_variants > 4) return 0;
    const long wgs = seq_grid(n_clips, n_variants), seqs = (long)n_clips * n_variants;
    // (no minimum fill: from 513 sequences on k_stack needs a second, mostly empty round - 1.10 ms per step whatever the size - where
    // k_seq's single pass of 129..192 workgroups takes 0.88-0.92 ms: 612 k against 492 k clip-steps/s at 544 clips, 763 k against 630 k at 704)
    const long passes_seq = (wgs + cus - 1) / cus, passes_stack = (seqs + 2L * cus - 1) / (2L * cus);
    // (V = 3 leaves a wave of every workgroup idle: measured 1197 us against k_stack's 1120 at 256 clips)
    return passes_seq * (n_variants == 3 ? 255 : 191) < passes_stack * 100 ? 1 : 0;
}

enum StepPath {
    STEP_ERROR,     // refused: StepPlan::error
    STEP_SEQ,       // k_seq: one wave per sequence, latent in fragment order (syn_seq.inc)
    STEP_LAT,       // k_lat: the persistent small-batch kernel (syn_latency.inc) [+ k_guided_update when by_seq]
    STEP_STACK,     // k_stack: the whole step in one token-resident kernel [+ k_combine and the output GEMM when not fuse_out]
    STEP_LAYERS,    // the per-operation A/B path: input GEMM, five kernels per block, [k_combine,] output GEMM
};

struct StepPlan {
    StepPath path = STEP_ERROR;
    const char* error = nullptr;
    bool by_seq = false;      // LAT: a guided batch's SEQUENCES are dealt to the XCDs and k_guided_update combines them
    int tile_rows = 0;        // STACK: 32 or 64; LAYERS: the row tile of every GEMM of the stack
    int tp = 1;               // STACK: workgroups (of one XCD) a 32-row tile is split over: 1, 2 or 4
    bool fuse_out = false;    // STACK: the output stage runs inside k_stack (a single conditioning variant)
    int out_tile = 0;         // STACK without fuse_out, LAYERS: the row tile of the output GEMM
};

struct StepQuery {
    int n_clips, n_variants, m_tile, reserved, x_fragment_order;      // the fields of syn_step
    bool ws_sync, ws_xch, ws_x0v;                                     // whether syn_step has them
    int cus;                                                          // device_cus()
    bool xcd8x32;                                                     // latency_path_ok(): 8 XCDs x 32 CUs
};

inline StepPlan plan_error(const char* msg) { StepPlan p; p.error = msg; return p; }

// reserved: bits 0-1 = 0 automatic / 1 per-operation path / 3 small-batch kernel; bit 2 pins the whole-step kernel (5 = bits 0 and 2: the
// wave-per-sequence kernel); bit 3 switches split tiles off.
inline StepPlan plan_step(const StepQuery& q) {
    const int B = q.n_clips, V = q.n_variants;
    StepPlan p;
    if (q.x_fragment_order || (q.reserved & 7) == 5) {
        // large batches: one wave per sequence, weights streamed once per 128 rows (syn_seq.inc)
        if (!q.x_fragment_order) return plan_error("syn_denoise_step: the wave-per-sequence kernel needs the latent in fragment order (x_fragment_order = 1)");
        if (V > 4) return plan_error("syn_denoise_step: fragment-order latents take at most 4 variants per clip (a clip's variants are the waves of one workgroup)");
        p.path = STEP_SEQ;
        return p;
    }
    const int mode = q.reserved & 3;
    if (mode == 2) return plan_error("syn_denoise_step: kernel selection 2 (two kernels per block) was removed in ABI 8; 1 = the per-operation path");
    // Small batches: the persistent feature-split kernel (syn_latency.inc) beats the token-resident one while a
    // group (XCD) holds at most 4 sequences (measured per step: 161 / 239 / 405 us at 1 / 2 / 4 sequences per
    // group against ~445 us, and 733 us at 8).  Guided batches (V > 1) deal SEQUENCES to the XCDs when the caller
    // provides ws_x0v (each variant's x0_hat is produced on its own XCD, k_guided_update combines them), else whole
    // clips with all their variants.  reserved bit 2 pins the whole-step kernel (A/B runs, bitwise cross-checks
    // against layer modes 1 / 2).
    const bool by_seq = V > 1 && q.ws_x0v;
    const int per_group = by_seq ? (B * V + kPlanXcds - 1) / kPlanXcds : ((B + kPlanXcds - 1) / kPlanXcds) * V;
    // 9..128 sequences (measured: 216-231 us per step at 9..48 sequences, 270 at 64, 312-337 us at 65..128, against
    // 235-400 us of the small-batch kernel at 9..32 and 405-413 us of one workgroup per tile above): the whole-step kernel with every
    // 32-row tile split over 4 (<= 64 sequences) or 2 workgroups of one XCD, see k_stack.  reserved bit 3 (value 8)
    // switches it off, and so does pinning a kernel (bit 2) or a tile size.
    // (129..256 sequences as 64-row tiles split over 2 workgroups: measured in round 5 and slower than one 32-row tile per CU - lab notebook)
    const int seqs = V * B;
    const bool split = mode == 0 && q.m_tile == 0 && !(q.reserved & 12) && q.ws_sync && q.ws_xch && seqs >= 9 && seqs <= 128 && q.xcd8x32;
    if (mode == 3 || (mode == 0 && !split && !(q.reserved & 4) && q.ws_sync && per_group <= 4 && q.xcd8x32)) {
        if (!q.ws_sync) return plan_error("syn_denoise_step: the latency path needs ws_sync");
        if (!q.xcd8x32) return plan_error("syn_denoise_step: the latency path needs a 256-CU (8 XCD x 32) device");
        p.path = STEP_LAT;
        p.by_seq = by_seq;
        return p;
    }
    const int mt = q.m_tile ? q.m_tile : pick_tile(seqs * kPlanT, q.cus);
    p.out_tile = q.m_tile ? q.m_tile : pick_tile(B * kPlanT, q.cus);
    if (mode == 1) {
        p.path = STEP_LAYERS;
        p.tile_rows = mt;
        return p;
    }
    p.path = STEP_STACK;
    p.fuse_out = V == 1;
    p.tile_rows = split ? 32 : mt > 64 ? 64 : mt;      // (the whole-step kernel has no 128-row instance)
    p.tp = !split ? 1 : seqs <= 64 ? 4 : 2;
    return p;
}
