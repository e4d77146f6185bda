/*
 * syn_hip.h — C ABI of libsyn_hip.so: the MI355X (gfx950) denoising-step kernels for SynTalker.
 *
 * The reference (RobinWitch/SynTalker) is pure Python: it has no FFI of its own.  This ABI sits
 * beneath the two Python seams the reference's drivers use:
 *     models/denoiser.py:132      MDM.forward(x, timesteps, y)            -> syn_denoise_step (c_x0=1, c_xt=0, sigma=0)
 *     diffusion/gaussian_diffusion.py:505   GaussianDiffusion.p_sample    -> syn_denoise_step (DDPM coefficients)
 *     diffusion/gaussian_diffusion.py:741   GaussianDiffusion.ddim_sample -> syn_denoise_step (DDIM coefficients)
 *     diffusion/cfg_sampler.py:10-167       the four CFG wrappers         -> syn_denoise_step with n_variants > 1
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no exceptions; every entry point returns 0 on success, <0 on error;
 *     syn_last_error() returns a thread-local message for the last failure.
 *   - every pointer is a DEVICE pointer owned by the caller unless stated otherwise;
 *     nothing is allocated, freed or synchronised inside an entry point (syn_denoise_step_profile excepted), so
 *     all of them can be captured in a hipGraph.  `stream` is a hipStream_t (NULL = default stream).
 *   - "token-major" latent = [clip][frame 0..31][channel 0..1535]; the reference's layout
 *     (B, 1536, 1, 32) is "channel-major".  The sampling loop keeps x token-major across steps.
 *   - bf16 buffers are passed as void*; "packed" weights are in MFMA fragment order, produced
 *     by syn_pack_weight.
 */
#ifndef SYN_HIP_H
#define SYN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYN_ABI_VERSION 9     /* 9: syn_conv1d_wgrad_shares takes the layer's output channels (the share count follows the number of gradient slices a layer is cut in);
                                * syn_conv1d_first_wgrad_tail, syn_bn_block_bwd with dy = NULL, syn_conv1d_train_wgrad_pair, syn_wgrad_sum_job.share_pitch, syn_conv1d_first_wgrad_bn_lin;
                                * 8: the seams of the training step (syn_rows_concat_bf16, syn_embed_rows_bf16, syn_bct_to_rows_bf16, syn_rows_group_sum, syn_touch,
                                * syn_masked_smooth_l1 / _grad on the output Linear's rows), syn_linear_bwd_prep reads a strided / row-repeated dy, syn_pack_job.src_dim,
                                * syn_linear_pair on 128-column tiles, syn_embedding_wgrad ld; superseded kernels and their switches removed;
                                * 7: fused tail of the audio encoder's BasicBlock in training (syn_bn_finalize / syn_bn_apply2 / syn_bn_block_bwd,
                                * syn_conv1d_train_fwd_norm / _wgrad_norm, syn_conv1d_first_fwd_stats / _tiles), syn_test_mfma_rate;
                                * 6: pose formats either side of the RVQ-VAEs - syn_axis_angle_to_rot6d, syn_rot6d_to_axis_angle;
                                * 5: training block entry points - bf16 outputs of syn_ln_fwd / syn_gelu_fwd / syn_attn_fwd, syn_linear_res (residual + DropPath factor
                                * in the GEMM's epilogue), syn_linear_bwd_prep row_scale, syn_linear_pair bias_grad;
                                * 4: syn_model.tape carries its first 4 chunks again behind the last (no wrap test in k_seq's weight stream);
                                * 3: training entry points reworked (syn_ln_bwd add, syn_bn_act_* ws_chunks / beta, syn_conv1d_train_fwd bn_part,
                                * syn_linear_bwd_prep colsum; new: syn_linear_pair / _and_pack, syn_pack_weights, syn_embedding_wgrad, syn_conv1d_first_*) */
#define SYN_D        512   /* hidden width               (models/denoiser.py:19)  */
#define SYN_T        32    /* latent frames per clip     (128 pose frames / 4)    */
#define SYN_C        1536  /* latent channels            (models/denoiser.py:37)  */
#define SYN_FF       1024  /* MLP width                  (models/denoiser.py:20)  */
#define SYN_HEADS    4     /* attention heads x 128      (models/denoiser.py:22)  */
#define SYN_LAYERS   8     /* transformer blocks         (models/denoiser.py:21)  */

int         syn_version(void);
const char* syn_last_error(void);

/* One transformer block (models/timm_transformer/transformer.py:154-198). */
typedef struct syn_layer {
    const float* ln1_g;  const float* ln1_b;      /* norm1 (512)                               */
    const void*  w_qkv;                           /* packed bf16, attn.qkv.weight (1536 x 512)  */
    const void*  w_proj; const float* b_proj;     /* packed bf16 (512 x 512), bias (512)        */
    const float* ln2_g;  const float* ln2_b;      /* norm2 (512)                                */
    const void*  w_fc1;  const float* b_fc1;      /* packed bf16 (1024 x 512), bias (1024)      */
    const void*  w_fc2;  const float* b_fc2;      /* packed bf16 (512 x 1024), bias (512)       */
} syn_layer;

/* Everything the step needs that depends only on the weights. */
typedef struct syn_model {
    const void*  w_in;      /* packed bf16 (512 x 1536): folded input matrix A   */
    const float* te;        /* [n_te][512] time_embed(pe[t]) . W2a^T, row = ORIGINAL timestep    */
    int32_t      n_te;
    const float* rot_cos;   /* [32][32] cos(pos * inv_freq[j])   (models/denoiser.py:324-343)    */
    const float* rot_sin;   /* [32][32]                                                          */
    syn_layer    layer[SYN_LAYERS];
    const void*  w_out;     /* packed bf16 (1536 x 512): output_process.poseFinal.weight         */
    const float* b_out;     /* (1536)                                                            */
    /* the same weights as ONE contiguous tape of 1 KB MFMA fragments in consumption order + per-block bias sets, for the
     * wave-per-sequence step kernel (large batches; host: syntalker_amd/tape.py).  NULL = that kernel is never chosen. */
    const void*  tape;        /* bf16 [tape_chunks + 4][16 fragments][64 lanes][8] (1 KB fragments): the step's chunks followed by the
                               * first 4 of them once more (ABI 4: the kernel's DMA look-ahead runs across the step boundary)      */
    const float* tape_bias;   /* [9][4096]                                                        */
    int32_t      tape_chunks; /* 2256 chunks of 16 fragments (36 096 fragments, 35.25 MB)           */
} syn_model;

/* One denoising step over n_clips clips, each evaluated under n_variants conditionings
 * (classifier-free guidance as ONE fused batch of n_variants*n_clips sequences). */
typedef struct syn_step {
    int32_t n_clips;        /* B                                                                 */
    int32_t n_variants;     /* V >= 1                                                            */
    int32_t m_tile;         /* rows per workgroup: 0 = auto, else 32 / 64 / 128                  */
    int32_t reserved;       /* kernel selection: 0 = auto, one rule (plan_step in csrc/syn_step_plan.inc): the small-batch kernel while an XCD holds at most
                               4 sequences (ws_sync != NULL; sequences are dealt to the 8 XCDs when V == 1 or ws_x0v != NULL - up to 32 of them - else
                               whole clips with their V variants), unless the whole-step kernel's split tiles apply (9..128 sequences, ws_sync and
                               ws_xch != NULL); else the whole-step kernel on whole tiles; 4 = whole-step kernel always;
                               3 = small-batch kernel always; 1 = five kernels per block (the plain restatement the whole-step kernel is checked against bit for bit);
                               5 = wave-per-sequence kernel always (needs x_fragment_order = 1);
                               +8 = never split a tile over several workgroups (see ws_xch)               */
    /* conditioning, row (v*B + b)*32 + frame */
    const float*   cond;    /* [V*B*32][512] per-clip term: cbias + c_frame + seed/style term    */
    const int32_t* t_model; /* [V*B] ORIGINAL timestep -> row of syn_model.te                    */
    const float*   cfg_w;   /* [3][V] weights of the variants for output channels 0:512, 512:1024,
                               1024:1536; NULL iff V == 1.  With cfg_w_clip_stride = 3 V (below):
                               [B][3][V], one table per clip - the reference's per-sample guidance
                               scales, y['scale'].view(-1, 1, 1, 1) (diffusion/cfg_sampler.py:28,54,167) */
    /* state, token-major */
    const float*   x_t;       /* [B*32][1536] fp32                                               */
    const void*    x_t_bf16;  /* [B*32][1536] bf16 copy of x_t (GEMM operand)                    */
    const float*   noise;     /* [B*32][1536] fp32 N(0,1) to inject, or NULL                     */
    const uint64_t* rng;      /* used when noise == NULL: device {seed, first_clip} -> the output GEMM's epilogue
                                 draws N(0,1) itself, identical to syn_randn(seed, stream_id = t_coef[clip],
                                 first_index = first_clip*32*1536); NULL = no noise term            */
    const float*   coef;      /* [n][4] rows (c_x0, c_xt, sigma, unused)                         */
    const int32_t* t_coef;    /* [B] row of coef used by each clip                               */
    float*         x_next;      /* [B*32][1536] = c_x0*x0_hat + c_xt*x_t + sigma*noise; may alias x_t */
    void*          x_next_bf16; /* bf16 copy of x_next; may alias x_t_bf16                       */
    float*         pred_x0;     /* [B*32][1536] x0_hat, or NULL                                  */
    /* workspace (caller-owned, contents undefined on return); R = V*B*32 rows */
    float* ws_h;      /* [R][512]  fp32 residual stream                                          */
    void*  ws_xn;     /* [R][512]  bf16 normalised activations                                   */
    void*  ws_q;      /* [R][512]  bf16                                                          */
    void*  ws_k;      /* [R][512]  bf16                                                          */
    void*  ws_vt;     /* [V*B*4*128][32] bf16, V transposed per (clip, head)                     */
    void*  ws_o;      /* [R][512]  bf16 attention output                                         */
    void*  ws_hid;    /* [R][1024] bf16 MLP hidden                                               */
    void*  ws_hc;     /* [3][B*32][512] bf16 guidance-combined stream (only if V > 1)            */
    uint32_t* ws_sync; /* [320] u32, zeroed ONCE by the caller; small-batch path only (group-barrier
                          counters; word 256 = sticky error flag: a barrier wait ran out)        */
    float* ws_x0v;     /* [V*B*32][1536] fp32 or NULL; small-batch path with V > 1: lets the variants of a clip run on
                          different XCDs (each writes its x0_hat here, a small second kernel combines them)   */
    float* ws_xch;     /* [V*B][8][32*512] fp32 or NULL; with it (and ws_sync) batches of 9..128 sequences run the whole-step
                          kernel with every 32-row tile split over 2 or 4 workgroups of one XCD (heads / MLP slices / output
                          chunks dealt to the members, partial residual streams exchanged through these slots)      */
    int32_t x_fragment_order; /* 0: x_t / x_t_bf16 / noise / x_next / pred_x0 are token-major (above); 1: they are in the
                          wave-per-sequence kernel's fragment order (syn_x_to_fragment), and that kernel runs the step
                          (n_variants <= 4, syn_model.tape non-NULL; of the workspaces only cfg_w is used).  syn_prefers_fragment_order() says when the
                          library would like a caller to keep its latent that way.                                   */
    int32_t cfg_w_clip_stride; /* (ABI 8) floats between the cfg_w tables of consecutive clips: 0 = one table for the batch, 3 * n_variants = one per clip */
} syn_step;

/* 1 when a step over n_clips x n_variants is best run by the wave-per-sequence kernel, i.e. the caller should keep the
 * latent in fragment order for the whole loop (batches whose passes of 4 sequences per CU beat the token-resident kernel's passes
 * of 2: 513..1024, 1537..2048, ... sequences; the <= 4
 * variants of a guided clip are the waves of one workgroup and meet in the output stage through LDS); 0 otherwise. */
int32_t syn_prefers_fragment_order(int32_t n_clips, int32_t n_variants);

/* Enqueue one full step on `stream`: one kernel (k_stack, or k_lat for small batches; + k_guided_update when the
 * variants of a small guided batch were dealt to different XCDs), or the 42-kernel A/B path (reserved = 1). */
int syn_denoise_step(const syn_model* model, const syn_step* step, void* stream);

/* In-painting (diffusion/gaussian_diffusion.py:316-320, y['inpainting_mask'] / y['inpainted_motion']): the model's x0_hat is
 * replaced by `known` wherever `keep` is set - after the guidance combination, before the update x_next = c_x0*x0_hat + c_xt*x_t +
 * sigma*noise, and before pred_x0 is written (the reference returns the blended pred_xstart).  Both tensors are token-major like x_t and,
 * like it, read four consecutive channels at a time: keep must be 4-byte aligned and known 16-byte aligned. */
typedef struct syn_edit {
    const uint8_t* keep;    /* [B*32][1536] nonzero = keep the known value                      */
    const float*   known;   /* [B*32][1536] fp32, the values to keep                            */
} syn_edit;

/* syn_denoise_step with the blend above in the output stage of whichever token-major kernel runs the step; the same contract
 * (nothing allocated or synchronised, graph-capturable).  edit == NULL, or both of its pointers NULL: exactly syn_denoise_step.
 * Refused: exactly one of keep / known NULL; x_fragment_order = 1 or reserved = 5 (the wave-per-sequence kernel takes no edit, so a
 * batch with an edit runs token-major at every size).  syn_denoise_steps has no such variant. */
int syn_denoise_step_edit(const syn_model* model, const syn_step* step, const syn_edit* edit, void* stream);

/* Loop helper: fills t_coef[0..n_t_coef) with sched[2i] and t_model[0..n_t_model) with sched[2i + 1], i = *counter, then
 * advances *counter - a whole p_sample_loop iteration (gaussian_diffusion.py:714-739) becomes one graph replay
 * (this launch + syn_denoise_step) with no host work in between. */
int syn_step_advance(const int32_t* sched, int32_t* counter, int32_t* t_model, int32_t n_t_model, int32_t* t_coef, int32_t n_t_coef,
                     void* stream);
/* The same for the next n_steps steps at once: row s of t_model [n_steps][n_t_model] / t_coef [n_steps][n_t_coef] belongs
 * to step *counter + s; *counter advances by n_steps.  A graph of n_steps captured steps, each pointing at its own row,
 * needs one of these per replay instead of one per step. */
int syn_steps_advance(const int32_t* sched, int32_t* counter, int32_t* t_model, int32_t n_t_model, int32_t* t_coef,
                      int32_t n_t_coef, int32_t n_steps, void* stream);

/* Pseudo linear multistep sampling (diffusion/gaussian_diffusion.py:1004-1086, orders 2-4).  A PLMS step is syn_denoise_step with a coefficient
 * row that carries the Adams-Bashforth weight of the step's own noise estimate and noise = H, the weighted sum of the earlier estimates;
 * syn_plms_update keeps that history.  One row of its table per launch of a loop: */
typedef struct syn_plms_row {
    float   r, inv_m;   /* e_new = (r * x_t - pred_x0) * inv_m: sqrt_recip_alphas_cumprod[t], 1 / sqrt_recipm1_alphas_cumprod[t]            */
    float   h_x;        /* H = h_x * x_t + w_new * e_new + sum_k w[k] * ring[k]: what the NEXT step injects                                */
    float   w_new;
    float   w[3];       /* by ring slot; a slot with weight 0 is not read                                                                   */
    int32_t store;      /* ring slot e_new overwrites, -1: e_new is not kept.  A row with store < 0 and every weight 0 does nothing          */
} syn_plms_row;

/* After a step that read x_t and wrote pred_x0 (x_next != x_t: the step must not have overwritten its input): row *counter - back of
 * table [n_rows] (outside the table: nothing happens) -> e_new into ring [3][n], the next step's H into h [n].  Element-wise over n floats
 * (a multiple of 4; every pointer 16-byte aligned), the same for token-major and fragment-order latents.  `counter` is the step counter
 * syn_step_advance / syn_steps_advance maintain, `back` how many steps it is ahead of the step this call follows (1 after syn_step_advance;
 * n_steps - s for step s of a syn_steps_advance row set).  Graph-capturable like everything else. */
int syn_plms_update(const syn_plms_row* table, int32_t n_rows, const int32_t* counter, int32_t back, const float* x_t, const float* pred_x0,
                    float* ring, float* h, int64_t n, void* stream);

/* The variational bound per timestep (diffusion/gaussian_diffusion.py:1201-1234, 1548-1603: calc_bpd_loop / _vb_terms_bpd).  No timestep of
 * that loop depends on another, so clips x timesteps are one batch of independent sequences: syn_denoise_step evaluates the model on all of
 * them (t_model / t_coef hold one timestep per sequence) and syn_bpd_terms reduces each to the loop's three scalars.  One row per timestep: */
typedef struct syn_bpd_row {
    float   c1, c2;     /* posterior_mean_coef1 / 2[t]: mean = c1 * pred_x0 + c2 * x_t                                                    */
    float   log_var;    /* posterior_log_variance_clipped[t] (FIXED_SMALL: the log-variance of q's posterior and of p)                     */
    float   r, inv_m;   /* eps = (r * x_t - pred_x0) * inv_m, as syn_plms_row                                                              */
    int32_t first;      /* nonzero at t == 0: vb is the decoder NLL (diffusion/losses.py discretized_gaussian_log_likelihood), else the KL */
} syn_bpd_row;

/* Sequence i of n_seq: row t_row[i] of table [n_rows], x_start of clip clip[i] (clip = NULL: clip i, n_seq <= n_clips), its own 49 152
 * floats of x_t, noise and pred_x0 -> out [3][n_seq]: vb in bits per dimension, xstart_mse = mean((pred_x0 - x_start)^2), mse =
 * mean((eps - noise)^2).  An index outside its table gives NaN in the three outputs of that sequence and reads nothing.  One workgroup per
 * sequence, no atomics; the sum over a sequence's 16-byte groups is exact (csrc/syn_bpd.inc), so a sequence's outputs are bitwise the same
 * on every run, whatever n_seq is and whichever sequences share the launch, and for every order of the groups: a sequence's floats are
 * contiguous in both latent layouts and the kernel does not care which it is given, provided the four tensors share it.  x_start, x_t,
 * noise and pred_x0 16-byte aligned.  Enqueues on `stream`, allocates nothing, graph-capturable. */
int syn_bpd_terms(const syn_bpd_row* table, int32_t n_rows, const int32_t* t_row, const int32_t* clip, const float* x_start, int32_t n_clips,
                  const float* x_t, const float* noise, const float* pred_x0, int32_t n_seq, float* out, void* stream);

/* Gradient-guided sampling (diffusion/gaussian_diffusion.py:427-503, 549-605, 765-848; additive, SYN_ABI_VERSION stays 9).  The denoiser is differentiated
 * with respect to x_t only: x_t enters through h0 = rotary(x_t^T A^T + cond + TE[t]) (A: the folded input chain, 512 x 1536), the eight blocks are
 * syn_train_stack_fwd / syn_train_stack_bwd, the output Linear and its data gradient syn_linear.
 * syn_guide_in_fwd: x_bct (n_x, 1536, 1, 32) fp32 -> h0 [32 n_seq][512] fp32 in one launch.  Sequence s reads clip s % n_x (the conditioning variants of
 * a clip share its latent), row 32 s + f of cond and row t_model[s] of te [n_te][512] (clamped into the table); a_packed = syn_pack_weight of A.
 * Sequences n_live .. n_seq - 1 are padding: their rows of h0 are zero and nothing is read for them (cond, t_model hold n_live sequences).
 * syn_guide_in_bwd: the adjoint, dh0 [32 n_seq][512] -> dx_bct (n_seq, 1536, 1, 32) fp32 (inverse rotation, GEMM against at_packed = syn_pack_weight of
 * A^T [1536][512], channel-major store); accumulate != 0: dx_bct += (a read-modify-write by the element's one owner: no atomics, and the sum over
 * the variants of a clip, one call after the other on one stream, is bitwise reproducible).  Every pointer 16-byte aligned. */
int syn_guide_in_fwd(const float* x_bct, int32_t n_x, const void* a_packed, const float* cond, const float* te, int32_t n_te, const int32_t* t_model,
                     const float* rot_cos, const float* rot_sin, int32_t n_live, int32_t n_seq, float* h0, void* stream);
int syn_guide_in_bwd(const float* dh0, const void* at_packed, const float* rot_cos, const float* rot_sin, int32_t n_seq, int32_t accumulate, float* dx_bct,
                     void* stream);
/* The update behind cond_fn's gradient `grad`, element-wise on (n_clips, 1536, 1, 32) fp32; clip b takes row t_idx[b] of coef [n_rows][8] (an index
 * outside the table: NaN in that clip's output, nothing read for it):
 *   mode 0 (condition_mean, p_sample)    row {variance, exp(0.5 log_variance)}; a = the posterior mean:
 *          out = a + variance grad + [t != 0] sigma noise
 *   mode 1 (condition_score, ddim_sample) row {sqrt(1 - ab), sqrt(1 / ab), sqrt(1 / ab - 1), sqrt(ab_prev), sqrt(1 - ab_prev - sigma^2), sigma}; a = x_t:
 *          eps = (r a - pred_x0) / m - sqrt(1 - ab) grad;  x0' = r a - m eps;  eps' = (r a - x0') / m;  out = x0' sqrt(ab_prev) + dir eps' + [t != 0] sigma noise
 * noise: (n_clips, 1536, 1, 32), or NULL and draw != 0: element (b, channel c, frame f) is element ((first_clip + b) 32 + f) 1536 + c of
 * syn_randn(seed, stream_id = t_idx[b]) - bitwise the step kernels' draw; NULL and draw == 0: no noise.  Clips with t_idx == 0 or sigma == 0 neither read
 * nor draw.  pred_x0 is left as it is (the reference returns the unguided one, :557, :791, :848). */
int syn_guide_update(int32_t mode, const float* a, const float* pred_x0, const float* grad, const float* noise, int32_t draw, uint64_t seed,
                     uint64_t first_clip, const float* coef, int32_t n_rows, const int32_t* t_idx, int32_t n_clips, float* out, void* stream);

/* Motion metrics behind the sampler (the reference's test(), diffusion_rvqvae_trainer.py:626-684, 722-728; utils/metric.py; utils/plot_script.py:15-52;
 * additive, SYN_ABI_VERSION stays 9; csrc/syn_joints.inc).  fp32 device tensors unless noted; deterministic, no floating-point atomics; every call
 * enqueues on `stream`, allocates nothing and is graph-capturable.
 *
 * syn_fk_joints: forward kinematics of a tree of n_joints <= 64 joints.  parents [n_joints] int32, every parent an EARLIER joint, roots -1 (an entry
 * that is not an earlier joint is taken as a root); rest_joints (n_takes, n_joints, 3); rot (n_frames, n_joints, 3) axis-angle (rot6d == 0: Rodrigues,
 * exact at 0) or (n_frames, n_joints, 6) (rot6d != 0: the Gram-Schmidt of syn_rot6d_to_axis_angle's first half); transl (n_frames, 3) or NULL.  Frame n
 * belongs to take take_of_frame[n], or to take n / frames_per_take where take_of_frame is NULL; a take outside [0, n_takes) gives NaN joints.
 * pose_mean [n_joints][3] or NULL: added to the axis-angle vectors before Rodrigues - SMPL-X's `full_pose += pose_mean`, i.e. the hands' mean pose of a
 * model built with flat_hand_mean = False, as the reference builds it (axis-angle input only: refused with rot6d != 0).
 * joints_out (n_frames, n_joints, 3): G_j = G_parent . [R_j | rest_j - rest_parent], the root at rest_0 (+ transl). */
int syn_fk_joints(const int32_t* parents, int32_t n_joints, const float* rest_joints, int32_t n_takes, const float* rot, int32_t rot6d, const float* transl,
                  const int32_t* take_of_frame, int32_t frames_per_take, int64_t n_frames, const float* pose_mean, float* joints_out, void* stream);
/* joints_in (n_takes, n_frames >= 2, n_joints, 3) -> speed (n_takes, n_frames, n_joints): forward / central / backward differences times fps within each
 * take, Euclidean norm per joint, divided by mmae [n_joints] where it is not NULL (metric.py:98-109). */
int syn_joint_speed(const float* joints_in, int32_t n_takes, int32_t n_frames, int32_t n_joints, float fps, const float* mmae, float* speed, void* stream);
/* vel (n_takes, n_frames, n_joints) -> mask (n_takes, t_end - t_start, n_joints) uint8, 0 <= t_start <= t_end <= n_frames: slice index j of joint i is a
 * beat where vel[t_start + j, i] is strictly below its `order` neighbours on either side (indices clipped to the slice: argrelextrema's mode 'clip')
 * AND vel[j, i] > threshold - frame j of the whole take, as the reference has it (metric.py:111-127). */
int syn_motion_beats(const float* vel, int32_t n_takes, int32_t n_frames, int32_t n_joints, int32_t t_start, int32_t t_end, int32_t order, float threshold,
                     uint8_t* mask, void* stream);
/* Beat consistency (metric.py:205-241).  mask as above (n_slice <= 16000: n_slice / 2 + 1 doubles of LDS per workgroup); upper_body [n_upper] int32 joint indices; onsets: fp64 seconds, take k's are
 * onsets[onset_offsets[k] .. onset_offsets[k + 1]) (at least one per take: the host's to check).  per_joint (n_takes, n_upper): the mean over a take's
 * onsets of exp(-d^2 / 2 sigma^2), d the distance to the joint's nearest beat time j / pose_fps (0 for a joint without beats); bc [n_takes]: the mean
 * over the joints. */
int syn_beat_align(const uint8_t* mask, int32_t n_takes, int32_t n_slice, int32_t n_joints, const int32_t* upper_body, int32_t n_upper, const double* onsets,
                   const int32_t* onset_offsets, double pose_fps, float sigma, float* per_joint, float* bc, void* stream);
/* L1 diversity (metric.py:12-27): out[k] (fp64) = sum over take k of x (n_takes, n, channels) of |x - the take's mean over its rows|; x is only read.
 * fp64 sums in an order fixed by (n, channels) alone: bitwise the same on every run, for every `blocks` (the grid of the two passes; 0 = the library's
 * choice) and whichever takes share the call.  workspace: syn_l1div_workspace_bytes(n_takes, n, channels) bytes (-1 for counts
 * below 1), 8-byte aligned. */
int64_t syn_l1div_workspace_bytes(int32_t n_takes, int64_t n, int32_t channels);
int syn_l1div(const float* x, int32_t n_takes, int64_t n, int32_t channels, void* workspace, int32_t blocks, double* out, void* stream);
/* HumanML3D features (n_seq, n_frames, channels >= 4 + 3 (joints_num - 1)) -> joints_out (n_seq, n_frames, joints_num, 3) (plot_script.py:15-52): root yaw
 * = exclusive prefix sum of channel 0, quaternion (cos a, 0, sin a, 0) as the reference has it, root xz = inclusive prefix sum of the previous frame's
 * velocity turned by its inverse, y = channel 3; the joints turned the same way and moved by the root's xz.  root_quat (n_seq, n_frames, 4) or NULL: the
 * root quaternions (recover_root_rot_pos's first result; joint 0 of joints_out is its second).  One workgroup scan per sequence. */
int syn_recover_from_ric(const float* data, int32_t n_seq, int32_t n_frames, int32_t channels, int32_t joints_num, float* joints_out, float* root_quat,
                         void* stream);

/* The SMPL-X mesh: linear blend skinning of the model's vertices, what smplx(...)["vertices"] gives test() (:640-675) and the renderers (additive,
 * SYN_ABI_VERSION stays 9; csrc/syn_mesh.inc).  fp32 device tensors unless noted; deterministic, no floating-point atomics; every call
 * enqueues on `stream`, allocates nothing and is graph-capturable.  J = n_joints, P = 9 (J - 1) pose-corrective directions, E = n_expr expression
 * directions, Kc = P + E <= 1024, Kcp = Kc rounded up to 16, Vp = n_verts rounded up to 64.
 *
 * syn_mesh_pack_dirs: posedirs (n_verts, 3, n_pose) and exprdirs (n_verts, 3, n_expr) (NULL with n_expr == 0), as the model file lays them out, ->
 * out [Vp / 16][Kcp / 16][3][64][4] floats (Vp * 3 * Kcp): the B fragments of v_mfma_f32_16x16x4_f32, lane l of tile t, group g, plane p, element u =
 * direction k = 16 g + 4 (l >> 4) + u (pose correctives first, then expressions) of coordinate p of vertex 16 t + (l & 15); zero for k >= Kc and for
 * vertices >= n_verts. */
int syn_mesh_pack_dirs(const float* posedirs, const float* exprdirs, int32_t n_verts, int32_t n_pose, int32_t n_expr, float* out, void* stream);
/* The joint transforms of n_frames poses: syn_fk_joints' tree walk (2 <= n_joints <= 64; parents, rest_joints (n_takes, n_joints, 3), pose_mean,
 * take_of_frame / frames_per_take as there: a take outside [0, n_takes) gives NaN transforms and joints, nothing read for it).  pose (n_frames, J, 3)
 * axis-angle.  With n_expr > 0 frame n's rest joints are its take's + joint_dirs (J, 3, n_expr) . expression (n_frames, n_expr) - SMPL-X regresses
 * the joints from the shaped vertices, expression term included; n_expr == 0: no expression (zero), whatever the mesh's directions hold.  kc: the
 * contraction length of the syn_mesh_vertices call that follows, 9 (J - 1) + n_expr <= kc <= 1024.  Outputs:
 *   feat (n_frames, Kcp)          R_j - I of joints 1 .. J - 1 row-major (the pose feature), then the expression, then zeros up to Kcp = kc rounded up
 *                                 to 16: syn_mesh_vertices' A rows
 *   xforms (n_frames, J, 3, 4)    the rows of A_j = [G_j^R | G_j^t - G_j^R J_rest,j], G_j = G_parent . [R_j | J_rest,j - J_rest,parent]
 *   joints_out (n_frames, J, 3)   G_j^t + transl (n_frames, 3) (or NULL).  With n_expr == 0 they are written by syn_fk_joints' own kernel: its bits, for the
 *                                 same arguments */
int syn_fk_transforms(const int32_t* parents, int32_t n_joints, const float* rest_joints, int32_t n_takes, const float* pose, const float* pose_mean,
                      const float* joint_dirs, const float* expression, int32_t n_expr, int32_t kc, const float* transl, const int32_t* take_of_frame,
                      int32_t frames_per_take, int64_t n_frames, float* feat, float* xforms, float* joints_out, void* stream);
/* vertices_out (n_frames, n_verts, 3) = sum_j w_vj (A_j^R v_posed + A_j^t) + transl, v_posed = v_shaped[take] + dirs . feat, in one kernel: v_posed
 * stays in the MFMA accumulators.  dirs_packed: syn_mesh_pack_dirs' output for the same n_verts and kc; feat, xforms: syn_fk_transforms' (all three
 * 16-byte aligned); v_shaped (n_takes, n_verts, 3); the skin weights as fixed-width lists, skin_index / skin_weight (n_verts, width), 1 <= width <=
 * n_joints, entries with weight 0 skipped (the padding of a shorter list), indices clamped to [0, J).  A take outside [0, n_takes): NaN vertices.  Every
 * element is summed in an order fixed by kc and the vertex's list: a frame's vertices are bitwise the same whichever frames share the call. */
int syn_mesh_vertices(const float* dirs_packed, int32_t n_verts, int32_t kc, const float* feat, const float* xforms, int32_t n_joints,
                      const float* v_shaped, int32_t n_takes, const int32_t* skin_index, const float* skin_weight, int32_t width, const float* transl,
                      const int32_t* take_of_frame, int32_t frames_per_take, int64_t n_frames, float* vertices_out, void* stream);
/* test()'s face numbers (:672-673) of rec, tar (n, channels): out[0] = mean (rec - tar)^2; out[1] = mean |(rec[1:] - tar[:-1]) - (tar[1:] - tar[:-1])|
 * as the reference writes it (fp32 differences), NaN for n == 1.  fp64 sums in an order fixed by (n, channels) alone: bitwise the same on every run and
 * for every `blocks` (the grid; 0 = the library's choice).  workspace: syn_vertex_losses_workspace_bytes(n, channels) bytes (-1 for counts below 1),
 * 8-byte aligned like out. */
int64_t syn_vertex_losses_workspace_bytes(int64_t n, int32_t channels);
int syn_vertex_losses(const float* rec, const float* tar, int64_t n, int32_t channels, void* workspace, int32_t blocks, double* out, void* stream);

/* Drawing the mesh: the scene of the reference's utils/fast_render.py:16-43 (one mesh, one orthographic camera, one directional light, one uniform
 * colour) as a software rasteriser in three stages (additive, SYN_ABI_VERSION stays 9; csrc/syn_render.inc).  Every call enqueues on
 * `stream`, allocates nothing, is graph-capturable, deterministic and uses no atomics of any kind; a frame's output is bitwise the same whichever frames
 * share the call.  width, height: 1 .. 8192 pixels, row 0 on top.  faces (n_faces, 3) int32 vertex indices; a face with an index outside
 * [0, n_verts) is skipped by every stage.
 *
 * syn_render_project: vertices (n_frames, n_verts, 3) in world space, view_3x4 = the first three rows of the inverse camera pose (12 floats on the
 * device) ->
 *   xy_sub (n_frames, n_verts, 2) int32   rint(16 x_pix), rint(16 y_pix): x_pix = W/2 + x_cam (H/2)/ymag, y_pix = H/2 - y_cam (H/2)/ymag (square
 *                                         pixels, ymag spans half the height); INT32_MIN, INT32_MIN for a vertex that is not finite; finite positions
 *                                         are clamped to +-2^30
 *   z (n_frames, n_verts)                 -z_cam, the distance in front of the camera
 *   normal (n_frames, n_verts, 3)         normalise(sum (p1 - p0) x (p2 - p0)) over the vertex's faces in ascending face index (zero for a zero sum),
 *                                         in world space.  vf_offsets (n_verts + 1), vf_faces (n_incident): the vertex -> faces CSR index, built once
 *                                         on the host.  Faces with a vertex that is not finite are left out of the sum.
 * syn_render_raster: -> face_id (n_frames, height, width) int32 (-1: background), depth (n_frames, height, width) fp32 (+inf: background).  The sample
 * of pixel (i, j) is (16 i + 8, 16 j + 8) in xy_sub's units.  A face is oriented to a positive doubled area A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0)
 * (vertices 1 and 2 swap otherwise); with E_ab(p) = (bx - ax)(py - ay) - (by - ay)(px - ax), w0 = E_12, w1 = E_20, w2 = E_01 in int64, a sample is
 * covered when every w > 0, or = 0 on a top (dy = 0, dx > 0) or left (dy < 0) edge.  Dropped whole: faces of zero area, with a sentinel vertex, or with
 * a vertex more than 16 max(width, height) units (one image side) outside a border; faces partly outside the image are clipped by the pixel loop.
 * Depth = ((w0 z0 + w1 z1) + w2 z2) / A in fp32, w and A converted from their integers, every operation rounded on its own; a fragment outside
 * [znear, zfar] is rejected; the nearer fragment wins, on equal depth the lower face index.  workspace: syn_render_workspace_bytes(n_frames, n_faces)
 * bytes (-1 for counts below 1), 16-byte aligned; xy_sub 8-byte aligned.
 * syn_render_shade: -> rgb (n_frames, height, width, 3) bytes.  Covered pixel: b = w / A, n = normalise((b0 n0 + b1 n1) + b2 n2), c = base *
 * min(1, ambient + diffuse * max(0, n . light)), channel = rint(255 c); light = the unit vector towards the light, world space; no culling, no normal
 * flip.  Other pixels: the background bytes.  A Lambert term of this project's own, not pyrender's shader. */
int64_t syn_render_workspace_bytes(int64_t n_frames, int32_t n_faces);
int syn_render_project(const float* vertices, int64_t n_frames, int32_t n_verts, const float* view_3x4, int32_t width, int32_t height, float ymag,
                       const int32_t* faces, int32_t n_faces, const int32_t* vf_offsets, const int32_t* vf_faces, int32_t n_incident, int32_t* xy_sub,
                       float* z, float* normal, void* stream);
int syn_render_raster(const int32_t* xy_sub, const float* z, int64_t n_frames, int32_t n_verts, const int32_t* faces, int32_t n_faces, int32_t width,
                      int32_t height, float znear, float zfar, void* workspace, int32_t* face_id, float* depth, void* stream);
int syn_render_shade(const int32_t* face_id, const int32_t* xy_sub, const float* normal, int64_t n_frames, int32_t n_verts, const int32_t* faces,
                     int32_t n_faces, int32_t width, int32_t height, float light_x, float light_y, float light_z, float base_r, float base_g, float base_b,
                     float ambient, float diffuse, int32_t background_r, int32_t background_g, int32_t background_b, uint8_t* rgb, void* stream);

/* Stick figures of h3d takes: the scene of the reference's utils/plot_script.py:86-177 (one perspective camera, a translucent ground rectangle, the
 * root's past trajectory, 5 or 15 polylines) as a rasteriser of thick lines (additive, SYN_ABI_VERSION stays 9; csrc/syn_plot.inc).  Every
 * call enqueues on `stream`, allocates nothing, is graph-capturable, deterministic and uses no atomics of any kind; a frame's output depends on the
 * take's trajectory, that frame's joints and its index alone.  size: 1 .. 4096 pixels a side, row 0 on top.  Positions are in units of 1/16 pixel.
 *
 * syn_plot_setup: data (n_frames, n_joints, 3) the prepared joints of the frames to draw, trajec (n_take, 2) the whole take's root (x, z), index
 * (n_frames) int32 on the device: each frame's position in the take (outside [0, n_take): no ground, no trajectory), bounds {min x, max x, min z,
 * max z} of the take, segments (n_segments, 4) int32 {joint a, joint b, layer >= 2, half-width R} with layers ascending, camera 22 doubles: the 4 x 4 projection M row by row,
 * then the 2 x 3 map A from projected (u, v) to pixel (col, row).  n_slots >= n_segments + max(0, max index - 1).  It writes into the workspace
 *   records (n_frames, n_slots, 8) int32  {ax, ay, bx, by, T, R | layer << 16, x0 | x1 << 16, y0 | y1 << 16} per slot, in paint order: the frame's
 *                                         max(0, index - 1) trajectory segments trajec[k] - trajec[index] -> trajec[k + 1] - trajec[index] on y = 0
 *                                         (fp32 differences; layer 1, half-width traj_half_width), then the chain segments in table order; every
 *                                         other slot, and a dropped segment, is {0, 0, 0, 0, -1, 0, 1, 1} (x0 > x1: no pixel)
 *   grounds (n_frames, 24) int32          {corners n, slots of the frame, x0 | x1 << 16, y0 | y1 << 16, n x (x, y), zeros}: the quad [min x - tx, max x -
 *                                         tx] x [min z - tz, max z - tz] on y = 0 ((tx, tz) = trajec[index], fp32 differences), n = 0 when nothing is left
 * A point p becomes clip = M p, each used row (0, 1, 3) summed as ((m0 x + m1 y) + m2 z) + m3, then (u, v) = (clip.x / clip.w, clip.y / clip.w), col =
 * (a00 u + a01 v) + a02, row = (a10 u + a11 v) + a12, and is snapped to rint(16 col), rint(16 row): fp64, every operation rounded on its own.  A
 * segment with an end that is not finite, with R outside [1, min(4095, 16 size)] or a joint outside [0, n_joints) is dropped.  A segment that crosses
 * w = 1/16 is cut there (the end behind becomes in + t (out - in), t = (in.w - 1/16) / (in.w - out.w), w = 1/16); wholly behind, it is dropped.  A
 * segment with a snapped end more than 16 size units (one image side: the guard band) beyond a border is dropped whole.  T = isqrt(R^2 |b - a|^2), the
 * exact integer root; -1 for a segment of zero length (a disc).  The pixel box holds every pixel with a sample in [min - R, max + R], clipped to the
 * image.  The ground is clipped, not dropped: in clip space against w >= 1/16, then in pixels against the four sides of the guard band (corner = in + t
 * (out - in), t = (bound - in.c) / (out.c - in.c), the clipped coordinate set to the bound), snapped, clamped to the band, consecutive duplicates
 * removed and oriented to a positive doubled area: up to 9 corners.
 * syn_plot_draw: -> rgb (n_frames, size, size, 3) bytes from the same workspace.  Pixel (i, j) has 16 samples (16 i + 2 + 4 u, 16 j + 2 + 4 v), u, v = 0 .. 3.
 * A segment a-b covers a sample s when 0 <= (s - a).(b - a) <= |b - a|^2 and |(b - a) x (s - a)| <= T, or |s - a|^2 <= R^2, or |s - b|^2 <= R^2 (a capsule:
 * round caps and joins), all in int64.  A layer's 16-bit mask is the OR over its segments; with k = popcount(mask) a line layer paints c = (c (16 - k) +
 * colour k + 8) >> 4 per channel.  The ground covers a sample when every edge value E_ab(s) = (bx - ax)(sy - ay) - (by - ay)(sx - ax) is > 0, or = 0 on a
 * top (dy = 0, dx > 0) or left (dy < 0) edge, and paints c = (c (32 - k) + 128 k + 16) >> 5.  White, then the ground, then the layers in ascending
 * order.  colours (n_layers) int32 r | g << 8 | b << 16 per layer (entry 0, the ground's, is not read); a record whose layer is outside [1, n_layers)
 * is skipped.  workspace: syn_plot_workspace_bytes(n_frames, n_slots) = 32 n_frames n_slots + 96 n_frames bytes (-1 for counts below 1), 16-byte
 * aligned, as is the segment table. */
int64_t syn_plot_workspace_bytes(int64_t n_frames, int32_t n_slots);
int syn_plot_setup(const float* data, int64_t n_frames, int32_t n_joints, const float* trajec, int64_t n_take, const int32_t* index, const float* bounds,
                   const int32_t* segments, int32_t n_segments, const double* camera, int32_t size, int32_t traj_half_width, int32_t n_slots,
                   void* workspace, void* stream);
int syn_plot_draw(const void* workspace, int64_t n_frames, int32_t n_slots, const int32_t* colours, int32_t n_layers, int32_t size, uint8_t* rgb,
                  void* stream);

/* The audio front end: amplitude envelope and onset detection of 16 kHz waveforms (additive, SYN_ABI_VERSION stays 9; csrc/syn_audio.inc) -
 * what dataloaders/beat_sep_lower.py:391-409 and utils/metric.py:64-76 take from numpy stride tricks and librosa.onset.onset_detect.  Several takes of
 * different lengths share a call: y [total samples] fp32 is the takes back to back, sample_off and frame_off [n_takes + 1] int64 ON THE DEVICE are
 * their first sample and first frame (take i: n_i samples, T_i = 1 + n_i / hop frames); max_samples / max_frames = the longest take's, total_frames =
 * frame_off[n_takes].  Every call enqueues on `stream`, allocates nothing, uses no atomics; all arithmetic behind the samples is fp64 in a fixed order,
 * and a take's result is bitwise the same whichever takes share the call.
 *
 * syn_audio_amplitude: out [total samples] fp32, per take a[i] = max |y[i .. i + frame_length)| for i <= n - frame_length, the last frame_length - 1
 *   entries repeat a[n - frame_length]; frame_length 1 .. 4096; a take shorter than frame_length is left unwritten.
 * syn_audio_power_spectrum: power [total_frames][1025] fp64 = |DFT_2048 of the Hann-windowed (periodic) frame ypad[t hop .. t hop + 2048)|^2, ypad = y
 *   between 1024 zeros; hop 1 .. 2048.  A GEMM against the [cos | -sin] basis on v_mfma_f64_16x16x4_f64, angles reduced as integers (jk mod 2048).
 * syn_audio_mel_db: mel_db [total_frames][128] fp64 = max(S, max over the take of S - 80), S = 10 log10(max(1e-10, Slaney mel filterbank (128 bands,
 *   0 .. sr / 2) . power)); workspace: syn_audio_workspace_bytes(total_frames) bytes (-1 for a count below 1), 8-byte aligned - it holds `power`.
 * syn_audio_onset_env: env [total_frames] fp64, env[t] = 0 for t < lag, else the mean over the bands (summed in ascending band order) of
 *   max(0, mel_db[t - lag + 1] - mel_db[t - lag]), lag = 1 + 2048 / (2 hop) (the difference's lag plus librosa's centring shift; 3 at hop 512); env_norm = (env - min) / ((max - min) + FLT_MIN), min and max over the take.
 * syn_audio_peak_pick: mask [total_frames] uint8, count [n_takes] int32.  Frame i of a take is an onset iff x[i] is the maximum of
 *   x[max(0, i - pre_max) .. min(T, i + post_max)), x[i] >= delta + the mean of x[max(0, i - pre_avg) .. min(T, i + post_avg)) (summed in ascending
 *   order, divided by the truncated window's length), and the previous onset is more than `wait` frames back (frames taken in order).  env_raw (may be
 *   NULL): a take whose env_raw is zero everywhere has no onsets. */
int64_t syn_audio_workspace_bytes(int64_t total_frames);
int syn_audio_amplitude(const float* y, const int64_t* sample_off, int32_t n_takes, int64_t max_samples, int32_t frame_length, float* out, void* stream);
int syn_audio_power_spectrum(const float* y, const int64_t* sample_off, const int64_t* frame_off, int32_t n_takes, int64_t max_frames, int64_t total_frames,
                             int32_t hop, double* power, void* stream);
int syn_audio_mel_db(const float* y, const int64_t* sample_off, const int64_t* frame_off, int32_t n_takes, int64_t max_frames, int64_t total_frames, double sr,
                     int32_t hop, void* workspace, double* mel_db, void* stream);
int syn_audio_onset_env(const double* mel_db, const int64_t* frame_off, int32_t n_takes, int64_t max_frames, int32_t hop, double* env, double* env_norm,
                        void* stream);
int syn_audio_peak_pick(const double* x, const double* env_raw, const int64_t* frame_off, int32_t n_takes, int32_t pre_max, int32_t post_max, int32_t pre_avg,
                        int32_t post_avg, int32_t wait, double delta, uint8_t* mask, int32_t* count, void* stream);

/* Audio resampling (additive, SYN_ABI_VERSION stays 9; csrc/syn_audio_resample.inc): a waveform from any integer rate to any other, what
 * the reference takes from librosa.load + librosa.resample (dataloaders/beat_sep_lower.py:392-393, diffusion_rvqvae_trainer.py:679-680).  Band-limited
 * interpolation with a Kaiser-windowed sinc on the exact rational grid: with up / down = target rate / source rate in lowest terms (a common factor is
 * refused) a take of n samples becomes ceil(n up / down) samples,
 *   out[m] = sum_j y[j] h[m down - j up],  y zero outside the take,  h[k] = 0 for |k| > K,
 * each sum one fp64 fma chain over ASCENDING j from 0.0; out64 receives the sum, out32 the sum rounded once to fp32.  Either may be NULL, not both.
 *
 * Takes as above: y [total samples] fp32 back to back, sample_off and out_off [n_takes + 1] int64 ON THE DEVICE, the first sample of take i in y and
 * its first output in out32 / out64 (out_off[n_takes] is not read); max_samples = the longest take's samples (it sizes the grid; 1 .. 2^46 / up).
 * taps [n_taps] fp64 on the device, 16-byte aligned, is h in PAIRS, tap-major over the outputs' residues: with W = K / up (integer division) and
 * T = 2 W + 2, n_taps = T up and
 *   taps[((t / 2) up + r) 2 + t % 2] = h[p + (W - t) up] for t = 0 .. T - 1, r = 0 .. up - 1, p = (r down) mod up, zero where |p + (W - t) up| > K,
 * so that output m, m down = j0 up + p, reads column r = m mod up downwards against y[j0 - W + t], two taps a step, and the threads of consecutive
 * outputs read consecutive pairs (syntalker_amd.audio.pack_taps makes it from the natural-order table).  A table size that is not a whole number of
 * pair rows, n_taps = 2 up (W + 1), is refused.
 *
 * The call enqueues on `stream`, allocates nothing and uses no atomics.  It writes exactly ceil(n_i up / down) values per take from out_off[i] on and
 * nothing else; a take's bits do not depend on what shares the call; every index that grows with the take is 64-bit (m down passes 2^31 within
 * seconds of audio).  Refused before any launch, non-zero with syn_last_error naming the function: a null pointer (y, the offsets, taps, or both
 * outputs), n_takes outside 1 .. 65535, up or down < 1, gcd(up, down) != 1, a negative or ill-shaped n_taps, a misaligned taps or out64. */
int syn_audio_resample(const float* y, const int64_t* sample_off, const int64_t* out_off, int32_t n_takes, int64_t max_samples, int32_t up, int32_t down,
                       const double* taps, int64_t n_taps, float* out32, double* out64, void* stream);

/* Baseline JPEG of device frames (additive, SYN_ABI_VERSION stays 9; csrc/syn_jpeg.inc): what the reference's utils/media.py hands to
 * ffmpeg frame by frame is encoded where syn_render_shade left it, so that a picture crosses to the host as a file of a fiftieth of its size.  Every
 * call enqueues on `stream`, allocates nothing and uses no atomics.  Nothing is floating point: a frame's bytes are those of the numpy restatement
 * (tests/jpeg_ref.py) and do not depend on its batch mates, on how a take is cut into calls, or on the launch geometry.
 *
 * Input    rgb: n_frames pictures of (height, width, 3) bytes, R G B, rows top down, densely packed, frame_stride bytes apart (>= 3 width height);
 *          width, height 1 .. 8192.
 * Padding  to multiples of 16 (W16, H16) by repeating the last column and row.
 * Colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *          Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *          Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16            (arithmetic shifts)
 * Chroma   4:2:0: (a + b + c + d + 2) >> 2 over each 2 x 2.        Level shift: s = p - 128.
 * DCT      M[u][x] = rint(8192 * 1/2 * c(u) * cos((2x + 1) u pi / 16)), c(0) = 1/sqrt 2, else 1: 64 integer constants in the source.
 *          T = (S M^T + 1024) >> 11 (arithmetic), F = M T: the DCT scaled by 2^15.  All of it is int32: a row of M sums to at most 23168 in absolute
 *          value (row 0), so |S M^T| <= 128 * 23168 < 3.0e6, |T| <= 1448, |F| <= 1448 * 23168 < 3.4e7, and |F| + (Q << 14) < 3.8e7.
 * Quantise q = sign(F) * ((|F| + (Q << 14)) / (Q << 15)), an integer division; |q| <= 1024.
 * Tables   Q = clamp((base * s + 50) / 100, 1, 255), base = the luminance / chrominance table of ITU T.81 Annex K.1, s = 5000 / quality below
 *          quality 50, else 200 - 2 quality (the IJG rule); quality 1 .. 100.
 * Entropy  baseline sequential, the four Huffman tables of Annex K.3, one interleaved scan, MCU = Y00 Y01 Y10 Y11 Cb Cr, zigzag order.  The restart
 *          interval is one MCU row (DRI = W16 / 16): the DC prediction starts from 0 in every interval, the interval's last byte is filled with
 *          1-bits, 0xFF is followed by 0x00 inside entropy data, intervals are joined by RST(row & 7).  That makes the rows independent work.
 * File     SOI, JFIF APP0, two DQT, SOF0 (8 bit, height, width, components 0x22 / 0x11 / 0x11), four DHT, DRI, SOS, data, EOI.  Everything in
 *          front of the data is constant per width, height and quality; the caller passes it (syntalker_amd/video.py jpeg_header).
 *
 * Capacity: count first, write second.  No stage writes by a guessed size.  syn_jpeg_measure runs the entropy coder without storing a byte and
 * leaves every interval's exact size; syn_jpeg_write runs the same code again and stores each interval at the place the sizes give it.  A `data` of
 * fewer than offsets[n_frames] bytes is left untouched, every store of an interval is held below its counted size, and an interval whose place
 * does not lie inside data[0 .. capacity) is skipped: whatever the workspace holds, syn_jpeg_write stores nowhere else.  Inside the coder a block
 * has a fixed region of 53 words, above the proven bound: a block codes to at most 20 + 63 * 26 = 1658 bits = 52 words before stuffing (the coder
 * clamps a DC difference to +-2047 and an AC coefficient to +-1023, which the transform never exceeds, so the bound holds for any input).
 *
 * workspace: syn_jpeg_workspace_bytes(n_frames, width, height) bytes (-1 for a count below 1 or a size out of range), 16-byte aligned: the quantised
 * coefficients (int16, 768 bytes per MCU, scan order), the interval sizes and their places.  The three calls of a batch share it, in this order:
 * syn_jpeg_transform  rgb -> the coefficients.
 * syn_jpeg_measure    -> offsets (n_frames + 1) int64 on the device: frame k will occupy data[offsets[k] .. offsets[k + 1]), a complete file with
 *                     header_bytes of header in front.
 * syn_jpeg_write      -> data (capacity >= offsets[n_frames] bytes, which the caller has read back): header (header_bytes on the device), intervals,
 *                     RST markers and EOI of every frame.  offsets as syn_jpeg_measure left them. */
int64_t syn_jpeg_workspace_bytes(int64_t n_frames, int32_t width, int32_t height);
int syn_jpeg_transform(const uint8_t* rgb, int64_t frame_stride, int64_t n_frames, int32_t width, int32_t height, int32_t quality, void* workspace,
                       void* stream);
int syn_jpeg_measure(int64_t n_frames, int32_t width, int32_t height, int32_t header_bytes, void* workspace, int64_t* offsets, void* stream);
int syn_jpeg_write(int64_t n_frames, int32_t width, int32_t height, const uint8_t* header, int32_t header_bytes, const void* workspace,
                   const int64_t* offsets, uint8_t* data, int64_t capacity, void* stream);

/* n_steps consecutive steps of a hook-free stretch of p_sample_loop / ddim_sample_loop (gaussian_diffusion.py:714-739,
 * 905-931), in place (x_next = x_t): step j takes its timesteps from t_model + j * t_model_stride and
 * t_coef + j * t_coef_stride (the rows syn_steps_advance fills), its noise from rng (noise must be NULL when n_steps > 1).
 * Fragment-order latents: ONE persistent launch per CU-filling slice of the batch - every workgroup carries its four sequences through all the steps, so the
 * workgroups drift out of phase and the HBM traffic of the input / output stages of some overlaps the matrix work of the
 * others.  Token-major latents: the launches of syn_denoise_step, n_steps times. */
int syn_denoise_steps(const syn_model* model, const syn_step* step, int32_t n_steps, int32_t t_model_stride,
                      int32_t t_coef_stride, void* stream);

/* Same step, eagerly, with a hipEvent after every launch: fills ms_out[8] / count_out[8] with the elapsed
 * milliseconds and launch count per stage class {0 input GEMM, 1 qkv GEMM, 2 attention, 3 proj GEMM,
 * 4 fc1 GEMM, 5 fc2 GEMM, 6 guidance combine, 7 output GEMM}.  Synchronises `stream`; not graph-capturable. */
int syn_denoise_step_profile(const syn_model* model, const syn_step* step, void* stream, float* ms_out, int32_t* count_out);

/* Training-mode forward of one Conv1d(k = 15) of the WavEncoder (models/utils/layer.py:144-184 conv1 / conv2 / downsample[0],
 * called from models/denoiser.py:304-322 with BatchNorm on batch statistics, so nothing is folded): x fp32 channels-last
 * [n_clips][l_in][cin] (what PyTorch calls an (N, C, 1, L) channels_last tensor), y fp32 [n_clips][l_out][cout],
 * l_out = (l_in + 2 pad - 15) / stride + 1.  w_hi / w_lo: syn_pack_weight of the hi / lo bf16 halves of the GEMM matrix
 * W'[cout][tap][cin] (taps zero-padded to a multiple of the stride); products are hi.hi + lo.hi + hi.lo on the bf16 matrix
 * pipe, i.e. fp32-grade.  bias may be NULL.  Supported (cin, stride, cout): the encoder's own, see the error text. */
/* Weight gradient of a stride-1, padding-7 Conv1d(k = 15) of the encoder (cout 64 / 128 / 256; cin a multiple of 16; the
 * encoder's unpadded strided layers too - (cin, stride, cout) = (64, 6, 64), (64, 6, 128), (128, 3, 256), read as stride-1 convolutions
 * over rows of stride x cin = 384 channels): dw [cout][cin][15] = sum over clips and output
 * positions of dy[l][co] x[l stride + t - pad][ci], x fp32 channels-last [n_clips][l_in][cin], dy [n_clips][l_out][cout].
 * Split operands like the forward (fp32-grade); workgroup partial sums go through ws -
 * syn_conv1d_wgrad_shares(n_clips, l_out, stride * cin, cout) * cout * ceil(15 / stride) * stride * cin floats - and are added in a
 * fixed order (no atomics).  (ABI 9: cout - a workgroup owns a slice of the gradient (output-channel tile x input-channel block) and a share of the
 * positions; the more slices a layer is cut in, the fewer shares fill the chip, and every share is a full-size partial gradient through HBM.) */
int32_t syn_conv1d_wgrad_shares(int32_t n_clips, int32_t l_out, int32_t cin_rows, int32_t cout);
int syn_conv1d_train_wgrad(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                           int32_t cout, float* ws, float* dw, void* stream);

/* The encoder's first layer in training mode - Conv1d(cin = 1 | 2 -> 64, k 15, stride, padding) of block 0's conv1 and of its
 * shortcut (models/denoiser.py:308, models/utils/layer.py:150,158; stride 5, padding 1700 there) - without the bias (see
 * syn_bn_act_fwd): exact fp32 - the forward on fp32 FMAs, the weight gradient on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, a persistent stream over the batch).  x fp32 [n_clips][l_in][cin] (the waveform as the reference passes it), w the module's weight
 * [64][cin][15], y / dy fp32 channels-last [n_clips][l_out][64], l_out = (l_in + 2 pad - 15) / stride + 1.  The weight gradient
 * needs ws of syn_conv1d_first_parts(n_clips, l_out) * 64 * cin * 15 floats (workgroup partial sums, added in a fixed order) and
 * writes dw [64][cin][15].  There is no data gradient: the waveform is an input. */
int32_t syn_conv1d_first_parts(int32_t n_clips, int32_t l_out);
int syn_conv1d_first_fwd(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const float* w, float* y,
                         void* stream);
int syn_conv1d_first_wgrad(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws,
                           float* dw, void* stream);
/* (ABI 7) the forward with the BatchNorm statistics of its output from the same launch: bn_part (NULL, or syn_conv1d_first_tiles(n_clips, l_out) x 2 x 64
 * floats) = per-workgroup sum and sum of squares of every output channel, what syn_bn_finalize takes (chunks = that tile count). */
int32_t syn_conv1d_first_tiles(int32_t n_clips, int32_t l_out);
/* (ABI 7) block 0's conv1 and its shortcut convolution (same input, kernel, stride, padding: models/utils/layer.py:150,158) as ONE launch over the waveform
 * window: y_a / y_b and their statistics (both NULL or both given, syn_conv1d_first_tiles(...) x 2 x 64 floats each). */
int syn_conv1d_first_fwd2(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const float* w_a, const float* w_b,
                          float* y_a, float* y_b, float* bn_part_a, float* bn_part_b, void* stream);
/* (ABI 7) the first layer's weight gradient with the backward of the BatchNorm + LeakyReLU behind it folded in: dz = the gradient at the activation's output,
 * y = the convolution's raw output, stats / affine from syn_bn_finalize, dgamma_dbeta from syn_bn_bwd_stats (below); dy = scale (dp - dbeta / M - xhat dgamma / M),
 * dp = dz act'(a(y)), is formed as the values are loaded and never written.  stride 5 (the encoder's). */
int syn_conv1d_first_wgrad_bn(const float* x, const float* dz, const float* y, const float* stats, const float* affine, const float* dgamma_dbeta,
                              int32_t act, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dw, void* stream);
/* (ABI 9) Block 0's conv1: its weight gradient AND bn1's backward sums from ONE pass over (dz, y) - the BatchNorm backward is linear in dgamma / dbeta and only a
 * reduction consumes dy here (the waveform takes no gradient): dW = scale (S1 - dbeta / M S2 - dgamma / M S3) with S1 = sum dp win, S2 = sum win, S3 = sum xhat win
 * accumulated side by side.  Replaces syn_bn_bwd_stats + syn_conv1d_first_wgrad_bn (a second read of both tensors).  dw [64][cin][15] and dgamma_dbeta [3][64] are
 * written by this call (no partial sums left for syn_conv1d_wgrad_sums); ws: syn_conv1d_first_parts(n_clips, l_out) * (2 * 64 * cin * 15 + 160) floats.  stride 5. */
int syn_conv1d_first_wgrad_bn_lin(const float* x, const float* dz, const float* y, const float* stats, const float* affine, int32_t act,
                                  int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dw, float* dgamma_dbeta, void* stream);
/* (ABI 9) Block 0's SHORTCUT convolution: its weight-gradient partial sums (ws as syn_conv1d_first_wgrad) with the block tail's backward folded into the loads -
 * dout = the gradient at the block's output, y2 / y_short the raw outputs of conv2 and of the shortcut convolution with the statistics, affines and
 * [dgamma | dbeta | 0] of their BatchNorms (syn_bn_block_bwd with dy = NULL leaves exactly those).  d = dout act'(a2(y2) + a_s(y_short)); the shortcut's
 * dy_s = its BatchNorm's backward of d feeds the matrix pipe and is never written; dy2 = bn2's backward of d IS written ([n_clips][l_out][64]: conv2's data
 * and weight gradients read it).  Against syn_bn_block_bwd's apply pass + syn_conv1d_first_wgrad: one write and one read of a 117 MB tensor less.  stride 5. */
int syn_conv1d_first_wgrad_tail(const float* x, const float* dout, const float* y2, const float* y_short, const float* stats2, const float* affine2,
                                const float* short_stats, const float* short_affine, const float* dgb2, const float* short_dgb, int32_t act,
                                int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, float* ws, float* dy2, void* stream);
/* (ABI 7) the statistics half of syn_bn_act_bwd: dgamma_dbeta [3][channels] only (ws as there). */
int syn_bn_bwd_stats(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta, int64_t rows,
                     int32_t channels, int32_t act, float* ws, float* dgamma_dbeta, void* stream);
int syn_conv1d_first_fwd_stats(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, const float* w, float* y,
                               float* bn_part, void* stream);

/* The two fragment sets syn_conv1d_train_fwd takes, from the module's weight w [cout][cin][15] (fp32) in one launch; each
 * output holds syn_conv1d_pack_bytes(...) bytes.  transposed = 1: the matrix of the DATA GRADIENT (stride 1; for a strided
 * convolution the form syn_conv1d_train_dgrad_sum takes: a stride-1 convolution over dy whose output rows are `stride` consecutive positions x cin channels)
 * of that convolution (taps reversed, channel roles swapped: N = cin, C = cout) - the gradient then is
 * syn_conv1d_train_fwd(dy, ..., cin = cout, stride 1, pad 7, ..., cout = cin). */
int syn_conv1d_pack_split(const float* w, int32_t cout, int32_t cin, int32_t stride, int32_t transposed, void* out_hi, void* out_lo,
                          void* stream);
/* (ABI 5) Up to SYN_CONV_PACK_MAX syn_conv1d_pack_split calls as ONE launch (requests: a host array, read at call time): the training step packs every
 * fragment set its convolutions take - forward and data-gradient forms - once per step, the weights only change in optimizer.step(). */
#define SYN_CONV_PACK_MAX 40
typedef struct syn_conv_pack_req { const float* w; void* out_hi; void* out_lo; int32_t cout, cin, stride, transposed; } syn_conv_pack_req;
int syn_conv1d_pack_split_many(const syn_conv_pack_req* reqs, int32_t n_reqs, void* stream);
/* Bytes of each of syn_conv1d_pack_split's two outputs. */
int64_t syn_conv1d_pack_bytes(int32_t cout, int32_t cin, int32_t stride, int32_t transposed);
/* (ABI 8) syn_conv1d_train_wgrad / _wgrad_norm / syn_conv1d_first_wgrad / _wgrad_bn with dw = NULL leave their per-share partial sums in ws; this
 * adds up to SYN_WGRAD_SUM_MAX such gradients up in ONE launch (the three convolutions of a BasicBlock), each in the order its own launch would have used.
 * A job: part = that call's ws, dw = the module-layout gradient [cout][cin][15], the call's n_clips / cin / stride / cout and ITS l_out;
 * first_layer != 0: the job is a syn_conv1d_first_wgrad* call (cin 1 | 2, cout 64). */
#define SYN_WGRAD_SUM_MAX 4
typedef struct syn_wgrad_sum_job { const float* part; float* dw; int32_t n_clips, l_out, cin, stride, cout, first_layer;
                                   int32_t share_pitch;   /* (ABI 9) floats between consecutive shares of `part`; 0 = the gradient's own size (a share that holds two
                                                           * gradients - syn_conv1d_train_wgrad_pair - has twice that, and the second job's `part` starts one gradient in) */
                                   int32_t reserved; } syn_wgrad_sum_job;
int syn_conv1d_wgrad_sums(const syn_wgrad_sum_job* jobs, int32_t n_jobs, void* stream);
/* (ABI 7) The data gradient that reaches a BasicBlock's input, written once: dx [n_clips][l_in][cin] = conv^T dy [+ conv2^T dy2] [+ residual].
 * Strided, unpadded layers (a down-sampling block: conv1 and the shortcut convolution share input and geometry): dy / dy2 [n_clips][l_out][cout] with their
 * transposed fragment sets, both accumulated in one launch instead of two tensors and an add; residual must be NULL.  Stride 1, padding 7 (a block with an
 * identity shortcut): dy2 NULL, residual (laid out like dx; the gradient arriving along the shortcut) added in the epilogue. */
int syn_conv1d_train_dgrad_sum(const float* dy, const void* w_hi, const void* w_lo, const float* dy2, const void* w2_hi, const void* w2_lo,
                               const float* residual, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, int32_t cout, float* dx,
                               void* stream);
int syn_conv1d_train_fwd(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                         const void* w_hi, const void* w_lo, const float* bias, int32_t cout, float* y, float* bn_part, void* stream);
/* bn_part (NULL, or syn_conv1d_train_fwd_tiles(...) x 2 x cout floats; bias must then be NULL): per-workgroup sum and sum of squares
 * of every output channel, straight from the accumulators - the BatchNorm that follows takes them as syn_bn_act_fwd's ws with
 * ws_chunks = that tile count and skips its own pass over y. */
int32_t syn_conv1d_train_fwd_tiles(int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, int32_t cout);
/* (ABI 7) the stride-1 layers with the BatchNorm (+ LeakyReLU) of the convolution in front applied to the input as it is staged - x is that
 * convolution's raw output, the kernel reads act(x * in_affine[0][c] + in_affine[1][c]) (in_affine [2][cin] from syn_bn_finalize; in_act != 0:
 * LeakyReLU(0.01)), zero outside the clip; no bias.  The weight gradient with the same view of x. */
/* (ABI 8) conv1 and the shortcut convolution of a down-sampling BasicBlock (models/utils/layer.py:150-158: the same input, stride, padding and
 * width) as ONE launch: the input tile is staged (and split into its bf16 halves) once for both weight sets.  The encoder's strided layers only
 * (64x6->64, 64x6->128, 128x3->256); y_a / y_b and the statistics as syn_conv1d_train_fwd's. */
int syn_conv1d_train_fwd_pair(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad, int32_t cout,
                              const void* wa_hi, const void* wa_lo, float* y_a, float* bn_part_a,
                              const void* wb_hi, const void* wb_lo, float* y_b, float* bn_part_b, void* stream);
int syn_conv1d_train_fwd_norm(const float* x, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                              const void* w_hi, const void* w_lo, int32_t cout, const float* in_affine, int32_t in_act, float* y, float* bn_part,
                              void* stream);
int syn_conv1d_train_wgrad_norm(const float* x, const float* dy, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                                int32_t cout, const float* in_affine, int32_t in_act, float* ws, float* dw, void* stream);
/* (ABI 9) conv1 and the shortcut convolution of a down-sampling block - same input, stride, padding and width - leave BOTH weight gradients' partial sums from one
 * launch that stages the input once: ws [shares][2 cout][taps][stride cin] with shares = syn_conv1d_wgrad_shares(n_clips, l_out, stride cin, cout); rows 0 .. cout - 1 of
 * a share are dy_a's gradient, the rest dy_b's (two syn_wgrad_sum_job with share_pitch = 2 cout taps stride cin, the second's part one gradient in).
 * (cin, stride, pad, cout) = (64, 6, 0, 64): block 1, whose input is the encoder's largest tensor. */
int syn_conv1d_train_wgrad_pair(const float* x, const float* dy_a, const float* dy_b, int32_t n_clips, int32_t l_in, int32_t cin, int32_t stride, int32_t pad,
                                int32_t cout, float* ws, void* stream);

/* Every bf16 fragment set the training step's Linear layers need, from the fp32 master weights in ONE launch (the weights change
 * once per step, in optimizer.step()): job j packs src (n x k row-major, transposed = 0: as syn_pack_weight; k x n row-major,
 * transposed = 1: as syn_pack_weight_t) into out.  jobs_dev: device array; max_fragments = max over the jobs of n / 16 * k / 32. */
/* (ABI 8) src_dim > 0: the source's real extent along a zero-PADDED dimension - k of a row-major [n][src_dim] source (transposed = 0), n of a
 * row-major [k][src_dim] source (transposed = 1): text_encoder_body's 300 input features as 384 columns. */
typedef struct syn_pack_job { const float* src; void* out; int32_t n, k, transposed, src_dim; } syn_pack_job;
int syn_pack_weights(const syn_pack_job* jobs_dev, int32_t n_jobs, int64_t max_fragments, void* stream);

/* ---- training path: fp32 forward / backward of the non-GEMM pieces of a transformer block ----
 * LayerNorm(512, eps 1e-5) of `rows` rows (models/timm_transformer/transformer.py:160,162,183,193); the backward
 * needs scratch of ceil(rows/16)*1024 floats and writes dgamma[512], dbeta[512] (deterministic two-stage sums); `add` (NULL or
 * [rows][512]) is added to dx: the gradient that reaches x along the block's residual connection (transformer.py:195-198). */
/* (ABI 5) y fp32 and / or y_bf16 [rows][512] (either may be NULL): the Linear that follows takes bf16 operands, and nothing else
 * reads a pre-LN block's normalised rows - the training step asks for the bf16 copy only. */
int syn_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, void* y_bf16, float* mean, float* rstd, int32_t rows,
               void* stream);
int syn_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* add, float* dx,
               float* dgamma, float* dbeta, float* scratch, int32_t rows, void* stream);
/* nn.GELU() (exact erf form, transformer.py:117-151), n % 4 == 0 elements. */
/* (ABI 5) y fp32 and / or y_bf16 (either may be NULL), as syn_ln_fwd. */
int syn_gelu_fwd(const float* x, float* y, void* y_bf16, int64_t n, void* stream);
int syn_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* (ABI 6) Rotary position embedding on the hidden state (models/denoiser.py:178-186, 324-343: SinusoidalEmbeddings + apply_rotary_pos_emb on the
 * (B x 8, 32, 64) view): x, y fp32 [n_seq][32][512] (may alias), a token's features = 8 groups of 64, (u, v) = (first, last 32 of a group) ->
 * (u cos - v sin, v cos + u sin); cos_t / sin_t fp32 [32 positions][32] = cos / sin(position x inv_freq[j]).  inverse != 0: the transposed
 * rotation, i.e. the gradient with respect to x. */
int syn_rotary(const float* x, const float* cos_t, const float* sin_t, int32_t n_seq, int32_t inverse, float* y, void* stream);
/* (ABI 6) Weight / bias gradient of an nn.Linear whose input has few rows (the timestep MLP and embed_text see one row per clip, models/denoiser.py:92,
 * 231-245): dw fp32 [n][k] = sum_m dy[m][n] x[m][k], db [n] = sum_m dy[m][n] (NULL to skip); dy fp32 [m_rows][n], x bf16 [m_rows][k] (the operand
 * the forward GEMM took), m_rows <= 64, n % 16 == 0.  fp32 FMAs in row order. */
int syn_linear_wgrad_rows(const float* dy, const void* x_bf16, int32_t m_rows, int32_t n, int32_t k, float* dw, float* db, void* stream);
/* (ABI 8) masked_l2 of training_losses (gaussian_diffusion.py:202-215, 1307-1314: SmoothL1(beta 1) x mask, summed, / (sum(mask) x C)).
 * target fp32 (B, C, 1, T) as the reference lays it out; out either the same (out_rows = 0) or the output Linear's own rows [B][T][C] (out_rows = 1:
 * what models/denoiser.py:294-300's reshape / permute is a view of); mask bytes [batch][t_len]; part: [batch][channels / 64] floats of scratch;
 * loss [batch].  channels % 64 == 0, t_len <= 64.  Two launches (tile sums, then their sum in tile order).
 * poison_flag (NULL or one device int): while it is nonzero every loss is NaN - pass syn_train_stack.sync + 256, the persistent block kernels' sticky
 * barrier-timeout flag (see syn_train_stack_fwd), so that a step computed from partial sums that never arrived cannot pass for a step. */
int syn_masked_smooth_l1(const float* target, const float* out, const uint8_t* mask, int32_t batch, int32_t channels, int32_t t_len, int32_t out_rows,
                         float* part, const int32_t* poison_flag, float* loss, void* stream);
/* Its gradient: dout (laid out like out) = sample_scale[b] (NULL: 1) x d loss[b] / d out - one pass in the backward, the incoming gradient of
 * loss[b] folded in. */
int syn_masked_smooth_l1_grad(const float* target, const float* out, const uint8_t* mask, int32_t batch, int32_t channels, int32_t t_len, int32_t out_rows,
                              const float* sample_scale, float* dout, void* stream);
/* (ABI 8) bf16 GEMM operand [m_rows][out_ld] = up to SYN_CONCAT_MAX fp32 sources side by side, columns beyond them zero (torch.cat along the feature
 * axis + the operand rounding + the zero padding to the GEMM's 128-column granularity, models/denoiser.py:155-174, denoiser_h3d.py:187-200).  Source i:
 * `width` columns of rows of pitch ld; operand row r reads source row r / row_div (a per-clip vector repeated over the clip's frames), p2 (NULL or
 * like p) added first; or pool > 1: the mean of source rows r * pool .. + pool - 1 (F.avg_pool1d over the frame axis, denoiser.py:157).
 * width % 4 == 0, ld % 4 == 0. */
#define SYN_CONCAT_MAX 4
typedef struct syn_concat_src { const float* p; const float* p2; int32_t width, ld, row_div, pool; } syn_concat_src;
int syn_rows_concat_bf16(const syn_concat_src* srcs, int32_t n_src, int32_t m_rows, int32_t out_ld, void* out_bf16, void* stream);
/* (ABI 8) nn.Embedding lookup (models/denoiser.py:72,152) written as the next Linear's operand: out bf16 [m_rows][out_ld], columns dim .. out_ld zero. */
int syn_embed_rows_bf16(const int64_t* ids, const float* table, int32_t vocab, int32_t dim, int32_t m_rows, int32_t out_ld, void* out_bf16, void* stream);
/* (ABI 8) (B, C, 1, T) fp32 -> bf16 rows [B * T][C]: the permute of models/denoiser.py:160 + the operand rounding; channels % 64 == 0, t_len == 32. */
int syn_bct_to_rows_bf16(const float* x_bct, int32_t n_clips, int32_t channels, int32_t t_len, void* out_bf16, void* stream);
/* (ABI 8) out [n_groups][width] = sums over the `group` consecutive rows (pitch ld) of each group, in row order: the gradient of a vector the forward
 * repeated over a clip's frames. */
int syn_rows_group_sum(const float* src, int32_t ld, int32_t width, int32_t group, int32_t n_groups, float* out, void* stream);
/* (ABI 8) out fp32 [m_rows][width] = scale x src[r / row_div][0:width] (src rows of pitch ld): the backward of an average pool over row_div rows. */
int syn_rows_expand(const float* src, int32_t ld, int32_t width, int32_t row_div, float scale, int32_t m_rows, float* out, void* stream);
/* (ABI 8) out [n] = sum over i < rows of part [i][n], in order: a Linear's bias gradient from syn_linear_bwd_prep's colsum_part when no syn_linear_pair
 * launch carries it (a Linear whose input takes no gradient). */
int syn_colsum_parts(const float* part, int32_t rows, int32_t n, float* out, void* stream);
/* (ABI 8) One read pass over a buffer (a dword per 64-byte line): pulls it back into the memory-side cache ahead of a latency-bound consumer. */
int syn_touch(const void* p, int64_t bytes, void* stream);
/* nn.BatchNorm1d in training mode (batch statistics, running statistics updated as PyTorch does) [+ shortcut] [+ LeakyReLU(0.01)]
 * of the audio encoder's BasicBlock (models/utils/layer.py:171-184) on channels-last fp32 [rows][channels], rows = clips x
 * positions: z = act(gamma (y - mean) rstd + beta [+ shortcut]).  ws: 2 * syn_bn_chunks(rows) * channels floats; stats
 * [2][channels] receives mean / rstd for the backward; run_mean / run_var may be NULL; conv_bias (or NULL): the bias of the
 * convolution that produced y, NOT added to y by the caller - under batch statistics it only shifts the running mean.  Backward: dgamma_dbeta [3][channels]
 * (ABI 5: the third row is written with zeros - the gradient of conv_bias, which the mean subtraction cancels), dy, and dshortcut (NULL when there is none) from dz, the saved z and y.  z may be NULL when there was no shortcut (beta then
 * required): the activation's sign is recomputed from y, which the passes read anyway. */
int32_t syn_bn_chunks(int64_t rows);
int syn_bn_act_fwd(const float* y, const float* shortcut, int64_t rows, int32_t channels, const float* gamma, const float* beta, float eps,
                   float momentum, float* run_mean, float* run_var, const float* conv_bias, int32_t act, float* ws, int32_t ws_chunks, float* stats,
                   float* z, void* stream);
int syn_bn_act_bwd(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta, int64_t rows,
                   int32_t channels, int32_t act, float* ws, float* dgamma_dbeta, float* dy, float* dshortcut, void* stream);
/* The same with the statistics reduced over several ranks - nn.SyncBatchNorm, which the reference's DDP branch converts every BatchNorm to
 * (train.py:90; torch/nn/modules/_functions.py SyncBatchNorm).  The library reduces to per-channel sums in fp64 ([2][channels]: forward
 * sum y, sum y^2; backward sum d, sum d * xhat), the CALLER all-reduces them over its process group (RCCL) together with the row count, and the
 * second call finalises with the global numbers: normalisation and the data gradient use the global sums, dgamma / dbeta stay this rank's own
 * (DDP averages parameter gradients), the running statistics move towards the GLOBAL batch statistics.  scratch: 2 * channels floats. */
int syn_bn_sums(const float* y, int64_t rows, int32_t channels, float* ws, int32_t ws_chunks, double* sums, void* stream);
int syn_bn_act_apply(const float* y, const float* shortcut, int64_t rows, int64_t rows_total, int32_t channels, const float* gamma, const float* beta,
                     float eps, float momentum, float* run_mean, float* run_var, const float* conv_bias, int32_t act, const double* sums_total,
                     float* stats, float* z, void* stream);
int syn_bn_bwd_sums(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta, int64_t rows,
                    int32_t channels, int32_t act, float* ws, double* sums, void* stream);
int syn_bn_act_bwd_apply(const float* dz, const float* z, const float* y, const float* stats, const float* gamma, const float* beta,
                         const double* sums_local, const double* sums_total, int64_t rows, int64_t rows_total, int32_t channels, int32_t act,
                         float* dgamma_dbeta, float* scratch, float* dy, float* dshortcut, void* stream);

/* (ABI 7) The same block tail with fewer passes over its tensors (models/utils/layer.py:171-184: conv1 -> bn1 -> act -> conv2 -> bn2 (+ shortcut | + bn(conv(x)))
 * -> act).  A batch-statistics BatchNorm is a per-channel affine map a(v) = v * scale + shift once its statistics exist:
 *   syn_bn_finalize   part [chunks][2][channels] (sum, sum of squares: a convolution's bn_part) -> stats [2][channels] = mean, rstd; affine [2][channels] =
 *                     scale = rstd gamma, shift = beta - mean rstd gamma; running statistics as nn.BatchNorm1d updates them (conv_bias as in syn_bn_act_fwd)
 *   syn_bn_apply2     z = act(a(y) + s), s = a_s(shortcut) when short_affine is given (the down-sampling branch's BatchNorm, applied here instead of in a
 *                     pass of its own), the raw shortcut otherwise, nothing when shortcut is NULL
 *   syn_bn_block_bwd  from dz = d loss / d z: dp = dz act'(p) with the pre-activation p RECOMPUTED from y and the shortcut (the block's output is neither
 *                     read nor needed by the backward); dgb [3][channels] = dgamma, dbeta, 0 of a; dy; with a normalised shortcut also short_dgb and
 *                     dshortcut = the data gradient of ITS BatchNorm, with a raw one dshortcut = dp.  One statistics pass and one apply pass over
 *                     (dz, y, shortcut) for both BatchNorms.  ws: 3 * syn_bn_chunks(rows) * channels floats.  (ABI 9) dy = NULL (and dshortcut NULL): the
 *                     statistics pass and [dgamma | dbeta | 0] only - the caller's next kernel forms the gradients itself (syn_conv1d_first_wgrad_tail).
 * bn1 + LeakyReLU in front of conv2 is applied by conv2 itself while it stages its input (syn_conv1d_train_fwd_norm; the weight gradient recomputes it the
 * same way, syn_conv1d_train_wgrad_norm): in_affine [2][cin] = bn1's affine, in_act != 0: LeakyReLU(0.01); positions outside the clip stay zero. */
int syn_bn_finalize(const float* part, int32_t chunks, int64_t rows, int32_t channels, const float* gamma, const float* beta, float eps, float momentum,
                    float* run_mean, float* run_var, const float* conv_bias, float* stats, float* affine, void* stream);
/* (ABI 8) Two syn_bn_finalize calls as one launch: bn1 and the shortcut's BatchNorm of a down-sampling block, whose partial sums exist together. */
typedef struct syn_bn_finalize_job { const float* part; int32_t chunks, channels; int64_t rows; const float* gamma; const float* beta; float eps, momentum;
                                     float* run_mean; float* run_var; const float* conv_bias; float* stats; float* affine; } syn_bn_finalize_job;
int syn_bn_finalize_pair(const syn_bn_finalize_job* a, const syn_bn_finalize_job* b, void* stream);
int syn_bn_apply2(const float* y, const float* affine, const float* shortcut, const float* short_affine, int64_t rows, int32_t channels, int32_t act,
                  float* z, void* stream);
int syn_bn_block_bwd(const float* dz, const float* y, const float* shortcut, const float* stats, const float* affine, const float* short_stats,
                     const float* short_affine, int64_t rows, int32_t channels, int32_t act, float* ws, float* dgb, float* short_dgb, float* dy,
                     float* dshortcut, void* stream);

/* (ABI 7) The eight transformer blocks of the TRAINING forward as one persistent launch (models/timm_transformer/transformer.py:154-198 in train() mode:
 * h + drop_path(attn(norm1(h))), then h + drop_path(mlp(norm2(h))), x 8), 1 .. 64 sequences of 32 tokens: a sequence's 32 rows are shared by 4 workgroups of
 * one XCD (head j / MLP slice j each, partial sums exchanged through that XCD's L2: the whole-step sampling kernel's tile-split mode).  Weights: the packed
 * fragment sets of syn_layer (syn_pack_weight / syn_pack_weights).  drop_path: NULL, or the factors [16][n_seq] (row 2 l: attention branch of block l, row
 * 2 l + 1: its MLP branch; 0 or 1 / keep).  Written for the backward, per block, with M = 32 n_seq rows: the two branch inputs h (fp32 [M][512]) and their LayerNorm
 * mean / rstd [M]; qkv fp32 [M][1536]; the fc1 output + bias before the GELU, fp32 [M][1024]; and the transposed bf16 operands of the four weight-gradient GEMMs as
 * packed fragments (what syn_linear_and_pack's xt_packed holds): LN1(h)^T, attention output^T, LN2(h)^T (512 x M each), GELU output^T (1024 x M).
 * sync: 320 zeroed uint32 (left zeroed); xch: n_seq x 8 x 16384 floats of scratch.
 * sync[256] is a STICKY ERROR FLAG shared by syn_train_stack_fwd and syn_train_stack_bwd: the XCD-local barrier waits of the member workgroups are
 * bounded, and a wait that runs out (another kernel holding CUs of the XCD) sets it and lets the kernel finish on whatever partial sums it found - the
 * results of that launch, and of every later one that finds the flag set (its waits give up after 256 polls), are wrong.  Nothing in the library clears it:
 * the host reads it back now and then and zeroes `sync` (syntalker_amd.training.check_stack_sync), and syn_masked_smooth_l1's poison_flag turns the step's
 * loss into NaN while it is set. */
typedef struct syn_train_block_save {
    float* h_attn; float* mean_attn; float* rstd_attn; float* qkv; void* xt_ln1; void* xt_attn;
    float* h_mlp; float* mean_mlp; float* rstd_mlp; float* pre; void* xt_ln2; void* xt_gelu;
} syn_train_block_save;
typedef struct syn_train_stack {
    const float* h_in; float* h_out;                 /* fp32 [32 n_seq][512] */
    syn_layer layer[SYN_LAYERS];
    syn_train_block_save save[SYN_LAYERS];
    const float* drop_path;
    int32_t n_seq, reserved;
    uint32_t* sync; float* xch;
} syn_train_stack;
int syn_train_stack_fwd(const syn_train_stack* a, void* stream);
/* (ABI 7) The backward of those eight blocks.  syn_train_stack_bwd: the data-gradient chain as one persistent launch (same decomposition: member = head / MLP
 * slice, two exchanges per block): dh_in [M][512] from dh_out, reading what the forward wrote (`fwd`: the forward's own struct, unchanged) and the TRANSPOSED
 * fragment sets of the weights (layer_t[l].w_* = fragments of W^T as syn_pack_weight_t / syn_pack_weights(transposed = 1) make them; ln1_g / ln2_g the gains;
 * the other members unused).  It leaves, per block: the gradients at the outputs of fc2, fc1, proj, qkv TRANSPOSED in bf16 ([512 | 1024 | 512 | 1536][M]:
 * the left operands of the weight-gradient GEMMs) and `part` [n_seq][4096], per-sequence partial sums of [dLN2 gain 512 | dLN2 shift 512 | dfc2 bias 512 |
 * dfc1 bias 1024 | dLN1 gain 512 | dLN1 shift 512 | dproj bias 512].  stash: n_seq x 4 x 16384 floats of scratch.
 * syn_train_stack_wgrad: the 32 weight-gradient GEMMs dW [n][k] = dY^T . X, four per launch (dw_* fp32, the module's layout), and the sums of `part` over the
 * sequences, each of its seven segments into its own tensor (d_*). */
typedef struct syn_train_block_grad {
    void* dyt_fc2; void* dyt_fc1; void* dyt_proj; void* dyt_qkv; float* part;
    float* dw_fc2; float* dw_fc1; float* dw_proj; float* dw_qkv;
    float* d_ln2_g; float* d_ln2_b; float* d_fc2_b; float* d_fc1_b; float* d_ln1_g; float* d_ln1_b; float* d_proj_b;    /* [512] each, d_fc1_b [1024] */
} syn_train_block_grad;
typedef struct syn_train_stack_grad {
    const syn_train_stack* fwd;
    const float* dh_out; float* dh_in;
    syn_layer layer_t[SYN_LAYERS];
    syn_train_block_grad grad[SYN_LAYERS];
    float* stash;
    int32_t first_block, last_block;          /* the blocks a call covers, SYN_LAYERS > first_block >= last_block >= 0 (the chain walks them downwards): cut in pieces,
                                               * the weight-gradient GEMMs of a finished piece can run on another stream beside the next piece of the chain */
} syn_train_stack_grad;
int syn_train_stack_bwd(const syn_train_stack_grad* a, void* stream);
int syn_train_stack_wgrad(const syn_train_stack_grad* a, void* stream);

/* (ABI 5) The optimizer step of the reference's training loop (diffusion_rvqvae_trainer.py:351-356: clip_grad_norm_(grad_norm), then Adam)
 * over lists of <= SYN_OPT_MAX fp32 tensors, pointers as kernel arguments (a captured step holds them by value):
 *   syn_opt_sqnorm    partials[b] = sum of g^2 over workgroup b's 8192-element chunk, b < syn_opt_blocks(list)        (one read of the gradients)
 *   syn_opt_scalars   *step_dev += 1; scal4 = {clip = min(1, max_norm / (sqrt(sum partials) + 1e-6)) (1 if max_norm <= 0), lr / (1 - beta1^step),
 *                     1 / sqrt(1 - beta2^step), total norm}; lr read from lr_dev when that is not NULL (a scheduler's device-resident rate)
 *   syn_opt_adam      g' = clip * g (+ weight_decay * p); m += (1 - beta1)(g' - m); v = beta2 v + (1 - beta2) g'^2;
 *                     p -= scal4[1] * m / (sqrt(v) * scal4[2] + eps)       (torch.optim.Adam, amsgrad off; the gradients are not rewritten) */
#define SYN_OPT_MAX 64
typedef struct syn_opt_list { float* p[SYN_OPT_MAX]; const float* g[SYN_OPT_MAX]; float* m[SYN_OPT_MAX]; float* v[SYN_OPT_MAX];
                              int32_t numel[SYN_OPT_MAX]; int32_t n; } syn_opt_list;
int32_t syn_opt_blocks(const syn_opt_list* l);
int syn_opt_sqnorm(const syn_opt_list* l, float* partials, void* stream);
int syn_opt_scalars(const float* partials, int32_t n_partials, float max_norm, const float* lr_dev, float lr, float beta1, float beta2, float* step_dev,
                    float* scal4, void* stream);
int syn_opt_adam(const syn_opt_list* l, const float* scal4, float beta1, float beta2, float eps, float weight_decay, void* stream);
/* Gradient of an nn.Embedding table (models/denoiser.py:72, the word embedding in front of text_encoder_body): dw [vocab][dim] =
 * sum over the positions p with ids[p] == v of dy[p][:], added in increasing p (no atomics on the result; every row written by the one launch).
 * ids int64 [n_pos] (n_pos <= 8192 per call), dy fp32 rows of pitch ld >= dim (ABI 8: a column slice of the next Linear's data gradient), dim <= 512,
 * vocab <= 65536. */
int syn_embedding_wgrad(const int64_t* ids, const float* dy, int32_t ld, int32_t n_pos, int32_t vocab, int32_t dim, float* dw, void* stream);
/* Backward of an nn.Linear, the operand preparation in one pass over its output gradient [m_rows][n] fp32: the bf16 copy (data-gradient GEMM),
 * the bf16 transpose [n][m_rows] (weight-gradient GEMM) and colsum_part [m_rows / 64][n] = column sums of every 64-row block
 * (NULL to skip; the bias gradient is their sum over the first index: syn_linear_pair's bias_grad).
 * (ABI 8) The gradient is read where its producer left it: row r = row r / row_div of `dy`, rows of pitch ld floats (a column slice of a wider
 * data gradient = one piece of a torch.cat's backward; row_div > 1 = the backward of an average pool over row_div rows with const_scale = 1 / row_div),
 * times const_scale.
 * (ABI 5) row_scale (NULL or one float per rows_per_scale rows): times its row's factor - the backward of
 * syn_linear_res's `residual + row_scale * (x W^T + b)`, i.e. of x + DropPath(branch) (timm_transformer/transformer.py:21-38,195-198). */
int syn_linear_bwd_prep(const float* dy, int32_t ld, int32_t row_div, float const_scale, int32_t m_rows, int32_t n, const float* row_scale,
                        int32_t rows_per_scale, void* dy_bf16, void* dy_bf16_t, float* colsum_part, void* stream);
/* Attention core (transformer.py:83-104, 4 heads x 128, 32 tokens, no mask, no dropout) on the packed output of the
 * qkv Linear: qkv [n_seq][32][3][4][128] -> o [n_seq][32][512]; backward recomputes the probabilities. */
/* (ABI 5) o fp32 and / or o_bf16 (either may be NULL), as syn_ln_fwd. */
int syn_attn_fwd(const float* qkv, float* o, void* o_bf16, int32_t n_seq, void* stream);
int syn_attn_bwd(const float* qkv, const float* d_o, float* dqkv, int32_t n_seq, void* stream);

/* ---- per-clip conditioning: audio encoder -------------------------------------
 * WavEncoder.forward in eval mode (models/denoiser.py:304-322; BasicBlock models/utils/layer.py:144-184) with the
 * BatchNorms folded into the convolutions by the caller.  wav [n_clips][n_samples][cin] fp32 ->
 * out [n_clips][syn_wav_out_frames(n_samples)][256] fp32 (128 frames for the 68224 / 68266-sample clips).
 * conv[i]: fragment-packed (syn_pack_weight) bf16 weights W'[cout][tap][cin'] and fp32 bias of, in order:
 *   b0.conv2, b1.conv1|shortcut, b1.conv2, b2.conv1, b2.conv2, b3.conv1|shortcut, b3.conv2, b4.conv1, b4.conv2,
 *   b5.conv1|shortcut, b5.conv2  ("conv1|shortcut": output channels concatenated; strided convs as stride-1 convs
 *   over s-row groups: taps ceil(15/s), cin' = s*cin, taps >= 15 zero - syntalker_amd/conditioning.py builds them).
 * w_first: block 0's conv1 and shortcut, fp32 [2][15*cin][64] (tap-major) followed by the biases [2][64].
 * workspace: syn_wav_workspace_bytes() bytes, zeroed ONCE by the caller for a given (n_clips, n_samples). */
typedef struct syn_wav_conv { const void* w; const float* bias; } syn_wav_conv;
typedef struct syn_wavenc {
    int32_t cin;            /* waveform channels: 1 or 2 */
    int32_t reserved;
    const float* w_first;
    syn_wav_conv conv[11];
} syn_wavenc;
int32_t syn_wav_out_frames(int32_t n_samples);
int64_t syn_wav_workspace_bytes(int32_t n_clips, int32_t n_samples);
/* Where a clip's intermediates lie in the workspace (additive, SYN_ABI_VERSION stays 9; host only: no launch, no GPU needed) - the plan syn_wav_encode
 * itself runs from, for tests and tools that read the layers back.  Clip i starts at bf16 element i * per_clip.  out[SYN_WAV_LAYOUT_WORDS], in order:
 *   L1 L2 L3 L4          positions after blocks 0, 1 (= 2), 3 (= 4), 5 (L4 = syn_wav_out_frames)
 *   per_clip             bf16 elements of a clip's workspace (x 2 x n_clips = syn_wav_workspace_bytes)
 *   x1 z1 s1 x2 z2 x3 z3 s3 x4 z4 x5 z5 s5     bf16-element offsets inside a clip: x = a block's input, z = its conv1 output, s = its shortcut conv;
 *                        channels-last rows of 64 (x1 .. x3), 128 (z3 .. x5) or 256 (z5, s5) channels
 *   halo slack           zero rows in front of and behind the tensors a padded convolution reads (z1, x2, z2, z3, x4, z4, z5: row 0 of the data is
 *                        row `halo` of the region), zero rows behind those and behind the tensors a strided convolution reads in row groups (x1, x3, x5)
 * Non-zero with a syn_last_error message for out = NULL or n_samples < 15. */
#define SYN_WAV_LAYOUT_WORDS 20
int syn_wav_layout(int32_t n_samples, int64_t* out);
int syn_wav_encode(const syn_wavenc* enc, const float* wav, int32_t n_clips, int32_t n_samples, void* workspace, float* out,
                   void* stream);

/* ---- per-clip conditioning behind the audio encoder --------------------------------
 * models/denoiser.py:147-157,160-174: word embedding -> Linear 300->256, cat with the audio features -> mix_audio_text
 * (512->256) -> avg_pool1d(4) -> . W2c^T, plus embed_text(seed) . W2a^T [+ style . W3s^T] and every bias: the additive
 * tensor `cond` of syn_step.  All of it is affine, so the caller folds it once per weight set (syntalker_amd/conditioning.py
 * CondWeights, fp64) into
 *   gt [256][512] = (W2c Wm_a)^T        tw [vocab][512] = word_embedding (W2c Wm_w Wt)^T      (the word path is a lookup)
 *   st [seed_dim + style_dim][512] = [W2a W_embed_text | W3s]^T        c0 [512] = all constant terms
 * audio_feat [n_clips][128][256] fp32 (syn_wav_encode), word [n_clips][128] int64, seed [n_clips][seed_dim], style
 * [n_clips][style_dim] or NULL, d_scratch [SYN_COND_SCRATCH_ROWS][n_clips][512] (ABI 4: the seed / style GEMM is split over K,
 * its partial sums are added in a fixed order) -> cond [n_clips][32][512].  Two launches, fp32 arithmetic. */
#define SYN_COND_SCRATCH_ROWS 8
typedef struct syn_cond_weights {
    const float* gt; const float* tw; const float* st; const float* c0;
    int32_t vocab, seed_dim, style_dim, reserved;
} syn_cond_weights;
int syn_cond_encode(const syn_cond_weights* w, const float* audio_feat, const int64_t* word, const float* seed, const float* style,
                    int32_t n_clips, float* d_scratch, float* cond, void* stream);

/* ---- load-time helpers -------------------------------------------------------------------- */
/* fp32 row-major W[n][k] (nn.Linear.weight layout) -> packed bf16 fragments (n*k*2 bytes).
 * n % 16 == 0, k % 32 == 0. */
int syn_pack_weight(const float* w, int32_t n, int32_t k, void* out_packed, void* stream);
/* Same fragments for W = S^T, S row-major [k][n], fp32 (is_bf16 = 0) or bf16: the training path packs W^T (dgrad) and
 * x^T (wgrad) without materialising transposed copies. */
int syn_pack_weight_t(const void* s_kn, int32_t is_bf16, int32_t n, int32_t k, void* out_packed, void* stream);

/* ---- layout at loop entry / exit ----------------------------------------------------------- */
/* Fragment order of the wave-per-sequence kernel: fp32 [clip][channel/32][q][lane = 32 hi + frame][r] holds channel
 * 32 nf + 8 q + 4 hi + r (what a lane owns after the output GEMM); bf16 [clip][channel/32][c][lane][e] holds channel
 * 32 nf + 16 c + 8 (e >> 2) + 4 hi + (e & 3) (the B operand of the input GEMM).  (B,1536,1,32) fp32 -> both (nullable). */
int syn_x_to_fragment(const float* x_bct, int32_t n_clips, float* out_f32, void* out_bf16, void* stream);
/* fragment-order fp32 -> (B,1536,1,32) fp32. */
int syn_x_from_fragment(const float* x_frag, int32_t n_clips, float* out_bct, void* stream);
/* (B,1536,1,32) fp32 -> token-major fp32 (nullable) and bf16 (nullable). */
int syn_to_token_major(const float* x_bct, int32_t n_clips, float* out_f32, void* out_bf16, void* stream);
/* token-major fp32 -> (B,1536,1,32) fp32. */
int syn_from_token_major(const float* x_btc, int32_t n_clips, float* out_bct, void* stream);

/* q_sample / generic axpby on flat fp32 buffers: out = a[t_row[clip]]*x + b[t_row[clip]]*y, clip = i / per_clip.
 * (diffusion/gaussian_diffusion.py:235-253). */
int syn_axpby_rows(const float* x, const float* y, const float* coef_ab /*[n][2]*/, const int32_t* t_row,
                   int32_t n_clips, int32_t per_clip, float* out, void* stream);

/* Philox4x32-10 + Box-Muller N(0,1): out[i] depends only on (seed, stream_id, i) — the same values
 * for any batch sharding across GPUs.  n % 4 == 0. */
int syn_randn(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t first_index, void* stream);

/* ---- RVQ-VAE either side of the loop (eval mode) ---------------------------------------------
 * One Conv1d of models/vq/encdec.py / resnet.py on channels-last activations:
 *   out[t][co] = bias[co] + sum_{tap,ci} W[co][ci][tap] * relu_in?(in[(t*stride + tap*dil - pad) >> up][ci])  (+ resid[t][co])
 * x_bf16 [clips][t_in][cin] (MFMA operand), outputs fp32 [clips][t_out][ldy] (first cout_valid channels) and/or bf16
 * [clips][t_out][cout].  w_packed: fragments [taps][cout/16][cin/32][64 lanes][8 bf16] (host: rvqvae.pack_conv).
 * up = 1 folds nn.Upsample(scale_factor=2, nearest) (encdec.py:56) into the read.  cin % 32 == 0, cout % 128 == 0
 * (callers zero-pad; cout_valid = real channel count). */
typedef struct syn_vq_conv {
    const void*  w_packed;
    const float* bias;            /* [cout] */
    int32_t cin, cout, cout_valid, taps, stride, dil, pad, up, relu_in, relu_out;
} syn_vq_conv;
int syn_vq_conv1d(const syn_vq_conv* cv, const void* x_bf16, const float* resid, float* y_f32, int32_t ldy, void* y_bf16,
                  int32_t clips, int32_t t_in, int32_t t_out, void* stream);

/* The whole model of one body part (models/vq/model.py:RVQVAE as diffusion_rvqvae_trainer.py:105-150 builds it):
 * enc = model.0, then per down stage { k4 s2 conv, 3 x (conv1, conv2) with dilations 9, 3, 1 }, final conv (16 convs);
 * dec = model.0, per up stage { 3 x (conv1, conv2), the conv behind nn.Upsample }, model.4, model.6 (17 convs). */
typedef struct syn_vq_model {
    int32_t pose_dim, reserved;
    syn_vq_conv enc[16];
    syn_vq_conv dec[17];
    const float* codebooks;       /* [6][512][512] */
    const float* codebooks_t;     /* [6][dim][code] */
    const float* code_sq;         /* [6][512] */
} syn_vq_model;
/* bytes of scratch for `clips` clips of `t_pose` pose frames (t_pose = 4 x latent rows) */
int64_t syn_vq_workspace_bytes(int32_t clips, int32_t t_pose, int32_t pose_dim);
/* RVQVAE.map2latent (models/vq/model.py:95-100): pose fp32 [clips][t_pose][pose_dim] -> latent fp32 [clips][t_pose/4][512] */
int syn_vq_map2latent(const syn_vq_model* m, const float* pose, int32_t clips, int32_t t_pose, void* workspace, float* latent,
                      void* stream);
/* RVQVAE.latent2origin (:102-109): latent fp32 [clips][t_lat][512] -> pose fp32 [clips][4 t_lat][pose_dim]; idx, sqerr,
 * hist as in syn_vq_quantize (hist zeroed by the caller). */
int syn_vq_latent2origin(const syn_vq_model* m, const float* latent, int32_t clips, int32_t t_lat, void* workspace, float* pose_out,
                         int32_t* idx, float* sqerr, int32_t* hist, void* stream);
/* RVQVAE.forward_decoder (:86-93): indices [clips][t_lat][n_q] -> pose fp32 [clips][4 t_lat][pose_dim] */
int syn_vq_forward_decoder(const syn_vq_model* m, const int32_t* idx, int32_t n_q, int32_t clips, int32_t t_lat, void* workspace,
                           float* pose_out, void* stream);

/* ---- pose formats either side of the RVQ-VAEs (diffusion_rvqvae_trainer.py:257-272 `_load_data`, :503-531 `_g_test`) ---------------------------
 * SMPL-X joint rotations: axis-angle fp32 [n_joints][3] <-> the 6D representation fp32 [n_joints][6] (first two rows of the rotation matrix).
 * syn_axis_angle_to_rot6d replaces rc.matrix_to_rotation_6d(rc.axis_angle_to_matrix(x)) (utils/rotation_conversions.py:416-430, 448-477, 36-64,
 * 535-550); syn_rot6d_to_axis_angle replaces rc.matrix_to_axis_angle(rc.rotation_6d_to_matrix(x)) (:511-533, 96-118, 432-446, 480-508).  The
 * reference's arithmetic operation for operation (small-angle series below 1e-6 rad, sqrt-of-positive-part + copysign quaternion); in and
 * out may not alias; n_joints = 0 is a no-op. */
int syn_axis_angle_to_rot6d(const float* axis_angle, int64_t n_joints, float* rot6d, void* stream);
int syn_rot6d_to_axis_angle(const float* rot6d, int64_t n_joints, float* axis_angle, void* stream);

/* ---- TMR encoders (models/temos/motionencoder/actor.py, textencoder/distillbert_actor.py; h3d_diffusion_new_trainer.py:170-176, 370-374) ----
 * ActorAgnosticEncoder's stack: input Linear (ReLU first for the text encoder's projection), [mu_token; logvar_token; rows] + pe, 4 post-norm
 * nn.TransformerEncoderLayer (256 wide, 4 heads x 64, FF 1024, erf GELU, LayerNorm eps 1e-5, dropout inactive), keys >= 2 + length masked;
 * out: mu = final[0], logvar = final[1].  GEMMs on hi + lo bf16 operands, attention on bf16 operands, fp32 residual / LayerNorm / softmax. */
#define SYN_TMR_D         256
#define SYN_TMR_LAYERS    4
#define SYN_TMR_MAX_LEN   254      /* rows per sequence without the two distribution tokens */
#define SYN_TMR_MAX_FEATS 4096     /* columns of the input Linear */
#define SYN_TMR_MAX_SEQ   65536

typedef struct syn_tmr_layer {
    const void*  w_qkv;  const float* b_qkv;      /* packed self_attn.in_proj_weight (768 x 256), in_proj_bias      */
    const void*  w_out;  const float* b_out;      /* packed self_attn.out_proj (256 x 256), bias                   */
    const float* ln1_g;  const float* ln1_b;      /* norm1                                                          */
    const void*  w_fc1;  const float* b_fc1;      /* packed linear1 (1024 x 256), bias                              */
    const void*  w_fc2;  const float* b_fc2;      /* packed linear2 (256 x 1024), bias                              */
    const float* ln2_g;  const float* ln2_b;      /* norm2                                                          */
} syn_tmr_layer;

typedef struct syn_tmr_model {
    int32_t      nfeats;                          /* columns of the input Linear (623 motion, 768 DistilBERT)       */
    int32_t      relu_in;                         /* 1: ReLU before the input Linear (projection = ReLU, Linear)    */
    const void*  w_in;   const float* b_in;       /* packed skel_embedding / projection.1 (256 x nfeats), bias      */
    const float* mu_token; const float* logvar_token;   /* (256) each                                              */
    const float* pe;                              /* sequence_pos_encoding.pe: >= max_len + 2 rows of 256           */
    syn_tmr_layer layer[SYN_TMR_LAYERS];
} syn_tmr_model;

/* fp32 w [n][k] (nn.Linear layout) -> `out`: hi then lo bf16 MFMA fragments, 2 x n x roundup(k, 32) bf16 (4 n roundup(k, 32) bytes).
 * n a multiple of 16, 1 <= k <= SYN_TMR_MAX_FEATS.  Once per weight change. */
int syn_tmr_pack_weight(const float* w, int32_t n, int32_t k, void* out, void* stream);
/* features fp32 [n_seq][max_len][nfeats] -> mu, logvar fp32 [n_seq][256].  lengths: device int32 [n_seq] valid rows per sequence (clamped to
 * 0 .. max_len), NULL = all max_len.  workspace: (max_len + 2) n_seq x 7680 bytes (x fp32 256 | qkv bf16 768 | attention fp32 256 |
 * FF hidden fp32 1024 per row).  1 <= max_len <= SYN_TMR_MAX_LEN, 1 <= n_seq <= SYN_TMR_MAX_SEQ.  22 launches, no allocation, no sync. */
int syn_tmr_encode(const syn_tmr_model* m, const float* features, int32_t n_seq, int32_t max_len, const int32_t* lengths, void* workspace,
                   float* mu, float* logvar, void* stream);

/* ---- DistilBERT in front of the TMR text encoder (transformers' DistilBertModel as textencoder/distillbert_actor.py:44-49 calls it) ----
 * token ids -> last_hidden_state: word_embeddings[id] + position_embeddings[position], LayerNorm; n_layers post-norm TransformerBlocks
 * (q_lin | k_lin | v_lin as one 2304 x 768 product, 12 heads x 64 with scale 1/8 and keys >= length masked, out_lin + residual +
 * sa_layer_norm, lin1 + erf GELU, lin2 + residual + output_layer_norm); every LayerNorm with eps 1e-12, dropout inactive.  GEMMs and both
 * attention products on hi + lo bf16 operands (three MFMAs per product, fp32 accumulate), fp32 residual / LayerNorm / softmax. */
#define SYN_BERT_D          768
#define SYN_BERT_HEADS      12
#define SYN_BERT_FF         3072
#define SYN_BERT_MAX_LAYERS 12

typedef struct syn_bert_layer {
    const void*  w_qkv;  const float* b_qkv;      /* packed [q_lin; k_lin; v_lin].weight (2304 x 768), the three biases (2304)  */
    const void*  w_out;  const float* b_out;      /* packed attention.out_lin (768 x 768), bias                                 */
    const float* ln1_g;  const float* ln1_b;      /* sa_layer_norm                                                               */
    const void*  w_fc1;  const float* b_fc1;      /* packed ffn.lin1 (3072 x 768), bias                                          */
    const void*  w_fc2;  const float* b_fc2;      /* packed ffn.lin2 (768 x 3072), bias                                          */
    const float* ln2_g;  const float* ln2_b;      /* output_layer_norm                                                           */
} syn_bert_layer;

typedef struct syn_bert_model {
    int32_t      n_layers;                        /* 1 .. SYN_BERT_MAX_LAYERS                                                    */
    int32_t      vocab;                           /* rows of `word`; ids are clamped to 0 .. vocab - 1 inside the kernel         */
    int32_t      n_pos;                           /* rows of `pos` (>= max_len of a call)                                        */
    int32_t      reserved;
    const float* word;   const float* pos;        /* embeddings.word_embeddings (vocab x 768), position_embeddings (n_pos x 768), fp32, 16-byte aligned */
    const float* emb_ln_g; const float* emb_ln_b; /* embeddings.LayerNorm                                                        */
    syn_bert_layer layer[SYN_BERT_MAX_LAYERS];    /* packed with syn_tmr_pack_weight                                             */
} syn_bert_model;

/* ids int32 [n_seq][max_len] -> hidden fp32 [n_seq][max_len][768] (last_hidden_state); rows at or beyond a sequence's length are written as
 * zeros.  lengths: device int32 [n_seq] valid tokens per sequence, a prefix (clamped to 0 .. max_len), NULL = all max_len.
 * workspace: n_seq max_len x 24576 bytes (qkv fp32 2304, reused for a Linear's output before its LayerNorm | attention fp32 768 | FF hidden
 * fp32 3072 per row), 16-byte aligned like `hidden`.  1 <= max_len <= SYN_TMR_MAX_LEN, 1 <= n_seq <= SYN_TMR_MAX_SEQ.
 * 1 + 7 n_layers launches, no allocation, no sync. */
int syn_bert_encode(const syn_bert_model* m, const int32_t* ids, int32_t n_seq, int32_t max_len, const int32_t* lengths, void* workspace,
                    float* hidden, void* stream);

/* ---- FGD motion embedder (models/motion_representation.py:67-75 VAESKConv.map2latent = LocalEncoder, models/motion_encoder.py:698-787;
 * diffusion_rvqvae_trainer.py:613-619, 716-718) ----------------------------------------------------------------------------------------------
 * Four SkeletonResidual layers (models/utils/skeleton.py:547-586) over the SMPL-X edge graph, frames halved by each:
 *     r = GroupNorm(10, cout)(conv1d(x, W*M, b, kernel 4, stride 2, zero pad 1)),  s = conv1d(x, Ws*Ms, bs, kernel 1, stride 2),
 *     out = tanh(P (r + s))                  (P: SkeletonPool's mean pooling, :162-235; identity where the layer keeps its edges)
 * GroupNorm per clip over cout / 10 channels x all frames, eps 1e-5.  fp32 operands on v_mfma_f32_16x16x4_f32 (exact fp32 products). */
#define SYN_SKEL_LAYERS   4
#define SYN_SKEL_MAX_C    384      /* input / output channels of a layer (its 34-frame input window is staged in LDS, 64 KB at most) */
#define SYN_SKEL_POOL_MAX 4        /* inputs one pooled channel averages */
#define SYN_SKEL_MAX_CLIPS 65536  /* and at most 2^24 clip x 16-frame tiles in layer 0 */

typedef struct syn_skel_layer {
    const float*   w;          /* syn_skel_pack_weight's fragments: 64 floats per kept chunk                                        */
    const int32_t* chunk_off;  /* [2 roundup(cout, 16) / 16 + 1]: kept chunks of output-column tile t are chunk_off[t] .. chunk_off[t+1] - 1 */
    const int32_t* chunk_k;    /* per kept chunk: (tap << 16) | first input channel (a multiple of 4) of its 4 consecutive channels    */
    const float*   bias;       /* [2 roundup(cout, 16)]: residual.0.bias | shortcut.bias, each zero-padded to roundup(cout, 16)          */
    const float*   gn_g;       /* residual.1.weight [cout] */
    const float*   gn_b;       /* residual.1.bias   [cout] */
    const int32_t* pool_src;   /* [out_width][SYN_SKEL_POOL_MAX]: channels of (r + s) an output channel averages, -1 = none          */
    const float*   pool_w;     /* [out_width][SYN_SKEL_POOL_MAX]: their weights (common.0.weight's nonzeros; 1 for identity)        */
    int32_t        cin;        /* input channels (the previous layer's out_width)                                                  */
    int32_t        cout;       /* conv output channels, a multiple of 10                                                           */
    int32_t        out_width;  /* channels after the pooling                                                                       */
    int32_t        reserved;
} syn_skel_layer;

typedef struct syn_skel_model {
    syn_skel_layer layer[SYN_SKEL_LAYERS];
} syn_skel_model;

/* One layer's weights, both branches in one matrix: column n < cout_p = roundup(cout, 16) is residual.0's output channel n, column
 * cout_p + n the shortcut's; row k = tap * roundup(cin, 4) + c (the shortcut reads tap 1, x[2t], only).  w [cout][cin][4] * mask,
 * ws [cout][cin][1] * ms, gathered for the kept chunks listed in chunk_off / chunk_k (the caller chooses them: chunks holding a nonzero)
 * into out [chunk_off[last]][64] as the MFMA's B operand (lane l: row 4 chunk + (l >> 4), column 16 t + (l & 15)).  Once per weight change. */
int syn_skel_pack_weight(const float* w, const float* mask, const float* ws, const float* ms, int32_t cout, int32_t cin, const int32_t* chunk_off,
                         const int32_t* chunk_k, float* out, void* stream);
/* x fp32 [n_clips][n_frames][layer[0].cin] -> out fp32 [n_clips][n_frames / 16][layer[3].out_width].  n_frames a positive multiple of 16,
 * 1 <= n_clips <= SYN_SKEL_MAX_CLIPS.  workspace: per layer i (T = n_frames >> (i + 1)), the pre-norm r | s fp32 [n_clips][T][2 roundup(cout, 16)]
 * then the GroupNorm partial sums fp64 [n_clips][ceil(T / 16)][10][sum, sum of squares], each region rounded up to 256 bytes.  Five launches
 * (a conv per layer, each normalising its input while staging it; one for the last layer's output), no allocation, no sync, no atomics:
 * bitwise reproducible, and each clip independent of the others in the batch. */
int syn_skel_encode(const syn_skel_model* m, const float* x, int32_t n_clips, int32_t n_frames, void* workspace, float* out, void* stream);

/* ---- T2M text-motion co-embedding evaluator (utils/t2m_eval_tools.py:332-351 MovementConvEncoder, :564-639 TextEncoderBiGRUCo /
 * MotionEncoderBiGRUCo; EvaluatorMDMWrapper :833-899), eval mode ---------------------------------------------------------------------------------
 *   movement: Conv1d(619 -> 512, k4, s2, p1), LeakyReLU 0.2, Conv1d(512 -> 512, k4, s2, p1), LeakyReLU 0.2, Linear(512, 512)
 *   motion:   Linear(512 -> 1024), bidirectional GRU H = 1024 over `lengths` steps from the learned initial state, forward | reverse final
 *             state -> Linear(2048 -> 1024), LayerNorm, LeakyReLU 0.2, Linear(1024 -> 512)
 *   text:     word_embs + Linear(15 -> 300)(pos_onehot), Linear(300 -> 512), bidirectional GRU H = 512, the same head (1024 -> 512 -> 512)
 * GRU gates in torch's order r | z | n.  fp32 operands on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation) throughout. */
#define SYN_T2M_POSE       619     /* pose channels the movement encoder reads (the first 619 of each `ld`-wide frame)   */
#define SYN_T2M_MOVE       512
#define SYN_T2M_MOTION_H   1024
#define SYN_T2M_TEXT_H     512
#define SYN_T2M_WORD       300
#define SYN_T2M_POS        15
#define SYN_T2M_EMB        512
#define SYN_T2M_MAX_SEQ    65536
#define SYN_T2M_MAX_FRAMES 1024    /* frames of a motion / tokens of a caption */
#define SYN_T2M_MOTION     0       /* `kind` of syn_t2m_workspace_bytes */
#define SYN_T2M_TEXT       1

typedef struct syn_t2m_gru {       /* nn.GRU(H, H, bidirectional): H = 1024 (motion) or 512 (text)                              */
    const float* w_ih;             /* packed (layout 0) [weight_ih_l0 ; weight_ih_l0_reverse], 6 H x H                          */
    const float* b_ih;             /* [bias_ih_l0 ; bias_ih_l0_reverse], 6 H                                                     */
    const float* w_hh[2];          /* packed (layout H) weight_hh_l0, weight_hh_l0_reverse, 3 H x H each                        */
    const float* b_hh;             /* [bias_hh_l0 ; bias_hh_l0_reverse], 6 H                                                     */
    const float* hidden;           /* the module's `hidden` (2, 1, H): initial state per direction                              */
} syn_t2m_gru;

typedef struct syn_t2m_head {      /* output_net: Linear(2 H -> H), LayerNorm(H), LeakyReLU, Linear(H -> 512); w1, w2 packed    */
    const float* w1; const float* b1; const float* ln_g; const float* ln_b; const float* w2; const float* b2;
} syn_t2m_head;

typedef struct syn_t2m_model {     /* every w packed by syn_t2m_pack_weight (layout 0 unless noted), every bias plain fp32      */
    const float* conv1_w; const float* conv1_b;            /* main.0 (512, 619, 4): packed with conv_cin 619                     */
    const float* conv2_w; const float* conv2_b;            /* main.3 (512, 512, 4): packed with conv_cin 512                     */
    const float* out_w;   const float* out_b;              /* out_net                                                             */
    const float* motion_in_w; const float* motion_in_b;    /* MotionEncoderBiGRUCo.input_emb                                      */
    syn_t2m_gru  motion_gru;  syn_t2m_head motion_head;
    const float* pos_w;   const float* pos_b;              /* TextEncoderBiGRUCo.pos_emb (300, 15)                                */
    const float* text_in_w; const float* text_in_b;        /* TextEncoderBiGRUCo.input_emb                                        */
    syn_t2m_gru  text_gru;    syn_t2m_head text_head;
} syn_t2m_model;                   /* an entry reads its own encoder's members only: a motion-only model may leave the text ones NULL */

/* fp32 w [n][k] (nn.Linear; conv_cin 0) or [n][conv_cin][4] (nn.Conv1d k4, k = 4 conv_cin, packed with row tap * conv_cin + c) -> `out`,
 * float4 MFMA fragments (element j of lane l: row 16 q + 4 (l >> 4) + j, column 16 tile + (l & 15); zero outside n x k).
 * layout 0: the GEMM's order, roundup(n, 128) x roundup(k, 16) floats.  layout H (512 or 1024; n = 3 H, k = H): the recurrent kernel's
 * consumption order (per wave of 8: H / 8 hidden units x 3 gates, K block by K block), 3 H x H floats.  Once per weight change. */
int syn_t2m_pack_weight(const float* w, int32_t n, int32_t k, int32_t conv_cin, int32_t layout, float* out, void* stream);
/* Bytes of `workspace` for a call (kind SYN_T2M_MOTION: max_len = n_frames; SYN_T2M_TEXT: max_len tokens); -1 for arguments the encoders
 * refuse.  Dominated by W_ih x of every step, 6 H floats per sequence and step. */
int64_t syn_t2m_workspace_bytes(int32_t n_seq, int32_t max_len, int32_t kind);
/* motions fp32 [n_seq][n_frames][ld] (the first 619 channels of a frame are read; zero beyond a motion's own frames, as the loader pads
 * them) -> out fp32 [n_seq][512], row i = sequence i.  lengths_dev: device int32 [n_seq] GRU steps per sequence (m_lens // 4, clamped to
 * 0 .. T'', T' = (n_frames - 2) / 2 + 1, T'' = (T' - 2) / 2 + 1).  order_dev: device int32 [n_seq], a permutation: the recurrent kernel
 * takes sequences order[16 b .. 16 b + 15] as workgroup b's tile and runs the tile for its longest member, so sort by length.
 * 4 <= n_frames <= SYN_T2M_MAX_FRAMES, 1 <= n_seq <= SYN_T2M_MAX_SEQ.  8 launches, no allocation, no sync, no atomics, no inter-workgroup
 * hand-off: bitwise reproducible, each sequence independent of the others in the batch. */
int syn_t2m_encode_motion(const syn_t2m_model* m, const float* motions, int32_t n_seq, int32_t n_frames, int32_t ld, const int32_t* lengths_dev,
                          const int32_t* order_dev, void* workspace, float* out, void* stream);
/* word_embs fp32 [n_seq][max_len][300], pos_onehot fp32 [n_seq][max_len][15] -> out fp32 [n_seq][512]; lengths_dev: tokens per caption
 * (clamped to 0 .. max_len), order_dev as above.  6 launches. */
int syn_t2m_encode_text(const syn_t2m_model* m, const float* word_embs, const float* pos_onehot, int32_t n_seq, int32_t max_len,
                        const int32_t* lengths_dev, const int32_t* order_dev, void* workspace, float* out, void* stream);

/* ResidualVQ.forward in eval mode (models/vq/residual_vq.py:91-140 over quantizer.py:62-69,143-171), fp32, 6 layers
 * of 512 codes x 512 dims: x [rows][512] -> q_f32 / q_bf16 [rows][512] (sum of the straight-through outputs), idx
 * [rows][6], sqerr [syn_vq_quantize_groups(rows)][6] (per-group sums of |residual - code|^2: commit loss numerators),
 * hist [6][512] (code usage for the perplexity; the caller zeroes it).  codebooks [6][512][512], codebooks_t
 * [6][dim][code] (transposed), code_sq [6][512] = |code|^2. */
int32_t syn_vq_quantize_groups(int32_t rows);
int syn_vq_quantize(const float* x, const float* codebooks, const float* codebooks_t, const float* code_sq, float* q_f32,
                    void* q_bf16, int32_t* idx, float* sqerr, int32_t* hist, int32_t rows, void* stream);
/* Sum of the codes of given indices (RVQVAE.forward_decoder, models/vq/model.py:86-89): idx [rows][n_q], -1 = no code. */
int syn_vq_codes(const int32_t* idx, const float* codebooks, float* q_f32, void* q_bf16, int32_t rows, int32_t n_q, void* stream);

/* ---- RVQ-VAE training (reference rvq_beatx_train.py over models/vq/ in train mode; additive, ABI 9) ----------
 * The step's convolutions - forward and data gradients - are syn_vq_conv1d calls; these are the pieces around them.  No entry point
 * allocates, synchronises or uses a floating-point atomic: a step is bitwise reproducible.
 * syn_vq_train_pack: n_jobs packing jobs in ONE launch, read from device memory: an array of
 *   { const float* w; void* out; int32_t cout, cin, taps, cout_p, cin_p, kind; }   (40 bytes)
 * kind 0: Conv1d weight fp32 [cout][cin][taps] -> syn_vq_conv.w_packed fragments for (cout_p, cin_p); kind 1: the data gradient's operand
 * W'[ci][co][taps-1-tap] = W[co][ci][tap], fragments for (cout_p = pad128(cin), cin_p = pad32(cout)); kind 2: fp32 vector [cout] -> [cout_p], zero
 * padded; kind 3: as kind 0 of bf16(w - float(bf16(w))), the part of the weight its bf16 copy drops.  max_units = the largest job's taps * cout_p/16 * cin_p/32 * 64 (kind 2: cout_p). */
int syn_vq_train_pack(const void* jobs_dev, int32_t n_jobs, int32_t max_units, void* stream);
/* x fp32 [rows][dim] -> bf16 [rows][dim_padded], zero padded (the first convolution's operand); out_lo_bf16 (NULL to skip) = bf16(x - float(bf16(x))) */
int syn_vq_train_cast(const float* x, int64_t rows, int32_t dim, int32_t dim_padded, void* out_bf16, void* out_lo_bf16, void* stream);
/* out = scale_resid * resid + scale_v * [relu_src > 0] * [keep != 0] * v over n (% 4 == 0) elements; resid, relu_src_bf16, keep (bytes) optional,
 * out_f32 / out_bf16 / out_lo_bf16: at least one.  out_lo_bf16 = bf16(out - float(bf16(out))), stored as zero where out <= 0 when lo_relu != 0 (for a
 * consumer that applies ReLU by the sign of the high part).  Dropout + residual add behind conv2 (resnet.py:66-67), the high / low split of the
 * training forward's activations, the ReLU masks of the backward, the encoder's gradient. */
int syn_vq_train_ew(const float* v, const float* resid, const void* relu_src_bf16, const uint8_t* keep, float scale_v, float scale_resid,
                    float* out_f32, void* out_bf16, void* out_lo_bf16, int32_t lo_relu, int64_t n, void* stream);
/* backward of nn.Upsample(2, nearest): out [rows_out][channels] = du[2 r] + du[2 r + 1] */
int syn_vq_train_pairsum(const float* du, float* out, int64_t rows_out, int32_t channels, void* stream);
/* out bf16 [2 rows_in][channels]: out[2 r] = dy[r], out[2 r + 1] = 0 - the stride-2 convolutions' data gradient as a stride-1 convolution */
int syn_vq_train_stuff(const void* dy_bf16, void* out_bf16, int64_t rows_in, int32_t channels, void* stream);
/* dw fp32 [cout][cin][taps] = sum_{n,t} dy[n][t][co] * x[n][(t*stride + tap*dil - pad) >> up][ci] (ReLU on x when relu_in), db [cout] = sum dy (NULL to
 * skip); dy bf16 [clips][t_out][ldy], x bf16 [clips][t_in][ldx].  bf16 MFMA, fp32 accumulation, one workgroup sums all positions of its tile in
 * order.  Reads outside a clip's frames are bounds-checked to zero. */
int syn_vq_train_wgrad(const void* dy_bf16, int32_t ldy, const void* x_bf16, int32_t ldx, float* dw, float* db, int32_t clips, int32_t t_in,
                       int32_t t_out, int32_t cout, int32_t cin, int32_t taps, int32_t stride, int32_t dil, int32_t pad, int32_t up, int32_t relu_in,
                       void* stream);
/* one layer's codebook fp32 [512][512] -> its transpose and |code|^2 [512] (what syn_vq_quantize / syn_vq_train_quantize take) */
int syn_vq_train_codebook_prep(const float* codebook, float* codebook_t, float* code_sq, void* stream);
/* init_codebook (quantizer.py:60-65): codebook = code_sum = _tile(x)[:512], code_count = 1; x fp32 [rows][512], noise fp32 [512][512] normal draws
 * (required when rows < 512: row c = x[c % rows] + noise[c] * 0.01 / sqrt(512)) */
int syn_vq_train_tile(const float* x, int32_t rows, const float* noise, float* codebook, float* code_sum, float* code_count, void* stream);
/* One layer of ResidualVQ.forward in training, without the codebook update: index = argmax(-distance / temperature + gumbel) (gumbel fp32
 * [rows][512], NULL: plain argmin), idx [rows][6] column `layer`; x_out = x_in - quantised (must not alias x_in); q_acc (+)= the straight-through
 * output, q_bf16 (NULL to skip) = bf16(q_acc), resid_sum (+)= x_in - code; `first` != 0 starts both sums.  sqerr [syn_vq_quantize_groups(rows)]. */
int syn_vq_train_quantize(const float* x_in, const float* codebook, const float* codebook_t, const float* code_sq, const float* gumbel, float temperature,
                          float* x_out, float* q_acc, void* q_bf16, float* resid_sum, int32_t* idx, float* sqerr, int32_t layer, int32_t first, int32_t rows,
                          void* stream);
/* update_codebook (quantizer.py:107-130) of one layer from its input rows and indices: EMA of the per-code sums (rows added in ascending order) and
 * counts, usage = count >= 1, unused codes <- _tile(x)[:512] (noise as in syn_vq_train_tile); batch_count fp32 [512] = this batch's counts. */
int syn_vq_train_codebook_update(const float* x_in, const int32_t* idx, int32_t layer, int32_t rows, const float* noise, float mu, float one_minus_mu,
                                 float* codebook, float* code_sum, float* code_count, float* batch_count, void* stream);
/* Reconstruction loss over the real channels (kind 0: MSE, 1: L1, 2: SmoothL1 beta 1; mean over rows * dim): parts [syn_vq_train_loss_parts] =
 * per-workgroup sums, d_rec_bf16 [rows][dim_padded] = d loss / d rec, zero in the padding. */
int32_t syn_vq_train_loss_parts(int64_t rows, int32_t dim_padded);
int syn_vq_train_loss(const float* rec, const float* gt, int64_t rows, int32_t dim, int32_t dim_padded, int32_t kind, void* d_rec_bf16, float* parts,
                      void* stream);
/* out4 = {loss, recons, commit, perplexity}: recons = sum(parts) / count, commit / perplexity = means over the n_active layers of
 * sqerr[q][groups] / (rows * 512) and exp(-sum p log(p + 1e-7)), p = batch_count[q] / rows; loss = recons + commit_weight * commit. */
int syn_vq_train_scalars(const float* parts, int32_t n_parts, int64_t count, const float* sqerr, int32_t groups, const float* batch_count, int32_t n_active,
                         int32_t rows, float commit_weight, float* out4, void* stream);

/* ---- training building block ------------------------------------------------------------------------
 * y[m][n] = sum_k x[m][k] * W[n][k] (+ bias[n]): nn.Linear forward on the MFMA GEMM (bf16 operands, fp32 accumulate
 * and output).  The same entry point serves the backward passes with re-packed operands:
 *   dgrad  dx = dy . W      -> x := dy (m x n_out),   w_packed := pack(W^T)   (n_in x n_out)
 *   wgrad  dW = dy^T . x    -> x := dy^T (n_out x m), w_packed := pack(x^T)   (n_in x m)
 * n % 128 == 0, k % 128 == 0 (callers zero-pad; n % 512 != 0 runs on the 128-column tiles, ABI 7).  Replaces torch.nn.functional.linear for
 * models/timm_transformer/transformer.py:85,102,146,149 and models/denoiser.py:148,162,170,195 in training. */
int syn_linear(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k, float* y,
               void* stream);
/* syn_linear and, in the same launch, syn_pack_weight_t(x_bf16, 1, k, m_rows, xt_packed): the fragments of x^T the weight-gradient
 * GEMM of the backward will take, packed in the shadow of the forward GEMM (which fills a quarter to three quarters of the chip). */
int syn_linear_and_pack(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k, float* y,
                        void* xt_packed, void* stream);
/* Two independent syn_linear calls (no bias) as ONE launch: the data-gradient GEMM dy . W and the weight-gradient GEMM dy^T . x of
 * an nn.Linear's backward fill half the chip each and do not depend on each other.  Same result as two calls, bitwise.
 * (ABI 8) n % 128 == 0 (512-column or 128-column tiles; shapes neither form takes as a pair go out as two launches + the bias sum). */
/* (ABI 5) bias_grad [part_n] (NULL to skip) = sum over i < part_rows of bias_parts [i][part_n], added in order by the same launch: the
 * Linear's bias gradient from syn_linear_bwd_prep's colsum_part without a reduction launch of its own. */
int syn_linear_pair(const void* x1_bf16, const void* w1_packed, int32_t m1, int32_t n1, int32_t k1, float* y1,
                    const void* x2_bf16, const void* w2_packed, int32_t m2, int32_t n2, int32_t k2, float* y2,
                    const float* bias_parts, int32_t part_rows, int32_t part_n, float* bias_grad, void* stream);
/* (ABI 5) The last Linear of a pre-LN residual branch with the branch's tail in its epilogue (transformer.py:195-198,
 * x = x + drop_path(attn(norm1(x))) / x + drop_path(mlp(norm2(x)))): y = residual + row_scale[m / rows_per_scale] * (x W^T + bias),
 * residual and y fp32 [m_rows][n] (may alias), row_scale NULL = 1 (DropPath off), one factor per sample = rows_per_scale rows.
 * xt_packed (NULL to skip): as syn_linear_and_pack. */
int syn_linear_res(const void* x_bf16, const void* w_packed, const float* bias, const float* residual, const float* row_scale,
                   int32_t rows_per_scale, int32_t m_rows, int32_t n, int32_t k, float* y, void* xt_packed, void* stream);
/* (ABI 5) fc1 of the MLP (transformer.py:117-151) with the GELU behind it in the epilogue: y fp32 [m_rows][n] = x W^T + bias (kept for the
 * backward) and y_gelu_bf16 = bf16(GELU(y)) (exact erf form), the operand fc2 takes.  xt_packed (NULL to skip): as syn_linear_and_pack. */
int syn_linear_gelu(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k, float* y, void* y_gelu_bf16,
                    void* xt_packed, void* stream);

/* ---- single stages, exported for unit tests and bisecting ----------------------------------- */
/* Y[m][n] = sum_k X[m][k] * W[n][k] (+ bias[n]); X bf16 [m_rows][k], W packed, Y fp32 [m_rows][n]. n % 512 == 0. */
int syn_test_gemm(const void* x_bf16, const void* w_packed, const float* bias, int32_t m_rows, int32_t n, int32_t k,
                  int32_t m_tile, float* y, void* stream);
/* Adversarial check of the XCD-group barrier's acquire (syn_latency.inc): on every XCD one workgroup republishes `words`
 * (<= 4096) 32-bit words `rounds` times with a new payload each round, a second workgroup of the same XCD re-reads them
 * (L1-warm) after the flag, under mode 0: no invalidate, 1: `buffer_inv sc0` (what the barrier uses), 2: `buffer_inv sc1`,
 * while the other 30 workgroups of the XCD stream from `stream` (NULL: idle).  stale[xcd] (+= ) counts words read with an
 * old value.  sync [320] and stale [9] zeroed by the caller; buf [8][4096]. */
int syn_test_handoff(uint32_t* sync_320_zeroed, uint32_t* buf_8x4096, const float* stream, int64_t stream_n, uint32_t* stale_9_zeroed,
                     int32_t words, int32_t rounds, int32_t mode, void* stream_h);
/* (ABI 7) the matrix pipe alone in k_seq's occupancy (one wave per SIMD, 12 independent v_mfma_f32_32x32x16_bf16 accumulators, register operands): iters x 192
 * MFMAs per wave on every CU; out: 256 floats per CU (keeps the loop alive); *flops (host, may be NULL) = the floating-point operations of the launch.
 * Timed by bench.py as roofline.practical_peak: what the chip delivers on this instruction at the clock it holds under that load. */
int syn_test_mfma_rate(int32_t iters, float* out, int64_t* flops, void* stream);
/* attention over ws_q/ws_k/ws_vt -> ws_o for n_seq sequences of 32 tokens, 4 heads x 128. */
int syn_test_attention(const void* q, const void* k, const void* vt, int32_t n_seq, void* o, void* stream);

/* ---- diagnostics (scripts/diag_*.py, scripts/ubench_*.py, A/B environment switches; never called by the product path in its default configuration:
 * syn_debug_conv_terms is reached from syntalker_amd/training.py only when SYN_CONV_TERMS asks for something other than 3,3,3) ------
 * Process-wide switches of the library, not thread-safe, no status to return.  They replace nothing in the reference. */
/* per-phase cycle counters of the step kernels: the attention / MLP phases write s_memtime stamps into these device buffers (NULL: off).
 * The first buffer also takes the training convolutions' stamps while it is set: k_conv_train 8 slots per workgroup (start, tile staged, barrier passed,
 * k loop done, end, HW_ID: scripts/diag_conv_phases.py), k_conv_wgrad 8 per workgroup (cycles in the tile stores, in the k loop, in all, chunks:
 * scripts/diag_wgrad_phases.py) - size it for the launch's workgroups. */
void syn_debug_timing(long long* attn_buf, long long* mlp_buf);
/* 16-row plain GEMMs of the training step: 1 (default) = activation block resident in the LDS, 0 = the streaming loop (A/B, bitwise equal) */
void syn_debug_gemm_resident(int on);
/* pin syn_linear's row tile (16 / 32 / 64 / 128); 0 = automatic */
void syn_debug_linear_tile(int rows);
/* training-mode convolutions (syn_conv1d_train_*): which cross products of the hi / lo operand split the NEXT launches issue - bit 0: A_lo . B_hi
 * (A = weights, or dy in the weight gradient), bit 1: A_hi . B_lo (B = the activations: x, or dy in the data gradient); 3 = both, fp32-grade; a negative mask restores the defaults (3 forward / data gradient,
 * 1 weight gradient: x is read rounded to bf16 there, the sum over positions averages it out) */
void syn_debug_conv_terms(int mask);
/* k_seq: delay workgroup i by (i % 8) * units_of_64_cycles * 64 cycles at launch (phase experiments); -1 = off */
void syn_debug_seq_skew(int units_of_64_cycles);
/* k_seq: which step of a multi-step launch syn_debug_timing's stamps are taken in */
void syn_debug_seq_step(int step);

#ifdef __cplusplus
}
#endif
#endif /* SYN_HIP_H */
