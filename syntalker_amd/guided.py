"""Gradient-guided sampling on the HIP denoiser: the model output as a function of x_t that autograd can differentiate.

`cond_fn` / `cond_fn_with_grad` of the reference's loops (diffusion/gaussian_diffusion.py:427-503, 559-605, 793-848) steer a sample with the
gradient of any differentiable objective on x_t or on pred_xstart.  The second form needs d(model output) / d(x_t).  Every weight is frozen while
sampling and the conditioning does not depend on x_t, so the node here (`DenoiseFn`) is much less than a training step:

  forward   syn_guide_in_fwd (x (B, C, 1, T) -> h0 = rotary(x^T A^T + cond + TE[t]), one launch) | syn_train_stack_fwd, drop_path = NULL |
            syn_linear (poseFinal) | the variants' weighted sum per 512-channel block
  backward  w_v * d_out per variant | syn_linear against poseFinal^T | syn_train_stack_bwd | syn_guide_in_bwd per variant, accumulating in
            variant order.  No weight-gradient launch, no bias or LayerNorm gradient, nothing handed to `_grad_out`: it returns dx and nothing else.

`cond` is the hoisted per-clip conditioning of `MDM.variant_conds` (the audio encoder runs once per loop, not per step) and TE the packed model's
time table.  The persistent block kernels take 4 | n_seq <= 64 sequences: other counts are padded with zero sequences (zero gradient, cut from
the output), more than 64 run as consecutive slices of whole clips through the same node on the same stream (`plan`).  The transposed weight
fragments are packed once per set of weights (`_packs`), apart from the training path's per-step packs: `StackFn` and its caches are untouched.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, engine

MAX_SEQ = 64          # sequences of one launch of the persistent block kernels (syn_train_stack_fwd)


def plan(n_clips: int, n_variants: int = 1) -> list[tuple[int, int, int, int]]:
    """Slices of whole clips -> [(first clip, end clip, live sequences, launched sequences)]: at most 64 sequences per slice (a clip's V variants
    stay together), the launched count the next multiple of 4 (the block kernels' tile)."""
    if n_clips < 1 or n_variants < 1 or n_variants > MAX_SEQ:
        raise ValueError(f"guided denoiser: {n_clips} clips x {n_variants} variants (1 .. {MAX_SEQ} variants, at least one clip)")
    per = MAX_SEQ // n_variants
    out = []
    for lo in range(0, n_clips, per):
        hi = min(n_clips, lo + per)
        live = (hi - lo) * n_variants
        out.append((lo, hi, live, -(-live // 4) * 4))
    return out


class _Packs:
    """What the node takes beside the packed model: A^T, poseFinal^T and the blocks' W^T as MFMA fragments (frozen weights: built once)."""

    def __init__(self, mdm, pm):
        sd = {k: v.detach() for k, v in mdm.state_dict().items()}
        tr = lambda w: engine.pack_weight(w.float().t().contiguous())
        self.At = tr(pm.folded["A"])
        self.WoT = tr(sd["output_process.poseFinal.weight"])
        self.layers = []
        for i in range(engine.LAYERS):
            p = f"mytimmblocks.{i}."
            self.layers.append(tuple(tr(sd[p + n]) for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")))


def _packs(mdm):
    pm = mdm.packed()
    ent = mdm.__dict__.get("_syn_guide_packs")
    if ent is None or ent[0] is not pm:
        ent = mdm.__dict__["_syn_guide_packs"] = (pm, _Packs(mdm, pm))
    return pm, ent[1]


class _Ctx:
    """The operands of one slice that are no tensors of the autograd graph."""

    def __init__(self, mdm, cond, t_model, weights, n_seq):
        self.mdm, self.cond, self.t_model, self.weights, self.n_seq = mdm, cond, t_model, weights, n_seq


def _channel_weights(weights, v, n_clips):
    """Column v of the (3, V) or (B, 3, V) table as a factor over the 1536 channels of rows (B, 32, 1536)."""
    w = weights[..., v].repeat_interleave(engine.CH // 3, dim=-1)
    return w.view(1, 1, engine.CH) if w.dim() == 1 else w.view(n_clips, 1, engine.CH)


class DenoiseFn(torch.autograd.Function):
    """x (B, 1536, 1, 32) -> sum_v w_v * model_v(x) (B, 1536, 1, 32) for the V conditioning variants of `c` (cond (V, B, 32, 512), t_model int32
    (V B,), weights (3, V) | (B, 3, V) | None for V = 1); V B <= n_seq <= 64, 4 | n_seq.  backward: dx."""

    @staticmethod
    def forward(ctx, x, c):
        lib = _lib.load()
        from . import training
        mdm = c.mdm
        pm, gp = _packs(mdm)
        dev = x.device
        B = x.shape[0]
        V = c.cond.shape[0]
        live, n_seq = V * B, c.n_seq
        if n_seq % 4 or not 4 <= n_seq <= MAX_SEQ or live > n_seq or live < 1 or tuple(x.shape[1:]) != (engine.CH, 1, engine.T):
            raise _lib.SynHipError(f"guided denoiser: {live} sequences in a launch of {n_seq} (4 | n_seq, 4 <= n_seq <= {MAX_SEQ}), x {tuple(x.shape)}")
        if not training.engine_has_xcd_groups(dev):
            raise _lib.SynHipError("the persistent block kernels need a 256-CU (8 XCD x 32) device")
        if tuple(c.cond.shape) != (V, B, engine.T, engine.D) or c.t_model.numel() != live or c.t_model.dtype is not torch.int32:
            raise _lib.SynHipError("guided denoiser: cond must be (V, B, 32, 512) and t_model int32 (V B,)")
        st = _lib.current_stream(dev)
        M = n_seq * engine.T
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        xc = x.detach().float().contiguous()
        cond = c.cond.detach().float().contiguous()
        h0 = f32(M, engine.D)
        _lib.check(lib.syn_guide_in_fwd(xc.data_ptr(), B, pm.c.w_in, cond.data_ptr(), pm.c.te, pm.c.n_te, c.t_model.data_ptr(), pm.c.rot_cos, pm.c.rot_sin,
                                        live, n_seq, h0.data_ptr(), st), "syn_guide_in_fwd")
        a = _lib.SynTrainStack()
        hout = f32(M, engine.D)
        a.h_in, a.h_out, a.n_seq, a.drop_path = h0.data_ptr(), hout.data_ptr(), n_seq, None
        sync, xch = training._stack_workspace(dev, n_seq)
        a.sync, a.xch = sync.data_ptr(), xch.data_ptr()
        # the transposed operands of the weight-gradient GEMMs are written by the kernel and read by nobody: one scratch set for all blocks
        scratch = [u8(512 * M * 2), u8(512 * M * 2), u8(512 * M * 2), u8(1024 * M * 2)]
        saves = []
        for l in range(engine.LAYERS):
            for name, _ in _lib.SynLayer._fields_:
                setattr(a.layer[l], name, getattr(pm.c.layer[l], name))
            sv = dict(h_attn=f32(M, 512), mean_attn=f32(M), rstd_attn=f32(M), qkv=f32(M, 1536), xt_ln1=scratch[0], xt_attn=scratch[1],
                      h_mlp=f32(M, 512), mean_mlp=f32(M), rstd_mlp=f32(M), pre=f32(M, 1024), xt_ln2=scratch[2], xt_gelu=scratch[3])
            for k, v in sv.items():
                setattr(a.save[l], k, v.data_ptr())
            saves.append(sv)
        _lib.check(lib.syn_train_stack_fwd(C.byref(a), st), "syn_train_stack_fwd")
        hb = hout.to(torch.bfloat16)
        rows = f32(M, engine.CH)
        _lib.check(lib.syn_linear(hb.data_ptr(), pm.c.w_out, pm.c.b_out, M, engine.CH, engine.D, rows.data_ptr(), st), "syn_linear")
        o = rows[:live * engine.T].view(V, B, engine.T, engine.CH)
        if V == 1:
            out = o[0]
        else:
            out = o[0] * _channel_weights(c.weights, 0, B)
            for v in range(1, V):                                       # fixed order: two runs are bit-equal
                out = out + o[v] * _channel_weights(c.weights, v, B)
        ctx.c, ctx.fwd, ctx.keep, ctx.dims = c, a, (h0, saves, scratch, pm, gp), (B, V, live, n_seq)
        training.check_stack_sync(dev)            # (a device read; a forward whose barrier wait ran out must not hand back its activations)
        return out.permute(0, 2, 1).unsqueeze(2).contiguous()

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        from . import training
        c, a = ctx.c, ctx.fwd
        _, _, _, pm, gp = ctx.keep
        B, V, live, n_seq = ctx.dims
        dev = d_out.device
        st = _lib.current_stream(dev)
        M = n_seq * engine.T
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dr = d_out.detach().float().squeeze(2).permute(0, 2, 1)                     # (B, 32, 1536) rows, a view
        dyb = torch.zeros(M, engine.CH, dtype=torch.bfloat16, device=dev)           # (padding sequences: zero gradient)
        dv = dyb[:live * engine.T].view(V, B, engine.T, engine.CH)
        for v in range(V):
            dv[v].copy_(dr if V == 1 else dr * _channel_weights(c.weights, v, B))
        dh_out = f32(M, engine.D)
        _lib.check(lib.syn_linear(dyb.data_ptr(), gp.WoT.data_ptr(), None, M, engine.D, engine.CH, dh_out.data_ptr(), st), "syn_linear")
        g = _lib.SynTrainStackGrad()
        g.fwd = C.pointer(a)
        dh_in = f32(M, engine.D)
        stash = f32(n_seq, 4, 32 * 512)
        g.dh_out, g.dh_in, g.stash = dh_out.data_ptr(), dh_in.data_ptr(), stash.data_ptr()
        # scratch for what the chain leaves for a weight-gradient launch that never comes: dy^T of the four Linears and the bias / LayerNorm partial sums
        bf = lambda n: torch.empty(n, M, dtype=torch.bfloat16, device=dev)
        scr = dict(dyt_fc2=bf(512), dyt_fc1=bf(1024), dyt_proj=bf(512), dyt_qkv=bf(1536), part=f32(n_seq, 4096))
        for l in range(engine.LAYERS):
            L, F = g.layer_t[l], pm.c.layer[l]
            L.ln1_g, L.ln2_g = F.ln1_g, F.ln2_g
            L.w_qkv, L.w_proj, L.w_fc1, L.w_fc2 = (t.data_ptr() for t in gp.layers[l])
            for k, v in scr.items():
                setattr(g.grad[l], k, v.data_ptr())
        g.first_block, g.last_block = engine.LAYERS - 1, 0
        _lib.check(lib.syn_train_stack_bwd(C.byref(g), st), "syn_train_stack_bwd")
        dx = f32(B, engine.CH, 1, engine.T)
        for v in range(V):                                                           # dx = sum_v dx_v, in variant order on one stream
            _lib.check(lib.syn_guide_in_bwd(dh_in[v * B * engine.T:].data_ptr(), gp.At.data_ptr(), pm.c.rot_cos, pm.c.rot_sin, B, int(v > 0), dx.data_ptr(), st),
                       "syn_guide_in_bwd")
        training.check_stack_sync(dev)            # (a device read: the guided loop is eager, a step waits for its cond_fn anyway)
        return dx, None


def denoise(mdm, x, t_model, conds, weights=None):
    """sum_v w_v model_v(x, t) with a gradient path to x.  x (B, 1536, 1, 32) on the device; t_model (B,) the MODEL's timesteps; conds (V, B, 32, 512)
    from `MDM.variant_conds`; weights (3, V) | (B, 3, V) | None.  Batches of more than 64 sequences run slice by slice."""
    engine._require_cuda(x, "x")
    if mdm.training:
        raise _lib.SynHipError("the guided denoiser is the eval-mode model with frozen weights: call .eval()")
    B, V = x.shape[0], conds.shape[0]
    if tuple(x.shape[1:]) != (engine.CH, 1, engine.T) or conds.shape[1] != B:
        raise _lib.SynHipError(f"guided denoiser: x {tuple(x.shape)} and cond {tuple(conds.shape)} do not describe (B, 1536, 1, 32) latents of one batch")
    if V > 1 and weights is None:
        raise _lib.SynHipError("guided denoiser: several conditioning variants need their weight table")
    t32 = t_model.to(device=x.device, dtype=torch.int32).reshape(-1)
    if t32.numel() != B:
        raise _lib.SynHipError("guided denoiser: one timestep per clip")
    outs = []
    for lo, hi, _, n_seq in plan(B, V):
        w = weights if (weights is None or weights.dim() == 2) else weights[lo:hi]
        c = _Ctx(mdm, conds[:, lo:hi].contiguous(), t32[lo:hi].repeat(V).contiguous(), None if w is None else w.float(), n_seq)
        outs.append(DenoiseFn.apply(x[lo:hi], c))
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


def forward(mdm, x, timesteps, y):
    """`MDM.forward` in eval mode for an x that requires grad: the model's own conditioning variant."""
    with torch.no_grad():
        conds = mdm.variant_conds(y, [mdm.own_variant(y)])
    return denoise(mdm, x, timesteps, conds)


# ---- the update behind cond_fn -------------------------------------------------------------------------------------------------------------------
def update_coefs(tab: dict, kind: str, eta: float, device) -> torch.Tensor:
    """[T][8] fp32 rows of syn_guide_update: kind "ddpm" -> mode 0, "ddim" -> mode 1 (the tables are fp64, rounded once, like `_tab`'s)."""
    f = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
    rows = np.zeros((len(tab["betas"]), 8), dtype=np.float32)
    if kind == "ddpm":
        # sigma as `p_sample` forms it - torch.exp(0.5 * log_variance) in fp32 on the device - so that with a zero gradient the guided step is
        # bit for bit the unguided one
        out = torch.from_numpy(rows).to(device)
        out[:, 0] = torch.from_numpy(f(tab["posterior_variance"])).to(device)
        out[:, 1] = torch.exp(0.5 * torch.from_numpy(f(tab["posterior_log_variance_clipped"])).to(device))
        return out
    ab, abp = f(tab["alphas_cumprod"]), f(tab["alphas_cumprod_prev"])
    sigma = np.float32(eta) * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    rows[:, 0] = np.sqrt(1 - ab)
    rows[:, 1], rows[:, 2] = f(tab["sqrt_recip_alphas_cumprod"]), f(tab["sqrt_recipm1_alphas_cumprod"])
    rows[:, 3], rows[:, 4], rows[:, 5] = np.sqrt(abp), np.sqrt(1 - abp - sigma ** 2), sigma
    return torch.from_numpy(rows).to(device)


def guide_update(kind, a, pred_x0, grad, coef, t_idx, noise=None, seed=None, first_clip=0):
    """One launch of `syn_guide_update` on (B, 1536, 1, 32) fp32 device tensors: kind "ddpm": a = the posterior mean; "ddim": a = x_t.
    noise: a tensor, or None with a seed (the in-library draw), or None without (no noise).  t_idx int32 (B,)."""
    engine._require_cuda(a, "a")
    c = lambda t: None if t is None else t.detach().float().contiguous()
    a_, x0_, g_, nz_ = c(a), c(pred_x0), c(grad), c(noise)
    B = a_.shape[0]
    if tuple(a_.shape[1:]) != (engine.CH, 1, engine.T) or any(t is not None and t.shape != a_.shape for t in (x0_, g_, nz_)) or g_ is None:
        raise _lib.SynHipError("syn_guide_update: every operand is a (B, 1536, 1, 32) tensor")
    if t_idx.dtype is not torch.int32 or t_idx.numel() != B or coef.dim() != 2 or coef.shape[1] != 8:
        raise _lib.SynHipError("syn_guide_update: t_idx int32 (B,), coef [T][8]")
    out = torch.empty_like(a_)
    _lib.check(_lib.load().syn_guide_update(0 if kind == "ddpm" else 1, a_.data_ptr(), _lib.ptr(x0_), g_.data_ptr(), _lib.ptr(nz_),
                                            int(nz_ is None and seed is not None), int(seed or 0) & (2 ** 64 - 1), int(first_clip), coef.data_ptr(),
                                            coef.shape[0], t_idx.data_ptr(), B, out.data_ptr(), _lib.current_stream(a_.device)), "syn_guide_update")
    return out


# ---- the loops ---------------------------------------------------------------------------------------------------------------------------------------
def sample_loop(diff, kind, mdm, plan_fn, shape, noise, clip_denoised, denoised_fn, cond_fn, with_grad, model_kwargs, eta, skip_timesteps,
                init_image, step_noise, seed, first_clip, progress):
    """p_sample_loop_progressive / ddim_sample_loop_progressive with cond_fn on a HIP `MDM` (gaussian_diffusion.py:672-739, 937-1002): eager - the
    user's cond_fn is arbitrary Python - x stays (B, C, 1, T); per step one model evaluation (`DenoiseFn` forward and backward with
    cond_fn_with_grad, the fused inference step without), cond_fn, one `syn_guide_update`.  The in-painting blend, denoised_fn and the clamp are
    applied to the node's output inside the autograd graph, so the gradient cond_fn takes is the gradient of what the sampler uses."""
    dev = next(mdm.parameters()).device
    y = model_kwargs["y"]
    B = shape[0]
    with torch.no_grad():
        p = plan_fn(y)
        V = len(p.variants)
        conds = mdm.variant_conds(y, p.variants)
        W = p.tensor(dev) if V > 1 else None
        img, indices = diff._start(shape, None if noise is None else noise.to(dev), dev, skip_timesteps, init_image)
        img = img.float()
        _, tmap = diff._model_timesteps(dev)
        coef = diff._cached(("guide_coef", kind, float(eta), dev), lambda: update_coefs(diff.tables(), kind, eta, dev))
    noisy = kind == "ddpm" or eta != 0.0
    if noisy and step_noise is None and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())                  # follows torch.manual_seed
    if progress:
        try:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        except ImportError:
            pass
    edit = "inpainting_mask" in y and "inpainted_motion" in y

    def finish(out):
        if edit:
            m = y["inpainting_mask"]
            out = (out * ~m) + (y["inpainted_motion"] * m)
        if denoised_fn is not None:
            out = denoised_fn(out)
        return out.clamp(-1, 1) if clip_denoised else out

    for k, i in enumerate(indices):
        t = torch.full((B,), i, device=dev, dtype=torch.long)
        t_model = torch.full((B,), int(tmap[i]), device=dev, dtype=torch.long)
        if with_grad:
            with torch.enable_grad():
                x = img.detach().requires_grad_()
                x0 = finish(denoise(mdm, x, t_model, conds, W))
                mean, var, logvar = diff.q_posterior_mean_variance(x0, x, t)
                grad = cond_fn(x, t, {"mean": mean, "variance": var, "log_variance": logvar, "pred_xstart": x0}, **model_kwargs)
            x0, mean = x0.detach(), mean.detach()
        else:
            with torch.no_grad():
                x = img
                x0 = finish(mdm.forward_variants(x, t_model, y, p.variants, W))
                mean = diff.q_posterior_mean_variance(x0, x, t)[0] if kind == "ddpm" else None
                grad = diff._wrap_model(cond_fn)(x, diff._scale_timesteps(t), **model_kwargs)
        with torch.no_grad():
            nz = None if (step_noise is None or not noisy) else step_noise[k].to(dev)
            img = guide_update(kind, mean if kind == "ddpm" else x, x0, grad.detach(), coef, t.to(torch.int32), nz,
                               seed if (noisy and nz is None) else None, first_clip)
        yield {"sample": img, "pred_xstart": x0}


# ---- a ready-made objective -------------------------------------------------------------------------------------------------------------------------
def keyframe_cond_fn(target, keep, scale, with_grad, alphas_cumprod=None):
    """Soft keyframes: pull the frames / body parts marked in `keep` (broadcastable to the latent; `longform.keep_mask` builds one) towards `target`.
    with_grad (pass cond_fn_with_grad=True): log p = -scale sum keep (pred_xstart - target)^2, differentiated through the model with respect to x.
    Without: the closed form on x itself, -2 scale keep (x - sqrt(alpha_bar_t) target) - the gradient of -scale sum keep (x - E[x_t | x_0 = target])^2;
    t is the base process's timestep there (respace.py:99-103), alphas_cumprod its table (default: the factory's 1000-step cosine schedule)."""
    if with_grad:
        def cond_fn(x, t, p_mean_var, **kwargs):
            w = keep.to(x)
            logp = -scale * (w * (p_mean_var["pred_xstart"] - target.to(x)) ** 2).sum()
            return torch.autograd.grad(logp, x)[0]
        return cond_fn
    if alphas_cumprod is None:
        from .process import get_named_beta_schedule
        alphas_cumprod = np.cumprod(1.0 - get_named_beta_schedule("cosine", 1000, 1.))
    root = torch.from_numpy(np.sqrt(np.asarray(alphas_cumprod, dtype=np.float64))).float()

    def cond_fn(x, t, **kwargs):
        r = root.to(x.device)[t].view(-1, *([1] * (x.dim() - 1)))
        return -2.0 * scale * keep.to(x) * (x - r * target.to(x))
    return cond_fn
