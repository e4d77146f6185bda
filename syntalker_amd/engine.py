"""Device-side engine: packed weights, workspaces and the fused denoising step / sampling loop.

Layout in HBM (one GPU, everything resident for the whole loop):
    packed weights   bf16 MFMA-fragment order, 19.1 M params = 38 MB          (syn_pack_weight)
    x                token-major fp32 [B*32][1536] + bf16 shadow copy (GEMM operand), updated in place
    cond             fp32 [V*B*32][512], computed once per clip (conditioning.py)
    workspace        h fp32 [R][512]; xn/q/k/o bf16 [R][512]; vt bf16 [R*512]; hid bf16 [R][1024]   (R = V*B*32)
One step = one ``syn_denoise_step`` call = one kernel launch (k_stack for large batches, the persistent k_lat for
small ones), hipGraph-captured and replayed; the timestep enters through two device int32 vectors so the same graph
serves every step, and in the sampling loops those vectors are advanced on the device (`syn_step_advance`), so a loop
iteration is one graph replay and nothing else.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import tape as _tape
from .conditioning import ClipConditioner, fold_input_stage, rotary_tables, time_table

T, CH, D, FF, LAYERS = 32, 1536, 512, 1024, 8


def weights_key(tensors) -> tuple:
    """The staleness key of every cache derived from module weights (folded / packed weights, fragment sets, tables): each tensor's address and
    in-place version.  The writers PyTorch cannot see - `ClipAdam`'s update, a replayed `GraphedTrainStep`, the BatchNorm finalize kernels of a
    training forward - write through raw pointers and bump the versions of exactly what they wrote (`torch.autograd.graph.increment_version`)."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def drop_caches(module) -> dict:
    """`__getstate__` of a module whose derived device-side state lives in `_syn_*` attributes (ctypes structs of raw pointers into ITS packed
    tensors, captured graphs): copy.deepcopy and torch.save take the module as nn.Module defines it, and the copy builds its own caches."""
    return {k: v for k, v in module.__dict__.items() if not k.startswith("_syn_")}


def derived(module, tensors, build) -> dict:
    """The module's cache of what `build` derives from `tensors`: `module.__dict__["_syn_packed"]` while its "ver" is their `weights_key`, else a
    fresh {"ver", "keep": [], "ws": {}} that `build(p)` fills ("keep": the tensors raw pointers refer to, "ws": per-shape workspaces).  It
    replaces the module's cache only once `build` has returned: a `build` that raises leaves none behind."""
    ver = weights_key(tensors)
    p = module.__dict__.get("_syn_packed")
    if p is None or p["ver"] != ver:
        p = {"ver": ver, "keep": [], "ws": {}}
        build(p)
        module.__dict__["_syn_packed"] = p
    return p


def workspace(cache: dict, key, nbytes, device) -> torch.Tensor:
    """The uint8 workspace cached under `key`; a miss on a cache that already holds more than four clears it, then allocates `nbytes` (an int,
    or a callable that gives one and runs on a miss only)."""
    ws = cache.get(key)
    if ws is None:
        if len(cache) > 4:
            cache.clear()
        ws = cache[key] = torch.empty(nbytes() if callable(nbytes) else nbytes, dtype=torch.uint8, device=device)
    return ws


def _require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise _lib.SynHipError(
            f"{what} is on {t.device}: the denoising path runs only on the MI355X HIP kernels "
            "(no CPU fallback). Move the model and inputs to a cuda device.")


def seq_pass_clips(n_variants: int, device) -> int:
    """Clips one full pass of the wave-per-sequence kernel takes: a workgroup per CU, its four waves = the variants of
    4 // V clips (V = 3 leaves a wave idle).  0 where that kernel does not apply."""
    device = torch.device(device)
    if device.type != "cuda" or not 1 <= n_variants <= 4:
        return 0
    return torch.cuda.get_device_properties(device).multi_processor_count * (4 // n_variants)


def plan_slices(n_clips: int, n_variants: int, device) -> list[tuple[int, int]]:
    """Contiguous clip ranges a batch is run as, one after the other (sequences never interact, noise is keyed by the
    global clip index: the result is the unsliced one).  Both whole-step kernels quantise to passes over the CUs - `k_seq`
    to passes of P = 1024 / V clips, `k_stack` to passes of 512 sequences - and `k_seq`'s pass is the cheaper per clip only
    when it is more than half full, so the library picks `k_stack` for q P + r clips with 0 < r <= P / 2 (1025-1536, ...):
    three `k_stack` passes where one `k_seq` pass and the best kernel for the r clips left do
    (1536 clips: 1.95 ms per step as one batch, 1.13 + 0.64 ms as 1024 + 512; `profiles/r03_diag_batch_sweep.txt`)."""
    P = seq_pass_clips(n_variants, device)
    if P == 0 or n_clips <= P or n_variants == 3:
        return [(0, n_clips)]
    r = n_clips % P
    if r == 0 or 2 * r > P:
        return [(0, n_clips)]
    return [(0, n_clips - r), (n_clips - r, n_clips)]


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """fp32 (n, k) nn.Linear weight -> packed bf16 MFMA fragments (uint8 view of n*k*2 bytes)."""
    _require_cuda(w, "weight")
    w = w.detach().float().contiguous()
    n, k = w.shape
    out = torch.empty(n * k * 2, dtype=torch.uint8, device=w.device)
    _lib.check(_lib.load().syn_pack_weight(w.data_ptr(), n, k, out.data_ptr(), _lib.current_stream(w.device)), "syn_pack_weight")
    return out


class PackedModel:
    """Folded + packed, step-resident view of an MDM state_dict (inference; eval-mode semantics)."""

    def __init__(self, sd: dict, variant: str, use_style: bool, n_te: int = 1000):
        dev = sd["input_process2.weight"].device
        _require_cuda(sd["input_process2.weight"], "model")
        self.device, self.variant, self.use_style = dev, variant, use_style
        f32 = lambda t: t.detach().float().contiguous()
        folded = fold_input_stage(sd, use_style)
        self.folded = folded
        self.keep = []                       # every tensor the C struct points at
        m = _lib.SynModel()

        def hold(t):
            self.keep.append(t)
            return t.data_ptr()

        m.w_in = hold(pack_weight(folded["A"].float()))
        self.te = time_table(sd, folded["W2a"], n_te)
        m.te, m.n_te = hold(self.te), n_te
        rc, rs = rotary_tables(f32(sd["rel_pos.inv_freq"]), T)
        m.rot_cos, m.rot_sin = hold(rc), hold(rs)
        for i in range(LAYERS):
            p, L = f"mytimmblocks.{i}.", m.layer[i]
            L.ln1_g, L.ln1_b = hold(f32(sd[p + "norm1.weight"])), hold(f32(sd[p + "norm1.bias"]))
            L.w_qkv = hold(pack_weight(sd[p + "attn.qkv.weight"]))
            L.w_proj, L.b_proj = hold(pack_weight(sd[p + "attn.proj.weight"])), hold(f32(sd[p + "attn.proj.bias"]))
            L.ln2_g, L.ln2_b = hold(f32(sd[p + "norm2.weight"])), hold(f32(sd[p + "norm2.bias"]))
            L.w_fc1, L.b_fc1 = hold(pack_weight(sd[p + "mlp.fc1.weight"])), hold(f32(sd[p + "mlp.fc1.bias"]))
            L.w_fc2, L.b_fc2 = hold(pack_weight(sd[p + "mlp.fc2.weight"])), hold(f32(sd[p + "mlp.fc2.bias"]))
        m.w_out = hold(pack_weight(sd["output_process.poseFinal.weight"]))
        m.b_out = hold(f32(sd["output_process.poseFinal.bias"]))
        # the same weights as one tape of MFMA fragments in consumption order: the wave-per-sequence kernel (large batches)
        tp, tb = _tape.build_tape(sd, folded["A"])
        m.tape, m.tape_bias, m.tape_chunks = hold(tp), hold(tb), _tape.TAPE_FRAGS // _tape.CHUNK_FRAGS   # (+ LOOK_CHUNKS repeated chunks behind them)
        self.c = m
        self.conditioner = ClipConditioner({k: (v.detach() if torch.is_tensor(v) else v) for k, v in sd.items()},
                                           folded, variant, use_style)
        torch.cuda.current_stream(dev).synchronize()


class StepBuffers:
    """State + workspace for B clips x V conditioning variants; owns the syn_step struct."""

    def __init__(self, B: int, V: int, device, want_x0: bool = False, m_tile: int = 0, layer_mode: int = 0, edit: bool = False,
                 plms: bool = False):
        """``edit``: the buffers carry an in-painting mask and motion (`load_edit`) and every step blends them in
        (`syn_denoise_step_edit`).  ``plms``: they also carry what the multistep sampler keeps between steps (`PlmsLoop`): a second
        latent the steps ping-pong with, the ring of three earlier noise estimates, and pred_x0; H, the weighted history a step
        injects, is the `noise` operand."""
        self.B, self.V = B, V
        want_x0 = want_x0 or plms
        # latent layout: fragment order when the wave-per-sequence kernel runs the steps (the library's choice for large
        # single-variant batches, or pinned with layer_mode 5), token-major otherwise - and always with an edit, which that kernel
        # does not take
        lib = _lib.load()
        self.fragment = bool(not edit and (layer_mode == 5 or (layer_mode == 0 and m_tile == 0 and lib.syn_prefers_fragment_order(B, V))))
        R, Mb = V * B * T, B * T
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=device)
        bf = torch.bfloat16
        self.x, self.xb = e(Mb, CH), e(Mb, CH, dt=bf)
        self.noise = e(Mb, CH)
        self.rng = torch.zeros(2, dtype=torch.int64, device=device)     # {seed, first_clip} of the in-epilogue generator
        self.x0 = e(Mb, CH) if want_x0 else None
        self.cond = e(R, D)
        self.t_model = torch.zeros(V * B, dtype=torch.int32, device=device)
        self.t_coef = torch.zeros(B, dtype=torch.int32, device=device)
        self.cfg_w = e(B, 3, V) if V > 1 else None      # one weight table per clip (`copy_` broadcasts a (3, V) table over the clips)
        self.h = e(R, D)
        self.xn, self.q, self.k, self.o = e(R, D, dt=bf), e(R, D, dt=bf), e(R, D, dt=bf), e(R, D, dt=bf)
        self.vt, self.hid = e(R * D, dt=bf), e(R, FF, dt=bf)
        self.hc = e(3, Mb, D, dt=bf) if V > 1 else None
        self.sync = torch.zeros(320, dtype=torch.int32, device=device)   # small-batch path: barrier counters + error flag
        s = _lib.SynStep()
        s.n_clips, s.n_variants, s.m_tile = B, V, m_tile
        # 0 auto, by plan_step (csrc/syn_step_plan.inc): the small-batch kernel while an XCD holds at most 4 sequences, unless the whole-step
        # kernel's split tiles apply at 9..128 sequences (with the buffers below: small-batch up to 8 sequences, split tiles to 128, whole
        # tiles beyond); 4 / 3 / 5 pin one of the kernels; 1 = five kernels per block (the restatement the whole-step kernel is checked
        # against bit for bit)
        s.reserved = layer_mode
        s.cond, s.t_model, s.cfg_w = self.cond.data_ptr(), self.t_model.data_ptr(), _lib.ptr(self.cfg_w)
        s.x_t, s.x_t_bf16, s.noise = self.x.data_ptr(), self.xb.data_ptr(), self.noise.data_ptr()
        s.t_coef = self.t_coef.data_ptr()
        s.rng = None
        s.x_next, s.x_next_bf16, s.pred_x0 = self.x.data_ptr(), self.xb.data_ptr(), _lib.ptr(self.x0)
        s.ws_h, s.ws_xn, s.ws_q, s.ws_k = self.h.data_ptr(), self.xn.data_ptr(), self.q.data_ptr(), self.k.data_ptr()
        s.ws_vt, s.ws_o, s.ws_hid, s.ws_hc = self.vt.data_ptr(), self.o.data_ptr(), self.hid.data_ptr(), _lib.ptr(self.hc)
        s.ws_sync = self.sync.data_ptr()
        # guided small batches: per-variant x0_hat, so that the variants of a clip can run on different XCDs
        self.x0v = e(R, CH) if (V > 1 and B * V <= 32) else None
        s.ws_x0v = _lib.ptr(self.x0v)
        # 9..128 sequences: exchange slots for the whole-step kernel's tensor-parallel mode (a tile split over 2 / 4 CUs)
        self.xch = e(V * B + 1, 8, 32 * D) if 8 < V * B <= 256 else None      # (129..256 sequences: 64-row tiles split in two, the same bytes per sequence)
        s.ws_xch = _lib.ptr(self.xch)
        s.x_fragment_order = int(self.fragment)
        s.cfg_w_clip_stride = 3 * V if V > 1 else 0
        self.c = s
        # in-painting: keep (nonzero = take `known` for x0) and known, token-major like x; captured graphs hold these pointers,
        # so a later loop refills them (`load_edit`)
        self.keep = torch.zeros(Mb, CH, dtype=torch.uint8, device=device) if edit else None
        self.known = torch.zeros(Mb, CH, dtype=torch.float32, device=device) if edit else None
        self.edit = None
        if edit:
            self.edit = _lib.SynEdit()
            self.edit.keep, self.edit.known = self.keep.data_ptr(), self.known.data_ptr()
        self.plms = plms
        if plms:
            z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)
            self.x2, self.xb2, self.ring = z(Mb, CH), z(Mb, CH, dt=bf), z(3, Mb, CH)
            for t in (self.x, self.xb, self.noise, self.x0):       # (the capture's warm-up launch runs on them as they stand)
                t.zero_()

    # layout ------------------------------------------------------------------------------------
    def _import(self, src: torch.Tensor, dst_f32, dst_bf16):
        lib = _lib.load()
        fn, name = (lib.syn_x_to_fragment, "syn_x_to_fragment") if self.fragment else (lib.syn_to_token_major, "syn_to_token_major")
        _lib.check(fn(src.data_ptr(), self.B, dst_f32.data_ptr(), _lib.ptr(dst_bf16), _lib.current_stream(src.device)), name)

    def load_x(self, x_bct: torch.Tensor):
        """(B,1536,1,32) fp32 -> x in the step kernel's layout + bf16 shadow."""
        self._import(x_bct.detach().float().contiguous(), self.x, self.xb)

    def load_noise(self, eps_bct: torch.Tensor):
        self._import(eps_bct.detach().float().contiguous(), self.noise, None)

    def load_edit(self, mask_bct: torch.Tensor, motion_bct: torch.Tensor):
        """(B,1536,1,32) bool mask and float motion of an in-painting call -> keep / known (buffers built with edit=True)."""
        if self.edit is None:
            raise ValueError("these StepBuffers carry no edit (edit=True)")
        shape = (self.B, CH, 1, T)
        if tuple(mask_bct.shape) != shape or tuple(motion_bct.shape) != shape or mask_bct.dtype is not torch.bool:
            raise ValueError(f"load_edit takes a bool mask and a motion of shape {shape}")
        dev = self.known.device
        motion = motion_bct.detach().to(dev, torch.float32).contiguous()
        _lib.check(_lib.load().syn_to_token_major(motion.data_ptr(), self.B, self.known.data_ptr(), None, _lib.current_stream(dev)),
                   "syn_to_token_major")
        self.keep.view(self.B, T, CH).copy_(mask_bct.detach().to(dev)[:, :, 0, :].permute(0, 2, 1))

    def set_rng(self, seed: int, first_clip: int = 0):
        """Key of the in-epilogue generator for the whole loop; the per-step stream id is the clip's t_coef."""
        self.rng.copy_(torch.tensor([seed, first_clip], dtype=torch.int64))

    def draw_noise(self, seed: int, step: int, first_clip: int = 0):
        """N(0,1) keyed by (seed, step, global element index): identical for any sharding of the batch."""
        n = self.B * T * CH
        dst = torch.empty_like(self.noise) if self.fragment else self.noise       # the generator's index space is token-major
        _lib.check(_lib.load().syn_randn(dst.data_ptr(), n, seed, step, first_clip * T * CH,
                                         _lib.current_stream(dst.device)), "syn_randn")
        if self.fragment:
            self.noise.view(-1).copy_(_tape.to_fragment_order(dst.view(self.B, T, CH)).view(-1))

    def check_sync(self):
        """The small-batch kernel's group barrier is bounded; a wait that ran out leaves a sticky flag."""
        flag = int(self.sync[256].item())
        if flag:
            self.sync.zero_()
            raise _lib.SynHipError(f"small-batch step kernel: group barrier wait ran out (flag {flag}); "
                                   "is another kernel occupying CUs of this device?")

    def read(self, src: torch.Tensor) -> torch.Tensor:
        self.check_sync()
        out = torch.empty(self.B, CH, 1, T, dtype=torch.float32, device=src.device)
        lib = _lib.load()
        fn, name = (lib.syn_x_from_fragment, "syn_x_from_fragment") if self.fragment else (lib.syn_from_token_major, "syn_from_token_major")
        _lib.check(fn(src.data_ptr(), self.B, out.data_ptr(), _lib.current_stream(src.device)), name)
        return out


def run_step(pm: PackedModel, sb: StepBuffers, coef: torch.Tensor, use_noise: bool = True, fused_rng: bool = False, steps: int = 1):
    """use_noise + fused_rng: the output GEMM's epilogue draws the noise, keyed by sb.rng = {seed, first_clip} and t_coef;
    use_noise only: the noise is read from sb.noise (injected or drawn by draw_noise)."""
    sb.c.coef = coef.data_ptr()
    sb.c.noise = sb.noise.data_ptr() if (use_noise and not fused_rng) else None
    sb.c.rng = sb.rng.data_ptr() if (use_noise and fused_rng) else None
    if steps > 1:        # sb.c.t_model / t_coef point at [steps][n] rows (syn_steps_advance fills them)
        if use_noise and not fused_rng:
            raise ValueError("injected noise is per step: multi-step launches draw theirs (fused_rng) or run without")
        if sb.edit is not None:
            # `syn_denoise_steps` takes no edit: its token-major form here, one `syn_denoise_step_edit` per row of the [steps][n] int32
            # timestep tables (row stride = 4 bytes x the vector's length, the strides `syn_denoise_steps` is given in elements)
            tm, tc = sb.c.t_model, sb.c.t_coef
            try:
                for j in range(steps):
                    sb.c.t_model, sb.c.t_coef = tm + 4 * j * sb.t_model.numel(), tc + 4 * j * sb.t_coef.numel()
                    _lib.check(_lib.load().syn_denoise_step_edit(C.byref(pm.c), C.byref(sb.c), C.byref(sb.edit),
                                                                 _lib.current_stream(pm.device)), "syn_denoise_step_edit")
            finally:
                sb.c.t_model, sb.c.t_coef = tm, tc
            return
        _lib.check(_lib.load().syn_denoise_steps(C.byref(pm.c), C.byref(sb.c), steps, sb.t_model.numel(), sb.t_coef.numel(),
                                                 _lib.current_stream(pm.device)), "syn_denoise_steps")
        return
    if sb.edit is not None:
        _lib.check(_lib.load().syn_denoise_step_edit(C.byref(pm.c), C.byref(sb.c), C.byref(sb.edit), _lib.current_stream(pm.device)),
                   "syn_denoise_step_edit")
        return
    _lib.check(_lib.load().syn_denoise_step(C.byref(pm.c), C.byref(sb.c), _lib.current_stream(pm.device)), "syn_denoise_step")


class StepGraph:
    """hipGraph of one step; replays read the timestep from sb.t_model / sb.t_coef (device memory).
    With ``scheduled=True`` the graph starts with `syn_step_advance`: the timestep vectors come from a device-resident
    schedule (`set_schedule`) and a loop iteration is nothing but `replay()`."""

    MAX_STEPS = 1024

    def __init__(self, pm: PackedModel, sb: StepBuffers, coef: torch.Tensor, use_noise: bool = True, fused_rng: bool = False,
                 scheduled: bool = False, steps: int = 1):
        """``steps`` > 1 (scheduled graphs only): that many consecutive steps per replay - no launch gaps between them."""
        assert steps == 1 or scheduled
        self.pm, self.sb, self.coef, self.scheduled, self.steps = pm, sb, coef, scheduled, steps
        if scheduled:
            self.sched = torch.zeros(self.MAX_STEPS, 2, dtype=torch.int32, device=pm.device)
            self.counter = torch.zeros(1, dtype=torch.int32, device=pm.device)
        if steps > 1:
            self.tm_rows = torch.zeros(steps, sb.t_model.numel(), dtype=torch.int32, device=pm.device)
            self.tc_rows = torch.zeros(steps, sb.t_coef.numel(), dtype=torch.int32, device=pm.device)
        if scheduled:
            # The warm-up launch below reads the timestep vectors as they stand, and a cached StepBuffers may carry the indices of
            # an earlier loop over a LONGER coefficient table (p_sample_loop's 1000 rows, then ddim_sample_loop's 50: row 999 of a
            # 50-row table is an out-of-bounds read).  A scheduled graph overwrites them from its schedule before every step anyway.
            sb.t_model.zero_(); sb.t_coef.zero_()
        side = torch.cuda.Stream(device=pm.device)
        side.wait_stream(torch.cuda.current_stream(pm.device))
        with torch.cuda.stream(side):          # warm-up launch outside capture (module load, etc.), the same launch(es) as captured
            x_save, xb_save = sb.x.clone(), sb.xb.clone()
            if steps > 1:
                try:
                    sb.c.t_model, sb.c.t_coef = self.tm_rows.data_ptr(), self.tc_rows.data_ptr()
                    run_step(pm, sb, coef, use_noise, fused_rng, steps=steps)
                finally:
                    sb.c.t_model, sb.c.t_coef = sb.t_model.data_ptr(), sb.t_coef.data_ptr()
            else:
                run_step(pm, sb, coef, use_noise, fused_rng)
            sb.x.copy_(x_save); sb.xb.copy_(xb_save)
        torch.cuda.current_stream(pm.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            if steps > 1:
                # one schedule kernel per replay: it fills a row of timestep vectors per captured step, and every captured
                # launch points at its own row (same-box A/B at B = 1: 160.5 -> 158.3 us per step)
                _lib.check(_lib.load().syn_steps_advance(self.sched.data_ptr(), self.counter.data_ptr(), self.tm_rows.data_ptr(),
                                                         sb.t_model.numel(), self.tc_rows.data_ptr(), sb.t_coef.numel(), steps,
                                                         _lib.current_stream(pm.device)), "syn_steps_advance")
                # syn_denoise_steps: `steps` launches for token-major latents; ONE persistent launch for fragment-order latents
                # (every workgroup takes its sequences through all the steps, the workgroups drift out of phase)
                try:
                    sb.c.t_model, sb.c.t_coef = self.tm_rows.data_ptr(), self.tc_rows.data_ptr()
                    run_step(pm, sb, coef, use_noise, fused_rng, steps=steps)
                finally:
                    sb.c.t_model, sb.c.t_coef = sb.t_model.data_ptr(), sb.t_coef.data_ptr()
            else:
                if scheduled:
                    _lib.check(_lib.load().syn_step_advance(self.sched.data_ptr(), self.counter.data_ptr(), sb.t_model.data_ptr(),
                                                            sb.t_model.numel(), sb.t_coef.data_ptr(), sb.t_coef.numel(),
                                                            _lib.current_stream(pm.device)), "syn_step_advance")
                run_step(pm, sb, coef, use_noise, fused_rng)
        # The first launch of an instantiated hipGraph uploads it to the device (measured at 1024 clips: the first 10-step replay takes
        # 12.6 ms, the following ones 11.1 - the stream idles ~1.5 ms while the host sets the launch up).  That belongs to building the
        # graph, like the capture: one replay here, on a snapshot of the latent (scheduled graphs read schedule row 0; the counter is
        # put back).
        x_save, xb_save = sb.x.clone(), sb.xb.clone()
        tm_save, tc_save = sb.t_model.clone(), sb.t_coef.clone()
        self.graph.replay()
        sb.x.copy_(x_save); sb.xb.copy_(xb_save); sb.t_model.copy_(tm_save); sb.t_coef.copy_(tc_save)
        if scheduled:
            self.counter.zero_()

    def set_schedule(self, t_coef_rows, t_model_rows):
        """Rows of the coefficient table and original timesteps of the coming replays, in order (<= MAX_STEPS)."""
        n = len(t_coef_rows)
        if n > self.MAX_STEPS:
            raise ValueError(f"schedule of {n} steps exceeds {self.MAX_STEPS}")
        host = torch.tensor(list(zip(t_coef_rows, t_model_rows)), dtype=torch.int32).reshape(-1, 2)
        self.sched[:n].copy_(host)
        self.counter.zero_()

    def copy_schedule_from(self, other: "StepGraph"):
        """Continue `other`'s schedule where it stands (a multi-step graph handing over to the single-step one)."""
        self.sched.copy_(other.sched)
        self.counter.copy_(other.counter)

    def replay(self):
        self.graph.replay()


# ---------------------------------------------------------------------------------------------
def posterior_coefs(tab: dict, device) -> torch.Tensor:
    """DDPM ancestral step as x_next = c0*x0 + c1*x_t + sigma*eps (gaussian_diffusion.py:255-277, 546-556)."""
    n = len(tab["betas"])
    c = np.zeros((n, 4), np.float64)
    c[:, 0], c[:, 1] = tab["posterior_mean_coef1"], tab["posterior_mean_coef2"]
    c[:, 2] = np.exp(0.5 * tab["posterior_log_variance_clipped"])
    c[0, 2] = 0.0                                         # nonzero_mask: no noise at t == 0
    return torch.tensor(c, dtype=torch.float32, device=device)


def ddim_coefs(tab: dict, eta: float, device) -> torch.Tensor:
    """DDIM step in the same linear form (gaussian_diffusion.py:771-791):
         eps_hat = (sqrt(1/ab) x_t - x0) / sqrt(1/ab - 1)
         x_next  = sqrt(ab_prev) x0 + sqrt(1 - ab_prev - sigma^2) eps_hat + sigma eps."""
    ab, abp = tab["alphas_cumprod"], tab["alphas_cumprod_prev"]
    sigma = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    dirc = np.sqrt(1 - abp - sigma ** 2)
    r, rm1 = tab["sqrt_recip_alphas_cumprod"], tab["sqrt_recipm1_alphas_cumprod"]
    c = np.zeros((len(ab), 4), np.float64)
    c[:, 0] = np.sqrt(abp) - dirc / rm1
    c[:, 1] = dirc * r / rm1
    c[:, 2] = sigma
    c[0, 2] = 0.0
    return torch.tensor(c, dtype=torch.float32, device=device)


def identity_coefs(device) -> torch.Tensor:
    """x_next = x0: a bare model evaluation (MDM.forward)."""
    return torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device=device)


# ---- pseudo linear multistep (gaussian_diffusion.py:1004-1086) -------------------------------------------------------------------------
AB_WEIGHTS = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}     # Adams-Bashforth


def plms_coefs(tab: dict, order: int, n_steps: int) -> dict:
    """The PLMS loop over timesteps n_steps - 1 .. 0 as n_steps + 1 launches of the step kernel, each followed by `syn_plms_update`, in fp64.

    With r, m = sqrt_recip / sqrt_recipm1_alphas_cumprod[t], p, q = sqrt(ab_prev[t]), sqrt(1 - ab_prev[t]), beta = q - p m and a_0..a_3 the
    Adams-Bashforth weights of the step's current order, the reference's x_next = p (r x_t - m eps') + q eps', eps' = a_0 eps + sum a_k e_k,
    eps = (r x_t - x0_hat) / m, is
        x_next = c_x0 x0_hat + c_xt x_t + beta H,   c_x0 = -beta a_0 / m,   c_xt = r (p + beta a_0 / m),   H = sum_{k >= 1} a_k e_k
    (a_0 = 1, H = 0: the DDIM eta = 0 row; t == 0: (1, 0, 0), the sample is pred_xstart).  The first step, two model calls (:1054-1061):
    launch 0 is the DDIM row at t into the other latent, its update keeps e_1 and leaves H = p r x_T + beta e_1 / 2; launch 1 evaluates the
    model there at t - 1 with the row (-beta / (2 m'), beta r' / (2 m'), 1), i.e. x_next = H + beta e_2 / 2, and e_2 is not kept.

    Rows by launch: "coef" (c_x0, c_xt, sigma, 0); "hist" (r, 1 / m, h_x, w_new, w[0..2]) and "store" as `syn_plms_row`; "t" the timestep of the
    launch's model call; "order" the current order of its step (1: the Euler start).  Estimate j (0: e_1 of the start, j: step j's) lives in
    ring slot j % 3."""
    if order not in (2, 3, 4):
        raise ValueError("order is 2, 3 or 4")
    n = int(n_steps)
    if n < 2 or n > len(tab["betas"]):
        raise ValueError(f"a PLMS loop takes 2 .. {len(tab['betas'])} steps (its first step calls the model at t and t - 1)")
    r_, m_ = np.asarray(tab["sqrt_recip_alphas_cumprod"], np.float64), np.asarray(tab["sqrt_recipm1_alphas_cumprod"], np.float64)
    abp = np.asarray(tab["alphas_cumprod_prev"], np.float64)
    p_, q_ = np.sqrt(abp), np.sqrt(1.0 - abp)
    beta_ = q_ - p_ * m_
    L = n + 1
    coef, hist, store = np.zeros((L, 4), np.float64), np.zeros((L, 7), np.float64), np.full(L, -1, np.int64)
    ts, orders = np.zeros(L, np.int64), np.ones(L, np.int64)
    t0 = n - 1
    r, m, p, q, beta = r_[t0], m_[t0], p_[t0], q_[t0], beta_[t0]
    ts[0], ts[1] = t0, t0 - 1
    coef[0] = (p - q / m, q * r / m, 0.0, 0.0)
    hist[0, :4], store[0] = (r, 1.0 / m, p * r, beta / 2), 0
    coef[1] = (-beta / (2 * m_[t0 - 1]), beta * r_[t0 - 1] / (2 * m_[t0 - 1]), 1.0, 0.0)
    hist[1, :2] = (r_[t0 - 1], 1.0 / m_[t0 - 1])

    def history(row, j_next, newest_in_register):
        """H of step j_next into `row`: estimate j_next - k has weight a_k; the newest one may still be in the update's registers."""
        if j_next > n - 1 or n - 1 - j_next == 0:            # nothing follows, or the t == 0 step: sigma = 0
            return
        a = AB_WEIGHTS[min(order, j_next + 1)]
        for k in range(1, len(a)):
            if k == 1 and newest_in_register:
                hist[row, 3] = a[k]
            else:
                hist[row, 4 + (j_next - k) % 3] = a[k]
    history(1, 1, False)
    for j in range(1, n):
        t, row = n - 1 - j, j + 1
        ts[row], orders[row] = t, min(order, j + 1)
        a0 = AB_WEIGHTS[orders[row]][0]
        coef[row] = (1.0, 0.0, 0.0, 0.0) if t == 0 else (-beta_[t] * a0 / m_[t], r_[t] * (p_[t] + beta_[t] * a0 / m_[t]), beta_[t], 0.0)
        hist[row, :2] = (r_[t], 1.0 / m_[t])
        history(row, j + 1, True)
        if order > 2 and j + 2 <= n - 2:          # read again after the next step (which takes it from this update's registers)
            store[row] = j % 3
    return {"coef": coef, "hist": hist, "store": store, "t": ts, "order": orders}


class PlmsLoop:
    """The captured graphs of PLMS loops over one StepBuffers (plms=True): every launch is `syn_step_advance`, the step, `syn_plms_update`.
    The step must not overwrite the x_t its update reads, so consecutive steps ping-pong between sb.x and sb.x2 (no bytes moved; the other
    choice, the update moving the result into place, is 10 more bytes per element) - one graph per direction, "start" for the two launches of
    the first step, and `MULTI` steps in one graph for stretches without hooks (an even count: it ends on the latent it started from).
    Coefficient and history tables sit in fixed device buffers (`load`), so the graphs outlive a loop and serve any order and step count."""

    MAX_ROWS, MULTI = StepGraph.MAX_STEPS, 10

    def __init__(self, pm: PackedModel, sb: StepBuffers):
        assert sb.plms
        dev = pm.device
        self.pm, self.sb = pm, sb
        self.sched = torch.zeros(self.MAX_ROWS, 2, dtype=torch.int32, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.coef = torch.zeros(self.MAX_ROWS, 4, dtype=torch.float32, device=dev)
        self.rows = torch.zeros(self.MAX_ROWS, C.sizeof(_lib.SynPlmsRow), dtype=torch.uint8, device=dev)
        self.tm_rows = torch.zeros(self.MULTI, sb.t_model.numel(), dtype=torch.int32, device=dev)
        self.tc_rows = torch.zeros(self.MULTI, sb.t_coef.numel(), dtype=torch.int32, device=dev)
        self.lat = ((sb.x, sb.xb), (sb.x2, sb.xb2))
        self.graphs, self.loaded = {}, None
        # warm-up launches outside capture (module load etc.), on the zeroed tables: row 0 keeps an all-zero estimate in ring slot 0
        sb.t_model.zero_(); sb.t_coef.zero_()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._issue("start")
        torch.cuda.current_stream(dev).wait_stream(side)
        self.counter.zero_()

    def _step(self, parity: int, back: int, tm_ptr: int, tc_ptr: int, want_x0: bool = True):
        """One step from latent `parity` into the other, then the history update on what it read."""
        sb, c = self.sb, self.sb.c
        saved = {f: getattr(c, f) for f in ("x_t", "x_t_bf16", "x_next", "x_next_bf16", "t_model", "t_coef", "pred_x0")}
        (x, xb), (y, yb) = self.lat[parity], self.lat[1 - parity]
        try:
            c.x_t, c.x_t_bf16, c.x_next, c.x_next_bf16 = x.data_ptr(), xb.data_ptr(), y.data_ptr(), yb.data_ptr()
            c.t_model, c.t_coef = tm_ptr, tc_ptr
            c.pred_x0 = sb.x0.data_ptr() if want_x0 else None
            run_step(self.pm, sb, self.coef, use_noise=True, fused_rng=False)
        finally:
            for f, v in saved.items():
                setattr(c, f, v)
        _lib.check(_lib.load().syn_plms_update(self.rows.data_ptr(), self.MAX_ROWS, self.counter.data_ptr(), back, x.data_ptr(),
                                               sb.x0.data_ptr(), sb.ring.data_ptr(), sb.noise.data_ptr(), x.numel(),
                                               _lib.current_stream(self.pm.device)), "syn_plms_update")

    def _issue(self, kind):
        sb, lib, stream = self.sb, _lib.load(), _lib.current_stream(self.pm.device)
        n_tm, n_tc = sb.t_model.numel(), sb.t_coef.numel()
        advance = lambda: _lib.check(lib.syn_step_advance(self.sched.data_ptr(), self.counter.data_ptr(), sb.t_model.data_ptr(), n_tm,
                                                          sb.t_coef.data_ptr(), n_tc, stream), "syn_step_advance")
        if kind == "start":
            # the second model call's x0_hat is not the step's pred_xstart (:1086) and its estimate is not kept: pred_x0 = NULL there
            advance(); self._step(0, 1, sb.t_model.data_ptr(), sb.t_coef.data_ptr())
            advance(); self._step(1, 1, sb.t_model.data_ptr(), sb.t_coef.data_ptr(), want_x0=False)
        elif kind == "multi":
            _lib.check(lib.syn_steps_advance(self.sched.data_ptr(), self.counter.data_ptr(), self.tm_rows.data_ptr(), n_tm,
                                             self.tc_rows.data_ptr(), n_tc, self.MULTI, stream), "syn_steps_advance")
            for j in range(self.MULTI):
                self._step(j % 2, self.MULTI - j, self.tm_rows[j].data_ptr(), self.tc_rows[j].data_ptr())
        else:
            advance(); self._step(kind, 1, sb.t_model.data_ptr(), sb.t_coef.data_ptr())

    def issue(self, kind, eager: bool = False):
        """"start", "multi", or the parity 0 / 1 of a single step: a replay of its graph (captured at first use), or the same launches eagerly."""
        if eager:
            return self._issue(kind)
        g = self.graphs.get(kind)
        if g is None:
            g = self.graphs[kind] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._issue(kind)
        g.replay()

    def load(self, key, make, t_model_of):
        """Tables of the coming loop (`make()` -> `plms_coefs`), launch schedule from the start; `t_model_of`: timestep -> the model's."""
        if self.loaded != key:
            tab = make()
            L = len(tab["store"])
            if L > self.MAX_ROWS:
                raise ValueError(f"a PLMS loop of {L - 1} steps exceeds {self.MAX_ROWS - 1}")
            rows = np.zeros(L, dtype=[("f", np.float32, 7), ("store", np.int32)])
            rows["f"], rows["store"] = tab["hist"], tab["store"]
            self.rows[:L].copy_(torch.from_numpy(rows.view(np.uint8).reshape(L, -1)))
            self.coef[:L].copy_(torch.from_numpy(tab["coef"].astype(np.float32)))
            sched = np.stack([np.arange(L), [t_model_of(int(t)) for t in tab["t"]]], 1).astype(np.int32)
            self.sched[:L].copy_(torch.from_numpy(sched))
            self.loaded, self.n_launches = key, L
        self.counter.zero_()
        self.sb.noise.zero_()                 # launch 0 has sigma = 0, but 0 * H must be 0

    def run(self, each=None, eager: bool = False) -> torch.Tensor:
        """The loaded loop on the latent in sb.x; returns the fp32 latent that holds the result (sb.x or sb.x2).  `each(k, x)` after step k."""
        n = self.n_launches - 1
        self.issue("start", eager)
        if each is not None:
            each(0, self.sb.x)
        j = 1
        while each is None and n - j >= self.MULTI:
            self.issue("multi", eager)
            j += self.MULTI
        while j < n:
            parity = (j - 1) % 2
            self.issue(parity, eager)
            if each is not None:
                each(j, self.lat[1 - parity][0])
            j += 1
        return self.lat[(n - 1) % 2][0]


# ---- the variational bound per timestep (gaussian_diffusion.py:1201-1234, 1548-1603) ---------------------------------------------------
BPD_ROW = np.dtype([("c1", np.float32), ("c2", np.float32), ("log_var", np.float32), ("r", np.float32), ("inv_m", np.float32),
                    ("first", np.int32)])                                           # include/syn_hip.h syn_bpd_row


def bpd_rows(tab: dict) -> np.ndarray:
    """One `syn_bpd_row` per timestep of the process, from the fp64 tables: the posterior mean's coefficients and log-variance
    (FIXED_SMALL: q's posterior and p share it, so the KL is 0.5 exp(-log_var) (c1 (x0 - x0_hat))^2), r and 1 / m of
    eps = (r x_t - x0_hat) / m, and `first` at t == 0, where the term is the decoder's discretised log-likelihood."""
    rows = np.zeros(len(tab["betas"]), BPD_ROW)
    rows["c1"], rows["c2"] = tab["posterior_mean_coef1"], tab["posterior_mean_coef2"]
    rows["log_var"] = tab["posterior_log_variance_clipped"]
    rows["r"] = tab["sqrt_recip_alphas_cumprod"]
    rows["inv_m"] = 1.0 / np.asarray(tab["sqrt_recipm1_alphas_cumprod"], np.float64)
    rows["first"][0] = 1
    return rows


def bpd_chunks(n_pairs: int, n_variants: int, device, chunk=None) -> list[tuple[int, int]]:
    """Ranges of the (clip, timestep) pairs a call runs as, one after the other.  ``chunk`` pairs each when given; else full passes of the
    wave-per-sequence kernel (`seq_pass_clips`), the last of them together with the remainder as `plan_slices` runs that many clips."""
    if chunk is not None:
        if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1:
            raise ValueError("chunk is a positive number of (clip, timestep) pairs")
        return [(lo, min(lo + int(chunk), n_pairs)) for lo in range(0, n_pairs, int(chunk))]
    P = seq_pass_clips(n_variants, device)
    if P == 0 or n_pairs <= P:
        return [(0, n_pairs)]
    q, r = divmod(n_pairs, P)
    lo = (q - 1) * P
    return [(i * P, (i + 1) * P) for i in range(q - 1)] + [(lo + a, lo + b) for a, b in plan_slices(P + r, n_variants, device)]


def seeded_noise(seed: int, first_clip: int, clips, steps, device) -> torch.Tensor:
    """(n, 1536, 1, 32) N(0,1) for the pairs (clips[k], steps[k]) (host sequences): pair (b, t) is `syn_randn(seed, stream_id = t,
    first_index = (first_clip + b) * 32 * 1536)` over the clip's latent in token-major order, like the loops' per-step draws - so a
    draw depends on neither the chunking of a call nor on how clips are sharded over ranks.  Runs of consecutive clips at one timestep
    are one launch."""
    lib, n = _lib.load(), len(clips)
    tm = torch.empty(n, T, CH, dtype=torch.float32, device=device)
    stream, k = _lib.current_stream(device), 0
    while k < n:
        j = k + 1
        while j < n and steps[j] == steps[k] and clips[j] == clips[j - 1] + 1:
            j += 1
        _lib.check(lib.syn_randn(tm[k].data_ptr(), (j - k) * T * CH, int(seed), int(steps[k]), (int(first_clip) + int(clips[k])) * T * CH,
                                 stream), "syn_randn")
        k = j
    out = torch.empty(n, CH, 1, T, dtype=torch.float32, device=device)
    _lib.check(lib.syn_from_token_major(tm.data_ptr(), n, out.data_ptr(), stream), "syn_from_token_major")
    return out


class BpdBatch:
    """calc_bpd_loop's (clip, timestep) pairs as batches of independent sequences: per chunk x_t = q_sample(x_start[clip], t, noise), one
    bare model evaluation of all its sequences (`run_step` with `identity_coefs`, one timestep per sequence), and `syn_bpd_terms` on
    (x_start, x_t, noise, x0_hat) in the step kernel's layout.  Nothing here waits for the device; `finish` checks the small-batch
    kernel's flag once.  StepBuffers are the model's cached ones, so chunks of one size share theirs."""

    def __init__(self, mdm, q_sample, rows: np.ndarray, t_model_of, x_start: torch.Tensor, conds: torch.Tensor, cfg_w):
        dev = x_start.device
        _require_cuda(x_start, "x_start")
        self.mdm, self.pm, self.q_sample = mdm, mdm.packed(), q_sample
        self.n_rows = len(rows)
        self.rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(self.n_rows, -1).copy()).to(dev)
        self.tmap = torch.tensor([int(t_model_of(t)) for t in range(self.n_rows)], dtype=torch.int32, device=dev)
        self.x_start = x_start.detach().float().contiguous()
        self.B, self.V = x_start.shape[0], conds.shape[0]
        self.conds, self.cfg_w = conds, cfg_w                  # (V, B, 32, 512); None, (3, V) or per clip (B, 3, V)
        self.ident = identity_coefs(dev)
        self._x0 = {}                                           # layout -> x_start in it
        self._used = []

    def _x_start_as(self, sb: StepBuffers) -> torch.Tensor:
        if sb.fragment not in self._x0:
            lib = _lib.load()
            dst = torch.empty(self.B * T, CH, dtype=torch.float32, device=self.x_start.device)
            fn, name = (lib.syn_x_to_fragment, "syn_x_to_fragment") if sb.fragment else (lib.syn_to_token_major, "syn_to_token_major")
            _lib.check(fn(self.x_start.data_ptr(), self.B, dst.data_ptr(), None, _lib.current_stream(dst.device)), name)
            self._x0[sb.fragment] = dst
        return self._x0[sb.fragment]

    def run(self, clips: torch.Tensor, steps: torch.Tensor, noise: torch.Tensor, out: torch.Tensor, want_pred: bool = False):
        """clips, steps: int64 [n] on the device (steps: rows of the table, i.e. the spaced timesteps); noise (n, 1536, 1, 32); out [3][n]
        (vb, xstart_mse, mse).  Returns x0_hat (n, 1536, 1, 32) when asked."""
        n, V, dev = clips.numel(), self.V, self.x_start.device
        lib, stream = _lib.load(), _lib.current_stream(dev)
        sb = self.mdm.step_buffers(n, V, want_x0=True)
        if not any(sb is s for s in self._used):
            self._used.append(sb)
        sb.load_x(self.q_sample(self.x_start[clips], steps, noise))
        sb.load_noise(noise)
        sb.cond.copy_(self.conds[:, clips].reshape(-1, D))
        if V > 1:
            sb.cfg_w.copy_(self.cfg_w if self.cfg_w.dim() == 2 else self.cfg_w[clips])
        t32, c32 = steps.to(torch.int32), clips.to(torch.int32)
        sb.t_model.copy_(self.tmap[steps].repeat(V))
        sb.t_coef.zero_()
        # the evaluation must leave x_t alone: x0_hat goes to sb.x0 as the step's x_next (identity row), its bf16 copy over the operand copy
        c = sb.c
        saved = (c.x_next, c.pred_x0)
        try:
            c.x_next, c.pred_x0 = sb.x0.data_ptr(), None
            run_step(self.pm, sb, self.ident, use_noise=False)
        finally:
            c.x_next, c.pred_x0 = saved
        assert out.shape == (3, n) and out.is_contiguous()
        _lib.check(lib.syn_bpd_terms(self.rows.data_ptr(), self.n_rows, t32.data_ptr(), c32.data_ptr(), self._x_start_as(sb).data_ptr(),
                                     self.B, sb.x.data_ptr(), sb.noise.data_ptr(), sb.x0.data_ptr(), n, out.data_ptr(), stream),
                   "syn_bpd_terms")
        del t32, c32                                           # (held until the launch is enqueued)
        if not want_pred:
            return None
        pred = torch.empty(n, CH, 1, T, dtype=torch.float32, device=dev)
        fn, name = (lib.syn_x_from_fragment, "syn_x_from_fragment") if sb.fragment else (lib.syn_from_token_major, "syn_from_token_major")
        _lib.check(fn(sb.x0.data_ptr(), n, pred.data_ptr(), stream), name)
        return pred

    def finish(self):
        for sb in self._used:
            sb.check_sync()
