"""Training the body-part RVQ-VAE codecs (reference rvq_beatx_train.py over models/vq/ in train mode) on the HIP kernels of
csrc/syn_rvq_train.inc and the eval path's convolution kernel.

`RVQTrainer` OWNS an eval-mode `rvqvae.RVQVAE` - training is not a mode of that module, whose `train()` keeps raising - and updates its fp32
parameters and codebooks in place: after a step, `model.map2latent` / `latent2origin` see the new weights through the usual staleness rule
(`engine.weights_key`: every tensor written through a raw pointer gets its version bumped).

    model = rvqvae.build(78).cuda()
    trainer = RVQTrainer(model)                       # the reference's defaults, rvq_beatx_train.py:94-124,299-325
    out = trainer.step(motion)                        # (N, T % 4 == 0, 78) -> {"loss", "recons", "commit", "perplexity"}: device scalars, no host sync
    trainer.save_net("net_last.pth")                  # {'net': state_dict}, what RVQVAE.load_state_dict and the reference load

Train-mode semantics, each from the reference: Dropout(0.2) behind conv2 of the 12 residual blocks (resnet.py:46,66-68); quantise dropout
(residual_vq.py:112-136: with probability 0.2 only layers 0 .. randrange(0, 6) run, losses and perplexities averaged over those); per active
layer (quantizer.py:132-158) init_codebook on its first forward, idx = argmax(-dist / 0.5 + gumbel), x_d from the codebook BEFORE the update,
commit = mse(x, x_d), then the EMA / usage / reset update; the residual is updated IN PLACE on the encoder output (residual_vq.py:146), so the
gradient that reaches the encoder is n_active times the decoder's input gradient plus the commit terms; loss = recons + 0.02 commit.
As in the reference, the `init` flags are not part of a `net` checkpoint: a trainer built on a loaded model RE-INITIALISES the codebooks from
its first batch unless the trainer's own `state_dict()` is restored.

`draws` (see `draw`) holds every random input of a step so that tests can inject them.  With draws=None the trainer draws them: the tensors
from torch's generator on the device (they follow torch.manual_seed), the quantise-dropout coin from its own `random.Random(seed)`.
No torch arithmetic, MIOpen or library GEMM runs on the step; a missing kernel is an error (no CPU path).
"""
from __future__ import annotations

import ctypes as C
import random

import torch

from . import _lib, engine
from .optim import ClipAdam
from .rvqvae import CODE_DIM, NB_CODE, NUM_Q, RVQVAE, _up

ENTRY_POINTS = ("syn_vq_train_pack", "syn_vq_train_cast", "syn_vq_train_ew", "syn_vq_train_pairsum", "syn_vq_train_stuff", "syn_vq_train_wgrad",
                "syn_vq_train_codebook_prep", "syn_vq_train_tile", "syn_vq_train_quantize", "syn_vq_train_codebook_update",
                "syn_vq_train_loss_parts", "syn_vq_train_loss", "syn_vq_train_scalars")
LOSS_KINDS = {"l2": 0, "l1": 1, "l1_smooth": 2}


def lr_at(iteration: int, lr=2e-4, warm_up_iter=1000, milestones=(50000, 400000), gamma=0.05) -> float:
    """Learning rate of optimiser step number `iteration` (0-based) of rvq_beatx_train.py:333-381: warm_up_iter - 1 warm-up steps at
    lr * (nb_iter + 1) / (warm_up_iter + 1), nb_iter = 1 .., then MultiStepLR - chainable, so it continues from the LAST warm-up value."""
    n_warm = max(warm_up_iter - 1, 0)
    if iteration < n_warm:
        return lr * (iteration + 2) / (warm_up_iter + 1)
    base = lr * warm_up_iter / (warm_up_iter + 1) if n_warm else lr
    return base * gamma ** sum(1 for m in milestones if m <= iteration - n_warm)


def body_part_mask(body_part: str, dataname: str = "beatx") -> list:
    """Channels of the full pose vector one body-part codec is trained on (rvq_beatx_train.py:210-295).  BEAT-X poses are 55 joints x rot6d + 3
    translation channels at 330 .. 332; the h3d_623 layout is 4 root channels, 51 x 3 positions, 51 x 6 rotations, 52 x 3 velocities, 4 foot
    contacts.  The reference's h3d `upper` branch builds this mask and then names an undefined variable; the mask it builds is used.  Parts the
    h3d section does not list keep the BEAT-X channels, as they do in the reference."""
    six = lambda joints: [j * 6 + k for j in joints for k in range(6)]
    upper, lower = [3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21], [0, 1, 2, 4, 5, 7, 8, 10, 11]
    masks = {"upper": six(upper), "hands": six(range(25, 55)), "lower": six(lower), "lower_trans": six(lower) + [330, 331, 332],
             "whole_trans": six(list(range(0, 22)) + list(range(25, 55))) + [330, 331, 332]}
    if body_part not in masks:
        raise ValueError(f"body_part must be one of {sorted(masks)}, got {body_part!r}")
    if dataname == "h3d_623" and body_part in ("upper", "hands", "lower_trans"):
        def joint(i):
            pos = [4 + (i - 1) * 3 + k for k in range(3)] if i > 0 else []
            rot = [4 + 51 * 3 + (i - 1) * 6 + k for k in range(6)] if i > 0 else []
            return pos + rot + [4 + 51 * 9 + i * 3 + k for k in range(3)]
        if body_part == "lower_trans":
            return list(range(0, 4)) + list(range(619, 623)) + [c for i in lower for c in joint(i)]
        return [c for i in (upper if body_part == "upper" else range(22, 52)) for c in joint(i)]
    return masks[body_part]


class RVQTrainer:
    def __init__(self, model: RVQVAE, *, lr=2e-4, betas=(0.9, 0.99), commit=0.02, recons_loss="l2", mu=0.99, quantize_dropout_prob=0.2,
                 temperature=0.5, dropout=0.2, warm_up_iter=1000, milestones=(50000, 400000), gamma=0.05, weight_decay=0.0, seed=0, forward_products=3):
        if not isinstance(model, RVQVAE):
            raise TypeError("RVQTrainer trains a syntalker_amd.rvqvae.RVQVAE")
        if weight_decay:
            raise NotImplementedError("RVQTrainer: weight_decay != 0 (AdamW's decoupled decay) is not implemented; the reference trains with 0")
        if forward_products not in (1, 3):
            raise ValueError("forward_products: 3 (W_hi x_hi + W_lo x_hi + W_hi x_lo, the default) or 1 (a plain bf16 forward - diagnostic: its gradients "
                             "miss the 3e-2 gate, scripts/diag_rvq_train_forward.py, DESIGN.md 16.3)")
        if recons_loss not in LOSS_KINDS:
            raise ValueError(f"recons_loss must be one of {sorted(LOSS_KINDS)}, got {recons_loss!r}")
        if not (0.0 <= dropout < 1.0 and 0.0 <= quantize_dropout_prob <= 1.0 and temperature > 0.0):
            raise ValueError("RVQTrainer: 0 <= dropout < 1, 0 <= quantize_dropout_prob <= 1, temperature > 0")
        self.model, self.dim = model, model.input_width
        self.lr, self.betas, self.commit, self.recons_loss, self.mu = float(lr), tuple(betas), float(commit), recons_loss, float(mu)
        self.quantize_dropout_prob, self.temperature, self.dropout = float(quantize_dropout_prob), float(temperature), float(dropout)
        self.warm_up_iter, self.milestones, self.gamma = int(warm_up_iter), tuple(milestones), float(gamma)
        self.forward_products = int(forward_products)
        self.iteration = 0
        self.init = [False] * NUM_Q
        self.code_sum = torch.zeros(NUM_Q, NB_CODE, CODE_DIM)
        self.code_count = torch.zeros(NUM_Q, NB_CODE)
        self._coin = random.Random(seed)
        self._opt, self._opt_state, self._lr_dev = None, None, None
        self._convs = [(key, cin, cout, taps, stride, dil, pad) for key, cin, cout, taps, stride, dil, pad in model._enc + model._dec]
        self._weights, self._bufs, self._grads = None, {}, None

    # ---- random inputs -------------------------------------------------------------------------------------------------------------
    def quantize_dropout_start(self):
        """residual_vq.py:112-117 on the trainer's own generator: None, or the index of the last layer that runs."""
        if self._coin.random() < self.quantize_dropout_prob:
            return self._coin.randrange(0, NUM_Q)
        return None

    def draw(self, n: int, t: int, device) -> dict:
        """Every random input of one step on (n, t) motion:
          "gumbel": 6 x (n t/4, 512) Gumbel noise (None for a layer quantise dropout skips)   quantizer.py:14-16
          "keep":  12 x (n, 512, t_b) keep masks of the residual blocks in execution order (t_b = t/2, t/4 encoder; t/4, t/2 decoder)
          "start": None or the quantise-dropout index (layers > start are skipped)
          "tile":  6 x list of (512, 512) normal draws `_tile` takes when n t/4 < 512, in call order (init_codebook first)"""
        start = self.quantize_dropout_start()
        n_active = NUM_Q if start is None else start + 1
        rows = n * t // 4
        gumbel = [torch.empty(rows, NB_CODE, device=device).exponential_().log_().neg_() if q < n_active else None for q in range(NUM_Q)]   # -log(Exp(1))
        keep = [torch.empty(n, CODE_DIM, tb, device=device).bernoulli_(1.0 - self.dropout).to(torch.bool)
                for tb in (t // 2,) * 3 + (t // 4,) * 6 + (t // 2,) * 3]
        tile = [[torch.randn(NB_CODE, CODE_DIM, device=device) for _ in range((0 if self.init[q] else 1) + 1)] if q < n_active and rows < NB_CODE else []
                for q in range(NUM_Q)]
        return {"gumbel": gumbel, "keep": keep, "start": start, "tile": tile}

    # ---- device-side state -----------------------------------------------------------------------------------------------------------
    def _device(self):
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise _lib.SynHipError("RVQTrainer runs on the HIP kernels only: move the model to the GPU (no CPU fallback)")
        return dev

    def _prepare(self, dev):
        """Parameters' gradient buffers, the optimiser, the fragment buffers and the packing jobs that fill them; rebuilt when a parameter moved."""
        params = dict(self.model.named_parameters())
        key = tuple(p.data_ptr() for p in params.values())
        if self._weights is not None and self._weights["key"] == key:
            return self._weights
        if self._opt is not None:                                        # the parameters moved (model.to(...), re-allocation): the Adam moments move with them
            self._opt_state = self._opt.state_dict()
        self.code_sum, self.code_count = self.code_sum.to(dev).contiguous(), self.code_count.to(dev).contiguous()
        self._grads = {k: torch.zeros_like(p) for k, p in params.items()}
        for k, p in params.items():
            p.grad = self._grads[k]
        self._lr_dev = torch.zeros((), device=dev)
        self._opt = ClipAdam(list(params.values()), lr=self._lr_dev, betas=self.betas, max_norm=None)
        if self._opt_state is not None:
            self._opt.load_state_dict(self._opt_state)
            self._opt.param_groups[0]["lr"] = self._lr_dev
            self._opt_state = None
        w = {"key": key, "fwd": [], "bwd": [], "keep": []}
        zero_bias = torch.zeros(512, device=dev)
        jobs, max_units = [], 0
        for i, (ck, cin, cout, taps, stride, dil, pad) in enumerate(self._convs):
            wt, bias = params[ck + ".weight"], params[ck + ".bias"]
            cin_p, cout_p = _up(cin, 32), _up(cout, 128)
            frag, frag_lo = (torch.empty(taps, cout_p // 16, cin_p // 32, 64, 8, dtype=torch.bfloat16, device=dev) for _ in range(2))
            jobs.append((wt.data_ptr(), frag.data_ptr(), cout, cin, taps, cout_p, cin_p, 0))
            jobs.append((wt.data_ptr(), frag_lo.data_ptr(), cout, cin, taps, cout_p, cin_p, 3))
            max_units = max(max_units, frag.numel() // 8)
            if cout_p != cout:
                bias_p = torch.empty(cout_p, device=dev)
                jobs.append((bias.data_ptr(), bias_p.data_ptr(), cout, 0, 0, cout_p, 0, 2))
            else:
                bias_p = bias
            # the forward's three products: W_hi x_hi + bias, W_lo x_hi, W_hi x_lo
            w["fwd"].append(tuple(_lib.SynVqConv(f.data_ptr(), bp.data_ptr(), cin_p, cout_p, cout, taps, stride, dil, pad, 0, 0, 0)
                                  for f, bp in ((frag, bias_p), (frag_lo, zero_bias), (frag, zero_bias))))
            w["keep"] += [frag, frag_lo, bias_p]
            if i == 0:
                w["bwd"].append(None)                                    # the pose needs no gradient
                continue
            # data gradient = the same kernel on W'[ci][co][taps - 1 - tap], stride 1 (the stride-2 convolutions take dy with zeros between
            # its frames, the convolution behind an upsample is followed by a pair sum), padding (taps - 1) dil - pad
            tcout_p, tcin_p = _up(cin, 128), _up(cout, 32)
            tfrag = torch.empty(taps, tcout_p // 16, tcin_p // 32, 64, 8, dtype=torch.bfloat16, device=dev)
            jobs.append((wt.data_ptr(), tfrag.data_ptr(), cout, cin, taps, tcout_p, tcin_p, 1))
            max_units = max(max_units, tfrag.numel() // 8)
            w["bwd"].append(_lib.SynVqConv(tfrag.data_ptr(), zero_bias.data_ptr(), tcin_p, tcout_p, cin, taps, 1, dil, (taps - 1) * dil - pad, 0, 0, 0))
            w["keep"].append(tfrag)
        table = (_lib.SynVqTrainPackJob * len(jobs))(*[_lib.SynVqTrainPackJob(*j) for j in jobs])
        w["jobs"] = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        w["n_jobs"], w["max_units"], w["zero_bias"] = len(jobs), max_units, zero_bias
        w["cbt"], w["cc"] = torch.empty(CODE_DIM, NB_CODE, device=dev), torch.empty(NB_CODE, device=dev)
        w["bcount"], w["out4"] = torch.zeros(NUM_Q, NB_CODE, device=dev), torch.zeros(4, device=dev)
        self._weights = w
        return w

    def _buffers(self, n, t, dev):
        b = self._bufs.get((n, t, str(dev)))
        if b is not None:
            return b
        if len(self._bufs) > 2:
            self._bufs.clear()
        lib = _lib.load()
        dp, rows = _up(self.dim, 32), n * t // 4
        bf = lambda tt, c=512: torch.empty(n, tt, c, dtype=torch.bfloat16, device=dev)
        f32 = lambda tt, c=512: torch.empty(n, tt, c, device=dev)
        t2, t4 = t // 2, t // 4
        groups = int(lib.syn_vq_quantize_groups(rows))
        b = {
            "in0": bf(t, dp), "a0": bf(t), "in0_lo": bf(t, dp), "a0_lo": bf(t), "xqb_lo": bf(t4), "u1b_lo": bf(t), "h15_lo": bf(t),
            "exb_lo": [[bf(tt) for _ in range(4)] for tt in (t2, t4)], "ehb_lo": [[bf(tt) for _ in range(3)] for tt in (t2, t4)],
            "dxb_lo": [[bf(tt) for _ in range(4)] for tt in (t4, t2)], "dhb_lo": [[bf(tt) for _ in range(3)] for tt in (t4, t2)],
            "rec_p": f32(t, _up(self.dim, 128)),
            "exf": [f32(t2), f32(t4)], "exb": [[bf(tt) for _ in range(4)] for tt in (t2, t4)], "ehb": [[bf(tt) for _ in range(3)] for tt in (t2, t4)],
            "lat": f32(t4), "rr": [f32(t4), f32(t4)], "xq": f32(t4), "xqb": bf(t4), "rsum": f32(t4),
            "idx": torch.empty(rows, NUM_Q, dtype=torch.int32, device=dev), "groups": groups, "sqerr": torch.zeros(NUM_Q, groups, device=dev),
            "dxf": [f32(t4), f32(t2), f32(t)], "dxb": [[bf(tt) for _ in range(4)] for tt in (t4, t2)], "dhb": [[bf(tt) for _ in range(3)] for tt in (t4, t2)],
            "u1b": bf(t), "h15": bf(t), "rec": torch.empty(n, t, self.dim, device=dev),
            "c2f": f32(t),                                                # conv2 outputs (forward), data-gradient outputs (backward): any resolution
            "drec": bf(t, dp), "parts": torch.empty(int(lib.syn_vq_train_loss_parts(n * t, dp)), device=dev),
            "gf": f32(t), "gb": bf(t), "gb2": bf(t),
        }
        self._bufs[(n, t, str(dev))] = b
        return b

    def _residual_vq(self, w, b, draws, n_active, rows, dev):
        """ResidualVQ.forward in training on b["lat"] (N T/4 rows), one layer per launch: a layer's first forward initialises its codebook from
        ITS input rows, every layer's codebook is updated behind its quantisation.  Fills b["xq"], b["rsum"], b["idx"], b["sqerr"], w["bcount"]."""
        lib, st = _lib.load(), _lib.current_stream(dev)
        b["idx"].fill_(-1)
        codebooks = [self.model.get_buffer(f"quantizer.layers.{q}.codebook") for q in range(NUM_Q)]
        one_minus_mu = 1.0 - self.mu
        for q in range(n_active):
            xin, xout = (b["lat"] if q == 0 else b["rr"][(q - 1) & 1]), b["rr"][q & 1]
            noise = [z.to(dev).contiguous().float() for z in draws["tile"][q]] if rows < NB_CODE else []
            if rows < NB_CODE and len(noise) != (1 if self.init[q] else 2):
                raise ValueError(f"draws['tile'][{q}]: {1 if self.init[q] else 2} (512, 512) normal draws needed at {rows} < 512 rows, got {len(noise)}")
            cb = codebooks[q]
            if not self.init[q]:
                _lib.check(lib.syn_vq_train_tile(xin.data_ptr(), rows, _lib.ptr(noise.pop(0) if noise else None), cb.data_ptr(),
                                                 self.code_sum[q].data_ptr(), self.code_count[q].data_ptr(), st), "syn_vq_train_tile")
                self.init[q] = True
            _lib.check(lib.syn_vq_train_codebook_prep(cb.data_ptr(), w["cbt"].data_ptr(), w["cc"].data_ptr(), st), "syn_vq_train_codebook_prep")
            g = draws["gumbel"][q].to(dev).contiguous().float()
            if tuple(g.shape) != (rows, NB_CODE):
                raise ValueError(f"draws['gumbel'][{q}]: expected {(rows, NB_CODE)}, got {tuple(g.shape)}")
            _lib.check(lib.syn_vq_train_quantize(xin.data_ptr(), cb.data_ptr(), w["cbt"].data_ptr(), w["cc"].data_ptr(), g.data_ptr(), self.temperature,
                                                 xout.data_ptr(), b["xq"].data_ptr(), None, b["rsum"].data_ptr(), b["idx"].data_ptr(),
                                                 b["sqerr"][q].data_ptr(), q, int(q == 0), rows, st), "syn_vq_train_quantize")
            _lib.check(lib.syn_vq_train_codebook_update(xin.data_ptr(), b["idx"].data_ptr(), q, rows, _lib.ptr(noise.pop(0) if noise else None), self.mu,
                                                        one_minus_mu, cb.data_ptr(), self.code_sum[q].data_ptr(), self.code_count[q].data_ptr(),
                                                        w["bcount"][q].data_ptr(), st), "syn_vq_train_codebook_update")
        torch.autograd.graph.increment_version(codebooks[:n_active])     # written through raw pointers (`engine.weights_key`)

    @torch.no_grad()
    def quantize(self, latent: torch.Tensor, draws: dict) -> dict:
        """The residual quantiser alone, in training mode, on latent (N, T', 512): what the reference's `quantizer(x, sample_codebook_temp=0.5)` does
        in train() - codebook initialisation, Gumbel sampling, EMA update.  draws: "gumbel", "start", "tile" as in `draw`.
        Returns {"xq" (N, T', 512), "idx" (N T', 6), "commit", "perplexity", "n_active"}."""
        dev = self._device()
        engine._require_cuda(latent, "latent")
        n, t4, c = latent.shape
        if c != CODE_DIM:
            raise ValueError(f"RVQTrainer.quantize: expected (N, T', {CODE_DIM}), got {tuple(latent.shape)}")
        lib, st = _lib.load(), _lib.current_stream(dev)
        w, b = self._prepare(dev), self._buffers(n, 4 * t4, dev)
        start = draws.get("start")
        n_active, rows = NUM_Q if start is None else int(start) + 1, n * t4
        b["lat"].copy_(latent.reshape(n, t4, c))
        self._residual_vq(w, b, draws, n_active, rows, dev)
        b["parts"][:1].zero_()
        _lib.check(lib.syn_vq_train_scalars(b["parts"].data_ptr(), 1, 1, b["sqerr"].data_ptr(), b["groups"], w["bcount"].data_ptr(), n_active, rows,
                                            self.commit, w["out4"].data_ptr(), st), "syn_vq_train_scalars")
        out4 = w["out4"].clone()
        return {"xq": b["xq"].clone(), "idx": b["idx"].clone(), "commit": out4[2], "perplexity": out4[3], "n_active": n_active}

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_backward(self, motion: torch.Tensor, draws: dict | None = None, forward_only: bool = False) -> dict:
        """Forward and backward of one step (no optimiser update; the codebooks ARE updated, as the reference's forward does).
        Returns {"loss", "recons", "commit", "perplexity"} (device scalars), "rec_pose" (N, T, dim), "latent" / "xq" (N, T/4, 512), "idx"
        (N T/4, 6; -1 in skipped layers), "n_active" and "grads": parameter name -> gradient.  Everything returned is a copy the caller owns, EXCEPT
        "grads": those are the parameters' `.grad` tensors themselves, which the optimiser reads and the next call overwrites - clone what must outlive it."""
        dev = self._device()
        engine._require_cuda(motion, "motion")
        n, t, d = motion.shape
        if d != self.dim or t % 4 or t < 4:
            raise ValueError(f"RVQTrainer: expected motion (N, T % 4 == 0, {self.dim}), got {tuple(motion.shape)}")
        lib, st = _lib.load(), _lib.current_stream(dev)
        w, b = self._prepare(dev), self._buffers(n, t, dev)
        if draws is None:
            draws = self.draw(n, t, dev)
        start = draws.get("start")
        n_active = NUM_Q if start is None else int(start) + 1
        if not 1 <= n_active <= NUM_Q:
            raise ValueError(f"draws['start'] must be None or 0 .. {NUM_Q - 1}")
        t2, t4, rows, dp = t // 2, t // 4, n * t // 4, _up(self.dim, 32)
        keep = []
        for i, tb in enumerate((t2,) * 3 + (t4,) * 6 + (t2,) * 3):
            k = draws["keep"][i]
            if tuple(k.shape) != (n, CODE_DIM, tb):
                raise ValueError(f"draws['keep'][{i}]: expected {(n, CODE_DIM, tb)}, got {tuple(k.shape)}")
            keep.append(k.to(dev).permute(0, 2, 1).contiguous().to(torch.uint8))      # channels-last bytes (layout change, no arithmetic)
        motion = motion.contiguous().float()
        E, D = w["fwd"][:16], w["fwd"][16:]
        inv_keep = 1.0 / (1.0 - self.dropout)

        def conv(cv, x, yf, yb, t_in, t_out, up=0, relu_in=0, relu_out=0, ldy=512, resid=None, cout_valid=None):
            cv.up, cv.relu_in, cv.relu_out = up, relu_in, relu_out
            if cout_valid is not None:
                cv.cout_valid = cout_valid
            _lib.check(lib.syn_vq_conv1d(C.byref(cv), x.data_ptr(), _lib.ptr(resid), _lib.ptr(yf), ldy, _lib.ptr(yb), n, t_in, t_out, st), "syn_vq_conv1d")

        def conv3(cvs, x, x_lo, yf, t_in, t_out, up=0, relu_in=0, relu_out=0):
            """One convolution of the training forward at fp32 grade: W_hi x_hi + bias, + W_lo x_hi, + W_hi x_lo, summed in fp32 through the kernel's
            residual input.  The low part of x arrives with its consumer's ReLU already applied (k_ew, lo_relu)."""
            if self.forward_products == 1:                             # diagnostic: the plain bf16 forward
                return conv(cvs[0], x, yf, None, t_in, t_out, up=up, relu_in=relu_in, relu_out=relu_out)
            conv(cvs[0], x, yf, None, t_in, t_out, up=up, relu_in=relu_in)
            conv(cvs[1], x, yf, None, t_in, t_out, up=up, relu_in=relu_in, resid=yf)
            conv(cvs[2], x_lo, yf, None, t_in, t_out, up=up, relu_out=relu_out, resid=yf)

        def ew(v, numel, resid=None, relu_src=None, keep_b=None, sv=1.0, sr=1.0, out_f=None, out_b=None, out_lo=None, lo_relu=0):
            _lib.check(lib.syn_vq_train_ew(v.data_ptr(), _lib.ptr(resid), _lib.ptr(relu_src), _lib.ptr(keep_b), sv, sr, _lib.ptr(out_f), _lib.ptr(out_b),
                                           _lib.ptr(out_lo), lo_relu, numel, st), "syn_vq_train_ew")

        def resnet_fwd(cvs, xf, xb, xl, hb, hl, keeps, tt):
            """Resnet1D in training: 3 x { x += dropout(conv2(relu(conv1(relu(x))))) }, the bf16 input of every convolution kept."""
            m = n * tt * 512
            for j in range(3):
                conv3(cvs[2 * j], xb[j], xl[j], b["c2f"], tt, tt, relu_in=1)
                ew(b["c2f"], m, out_b=hb[j], out_lo=hl[j], lo_relu=1)
                conv3(cvs[2 * j + 1], hb[j], hl[j], b["c2f"], tt, tt, relu_in=1)
                ew(b["c2f"], m, resid=xf, keep_b=keeps[j], sv=inv_keep, out_f=xf, out_b=xb[j + 1], out_lo=xl[j + 1], lo_relu=int(j < 2))

        # ---- forward ---------------------------------------------------------------------------------------------------------------------
        _lib.check(lib.syn_vq_train_pack(w["jobs"].data_ptr(), w["n_jobs"], w["max_units"], st), "syn_vq_train_pack")
        _lib.check(lib.syn_vq_train_cast(motion.data_ptr(), n * t, self.dim, dp, b["in0"].data_ptr(), b["in0_lo"].data_ptr(), st), "syn_vq_train_cast")
        conv3(E[0], b["in0"], b["in0_lo"], b["c2f"], t, t, relu_out=1)
        ew(b["c2f"], n * t * 512, out_b=b["a0"], out_lo=b["a0_lo"])
        x, x_lo, tt = b["a0"], b["a0_lo"], t
        for i in range(2):
            conv3(E[1 + 7 * i], x, x_lo, b["c2f"], tt, tt // 2)
            tt //= 2
            ew(b["c2f"], n * tt * 512, out_f=b["exf"][i], out_b=b["exb"][i][0], out_lo=b["exb_lo"][i][0], lo_relu=1)
            resnet_fwd(E[2 + 7 * i:8 + 7 * i], b["exf"][i], b["exb"][i], b["exb_lo"][i], b["ehb"][i], b["ehb_lo"][i], keep[3 * i:3 * i + 3], tt)
            x, x_lo = b["exb"][i][3], b["exb_lo"][i][3]
        conv3(E[15], x, x_lo, b["lat"], t4, t4)
        latent = b["lat"].clone()

        self._residual_vq(w, b, draws, n_active, rows, dev)

        # ---- decoder -----------------------------------------------------------------------------------------------------------------------
        ew(b["xq"], n * t4 * 512, out_b=b["xqb"], out_lo=b["xqb_lo"])
        conv3(D[0], b["xqb"], b["xqb_lo"], b["c2f"], t4, t4, relu_out=1)
        ew(b["c2f"], n * t4 * 512, out_f=b["dxf"][0], out_b=b["dxb"][0][0], out_lo=b["dxb_lo"][0][0], lo_relu=1)
        tt = t4
        for i in range(2):
            resnet_fwd(D[1 + 7 * i:7 + 7 * i], b["dxf"][i], b["dxb"][i], b["dxb_lo"][i], b["dhb"][i], b["dhb_lo"][i], keep[6 + 3 * i:9 + 3 * i], tt)
            conv3(D[7 + 7 * i], b["dxb"][i][3], b["dxb_lo"][i][3], b["c2f"], tt, 2 * tt, up=1)                  # Upsample x2 folded into the read
            tt *= 2
            if i == 0:
                ew(b["c2f"], n * tt * 512, out_f=b["dxf"][1], out_b=b["dxb"][1][0], out_lo=b["dxb_lo"][1][0], lo_relu=1)
            else:
                ew(b["c2f"], n * tt * 512, out_b=b["u1b"], out_lo=b["u1b_lo"])
        conv3(D[15], b["u1b"], b["u1b_lo"], b["c2f"], t, t, relu_out=1)
        ew(b["c2f"], n * t * 512, out_b=b["h15"], out_lo=b["h15_lo"])
        # the last convolution's cout is the pose width: its partial sums go through a scratch of the padded width (the kernel reads its residual
        # input at that pitch), the last product writes (N, T, dim)
        last, cp = D[16], _up(self.dim, 128)
        if self.forward_products == 1:
            conv(last[0], b["h15"], b["rec"], None, t, t, ldy=self.dim, cout_valid=self.dim)
        else:
            conv(last[0], b["h15"], b["rec_p"], None, t, t, ldy=cp, cout_valid=cp)
            conv(last[1], b["h15"], b["rec_p"], None, t, t, ldy=cp, cout_valid=cp, resid=b["rec_p"])
            conv(last[2], b["h15_lo"], b["rec"], None, t, t, ldy=self.dim, cout_valid=self.dim, resid=b["rec_p"])
        _lib.check(lib.syn_vq_train_loss(b["rec"].data_ptr(), motion.data_ptr(), n * t, self.dim, dp, LOSS_KINDS[self.recons_loss], b["drec"].data_ptr(),
                                         b["parts"].data_ptr(), st), "syn_vq_train_loss")
        _lib.check(lib.syn_vq_train_scalars(b["parts"].data_ptr(), b["parts"].numel(), n * t * self.dim, b["sqerr"].data_ptr(), b["groups"],
                                            w["bcount"].data_ptr(), n_active, rows, self.commit, w["out4"].data_ptr(), st), "syn_vq_train_scalars")
        out4 = w["out4"].clone()
        out = {"loss": out4[0], "recons": out4[1], "commit": out4[2], "perplexity": out4[3], "rec_pose": b["rec"].clone(), "latent": latent,
               "xq": b["xq"].clone(), "idx": b["idx"].clone(), "n_active": n_active, "grads": self._grads}
        if forward_only:
            return out

        # ---- backward --------------------------------------------------------------------------------------------------------------------
        G = self._grads
        B = w["bwd"]

        def wgrad(i, dy, x, t_in, t_out, up=0, relu_in=0, ldy=512, ldx=512):
            key, cin, cout, taps, stride, dil, pad = self._convs[i]
            _lib.check(lib.syn_vq_train_wgrad(dy.data_ptr(), ldy, x.data_ptr(), ldx, G[key + ".weight"].data_ptr(), G[key + ".bias"].data_ptr(), n, t_in, t_out,
                                              cout, cin, taps, stride, dil, pad, up, relu_in, st), "syn_vq_train_wgrad")

        def dgrad(i, dy, yf, yb, t_len):
            conv(B[i], dy, yf, yb, t_len, t_len)

        def resnet_bwd(first, xb, hb, keeps, tt):
            """Backward of resnet_fwd on gf (fp32, in place); leaves bf16(gf) in gb.  `first`: index of the first block's conv1 in self._convs."""
            m = n * tt * 512
            for j in (2, 1, 0):
                c1, c2 = first + 2 * j, first + 2 * j + 1
                ew(b["gf"], m, keep_b=keeps[j], sv=inv_keep, out_b=b["gb2"])                    # d conv2 output
                wgrad(c2, b["gb2"], hb[j], tt, tt, relu_in=1)
                dgrad(c2, b["gb2"], b["c2f"], None, tt)
                ew(b["c2f"], m, relu_src=hb[j], out_b=b["gb2"])                                 # through the ReLU in front of conv2
                wgrad(c1, b["gb2"], xb[j], tt, tt, relu_in=1)
                dgrad(c1, b["gb2"], b["c2f"], None, tt)
                ew(b["c2f"], m, resid=b["gf"], relu_src=xb[j], out_f=b["gf"], out_b=b["gb"])    # through the ReLU in front of conv1, + the skip path

        # last two convolutions
        wgrad(32, b["drec"], b["h15"], t, t, ldy=dp)
        dgrad(32, b["drec"], b["c2f"], None, t)
        ew(b["c2f"], n * t * 512, relu_src=b["h15"], out_b=b["gb"])
        wgrad(31, b["gb"], b["u1b"], t, t)
        dgrad(31, b["gb"], None, b["gb2"], t)
        # decoder stages, last first: the convolution behind the upsample, then the residual blocks
        tt, dy = t, b["gb2"]
        for i in (1, 0):
            wgrad(16 + 7 + 7 * i, dy, b["dxb"][i][3], tt // 2, tt, up=1)
            dgrad(16 + 7 + 7 * i, dy, b["c2f"], None, tt)
            tt //= 2
            _lib.check(lib.syn_vq_train_pairsum(b["c2f"].data_ptr(), b["gf"].data_ptr(), n * tt, 512, st), "syn_vq_train_pairsum")
            resnet_bwd(16 + 1 + 7 * i, b["dxb"][i], b["dhb"][i], keep[6 + 3 * i:9 + 3 * i], tt)
            dy = b["gb"]
        m4 = n * t4 * 512
        ew(b["gf"], m4, relu_src=b["dxb"][0][0], out_b=b["gb"])                                  # the ReLU behind the decoder's first convolution
        wgrad(16, b["gb"], b["xqb"], t4, t4)
        dgrad(16, b["gb"], b["c2f"], None, t4)
        # into the encoder: n_active straight-through paths (the in-place residual, residual_vq.py:146) + the commit terms 2 (x - x_d) / (rows 512)
        ew(b["c2f"], m4, resid=b["rsum"], sv=float(n_active), sr=self.commit * 2.0 / (n_active * rows * CODE_DIM), out_b=b["gb"])
        wgrad(15, b["gb"], b["exb"][1][3], t4, t4)
        dgrad(15, b["gb"], b["gf"], None, t4)
        tt = t4
        for i in (1, 0):
            resnet_bwd(2 + 7 * i, b["exb"][i], b["ehb"][i], keep[3 * i:3 * i + 3], tt)
            src = b["exb"][0][3] if i == 1 else b["a0"]
            wgrad(1 + 7 * i, b["gb"], src, 2 * tt, tt)
            _lib.check(lib.syn_vq_train_stuff(b["gb"].data_ptr(), b["gb2"].data_ptr(), n * tt, 512, st), "syn_vq_train_stuff")
            tt *= 2
            if i == 1:
                dgrad(1 + 7 * i, b["gb2"], b["gf"], None, tt)
            else:
                dgrad(1 + 7 * i, b["gb2"], b["c2f"], None, tt)
                ew(b["c2f"], n * tt * 512, relu_src=b["a0"], out_b=b["gb"])                     # the ReLU behind the first convolution
        wgrad(0, b["gb"], b["in0"], t, t, ldx=dp)
        return out

    def step(self, motion: torch.Tensor, draws: dict | None = None) -> dict:
        """One training step: forward, backward, Adam.  Returns {"loss", "recons", "commit", "perplexity"} as device scalars; nothing here waits
        for the device."""
        dev = self._device()
        self._prepare(dev)
        self._lr_dev.fill_(lr_at(self.iteration, self.lr, self.warm_up_iter, self.milestones, self.gamma))
        out = self.forward_backward(motion, draws)
        self._opt.step()                                                 # (bumps the parameters' versions: `engine.weights_key`)
        self.iteration += 1
        return {k: out[k] for k in ("loss", "recons", "commit", "perplexity")}

    # ---- checkpoints -------------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        opt = self._opt.state_dict() if self._opt is not None else self._opt_state
        return {"net": {k: v.detach().clone() for k, v in self.model.state_dict().items()}, "code_sum": self.code_sum.detach().clone(),
                "code_count": self.code_count.detach().clone(), "init": list(self.init), "optimizer": opt, "iteration": self.iteration,
                "coin": self._coin.getstate()}

    def load_state_dict(self, sd: dict):
        self.model.load_state_dict(sd["net"])
        dev = next(self.model.parameters()).device
        self.code_sum, self.code_count = sd["code_sum"].to(dev).float().contiguous().clone(), sd["code_count"].to(dev).float().contiguous().clone()
        self.init, self.iteration = [bool(v) for v in sd["init"]], int(sd["iteration"])
        self._coin.setstate(sd["coin"])
        if self._opt is not None and sd["optimizer"] is not None:
            self._opt.load_state_dict(sd["optimizer"])
            self._opt.param_groups[0]["lr"] = self._lr_dev
        else:
            self._opt_state = sd["optimizer"]

    def save_net(self, path: str):
        """The reference's checkpoint (rvq_beatx_train.py:404): {'net': state_dict}."""
        torch.save({"net": {k: v.detach().cpu() for k, v in self.model.state_dict().items()}}, path)
