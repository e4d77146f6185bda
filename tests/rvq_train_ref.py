"""Plain fp32 torch restatement of ONE train-mode step of the reference's body-part RVQ-VAE -- TEST INFRASTRUCTURE ONLY
(the role tests/evaluator_ref.py has for the evaluator).  The product path is syntalker_amd/rvq_training.py on the kernels
of csrc/syn_rvq_train.inc; it never imports this module.

Follows, on a reference-keyed state_dict:
  ResConv1DBlock with Dropout(0.2) behind conv2, before the residual add      models/vq/resnet.py:46,50-68
  encoder / decoder stacks                                                      models/vq/encdec.py:4-67
  QuantizeEMAReset.forward in training: init_codebook, Gumbel argmax at temperature 0.5, x_d from the codebook BEFORE the
  update, update_codebook (EMA, usage, reset from _tile), commit = mse(x, x_d)  models/vq/quantizer.py:49-65,107-158
  ResidualVQ.forward in training: quantise dropout, `residual -= quantized.detach()` IN PLACE on the encoder output
                                                                                models/vq/residual_vq.py:112-160
  loss = recons(pred, gt) + commit * commit_loss (velocity term 0)              rvq_beatx_train.py:372-376
Every random input of the step arrives in `draws` (no generator is touched here):
  draws["gumbel"][q]   (rows, 512) Gumbel noise of layer q (None for a layer quantise dropout skips)
  draws["keep"][b]     (N, 512, T_b) bool keep masks of the 12 residual blocks, in execution order (6 encoder, 6 decoder)
  draws["start"]       None (no quantise dropout) or the reference's start_drop_quantize_index: layers > start are skipped
  draws["tile"][q]     list of (512, 512) normal draws `_tile` consumes for layer q, in call order (init_codebook first)
Pinned against tests/golden/rvq_train_step.npz (outputs of the reference itself, tests/golden/make_rvq_train_golden.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

DOWN_T, DEPTH, GROWTH, NUM_Q, NB_CODE, CODE_DIM = 2, 3, 3, 6, 512, 512
P_DROP = 0.2


def new_state():
    """The quantiser state a freshly constructed reference model has (quantizer.py:39-43): nothing initialised."""
    return {"init": [False] * NUM_Q, "code_sum": [None] * NUM_Q, "code_count": [None] * NUM_Q}


def _conv(sd, key, x, stride=1, pad=1, dil=1):
    return F.conv1d(x, sd[key + ".weight"], sd[key + ".bias"], stride=stride, padding=pad, dilation=dil)


def _resnet(sd, key, x, keeps, p_drop):
    for i in range(DEPTH):
        d = GROWTH ** (DEPTH - 1 - i)
        h = _conv(sd, f"{key}.model.{i}.conv1", F.relu(x), pad=d, dil=d)
        h = _conv(sd, f"{key}.model.{i}.conv2", F.relu(h), pad=0)
        h = h * (keeps[i].to(h.dtype) * (1.0 / (1.0 - p_drop)))            # nn.Dropout in training (resnet.py:66)
        x = h + x
    return x


def encoder(sd, x, keeps, p_drop=P_DROP):
    """x (N, D, T) -> (N, 512, T / 4); keeps = the 6 encoder masks."""
    x = F.relu(_conv(sd, "encoder.model.0", x))
    for i in range(DOWN_T):
        x = _conv(sd, f"encoder.model.{2 + i}.0", x, stride=2, pad=1)
        x = _resnet(sd, f"encoder.model.{2 + i}.1", x, keeps[3 * i:3 * i + 3], p_drop)
    return _conv(sd, f"encoder.model.{2 + DOWN_T}", x)


def decoder(sd, x, keeps, p_drop=P_DROP):
    """x (N, 512, T) -> (N, 4 T, D); keeps = the 6 decoder masks."""
    x = F.relu(_conv(sd, "decoder.model.0", x))
    for i in range(DOWN_T):
        x = _resnet(sd, f"decoder.model.{2 + i}.0", x, keeps[3 * i:3 * i + 3], p_drop)
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        x = _conv(sd, f"decoder.model.{2 + i}.2", x)
    x = F.relu(_conv(sd, f"decoder.model.{2 + DOWN_T}", x))
    return _conv(sd, f"decoder.model.{4 + DOWN_T}", x).permute(0, 2, 1)


def tile(x, noise):
    """quantizer.py:49-58 followed by the [:nb_code] every caller takes; `noise` = the first 512 rows of its randn_like."""
    rows, dim = x.shape
    if rows < NB_CODE:
        reps = (NB_CODE + rows - 1) // rows
        std = 0.01 / np.sqrt(dim)
        return x.repeat(reps, 1)[:NB_CODE] + noise * std
    return x[:NB_CODE]


def logits_of(cb, x, gumbel, temperature):
    kw = cb.t()
    dist = torch.sum(x ** 2, dim=-1, keepdim=True) - 2 * torch.matmul(x, kw) + torch.sum(kw ** 2, dim=0, keepdim=True)
    return (-dist) / temperature + gumbel                                    # quantizer.py:27


@torch.no_grad()
def quantizer_layer(cb, st, q, x, gumbel, tile_noise, forced, mu, temperature):
    """One QuantizeEMAReset.forward in training on rows x (no gradient flows through anything here: the caller builds the
    straight-through output).  Updates st / returns (codebook used for x_d, new codebook, idx, perplexity)."""
    tile_noise = list(tile_noise or [])
    if not st["init"][q]:                                                    # init_codebook, quantizer.py:60-65
        cb = tile(x, tile_noise.pop(0) if x.shape[0] < NB_CODE else None)
        st["code_sum"][q], st["code_count"][q], st["init"][q] = cb.clone(), torch.ones(NB_CODE, device=x.device), True
    idx = logits_of(cb, x, gumbel, temperature).argmax(dim=-1) if forced is None else forced
    onehot = torch.zeros(NB_CODE, x.shape[0], device=x.device)
    onehot.scatter_(0, idx.view(1, -1), 1)
    code_sum, code_count = torch.matmul(onehot, x), onehot.sum(dim=-1)      # update_codebook, quantizer.py:107-130
    code_rand = tile(x, tile_noise.pop(0) if x.shape[0] < NB_CODE else None)
    st["code_sum"][q] = mu * st["code_sum"][q] + (1. - mu) * code_sum
    st["code_count"][q] = mu * st["code_count"][q] + (1. - mu) * code_count
    usage = (st["code_count"][q].view(NB_CODE, 1) >= 1.0).float()
    new_cb = usage * (st["code_sum"][q] / st["code_count"][q].view(NB_CODE, 1)) + (1 - usage) * code_rand
    prob = code_count / torch.sum(code_count)
    return cb, new_cb, idx, torch.exp(-torch.sum(prob * torch.log(prob + 1e-7)))


def residual_vq(codebooks, st, x, draws, forced_idx=None, mu=0.99, temperature=0.5):
    """ResidualVQ.forward in training on the encoder output x (N, 512, T), which it modifies IN PLACE as the reference does
    (residual_vq.py:146).  codebooks: list of 6 (512, 512), replaced entry by entry with the updated ones.
    Returns (quantised (N, 512, T), indices (N * T, 6) with -1 in skipped layers, commit loss, perplexity, n_active)."""
    n, c, t = x.shape
    start = draws.get("start")
    n_active = NUM_Q if start is None else start + 1
    residual, out = x, 0.
    idxs, losses, perps = [], [], []
    for q in range(NUM_Q):
        if q >= n_active:
            idxs.append(torch.full((n * t,), -1, dtype=torch.long, device=x.device))
            continue
        rows = residual.permute(0, 2, 1).reshape(n * t, c)                  # preprocess: a copy
        used, codebooks[q], idx, perp = quantizer_layer(codebooks[q], st, q, rows.detach(), draws["gumbel"][q], draws["tile"][q],
                                                        None if forced_idx is None else forced_idx[:, q].long(), mu, temperature)
        xd = F.embedding(idx, used)
        losses.append(F.mse_loss(rows, xd.detach()))
        quantized = (rows + (xd - rows).detach()).view(n, t, c).permute(0, 2, 1).contiguous()
        residual -= quantized.detach()
        out = out + quantized
        idxs.append(idx)
        perps.append(perp)
    return out, torch.stack(idxs, dim=-1), sum(losses) / len(losses), sum(perps) / len(perps), n_active


def recons_loss(kind, pred, gt):
    return {"l2": F.mse_loss, "l1": F.l1_loss, "l1_smooth": F.smooth_l1_loss}[kind](pred, gt)


def train_step(sd, st, motion, draws, forced_idx=None, commit=0.02, recons="l2", mu=0.99, temperature=0.5, p_drop=P_DROP, with_grads=True):
    """Forward and backward of one training step.  sd: reference-keyed state_dict (codebooks included; left untouched), st: quantiser
    state (`new_state()`; updated in place), motion (N, T, D).  Returns a dict: rec_pose, latent (the encoder output before the quantiser
    touches it), xq, idx, loss / recons / commit / perplexity, n_active, codebooks (the updated ones) and grads (name -> tensor)."""
    params = {k: v.detach().clone().float().requires_grad_(with_grads) for k, v in sd.items() if "codebook" not in k}
    codebooks = [sd[f"quantizer.layers.{q}.codebook"].detach().clone().float() for q in range(NUM_Q)]
    with torch.set_grad_enabled(with_grads):
        lat = encoder(params, motion.permute(0, 2, 1).float(), draws["keep"][:6], p_drop)
        latent = lat.detach().clone()
        xq, idx, commit_loss, perp, n_active = residual_vq(codebooks, st, lat, draws, forced_idx, mu, temperature)
        rec = decoder(params, xq, draws["keep"][6:], p_drop)
        rl = recons_loss(recons, rec, motion.float())
        loss = rl + commit * commit_loss
        grads = {}
        if with_grads:
            loss.backward()
            grads = {k: v.grad.detach() for k, v in params.items()}
    return {"rec_pose": rec.detach(), "latent": latent.permute(0, 2, 1).contiguous(), "xq": xq.detach().permute(0, 2, 1).contiguous(), "idx": idx,
            "loss": loss.detach(), "recons": rl.detach(), "commit": commit_loss.detach(), "perplexity": perp, "n_active": n_active,
            "codebooks": codebooks, "grads": grads}


def make_draws(n, t, start, seed, init, keep=True):
    """Draws for shapes the fixture does not hold, from a CPU generator: Gumbel noise -log(-log(u)) per active layer, the 12 keep masks
    (`keep=False`: none, for the quantiser alone) and `_tile`'s (512, 512) normals - one per call, two for a layer that is not initialised
    yet, none at 512 rows and more."""
    g = torch.Generator().manual_seed(seed)
    rows, n_active = n * t // 4, NUM_Q if start is None else start + 1
    u = lambda *s: torch.rand(*s, generator=g).clamp_(1e-20, 1.0)
    gumbel = [-torch.log((-torch.log(u(rows, NB_CODE))).clamp_min(1e-20)) if q < n_active else None for q in range(NUM_Q)]
    masks = [torch.rand(n, CODE_DIM, tb, generator=g) >= P_DROP for tb in (t // 2,) * 3 + (t // 4,) * 6 + (t // 2,) * 3] if keep else []
    return {"gumbel": gumbel, "keep": masks, "start": start,
            "tile": [[torch.randn(NB_CODE, CODE_DIM, generator=g) for _ in range(1 if init[q] else 2)] if q < n_active and rows < NB_CODE else []
                     for q in range(NUM_Q)]}


# ---- judging the quantiser at row counts where an fp32 distance chain may not be held to "indices equal" -------------------------
def layer_inputs(latent, codebooks, init, idx, n_active):
    """The fp32 rows every active layer reads and the codebook it quantises with, along the given picks: residual_vq.py:146 as the
    kernel and the restatement both write it, r - (r + (c - r)) - gathers and single roundings, so equal bit for bit on any device.
    latent (rows, 512), idx (rows, 6).  A layer that is not initialised uses its own first 512 input rows (512 rows and more only)."""
    r, out = latent.float().clone(), []
    for q in range(n_active):
        assert init[q] or r.shape[0] >= NB_CODE
        cb = codebooks[q].float() if init[q] else r[:NB_CODE].clone()
        out.append((r.clone(), cb))
        xd = cb[idx[:, q].long()]
        r = r - (r + (xd - r))
    return out


def judge_picks(latent, codebooks, init, idx, gumbel, n_active, temperature=0.5):
    """Per active layer, in fp64 along the picks `idx` (layer q's input = the latent minus the codes picked before it): the top-2 gap of
    the logits -dist / temperature + gumbel, the fp64 argmax, how far the pick's logit falls short of the best one, and the bound
    tau = 2 * 512 * 2^-24 * (|x| + max |c|)^2 / temperature - the worst case of the three 512-term fp32 sums in |x|^2 - 2 x.c + |c|^2
    (each at most 512 u times a sum of magnitudes that (|x| + |c|)^2 bounds, twice for the two roundings per term), over the temperature."""
    r, out = latent.double().clone(), []
    for q in range(n_active):
        cb = codebooks[q].double() if init[q] else r[:NB_CODE].clone()
        logits = logits_of(cb, r, gumbel[q].double(), temperature)
        top = logits.topk(2, dim=-1)
        picked = logits.gather(1, idx[:, q:q + 1].long()).squeeze(1)
        tau = 2 * CODE_DIM * 2.0 ** -24 * (r.norm(dim=-1) + cb.norm(dim=-1).max()) ** 2 / temperature
        out.append({"gap": top.values[:, 0] - top.values[:, 1], "argmax": top.indices[:, 0], "short": top.values[:, 0] - picked, "tau": tau})
        r = r - cb[idx[:, q].long()]
    return out


def check_picks(judged, idx, cap=0.03):
    """The condition on the inputs first (at most `cap` of the row-layers nearer a tie than tau), then the picks: the fp64 argmax where
    the gap is at least tau, within tau of the best logit elsewhere.  Returns the near-tie share."""
    near = torch.stack([j["gap"] < j["tau"] for j in judged], dim=-1)
    share = float(near.double().mean())
    assert share <= cap, f"near-tie share {share:.4f} over {cap}: take another seed"
    for q, j in enumerate(judged):
        clear = ~near[:, q]
        wrong = (idx[:, q].long() != j["argmax"]) & clear
        assert not bool(wrong.any()), (q, wrong.nonzero().flatten()[:8].tolist())
        assert bool((j["short"][near[:, q]] <= j["tau"][near[:, q]]).all()), q
    return share


def quantiser_step_ref(latent, codebooks, code_sum, code_count, init, draws, idx, mutate=None):
    """One restatement step of the quantiser alone from a given state, fed the picks `idx`; latent (N, T', 512).  Returns xq (N, T', 512),
    the updated codebooks / code_sum / code_count (lists over the active layers), commit, perplexity and n_active.
    mutate (sharpness checks only): "second_chunk" leaves rows 256 .. 511 out of the per-code sums and counts, "noise" adds `_tile`'s noise
    term to the reset rows although there are 512 rows or more."""
    st = {"init": list(init), "code_sum": [s.clone() for s in code_sum], "code_count": [c.clone() for c in code_count]}
    cbs = [c.clone() for c in codebooks]
    if mutate is None:
        xq, _, commit, perp, n_active = residual_vq(cbs, st, latent.permute(0, 2, 1).clone().float(), draws, forced_idx=idx)
        return {"xq": xq.permute(0, 2, 1).contiguous(), "codebooks": cbs[:n_active], "code_sum": st["code_sum"][:n_active],
                "code_count": st["code_count"][:n_active], "commit": commit, "perplexity": perp, "n_active": n_active}
    n_active = NUM_Q if draws.get("start") is None else draws["start"] + 1
    rows = latent.reshape(-1, CODE_DIM).float()
    out = {"codebooks": [], "code_sum": [], "code_count": []}
    for q, (x, cb) in enumerate(layer_inputs(rows, cbs, init, idx, n_active)):
        s_old, n_old = (cb.clone(), torch.ones(NB_CODE)) if not init[q] else (st["code_sum"][q], st["code_count"][q])
        onehot = torch.zeros(NB_CODE, x.shape[0]).scatter_(0, idx[:, q].long().view(1, -1), 1)
        if mutate == "second_chunk":
            onehot[:, 256:512] = 0
        s_new, n_new = 0.99 * s_old + (1. - 0.99) * (onehot @ x), 0.99 * n_old + (1. - 0.99) * onehot.sum(-1)
        rnd = x[:NB_CODE] + (torch.randn(NB_CODE, CODE_DIM, generator=torch.Generator().manual_seed(q)) * (0.01 / np.sqrt(CODE_DIM)) if mutate == "noise" else 0.)
        usage = (n_new.view(-1, 1) >= 1.0).float()
        out["codebooks"].append(usage * (s_new / n_new.view(-1, 1)) + (1 - usage) * rnd)
        out["code_sum"].append(s_new)
        out["code_count"].append(n_new)
    return out


def quantiser_latents(sd, n, t4, seed):
    """(n, t4, 512) latent frames at the scale the quantiser sees in training (|x| ~ 0.25): the restatement's encoder, dropout off, on
    synth.synth_vq_pose.  Only the encoder needs a pose: `RVQTrainer.quantize` takes (N, T', 512) latent frames as they are."""
    from syntalker_amd import synth
    dim = sd["encoder.model.0.weight"].shape[1]
    pose = synth.synth_vq_pose("lower_trans", dim, n=n, t=4 * t4, seed=seed)
    ones = [torch.ones(n, CODE_DIM, tb, dtype=torch.bool) for tb in (2 * t4,) * 3 + (t4,) * 3]
    with torch.no_grad():
        return encoder({k: v.float() for k, v in sd.items()}, pose.permute(0, 2, 1).float(), ones, p_drop=0.0).permute(0, 2, 1).contiguous()


def initialised_state(sd, seed=5):
    """An EMA state in which every layer has work to do on its first step: the codebooks of `sd`, code_count uniform in [0.5, 3] (a sixth of
    the codes start below the usage threshold of 1), code_sum = codebook x count.  Returns (code_sum (6, 512, 512), code_count (6, 512))."""
    count = 0.5 + 2.5 * torch.rand(NUM_Q, NB_CODE, generator=torch.Generator().manual_seed(seed))
    cbs = torch.stack([sd[f"quantizer.layers.{q}.codebook"].float() for q in range(NUM_Q)])
    return cbs * count.unsqueeze(-1), count


# ---- the weight gradient in fp64 ---------------------------------------------------------------------------------------------------
def wgrad_ref(dy, x, taps, stride, dil, pad, up, relu_in, mutate=None):
    """dW[co][ci][tap] = sum_{n,t} dy[n,t,co] x[n, (t stride + tap dil - pad) >> up, ci] in fp64, zero outside the clip's own frames;
    dy (clips, t_out, cout), x (clips, t_in, cin).  Returns (dW, sum of |dy x| per element, db, sum of |dy| per channel).
    mutate (sharpness checks only): "dilation" shifts by the tap index alone, "clip" reads the flat buffer across clip boundaries,
    "up" drops the >> up, "last" leaves the last position of a partial 64-position chunk out."""
    dy, x = dy.double(), x.double()
    if relu_in:
        x = x.clamp_min(0)
    clips, t_out, cout = dy.shape
    t_in, cin = x.shape[1], x.shape[2]
    K = clips * t_out
    if mutate == "last" and K % 64:
        dy = dy.clone()
        dy.view(K, cout)[K - 1] = 0
    flat = x.reshape(clips * t_in, cin)
    dw, mag = torch.zeros(cout, cin, taps, dtype=torch.float64), torch.zeros(cout, cin, taps, dtype=torch.float64)
    t = torch.arange(t_out)
    for tap in range(taps):
        u = t * stride + tap * (1 if mutate == "dilation" else dil) - pad
        src = u if mutate == "up" else u >> up
        ok = (u >= 0) & (u < (t_in << up)) & (src < t_in)
        rows = torch.arange(clips).view(-1, 1) * t_in + src.view(1, -1)                   # (clips, t_out) rows of the flat buffer
        if mutate == "clip":
            valid = (rows >= 0) & (rows < clips * t_in)
        else:
            valid = ok.view(1, -1).expand(clips, -1)
        xg = flat[rows.clamp(0, clips * t_in - 1)] * valid.unsqueeze(-1)                 # (clips, t_out, cin)
        dw[:, :, tap] = torch.einsum("nto,nti->oi", dy, xg)
        mag[:, :, tap] = torch.einsum("nto,nti->oi", dy.abs(), xg.abs())
    return dw, mag, dy.sum(dim=(0, 1)), dy.abs().sum(dim=(0, 1))


# (taps, stride, dilation, pad, up, relu_in) of every weight gradient RVQTrainer.forward_backward issues
WGRAD_GEOMETRY = {"k3": (3, 1, 1, 1, 0, 0), "k3_relu": (3, 1, 1, 1, 0, 1), "dil3": (3, 1, 3, 3, 0, 1), "dil9": (3, 1, 9, 9, 0, 1), "k4s2": (4, 2, 1, 1, 0, 0),
                  "up": (3, 1, 1, 1, 1, 0), "k1": (1, 1, 1, 0, 0, 1)}
# (geometry, cout, ldy, cin, ldx, clips, t_out).  K = clips * t_out: 3 (odd, fewer frames than any dilation), 8, 64, 96 (second chunk half full),
# 65 / 130 (one / two positions spill into a new chunk), 512; every geometry meets an odd K and a K of several chunks with a partial tail -
# but for `up`, whose t_out is even (26 = 2 x 13 frames, K 130; 2 frames, K 6).  Clips >= 2 wherever dilation >= t_out.  128 x 192 channels
# are 2 x 3 tiles; 57 in a pitch of 64 and 180 in a pitch of 192 end on a tile that is part padding.
WGRAD_CASES = [
    ("k3", 512, 512, 512, 512, 3, 1), ("k3", 512, 512, 512, 512, 8, 64), ("k3", 128, 128, 192, 192, 5, 13),
    ("k3", 512, 512, 57, 64, 2, 65), ("k3", 128, 128, 57, 64, 3, 1), ("k3", 57, 64, 512, 512, 5, 13), ("k3", 57, 64, 192, 192, 2, 4),
    ("k3", 128, 128, 180, 192, 3, 32), ("k3", 512, 512, 180, 192, 5, 13),
    ("k3_relu", 128, 128, 192, 192, 5, 13), ("k3_relu", 128, 128, 192, 192, 3, 1), ("k3_relu", 128, 128, 192, 192, 1, 64),
    ("dil3", 128, 128, 192, 192, 3, 1), ("dil3", 128, 128, 192, 192, 2, 65), ("dil3", 128, 128, 192, 192, 2, 4), ("dil3", 128, 128, 192, 192, 5, 13),
    ("dil9", 128, 128, 192, 192, 3, 1), ("dil9", 128, 128, 192, 192, 5, 13), ("dil9", 128, 128, 192, 192, 3, 32), ("dil9", 128, 128, 192, 192, 2, 4),
    ("dil9", 512, 512, 512, 512, 8, 64), ("dil9", 128, 128, 192, 192, 2, 65), ("dil9", 128, 128, 192, 192, 4, 3),
    ("k4s2", 128, 128, 192, 192, 3, 1), ("k4s2", 128, 128, 192, 192, 2, 65), ("k4s2", 128, 128, 192, 192, 1, 64), ("k4s2", 128, 128, 192, 192, 3, 32),
    ("k4s2", 128, 128, 192, 192, 5, 13),
    ("up", 128, 128, 192, 192, 2, 4), ("up", 128, 128, 192, 192, 5, 26), ("up", 128, 128, 192, 192, 1, 64), ("up", 128, 128, 192, 192, 3, 2),
    ("k1", 128, 128, 192, 192, 3, 1), ("k1", 128, 128, 192, 192, 2, 65), ("k1", 128, 128, 192, 192, 5, 13),
]


def wgrad_operands(case, seed=0):
    """dy (clips, t_out, ldy) and x (clips, t_in, ldx) of a WGRAD_CASES entry: asymmetric normal values rounded to bf16 (kept as fp32), the
    padded channels filled too - the kernel may read them, its stores may not show them."""
    geo, cout, ldy, cin, ldx, clips, t_out = case
    taps, stride, dil, pad, up, relu_in = WGRAD_GEOMETRY[geo]
    t_in = t_out * stride if not up else t_out // 2
    g = torch.Generator().manual_seed(1000 * seed + 7 * clips + t_out + cout + cin + dil)
    bf = lambda shift, *s: (torch.randn(*s, generator=g) + shift).to(torch.bfloat16).float()
    return bf(0.25, clips, t_out, ldy), bf(-0.125, clips, t_in, ldx), t_in


def wgrad_bound(mag, k):
    """|got - want| <= 2 K 2^-24 sum |dy x|: bf16 products are exact in fp32, K u bounds any order of the K-term sum, the factor 2 leaves
    room for the matrix unit's internal order."""
    return 2.0 * k * 2.0 ** -24 * mag


def sample(t, stride=97):
    """What the fixture keeps of a large tensor: its norm and every `stride`-th element (97 is prime to every tensor dimension here)."""
    f = t.detach().reshape(-1).float()
    return float(f.norm()), f[::stride].clone()


def lr_at(iteration, lr=2e-4, warm_up_iter=1000, milestones=(50000, 400000), gamma=0.05):
    """Learning rate of the `iteration`-th optimiser step (0-based) of rvq_beatx_train.py:333-381: warm_up_iter - 1 warm-up steps at
    lr * (nb_iter + 1) / (warm_up_iter + 1), nb_iter = 1 .., then MultiStepLR - which, being chainable, continues from the LAST warm-up value."""
    n_warm = max(warm_up_iter - 1, 0)
    if iteration < n_warm:
        return lr * (iteration + 2) / (warm_up_iter + 1)
    base = lr * warm_up_iter / (warm_up_iter + 1) if n_warm else lr
    return base * gamma ** sum(1 for m in milestones if m <= iteration - n_warm)


# ---- the fixture (tests/golden/make_rvq_train_golden.py) -----------------------------------------------------------------------
TILE_SEED = 7919
FIXTURE_FILES = ("rvq_train_step.npz", "rvq_train_step_case1.npz", "rvq_train_step_grads0.npz", "rvq_train_step_grads1.npz")


def tile_noise(seed, call):
    """The first 512 rows of the `call`-th randn_like of `_tile` in the generator run whose fixture stores `seed`."""
    return torch.randn(512, 512, generator=torch.Generator().manual_seed(TILE_SEED * (seed + 1) + call))


def load_fixture(golden_dir):
    """The four files of the fixture as one dict; gradient entries as `c{case}.grad.{names,norms,offsets,samples}`."""
    import os
    out = {}
    for name in FIXTURE_FILES:
        z = np.load(os.path.join(golden_dir, name))
        pre = f"c{name[-5]}.grad." if "grads" in name else ""
        out.update({pre + k: z[k] for k in z.files})
    return out


def fixture_draws(fx, case, step):
    """`draws` of step `step` of case `case`, as train_step takes them."""
    pre, seed = f"c{case}.s{step}.", int(fx["seed"])
    start = int(fx["cases"][case][3])
    g = torch.from_numpy(fx[pre + "gumbel"])
    keep = []
    for b in range(12):
        shape = tuple(int(v) for v in fx[pre + f"keep{b}.shape"])
        keep.append(torch.from_numpy(np.unpackbits(fx[pre + f"keep{b}"])[:int(np.prod(shape))].astype(bool)).view(shape))
    calls = fx[pre + "tile_calls"]
    return {"gumbel": [g[q] if q < g.shape[0] else None for q in range(NUM_Q)], "keep": keep, "start": None if start < 0 else start,
            "tile": [[tile_noise(seed, int(c)) for c in calls[q] if c >= 0] if q < len(calls) else [] for q in range(NUM_Q)]}
