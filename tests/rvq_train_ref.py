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
