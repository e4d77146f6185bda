"""Hazard weights for the denoising-step kernels: the synthetic state_dict (tests/refmodel.py) with a few entries edited so that one
evaluation reaches the ranges trained checkpoints reach and `randn * fan_in**-0.5` weights never do - large fc1 pre-activations, peaked
softmaxes, outlier channels in the residual stream, a residual stream far from zero mean.  Test infrastructure, shared by
tests/test_ranges_host.py (CPU: the lane-level model, and pins that every hazard is actually reached) and tests/test_gpu_ranges.py."""
import torch
import torch.nn.functional as F

from oracle import denoiser_ref as dr
from tests.refmodel import synth_state_dict

CASES = ("gelu", "sharp", "massive", "shifted")
GELU_BLOCKS = ((1, 12.0), (4, 16.0), (6, 24.0))        # (block, magnitude added to 16 fc1 biases and subtracted from 16 others)
SHARP_BLOCKS, SHARP_GAIN = (2, 5), 4.0                 # q and k rows of attn.qkv.weight times 4: logits times 16
MASSIVE_SHIFT, MASSIVE_SPIKE = 8.0, 100.0              # block 0's attn.proj.bias: + 8 everywhere, +- 100 on two channels each
SHIFTED_SHIFT = 30.0                                   # block 0's attn.proj.bias: + 30 everywhere


def hazard_state_dict(case, variant="beatx"):
    """A fresh copy of `synth_state_dict(variant)` with the edits of one hazard case (deterministic: one generator, seed 123)."""
    sd = {k: v.clone() for k, v in synth_state_dict(variant).items()}
    g = torch.Generator().manual_seed(123)
    if case == "gelu":
        for blk, mag in GELU_BLOCKS:
            perm = torch.randperm(1024, generator=g)
            b = sd[f"mytimmblocks.{blk}.mlp.fc1.bias"]
            b[perm[:16]] += mag
            b[perm[16:32]] -= mag
    elif case == "sharp":
        for blk in SHARP_BLOCKS:
            sd[f"mytimmblocks.{blk}.attn.qkv.weight"][:1024] *= SHARP_GAIN
    elif case == "massive":
        perm = torch.randperm(512, generator=g)
        b = sd["mytimmblocks.0.attn.proj.bias"]
        b += MASSIVE_SHIFT
        b[perm[:2]] += MASSIVE_SPIKE
        b[perm[2:4]] -= MASSIVE_SPIKE
    elif case == "shifted":
        sd["mytimmblocks.0.attn.proj.bias"] += SHIFTED_SHIFT
    else:
        raise ValueError(f"unknown hazard case {case!r}: one of {CASES}")
    return sd


def block_ranges(sd, h, i):
    """What block i of the oracle (oracle/denoiser_ref.block, same operations) sees on its way from the residual stream h (B, T, 512):
    the largest |logit| and the median top probability of its softmaxes, the largest |fc1 pre-activation| and how many lie beyond 10.5."""
    p = f"mytimmblocks.{i}."
    B, N, C = h.shape
    z = F.layer_norm(h, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
    qkv = F.linear(z, sd[p + "attn.qkv.weight"]).reshape(B, N, 3, dr.N_HEADS, C // dr.N_HEADS).permute(2, 0, 3, 1, 4)
    logits = qkv[0] @ qkv[1].transpose(-1, -2) * (C // dr.N_HEADS) ** -0.5
    prob = logits.softmax(-1)
    a = (prob @ qkv[2]).transpose(1, 2).reshape(B, N, C)
    x = h + F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    pre = F.linear(F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-5), sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])
    return {"logit": float(logits.abs().max()), "top_prob": float(prob.max(-1).values.median()),
            "fc1": float(pre.abs().max()), "fc1_beyond": int((pre.abs() > 10.5).sum())}


def stream_ranges(h):
    """Of a residual stream (B, T, 512): the largest |value|, how many channels lie beyond |80| at every token, the smallest share of a token's
    variance that its four largest deviations carry, and the largest mean^2 / variance of a token."""
    mean, var = h.mean(-1), h.var(-1, unbiased=False)
    dev2 = (h - mean[..., None]) ** 2
    return {"abs": float(h.abs().max()), "outlier_channels": int((h.abs().amin((0, 1)) > 80).sum()),
            "outlier_share": float((dev2.topk(4, -1).values.sum(-1) / dev2.sum(-1)).min()),
            "mean2_over_var": float((mean * mean / var).max())}
