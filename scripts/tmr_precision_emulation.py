#!/usr/bin/env python3
"""CPU emulation of the TMR stack's operand rounding (lab notebook): which operands of syn_tmr_encode must be split into
hi + lo bf16 to meet the 5e-3 per-clip bound on `loc`.  Each GEMM / attention product is computed in fp32 from operands rounded the way a
variant would feed the MFMAs (0: one bf16, 1: hi + lo bf16, 2: fp32), against torch's fp32 nn.TransformerEncoder on the same seeded
weights (synth.synth_tmr_state_dict) and inputs (synth.synth_tmr_motion(8, 128), full length).  CPU only, ~1 minute.

    python scripts/tmr_precision_emulation.py
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import synth, tmr  # noqa: E402

D = tmr.D


def rounded(t, mode):
    if mode == 2:
        return t
    hi = t.bfloat16().float()
    return hi if mode == 0 else hi + (t - hi).bfloat16().float()


def emulate(sd, pe, feat, split_act, split_w, split_attn):
    B, L, _ = feat.shape
    mm = lambda a, w: rounded(a, split_act) @ rounded(w, split_w).T
    x = mm(feat.reshape(-1, feat.shape[2]), sd["skel_embedding.weight"]).reshape(B, L, D) + sd["skel_embedding.bias"]
    x = torch.cat([sd["mu_token"].expand(B, 1, D), sd["logvar_token"].expand(B, 1, D), x], 1) + pe[:L + 2]
    S = L + 2
    for i in range(tmr.LAYERS):
        p = lambda k: sd[f"seqTransEncoder.layers.{i}.{k}"]
        qkv = mm(x.reshape(-1, D), p("self_attn.in_proj_weight")) + p("self_attn.in_proj_bias")
        q, k, v = qkv.reshape(B, S, 3, tmr.HEADS, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(rounded(q, split_attn) @ rounded(k, split_attn).transpose(-1, -2) / 8, -1)
        o = (rounded(a, split_attn) @ rounded(v, split_attn)).permute(0, 2, 1, 3).reshape(-1, D)
        h = F.layer_norm(x.reshape(-1, D) + mm(o, p("self_attn.out_proj.weight")) + p("self_attn.out_proj.bias"), (D,), p("norm1.weight"), p("norm1.bias"))
        f = F.gelu(mm(h, p("linear1.weight")) + p("linear1.bias"))
        x = F.layer_norm(h + mm(f, p("linear2.weight")) + p("linear2.bias"), (D,), p("norm2.weight"), p("norm2.bias")).reshape(B, S, D)
    return x[:, 0]


def main():
    m = tmr.ActorAgnosticEncoder(nfeats=synth.TMR_NFEATS)
    m.load_state_dict(synth.synth_tmr_state_dict(m))
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    pe = sd["sequence_pos_encoding.pe"][:, 0]
    feat = synth.synth_tmr_motion(8, 128)
    with torch.no_grad():
        xs = F.linear(feat, sd["skel_embedding.weight"], sd["skel_embedding.bias"]).permute(1, 0, 2)
        xs = torch.cat([sd["mu_token"].expand(1, 8, D), sd["logvar_token"].expand(1, 8, D), xs], 0) + pe[:130, None]
        want = m.seqTransEncoder(xs)[0]
        print("GEMM activations / GEMM weights / attention operands (0 bf16, 1 hi+lo bf16, 2 fp32): worst clip rel-L2 of loc")
        for cfg in [(2, 2, 2), (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1)]:
            got = emulate(sd, pe, feat, *cfg)
            err = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
            print(f"  {cfg}: {err:.2e}")


if __name__ == "__main__":
    main()
