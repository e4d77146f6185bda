#!/usr/bin/env python3
"""CPU emulation of the HIP DistilBERT's operand rounding: which operands of syn_bert_encode must be split into hi + lo bf16
for the hidden states, and `loc` / `scale` behind them, to stay inside the text encoder's bounds (5e-3 on loc, 1e-2 on scale).  Each GEMM /
attention product is computed in fp32 from operands rounded the way a variant would feed the MFMAs (0: one bf16, 1: hi + lo bf16, 2: fp32),
against transformers' fp32 DistilBertModel on the seeded synthetic directories (synth.synth_tmr_text_model, 2 and 6 layers).  `restate` at
(2, 2, 2) is the plain fp32 restatement of the model (tests/test_distilbert_host.py holds it to 1e-5 of transformers').  CPU only, ~1 minute.

    python scripts/distilbert_precision_emulation.py
"""
import os
import sys
import tempfile

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


def restate(sd, ids, mask, n_layers, split_act, split_w, split_attn):
    """DistilBertModel.forward's last_hidden_state (B, L, 768) from its state_dict `sd`, operands rounded per mode."""
    B, L = ids.shape
    mm = lambda a, w: rounded(a, split_act) @ rounded(w, split_w).T
    x = sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.position_embeddings.weight"][:L]
    x = F.layer_norm(x, (768,), sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], 1e-12).reshape(-1, 768)
    bias = torch.where(mask[:, None, None, :] > 0, 0.0, float("-inf"))
    for i in range(n_layers):
        p = lambda k: sd[f"transformer.layer.{i}.{k}"]
        lin = lambda a, n: mm(a, p(n + ".weight")) + p(n + ".bias")
        heads = lambda t: t.reshape(B, L, 12, 64).permute(0, 2, 1, 3)
        q, k, v = heads(lin(x, "attention.q_lin")), heads(lin(x, "attention.k_lin")), heads(lin(x, "attention.v_lin"))
        a = torch.softmax(rounded(q, split_attn) @ rounded(k, split_attn).transpose(-1, -2) / 8 + bias, -1)
        o = (rounded(a, split_attn) @ rounded(v, split_attn)).permute(0, 2, 1, 3).reshape(-1, 768)
        h = F.layer_norm(x + lin(o, "attention.out_lin"), (768,), p("sa_layer_norm.weight"), p("sa_layer_norm.bias"), 1e-12)
        f = F.gelu(lin(h, "ffn.lin1"))
        x = F.layer_norm(h + lin(f, "ffn.lin2"), (768,), p("output_layer_norm.weight"), p("output_layer_norm.bias"), 1e-12)
    return x.reshape(B, L, 768)


def stack(sd, hidden, mask, split_act, split_w, split_attn):
    """The TMR stack behind it (syn_tmr_encode's arithmetic at (1, 1, 0)): (mu, logvar)."""
    B, L, _ = hidden.shape
    pe = sd["sequence_pos_encoding.pe"][:, 0]
    mm = lambda a, w: rounded(a, split_act) @ rounded(w, split_w).T
    x = mm(F.relu(hidden).reshape(-1, 768), sd["projection.1.weight"]).reshape(B, L, D) + sd["projection.1.bias"]
    x = torch.cat([sd["mu_token"].expand(B, 1, D), sd["logvar_token"].expand(B, 1, D), x], 1) + pe[:L + 2]
    S = L + 2
    keys = torch.cat([torch.ones(B, 2, dtype=mask.dtype), mask], 1)
    bias = torch.where(keys[:, None, None, :] > 0, 0.0, float("-inf"))
    for i in range(tmr.LAYERS):
        p = lambda k: sd[f"seqTransEncoder.layers.{i}.{k}"]
        qkv = mm(x.reshape(-1, D), p("self_attn.in_proj_weight")) + p("self_attn.in_proj_bias")
        q, k, v = qkv.reshape(B, S, 3, tmr.HEADS, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(rounded(q, split_attn) @ rounded(k, split_attn).transpose(-1, -2) / 8 + bias, -1)
        o = (rounded(a, split_attn) @ rounded(v, split_attn)).permute(0, 2, 1, 3).reshape(-1, D)
        h = F.layer_norm(x.reshape(-1, D) + mm(o, p("self_attn.out_proj.weight")) + p("self_attn.out_proj.bias"), (D,), p("norm1.weight"), p("norm1.bias"))
        f = F.gelu(mm(h, p("linear1.weight")) + p("linear1.bias"))
        x = F.layer_norm(h + mm(f, p("linear2.weight")) + p("linear2.bias"), (D,), p("norm2.weight"), p("norm2.bias")).reshape(B, S, D)
    return x[:, 0], x[:, 1]


def worst_prompt(got, want, lengths):
    return max(((got[b, :n] - want[b, :n]).norm() / want[b, :n].norm()).item() for b, n in enumerate(lengths))


def worst_row(got, want):
    return ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()


def main():
    variants = [("fp32 restatement", (2, 2, 2)), ("plain bf16 everywhere", (0, 0, 0)), ("split GEMMs, bf16 Q / K / P / V", (1, 1, 0)),
                ("split GEMMs and attention operands", (1, 1, 1))]
    for layers in (2, 6):
        with tempfile.TemporaryDirectory() as td:
            synth.synth_tmr_text_model(td, seed=33, layers=layers)
            m = tmr.DistilbertActorAgnosticEncoder(td, num_layers=4)
        m.load_state_dict(synth.synth_tmr_state_dict(m))
        sd = {k: v.detach() for k, v in m.state_dict().items()}
        bsd = {k[len("text_model."):]: v for k, v in sd.items() if k.startswith("text_model.")}
        sets = [("prompts", list(synth.TMR_PROMPTS)), ("one prompt", [synth.TMR_PROMPT_ONE])]
        if layers == 2:
            sets.append(("ragged 2 .. 254", synth.synth_tmr_prompts(synth.TMR_RAGGED_TOKENS)))
        with torch.no_grad():
            for name, prompts in sets:
                ids, mask = m._tokenize_host(prompts)
                lengths = mask.sum(1).tolist()
                want = m.text_model(input_ids=ids, attention_mask=mask).last_hidden_state
                mu_ref, lv_ref = stack(sd, want, mask, 2, 2, 2)
                print(f"{layers} layers, {name} (token lengths {lengths}): worst prompt rel-L2 of hidden states | loc | scale")
                for label, cfg in variants:
                    got = restate(bsd, ids, mask, layers, *cfg)
                    mu, lv = stack(sd, got, mask, 1, 1, 0)
                    print(f"  {label:36s} {worst_prompt(got, want, lengths):.2e} | {worst_row(mu, mu_ref):.2e} | "
                          f"{worst_row(lv.exp().sqrt(), lv_ref.exp().sqrt()):.2e}")


if __name__ == "__main__":
    main()
