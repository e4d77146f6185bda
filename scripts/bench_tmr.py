#!/usr/bin/env python3
"""TMR encoder timing (not the contract bench): the HIP stack (syn_tmr_encode) vs a torch fp32 eager restatement with the same weights
(nn.Linear + tokens + pe + torch's own nn.TransformerEncoder), alternated in one process, device-event time per call.

    python scripts/bench_tmr.py [--reps 20] [--rounds 5]

Cases: the motion encoder at 200 x 128 frames (the h3d yaml's batch) and 32 x 128; the text encoder's stack for 1 and 8 prompts of 16
tokens (768-wide DistilBERT states; DistilBERT itself is PyTorch on both sides and not timed).  FLOP from shapes (the HIP path's work:
the last layer runs queries / out_proj / FFN on rows 0-1 only), TFLOP/s against the 2.5 PFLOP/s dense bf16 peak.  Each MFMA product
issues three bf16 MFMAs (hi / lo split), so the matrix pipe's share is 3x the bf16-equivalent fraction for the GEMMs."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import synth, tmr  # noqa: E402

PEAK_BF16 = 2.5e15


def flops(b, L, k):
    S, R, H = L + 2, b * (L + 2), 2 * b
    f = 2 * b * L * k * 256
    for layer in range(4):
        last = layer == 3
        f += 2 * R * 256 * (512 if last else 768) + (2 * H * 256 * 256 if last else 0)
        q = 2 if last else S
        f += 2 * 2 * b * q * S * 256
        rows = H if last else R
        f += 2 * rows * 256 * 256 + 2 * 2 * rows * 256 * 1024
    return f


class TorchStack(torch.nn.Module):
    def __init__(self, enc, relu):
        super().__init__()
        import copy
        self.lin = copy.deepcopy(enc.get_submodule(enc._in_linear))
        self.tok = torch.nn.Parameter(torch.stack([enc.mu_token.detach(), enc.logvar_token.detach()]))
        self.pe = enc.sequence_pos_encoding.pe.detach().clone()
        self.stack = copy.deepcopy(enc.seqTransEncoder)
        self.relu = relu

    def forward(self, x, pad_mask):
        x = self.lin(torch.relu(x) if self.relu else x).permute(1, 0, 2)
        b = x.shape[1]
        xs = torch.cat([self.tok[:, None].expand(2, b, 256), x], 0) + self.pe[: x.shape[0] + 2]
        f = self.stack(xs, src_key_padding_mask=pad_mask)
        return f[0], f[1]


def time_pair(hip, ref, reps, rounds):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {"hip": [], "torch": []}
    for _ in range(3):
        hip(), ref()
    for _ in range(rounds):
        for name, fn in (("hip", hip), ("torch", ref)):
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda"
    motion = tmr.ActorAgnosticEncoder(nfeats=623)
    motion.load_state_dict(synth.synth_tmr_state_dict(motion))
    motion = motion.to(dev)
    # the text encoder's stack with the motion encoder's layers: same kernel, 768-wide ReLU + Linear front end
    text_stack = tmr.ActorAgnosticEncoder(nfeats=768)
    sd = synth.synth_tmr_state_dict(text_stack)
    text_stack.load_state_dict(sd)
    text_stack._relu_in = 1
    text_stack = text_stack.to(dev)
    cases = [("motion", motion, 200, 128, 623), ("motion", motion, 32, 128, 623), ("text stack", text_stack, 1, 16, 768),
             ("text stack", text_stack, 8, 16, 768)]
    results = []
    with torch.no_grad():
        for name, enc, b, L, k in cases:
            x = torch.randn(b, L, k, device=dev)
            ref = TorchStack(enc, enc._relu_in).to(dev).eval()
            pad = torch.zeros(b, L + 2, dtype=torch.bool, device=dev)
            got, want = enc.encode(x), ref(x, pad)
            err = float((got[0] - want[0]).norm() / want[0].norm())
            t = time_pair(lambda: enc.encode(x), lambda: ref(x, pad), a.reps, a.rounds)
            f = flops(b, L, k)
            hip_med = sorted(t["hip"])[len(t["hip"]) // 2]
            torch_med = sorted(t["torch"])[len(t["torch"]) // 2]
            r = {"case": name, "batch": b, "rows": L, "gflop": round(f / 1e9, 2),
                 "hip_us": round(hip_med, 1), "hip_us_range": [round(min(t["hip"]), 1), round(max(t["hip"]), 1)],
                 "torch_fp32_us": round(torch_med, 1), "torch_us_range": [round(min(t["torch"]), 1), round(max(t["torch"]), 1)],
                 "speedup": round(torch_med / hip_med, 2), "hip_tflops": round(f / hip_med / 1e6, 1),
                 "bf16_peak_fraction": round(f / hip_med / 1e-6 / PEAK_BF16, 4), "loc_rel_l2_vs_torch_fp32": float(f"{err:.3e}")}
            results.append(r)
            print(json.dumps(r), flush=True)
    return results


if __name__ == "__main__":
    main()
