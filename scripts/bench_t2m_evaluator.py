#!/usr/bin/env python3
"""T2M text-motion evaluator timing (not the contract bench): EvaluatorMDMWrapper.get_co_embeddings on the HIP kernels
(syn_t2m_encode_motion / syn_t2m_encode_text) beside the torch fp32 restatement (tests/t2m_evaluator_ref.py: F.conv1d, F.linear and
nn.GRU over packed sequences, which is MIOpen on ROCm - the comparison only, never a product path) on the same GPU, alternated in one
process.  Warm-up calls, then device events around `--reps` back-to-back calls, `--rounds` times; the median round is reported with the
range.  Seeded weights; loader-shaped batches (196 frames, 22 tokens) of mixed lengths.

    python scripts/bench_t2m_evaluator.py [--reps 20] [--rounds 5] [--sizes 32,4096]

One JSON line per size, then one with all of them."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from syntalker_amd import synth, t2m_evaluator  # noqa: E402
from tests import t2m_evaluator_ref as ref  # noqa: E402


def time_pair(fns: dict, reps: int, rounds: int) -> dict:
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    for _ in range(rounds):
        for name, fn in fns.items():
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name].append(ev[0].elapsed_time(ev[1]) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="32,4096")
    a = ap.parse_args()
    dev = "cuda:0"
    state = ref.build_state()
    w = t2m_evaluator.EvaluatorMDMWrapper("humanml", dev, state=state)
    gstate = {k: {n: t.to(dev) for n, t in sd.items()} for k, sd in state.items()}
    grus = {k: ref.make_gru(gstate[k]) for k in ("motion_encoder", "text_encoder")}
    results = []
    with torch.no_grad():
        for n in (int(s) for s in a.sizes.split(",")):
            word, pos, cap_lens, motions, m_lens = synth.synth_t2m_batch(n, 400 + n)
            word, pos, motions = word.to(dev), pos.to(dev), motions.to(dev)
            torch_motion = lambda: ref.motion_embeddings(gstate, motions, m_lens, gru=grus["motion_encoder"])
            torch_text = lambda: ref.text_embeddings(gstate, word, pos, cap_lens, gru=grus["text_encoder"])
            text, motion = w.get_co_embeddings(word, pos, cap_lens, motions, m_lens)
            want_m, want_t = torch_motion(), torch_text()[ref.align_idx(m_lens)]
            t = time_pair({"hip_motion": lambda: w.get_motion_embeddings(motions, m_lens), "torch_motion": torch_motion,
                           "hip_text": lambda: w.text_encoder(word, pos, cap_lens), "torch_text": torch_text}, a.reps, a.rounds)
            r = {"sequences": n, "frames": motions.shape[1], "tokens": word.shape[1], "mean_steps": round(float((m_lens // 4).float().mean()), 1),
                 "max_abs_vs_torch_fp32": {"motion": float(f"{float((motion - want_m).abs().max()):.3e}"),
                                           "text": float(f"{float((text - want_t).abs().max()):.3e}")}}
            for k, v in t.items():
                v = sorted(v)
                r[k + "_ms"] = round(v[len(v) // 2], 3)
                r[k + "_ms_range"] = [round(v[0], 3), round(v[-1], 3)]
            r["motion_us_per_sequence"] = round(1e3 * r["hip_motion_ms"] / n, 2)
            r["speedup_motion"] = round(r["torch_motion_ms"] / r["hip_motion_ms"], 2)
            r["speedup_text"] = round(r["torch_text_ms"] / r["hip_text_ms"], 2)
            results.append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps({"bench": "t2m_evaluator", "reps": a.reps, "rounds": a.rounds, "results": results}), flush=True)
    return results


if __name__ == "__main__":
    main()
