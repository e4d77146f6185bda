#!/usr/bin/env python3
"""DistilBERT timing (not the contract bench): the HIP kernels (syn_bert_encode, text_on_hip=True) vs the module's own `text_model`
(transformers on PyTorch-ROCm, fp32 eager) with the same weights, alternated in one process on one GPU.

    python scripts/bench_distilbert.py [--rounds 5] [--sets 1,200,4096] [--out profiles/distilbert_bench.txt]

Prompt sets of 1, 200 (the h3d yaml's batch: every training step) and 4096 (the evaluator's captions) prompts drawn from the synthetic word
list with ragged lengths (4 .. 24 tokens, seeded), on a 6-layer synthetic DistilBERT (synth.synth_tmr_text_model).  Per set:
  distilbert  device-event time of DistilBERT alone on device-resident ids (HIP: hidden_states; torch: text_model(ids, mask));
  encode      host clock around the whole `encode(prompts)` (tokenizer on the host, copies, DistilBERT, the TMR stack) up to a synchronise;
  graph       encode_ids (DistilBERT + TMR stack) replayed from a captured graph, HIP only;
  kernels     launches per call: HIP from the launch sequence (1 + 7 layers, + 22 for the TMR stack), torch counted by torch.profiler;
  FLOP        what the model needs for the valid tokens, from shapes (per layer 2 T 768 (2304 + 768 + 2 x 3072) + 4 x 768 sum n^2), over time.
Each HIP product issues three bf16 MFMAs (hi + lo split), so the matrix pipe does 3x the FLOP counted here."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import synth, tmr  # noqa: E402

LAYERS = 6


def flops(lengths):
    t, sq = sum(lengths), sum(n * n for n in lengths)
    return LAYERS * (2 * t * 768 * (2304 + 768 + 2 * 3072) + 4 * 768 * sq)


def event_times(fns, reps, rounds):
    """Median and range of device-event milliseconds per call for each of `fns`, alternated round by round after a warm-up of every one."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    for _ in range(rounds):
        for k, fn in fns.items():
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[k].append(ev[0].elapsed_time(ev[1]) / reps)
    return out


def host_times(fns, reps, rounds):
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return out


def med(v):
    return sorted(v)[len(v) // 2]


def torch_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or "not measured"
    except Exception as e:                                     # the count is a by-product; the timings do not depend on it
        return f"not measured ({type(e).__name__})"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", default="1,200,4096")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_distilbert.py measures on the GPU; no device found")
    dev = "cuda"
    with tempfile.TemporaryDirectory() as td:
        synth.synth_tmr_text_model(td, seed=33, layers=LAYERS)
        hip = tmr.DistilbertActorAgnosticEncoder(td, num_layers=4, text_on_hip=True)
        ref = tmr.DistilbertActorAgnosticEncoder(td, num_layers=4)
    sd = synth.synth_tmr_state_dict(hip)
    hip.load_state_dict(sd)
    ref.load_state_dict(sd)
    hip, ref = hip.to(dev), ref.to(dev)
    lines = []
    with torch.no_grad():
        for n in [int(v) for v in a.sets.split(",")]:
            g = torch.Generator().manual_seed(100 + n)
            token_lengths = torch.randint(4, 25, (n,), generator=g).tolist()
            prompts = synth.synth_tmr_prompts(token_lengths, seed=200 + n)
            ids, mask = hip.tokenize(prompts)
            lengths = mask.sum(1, dtype=torch.int32)
            assert lengths.tolist() == token_lengths
            got = hip.hidden_states(ids, lengths)
            want = ref.text_model(input_ids=ids, attention_mask=mask).last_hidden_state * mask[..., None]
            err = max(float((got[b, :k] - want[b, :k]).norm() / want[b, :k].norm()) for b, k in enumerate(token_lengths[:64]))
            reps = max(3, min(100, 90000 // sum(token_lengths)))
            d = event_times({"hip": lambda: hip.hidden_states(ids, lengths),
                             "torch": lambda: ref.text_model(input_ids=ids, attention_mask=mask).last_hidden_state}, reps, a.rounds)
            e = host_times({"hip": lambda: hip.encode(prompts), "torch": lambda: ref.encode(prompts)}, max(1, reps // 4), a.rounds)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                hip.encode_ids(ids, lengths)
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                hip.encode_ids(ids, lengths)
            gt = event_times({"graph": graph.replay}, reps, a.rounds)
            del graph
            f = flops(token_lengths)
            r = {"prompts": n, "tokens": sum(token_lengths), "padded_rows": n * ids.shape[1], "gflop": round(f / 1e9, 2),
                 "distilbert_hip_ms": round(med(d["hip"]), 3), "distilbert_hip_ms_range": [round(min(d["hip"]), 3), round(max(d["hip"]), 3)],
                 "distilbert_torch_fp32_ms": round(med(d["torch"]), 3),
                 "distilbert_torch_ms_range": [round(min(d["torch"]), 3), round(max(d["torch"]), 3)],
                 "distilbert_speedup": round(med(d["torch"]) / med(d["hip"]), 2),
                 "hip_tflops": round(f / med(d["hip"]) / 1e9, 2), "torch_tflops": round(f / med(d["torch"]) / 1e9, 2),
                 "encode_hip_ms": round(med(e["hip"]), 3), "encode_torch_ms": round(med(e["torch"]), 3),
                 "encode_ids_graph_hip_ms": round(med(gt["graph"]), 3),
                 "kernels_hip_distilbert": 1 + 7 * LAYERS, "kernels_hip_encode": 1 + 7 * LAYERS + 22,
                 "kernels_torch_distilbert": torch_kernels(lambda: ref.text_model(input_ids=ids, attention_mask=mask)),
                 "hidden_rel_l2_vs_torch_fp32": float(f"{err:.3e}")}
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
