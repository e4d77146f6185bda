"""Codec-training timing (not the contract bench): one training step of a body-part RVQ-VAE at the reference's batch, 128 clips x 64 frames
(rvq_beatx_train.py:94-95), for the three BEAT-X parts, on the HIP kernels (rvq_training.RVQTrainer) and as the fp32 torch restatement
(tests/rvq_train_ref.py: the ops the reference's modules launch, eager, on PyTorch-ROCm).

    python scripts/bench_rvq_train.py [--clips 128] [--frames 64] [--rounds 5] [--reps 5]

Device-event time; both sides warmed up, then timed in ALTERNATING rounds in this one process; the median round is reported with the spread.
  HIP fwd+bwd   forward (three-product convolutions), quantiser with its EMA update, backward          } the same work as the
  torch fwd+bwd the restatement's forward + autograd backward on the same draws (no optimiser step)    } line below it
  HIP step      fwd+bwd + Adam (optim.ClipAdam): what RVQTrainer.step costs
Then ONE more HIP step with an event pair around every C ABI call gives the split by entry point (the events serialise nothing - one stream -
but the pass is not the one the step time comes from)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import _lib, rvq_training, rvqvae, synth          # noqa: E402
from tests import rvq_train_ref as ref                                # noqa: E402

DIMS = {"upper": 78, "hands": 180, "lower_trans": 57}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


class Split:
    """Stands in for the loaded library during one step: an event pair around every entry point that launches."""

    def __init__(self, lib):
        self.lib, self.events, self.convs = lib, [], 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith(("syn_vq_", "syn_opt_")) or name in ("syn_vq_quantize_groups", "syn_vq_train_loss_parts", "syn_opt_blocks"):
            return fn

        def call(*a):
            label = name
            if name == "syn_vq_conv1d":                                  # the step issues its 33 x 3 forward products first, then the 32 data gradients
                self.convs += 1
                label = "syn_vq_conv1d (forward, 3 products each)" if self.convs <= 99 else "syn_vq_conv1d (data gradient)"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.events.append((label, e0, e1))
            return rc
        return call

    def table(self):
        # the labels above go by call order: 33 convolutions x 3 forward products, then 32 data gradients - anything else and the table would lie
        assert self.convs == 131, f"{self.convs} syn_vq_conv1d calls in a step, 131 expected: update the labels of Split to the step's new call order"
        torch.cuda.synchronize()
        out = {}
        for label, e0, e1 in self.events:
            ms, n = out.get(label, (0.0, 0))
            out[label] = (ms + e0.elapsed_time(e1), n + 1)
        return sorted(out.items(), key=lambda kv: -kv[1][0])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--clips", type=int, default=128)
    p.add_argument("--frames", type=int, default=64)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    dev = torch.device("cuda")
    print(f"codec training step, {a.clips} clips x {a.frames} frames, {a.rounds} alternating rounds of {a.reps} steps, device-event ms per step (median [min .. max])")
    for part, dim in DIMS.items():
        sd = synth.synth_vq_state_dict(dim)
        model = rvqvae.build(dim)
        model.load_state_dict(sd)
        tr = rvq_training.RVQTrainer(model.to(dev), warm_up_iter=0, seed=1)
        gsd = {k: v.to(dev) for k, v in sd.items()}
        st = ref.new_state()
        motion = synth.synth_vq_motion(a.clips, a.frames, dim).to(dev)
        torch.manual_seed(1)
        draws = tr.draw(a.clips, a.frames, dev)
        draws["start"] = None
        draws["gumbel"] = [torch.empty(a.clips * a.frames // 4, 512, device=dev).exponential_().log_().neg_() for _ in range(6)]
        hip_fb = lambda: tr.forward_backward(motion, draws)
        hip_step = lambda: tr.step(motion, draws)
        torch_fb = lambda: ref.train_step(gsd, st, motion, draws)
        for fn in (hip_fb, hip_step, torch_fb):                          # warm-up: code objects, workspaces, the library's algorithm choices
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        res = {"HIP fwd+bwd": [], "torch fwd+bwd": [], "HIP step": []}
        for _ in range(a.rounds):
            res["HIP fwd+bwd"].append(timed(hip_fb, a.reps))
            res["torch fwd+bwd"].append(timed(torch_fb, a.reps))
            res["HIP step"].append(timed(hip_step, a.reps))
        print(f"\n{part} (dim {dim})")
        for k, v in res.items():
            print(f"  {k:14s} {statistics.median(v):8.3f}  [{min(v):8.3f} .. {max(v):8.3f}]")
        print(f"  torch / HIP (fwd+bwd, medians): {statistics.median(res['torch fwd+bwd']) / statistics.median(res['HIP fwd+bwd']):.2f}x")
        load = _lib.load
        split = Split(load())
        _lib.load = lambda: split                                        # every caller asks _lib.load() for the library at each call
        try:
            hip_step()
        finally:
            _lib.load = load
        tab = split.table()
        total = sum(ms for _, (ms, _) in tab)
        print(f"  split of one HIP step by entry point (sum {total:.3f} ms):")
        for label, (ms, n) in tab:
            print(f"    {label:44s} {ms:8.3f} ms  {100 * ms / total:5.1f} %  ({n} calls)")


if __name__ == "__main__":
    main()
