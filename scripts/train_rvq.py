#!/usr/bin/env python3
"""The reference's codec pre-training loop (rvq_beatx_train.py) on this build: one body-part RVQ-VAE trained by `rvq_training.RVQTrainer` on the
HIP kernels - warm-up loop (:333-361), main loop (:367-404), the log line every --print-iter steps, `net_<iter>.pth` checkpoints in the
reference's format ({'net': state_dict}) plus the trainer's own state (EMA sums, init flags, Adam moments) for resuming.

    python scripts/train_rvq.py --body-part upper|hands|lower|lower_trans|whole_trans [--dataname h3d_623] [--data poses.npy]
                                [--total-iter N] [--out-dir DIR] [--batch-size 128] [--window-size 64] [--warm-up-iter 1000] [--seed 123]
                                [--resume trainer_last.pth]

--data   .npy of full pose vectors: (frames, D) - one take - or (clips, frames, D); a batch is --batch-size random windows of --window-size
         frames, reduced to the body part's channels (`rvq_training.body_part_mask`, rvq_beatx_train.py:210-295).  The reference's lmdb data
         loaders are out of scope.  Without --data the loop runs on synthetic motion (synth.synth_vq_motion), as train_from_config.py does.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import rvq_training, rvqvae, synth          # noqa: E402


def parse():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--body-part", required=True, choices=["upper", "hands", "lower", "lower_trans", "whole_trans"])
    p.add_argument("--dataname", default="beatx", help="h3d_623 selects the HumanML3D-623 channel layout")
    p.add_argument("--data", default=None)
    p.add_argument("--total-iter", type=int, default=200000)
    p.add_argument("--warm-up-iter", type=int, default=1000)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--window-size", type=int, default=64)
    p.add_argument("--lr", type=float, default=2e-4)
    p.add_argument("--lr-scheduler", type=int, nargs="+", default=[50000, 400000])
    p.add_argument("--gamma", type=float, default=0.05)
    p.add_argument("--commit", type=float, default=0.02)
    p.add_argument("--recons-loss", default="l2", choices=["l1", "l2", "l1_smooth"])
    p.add_argument("--print-iter", type=int, default=200)
    p.add_argument("--save-iter", type=int, default=10000, help="rvq_beatx_train.py:366: eval_iter * 10")
    p.add_argument("--out-dir", default="output_vqfinal")
    p.add_argument("--resume", default=None)
    p.add_argument("--seed", type=int, default=123)
    return p.parse_args()


class Windows:
    """Random --window-size windows of a pose array, reduced to the body part's channels."""

    def __init__(self, path, mask, window, seed):
        a = np.load(path, mmap_mode="r")
        self.a = a[None] if a.ndim == 2 else a
        if self.a.ndim != 3 or self.a.shape[1] < window or self.a.shape[2] <= max(mask):
            raise SystemExit(f"--data: expected (frames >= {window}, D > {max(mask)}) or (clips, frames, D), got {a.shape}")
        self.mask, self.window, self.rng = np.asarray(mask), window, np.random.default_rng(seed)

    def batch(self, n, dev):
        c = self.rng.integers(0, self.a.shape[0], n)
        s = self.rng.integers(0, self.a.shape[1] - self.window + 1, n)
        x = np.stack([np.asarray(self.a[i, j:j + self.window])[:, self.mask] for i, j in zip(c, s)]).astype(np.float32)
        return torch.from_numpy(x).to(dev)


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("train_rvq.py needs the GPU: the step runs on the HIP kernels only")
    dev = torch.device("cuda")
    torch.manual_seed(a.seed)
    mask = rvq_training.body_part_mask(a.body_part, a.dataname)
    dim = len(mask)
    os.makedirs(a.out_dir, exist_ok=True)
    model = rvqvae.build(dim)
    params = dict(model.named_parameters())
    for name, p in params.items():                                             # nn.Conv1d's default initialisation: U(+-1 / sqrt(fan_in)) for both
        w = params[name.rsplit(".", 1)[0] + ".weight"]
        bound = (w.shape[1] * w.shape[2]) ** -0.5
        torch.nn.init.uniform_(p, -bound, bound)
    trainer = rvq_training.RVQTrainer(model.to(dev), lr=a.lr, commit=a.commit, recons_loss=a.recons_loss, warm_up_iter=a.warm_up_iter,
                                      milestones=tuple(a.lr_scheduler), gamma=a.gamma, seed=a.seed)
    if a.resume:
        trainer.load_state_dict(torch.load(a.resume, map_location=dev))
    data = Windows(a.data, mask, a.window_size, a.seed) if a.data else None
    n_warm = max(a.warm_up_iter - 1, 0)
    total, acc, t0 = n_warm + a.total_iter, [], time.time()
    print(f"{a.body_part} ({a.dataname}): {dim} channels, {n_warm} warm-up + {a.total_iter} steps of {a.batch_size} x {a.window_size}, "
          f"{'synthetic motion' if data is None else a.data}", flush=True)
    while trainer.iteration < total:
        it = trainer.iteration
        gt = data.batch(a.batch_size, dev) if data is not None else synth.synth_vq_motion(a.batch_size, a.window_size, dim, step=it).to(dev)
        out = trainer.step(gt)
        acc.append(torch.stack([out["recons"], out["perplexity"], out["commit"]]))
        warm = it < n_warm
        nb_iter = it + 1 if warm else it - n_warm + 1
        if nb_iter % a.print_iter == 0 or trainer.iteration == total:
            recons, ppl, commit = torch.stack(acc).mean(0).tolist()            # the only host synchronisation of the loop
            acc = []
            lr = rvq_training.lr_at(it, a.lr, a.warm_up_iter, tuple(a.lr_scheduler), a.gamma)
            print(f"{'Warmup' if warm else 'Train'}. Iter {nb_iter} :  lr {lr:.5f} \t Commit. {commit:.5f} \t PPL. {ppl:.2f} \t Recons.  {recons:.5f}"
                  f" \t ({time.time() - t0:.0f} s)", flush=True)
        if not warm and nb_iter % a.save_iter == 0:
            trainer.save_net(os.path.join(a.out_dir, f"net_{nb_iter}.pth"))
    trainer.save_net(os.path.join(a.out_dir, "net_last.pth"))
    torch.save(trainer.state_dict(), os.path.join(a.out_dir, "trainer_last.pth"))
    print("wrote", os.path.join(a.out_dir, "net_last.pth"), "and trainer_last.pth")


if __name__ == "__main__":
    main()
