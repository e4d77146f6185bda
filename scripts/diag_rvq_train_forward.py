#!/usr/bin/env python3
"""Why the codec trainer's forward multiplies three times: the same step with `forward_products=1` (a plain bf16 forward) and with
the default 3 (W_hi x_hi + W_lo x_hi + W_hi x_lo), each against the fp32 restatement's autograd fed the run's own indices.  The backward is the
same single-bf16 one in both.  Prints rec_pose's and every weight gradient's rel-L2 error per case, in backward order (last convolution first).

    python scripts/diag_rvq_train_forward.py            # the fixture's two cases, (N 2, T 32, dim 180) and (N 8, T 256, dim 57: 512 latent rows)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import rvq_training, rvqvae, synth          # noqa: E402
from tests import rvq_train_ref as ref                          # noqa: E402
from tests.rvq_train_ref import make_draws                      # noqa: E402
from tests.test_gpu_rvq_train import GOLDEN, STEP_CASES, rel_l2, to_dev   # noqa: E402

DEV = "cuda"


def main():
    fx = ref.load_fixture(GOLDEN)
    for name, (case, shape) in STEP_CASES.items():
        if case is not None:
            n, t, dim = (int(v) for v in fx["cases"][case][:3])
            part, draws = str(fx["parts"][case]), ref.fixture_draws(fx, case, 0)
        else:
            n, t, dim, part, start = shape
            draws = make_draws(n, t, start, 17, [False] * 6)
        pose = synth.synth_vq_pose(part, dim, n=n, t=t, seed=3)
        errs = {}
        for products in (1, 3):
            model = rvqvae.build(dim)
            model.load_state_dict(synth.synth_vq_state_dict(dim))
            got = rvq_training.RVQTrainer(model.to(DEV), forward_products=products).forward_backward(pose.to(DEV), to_dev(draws))
            want = ref.train_step(synth.synth_vq_state_dict(dim), ref.new_state(), pose, draws, forced_idx=got["idx"].cpu().long())
            errs[products] = ({k: rel_l2(got["grads"][k].cpu(), v) for k, v in want["grads"].items()}, rel_l2(got["rec_pose"].cpu(), want["rec_pose"]))
        print(f"\n{name}: rec_pose rel-L2 {errs[1][1]:.3e} (1 product) / {errs[3][1]:.3e} (3 products); gradient rel-L2, gate 3e-2")
        keys = [k for k in reversed(list(errs[1][0])) if k.endswith(".weight")]
        for k in keys:
            a, b = errs[1][0][k], errs[3][0][k]
            print(f"  {k:44s} {a:.4f} {'MISS' if a >= 3e-2 else '    '}   {b:.4f}")
        for p in (1, 3):
            worst = max(errs[p][0], key=errs[p][0].get)
            print(f"  worst with {p} product(s): {errs[p][0][worst]:.4f} ({worst}); tensors at or over 3e-2: {sum(v >= 3e-2 for v in errs[p][0].values())} of {len(errs[p][0])}")


if __name__ == "__main__":
    main()
