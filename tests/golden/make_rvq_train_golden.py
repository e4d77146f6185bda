#!/usr/bin/env python3
"""Golden vectors of the reference's RVQ-VAE in TRAINING mode (models/vq/model.py:RVQVAE(...).train(), the model rvq_beatx_train.py
trains), run on CPU in the build container.  Tensor.cuda is made the identity, as in make_vq_golden.py.  Weights are
syntalker_amd.synth.synth_vq_state_dict; poses are synth.synth_vq_pose.

    python tests/golden/make_rvq_train_golden.py            # the two single-step cases
    python tests/golden/make_rvq_train_golden.py --check    # regenerate them and compare the arrays (not the zip files) with the committed ones, bit for bit
    python tests/golden/make_rvq_train_golden.py --loop     # 100 steps of the reference's loop, three seeds (minutes of CPU time: run once)

Single steps: every random input the reference consumes is RECORDED as it is drawn - `gumbel_noise` (quantizer.py:14-16), the keep masks of
the 12 nn.Dropout(0.2) (resnet.py:46), `randn_like` inside `_tile` (quantizer.py:55) - except the quantise-dropout coin and index
(residual_vq.py:112-117), which are SET so that the cases cover both branches:
  case 0: N = 3, T = 16, dim 57, start = None (all six layers), two consecutive steps (the second on initialised codebooks, other pose)
  case 1: N = 2, T = 64, dim 78, start = 2 (layers 3 .. 5 skipped), one step
No optimiser step runs between the two steps of case 0: the pinned quantities are those of forward + backward.
The generator REFUSES a seed at which any row of any layer has a top-2 gap of its sampling logits below 1e-4 of the row's largest logit
magnitude (an index that fp32 summation order could flip) and moves to the next one; the seed used is stored.

--check compares the ARRAYS of a fresh run with the committed ones, bit for bit; the .npz files themselves differ from run to run, because
np.savez_compressed stamps every zip member with the time of writing.

The fixture is kept small BY CHOICE - every file under 1 MiB, a budget this generator sets for itself (the tree's other fixtures run to 4.9 MB;
every clone carries them) and tests/test_rvq_train_host.py holds it to - so (a) the fixture is four files - rvq_train_step.npz (case 0), rvq_train_step_case1.npz and one
rvq_train_step_grads{0,1}.npz per case - which tests/rvq_train_ref.py:load_fixture merges, (b) the (512, 512) normal draws of `_tile`
are stored as the seeds of the generators that drew them (tests/rvq_train_ref.py:tile_noise regenerates them), and (c) gradients, codebooks and code sums
are stored as their norm and every 97th element (tests/rvq_train_ref.py:sample), the 512 code counts in full.
--loop writes rvq_train_loop.npz: the reconstruction loss at steps 1 and 100 for each seed.
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, import_reference  # noqa: E402,F401  (puts the reference tree on sys.path)

from syntalker_amd import synth  # noqa: E402
from tests import rvq_train_ref as ref  # noqa: E402

CASES = ((3, 16, 57, "lower", None, 2), (2, 64, 78, "upper", 2, 1))      # N, T, dim, synth part name, start, steps
LOOP_N, LOOP_T, LOOP_DIM, LOOP_STEPS, LOOP_SEEDS = 8, 32, 78, 100, (1, 2, 3)
GAP = 1e-4


class GapTooSmall(Exception):
    pass


def vq_args():
    return types.SimpleNamespace(num_quantizers=6, shared_codebook=False, quantize_dropout_prob=0.2, mu=0.99)   # rvq_beatx_train.py:299-301, :112


class Recorder:
    """Hooks into the reference's modules; `self.step` collects what one forward draws."""

    def __init__(self, seed, Q, RV):
        self.seed, self.Q, self.RV, self.tile_calls = seed, Q, RV, 0
        self.start = None
        self.reset()
        orig_noise, orig_sample, rec = Q.gumbel_noise, Q.gumbel_sample, self

        def gumbel_noise(t):
            g = orig_noise(t)
            rec.gumbel.append(g.clone())
            return g

        def gumbel_sample(logits, temperature=1., stochastic=False, dim=-1, training=True):
            ind = orig_sample(logits, temperature=temperature, stochastic=stochastic, dim=dim, training=training)
            s = logits / temperature + rec.gumbel[-1]
            assert torch.equal(s.argmax(dim=dim), ind)
            top = s.topk(2, dim=-1).values
            if bool(((top[:, 0] - top[:, 1]) <= GAP * s.abs().max(dim=-1).values).any()):
                raise GapTooSmall()
            return ind

        orig_tile = Q.QuantizeEMAReset._tile

        def tile(qself, x):                                               # the reference's own _tile; its randn_like draw regenerable from a seed
            orig_randn_like = torch.randn_like

            def randn_like(out):
                noise = torch.zeros_like(out)                               # (rows past 512 are cut off by every caller: quantizer.py:62,116)
                noise[:512] = ref.tile_noise(rec.seed, rec.tile_calls)
                rec.tile_log[-1].append(rec.tile_calls)
                rec.tile_calls += 1
                return noise
            torch.randn_like = randn_like
            try:
                return orig_tile(qself, x)
            finally:
                torch.randn_like = orig_randn_like

        orig_fwd = Q.QuantizeEMAReset.forward

        def q_forward(qself, x, return_idx=False, temperature=0.):
            rec.tile_log.append([])
            return orig_fwd(qself, x, return_idx=return_idx, temperature=temperature)

        orig_drop = torch.nn.Dropout.forward

        def drop_forward(dself, x):
            m = orig_drop(dself, torch.ones_like(x))                        # the reference's own draw: 0 or 1 / (1 - p)
            rec.keep.append(m != 0)
            return x * m

        Q.gumbel_noise, Q.gumbel_sample = gumbel_noise, gumbel_sample
        Q.QuantizeEMAReset._tile, Q.QuantizeEMAReset.forward = tile, q_forward
        torch.nn.Dropout.forward = drop_forward
        RV.random = types.SimpleNamespace(random=lambda: 1.0 if rec.start is None else 0.0)
        RV.randrange = lambda a, b: rec.start

    def reset(self):
        self.gumbel, self.keep, self.tile_log = [], [], []


def run_cases(rec, seed):
    from models.vq.model import RVQVAE
    rec.seed, rec.tile_calls = seed, 0
    files = {"main": {"seed": np.int64(seed), "cases": np.array([[n, t, d, -1 if s is None else s, k] for n, t, d, _, s, k in CASES]),
                      "parts": np.array([c[3] for c in CASES])},
             "case1": {}, "grads0": {}, "grads1": {}}
    for ci, (n, t, dim, part, start, steps) in enumerate(CASES):
        out, gout = files["main" if ci == 0 else "case1"], files[f"grads{ci}"]
        torch.manual_seed(seed * 1000 + ci)
        m = RVQVAE(vq_args(), dim, 512, 512, 512, 2, 2, 512, 3, 3, "relu", None)
        m.load_state_dict(synth.synth_vq_state_dict(dim))
        m.train()
        rec.start = start
        n_active = 6 if start is None else start + 1
        for s in range(steps):
            pre = f"c{ci}.s{s}."
            rec.reset()
            pose = synth.synth_vq_pose(part, dim, n=n, t=t, seed=3 + s)
            m.zero_grad()
            lat = {}
            h = m.encoder.register_forward_hook(lambda mod, i, o: lat.__setitem__("x", o.detach().clone()))
            res = m(pose)
            h.remove()
            rl = torch.nn.functional.mse_loss(res["rec_pose"], pose)
            loss = rl + 0.02 * res["commit_loss"]
            loss.backward()
            assert len(rec.gumbel) == n_active and len(rec.keep) == 12 and len(rec.tile_log) == n_active
            out[pre + "gumbel"] = torch.stack(rec.gumbel).numpy()
            for b, k in enumerate(rec.keep):
                out[pre + f"keep{b}"] = np.packbits(k.numpy().reshape(-1))
                out[pre + f"keep{b}.shape"] = np.array(k.shape)
            out[pre + "tile_calls"] = np.array([c + [-1] * (2 - len(c)) for c in rec.tile_log])          # per active layer: up to two draws
            out[pre + "latent"] = lat["x"].permute(0, 2, 1).contiguous().numpy()
            out[pre + "rec_pose"] = res["rec_pose"].detach().numpy()
            out[pre + "scalars"] = np.array([float(v.detach()) for v in (loss, rl, res["commit_loss"], res["perplexity"])], np.float32)
            out[pre + "idx"] = IDX.pop().numpy()
            out[pre + "xq"] = XQ.pop().permute(0, 2, 1).contiguous().numpy()
            for q in range(n_active):
                layer = m.quantizer.layers[q]
                for name, tns in (("codebook", layer.codebook), ("code_sum", layer.code_sum)):
                    nrm, smp = ref.sample(tns)
                    out[pre + f"{name}{q}.norm"], out[pre + f"{name}{q}.sample"] = np.float32(nrm), smp.numpy()
                out[pre + f"code_count{q}"] = layer.code_count.detach().numpy()
            if s == 0:
                names = [k for k, _ in m.named_parameters()]
                samples = [ref.sample(p.grad) for _, p in m.named_parameters()]
                gout["names"] = np.array(names)
                gout["norms"] = np.array([a for a, _ in samples], np.float32)
                gout["offsets"] = np.cumsum([0] + [len(b) for _, b in samples])
                gout["samples"] = torch.cat([b for _, b in samples]).numpy()
        print(f"case {ci}: loss/recons/commit/perplexity of the last step", out[pre + "scalars"])
    return files


IDX, XQ = [], []


def hook_quantizer_outputs():
    """ResidualVQ.forward's indices and quantised sum of the latest call (model.py:72 drops the indices)."""
    import models.vq.residual_vq as RV
    orig = RV.ResidualVQ.forward

    def fwd(self, x, *a, **k):
        ret = orig(self, x, *a, **k)
        IDX.append(ret[1].reshape(-1, ret[1].shape[-1]).clone())
        XQ.append(ret[0].detach().clone())
        return ret
    RV.ResidualVQ.forward = fwd


def paths():
    return {"main": "rvq_train_step.npz", "case1": "rvq_train_step_case1.npz", "grads0": "rvq_train_step_grads0.npz", "grads1": "rvq_train_step_grads1.npz"}


def main_step(check):
    torch.Tensor.cuda = lambda self, *a, **k: self
    import models.vq.quantizer as Q
    import models.vq.residual_vq as RV
    hook_quantizer_outputs()
    rec, seed = Recorder(0, Q, RV), 0
    while True:
        try:
            files = run_cases(rec, seed)
            break
        except GapTooSmall:
            print(f"seed {seed}: a top-2 logit gap below {GAP} of the logit magnitude - next seed")
            seed += 1
    for key, name in paths().items():
        path = os.path.join(HERE, name)
        if check:
            old = np.load(path)
            assert sorted(old.files) == sorted(files[key]), name
            for k in old.files:
                assert np.array_equal(old[k], np.asarray(files[key][k])), (name, k)
            print("identical:", name)
        else:
            np.savez_compressed(path, **files[key])
            print("wrote", name, os.path.getsize(path) // 1024, "KiB")


def main_loop():
    """rvq_beatx_train.py:367-381 at lr 2e-4 (no warm-up: --warm-up-iter 0), AdamW betas (0.9, 0.99), l2, commit 0.02, on synth.synth_vq_motion
    batches; the seed sets torch's and Python's global generators, i.e. dropout, Gumbel noise, `_tile` noise and the quantise-dropout coin."""
    torch.Tensor.cuda = lambda self, *a, **k: self
    from models.vq.model import RVQVAE
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    first, last = [], []
    for seed in LOOP_SEEDS:
        torch.manual_seed(seed)
        random.seed(seed)
        net = RVQVAE(vq_args(), LOOP_DIM, 512, 512, 512, 2, 2, 512, 3, 3, "relu", None)
        net.load_state_dict(synth.synth_vq_state_dict(LOOP_DIM))
        net.train()
        opt = torch.optim.AdamW(net.parameters(), lr=2e-4, betas=(0.9, 0.99), weight_decay=0.0)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[50000, 400000], gamma=0.05)
        for it in range(LOOP_STEPS):
            gt = synth.synth_vq_motion(LOOP_N, LOOP_T, LOOP_DIM, step=it)
            pred, commit, _ = net(gt).values()
            rl = torch.nn.functional.mse_loss(pred, gt)
            loss = rl + 0.02 * commit
            opt.zero_grad()
            loss.backward()
            opt.step()
            sched.step()
            if it == 0:
                first.append(float(rl))
            if it % 10 == 9:
                print(f"seed {seed} step {it + 1}: recons {float(rl):.5f}", flush=True)
        last.append(float(rl))
    np.savez(os.path.join(HERE, "rvq_train_loop.npz"), seeds=np.array(LOOP_SEEDS), shape=np.array([LOOP_N, LOOP_T, LOOP_DIM, LOOP_STEPS]),
             recons_first=np.array(first, np.float32), recons_last=np.array(last, np.float32))
    print("ratios", [b / a for a, b in zip(first, last)])


if __name__ == "__main__":
    main_loop() if "--loop" in sys.argv else main_step("--check" in sys.argv)
