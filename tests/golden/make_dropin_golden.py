#!/usr/bin/env python3
"""Golden vectors of the drop-in claim (tests/test_dropin_reference_driver.py): the REFERENCE's own driver code -
`CustomTrainer._g_test` of diffusion_rvqvae_trainer.py, lifted from its file and compiled unchanged (make_longform_golden.lift_methods) -
driving THIS build's `MDM` and `create_gaussian_diffusion()` through the reference's import names (syntalker_amd/dropin), with the device
engine replaced by its CPU stand-ins (tests/cpu_engine.py).  Stored: what `_g_test` hands the three decoders (the stitched latents, divided
by the latent scale) and the shapes of what it returns.  Runs in the build container (needs the reference tree):
    python tests/golden/make_dropin_golden.py
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import make_longform_golden as gen  # noqa: E402  (puts the reference tree on sys.path)
from syntalker_amd import synth  # noqa: E402
from tests import cpu_engine  # noqa: E402

LATENT_SCALE = 5.0
SEED = 5                 # torch.manual_seed in front of the loop: x_T, then the loop's seed, in that order


def run():
    g_test, inverse_selection_tensor = gen.lift_methods("_g_test", "inverse_selection_tensor")
    # the reference's import statements, resolved to this build (train.py:85-94, diffusion_rvqvae_trainer.py:26-27)
    from syntalker_amd.dropin.diffusion.model_util import create_gaussian_diffusion
    from syntalker_amd.dropin.models.denoiser import MDM
    me = types.SimpleNamespace()
    me.args = types.SimpleNamespace(vqvae_squeeze_scale=4, pre_frames=4, pose_length=128, pose_dims=330, batch_size=1, pose_norm=True)
    me.joints = 55
    masks = synth.synth_joint_masks()
    me.joint_mask_upper, me.joint_mask_hands, me.joint_mask_lower = masks["upper"], masks["hands"], masks["lower"]
    me.inverse_selection_tensor = lambda *a: inverse_selection_tensor(me, *a)
    me.model = synth.synth_fill_(MDM(synth.default_args()).eval(), seed=0)
    me.diffusion = create_gaussian_diffusion(use_ddim=True)                   # `_g_test` calls its p_sample_loop: 50 ancestral steps per window
    me.vqvae_latent_scale, me.use_trans = LATENT_SCALE, True
    stats = synth.synth_pose_stats()
    me.trans_mean, me.trans_std = stats["trans"]
    (me.mean_upper, me.std_upper), (me.mean_hands, me.std_hands), (me.mean_lower, me.std_lower) = stats["upper"], stats["hands"], stats["lower"]
    seen = {}
    for part, dim in (("upper", 78), ("hands", 180), ("lower", 57)):          # the decoders are not the subject here: record what they are handed
        def l2o(x, part=part, dim=dim):
            seen[part] = x.clone()
            return torch.zeros(x.shape[0], 4 * x.shape[1], dim), 0.0, 0.0
        setattr(me, f"vq_model_{part}", types.SimpleNamespace(latent2origin=l2o))
    n = gen.N_POSE
    take = synth.synth_long_take(n, seed=21)
    data = {"tar_pose": take["pose"], "tar_beta": torch.zeros(1, n, 300), "tar_exps": torch.zeros(1, n, 100), "tar_contact": torch.zeros(1, n, 4),
            "tar_trans": torch.zeros(1, n, 3), "in_word": take["word"], "in_audio": take["audio"], "latent_in": take["latent"],
            "tar_id": torch.zeros(1, n, 1, dtype=torch.long)}
    torch.manual_seed(SEED)
    with torch.no_grad():
        res = g_test(me, data)                                                # the reference's lines, this build's model and loop
    theirs = torch.cat([seen[p] for p in ("upper", "hands", "lower")], dim=-1) / LATENT_SCALE
    return {"latents": theirs.numpy().astype(np.float32), "rec_pose_shape": np.array(res["rec_pose"].shape, dtype=np.int64),
            "rec_trans_shape": np.array(res["rec_trans"].shape, dtype=np.int64)}


def main():
    with pytest.MonkeyPatch.context() as mp:
        cpu_engine.install(mp)
        mp.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self, raising=False)
        out = run()
    dst = os.path.join(HERE, "dropin_driver_outputs.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: latents {out['latents'].shape}, rec_pose {tuple(out['rec_pose_shape'])}, rec_trans {tuple(out['rec_trans_shape'])}")


if __name__ == "__main__":
    main()
