#!/usr/bin/env python3
"""The reference's `test.py -c <yaml>` scenario on this build (diffusion_rvqvae_trainer.py:577-732):
YAML -> args namespace -> denoiser + diffusion + the three body-part RVQ-VAEs (+ translation statistics) ->
window-by-window sampling of whole takes -> RVQ-VAE decoding -> poses / root translation, all on the device -> optional
Fréchet statistic of the sampled latents against reference statistics.

    python scripts/sample_from_config.py configs.yaml [--seconds 8] [--takes 4] [--ddim] [--plms [--plms-order K]] [--seed 1]
                                         [--random-init] [--inputs in.npz] [--ref-stats ref.npz] [--out out.npz]
                                         [--upper-prompt TEXT] [--hands-prompt TEXT] [--lower-prompt TEXT]
                                         [--keep-from TAKE.npz [--keep-parts upper,hands,lower] [--keep-frames a:b]]
                                         [--guide-from TAKE.npz [--guide-parts upper,hands,lower] [--guide-frames a:b] [--guide-scale S]]

--plms          the pseudo linear multistep sampler (`plms_sample_loop`) over the 50-step respacing, at order K = 2 (default), 3 or 4.
--random-init   ignore the checkpoint / statistics paths of the YAML and use the name-keyed synthetic weights (there is no
                network for the reference's checkpoints here); without it every configured path must exist.
--inputs        npz with audio (B, n*533, 2), word (B, n), seed (B, n/4, 1536); default: synthetic inputs.
--ref-stats     npz with mu / sigma of `metrics.latent_embedding` (dim given by its shape) of reference samples.
--upper-prompt / --hands-prompt / --lower-prompt
                h3d configuration only (h3d_diffusion_new_trainer.py:489-511, test_h3d.py): each given prompt goes through the TMR text
                encoder (tmr.build_encoders: `tmr_base_path`, `tmr_text_model_path` or ./ckpt/distilbert-base-uncased) and the per-part
                style dict drives TwoClassifierFreeSampleModel_Bodypart; a part without a prompt gets the zero vector there.  Without
                any prompt the denoiser samples unguided with a zero style vector, as before.
--keep-from / --keep-parts / --keep-frames
                motion editing (in-painting, `longform.sample_long(edit=...)`; BEAT-X configuration): TAKE.npz holds the recorded take - pose
                (B, n, 165) axis-angle, optionally trans_v (B, n, 3) root velocity and mask_upper / mask_hands / mask_lower (0/1 over the 165
                channels).  A real take should carry its mask_* arrays - the reference's joint lists (dataloaders/data_tools.py, beat_smplx_upper /
                _hands / _lower); without them the stand-in masks of `synth.synth_joint_masks` are used, which have the reference's joint
                counts per part but are not guaranteed to be its joints.  It goes through `poses.encode_take` to the sampler's
                latents; the body parts named by --keep-parts (all frames) and the latent frames a:b (half-open, pose frame / 4; all channels)
                are kept from it and the rest is generated.
--guide-from / --guide-parts / --guide-frames / --guide-scale
                the soft counterpart (gradient guidance, `guided.keyframe_cond_fn` with cond_fn_with_grad=True; BEAT-X configuration): the same kind
                of take and the same selection, but the chosen parts / frames are PULLED towards the take with log p = -S sum keep (pred_xstart -
                take)^2 (default S = 0.05) instead of copied, and every entry stays generated.  One window (the take's first `pose_length` pose
                frames): guidance over windows is not built into `longform.sample_long`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syntalker_amd import config, longform, metrics, synth          # noqa: E402
from syntalker_amd.process import create_gaussian_diffusion         # noqa: E402

PATH_KEYS = ("test_ckpt", "vqvae_upper_path", "vqvae_hands_path", "vqvae_lower_path", "vqvae_lower_trans_path",
             "mean_trans_path", "std_trans_path", "tmr_base_path")
PROMPT_PARTS = ("upper", "hands", "lower")


def prompt_styles(args, prompts: dict, dev, random_init: bool) -> dict:
    """{'upper_mask': (1, 256) or None, ...}: `textencoder(prompt).loc` per prompted part (h3d_diffusion_new_trainer.py:505-510)."""
    from syntalker_amd import tmr
    _, text = tmr.build_encoders(args, dev, text=True)
    if random_init:
        text.load_state_dict(synth.synth_tmr_state_dict(text))
    with torch.no_grad():
        return {f"{part}_mask": (None if prompts[part] is None else text(prompts[part]).loc) for part in PROMPT_PARTS}


def edit_from_take(a, args, s, dev, n: int, batch: int, squeeze: int, flag: str = "keep"):
    """(known_latent, keep) of --keep-from / --keep-parts / --keep-frames for `sample_long(edit=...)` (flag "guide": of --guide-from / ...)."""
    from syntalker_amd import poses
    if config.is_h3d(args):
        raise SystemExit(f"--{flag}-from takes 165-channel SMPL-X poses: the BEAT-X configuration")
    path, parts_arg, frames_arg = (getattr(a, f"{flag}_{k}") for k in ("from", "parts", "frames"))
    z = np.load(path)
    pose = torch.from_numpy(z["pose"]).float().to(dev)
    if pose.shape[0] != batch or pose.shape[1] < n:
        raise SystemExit(f"--{flag}-from: pose is {tuple(pose.shape)}, the run has {batch} takes of {n} pose frames")
    pose = pose[:, :n - n % squeeze]
    trans_v = None
    if s.use_trans:
        trans_v = torch.from_numpy(z["trans_v"]).float().to(dev)[:, :pose.shape[1]] if "trans_v" in z else torch.zeros(*pose.shape[:2], 3, device=dev)
    masks = synth.synth_joint_masks()
    masks.update({k: z[f"mask_{k}"] for k in masks if f"mask_{k}" in z})
    stats = None if s.trans_mean is None else (s.trans_mean, s.trans_std)
    with torch.no_grad():
        known = poses.encode_take(pose, trans_v, s.vq["upper"], s.vq["hands"], s.vq["lower"], masks, None, stats, s.latent_scale)["latent_in"]
    parts = tuple(p for p in (parts_arg or "").split(",") if p)
    frames = None
    if frames_arg:
        lo, hi = frames_arg.split(":")
        frames = (int(lo or 0), int(hi) if hi else known.shape[1])
    return known, longform.keep_mask(known.shape[1], parts, frames)


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--seconds", type=float, default=8.0)
    ap.add_argument("--takes", type=int, default=1)
    ap.add_argument("--ddim", action="store_true")
    ap.add_argument("--plms", action="store_true")
    ap.add_argument("--plms-order", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--inputs")
    ap.add_argument("--ref-stats")
    ap.add_argument("--out")
    for part in PROMPT_PARTS:
        ap.add_argument(f"--{part}-prompt")
    ap.add_argument("--keep-from")
    ap.add_argument("--keep-parts")
    ap.add_argument("--keep-frames")
    ap.add_argument("--guide-from")
    ap.add_argument("--guide-parts")
    ap.add_argument("--guide-frames")
    ap.add_argument("--guide-scale", type=float, default=0.05)
    a = ap.parse_args(argv)
    if (a.guide_parts or a.guide_frames) and not a.guide_from:
        raise SystemExit("--guide-parts / --guide-frames need --guide-from: the take to pull them towards")
    if a.guide_from and not (a.guide_parts or a.guide_frames):
        raise SystemExit("--guide-from needs --guide-parts and / or --guide-frames: what to pull towards the take")
    if a.guide_from and (a.keep_from or a.plms):
        raise SystemExit("--guide-from goes with neither --keep-from nor --plms (the PLMS loop takes no cond_fn)")
    if (a.keep_parts or a.keep_frames) and not a.keep_from:
        raise SystemExit("--keep-parts / --keep-frames need --keep-from: the take to keep them from")
    if a.keep_from and not (a.keep_parts or a.keep_frames):
        raise SystemExit("--keep-from needs --keep-parts and / or --keep-frames: what to keep of the take")
    over = {k: None for k in PATH_KEYS} if a.random_init else {}
    args = config.load_args(a.config, **over)
    s = config.build_sampler(args)
    if a.random_init:
        synth.synth_fill_(s.model, 0)
        for m in s.vq.values():
            m.load_state_dict(synth.synth_vq_state_dict(m.input_width, seed=11))
    pose_length, pre, squeeze = int(getattr(args, "pose_length", 128)), int(getattr(args, "pre_frames", 4)), int(getattr(args, "vqvae_squeeze_scale", 4))
    dev = next(s.model.parameters()).device
    if a.inputs:
        z = np.load(a.inputs)
        audio, word, seed_lat = (torch.from_numpy(z[k]).to(dev) for k in ("audio", "word", "seed"))
    else:
        n, B = int(a.seconds * int(getattr(args, "pose_fps", 30))), a.takes
        g = torch.Generator().manual_seed(a.seed)
        audio = torch.randn(B, n * longform.AUDIO_PER_POSE, 2, generator=g).to(dev)
        word = torch.randint(0, synth.VOCAB, (B, n), generator=g).to(dev)
        seed_lat = torch.randn(B, n // squeeze, 1536, generator=g).to(dev)
    n = word.shape[1]
    _, rounds, _ = longform.window_plan(n, pose_length, pre, squeeze)
    if rounds < 1:
        raise SystemExit(f"{n} pose frames are less than one window of {pose_length}")
    if a.plms and a.ddim:
        raise SystemExit("--plms and --ddim are two samplers: give one")
    diffusion = create_gaussian_diffusion(use_ddim=a.ddim or a.plms)
    prompts = {part: getattr(a, f"{part}_prompt") for part in PROMPT_PARTS}
    model, y_extra, style_dim = s.model, None, 256 if config.is_h3d(args) else 512       # the h3d denoiser's style input is 256 wide
    if any(v is not None for v in prompts.values()):
        if not config.is_h3d(args):
            raise SystemExit("--upper-prompt / --hands-prompt / --lower-prompt need the h3d (text-prompt) configuration")
        from syntalker_amd.guidance import TwoClassifierFreeSampleModel_Bodypart
        model = TwoClassifierFreeSampleModel_Bodypart(s.model)
        y_extra = {"style_feature": prompt_styles(args, prompts, dev, a.random_init)}
    edit = edit_from_take(a, args, s, dev, n, word.shape[0], squeeze) if a.keep_from else None
    guide = edit_from_take(a, args, s, dev, n, word.shape[0], squeeze, "guide") if a.guide_from else None
    torch.cuda.synchronize(); t0 = time.perf_counter()
    if guide is not None:
        # one window under gradient guidance: the selection of the take as a soft objective on pred_xstart
        from syntalker_amd import guided
        round_l = longform.window_plan(n, pose_length, pre, squeeze)[0]
        target, keep = longform.window_edit(0, guide[0], guide[1].to(dev), round_l, pose_length // squeeze, squeeze)
        y = longform.window_inputs(0, audio, word, seed_lat, None, round_l, pre, squeeze, style_dim, y_extra)
        loop = diffusion.ddim_sample_loop if a.ddim else diffusion.p_sample_loop
        shape = (word.shape[0], 1536, 1, pose_length // squeeze)
        x_T = torch.randn(*shape, generator=torch.Generator().manual_seed(a.seed)).to(dev)      # (the whole run follows --seed)
        x = loop(model, shape, noise=x_T, clip_denoised=False, cond_fn=guided.keyframe_cond_fn(target, keep, a.guide_scale, True),
                 cond_fn_with_grad=True, model_kwargs={"y": y}, seed=a.seed)
        lat, rounds = x[:, :, 0, :].permute(0, 2, 1).contiguous(), 1
    else:
        lat = longform.sample_long(diffusion, model, audio, word, seed_lat, n, pose_length=pose_length, pre_frames=pre, squeeze=squeeze,
                                   use_ddim=a.ddim, seed=a.seed, style_dim=style_dim, y_extra=y_extra, edit=edit,
                                   **({"sampler": "plms", "plms_order": a.plms_order} if a.plms else {}))
    torch.cuda.synchronize(); t1 = time.perf_counter()
    out = longform.decode_take(lat, s.vq["upper"], s.vq["hands"], s.vq["lower"], s.latent_scale, use_trans=s.use_trans,
                               trans_mean=s.trans_mean, trans_std=s.trans_std)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    rep = {"config": a.config, "pose_frames": int(n), "windows": int(rounds), "takes": int(word.shape[0]),
           "sampler": f"plms50-order{a.plms_order}" if a.plms else "ddim50" if a.ddim else "ddpm1000", "sampling_s": round(t1 - t0, 4), "decoding_s": round(t2 - t1, 4),
           "latents": list(lat.shape), "poses": {k: (None if v is None else list(v.shape)) for k, v in out.items()},
           "prompts": {k: v for k, v in prompts.items() if v is not None},
           "finite": bool(all(v is None or bool(torch.isfinite(v).all()) for v in out.values()))}
    if edit is not None:
        kept = edit[1].to(lat.device)[:lat.shape[1]].expand(lat.shape)
        rep["edit"] = {"path": diffusion.last_path, "kept_fraction": round(float(kept.float().mean()), 4),
                       "kept_exact": bool(torch.equal(lat[kept], edit[0][:, :lat.shape[1]][kept]))}
    if guide is not None:
        w = keep[:, :, 0, :].permute(0, 2, 1).float()
        dist = lambda v: float((w * (v - target[:, :, 0, :].permute(0, 2, 1))).norm() / (w * target[:, :, 0, :].permute(0, 2, 1)).norm().clamp_min(1e-30))
        rep["guide"] = {"path": diffusion.last_path, "scale": a.guide_scale, "guided_fraction": round(float(w.mean()), 4), "rel_distance_to_take": round(dist(lat), 4)}
    if a.ref_stats:
        z = np.load(a.ref_stats)
        emb = metrics.latent_embedding(lat.float().cpu().numpy(), dim=int(z["mu"].shape[0]))
        rep["frechet_vs_ref"] = metrics.frechet_from_stats(*metrics.gaussian_stats(emb), z["mu"], z["sigma"])
    if a.out:
        np.savez(a.out, latents=lat.float().cpu().numpy(), **{k: v.float().cpu().numpy() for k, v in out.items() if v is not None})
    print(json.dumps(rep))
    rep["_latents"] = lat
    return rep


if __name__ == "__main__":
    main()
