"""Fréchet distance between Gaussian fits of two embedding sets.

The reference's FGD (dataloaders/data_tools.py:1615-1685, `FIDCalculator.frechet_distance` / `calculate_frechet_distance`)
is the pytorch-fid formula  d^2 = |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2))  over embeddings of its `VAESKConv` motion
encoder (weights/AESKConv_240_100.bin - not distributed with the repository).  This module is the formula, host side
(numpy / scipy like the reference's), and `fgd`, which runs it over that encoder's embeddings (evaluator.VAESKConv on the HIP
kernels) the way the reference's `test()` collects them.  `latent_embedding` - time-averaged sampler latents in a fixed seeded
projection - is the stand-in where no evaluator is at hand.
"""
from __future__ import annotations

import numpy as np


def gaussian_stats(emb) -> tuple[np.ndarray, np.ndarray]:
    e = np.asarray(emb, dtype=np.float64)
    return e.mean(0), np.cov(e, rowvar=False)


def frechet_from_stats(mu1, c1, mu2, c2, eps: float = 1e-6) -> float:
    from scipy import linalg
    mu1, mu2, c1, c2 = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (mu1, mu2, c1, c2))
    c1, c2 = np.atleast_2d(c1), np.atleast_2d(c2)
    covmean, _ = linalg.sqrtm(c1.dot(c2), disp=False)
    if not np.isfinite(covmean).all():                     # singular product: the reference's epsilon retry (:1668-1672)
        off = np.eye(c1.shape[0]) * eps
        covmean = linalg.sqrtm((c1 + off).dot(c2 + off))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):       # :1675-1678 raises ValueError, which `frechet_distance` (:1615-1626) turns into 1e10
            return 1e10
        covmean = covmean.real
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(covmean))


def frechet_distance(emb_a, emb_b) -> float:
    return frechet_from_stats(*gaussian_stats(emb_a), *gaussian_stats(emb_b))


def latent_embedding(latents, dim: int = 240, seed: int = 2021) -> np.ndarray:
    """(N, T, 1536) sampler latents -> (N, dim): mean over time, fixed Gaussian projection (stand-in for the motion encoder)."""
    x = np.asarray(latents, dtype=np.float64)
    x = x.reshape(x.shape[0], -1, x.shape[-1]).mean(1)
    proj = np.random.RandomState(seed).randn(x.shape[-1], dim) / np.sqrt(x.shape[-1])
    return x @ proj


def fgd(evaluator, rec_takes, tar_takes, vae_test_len: int = 32) -> float:
    """The reference's FGD (diffusion_rvqvae_trainer.py:613-619, 716-718): every take trimmed to a multiple of `vae_test_len`, embedded
    by `evaluator.map2latent` (a VAESKConv), its rows of `vae_length` collected over the takes, separately for the generated (`rec_takes`)
    and ground-truth (`tar_takes`) poses, then `frechet_distance` of the two sets.

    Takes are 6D poses of shape (n_i, 330) or (1, n_i, 330) - `_g_test`'s `rec_pose` / `tar_pose` - as tensors or arrays.  `test()` first
    sends them through rotation matrices and back (:613-616); on `_g_test`'s output, which already went that way (:528-529), that is the
    identity up to fp32 rounding, so it is not repeated here.  Takes of equal trimmed length share one batch (clips are independent in
    the encoder); a take shorter than `vae_test_len` contributes no rows."""
    import torch
    dev = next(evaluator.parameters()).device
    width = int(evaluator.vae_length)

    def rows(takes):
        trimmed = []
        for t in takes:
            t = torch.as_tensor(t).float()
            if t.dim() == 3 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 2:
                raise ValueError(f"fgd: a take must be (n, C) or (1, n, C), got {tuple(t.shape)}")
            trimmed.append(t[: t.shape[0] - t.shape[0] % vae_test_len])
        out = [None] * len(trimmed)
        for n in sorted({t.shape[0] for t in trimmed}):
            idx = [i for i, t in enumerate(trimmed) if t.shape[0] == n]
            if n == 0:
                for i in idx:
                    out[i] = np.zeros((0, width))
                continue
            emb = evaluator.map2latent(torch.stack([trimmed[i] for i in idx]).to(dev)).reshape(len(idx), -1, width).cpu().numpy()
            for k, i in enumerate(idx):
                out[i] = emb[k]
        return np.concatenate(out, 0) if out else np.zeros((0, width))

    return frechet_distance(rows(rec_takes), rows(tar_takes))
