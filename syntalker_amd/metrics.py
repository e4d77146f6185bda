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


# ---- the h3d text-motion metrics (utils/t2m_eval_tools.py:8-246) over EvaluatorMDMWrapper's co-embeddings (t2m_evaluator.py) -----------
# Host numpy like the reference, same signatures, same dtypes (float32 embeddings are not widened: the reference's numbers are those of
# float32 sums), same draws from numpy's global RNG.

def euclidean_distance_matrix(matrix1, matrix2):
    """(N1, D), (N2, D) -> (N1, N2) distances by |a|^2 - 2 a.b + |b|^2 (:8-22)."""
    assert matrix1.shape[1] == matrix2.shape[1]
    cross = -2 * np.dot(matrix1, matrix2.T)
    sq1 = np.sum(np.square(matrix1), axis=1, keepdims=True)
    sq2 = np.sum(np.square(matrix2), axis=1)
    return np.sqrt(cross + sq1 + sq2)


def calculate_top_k(mat, top_k):
    """mat (N, N) of ranked indices per row -> (N, top_k) bool: column k says whether row i's own index is among its first k + 1 (:24-36)."""
    own = np.arange(mat.shape[0])[:, None]
    return np.logical_or.accumulate(mat[:, :top_k] == own, axis=1)


def calculate_activation_statistics(activations):
    """(N, D) -> mean (D), covariance (D, D) (:40-50)."""
    return np.mean(activations, axis=0), np.cov(activations, rowvar=False)


def calculate_diversity(activation, diversity_times):
    """Mean distance between two draws of `diversity_times` rows, each without replacement from numpy's global RNG (:53-61)."""
    assert len(activation.shape) == 2
    assert activation.shape[0] > diversity_times
    n = activation.shape[0]
    first = np.random.choice(n, diversity_times, replace=False)
    second = np.random.choice(n, diversity_times, replace=False)
    return np.linalg.norm(activation[first] - activation[second], axis=1).mean()


def calculate_multimodality(activation, multimodality_times):
    """activation (prompts, repeats, D): mean distance between two draws of `multimodality_times` repeats, shared by the prompts (:64-72)."""
    assert len(activation.shape) == 3
    assert activation.shape[1] > multimodality_times
    n = activation.shape[1]
    first = np.random.choice(n, multimodality_times, replace=False)
    second = np.random.choice(n, multimodality_times, replace=False)
    return np.linalg.norm(activation[:, first] - activation[:, second], axis=2).mean()


def t2m_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """`calculate_frechet_distance` (:76-127): the formula of frechet_from_stats on the statistics as given, and a ValueError where sqrt(C1 C2)
    keeps an imaginary diagonal above 1e-3 (the FGD's wrapper turns that into 1e10; this one does not)."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, "mean vectors of different lengths"
    assert sigma1.shape == sigma2.shape, "covariances of different dimensions"
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        off = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + off).dot(sigma2 + off))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    d = mu1 - mu2
    return d.dot(d) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def get_metric_statistics(values, replication_times):
    """Mean and 95 % confidence half-width over replications (:242-246)."""
    return np.mean(values, axis=0), 1.96 * np.std(values, axis=0) / np.sqrt(replication_times)


def _say(file, line):
    print(line)
    print(line, file=file, flush=True)


def _align(m_lens):
    return np.argsort(m_lens.data.tolist())[::-1].copy()


def _per_batch_embeddings(eval_wrapper, batches, texts: bool):
    """[(text_embedding | None, motion_embedding)] as numpy, one pair per batch, each in its own batch's `align_idx` order - what a
    get_co_embeddings / get_motion_embeddings call per batch returns.  With this package's wrapper, whose embedding of a sequence does not
    depend on its batch (bitwise), batches of one shape are embedded in ONE call and handed back per batch: a call of 32 sequences leaves
    most of the chip idle."""
    import torch
    from .t2m_evaluator import EvaluatorMDMWrapper
    if not batches:
        return []
    same = all(b[4].shape[1:] == batches[0][4].shape[1:] and (not texts or b[0].shape[1:] == batches[0][0].shape[1:]) for b in batches)
    if not (isinstance(eval_wrapper, EvaluatorMDMWrapper) and same and len(batches) > 1):
        out = []
        for word, pos, _, sent_lens, motions, m_lens, _ in batches:
            if texts:
                t, m = eval_wrapper.get_co_embeddings(word_embs=word, pos_ohot=pos, cap_lens=sent_lens, motions=motions, m_lens=m_lens)
                out.append((t.cpu().numpy(), m.cpu().numpy()))
            else:
                out.append((None, eval_wrapper.get_motion_embeddings(motions=motions, m_lens=m_lens).cpu().numpy()))
        return out
    cat = lambda i: torch.cat([torch.as_tensor(b[i]) for b in batches])
    m_lens = cat(5)
    order = _align(m_lens)                                     # the one call's output order; undone below
    if texts:
        t, m = eval_wrapper.get_co_embeddings(word_embs=cat(0), pos_ohot=cat(1), cap_lens=cat(3), motions=cat(4), m_lens=m_lens)
        t = t.cpu().numpy()
    else:
        t, m = None, eval_wrapper.get_motion_embeddings(motions=cat(4), m_lens=m_lens)
    m = m.cpu().numpy()
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    out, i = [], 0
    for b in batches:
        rows = inv[i + _align(torch.as_tensor(b[5]))]
        out.append((None if t is None else t[rows], m[rows]))
        i += len(b[5])
    return out


def evaluate_matching_score(eval_wrapper, motion_loaders, file):
    """:129-179.  Per loader: the mean text-to-own-motion distance and R-precision (top 1 / 2 / 3) within each batch, and every motion
    embedding for the FID and Diversity.  Returns (match_score_dict, R_precision_dict, activation_dict)."""
    from collections import OrderedDict
    match_score_dict, r_precision_dict, activation_dict = OrderedDict(), OrderedDict(), OrderedDict()
    print("========== Evaluating Matching Score ==========")
    for name, loader in motion_loaders.items():
        score_sum, top_k_count, all_size, all_motion = 0, 0, 0, []
        for text_emb, motion_emb in _per_batch_embeddings(eval_wrapper, list(loader), texts=True):
            dist = euclidean_distance_matrix(text_emb, motion_emb)
            score_sum += dist.trace()
            top_k_count += calculate_top_k(np.argsort(dist, axis=1), top_k=3).sum(axis=0)
            all_size += text_emb.shape[0]
            all_motion.append(motion_emb)
        matching_score, r_precision = score_sum / all_size, top_k_count / all_size
        match_score_dict[name], r_precision_dict[name] = matching_score, r_precision
        activation_dict[name] = np.concatenate(all_motion, axis=0)
        _say(file, f"---> [{name}] Matching Score: {matching_score:.4f}")
        _say(file, f"---> [{name}] R_precision: " + "".join("(top %d): %.4f " % (i + 1, r) for i, r in enumerate(r_precision)))
    return match_score_dict, r_precision_dict, activation_dict


def evaluate_fid(eval_wrapper, groundtruth_loader, activation_dict, file):
    """:183-206: the Frechet distance of each entry of activation_dict to the ground-truth loader's motion embeddings."""
    from collections import OrderedDict
    print("========== Evaluating FID ==========")
    gt = np.concatenate([m for _, m in _per_batch_embeddings(eval_wrapper, list(groundtruth_loader), texts=False)], axis=0)
    gt_mu, gt_cov = calculate_activation_statistics(gt)
    eval_dict = OrderedDict()
    for name, emb in activation_dict.items():
        mu, cov = calculate_activation_statistics(emb)
        eval_dict[name] = t2m_frechet_distance(gt_mu, gt_cov, mu, cov)
        _say(file, f"---> [{name}] FID: {eval_dict[name]:.4f}")
    return eval_dict


def evaluate_diversity(activation_dict, file, diversity_times):
    """:209-217."""
    from collections import OrderedDict
    print("========== Evaluating Diversity ==========")
    eval_dict = OrderedDict()
    for name, emb in activation_dict.items():
        eval_dict[name] = calculate_diversity(emb, diversity_times)
        _say(file, f"---> [{name}] Diversity: {eval_dict[name]:.4f}")
    return eval_dict


def evaluate_multimodality(eval_wrapper, mm_motion_loaders, file, mm_num_times):
    """:220-239: each batch is ((1, repeats, T, D) motions, (1, repeats) lengths) of one prompt; 0 for an empty loader."""
    from collections import OrderedDict
    import torch
    print("========== Evaluating MultiModality ==========")
    eval_dict = OrderedDict()
    for name, loader in mm_motion_loaders.items():
        embs = [eval_wrapper.get_motion_embeddings(motions[0], m_lens[0]).unsqueeze(0) for motions, m_lens in loader]
        multimodality = calculate_multimodality(torch.cat(embs, dim=0).cpu().numpy(), mm_num_times) if embs else 0
        _say(file, f"---> [{name}] Multimodality: {multimodality:.4f}")
        eval_dict[name] = multimodality
    return eval_dict
