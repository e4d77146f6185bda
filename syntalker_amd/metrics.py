"""Fréchet distance between Gaussian fits of two embedding sets.

The reference's FGD (dataloaders/data_tools.py:1615-1685, `FIDCalculator.frechet_distance` / `calculate_frechet_distance`)
is the pytorch-fid formula  d^2 = |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2))  over embeddings of its `VAESKConv` motion
encoder (weights/AESKConv_240_100.bin - not distributed with the repository).  This module is the formula, host side
(numpy / scipy like the reference's), and `fgd`, which runs it over that encoder's embeddings (evaluator.VAESKConv on the HIP
kernels) the way the reference's `test()` collects them.  `latent_embedding` - time-averaged sampler latents in a fixed seeded
projection - is the stand-in where no evaluator is at hand.

Further down: the h3d text-motion metrics, and the beatx evaluation's other two numbers - `L1div` and `alignment` (beat consistency) of
utils/metric.py on the kernels of csrc/syn_joints.inc, over the skeleton joints of `syntalker_amd.joints`.
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


# ---- the beatx evaluation's other two numbers: L1 diversity and beat consistency (utils/metric.py:12-27, 54-241) -----------------------
# The reference's classes with their signatures and return types, numpy in and out as `test()` uses them (diffusion_rvqvae_trainer.py:677-684),
# on the kernels of csrc/syn_joints.inc; device tensors are taken as they are.  `SRGR` has no caller in the reference and is not here.

UPPER_BODY = (3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)


def _device_f32(x, what):
    """numpy array or tensor -> contiguous fp32 tensor on the GPU (a CPU TENSOR is refused like everywhere else; arrays are the reference's
    host interface and are copied to the current device)."""
    import torch
    from . import engine
    if torch.is_tensor(x):
        engine._require_cuda(x, what)
        return x.detach().float().contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).cuda()


def l1_sum(x, blocks: int = 0):
    """sum |x - mean over rows| of an (n, C) array -> float, or of each of T equally long takes (T, n, C) -> (T,) float64 numpy, in one call
    (`syn_l1div`): fp64 sums in a fixed order, the input left as it is.  `blocks`: the grid of the two passes (0: the library's choice) - the
    result does not depend on it."""
    import torch
    from . import _lib
    x = _device_f32(x, "L1div input")
    if x.dim() not in (2, 3) or x.numel() == 0:
        raise ValueError(f"l1_sum: a non-empty (n, C) or (T, n, C) array, got {tuple(x.shape)}")
    t, (n, c) = (x.shape[0] if x.dim() == 3 else 1), x.shape[-2:]
    lib = _lib.load()
    ws = torch.empty(lib.syn_l1div_workspace_bytes(t, n, c) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(t, dtype=torch.float64, device=x.device)
    _lib.check(lib.syn_l1div(x.data_ptr(), t, n, c, ws.data_ptr(), int(blocks), out.data_ptr(), _lib.current_stream(x.device)), "syn_l1div")
    return out.cpu().numpy() if x.dim() == 3 else float(out.item())


class L1div(object):
    """utils/metric.py:12-27.  `run` does NOT overwrite its argument (the reference's does: it leaves the deviations in `results`)."""

    def __init__(self):
        self.counter = 0
        self.sum = 0

    def run(self, results):
        self.counter += results.shape[0]
        self.sum += l1_sum(results)

    def avg(self):
        return self.sum / self.counter

    def reset(self):
        self.counter = 0
        self.sum = 0


def motion_beat_mask(vel, t_start: int, t_end: int, order: int, threshold: float = 0.3):
    """vel (n, J) or (T, n, J) device speeds -> uint8 mask (n_slice, J) / (T, n_slice, J) of `syn_motion_beats` over the slice vel[t_start:t_end]
    (Python slice semantics).  Entry (j, i) says slice index j is a beat of joint i - with the reference's threshold test on vel[j, i], not
    vel[j + t_start, i] (utils/metric.py:113-123)."""
    import torch
    from . import _lib, engine
    engine._require_cuda(vel, "speeds")
    v = vel.detach().float().contiguous()
    batched = v.dim() == 3
    if v.dim() not in (2, 3):
        raise ValueError(f"motion_beat_mask: speeds are (n, J) or (T, n, J), got {tuple(vel.shape)}")
    v3 = v if batched else v[None]
    t, n, j = v3.shape
    s, e, _ = slice(t_start, t_end).indices(n)
    e = max(e, s)
    mask = torch.zeros(t, e - s, j, dtype=torch.uint8, device=v.device)
    if mask.numel():
        _lib.check(_lib.load().syn_motion_beats(v3.data_ptr(), t, n, j, s, e, int(order), float(threshold), mask.data_ptr(), _lib.current_stream(v.device)),
                   "syn_motion_beats")
    return mask if batched else mask[0]


def beat_align(mask, onset_times, upper_body=UPPER_BODY, pose_fps: float = 30.0, sigma: float = 0.3):
    """mask (n_slice, J) / (T, n_slice, J) uint8 on the device; onset_times: seconds, one array (or one per take) -> (per_joint (U,) / (T, U), bc
    float / (T,)) as numpy (`syn_beat_align`).  No onsets in a take: ValueError (the reference divides by zero there)."""
    import torch
    from . import _lib, engine
    engine._require_cuda(mask, "beat mask")
    batched = mask.dim() == 3
    m = (mask if batched else mask[None]).to(torch.uint8).contiguous()
    t, n_slice, j = m.shape
    per_take = [np.asarray(o, dtype=np.float64).reshape(-1) for o in (onset_times if batched else [onset_times])]
    if len(per_take) != t:
        raise ValueError(f"beat_align: {t} takes, {len(per_take)} onset lists")
    if any(o.size == 0 for o in per_take):
        raise ValueError("beat_align: a take without audio onsets has no beat consistency (the mean over its onsets is 0 / 0)")
    ub = np.asarray(list(upper_body), dtype=np.int32)
    if ub.size == 0 or ub.min() < 0 or ub.max() >= j:
        raise ValueError(f"beat_align: upper_body must name joints of [0, {j})")
    dev = m.device
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([o.size for o in per_take])]).astype(np.int32)).to(dev)
    ons = torch.from_numpy(np.concatenate(per_take)).to(dev)
    ubt = torch.from_numpy(ub).to(dev)
    per_joint = torch.empty(t, ub.size, dtype=torch.float32, device=dev)
    bc = torch.empty(t, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().syn_beat_align(m.data_ptr(), t, n_slice, j, ubt.data_ptr(), int(ub.size), ons.data_ptr(), offs.data_ptr(), float(pose_fps),
                                          float(sigma), per_joint.data_ptr(), bc.data_ptr(), _lib.current_stream(dev)), "syn_beat_align")
    pj, b = per_joint.cpu().numpy(), bc.cpu().numpy()
    return (pj, b) if batched else (pj[0], float(b[0]))


class alignment(object):
    """utils/metric.py:54-241 with the reference's signatures.  `load_pose` and `calculate_align` run on the device; `load_audio` is librosa's
    onset detector and nothing else, so it stays librosa's (imported when called); `load_audio_hip` is the same call on this package's detector."""

    def __init__(self, sigma, order, mmae=None, upper_body=[3, 6, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21]):
        self.sigma = sigma
        self.order = order
        self.upper_body = upper_body
        self.pose_data = []
        self.mmae = mmae
        self.threshold = 0.3

    def load_audio(self, wave, t_start=None, t_end=None, without_file=False, sr_audio=16000):
        try:
            import librosa
        except ImportError as e:
            raise ImportError("alignment.load_audio needs librosa (librosa.onset.onset_detect finds the audio onsets); it is not installed. "
                              "Compute the onset times elsewhere and pass them to calculate_align / beat_consistency.") from e
        y = wave if without_file else librosa.load(wave)[0]
        short_y = y if t_start is None else y[t_start:t_end]
        return librosa.onset.onset_detect(y=short_y, sr=sr_audio, hop_length=512, units="time")

    def load_audio_hip(self, wave, t_start=None, t_end=None, without_file=False, sr_audio=16000):
        """`load_audio` on this package's onset detector (syntalker_amd.audio, csrc/syn_audio.inc) instead of librosa's: the onset times in seconds of
        wave[t_start:t_end] as a float64 numpy array.  `wave`: the waveform at `sr_audio` (without_file=True, as test() calls it), or a `.wav` / `.npy`
        file AT that rate - the reference's `librosa.load` resamples a file to 22.05 kHz and detects at `sr_audio` all the same; this does not."""
        from . import audio
        y = wave if without_file else audio.read_wave(wave, sr_audio)
        short_y = y if t_start is None else y[t_start:t_end]
        return np.asarray(audio.onset_detect(short_y, sr=sr_audio, hop_length=512, units="time"), dtype=np.float64)

    def load_pose(self, pose, t_start, t_end, pose_fps, without_file=False):
        """pose (n, J * 3) joints -> one array of beat indices (slice indices) per joint."""
        if not without_file:
            raise NotImplementedError("alignment.load_pose reads joints from memory (without_file=True, as test() calls it); the BVH text reader is not ported")
        from . import joints as jt
        mask = motion_beat_mask(jt.joint_speed(_device_f32(pose, "pose"), pose_fps, self.mmae), t_start, t_end, self.order, self.threshold).cpu().numpy()
        return [np.array(np.nonzero(mask[:, i])[0].tolist()) for i in range(mask.shape[1])]       # (an empty list gives the reference's float64 empty array)

    @staticmethod
    def motion_frames2time(vel, offset, pose_fps):
        return vel / pose_fps + offset

    @staticmethod
    def GAHR(a, b, sigma):
        """Mean over b of exp(-min_a |a - b|^2 / 2 sigma^2) (0 for an empty a): one (take, joint) of `syn_beat_align`, on the host in fp64 for
        callers that hold times rather than a beat mask."""
        a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
        if b.size == 0:
            raise ValueError("GAHR: no audio onsets (the mean over them is 0 / 0)")
        if a.size == 0:
            return 0.0
        d = np.abs(a[None, :] - b[:, None]).min(1)
        return float(np.exp(-(d ** 2) / (2 * sigma ** 2)).sum() / b.size)

    def calculate_align(self, onset_bt_rms, beat_vel, pose_fps=30):
        """onset times (seconds) and `load_pose`'s list -> the mean over the upper-body joints of GAHR(beat times, onsets)."""
        import torch
        onsets = np.asarray(onset_bt_rms, dtype=np.float64).reshape(-1)
        if onsets.size == 0:
            raise ValueError("calculate_align: no audio onsets (the reference divides by zero here)")
        n_slice = 1 + max([int(np.max(b)) for b in beat_vel if len(b)], default=0)
        mask = np.zeros((n_slice, len(beat_vel)), dtype=np.uint8)
        for i, b in enumerate(beat_vel):
            if len(b):
                mask[np.asarray(b, dtype=np.int64), i] = 1
        return beat_align(torch.from_numpy(mask).cuda(), onsets, self.upper_body, pose_fps, self.sigma)[1]


def beat_consistency(joints, onset_times, mmae, align_mask: int = 60, sigma: float = 0.3, order: int = 7, upper_body=UPPER_BODY, pose_fps: float = 30.0,
                     threshold: float = 0.3):
    """BC of one take, or of T equally long takes, in one pass on the device: joints (n, J * 3) | (n, J, 3) | (T, n, J, 3) -> speeds / mmae ->
    beats of the slice [align_mask, n - align_mask) -> alignment with the onsets (seconds; one array, or one per take).  What `test()` computes
    per take at diffusion_rvqvae_trainer.py:683-684 (there: sigma 0.3, order 7, mask 60).  Returns a float, or (T,) numpy."""
    from . import joints as jt
    x = _device_f32(joints, "joints")
    vel = jt.joint_speed(x, pose_fps, mmae)
    n = vel.shape[-2]
    mask = motion_beat_mask(vel, align_mask, n - align_mask, order, threshold)
    return beat_align(mask, onset_times, upper_body, pose_fps, sigma)[1]


def audio_slice_of_test(wave, n_frames: int, align_mask: int = 60, audio_sr=16000, pose_fps: float = 30.0):
    """The stretch of a take's waveform `test()` detects onsets on (diffusion_rvqvae_trainer.py:681-683), as written there: the wave is cropped to
    int(audio_sr / pose_fps * n) samples, and of THAT the slice [a_offset : len(wave) - a_offset] is taken, a_offset = int(align_mask * (audio_sr /
    pose_fps)) - the end of the slice is counted from the end of the UNCROPPED wave, so it cuts into the crop only where the file is less than
    a_offset samples longer than the motion."""
    a_offset = int(align_mask * (audio_sr / pose_fps))
    return wave[:int(audio_sr / pose_fps * n_frames)][a_offset:len(wave) - a_offset]


def beat_consistency_from_audio(joints, wave, mmae, align_mask: int = 60, sigma: float = 0.3, order: int = 7, upper_body=UPPER_BODY, threshold: float = 0.3,
                                audio_sr=16000, pose_fps: float = 30.0):
    """`beat_consistency` of one take from its waveform at `audio_sr` (1-D: numpy, CPU or device tensor) instead of onset times: the onsets are those of
    `audio_slice_of_test(wave, n)` by syntalker_amd.audio.onset_detect (hop 512, units 'time') - lines 681-684 of the reference's test() on a machine
    without librosa.  A slice without onsets is a ValueError, as in `beat_align`."""
    from . import audio
    shape = tuple(joints.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"beat_consistency_from_audio: one take of joints, (n, J * 3) or (n, J, 3), got {shape}")
    if len(tuple(wave.shape)) != 1:
        raise ValueError(f"beat_consistency_from_audio: the waveform is 1-D, got {tuple(wave.shape)}")
    short = audio_slice_of_test(wave, shape[0], align_mask, audio_sr, pose_fps)
    if len(short) == 0:
        raise ValueError("beat_consistency_from_audio: the take's audio slice is empty (no onsets)")
    onsets = audio.onset_detect(short, sr=audio_sr, hop_length=512, units="time")
    return beat_consistency(joints, onsets, mmae, align_mask=align_mask, sigma=sigma, order=order, upper_body=upper_body, pose_fps=pose_fps, threshold=threshold)


# ---- the face numbers of test(): `l2 loss` and `lvel loss` over the face meshes (diffusion_rvqvae_trainer.py:640-675) -----------------------------
def vertex_losses(rec_vertices, tar_vertices, blocks: int = 0):
    """(l2, lvel) of two equally shaped vertex arrays (n, V, 3) | (n, C) as Python floats (`syn_vertex_losses`): l2 = mean (rec - tar)^2
    (nn.MSELoss, :673); lvel = mean |(rec[1:] - tar[:-1]) - (tar[1:] - tar[:-1])| (nn.L1Loss on the two differences AS WRITTEN at :672 - the
    reference differences `rec` against the previous TARGET frame), fp32 differences, fp64 sums in a fixed order.  n = 1: lvel is NaN.  `blocks`: the
    grid (0: the library's choice) - the result does not depend on it."""
    import torch
    from . import _lib
    r, t = _device_f32(rec_vertices, "rec vertices"), _device_f32(tar_vertices, "tar vertices")
    if r.shape != t.shape or r.dim() < 2 or r.numel() == 0:
        raise ValueError(f"vertex_losses: two non-empty arrays of one shape (n, ...), got {tuple(r.shape)} and {tuple(t.shape)}")
    n, c = r.shape[0], r.numel() // r.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.syn_vertex_losses_workspace_bytes(n, c) // 8, dtype=torch.float64, device=r.device)
    out = torch.empty(2, dtype=torch.float64, device=r.device)
    _lib.check(lib.syn_vertex_losses(r.data_ptr(), t.data_ptr(), n, c, ws.data_ptr(), int(blocks), out.data_ptr(), _lib.current_stream(r.device)),
               "syn_vertex_losses")
    l2, lvel = out.cpu().tolist()
    return l2, lvel


JAW = slice(66, 69)          # the jaw's axis-angle vector in test()'s (n, 165) pose


def face_losses(model, rec_pose, tar_pose, rec_exps, tar_exps):
    """diffusion_rvqvae_trainer.py:640-675 in one call: both face meshes with zero global, body, eye and hand pose and zero transl (the hands' mean
    pose is still added: `smplx` adds `pose_mean` to a zero hand pose too), each with its OWN jaw pose (:644, :658) and expression, then
    `vertex_losses`.  model: `mesh.smplx_mesh` of the take's betas; poses (n, 165) axis-angle or (n, 330) 6D; expressions (n, E).  Returns (l2, lvel),
    to be weighted by n as test() does (:674-675)."""
    import torch
    from . import engine, mesh, poses

    def face(pose, exps):
        engine._require_cuda(pose, "pose")
        p = pose.detach().float().reshape(-1, pose.shape[-1])
        if p.shape[1] == 330:
            p = poses.rotation_6d_to_axis_angle(p.reshape(-1, 55, 6)).reshape(-1, 165)
        if p.shape[1] != 165:
            raise ValueError(f"face_losses: poses are (n, 165) axis-angle or (n, 330) 6D, got {tuple(pose.shape)}")
        jaw_only = torch.zeros_like(p)
        jaw_only[:, JAW] = p[:, JAW]
        return mesh.smplx_vertices(model, jaw_only, exps)
    return vertex_losses(face(rec_pose, rec_exps), face(tar_pose, tar_exps))
