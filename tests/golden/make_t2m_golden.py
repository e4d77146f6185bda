#!/usr/bin/env python3
"""Golden outputs of the reference's T2M evaluator (utils/t2m_eval_tools.py: EvaluatorMDMWrapper over MovementConvEncoder,
MotionEncoderBiGRUCo, TextEncoderBiGRUCo, and its metric functions), run on CPU in fp32 with the seeded weights of
synth.synth_t2m_state_dict.  Runs in the build container only; the module is loaded from its file (it needs torch, numpy and scipy only).

Stored in tests/golden/t2m_evaluator_outputs.npz (inputs are regenerated from their seeds by synth.synth_t2m_batch, not stored):
  keys_* / shapes_*            the three state dicts' layout
  batch_seeds                  seeds of the four batches of 32 (scanned upwards from 100; see the gap check below)
  text_k, motion_k             get_co_embeddings of batch k (align_idx order), k = 0 .. 3; batch 0 is the golden case of the GPU test
  edge_text, edge_motion       get_co_embeddings of 3 sequences: motions of (196, 23, 4) frames, captions of (22, 5, 1) tokens
  tie_lens, tie_align          a batch's m_lens with ties and the reference's align_idx for it
  dist_k, topk_k, ...          every metric function on batches 0 .. 2 (diversity / multimodality after np.random.seed(k))
  ms_*, rp_*, fid_*, div_*     evaluate_matching_score / evaluate_fid / evaluate_diversity over the loaders a = batches (0, 1, 2) and
                               b = batches (2, 3), ground truth = loader b
The generator ASSERTS what the GPU tests rely on: in batches 0 .. 2 every row's sorted distances at ranks 1 - 4 are >= 2e-3 apart (an
embedding error of 2e-5 per element moves a distance by at most 2 * 2e-5 * sqrt(512) = 9e-4, so the reference's own ranks stay decided),
and the mean |embedding| lies in [0.05, 5] (the absolute tolerance means something).
    python tests/golden/make_t2m_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO  # noqa: E402,F401

from syntalker_amd import synth  # noqa: E402

GAP, FIRST_SEED, DIVERSITY_TIMES, MM_TIMES = 2e-3, 100, 30, 10
EDGE_SEED, EDGE_M_LENS, EDGE_CAP_LENS = 90, (196, 23, 4), (22, 5, 1)
TIE_LENS = (64, 196, 64, 40, 196, 64, 100, 40, 196, 7)


def batch_tuple(b):
    word, pos, cap_lens, motions, m_lens = b
    return word, pos, None, cap_lens, motions, m_lens, None


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    spec = importlib.util.spec_from_file_location("ref_t2m_eval_tools", os.path.join(REF, "utils", "t2m_eval_tools.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    w = ref.EvaluatorMDMWrapper.__new__(ref.EvaluatorMDMWrapper)         # (its __init__ reads a checkpoint from a fixed path)
    w.opt, w.device = {"unit_length": 4}, "cpu"
    w.movement_encoder = ref.MovementConvEncoder(619, 512, 512)
    w.text_encoder = ref.TextEncoderBiGRUCo(word_size=300, pos_size=len(ref.POS_enumerator), hidden_size=512, output_size=512, device="cpu")
    w.motion_encoder = ref.MotionEncoderBiGRUCo(input_size=512, hidden_size=1024, output_size=512, device="cpu")
    out = {}
    for name in ("movement_encoder", "text_encoder", "motion_encoder"):
        m = getattr(w, name).eval()
        m.load_state_dict(synth.synth_t2m_state_dict(m, synth.T2M_STATE_SEEDS[name]), strict=True)
        sd = m.state_dict()
        out["keys_" + name] = np.array(list(sd.keys()))
        out["shapes_" + name] = np.array([",".join(map(str, v.shape)) for v in sd.values()])

    def embed(b):
        t, m = w.get_co_embeddings(*b)
        return t.numpy(), m.numpy()

    seeds, embs, seed = [], [], FIRST_SEED
    while len(seeds) < 4:
        t, m = embed(synth.synth_t2m_batch(32, seed))
        gaps = np.diff(np.sort(ref.euclidean_distance_matrix(t, m), axis=1)[:, :4], axis=1)
        print(f"seed {seed}: smallest gap at ranks 1-4 {gaps.min():.2e}, mean |emb| {np.abs(m).mean():.3f} / {np.abs(t).mean():.3f}")
        if gaps.min() >= GAP or len(seeds) == 3:                         # batch 3 is in loader b only (no R-precision test on the GPU)
            assert 0.05 <= np.abs(m).mean() <= 5 and 0.05 <= np.abs(t).mean() <= 5
            seeds.append(seed)
            embs.append((t, m))
        seed += 1
        assert seed < FIRST_SEED + 200, "no batch met the gap"
    out["batch_seeds"] = np.array(seeds)
    for k, (t, m) in enumerate(embs):
        out[f"text_{k}"], out[f"motion_{k}"] = t, m
    for k in range(3):
        gaps = np.diff(np.sort(ref.euclidean_distance_matrix(*embs[k]), axis=1)[:, :4], axis=1)
        assert gaps.min() >= GAP, (k, gaps.min())

    edge = synth.synth_t2m_batch(3, EDGE_SEED, m_lens=EDGE_M_LENS, cap_lens=EDGE_CAP_LENS)
    out["edge_text"], out["edge_motion"] = embed(edge)
    out["tie_lens"] = np.array(TIE_LENS)
    out["tie_align"] = np.argsort(torch.tensor(TIE_LENS).data.tolist())[::-1].copy()
    tie = synth.synth_t2m_batch(len(TIE_LENS), EDGE_SEED + 1, m_lens=TIE_LENS)
    out["tie_motion"] = w.get_motion_embeddings(tie[3], tie[4]).numpy()

    # every metric function on batches 0 .. 2
    for k in range(3):
        t, m = embs[k]
        d = ref.euclidean_distance_matrix(t, m)
        out[f"dist_{k}"] = d
        out[f"topk_{k}"] = ref.calculate_top_k(np.argsort(d, axis=1), top_k=3)
    allm = np.concatenate([m for _, m in embs[:3]])
    mu, cov = ref.calculate_activation_statistics(allm[:, :24])          # (24 of the 512 columns: a 512 x 512 fp64 covariance is 2 MB)
    mu2, cov2 = ref.calculate_activation_statistics(np.concatenate([embs[2][1], embs[3][1]])[:, :24])
    out["stat_mu"], out["stat_cov"] = mu, cov
    out["frechet_24"] = np.array(ref.calculate_frechet_distance(mu, cov, mu2, cov2))
    for k in range(3):
        np.random.seed(k)
        out[f"diversity_{k}"] = np.array(ref.calculate_diversity(allm, DIVERSITY_TIMES))
        np.random.seed(k)
        out[f"multimodality_{k}"] = np.array(ref.calculate_multimodality(allm.reshape(3, 32, -1), MM_TIMES))
    vals = np.array([[float(out[f"diversity_{k}"]), float(out[f"multimodality_{k}"])] for k in range(3)])
    out["metric_values"] = vals
    out["metric_mean"], out["metric_conf"] = ref.get_metric_statistics(vals, 3)

    # the loader-level functions
    batches = [batch_tuple(synth.synth_t2m_batch(32, s)) for s in seeds]
    loaders = {"a": batches[:3], "b": batches[2:]}
    with open(os.devnull, "w") as f:
        ms, rp, act = ref.evaluate_matching_score(w, loaders, f)
        fid = ref.evaluate_fid(w, loaders["b"], act, f)
        np.random.seed(7)
        div = ref.evaluate_diversity(act, f, DIVERSITY_TIMES)
        mm_loader = [(b[4][None, :12], b[5][None, :12]) for b in batches[:3]]
        np.random.seed(8)
        mm = ref.evaluate_multimodality(w, {"a": mm_loader}, f, MM_TIMES)
    for name in loaders:
        out["ms_" + name], out["rp_" + name] = np.array(ms[name]), np.array(rp[name])
        out["fid_" + name], out["div_" + name] = np.array(fid[name]), np.array(div[name])
        assert np.array_equal(act[name], np.concatenate([embs[k][1] for k in ((0, 1, 2) if name == "a" else (2, 3))]))
    out["mm_a"] = np.array(mm["a"])
    path = os.path.join(HERE, "t2m_evaluator_outputs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; seeds", seeds, "ms", ms, "rp", rp, "fid", fid, "div", div, "mm", mm)


if __name__ == "__main__":
    main()
