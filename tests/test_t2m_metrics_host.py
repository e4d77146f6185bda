"""The h3d text-motion evaluator without a GPU: the metric functions of syntalker_amd.metrics against the reference's recorded results
(tests/golden/t2m_evaluator_outputs.npz, make_t2m_golden.py), the loader-level evaluate_* over a stub wrapper that returns the recorded
embeddings, the three modules' state_dict layout, the wrapper's output order, the refusals and the drop-in import name."""
import io
import os
import sys

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, metrics, synth, t2m_evaluator as te
from tests import t2m_evaluator_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
DIVERSITY_TIMES, MM_TIMES = 30, 10             # make_t2m_golden.py


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "t2m_evaluator_outputs.npz"))


def close(got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.all(np.abs(got - want) <= rel * np.abs(want))


def test_distance_matrix_and_top_k_are_the_references(fx):
    for k in range(3):
        d = metrics.euclidean_distance_matrix(fx[f"text_{k}"], fx[f"motion_{k}"])
        assert d.dtype == fx[f"dist_{k}"].dtype and close(d, fx[f"dist_{k}"])
        top = metrics.calculate_top_k(np.argsort(d, axis=1), top_k=3)
        assert top.dtype == np.bool_ and top.shape == (32, 3) and np.array_equal(top, fx[f"topk_{k}"])
    mat = np.array([[2, 0, 1], [1, 2, 0], [0, 1, 2]])
    assert metrics.calculate_top_k(mat, 3).tolist() == [[False, True, True], [True, True, True], [False, False, True]]


def test_activation_statistics_and_frechet_distance(fx):
    a = np.concatenate([fx[f"motion_{k}"] for k in range(3)])[:, :24]
    b = np.concatenate([fx["motion_2"], fx["motion_3"]])[:, :24]
    mu, cov = metrics.calculate_activation_statistics(a)
    assert mu.dtype == fx["stat_mu"].dtype and close(mu, fx["stat_mu"]) and close(cov, fx["stat_cov"])
    got = metrics.t2m_frechet_distance(mu, cov, *metrics.calculate_activation_statistics(b))
    assert close(got, fx["frechet_24"], 1e-10)                  # (sqrtm's own reproducibility across BLAS builds)


def test_frechet_distance_raises_on_an_imaginary_component(monkeypatch):
    from scipy import linalg
    monkeypatch.setattr(linalg, "sqrtm", lambda m, disp=False: (np.eye(2) * (1 + 0.5j), 0.0))
    with pytest.raises(ValueError, match="Imaginary component"):
        metrics.t2m_frechet_distance(np.zeros(2), np.eye(2), np.zeros(2), np.eye(2))
    assert metrics.frechet_from_stats(np.zeros(2), np.eye(2), np.zeros(2), np.eye(2)) == 1e10      # the FGD's variant keeps its sentinel


def test_diversity_and_multimodality_draw_like_the_reference(fx):
    allm = np.concatenate([fx[f"motion_{k}"] for k in range(3)])
    for k in range(3):
        np.random.seed(k)
        assert close(metrics.calculate_diversity(allm, DIVERSITY_TIMES), fx[f"diversity_{k}"])
        after = np.random.randint(1 << 30)
        np.random.seed(k)
        np.random.choice(len(allm), DIVERSITY_TIMES, replace=False)
        np.random.choice(len(allm), DIVERSITY_TIMES, replace=False)
        assert after == np.random.randint(1 << 30)              # two draws of that size, nothing else, from the global RNG
        np.random.seed(k)
        assert close(metrics.calculate_multimodality(allm.reshape(3, 32, -1), MM_TIMES), fx[f"multimodality_{k}"])
    mean, conf = metrics.get_metric_statistics(fx["metric_values"], 3)
    assert close(mean, fx["metric_mean"]) and close(conf, fx["metric_conf"])
    with pytest.raises(AssertionError):
        metrics.calculate_diversity(allm[:DIVERSITY_TIMES], DIVERSITY_TIMES)


class StubWrapper:
    """Returns the recorded embeddings of the batch it is handed (recognised by its m_lens)."""

    def __init__(self, fx, batches):
        self.by_lens = {tuple(b[5].tolist()): (fx[f"text_{k}"], fx[f"motion_{k}"]) for k, b in enumerate(batches)}
        self.calls = 0

    def get_co_embeddings(self, word_embs, pos_ohot, cap_lens, motions, m_lens):
        self.calls += 1
        t, m = self.by_lens[tuple(m_lens.tolist())]
        return torch.from_numpy(t), torch.from_numpy(m)

    def get_motion_embeddings(self, motions, m_lens):
        self.calls += 1
        key = tuple(m_lens.tolist())                            # (12 long: the multimodality loader, the first 12 motions of a batch)
        full, m = next((k, v[1]) for k, v in self.by_lens.items() if k[:len(key)] == key)
        by_input = np.empty_like(m)
        by_input[ref.align_idx(torch.tensor(full))] = m         # recorded in the 32's align_idx order
        return torch.from_numpy(by_input[:len(key)][ref.align_idx(m_lens)])


def test_evaluate_functions_over_in_memory_loaders(fx, capsys):
    batches = [synth.synth_t2m_batch(32, int(s)) for s in fx["batch_seeds"]]
    tuples = [(b[0], b[1], None, b[2], b[3], b[4], None) for b in batches]
    loaders = {"a": tuples[:3], "b": tuples[2:]}
    w = StubWrapper(fx, tuples)
    log = io.StringIO()
    ms, rp, act = metrics.evaluate_matching_score(w, loaders, log)
    assert list(ms) == list(rp) == list(act) == ["a", "b"] and w.calls == 5            # a foreign wrapper is called batch by batch
    for name in loaders:
        assert close(ms[name], fx["ms_" + name]) and np.array_equal(rp[name], fx["rp_" + name])
    assert np.array_equal(act["a"], np.concatenate([fx[f"motion_{k}"] for k in range(3)]))
    fid = metrics.evaluate_fid(w, loaders["b"], act, log)
    assert close(fid["a"], fx["fid_a"], 1e-9) and abs(fid["b"] - float(fx["fid_b"])) < 1e-6
    np.random.seed(7)
    div = metrics.evaluate_diversity(act, log, DIVERSITY_TIMES)
    assert all(close(div[n], fx["div_" + n]) for n in loaders)
    np.random.seed(8)
    mm = metrics.evaluate_multimodality(w, {"a": [(b[4][None, :12], b[5][None, :12]) for b in tuples[:3]], "none": []}, log, MM_TIMES)
    assert close(mm["a"], fx["mm_a"], 1e-6)                     # (recorded from calls of 12; the stub cuts them out of calls of 32)
    assert mm["none"] == 0
    text = log.getvalue()
    assert "---> [a] Matching Score: 24.5108" in text and "(top 3): 0.0625" in text and "---> [a] FID: 77.4534" in text
    assert "---> [a] Diversity:" in text and "---> [a] Multimodality:" in text
    printed = capsys.readouterr().out
    assert all(line in printed for line in text.splitlines())   # the reference prints each line to stdout too


def test_state_dicts_have_the_references_layout_and_load_strictly(fx):
    state = ref.build_state()
    mods = {"movement_encoder": te.MovementConvEncoder(619, 512, 512), "text_encoder": te.TextEncoderBiGRUCo(300, 15, 512, 512, "cpu"),
            "motion_encoder": te.MotionEncoderBiGRUCo(512, 1024, 512, "cpu")}
    for name, m in mods.items():
        sd = m.state_dict()
        assert list(sd.keys()) == list(fx["keys_" + name])
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(fx["shapes_" + name])
        m.load_state_dict(state[name], strict=True)
        assert not m.training
    with pytest.raises(RuntimeError):
        mods["motion_encoder"].load_state_dict({k: v for k, v in state["motion_encoder"].items() if k != "hidden"}, strict=True)


def test_wrapper_loads_a_checkpoint_file_or_state_dicts(tmp_path):
    state = ref.build_state()
    d = tmp_path / "t2m" / "text_mot_match" / "model"
    d.mkdir(parents=True)
    torch.save({**state, "epoch": 3}, d / "finest.tar")
    w = te.EvaluatorMDMWrapper("humanml", "cpu", checkpoints_dir=str(tmp_path))
    w2 = te.EvaluatorMDMWrapper("humanml", "cpu", state=state)
    for a, b in ((w.text_encoder, w2.text_encoder), (w.motion_encoder, w2.motion_encoder), (w.movement_encoder, w2.movement_encoder)):
        assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values())) and not a.training
    with pytest.raises(ValueError):
        te.EvaluatorMDMWrapper("humanml", "cpu")


def test_align_idx_keeps_numpys_tie_order(fx):
    lens = torch.tensor(fx["tie_lens"])
    assert np.array_equal(ref.align_idx(lens), fx["tie_align"])
    assert np.array_equal(metrics._align(lens), fx["tie_align"])


def test_modules_are_eval_only_and_refuse_the_cpu():
    w = te.EvaluatorMDMWrapper("humanml", "cpu", state=ref.build_state())
    for m in (w.text_encoder, w.motion_encoder, w.movement_encoder):
        with pytest.raises(NotImplementedError):
            m.train()
        with pytest.raises(NotImplementedError):
            m.train(True)
        assert m.eval() is m and not m.training
        with pytest.raises(_lib.SynHipError):
            m.packed()
    word, pos, cap_lens, motions, m_lens = synth.synth_t2m_batch(2, 1, frames=16, text_len=4, m_range=(8, 16), cap_range=(1, 4))
    with pytest.raises(_lib.SynHipError):
        w.get_motion_embeddings(motions, m_lens)
    with pytest.raises(_lib.SynHipError):
        w.get_co_embeddings(word, pos, cap_lens, motions, m_lens)
    with pytest.raises(_lib.SynHipError):
        w.text_encoder(word, pos, cap_lens)
    with pytest.raises(NotImplementedError):
        w.movement_encoder(motions[..., :-4])


def test_c_structs_match_their_ctypes_mirrors():
    import ctypes as C
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.SynT2mGru) == 6 * p and C.sizeof(_lib.SynT2mHead) == 6 * p
    assert C.sizeof(_lib.SynT2mModel) == (8 + 4) * p + 2 * (6 + 6) * p
    header = open(os.path.join(os.path.dirname(HERE), "include", "syn_hip.h")).read()
    for name in ("syn_t2m_pack_weight", "syn_t2m_workspace_bytes", "syn_t2m_encode_motion", "syn_t2m_encode_text"):
        assert name in _lib.EXPORTS and name + "(" in header
    for macro, value in (("SYN_T2M_POSE", _lib.SYN_T2M_POSE), ("SYN_T2M_MOTION_H", _lib.SYN_T2M_MOTION_H), ("SYN_T2M_TEXT_H", _lib.SYN_T2M_TEXT_H),
                         ("SYN_T2M_MAX_SEQ", _lib.SYN_T2M_MAX_SEQ), ("SYN_T2M_MAX_FRAMES", _lib.SYN_T2M_MAX_FRAMES)):
        assert any(line.split()[:3] == ["#define", macro, str(value)] for line in header.splitlines()), macro


def test_dropin_import_path_resolves():
    from syntalker_amd import dropin
    saved = {k: sys.modules.get(k) for k in ("utils", "utils.t2m_eval_tools")}
    path = os.path.dirname(dropin.__file__)
    sys.path.insert(0, path)
    try:
        for k in saved:
            sys.modules.pop(k, None)
        from utils.t2m_eval_tools import EvaluatorMDMWrapper, calculate_frechet_distance, evaluate_fid, evaluate_matching_score  # noqa: F401
        assert EvaluatorMDMWrapper is te.EvaluatorMDMWrapper and evaluate_fid is metrics.evaluate_fid
        assert calculate_frechet_distance is metrics.t2m_frechet_distance
        for k in saved:
            sys.modules.pop(k, None)
        dropin.install()
        assert "utils.t2m_eval_tools" not in sys.modules
        dropin.install(t2m=True)
        assert sys.modules["utils.t2m_eval_tools"].EvaluatorMDMWrapper is te.EvaluatorMDMWrapper
    finally:
        sys.path.remove(path)
        for k, v in saved.items():
            sys.modules.pop(k, None)
            if v is not None:
                sys.modules[k] = v
