"""The h3d text-motion evaluator on the MI355X (syntalker_amd/t2m_evaluator.py, csrc/syn_t2m.inc) against the reference's recorded outputs
(tests/golden/t2m_evaluator_outputs.npz, make_t2m_golden.py) and the CPU restatement (tests/t2m_evaluator_ref.py).

Tolerances: rel-L2 <= 1e-5 and max |delta| <= 2e-5 on embeddings of mean magnitude 0.6.  The reference against an fp32 restatement that sums
in another order differs by 3e-6 / 8e-7, against its fp64 self by 2.6e-6 / 6.3e-7, so the gates sit 6x / 12x above fp32 reordering noise;
a split-bf16 product (3.9e-5 / 1.0e-5) fails the max-abs gate."""
import copy
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, metrics, synth, t2m_evaluator as te
from tests import t2m_evaluator_ref as ref
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
REL, ABS = 1e-5, 2e-5


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "t2m_evaluator_outputs.npz"))


@pytest.fixture(scope="module")
def state():
    return ref.build_state()


@pytest.fixture(scope="module")
def wrapper(state):
    return te.EvaluatorMDMWrapper("humanml", DEV, state=state)


def _close(got, want, what=""):
    got, want = torch.as_tensor(got).detach().cpu().float(), torch.as_tensor(want).float()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    rel, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"{what}: rel-L2 {rel:.2e} max |delta| {mx:.2e}")
    assert rel <= REL and mx <= ABS, (what, rel, mx)


def test_golden_co_embeddings_of_a_loader_batch(fx, wrapper):
    b = synth.synth_t2m_batch(32, int(fx["batch_seeds"][0]))
    text, motion = wrapper.get_co_embeddings(*b)                # CPU batches, as the loader hands them: the wrapper moves them
    assert text.dtype == motion.dtype == torch.float32 and text.device == motion.device == torch.device(DEV)
    _close(text, fx["text_0"], "text, 32 captions of 4-22 tokens")
    _close(motion, fx["motion_0"], "motion, 32 motions of 40-196 frames")


def test_golden_shortest_and_longest_sequences(fx, wrapper):
    """196, 23 and 4 frames are 49, 5 and 1 steps; 22, 5 and 1 tokens."""
    b = synth.synth_t2m_batch(3, 90, m_lens=(196, 23, 4), cap_lens=(22, 5, 1))
    text, motion = wrapper.get_co_embeddings(*b)
    _close(text, fx["edge_text"], "text (22, 5, 1)")
    _close(motion, fx["edge_motion"], "motion (196, 23, 4)")
    _close(wrapper.get_motion_embeddings(b[3], b[4]), fx["edge_motion"], "get_motion_embeddings (196, 23, 4)")


def test_tied_lengths_come_back_in_numpys_order(fx, wrapper):
    lens = [int(v) for v in fx["tie_lens"]]
    b = synth.synth_t2m_batch(len(lens), 91, m_lens=lens)
    got = wrapper.get_motion_embeddings(b[3].to(DEV), b[4])
    _close(got, fx["tie_motion"], "tied lengths")
    alone = torch.cat([wrapper.get_motion_embeddings(b[3][i:i + 1].to(DEV), b[4][i:i + 1]) for i in fx["tie_align"]])
    assert torch.equal(got, alone)                              # row k is input align_idx[k], not another motion of the same length


def _lens(n, lo, hi, seed):
    return torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed))


EDGE_CASES = {
    # name: (n, frames, text_len, m_lens, cap_lens)
    "one-sequence": (1, 8, 4, [7], [3]),
    "three": (3, 64, 9, [64, 9, 33], [2, 9, 5]),
    "tile-tail-196": (33, 196, 22, _lens(33, 40, 196, 1), _lens(33, 1, 22, 2)),
    "past-two-tiles": (70, 64, 12, _lens(70, 4, 64, 3), _lens(70, 1, 12, 4)),
    "all-equal": (33, 64, 6, [64] * 33, [6] * 33),
    "all-one-step": (20, 64, 5, _lens(20, 4, 7, 5), [1] * 20),
    "one-full-among-one-step": (17, 196, 22, [5, 4, 7, 6] * 2 + [196] + [4, 7, 5, 6] * 2, [1] * 8 + [22] + [1] * 8),
}


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_shapes_match_the_restatement(case, state, wrapper):
    n, frames, text_len, m_lens, cap_lens = EDGE_CASES[case]
    b = synth.synth_t2m_batch(n, 200 + n, frames=frames, text_len=text_len, m_lens=m_lens, cap_lens=cap_lens)    # cap_lens in any order
    text, motion = wrapper.get_co_embeddings(*b)
    want_text, want_motion = ref.co_embeddings(state, *b)
    _close(text, want_text, case + " text")
    _close(motion, want_motion, case + " motion")


def test_repeated_calls_and_batch_mates_do_not_change_a_row(state, wrapper):
    """Bitwise: a call repeated; a sequence alone against the same sequence sharing a tile with longer and shorter ones (a finished row's
    state stays untouched while its tile runs on); zero frames appended, to an even or odd length.

    Appended frames: the last of a motion's L = m_len // 4 steps reads the first convolution's positions up to 2 L, so frames up to
    4 L + 2.  Where the batch is at least that long (T >= 4 L + 2) everything past m_len is a zero either way and appending changes no bit.
    A motion that fills the batch (4 L + 2 > T) has the second convolution's own zero padding at position T // 2; in a longer batch that
    position is the first convolution over the motion's last frames, LeakyReLU(bias + ...) != 0, and the reference's embedding moves with
    it (0.34 on the 64-frame row here, CPU restatement).  Such rows are held to the restatement of the padded batch instead."""
    n, frames = 35, 64
    word, pos, cap_lens, motions, m_lens = synth.synth_t2m_batch(n, 300, frames=frames, text_len=10, m_lens=_lens(n, 4, frames, 6),
                                                                 cap_lens=_lens(n, 1, 10, 7))
    word, pos, motions = word.to(DEV), pos.to(DEV), motions.to(DEV)
    text, motion = wrapper.get_co_embeddings(word, pos, cap_lens, motions, m_lens)
    again = wrapper.get_co_embeddings(word, pos, cap_lens, motions, m_lens)
    assert torch.equal(text, again[0]) and torch.equal(motion, again[1])
    align = ref.align_idx(m_lens)
    for k in (0, 1, 15, 16, 17, 33, 34):
        i = int(align[k])
        assert torch.equal(motion[k:k + 1], wrapper.get_motion_embeddings(motions[i:i + 1], m_lens[i:i + 1])), (k, i)
        assert torch.equal(text[k:k + 1], wrapper.text_encoder(word[i:i + 1], pos[i:i + 1], cap_lens[i:i + 1])), (k, i)
    sorted_lens = m_lens[align]
    inside = (sorted_lens // 4 * 4 + 2 <= frames).to(DEV)       # rows whose last step reads nothing past the unpadded batch
    assert int(sorted_lens.max()) == frames and 0 < int(inside.sum()) < n
    for extra in (1, 4, 8, 11):
        padded = torch.cat([motions, torch.zeros(n, extra, motions.shape[2], device=DEV)], dim=1)
        got = wrapper.get_motion_embeddings(padded, m_lens)
        assert torch.equal(motion[inside], got[inside]), extra
        if (frames + extra) // 2 == frames // 2:                # the first convolution gains no position: every row
            assert torch.equal(motion, got), extra
        else:
            _close(got[~inside], ref.motion_embeddings(state, padded.cpu(), m_lens)[~inside.cpu()], f"full-length rows, {extra} frames appended")
    longer = torch.cat([word, torch.ones(n, 3, 300, device=DEV)], dim=1), torch.cat([pos, torch.zeros(n, 3, 15, device=DEV)], dim=1)
    assert torch.equal(text, wrapper.get_co_embeddings(*longer, cap_lens, motions, m_lens)[0])


def test_refusals(wrapper):
    word, pos, cap_lens, motions, m_lens = synth.synth_t2m_batch(3, 301, frames=16, text_len=4, m_lens=[16, 8, 4], cap_lens=[4, 2, 1])
    g = lambda t: t.to(DEV)
    for bad_motions, bad_lens in ((motions[..., :-1], m_lens), (motions, torch.tensor([16, 8, 3])), (motions, torch.tensor([17, 8, 4])),
                                  (motions[:0], m_lens[:0]), (motions, m_lens[:2]), (motions[:, :3], torch.tensor([3, 3, 3]))):
        with pytest.raises(ValueError):
            wrapper.get_motion_embeddings(g(bad_motions), bad_lens)
    for bad in ((word[..., :-1], pos, cap_lens), (word, pos[..., :-1], cap_lens), (word, pos, torch.tensor([4, 2, 0])),
                (word, pos, torch.tensor([5, 2, 1])), (word[:0], pos[:0], cap_lens[:0])):
        with pytest.raises(ValueError):
            wrapper.text_encoder(g(bad[0]), g(bad[1]), bad[2])
    with pytest.raises(ValueError):
        wrapper.get_co_embeddings(word, pos, torch.tensor([4, 2, 0]), motions, m_lens)
    with pytest.raises(_lib.SynHipError):                      # the encoders take GPU tensors only; the wrapper moves its inputs as the reference's does
        wrapper.text_encoder(word, pos, cap_lens)
    with pytest.raises(_lib.SynHipError):
        te.embed_motions(wrapper.movement_encoder, wrapper.motion_encoder, motions, m_lens)
    with pytest.raises(_lib.SynHipError):
        te.EvaluatorMDMWrapper("humanml", "cpu", state=ref.build_state()).get_motion_embeddings(motions, m_lens)
    with pytest.raises(NotImplementedError):
        wrapper.text_encoder.train()


def test_loading_other_weights_repacks(state):
    w = te.EvaluatorMDMWrapper("humanml", DEV, state=state)
    b = synth.synth_t2m_batch(5, 302, frames=32, text_len=6, m_lens=[32, 4, 17, 9, 32], cap_lens=[6, 1, 3, 6, 2])
    before = w.get_co_embeddings(*b)
    other = ref.build_state(shift=10)
    for name in other:
        getattr(w, name).load_state_dict(other[name])
    after = w.get_co_embeddings(*b)
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    want = ref.co_embeddings(other, *b)
    _close(after[0], want[0], "text after load_state_dict")
    _close(after[1], want[1], "motion after load_state_dict")


def test_motion_embeddings_in_a_cuda_graph(wrapper):
    m_lens = torch.tensor([40, 64, 12, 64, 7])
    x = synth.synth_t2m_batch(5, 303, frames=64, m_lens=m_lens)[3].to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        wrapper.get_motion_embeddings(x, m_lens)               # warm: packed weights, workspace and index tensors exist before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = wrapper.get_motion_embeddings(x, m_lens)
    x.copy_(synth.synth_t2m_batch(5, 304, frames=64, m_lens=m_lens)[3].to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, wrapper.get_motion_embeddings(x, m_lens))


def test_used_wrapper_deep_copies_and_pickles(wrapper):
    b = synth.synth_t2m_batch(4, 305, frames=32, text_len=5, m_lens=[32, 30, 8, 5], cap_lens=[5, 4, 2, 1])
    text, motion = wrapper.get_co_embeddings(*b)
    mods = lambda w: (w, w.text_encoder, w.motion_encoder, w.movement_encoder)
    assert all(any(k.startswith("_syn_") for k in m.__dict__) for m in mods(wrapper))
    buf = io.BytesIO()
    torch.save(wrapper, buf)
    buf.seek(0)
    for w2 in (copy.deepcopy(wrapper), torch.load(buf, weights_only=False)):
        assert not any(k.startswith("_syn_") for m in mods(w2) for k in m.__dict__)
        t2, m2 = w2.get_co_embeddings(*b)
        assert torch.equal(t2, text) and torch.equal(m2, motion)


def test_metrics_end_to_end_match_the_references(fx, wrapper):
    """Matching Score within 1e-5 relative, R-precision counts equal (the fixture's batches keep >= 2e-3 between the distances that decide
    ranks 1-3, twice what a 2e-5 embedding error can move one), FID within 1e-4 relative (the margin of test_fgd_matches_the_reference_fgd)."""
    batches = [synth.synth_t2m_batch(32, int(s)) for s in fx["batch_seeds"]]
    tuples = [(b[0], b[1], None, b[2], b[3], b[4], None) for b in batches]
    loaders = {"a": tuples[:3], "b": tuples[2:]}
    log = io.StringIO()
    ms, rp, act = metrics.evaluate_matching_score(wrapper, loaders, log)
    for name in loaders:
        want = float(fx["ms_" + name])
        print(f"matching score {name}: {float(ms[name]):.6f} vs {want:.6f}")
        assert abs(float(ms[name]) - want) <= 1e-5 * want
    n_a = 96
    assert np.array_equal(np.rint(rp["a"] * n_a), np.rint(fx["rp_a"] * n_a))
    fid = metrics.evaluate_fid(wrapper, loaders["b"], act, log)
    want = float(fx["fid_a"])
    print(f"FID a: {fid['a']:.6f} vs {want:.6f}")
    assert abs(fid["a"] - want) <= 1e-4 * want
    # a loader embedded in one call gives what a call per batch gives
    per_batch = np.concatenate([wrapper.get_co_embeddings(*b)[1].cpu().numpy() for b in batches[:3]])
    assert np.array_equal(act["a"], per_batch)
    mm_loader = [(b[3][None, :12], b[4][None, :12]) for b in batches[:3]]
    np.random.seed(8)
    mm = metrics.evaluate_multimodality(wrapper, {"a": mm_loader}, log, 10)
    assert abs(float(mm["a"]) - float(fx["mm_a"])) <= 1e-5 * float(fx["mm_a"])


def test_c_abi_refuses_null_and_zero_arguments():
    lib = _lib.load()
    model = _lib.SynT2mModel()                                  # all NULL
    one = torch.zeros(64, device=DEV)
    p = one.data_ptr()
    assert lib.syn_t2m_pack_weight(None, 16, 16, 0, 0, p, None) != 0 and lib.syn_t2m_pack_weight(p, 16, 16, 0, 0, None, None) != 0
    assert lib.syn_t2m_pack_weight(p, 0, 16, 0, 0, p, None) != 0 and lib.syn_t2m_pack_weight(p, 16, 0, 0, 0, p, None) != 0
    assert lib.syn_t2m_pack_weight(p, 16, 16, 5, 0, p, None) != 0 and lib.syn_t2m_pack_weight(p, 16, 16, 0, 256, p, None) != 0
    assert lib.syn_t2m_workspace_bytes(0, 196, 0) < 0 and lib.syn_t2m_workspace_bytes(4, 3, 0) < 0 and lib.syn_t2m_workspace_bytes(4, 0, 1) < 0
    assert lib.syn_t2m_workspace_bytes(4, 196, 2) < 0 and lib.syn_t2m_workspace_bytes(4, 196, 0) > 0 and lib.syn_t2m_workspace_bytes(1, 1, 1) > 0
    m = C.byref(model)
    assert lib.syn_t2m_encode_motion(None, p, 1, 8, 623, p, p, p, p, None) != 0
    assert lib.syn_t2m_encode_motion(m, p, 1, 8, 623, p, p, p, p, None) != 0              # a model of NULL pointers
    for args in ((None, 1, 8, 623, p, p, p, p), (p, 0, 8, 623, p, p, p, p), (p, 1, 3, 623, p, p, p, p), (p, 1, 8, 618, p, p, p, p),
                 (p, 1, 8, 623, None, p, p, p), (p, 1, 8, 623, p, None, p, p), (p, 1, 8, 623, p, p, None, p), (p, 1, 8, 623, p, p, p, None)):
        assert lib.syn_t2m_encode_motion(m, *args, None) != 0, args
    for args in ((None, p, 1, 4, p, p, p, p), (p, None, 1, 4, p, p, p, p), (p, p, 0, 4, p, p, p, p), (p, p, 1, 0, p, p, p, p),
                 (p, p, 1, 4, None, p, p, p), (p, p, 1, 4, p, p, None, p), (p, p, 1, 4, p, p, p, None), (p, p, 1, 4, p, p, p, p)):
        assert lib.syn_t2m_encode_text(m, *args, None) != 0, args
    assert b"syn_t2m" in lib.syn_last_error()
    torch.cuda.synchronize()
    assert float(one.abs().sum()) == 0.0                        # nothing was launched on the buffers
