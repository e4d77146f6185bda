"""DistilBERT on the HIP kernels (syn_bert_encode, DistilbertActorAgnosticEncoder(text_on_hip=True)) vs the reference's outputs
(tests/golden/distilbert_outputs.npz, make_distilbert_golden.py; tmr_outputs.npz): hidden states rel-L2 per prompt <= 5e-3, loc <= 5e-3 and
scale <= 1e-2 per prompt (test_gpu_tmr.py's constants); the HIP path really runs, batch invariance, determinism, zero padding rows, graph
capture, staleness of the packed copy, limits."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, synth, tmr
from tests.conftest import rel_l2

pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda"
HIDDEN_TOL, LOC_TOL, SCALE_TOL = 5e-3, 5e-3, 1e-2


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "distilbert_outputs.npz"))


@pytest.fixture(scope="module")
def tmr_fx():
    return np.load(os.path.join(HERE, "golden", "tmr_outputs.npz"))


def _build(path, layers):
    synth.synth_tmr_text_model(str(path), seed=33, layers=layers)
    m = tmr.DistilbertActorAgnosticEncoder(str(path), num_layers=4, text_on_hip=True)
    m.load_state_dict(synth.synth_tmr_state_dict(m))
    return m.to(DEV)


@pytest.fixture(scope="module")
def enc2(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("distilbert2"), 2)


@pytest.fixture(scope="module")
def enc6(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("distilbert6"), 6)


def _inputs(fx, key):
    return torch.from_numpy(fx[key + "ids"]).to(DEV), torch.from_numpy(fx[key + "lengths"]).to(DEV)


@pytest.fixture(scope="module")
def ragged(enc2, fx):
    """The ragged batch (b) once: ids, lengths, hidden states, mu, logvar.  Read-only."""
    ids, lengths = _inputs(fx, "l2_ragged_")
    hidden = enc2.hidden_states(ids, lengths)
    mu, logvar = enc2.encode_ids(ids, lengths)
    return ids, lengths, hidden, mu, logvar


def _worst(errs, tol, what):
    print(f"{what}: worst rel-L2 {max(errs):.3e}")
    assert max(errs) <= tol, (what, errs)


@pytest.mark.parametrize("layers", [2, 6])
def test_hidden_states_vs_reference(layers, enc2, enc6, fx):
    m = enc2 if layers == 2 else enc6
    for name in ("text3", "text1"):
        key = f"l{layers}_{name}_"
        ids, lengths = _inputs(fx, key)
        hidden = m.hidden_states(ids, lengths).cpu()
        assert hidden.shape == (ids.shape[0], ids.shape[1], 768) and hidden.dtype == torch.float32
        want = torch.from_numpy(fx[key + "hidden"])
        errs, at = [], 0
        for b, n in enumerate(fx[key + "lengths"]):
            errs.append(rel_l2(hidden[b, :n], want[at:at + n]))
            at += n
        _worst(errs, HIDDEN_TOL, f"{layers} layers {name} hidden states")


def test_hidden_rows_of_the_ragged_batch_vs_reference(ragged, fx):
    hidden = ragged[2].cpu()
    rows, want = fx["l2_ragged_rows"], torch.from_numpy(fx["l2_ragged_hidden"])
    errs = []
    for b in range(hidden.shape[0]):
        pick = np.nonzero(rows[:, 0] == b)[0]
        errs.append(rel_l2(hidden[b, rows[pick, 1]], want[pick]))
    _worst(errs, HIDDEN_TOL, "2 layers ragged 2 .. 254 hidden rows")


@pytest.mark.parametrize("layers", [2, 6])
def test_whole_path_vs_reference(layers, enc2, enc6, fx, ragged):
    m = enc2 if layers == 2 else enc6
    for name, prompts in (("text3", synth.TMR_PROMPTS), ("text1", synth.TMR_PROMPT_ONE)):
        d = m(prompts)
        key = f"l{layers}_{name}_"
        assert d.loc.shape == (fx[key + "loc"].shape[0], 256)
        _worst([rel_l2(g, w) for g, w in zip(d.loc.cpu(), fx[key + "loc"])], LOC_TOL, f"{layers} layers {name} loc")
        _worst([rel_l2(g, w) for g, w in zip(d.scale.cpu(), fx[key + "scale"])], SCALE_TOL, f"{layers} layers {name} scale")
    if layers == 2:
        mu, logvar = ragged[3], ragged[4]
        _worst([rel_l2(g, w) for g, w in zip(mu.cpu(), fx["l2_ragged_loc"])], LOC_TOL, "2 layers ragged loc")
        _worst([rel_l2(g, w) for g, w in zip(logvar.exp().pow(0.5).cpu(), fx["l2_ragged_scale"])], SCALE_TOL, "2 layers ragged scale")


def test_whole_path_vs_the_tmr_fixture(enc2, tmr_fx):
    """The existing tmr_outputs.npz text keys (test_gpu_tmr.py's `text` fixture, DistilBERT on PyTorch there) with DistilBERT on HIP."""
    for name, prompts in (("text3", synth.TMR_PROMPTS), ("text1", synth.TMR_PROMPT_ONE)):
        d = enc2(prompts)
        _worst([rel_l2(g, w) for g, w in zip(d.loc.cpu(), tmr_fx[name + "_loc"])], LOC_TOL, f"tmr_outputs {name} loc")
        _worst([rel_l2(g, w) for g, w in zip(d.scale.cpu(), tmr_fx[name + "_scale"])], SCALE_TOL, f"tmr_outputs {name} scale")


def test_the_hip_path_runs_without_the_torch_module(enc2, fx, monkeypatch):
    want = enc2(synth.TMR_PROMPTS).loc

    def refuse(*a, **k):
        raise AssertionError("text_model.forward ran on the text_on_hip path")
    monkeypatch.setattr(enc2.text_model, "forward", refuse)
    for sub in enc2.text_model.modules():
        if sub is not enc2.text_model:
            monkeypatch.setattr(sub, "forward", refuse)
    d = enc2(synth.TMR_PROMPTS)
    assert torch.equal(d.loc, want) and d.loc.shape == (3, 256)


def test_prompt_alone_equals_prompt_in_batch_and_calls_repeat(enc2, ragged):
    ids, lengths, hidden, mu, logvar = ragged
    again = enc2.hidden_states(ids, lengths)
    mu2, lv2 = enc2.encode_ids(ids, lengths)
    assert torch.equal(again, hidden) and torch.equal(mu2, mu) and torch.equal(lv2, logvar)
    for b, n in enumerate(lengths.tolist()):
        assert n == synth.TMR_RAGGED_TOKENS[b]
        assert (hidden[b, n:] == 0).all(), b                      # padding rows are exactly zero
        assert torch.isfinite(hidden[b, :n]).all() and (hidden[b, :n].abs().sum(1) > 0).all(), b
        h1 = enc2.hidden_states(ids[b:b + 1, :n], lengths[b:b + 1])
        m1, l1 = enc2.encode_ids(ids[b:b + 1, :n], lengths[b:b + 1])
        assert torch.equal(h1[0], hidden[b, :n]), b
        assert torch.equal(m1[0], mu[b]) and torch.equal(l1[0], logvar[b]), b


def test_encode_ids_in_a_cuda_graph(enc2, fx):
    ids, lengths = _inputs(fx, "l2_text3_")
    ids, lengths = ids.clone(), lengths.clone()
    other_ids = torch.from_numpy(fx["l2_ragged_ids"][1:4, :ids.shape[1]].copy()).to(DEV)     # other tokens, other lengths, same buffers
    other_lengths = torch.tensor([13, 2, 9], dtype=lengths.dtype, device=DEV)
    want = enc2.encode_ids(ids, lengths)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc2.encode_ids(ids, lengths)                          # warm: packed weights and the workspaces exist before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = enc2.encode_ids(ids, lengths)
    first_ids, first_lengths = ids.clone(), lengths.clone()
    ids.copy_(other_ids)
    lengths.copy_(other_lengths)
    g.replay()
    torch.cuda.synchronize()
    fresh = enc2.encode_ids(ids, lengths)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    assert not torch.equal(fresh[0], want[0])
    ids.copy_(first_ids)
    lengths.copy_(first_lengths)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_packed_copy_follows_weight_writes_and_stays_out_of_deep_copies(tmp_path, fx):
    """`m.text_model.transformer.layer[1].ffn.lin2.weight.data.mul_(1.5)`: a write through `.data` goes past the parameter's version counter
    (`.data` carries its own), so it is followed by what `engine.weights_key` asks of every writer PyTorch cannot see,
    `torch.autograd.graph.increment_version` on the tensor written.  The output changes and equals a freshly built module's."""
    m = _build(tmp_path / "a", 2)
    ids, lengths = _inputs(fx, "l2_text3_")
    before = [t.clone() for t in m.encode_ids(ids, lengths)]
    assert "_syn_packed" in m.__dict__ and "bert" in m.__dict__["_syn_packed"]
    m2 = copy.deepcopy(m)                                      # a used module copies without its packed caches and encodes the same
    assert not any(k.startswith("_syn_") for k in m2.__dict__)
    again = m2.encode_ids(ids, lengths)
    assert torch.equal(again[0], before[0]) and torch.equal(again[1], before[1])
    w = m.text_model.transformer.layer[1].ffn.lin2.weight
    w.data.mul_(1.5)
    torch.autograd.graph.increment_version(w)
    after = m.encode_ids(ids, lengths)
    assert not torch.equal(after[0], before[0])
    fresh = tmr.DistilbertActorAgnosticEncoder(str(tmp_path / "a"), num_layers=4, text_on_hip=True)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    got = fresh.to(DEV).encode_ids(ids, lengths)
    assert torch.equal(got[0], after[0]) and torch.equal(got[1], after[1])
    m.load_state_dict({k: v.cpu() for k, v in m2.state_dict().items()})       # load_state_dict re-packs as well
    back = m.encode_ids(ids, lengths)
    assert torch.equal(back[0], before[0]) and torch.equal(back[1], before[1])


def test_limits(enc2):
    with pytest.raises(ValueError):
        enc2.encode_ids(torch.zeros(1, tmr.MAX_LEN + 1, dtype=torch.int64, device=DEV), torch.tensor([tmr.MAX_LEN + 1], device=DEV))
    with pytest.raises(ValueError):
        enc2.hidden_states(torch.zeros(2, 8, dtype=torch.int64, device=DEV), torch.tensor([8], device=DEV))
    p = enc2.packed()
    lib = _lib.load()
    ids = torch.zeros(1, 255, dtype=torch.int32, device=DEV)
    ws = torch.empty(tmr.bert_workspace_bytes(1, 255), dtype=torch.uint8, device=DEV)
    canary = torch.full((1, 255, 768), 7.0, device=DEV)
    call = lambda model, max_len: lib.syn_bert_encode(ctypes.byref(model), ids.data_ptr(), 1, max_len, None, ws.data_ptr(), canary.data_ptr(), None)
    assert call(p["bert"], 255) != 0 and b"max_len" in lib.syn_last_error()
    bad = _lib.SynBertModel.from_buffer_copy(p["bert"])
    for n in (0, 13):
        bad.n_layers = n
        assert call(bad, 16) != 0 and b"n_layers" in lib.syn_last_error()
    torch.cuda.synchronize()
    assert (canary == 7.0).all()                               # nothing was launched
    full = enc2.hidden_states(torch.full((1, tmr.MAX_LEN), 5, dtype=torch.int64, device=DEV), torch.tensor([tmr.MAX_LEN], device=DEV))
    assert torch.isfinite(full).all()                          # the largest supported length runs
