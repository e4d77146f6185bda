"""DistilBERT on the HIP kernels (syntalker_amd/tmr.py, text_on_hip=True) without a GPU: the tokenizer against the golden's ids, the constructor's
contract, the state_dict, the workspace formula and the C structs against the header, the entry point's binding, and the precision
emulation's fp32 restatement against transformers."""
import ctypes
import importlib.util
import inspect
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, synth, tmr
from tests.conftest import rel_l2

pytest.importorskip("transformers")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "distilbert_outputs.npz"))


@pytest.fixture(scope="module")
def text_dir(tmp_path_factory):
    return synth.synth_tmr_text_model(str(tmp_path_factory.mktemp("distilbert")))        # seed 33, 2 layers


@pytest.fixture(scope="module")
def on(text_dir):
    m = tmr.DistilbertActorAgnosticEncoder(text_dir, num_layers=4, text_on_hip=True)
    m.load_state_dict(synth.synth_tmr_state_dict(m), strict=True)
    return m


def test_tokenizer_reproduces_the_golden_ids(on, fx):
    for name, prompts in (("text3", synth.TMR_PROMPTS), ("text1", synth.TMR_PROMPT_ONE), ("ragged", synth.synth_tmr_prompts(synth.TMR_RAGGED_TOKENS))):
        ids, mask = on.tokenize(prompts)
        assert np.array_equal(ids.numpy(), fx[f"l2_{name}_ids"]), name
        assert np.array_equal(mask.sum(1).numpy(), fx[f"l2_{name}_lengths"]), name
        if name != "ragged":                                       # the same tokenizer files at either depth
            assert np.array_equal(fx[f"l6_{name}_ids"], fx[f"l2_{name}_ids"])
    assert tuple(fx["l2_ragged_lengths"]) == synth.TMR_RAGGED_TOKENS
    assert [int(v) for v in fx["l2_text3_lengths"]] == [8, 13, 5] and int(fx["l2_text1_lengths"][0]) == 10
    for b, n in enumerate(fx["l2_ragged_lengths"]):                # right padding: the mask is a prefix of ones
        assert (fx["l2_ragged_ids"][b, n:] == 0).all() and (fx["l2_ragged_ids"][b, :n] != 0).all()


def test_text_on_hip_is_a_named_parameter_and_an_attribute(text_dir, on):
    p = inspect.signature(tmr.DistilbertActorAgnosticEncoder.__init__).parameters["text_on_hip"]
    assert p.default is False and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    off = tmr.DistilbertActorAgnosticEncoder(text_dir, num_layers=4)
    assert off.text_on_hip is False and on.text_on_hip is True
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert [tuple(v.shape) for v in on.state_dict().values()] == [tuple(v.shape) for v in off.state_dict().values()]
    off.load_state_dict(on.state_dict(), strict=True)
    with pytest.raises(_lib.SynHipError):                           # the HIP DistilBERT is an opt-in, and there is no CPU fallback for it
        off.encode_ids(torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4]))
    with pytest.raises(_lib.SynHipError):
        on.encode_ids(torch.zeros(1, 4, dtype=torch.int64), torch.tensor([4]))


def _model_dir(path, **over):
    """synth.synth_tmr_text_model's directory with other configuration fields (one layer unless asked: small)."""
    from transformers import DistilBertConfig, DistilBertModel, DistilBertTokenizer
    synth.synth_tmr_text_model(str(path), layers=1)
    vocab = len(open(os.path.join(path, "vocab.txt")).read().split())
    cfg = dict(vocab_size=vocab, dim=768, n_layers=1, n_heads=12, hidden_dim=3072, max_position_embeddings=512)
    cfg.update(over)
    DistilBertModel(DistilBertConfig(**cfg)).save_pretrained(str(path))
    return str(path)


@pytest.mark.parametrize("field,over", [("dim", dict(dim=384)), ("n_heads", dict(n_heads=8)), ("hidden_dim", dict(hidden_dim=1024)),
                                        ("activation", dict(activation="relu")), ("n_layers", dict(n_layers=13, dim=768))])
def test_unsupported_configurations_raise_at_construction(tmp_path, field, over):
    if field == "n_layers":                                        # 13 layers: only the configuration says so (no 13-layer file is written)
        path = _model_dir(tmp_path)
        cfg = json.load(open(os.path.join(path, "config.json")))
        cfg["n_layers"] = 13
        json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    else:
        path = _model_dir(tmp_path, **over)
    with pytest.raises(NotImplementedError, match=field):
        tmr.DistilbertActorAgnosticEncoder(path, num_layers=4, text_on_hip=True)
    if field != "n_layers":
        assert tmr.DistilbertActorAgnosticEncoder(path, num_layers=4).text_on_hip is False     # the PyTorch path still takes it


def test_sinusoidal_position_table_is_supported(tmp_path):
    m = tmr.DistilbertActorAgnosticEncoder(_model_dir(tmp_path, sinusoidal_pos_embds=True), num_layers=4, text_on_hip=True)
    assert m.text_on_hip and m.text_model.embeddings.position_embeddings.weight.shape == (512, 768)


def test_build_encoders_passes_the_flag_through(text_dir):
    from types import SimpleNamespace
    _, t = tmr.build_encoders(SimpleNamespace(tmr_base_path="", tmr_text_model_path=text_dir, tmr_text_on_hip=True), device="cpu")
    assert t.text_on_hip is True
    _, t = tmr.build_encoders(SimpleNamespace(tmr_base_path="", tmr_text_model_path=text_dir), device="cpu")
    assert t.text_on_hip is False


def test_workspace_formula_and_structs_follow_the_header():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    per_row = int(re.search(r"workspace: n_seq max_len x (\d+) bytes", header).group(1))
    assert per_row == 4 * (2304 + 768 + 3072)
    assert tmr.bert_workspace_bytes(3, 10) == 3 * 10 * per_row and tmr.bert_workspace_bytes(200, 254) == 200 * 254 * per_row
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include "syn_hip.h"\nint main(void){printf("%zu %zu %d %d %d %d %d %d\\n", sizeof(syn_bert_layer), '
                             'sizeof(syn_bert_model), SYN_BERT_D, SYN_BERT_HEADS, SYN_BERT_FF, SYN_BERT_MAX_LAYERS, SYN_TMR_MAX_SEQ, SYN_ABI_VERSION);return 0;}\n')
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", os.path.join(td, "sz")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SynBertLayer), ctypes.sizeof(_lib.SynBertModel), _lib.SYN_BERT_D, _lib.SYN_BERT_HEADS, _lib.SYN_BERT_FF,
                   _lib.SYN_BERT_MAX_LAYERS, _lib.SYN_TMR_MAX_SEQ, 9]
    assert got[0] == 12 * 8 and got[1] == 16 + 4 * 8 + 12 * 12 * 8
    assert (tmr.BERT_D, tmr.BERT_HEADS, tmr.BERT_FF, tmr.BERT_MAX_LAYERS) == (768, 12, 3072, 12)


def test_entry_point_is_bound_and_refuses_bad_arguments_before_any_launch():
    assert "syn_bert_encode" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.syn_bert_encode.argtypes is not None and len(lib.syn_bert_encode.argtypes) == 8
    fake = 256                                                     # non-NULL, 16-byte aligned stand-ins: every refusal happens before any launch
    m = _lib.SynBertModel()
    m.n_layers, m.vocab, m.n_pos, m.word, m.pos, m.emb_ln_g, m.emb_ln_b = 2, 40, 512, fake, fake, fake, fake
    for i in range(2):
        m.layer[i] = _lib.SynBertLayer(*([fake] * 12))
    args = lambda n_seq, max_len: (ctypes.byref(m), fake, n_seq, max_len, None, fake, fake, None)
    assert lib.syn_bert_encode(*args(1, _lib.SYN_TMR_MAX_LEN + 1)) != 0 and b"max_len" in lib.syn_last_error()
    assert lib.syn_bert_encode(*args(0, 16)) != 0 and b"n_seq" in lib.syn_last_error()
    assert lib.syn_bert_encode(*args(_lib.SYN_TMR_MAX_SEQ + 1, 16)) != 0 and b"n_seq" in lib.syn_last_error()
    for n in (0, 13):
        m.n_layers = n
        assert lib.syn_bert_encode(*args(1, 16)) != 0 and b"n_layers" in lib.syn_last_error()
    m.n_layers, m.n_pos = 2, 8
    assert lib.syn_bert_encode(*args(1, 16)) != 0 and b"n_pos" in lib.syn_last_error()
    m.n_pos = 512
    m.layer[1].w_fc2 = None
    assert lib.syn_bert_encode(*args(1, 16)) != 0 and b"layer" in lib.syn_last_error()
    m.layer[1].w_fc2 = fake
    assert lib.syn_bert_encode(ctypes.byref(m), fake, 1, 16, None, fake + 4, fake, None) != 0 and b"aligned" in lib.syn_last_error()
    assert lib.syn_bert_encode(ctypes.byref(m), None, 1, 16, None, fake, fake, None) != 0 and b"null" in lib.syn_last_error()


def test_out_of_range_ids_are_refused_on_the_host(on, monkeypatch):
    vocab = on.text_model.embeddings.word_embeddings.weight.shape[0]
    for bad in (vocab, -1):
        monkeypatch.setattr(on, "_tokenize_host", lambda texts, bad=bad: (torch.tensor([[2, bad, 3]]), torch.ones(1, 3, dtype=torch.int64)))
        with pytest.raises(ValueError, match="token id"):
            on.encode("x")


def test_emulation_restatement_agrees_with_transformers(on, fx):
    """scripts/distilbert_precision_emulation.py's `restate` at fp32 operands is DistilBertModel.forward: rel-L2 per prompt <= 1e-5 on the 2-layer
    fixture (measured at or below 1e-6), against transformers' module and against the golden's hidden rows."""
    spec = importlib.util.spec_from_file_location("distilbert_precision_emulation", os.path.join(REPO, "scripts", "distilbert_precision_emulation.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    sd = {k: v.detach() for k, v in on.text_model.state_dict().items()}
    for name in ("text3", "text1", "ragged"):
        ids = torch.from_numpy(fx[f"l2_{name}_ids"]).long()
        lengths = [int(v) for v in fx[f"l2_{name}_lengths"]]
        mask = (torch.arange(ids.shape[1])[None] < torch.tensor(lengths)[:, None]).long()
        with torch.no_grad():
            want = on.text_model(input_ids=ids, attention_mask=mask).last_hidden_state
            got = emu.restate(sd, ids, mask, 2, 2, 2, 2)
        errs = [rel_l2(got[b, :n], want[b, :n]) for b, n in enumerate(lengths)]
        print(f"{name}: restatement vs transformers, worst prompt rel-L2 {max(errs):.2e}")
        assert max(errs) <= 1e-5, (name, errs)
        if name != "ragged":
            gold = torch.from_numpy(fx[f"l2_{name}_hidden"])
            mine = torch.cat([got[b, :n] for b, n in enumerate(lengths)])
            assert rel_l2(mine, gold) <= 1e-5
