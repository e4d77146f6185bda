"""TMR encoders (syntalker_amd/tmr.py) without a GPU: the reference's state_dict layout, strict loading, the frozen-module contract,
the drop-in import names and the C structs' ctypes mirrors."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, synth, tmr

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "tmr_outputs.npz"))


def _keys_shapes(sd):
    return list(sd.keys()), [",".join(map(str, v.shape)) for v in sd.values()]


def test_motion_encoder_state_dict_is_the_references(fixture):
    m = tmr.ActorAgnosticEncoder(nfeats=623, vae=True, num_layers=4)
    keys, shapes = _keys_shapes(m.state_dict())
    assert keys == list(fixture["motion_keys"]) and shapes == list(fixture["motion_shapes"])
    assert m.state_dict()["sequence_pos_encoding.pe"].shape == (5000, 1, 256)
    ref = {k: torch.randn([int(v) for v in s.split(",")]) for k, s in zip(fixture["motion_keys"], fixture["motion_shapes"])}
    m.load_state_dict(ref, strict=True)                        # a reference-keyed checkpoint loads strictly
    assert torch.equal(m.seqTransEncoder.layers[3].self_attn.in_proj_weight, ref["seqTransEncoder.layers.3.self_attn.in_proj_weight"])


def test_positional_table_is_the_sinusoid():
    pe = tmr.PositionalEncoding(256).pe[:, 0]
    s, i = 37, 5
    w = 10000.0 ** (-2 * i / 256)
    assert abs(pe[s, 2 * i] - np.sin(s * w)) < 1e-5 and abs(pe[s, 2 * i + 1] - np.cos(s * w)) < 1e-5


def test_frozen_inference_module_and_reference_configuration_only():
    m = tmr.ActorAgnosticEncoder(nfeats=623)
    assert not m.training and not m.seqTransEncoder.layers[0].training
    with pytest.raises(NotImplementedError):
        m.train(True)
    with pytest.raises(NotImplementedError):
        m.train()
    m.eval()                                                   # eval() stays allowed
    for bad in (dict(vae=False), dict(num_layers=2), dict(latent_dim=512), dict(activation="relu"), dict(num_heads=8), dict(ff_size=2048)):
        with pytest.raises(NotImplementedError, match="h3d_diffusion_new_trainer.py"):
            tmr.ActorAgnosticEncoder(nfeats=623, **bad)


def test_no_cpu_fallback():
    m = tmr.ActorAgnosticEncoder(nfeats=623)
    with pytest.raises(_lib.SynHipError):
        m.encode(torch.zeros(1, 4, 623))


def test_dropin_import_names():
    import importlib
    a = importlib.import_module("syntalker_amd.dropin.models.temos.motionencoder.actor")
    assert a.ActorAgnosticEncoder is tmr.ActorAgnosticEncoder
    t = importlib.import_module("syntalker_amd.dropin.models.temos.textencoder.distillbert_actor")
    assert t.DistilbertActorAgnosticEncoder is tmr.DistilbertActorAgnosticEncoder


def test_build_encoders_paths(tmp_path):
    from types import SimpleNamespace
    with pytest.raises(FileNotFoundError):
        tmr.build_encoders(SimpleNamespace(tmr_base_path=str(tmp_path / "absent")), device="cpu", text=False)
    m, t = tmr.build_encoders(SimpleNamespace(tmr_base_path=""), device="cpu", text=False)
    assert isinstance(m, tmr.ActorAgnosticEncoder) and t is None
    sd = synth.synth_tmr_state_dict(m)
    torch.save(sd, tmp_path / "motion_epoch=299.ckpt")
    m, _ = tmr.build_encoders(SimpleNamespace(tmr_base_path=str(tmp_path)), device="cpu", text=False)
    assert torch.equal(m.mu_token, sd["mu_token"])


def test_synth_recipe_layernorms_are_not_identity():
    sd = synth.synth_tmr_state_dict(tmr.ActorAgnosticEncoder(nfeats=623))
    for k, v in sd.items():
        if ".norm" in k:
            assert (v != (1.0 if k.endswith("weight") else 0.0)).all(), k
    assert torch.equal(sd["sequence_pos_encoding.pe"], tmr.PositionalEncoding(256).pe)


def test_text_encoder_state_dict_is_the_references(fixture, tmp_path):
    pytest.importorskip("transformers")
    synth.synth_tmr_text_model(str(tmp_path))
    m = tmr.DistilbertActorAgnosticEncoder(str(tmp_path), num_layers=4)
    keys, shapes = _keys_shapes(m.state_dict())
    assert keys == list(fixture["text_keys"]) and shapes == list(fixture["text_shapes"])
    m.load_state_dict(synth.synth_tmr_state_dict(m), strict=True)
    ids, mask = m.tokenize(synth.TMR_PROMPTS)
    assert np.array_equal(ids.numpy(), fixture["text3_ids"]) and np.array_equal(mask.numpy(), fixture["text3_mask"])
    ids, mask = m.tokenize(synth.TMR_PROMPT_ONE)              # a bare str is a batch of one, as the reference's tokenizer call makes it
    assert np.array_equal(ids.numpy(), fixture["text1_ids"]) and np.array_equal(mask.numpy(), fixture["text1_mask"])
    with pytest.raises(NotImplementedError):
        m.train(True)


def test_c_abi_tmr_struct_sizes_match_the_ctypes_mirrors():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include "syn_hip.h"\nint main(void){printf("%zu %zu %d %d\\n", sizeof(syn_tmr_layer), '
                             'sizeof(syn_tmr_model), SYN_TMR_MAX_LEN, SYN_TMR_MAX_FEATS);return 0;}\n')
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", os.path.join(td, "sz")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SynTmrLayer), ctypes.sizeof(_lib.SynTmrModel), _lib.SYN_TMR_MAX_LEN, _lib.SYN_TMR_MAX_FEATS]
    assert got[0] == 12 * 8 and got[1] == 8 + 5 * 8 + 4 * 12 * 8


def test_workspace_bytes_follow_the_header():
    assert tmr.workspace_bytes(3, 10) == 3 * 12 * 7680


def test_c_abi_tmr_entry_points_refuse_out_of_range_sizes():
    """The C side's own bounds (no launch is reached): nfeats of the model, max_len, n_seq, and the packer's columns."""
    lib = _lib.load()
    m = _lib.SynTmrModel()
    fake = 256                                                  # non-NULL stand-ins: every refusal happens before any launch
    m.nfeats, m.w_in, m.b_in, m.mu_token, m.logvar_token, m.pe = _lib.SYN_TMR_MAX_FEATS + 1, fake, fake, fake, fake, fake
    for i in range(_lib.SYN_TMR_LAYERS):
        m.layer[i] = _lib.SynTmrLayer(*([fake] * 12))
    args = lambda n_seq, max_len: (ctypes.byref(m), fake, n_seq, max_len, None, fake, fake, fake, None)
    assert lib.syn_tmr_encode(*args(1, 16)) != 0 and b"nfeats" in lib.syn_last_error()
    m.nfeats = 623
    assert lib.syn_tmr_encode(*args(1, _lib.SYN_TMR_MAX_LEN + 1)) != 0 and b"max_len" in lib.syn_last_error()
    assert lib.syn_tmr_encode(*args(0, 16)) != 0 and b"n_seq" in lib.syn_last_error()
    m.layer[2].w_fc1 = None
    assert lib.syn_tmr_encode(*args(1, 16)) != 0 and b"layer" in lib.syn_last_error()
    assert lib.syn_tmr_pack_weight(fake, 256, _lib.SYN_TMR_MAX_FEATS + 1, fake, None) != 0
    assert lib.syn_tmr_pack_weight(fake, 24, 256, fake, None) != 0          # rows not a multiple of 16


def test_text_checkpoint_with_a_persistent_position_ids_buffer_loads_strictly(tmp_path):
    pytest.importorskip("transformers")
    synth.synth_tmr_text_model(str(tmp_path))
    m = tmr.DistilbertActorAgnosticEncoder(str(tmp_path), num_layers=4)
    sd = synth.synth_tmr_state_dict(m)
    assert "text_model.embeddings.position_ids" not in sd
    sd["text_model.embeddings.position_ids"] = torch.arange(512)[None]      # what older transformers releases saved
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.mu_token, sd["mu_token"])
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)       # any other unexpected key still fails
