"""FGD evaluator (syntalker_amd/evaluator.py) without a GPU: the reference's topology, state_dict layout and checkpoint format, the torch
restatement against the reference's outputs (tests/golden/evaluator_outputs.npz, make_evaluator_golden.py), the refusals, the C structs'
ctypes mirrors and the drop-in import name."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, checkpoint, evaluator, synth
from tests import evaluator_ref
from tests.conftest import rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PARENTS = json.load(open(os.path.join(HERE, "golden", "smplx_kintree.json")))["parents"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "evaluator_outputs.npz"))


def _args(tmp, parents=PARENTS, **over):
    synth.synth_smplx_model(str(tmp), parents)
    a = dict(data_path_1=str(tmp) + "/", vae_layer=4, vae_grow=[1, 1, 2, 1], vae_length=240, vae_test_dim=330, variational=False)
    a.update(over)
    return SimpleNamespace(**a)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    m = evaluator.VAESKConv(_args(tmp_path_factory.mktemp("smplx")))
    m.load_state_dict(synth.synth_evaluator_state_dict(m))
    return m


def test_topology_of_every_layer_is_the_references(fx, model):
    topo = json.loads(str(fx["topology"]))
    assert len(topo) == len(model.plan) == 4
    for want, got in zip(topo, model.plan):
        assert [list(e) for e in got["edges"]] == want["edges"]
        assert got["neighbours"] == want["neighbours"]
        assert (got["pooling"] is not None) == want["pooled"]
        if want["pooled"]:
            assert got["pooling"] == want["pooling"]
        assert (got["cin"], got["cout"]) == (want["cin"], want["cout"])
    assert [(p["cin"], p["cout"], p["out_width"]) for p in model.plan] == [(330, 330, 210), (210, 210, 120), (120, 240, 240), (240, 240, 240)]


def test_state_dict_keys_and_shapes_are_the_references(fx, model):
    sd = model.state_dict()
    assert list(sd.keys()) == list(fx["keys"]) and len(sd) == 56
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(fx["shapes"])
    assert sum(v.numel() for v in sd.values()) > 4e6


def test_reference_format_checkpoint_with_module_prefixes_loads(model, tmp_path):
    m = evaluator.VAESKConv(_args(tmp_path / "tree"))
    path = str(tmp_path / "AESKConv_240_100.bin")
    torch.save({"model_state": {"module." + k: v.clone() for k, v in model.state_dict().items()}}, path)
    checkpoint.load_checkpoints(m, path)
    for k, v in model.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    torch.save({"model_state": {k: v for k, v in model.state_dict().items() if not k.startswith("decoder.")}}, path)
    with pytest.raises(KeyError):
        checkpoint.load_checkpoints(m, path)                   # a strict load: the decoder's tensors are required too


def test_build_evaluator_loads_data_path_plus_e_path_or_names_it(model, tmp_path):
    from syntalker_amd import config
    args = _args(tmp_path / "tree", data_path=str(tmp_path) + "/", e_path="weights/AESKConv_240_100.bin")
    with pytest.raises(FileNotFoundError, match="AESKConv_240_100.bin"):
        config.build_evaluator(args, device="cpu")
    os.makedirs(tmp_path / "weights")
    torch.save({"model_state": model.state_dict()}, str(tmp_path / "weights" / "AESKConv_240_100.bin"))
    m = config.build_evaluator(args, device="cpu")
    assert torch.equal(m.encoder.layers[2][0].shortcut.weight, model.encoder.layers[2][0].shortcut.weight)


def test_torch_restatement_reproduces_the_reference(fx, model):
    sd = model.state_dict()
    for b, n, seed in synth.EVALUATOR_CASES:
        got = evaluator_ref.encode(sd, synth.synth_evaluator_input(b, n, seed))
        want = torch.from_numpy(fx[f"out_{b}x{n}"])
        assert got.shape == (b, n // 16, 240)
        assert rel_l2(got, want) <= 1e-6, (b, n)


def test_refusals(model, tmp_path):
    with pytest.raises(_lib.SynHipError):
        model.map2latent(torch.zeros(1, 32, 330))              # no CPU fallback
    with pytest.raises(NotImplementedError):
        model.train(True)
    with pytest.raises(NotImplementedError):
        model.train()
    model.eval()
    with pytest.raises(NotImplementedError, match="motion_representation.py"):
        model.decode(torch.zeros(1, 2, 240))
    var = evaluator.VAESKConv(_args(tmp_path / "v", variational=True))
    with pytest.raises(NotImplementedError, match="randn_like"):
        var.map2latent(torch.zeros(1, 32, 330))
    with pytest.raises(ValueError, match="ends at"):
        evaluator.VAESKConv(_args(tmp_path / "w", vae_grow=[1, 1, 1, 1]))
    with pytest.raises(ValueError, match="ends at"):
        evaluator.VAESKConv(_args(tmp_path / "p", parents=[-1] + [0] * 54))     # 55 joints on the root: nothing pools, 660 channels


def test_group_norm_width_must_divide_by_ten():
    edges = evaluator.build_edge_topology([-1, 0, 1])         # 3 edges: 18 channels, GroupNorm(10, 18) does not exist
    assert edges == [(0, 3), (0, 1), (1, 2)]
    with pytest.raises(ValueError, match="divisible by 10"):
        evaluator.layer_plan([-1, 0, 1], [1, 1, 1, 1], 18)


def test_c_structs_match_their_ctypes_mirrors():
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include "syn_hip.h"\nint main(void){printf("%zu %zu %d %d %d\\n", sizeof(syn_skel_layer), '
                             'sizeof(syn_skel_model), SYN_SKEL_LAYERS, SYN_SKEL_MAX_C, SYN_SKEL_POOL_MAX);return 0;}\n')
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", os.path.join(td, "sz")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SynSkelLayer), ctypes.sizeof(_lib.SynSkelModel), _lib.SYN_SKEL_LAYERS, _lib.SYN_SKEL_MAX_C,
                   _lib.SYN_SKEL_POOL_MAX]


def test_workspace_size_formula():
    # layer i: r | s fp32 [B][n >> (i+1)][2 roundup(cout, 16)], partial sums fp64 [B][tiles][10][2], each rounded up to 256 bytes
    b, n = 3, 48
    want = 0
    for i, cout in enumerate((330, 210, 240, 240)):
        t = n >> (i + 1)
        want += -(-b * t * 2 * (-(-cout // 16) * 16) * 4 // 256) * 256 + -(-b * -(-t // 16) * 160 // 256) * 256
    assert evaluator.workspace_bytes([330, 210, 240, 240], b, n) == want


def test_dropin_installs_the_evaluator_only_on_request():
    import importlib
    from syntalker_amd import dropin
    saved = sys.modules.pop("models.motion_representation", None)
    try:
        dropin.install()
        assert "models.motion_representation" not in sys.modules
        dropin.install(evaluator=True)
        assert getattr(importlib.import_module("models.motion_representation"), "VAESKConv") is evaluator.VAESKConv
    finally:
        sys.modules.pop("models.motion_representation", None)
        if saved is not None:
            sys.modules["models.motion_representation"] = saved
