"""FGD evaluator on the HIP kernels (syn_skel_encode) vs the reference's outputs (tests/golden/evaluator_outputs.npz) and the torch fp32
restatement (tests/evaluator_ref.py): rel-L2 <= 1e-5 and max |diff| <= 1e-5; batch invariance and determinism (bitwise), the masks, the
pack cache, graph capture, copies, metrics.fgd against the reference's FGD and scripts/fgd_from_results.py."""
import copy
import io
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from syntalker_amd import evaluator, metrics, synth
from tests import evaluator_ref
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = "cuda"
PARENTS = json.load(open(os.path.join(HERE, "golden", "smplx_kintree.json")))["parents"]
ARGS = dict(vae_layer=4, vae_grow=[1, 1, 2, 1], vae_length=240, vae_test_dim=330, vae_test_len=32, variational=False)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "evaluator_outputs.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    d = tmp_path_factory.mktemp("hub")
    synth.synth_smplx_model(str(d), PARENTS)
    return str(d) + "/"


def _model(tree):
    m = evaluator.VAESKConv(SimpleNamespace(data_path_1=tree, **ARGS))
    m.load_state_dict(synth.synth_evaluator_state_dict(m))
    return m.to(DEV)


@pytest.fixture(scope="module")
def model(tree):
    return _model(tree)


def _close(got, want):
    assert got.shape == want.shape
    assert rel_l2(got, want) <= 1e-5 and float((got.double() - want.double()).abs().max()) <= 1e-5, (rel_l2(got, want),
                                                                                                  float((got - want).abs().max()))


def test_matches_the_reference_golden(fx, model):
    for b, n, seed in synth.EVALUATOR_CASES:
        got = model.map2latent(synth.synth_evaluator_input(b, n, seed).to(DEV)).cpu()
        _close(got, torch.from_numpy(fx[f"out_{b}x{n}"]))
        assert float(got.abs().max()) <= 1.0


def test_matches_the_restatement_at_other_shapes(model):
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    for b in (1, 3):
        for n in (16, 48, 1792, 8992):
            x = synth.synth_evaluator_input(b, n, seed=n + b).to(DEV)
            _close(model.map2latent(x), evaluator_ref.encode(sd, x))


def test_batch_equals_per_take_calls_and_calls_repeat_bitwise(model):
    x = synth.synth_evaluator_input(5, 96, seed=7).to(DEV)
    y = model.map2latent(x)
    assert torch.equal(model.map2latent(x), y)
    for i in range(5):
        assert torch.equal(model.map2latent(x[i:i + 1]), y[i:i + 1]), i


def test_shape_refusals(model):
    for bad in ((1, 40, 330), (1, 8, 330), (1, 32, 331), (32, 330), (0, 32, 330)):
        with pytest.raises(ValueError):
            model.map2latent(torch.zeros(*bad, device=DEV))


def test_weights_outside_the_masks_do_not_matter(tree):
    m = _model(tree)
    x = synth.synth_evaluator_input(2, 128, seed=8).to(DEV)
    want = m.map2latent(x)
    with torch.no_grad():
        for blk in m.encoder.layers:
            for conv in (blk[0].residual[0], blk[0].shortcut):
                conv.weight.add_(torch.randn_like(conv.weight) * (conv.mask == 0))
    assert torch.equal(m.map2latent(x), want)


def test_loading_new_weights_repacks(tree):
    m = _model(tree)
    x = synth.synth_evaluator_input(1, 64, seed=9).to(DEV)
    before = m.map2latent(x)
    m.load_state_dict(synth.synth_evaluator_state_dict(m, seed=77))
    after = m.map2latent(x)
    assert not torch.equal(before, after)
    _close(after, evaluator_ref.encode({k: v.detach() for k, v in m.state_dict().items()}, x))


def test_map2latent_in_a_cuda_graph(model):
    x = synth.synth_evaluator_input(2, 160, seed=10).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.map2latent(x)                                    # warm: packed weights and the workspace exist before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = model.map2latent(x)
    x.copy_(synth.synth_evaluator_input(2, 160, seed=11).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, model.map2latent(x))


def test_used_evaluator_deep_copies_and_pickles(model):
    x = synth.synth_evaluator_input(2, 64, seed=12).to(DEV)
    y = model.map2latent(x)
    assert "_syn_packed" in model.__dict__
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    for m2 in (copy.deepcopy(model), torch.load(buf, weights_only=False)):
        assert not any(k.startswith("_syn_") for k in m2.__dict__)
        assert torch.equal(m2.map2latent(x), y)


def test_fgd_matches_the_reference_fgd(fx, model):
    sets = {name: synth.synth_evaluator_takes(lengths, seed, scale, shift) for name, (lengths, seed, scale, shift) in
            synth.EVALUATOR_FGD_TAKES.items()}
    got = metrics.fgd(model, sets["rec"], [t[None] for t in sets["tar"]], vae_test_len=32)
    want = float(fx["fgd"])
    assert abs(got - want) <= 1e-4 * abs(want), (got, want)


def _results_dir(path):
    """Three res / gt pairs of different lengths and one gt file without a partner, as the reference's test() writes them."""
    os.makedirs(path)
    g = torch.Generator().manual_seed(13)
    takes = {}
    for i, n in (("a", 200), ("b", 333), ("c", 96)):
        rec, tar = (0.4 * torch.randn(n, 165, generator=g)).numpy(), (0.4 * torch.randn(n, 165, generator=g)).numpy()
        np.savez(os.path.join(path, f"res_{i}.npz"), poses=rec, model="smplx2020")
        np.savez(os.path.join(path, f"gt_{i}.npz"), poses=tar, model="smplx2020")
        takes[i] = (rec, tar)
    np.savez(os.path.join(path, "gt_lonely.npz"), poses=np.zeros((64, 165), np.float32))
    return takes


def _fgd_of(m, takes):
    from syntalker_amd import poses
    to6 = lambda a: poses.axis_angle_to_rotation_6d(torch.from_numpy(a).to(DEV).reshape(a.shape[0], 55, 3)).reshape(a.shape[0], 330)
    ids = sorted(takes)
    return metrics.fgd(m, [to6(takes[i][0]) for i in ids], [to6(takes[i][1]) for i in ids])


def test_fgd_from_results_script(tmp_path, tree, model):
    import yaml
    import torch as _t
    takes = _results_dir(str(tmp_path / "results"))
    data = str(tmp_path / "data") + "/"
    cfg = dict(ARGS, data_path=data, data_path_1=tree, e_path="weights/AESKConv_240_100.bin")
    yml = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(yml, "w"))
    script = os.path.join(REPO, "scripts", "fgd_from_results.py")

    def run(*extra):
        r = subprocess.run([sys.executable, script, str(tmp_path / "results"), "-c", yml, *extra], capture_output=True, text=True, cwd=REPO,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "gt_lonely.npz" in r.stderr
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = run("--random-init")
    assert out["takes"] == 3 and out["frames"] == 200 + 333 + 96
    assert out["fgd"] == pytest.approx(_fgd_of(model, takes), rel=1e-9, abs=1e-9)
    other = _model(tree)
    other.load_state_dict(synth.synth_evaluator_state_dict(other, seed=5))
    os.makedirs(data + "weights")
    _t.save({"model_state": {"module." + k: v.cpu() for k, v in other.state_dict().items()}}, data + cfg["e_path"])
    out = run()
    assert out["fgd"] == pytest.approx(_fgd_of(other, takes), rel=1e-9, abs=1e-9)
