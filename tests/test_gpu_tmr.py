"""TMR encoders on the HIP stack kernel vs the reference's outputs (tests/golden/tmr_outputs.npz, make_tmr_golden.py): rel-L2 per clip
<= 5e-3 for loc, <= 1e-2 for scale; batch invariance, determinism, graph capture, limits, prompts through the body-part sampler and
the h3d trainer script on motion features."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, synth, tmr
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DEV = "cuda"
LOC_TOL, SCALE_TOL = 5e-3, 1e-2


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "tmr_outputs.npz"))


@pytest.fixture(scope="module")
def motion():
    m = tmr.ActorAgnosticEncoder(nfeats=623, vae=True, num_layers=4)
    m.load_state_dict(synth.synth_tmr_state_dict(m))
    return m.to(DEV)


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    pytest.importorskip("transformers")
    path = synth.synth_tmr_text_model(str(tmp_path_factory.mktemp("distilbert")))
    m = tmr.DistilbertActorAgnosticEncoder(path, num_layers=4)
    m.load_state_dict(synth.synth_tmr_state_dict(m))
    return m.to(DEV)


def _per_clip(got, want, tol, what):
    errs = [rel_l2(g, w) for g, w in zip(got.cpu(), torch.as_tensor(want))]
    print(f"{what}: worst rel-L2 {max(errs):.3e}")
    assert max(errs) <= tol, (what, max(errs), int(np.argmax(errs)))


def test_motion_b8_padded_vs_reference(motion, fx):
    x = synth.synth_tmr_motion(8, 128).to(DEV)
    d = motion(x, [int(v) for v in fx["motion8_lengths"]])
    _per_clip(d.loc, fx["motion8_loc"], LOC_TOL, "motion B=8 loc")
    _per_clip(d.scale, fx["motion8_scale"], SCALE_TOL, "motion B=8 scale")
    d2 = motion(x, torch.as_tensor(fx["motion8_lengths"]).to(DEV))     # device lengths: the same call
    assert torch.equal(d.loc, d2.loc)


def test_motion_b200_vs_reference(motion, fx):
    d = motion(synth.synth_tmr_motion(200, 128, seed=34).to(DEV))
    _per_clip(d.loc, fx["motion200_loc"], LOC_TOL, "motion B=200 loc")
    _per_clip(d.scale, fx["motion200_scale"], SCALE_TOL, "motion B=200 scale")


def test_text_vs_reference(text, fx):
    for name, prompts in (("text3", synth.TMR_PROMPTS), ("text1", synth.TMR_PROMPT_ONE)):
        d = text(prompts)
        assert d.loc.shape == (fx[name + "_loc"].shape[0], 256)
        _per_clip(d.loc, fx[name + "_loc"], LOC_TOL, name + " loc")
        _per_clip(d.scale, fx[name + "_scale"], SCALE_TOL, name + " scale")


def test_clip_alone_equals_clip_in_batch_and_calls_repeat(motion):
    x = synth.synth_tmr_motion(8, 128).to(DEV)
    lengths = torch.tensor([128, 97, 64, 33, 1, 128, 128, 2], device=DEV)
    mu, lv = motion.encode(x, lengths)
    mu2, lv2 = motion.encode(x, lengths)
    assert torch.equal(mu, mu2) and torch.equal(lv, lv2)
    for i in (0, 3, 7):
        a, b = motion.encode(x[i:i + 1], lengths[i:i + 1])
        assert torch.equal(a[0], mu[i]) and torch.equal(b[0], lv[i]), i


def test_encode_in_a_cuda_graph(motion):
    x = synth.synth_tmr_motion(4, 40).to(DEV)
    lengths = torch.tensor([40, 17, 3, 40], device=DEV)
    want = motion.encode(x, lengths)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        motion.encode(x, lengths)                              # warm: packed weights and the workspace exist before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = motion.encode(x, lengths)
    x.copy_(synth.synth_tmr_motion(4, 40, seed=5).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    fresh = motion.encode(x, lengths)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    x.copy_(synth.synth_tmr_motion(4, 40).to(DEV))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_unsupported_shapes_raise(motion):
    with pytest.raises(ValueError):
        motion.encode(torch.zeros(1, tmr.MAX_LEN + 1, 623, device=DEV))
    with pytest.raises(ValueError):
        motion.encode(torch.zeros(2, 16, 600, device=DEV))
    m = motion.packed()["model"]
    lib = _lib.load()
    ws = torch.empty(tmr.workspace_bytes(1, 300), dtype=torch.uint8, device=DEV)
    out = torch.empty(2, 256, device=DEV)
    x = torch.zeros(1, 300, 623, device=DEV)
    assert lib.syn_tmr_encode(m, x.data_ptr(), 1, 255, None, ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None) != 0
    assert b"max_len" in lib.syn_last_error()
    full = motion.encode(torch.zeros(1, tmr.MAX_LEN, 623, device=DEV))      # the largest supported length runs
    assert torch.isfinite(full[0]).all()


def test_prompt_vectors_through_the_bodypart_sampler(text, fx):
    """One h3d clip, DDIM-50 under TwoClassifierFreeSampleModel_Bodypart, with the HIP prompt vectors and with the reference's."""
    from syntalker_amd import guidance as G
    from syntalker_amd.process import create_gaussian_diffusion
    from tests.test_gpu_parity import _model
    h3d = _model("h3d")
    y = synth.to_device(synth.synth_clip_inputs(1, seed=8, style_dim=256, style_zero=False), DEV)
    x = synth.synth_latent(1, seed=8).to(DEV)
    loc = text(synth.TMR_PROMPTS).loc
    ref = torch.as_tensor(fx["text3_loc"]).to(DEV)
    out = []
    for v in (loc, ref):
        parts = {"upper_mask": v[0:1], "hands_mask": v[1:2], "lower_mask": v[2:3]}
        with torch.no_grad():
            w = G.TwoClassifierFreeSampleModel_Bodypart(h3d)
            out.append(create_gaussian_diffusion(use_ddim=True).ddim_sample_loop(
                w, (1, 1536, 1, 32), noise=x.clone(), clip_denoised=False, model_kwargs={"y": dict(y, style_feature=parts)},
                step_noise=synth.synth_step_noise(50, 1, seed=9)).cpu())
    e = rel_l2(out[0], out[1])
    print(f"DDIM-50 body-part guidance, HIP vs reference prompt vectors: rel-L2 {e:.3e}")
    assert e < 3e-2, e


def test_train_from_config_on_motion_features(tmp_path):
    """scripts/train_from_config.py on the h3d configuration with a --data file carrying tmr_tar_pose (and no style_feature): the batch's
    style_feature comes from the HIP motion encoder; two steps with finite losses, eager and captured (--graph)."""
    import json
    import yaml
    cfg = json.load(open(os.path.join(HERE, "golden", "reference_configs.json")))["diffusion_h3d.yaml"]
    (tmp_path / "h3d.yaml").write_text(yaml.safe_dump(cfg))
    n = 4
    g = torch.Generator().manual_seed(41)
    np.savez(tmp_path / "h3d.npz", latent=torch.randn(n, 1536, 1, 32, generator=g).numpy(), audio=torch.randn(n, 68266, 2, generator=g).numpy(),
             word=torch.randint(0, synth.VOCAB, (n, 128), generator=g).numpy(), seed=torch.randn(n, 4, 1536, generator=g).numpy(),
             tmr_tar_pose=synth.synth_tmr_motion(n, 128, seed=40).numpy())
    for extra in ([], ["--graph"]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_from_config.py"), str(tmp_path / "h3d.yaml"),
                            "--data", str(tmp_path / "h3d.npz"), "--epochs", "1", "--batch-size", "2", "--out", str(tmp_path / "out")] + extra,
                           capture_output=True, text=True, timeout=900, cwd=REPO)
        print(r.stdout[-2000:], r.stderr[-2000:])
        assert r.returncode == 0, extra
        assert "TMR motion encoder on tmr_tar_pose" in r.stdout
        logs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"epoch"')]
        assert logs and logs[0]["steps"] == 2 and np.isfinite(logs[0]["loss"]), logs


def test_packed_weights_follow_parameter_writes(motion):
    """packed() keys on the parameters' version counters: an in-place write re-packs, and the result equals a fresh module's."""
    m = tmr.ActorAgnosticEncoder(nfeats=623)
    m.load_state_dict(synth.synth_tmr_state_dict(m))
    m = m.to(DEV)
    x = synth.synth_tmr_motion(3, 50).to(DEV)
    before = m.encode(x)[0].clone()
    with torch.no_grad():
        m.seqTransEncoder.layers[2].linear1.weight.mul_(1.5)
        m.mu_token.add_(0.25)
    after = m.encode(x)[0]
    assert not torch.equal(before, after)
    fresh = tmr.ActorAgnosticEncoder(nfeats=623)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    assert torch.equal(fresh.to(DEV).encode(x)[0], after)


def test_used_encoder_deep_copies_and_pickles(motion):
    """An encoder that has run holds a ctypes struct of raw pointers into its own packed tensors: copy.deepcopy and torch.save / torch.load take the
    module without its `_syn_*` caches (`engine.drop_caches`), and each copy packs its own and encodes bit-equal to the original."""
    import copy
    import io
    x = synth.synth_tmr_motion(3, 50).to(DEV)
    mu, lv = motion.encode(x)
    assert "_syn_packed" in motion.__dict__
    buf = io.BytesIO()
    torch.save(motion, buf)
    buf.seek(0)
    for m2 in (copy.deepcopy(motion), torch.load(buf, weights_only=False)):
        assert not any(k.startswith("_syn_") for k in m2.__dict__)
        mu2, lv2 = m2.encode(x)
        assert torch.equal(mu2, mu) and torch.equal(lv2, lv)


def _h3d_yaml(tmp_path, **extra):
    import json
    import yaml
    cfg = json.load(open(os.path.join(HERE, "golden", "reference_configs.json")))["diffusion_h3d.yaml"]
    path = tmp_path / "h3d_extra.yaml"
    path.write_text(yaml.safe_dump(dict(cfg, **extra)))
    return path


def test_train_from_config_replaces_rows_with_prompt_vectors(tmp_path):
    """text_sample_stride > 0 with prompt_text / tar_id in the file (h3d_diffusion_new_trainer.py:371-374): the text encoder is built from
    tmr_text_model_path and its rows replace every stride-th motion row with tar_id == 99."""
    pytest.importorskip("transformers")
    import json
    text_dir = synth.synth_tmr_text_model(str(tmp_path / "distilbert"))
    cfg = _h3d_yaml(tmp_path, text_sample_stride=1, tmr_text_model_path=text_dir)
    n = 4
    g = torch.Generator().manual_seed(42)
    np.savez(tmp_path / "h3d_text.npz", latent=torch.randn(n, 1536, 1, 32, generator=g).numpy(), audio=torch.randn(n, 68266, 2, generator=g).numpy(),
             word=torch.randint(0, synth.VOCAB, (n, 128), generator=g).numpy(), seed=torch.randn(n, 4, 1536, generator=g).numpy(),
             tmr_tar_pose=synth.synth_tmr_motion(n, 128, seed=43).numpy(), tar_id=np.array([99, 3, 99, 99]),
             prompt_text=np.array(synth.TMR_PROMPTS + [synth.TMR_PROMPT_ONE]))
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train_from_config.py"), str(cfg), "--data", str(tmp_path / "h3d_text.npz"),
                        "--epochs", "1", "--batch-size", "2", "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=900, cwd=REPO)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "text encoder on prompt_text" in r.stdout
    logs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"epoch"')]
    assert logs and logs[0]["steps"] == 2 and np.isfinite(logs[0]["loss"]), logs


def test_tmr_style_rows(tmp_path):
    """TmrStyle itself: rows with tar_id == 99 at the stride take the text encoder's loc, the others keep the motion encoder's."""
    pytest.importorskip("transformers")
    from types import SimpleNamespace
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    from train_from_config import TmrStyle
    text_dir = synth.synth_tmr_text_model(str(tmp_path / "distilbert"))
    prompts = np.array(synth.TMR_PROMPTS + [synth.TMR_PROMPT_ONE])
    z = {"tmr_tar_pose": synth.synth_tmr_motion(4, 64, seed=44).numpy(), "tar_id": np.array([99, 3, 99, 99]), "prompt_text": prompts}
    st = TmrStyle(SimpleNamespace(text_sample_stride=2, tmr_text_model_path=text_dir, tmr_base_path=""), DEV, z)
    ix = np.arange(4)
    got = st(z, ix, DEV)
    motion = st.motion(torch.from_numpy(z["tmr_tar_pose"]).to(DEV)).loc
    text = st.text(list(prompts)).loc
    # tar_id == 99 at rows 0, 2, 3; every 2nd of them: rows 0 and 3
    for i, want in ((0, text), (1, motion), (2, motion), (3, text)):
        assert torch.equal(got[i], want[i]), i


def test_sample_from_config_with_body_part_prompts(tmp_path):
    """scripts/sample_from_config.py on the h3d configuration: --upper-prompt / --lower-prompt through the HIP text encoder into
    TwoClassifierFreeSampleModel_Bodypart; finite, and not the no-prompt result."""
    pytest.importorskip("transformers")
    import importlib.util
    spec = importlib.util.spec_from_file_location("sample_from_config", os.path.join(REPO, "scripts", "sample_from_config.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    text_dir = synth.synth_tmr_text_model(str(tmp_path / "distilbert"))
    cfg = _h3d_yaml(tmp_path, tmr_text_model_path=text_dir, tmr_base_path="./ckpt/absent_tmr", pose_fps=30, pre_frames=4)
    common = [str(cfg), "--random-init", "--ddim", "--seconds", "4.3", "--seed", "3"]
    plain = drv.main(common + ["--out", str(tmp_path / "plain.npz")])
    guided = drv.main(common + ["--upper-prompt", synth.TMR_PROMPTS[0], "--lower-prompt", synth.TMR_PROMPTS[1], "--out", str(tmp_path / "guided.npz")])
    assert plain["finite"] and guided["finite"] and guided["windows"] == plain["windows"] == 1
    assert guided["prompts"] == {"upper": synth.TMR_PROMPTS[0], "lower": synth.TMR_PROMPTS[1]} and plain["prompts"] == {}
    a, b = plain["_latents"].float(), guided["_latents"].float()
    assert torch.isfinite(b).all() and a.shape == b.shape
    e = rel_l2(b.cpu(), a.cpu())
    print(f"prompted vs unprompted latents: rel-L2 {e:.3e}")
    assert e > 1e-2
    with pytest.raises(FileNotFoundError):          # without --random-init the configured TMR checkpoint directory must exist
        drv.main([str(cfg), "--ddim", "--seconds", "4.3", "--upper-prompt", "a man jumps"])
