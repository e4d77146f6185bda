"""calc_bpd_loop, host side (no GPU): the generic torch path against the reference's recorded outputs (tests/golden/bpd_outputs.npz, written by
tests/golden/make_bpd_golden.py), `engine.bpd_rows` against the reference's fp64 tables, the chunk plan, the signatures and probes, and the
bookkeeping of the C entry point `syn_bpd_terms`."""
import ast
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from syntalker_amd import _lib, engine, process, synth

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
NOISE_SEED = 5
KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLD, "bpd_outputs.npz")))


@pytest.fixture(scope="module")
def inputs():
    return synth.synth_latent(2, seed=31), synth.synth_clip_inputs(2, seed=31), synth.synth_step_noise(50, 2, seed=NOISE_SEED)


def toy_denoiser():
    """make_golden.ToyDenoiser without importing the generator (its import pulls the reference tree onto sys.path)."""
    path = os.path.join(GOLD, "make_golden.py")
    tree = ast.parse(open(path).read())
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ToyDenoiser"], type_ignores=[]), path, "exec"), ns)
    return ns["ToyDenoiser"]()


def close(a, want):
    return np.allclose(a.numpy(), want, rtol=2e-6, atol=1e-6 * float(np.abs(want).max()))


# ---- H1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["identity_ddim50", "toy_ddim50_clipped"])
def test_generic_path_matches_the_reference_op_for_op(fx, inputs, case):
    """The same operations on the same dtypes as the reference: the `close` rule of test_rest_of_the_gaussian_diffusion_surface_matches_reference."""
    x, y, noise = inputs
    d = process.create_gaussian_diffusion(use_ddim=True)
    if case == "identity_ddim50":
        model, kw, clip = (lambda x, t, **k: x), {"y": {}}, False
    else:
        model, kw, clip = toy_denoiser(), {"y": {"seed": y["seed"]}}, True
    res = d.calc_bpd_loop(model, x, clip_denoised=clip, model_kwargs=kw, noise=noise, return_pred_xstart=True)
    assert d.last_path == "generic" and set(res) == set(KEYS) | {"pred_xstart"}
    for k in KEYS:
        assert res[k].shape == fx[f"{case}.{k}"].shape and res[k].dtype is torch.float32, k
        print(f"{case}.{k}: max |delta| {float(np.abs(res[k].numpy() - fx[f'{case}.{k}']).max()):.3e}")
        assert close(res[k], fx[f"{case}.{k}"]), k
    # column j is t = T - 1 - j: the last one is the decoder NLL at t = 0, from the last row of the noise
    t0 = torch.zeros(2, dtype=torch.long)
    x_t = d.q_sample(x, t0, noise[-1])
    term = d._vb_terms_bpd(model, x, x_t, t0, clip_denoised=clip, model_kwargs=kw)
    assert torch.equal(term["output"], res["vb"][:, -1]) and torch.equal(term["pred_xstart"], res["pred_xstart"][-1])
    mean = d.q_posterior_mean_variance(term["pred_xstart"], x_t, t0)[0]
    lv = torch.from_numpy(d.posterior_log_variance_clipped).float()[t0].view(-1, 1, 1, 1).expand(x.shape)
    nll = -process.discretized_gaussian_log_likelihood(x, means=mean, log_scales=0.5 * lv)
    assert torch.equal(process.mean_flat(nll) / np.log(2.0), res["vb"][:, -1])
    # ... and the first one the KL at t = T - 1
    tl = torch.full((2,), 49)
    term = d._vb_terms_bpd(model, x, d.q_sample(x, tl, noise[0]), tl, clip_denoised=clip, model_kwargs=kw)
    assert torch.equal(term["output"], res["vb"][:, 0])
    if case == "identity_ddim50":
        assert 1.3 < float(res["vb"][:, -1].min()) and float(res["vb"][:, -1].max()) < 1.6        # the interior of the discretised likelihood
    without = d.calc_bpd_loop(model, x, clip_denoised=clip, model_kwargs=kw, noise=noise)
    assert set(without) == set(KEYS) and all(torch.equal(without[k], res[k]) for k in KEYS)


def test_generic_path_noise_and_seed_arguments():
    d = process.create_gaussian_diffusion(use_ddim=True)
    x = torch.randn(2, 8, 1, 4)
    ident = lambda x, t, **k: x
    with pytest.raises(ValueError, match="noise must have shape"):
        d.calc_bpd_loop(ident, x, noise=torch.zeros(49, 2, 8, 1, 4))
    with pytest.raises(ValueError, match="noise must have shape"):
        d.calc_bpd_loop(ident, x, noise=torch.zeros(50, 1, 8, 1, 4))
    a, b, c = (d.calc_bpd_loop(ident, x, seed=s) for s in (7, 7, 8))
    assert all(torch.equal(a[k], b[k]) for k in KEYS) and not torch.equal(a["vb"], c["vb"])
    assert torch.equal(a["total_bpd"], a["vb"].sum(1) + a["prior_bpd"]) and a["vb"].shape == (2, 50)


# ---- H2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,use_ddim", [("ddim", True), ("ddpm", False)])
def test_bpd_rows_against_the_reference_tables(tag, use_ddim):
    g = np.load(os.path.join(GOLD, "tables.npz"))
    tab = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".")}
    rows = engine.bpd_rows(tab)
    n = len(tab["betas"])
    assert rows.dtype.itemsize == ctypes.sizeof(_lib.SynBpdRow) == 24 and len(rows) == n
    for name, (_, offset) in rows.dtype.fields.items():
        assert getattr(_lib.SynBpdRow, name).offset == offset, name
    for field, table in (("c1", "posterior_mean_coef1"), ("c2", "posterior_mean_coef2"), ("log_var", "posterior_log_variance_clipped"),
                         ("r", "sqrt_recip_alphas_cumprod")):
        assert np.array_equal(rows[field], tab[table].astype(np.float32)), field          # fp64 -> fp32, rounded once
    assert np.array_equal(rows["inv_m"], (1.0 / tab["sqrt_recipm1_alphas_cumprod"]).astype(np.float32))
    assert rows["first"][0] == 1 and not rows["first"][1:].any()
    assert rows["c1"][0] == 1.0 and rows["c2"][0] == 0.0                                   # at t = 0 the mean is pred_xstart
    # the same rows from this project's own process
    own = engine.bpd_rows(process.create_gaussian_diffusion(use_ddim=use_ddim).tables())
    for field in rows.dtype.names:
        assert np.allclose(own[field], rows[field], rtol=1e-6, atol=0), field


def test_chunk_plan(monkeypatch):
    assert engine.bpd_chunks(100, 1, "cpu") == [(0, 100)]                                   # (no wave-per-sequence kernel: one batch)
    assert engine.bpd_chunks(100, 1, "cpu", 8) == [(8 * i, min(8 * i + 8, 100)) for i in range(13)]
    assert engine.bpd_chunks(100, 1, "cpu", 64) == [(0, 64), (64, 100)]
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            engine.bpd_chunks(100, 1, "cpu", bad)
    monkeypatch.setattr(engine, "seq_pass_clips", lambda v, dev: 1024 // v if v != 3 else 256)
    plan = lambda n, v=1: engine.bpd_chunks(n, v, "cpu")
    assert plan(1000) == [(0, 1000)] and plan(1024) == [(0, 1024)]
    assert plan(2000) == [(0, 2000)]                                   # 976 left: more than half a pass, one batch of two passes
    assert plan(1200) == [(0, 1024), (1024, 1200)]                     # 176 left: on their own, with the kernel that suits them
    assert plan(2048) == [(0, 1024), (1024, 2048)]
    assert plan(40000) == [(1024 * i, 1024 * i + 1024) for i in range(39)] + [(39936, 40000)]
    assert plan(1300, 2) == [(0, 512), (512, 1300)] and plan(1200, 2) == [(0, 512), (512, 1024), (1024, 1200)]
    for n in (1, 1025, 3071, 5000):
        got = plan(n)
        assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))


# ---- H3 ------------------------------------------------------------------------------------------------------------------------------
def test_signatures_equal_the_reference_parameters_plus_keyword_only_extras(fx):
    want = {s.split("(", 1)[0]: s.split("(", 1)[1][:-1] for s in fx["signatures"]}
    extras = {"_vb_terms_bpd": [], "_prior_bpd": [], "calc_bpd_loop": ["noise", "seed", "first_clip", "chunk", "return_pred_xstart"]}
    assert set(want) == set(extras)
    for name, ref in want.items():
        ps = [p for p in inspect.signature(getattr(process.SpacedDiffusion, name)).parameters.values() if p.name != "self"]
        pos = [p for p in ps if p.kind is p.POSITIONAL_OR_KEYWORD]
        assert ",".join(p.name + ("" if p.default is p.empty else "=" + repr(p.default)) for p in pos) == ref, name
        assert [p.name for p in ps if p.kind is p.KEYWORD_ONLY] == extras[name] and len(ps) == len(pos) + len(extras[name])
        assert all(p.default is not p.empty for p in ps if p.kind is p.KEYWORD_ONLY)


def test_a_probe_call_is_a_type_error_that_still_names_the_reference_line():
    d = process.create_gaussian_diffusion()
    for name, line in (("calc_bpd_loop", "1548"), ("_vb_terms_bpd", "1201"), ("_prior_bpd", "1530")):
        for exc in (TypeError, NotImplementedError):
            with pytest.raises(exc, match=rf"gaussian_diffusion\.py:{line}"):
                getattr(d, name)(None)
    with pytest.raises(TypeError, match="unexpected keyword"):
        d.calc_bpd_loop(None, torch.zeros(1, 8, 1, 4), steps=3)
    with pytest.raises(process.UnboundCall, match="1548"):
        d.calc_bpd_loop(None, None)


# ---- H4 ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_mirrored():
    header = open(os.path.join(REPO, "include", "syn_hip.h")).read()
    assert re.search(r"^int\s+syn_bpd_terms\s*\(", header, flags=re.M) and "syn_bpd_terms" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.syn_bpd_terms.argtypes is not None and len(lib.syn_bpd_terms.argtypes) == 12
    assert lib.syn_version() == 9 == _lib.ABI_VERSION                   # additive: the version stays
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "syn_hip.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(syn_bpd_row), '
                             'offsetof(syn_bpd_row, log_var), offsetof(syn_bpd_row, first));return 0;}\n')
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", os.path.join(td, "sz")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SynBpdRow), _lib.SynBpdRow.log_var.offset, _lib.SynBpdRow.first.offset] == [24, 8, 20]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    ok = dict(table=256, n_rows=4, t_row=256, clip=256, x_start=256, n_clips=2, x_t=256, noise=256, pred=256, n_seq=5, out=256)
    order = ("table", "n_rows", "t_row", "clip", "x_start", "n_clips", "x_t", "noise", "pred", "n_seq", "out")
    bad = [("table", None), ("n_rows", 0), ("t_row", None), ("x_start", None), ("n_clips", 0), ("x_t", None), ("noise", None), ("pred", None),
           ("n_seq", 0), ("n_seq", -1), ("out", None), ("x_start", 264), ("x_t", 260), ("noise", 272 + 4), ("pred", 258), ("out", 258),
           ("t_row", 257), ("clip", 258)]
    for k, v in bad:
        a = dict(ok, **{k: v})
        assert lib.syn_bpd_terms(*[a[n] for n in order], None) != 0, (k, v)
        assert b"syn_bpd_terms" in lib.syn_last_error()
    a = dict(ok, clip=None)                                              # clip = NULL pairs sequence i with clip i
    assert lib.syn_bpd_terms(*[a[n] for n in order], None) != 0 and b"n_seq must not exceed n_clips" in lib.syn_last_error()
