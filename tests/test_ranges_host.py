"""CPU pins of the step kernels' numerical ranges (no GPU): the wave-per-sequence kernel's activation (`gelu_fast` of syn_seq.inc, restated in
float32 as tests/kseq_model.gelu_kseq) against the exact GELU over the whole float range; the kernel's lane-level model on the hazard weights
of tests/outlier_weights.py against the fp64 oracle; and the blind spot those weights close - the stock synthetic weights never show a step
kernel a pre-activation beyond 6, and every hazard case must keep reaching the range it is named for."""
import functools

import numpy as np
import pytest
import torch

from oracle import denoiser_ref as dr
from syntalker_amd import synth, tape
from tests import kseq_model as km
from tests import outlier_weights as ow
from tests.refmodel import synth_state_dict
from tests.test_gpu_parity import FWD_TOL        # the project's bound on one model evaluation (2e-2)

GELU_TOL = 3e-5                # the fit's own figure: 2.55e-5 measured for every clamp of x^2 in [36, 100]


def _gelu_exact(x32):
    x = torch.from_numpy(np.asarray(x32, np.float32)).double()
    return (0.5 * x * torch.special.erfc(-x / np.sqrt(2.0))).numpy()


def _sweep_points():
    special = [1e4, 1e10, 1e19, 3e38, 0.0, 1e-30, 1e-40]                 # 1e-40: a float32 denormal
    return np.concatenate([np.linspace(-40.0, 40.0, 800001), special, [-v for v in special]]).astype(np.float32)


def test_kseq_gelu_against_the_exact_gelu_over_the_float_range():
    x = _sweep_points()
    assert x.size == 800015 and np.signbit(x[-3]) and x[-3] == 0 and 0 < x[800007] < 1.2e-38
    got = km.gelu_kseq(x)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - _gelu_exact(x))
    print(f"gelu_kseq: max |error| {err.max():.3e} at x = {x[err.argmax()]:.4f}")
    assert err.max() <= GELU_TOL
    # any clamp of x^2 in [36, 100] does: the constant is not a tuned one
    for clamp in (36.0, 100.0):
        assert np.abs(km.gelu_kseq(x, np.float32(clamp)).astype(np.float64) - _gelu_exact(x)).max() <= GELU_TOL


def test_the_sweep_tells_the_unclamped_formula_apart():
    """The formula as the kernel ran it before the clamp: the quartic turns over at x^2 = 123.7, a strongly active unit is silenced and a
    strongly inactive one passes its negative value through.  The sweep above must see that."""
    x = np.array([10.5, 11.0, 11.2, 12.0, -12.0, -15.0], np.float32)
    err = np.abs(km.gelu_kseq(x, clamp=None).astype(np.float64) - _gelu_exact(x))
    assert err[0] < 1e-4 and err[1] > 0.5 and err[2] > 9 and err[3] > 11.9 and err[4] > 11.9 and err[5] > 14.9, err
    xs = _sweep_points()
    assert np.abs(km.gelu_kseq(xs, clamp=None).astype(np.float64) - _gelu_exact(xs)).max() > 1e37


def test_kseq_gelu_hands_a_nan_on():
    """The clamp is a v_min_f32, which drops a NaN operand: the NaN has to survive through x itself, or an upstream fault would be laundered."""
    out = km.gelu_kseq(np.array([np.nan, 1.0, -np.nan], np.float32))
    assert np.isnan(out[0]) and np.isnan(out[2]) and np.isfinite(out[1])


# ---------------------------------------------------------------------------------------------------------------------------------
def _inputs():
    return synth.synth_clip_inputs(1, seed=5), synth.synth_latent(1, seed=5), torch.tensor([417])


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """One sequence at t = 417 through the oracle: (state dict, fp64 forward, fp32 taps of the residual stream h0..h8)."""
    sd = synth_state_dict("beatx") if case == "stock" else ow.hazard_state_dict(case)
    y, x, t = _inputs()
    y64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in y.items()}
    taps = {}
    with torch.no_grad():
        got32 = dr.mdm_forward(sd, x, t, y, taps=taps)
        want = dr.mdm_forward(dr.cast_sd(sd, torch.float64), x.double(), t, y64)
    e = float((got32 - want).norm() / want.norm())
    assert e < 1e-5, (case, e)                   # the fp32 oracle (the taps below) is the fp64 one to rounding on these weights too
    return sd, want, taps


def _lane_model(sd, gelu):
    """tests/test_tape_layout.py's run of the lane-level model: the tape of `sd`, one sequence -> (1, 1536, 1, 32)."""
    fw = dr.fold_weights(sd)
    t_tape, bias = tape.build_tape(sd, fw["A"])
    y, x, t = _inputs()
    with torch.no_grad():
        cond, te = dr.clip_conditioning(sd, y, fw), dr.time_table(sd, fw)
    xb = tape.to_fragment_order_bf16(x.reshape(1, 1536, 32).transpose(1, 2).contiguous())[0].float().numpy()
    fr = torch.einsum("i,j->ij", torch.arange(32.), sd["rel_pos.inv_freq"].float())
    w = km.Wave(t_tape[:tape.TAPE_FRAGS].float().numpy(), bias.numpy())
    out = w.step(xb, cond[0].numpy(), te[int(t[0])].numpy(), fr.cos().numpy(), fr.sin().numpy(), gelu)
    return tape.from_fragment_order(torch.from_numpy(out)[None])[0].T.reshape(1, 1536, 1, 32)


@pytest.mark.parametrize("case", ow.CASES)
def test_lane_level_model_on_hazard_weights_vs_fp64_oracle(case):
    """k_seq's dataflow and rounding points (bf16 operands, fp32 accumulation, one-pass LayerNorm statistics, the clamped activation) on each hazard
    case, against the fp64 oracle.  FWD_TOL / 2: the design's own rounding leaves the GPU tests of tests/test_gpu_ranges.py a factor of two.
    Measured: gelu 3.8e-3, sharp 8.6e-3, massive 2.5e-3, shifted 2.3e-3 (stock weights: 4.9e-3); gelu with the activation unclamped: 1.2."""
    sd, want, _ = _oracle(case)
    got = _lane_model(sd, km.gelu_kseq)
    e = float((got.double() - want).norm() / want.norm())
    print(f"lane-level model, {case} weights: rel-L2 vs fp64 oracle {e:.3e}")
    assert e <= FWD_TOL / 2


def test_stock_weights_never_leave_the_fitted_range():
    """The blind spot itself: with `synth_state_dict` no fc1 pre-activation exceeds 6, attention is nearly uniform and a token's mean is small
    against its spread - a test on those weights alone says nothing about the ranges below."""
    sd, _, taps = _oracle("stock")
    blocks = [ow.block_ranges(sd, taps[f"h{i}"], i) for i in range(8)]
    streams = [ow.stream_ranges(taps[f"h{i + 1}"]) for i in range(8)]
    print("stock weights:", max(b["fc1"] for b in blocks), max(b["logit"] for b in blocks), max(b["top_prob"] for b in blocks),
          max(s["mean2_over_var"] for s in streams))
    assert max(b["fc1"] for b in blocks) < 6 and sum(b["fc1_beyond"] for b in blocks) == 0
    assert max(b["top_prob"] for b in blocks) < 0.2 and max(s["mean2_over_var"] for s in streams) < 0.02


def test_every_hazard_case_reaches_its_range():
    """Measured on one sequence (seed 5, t = 417); each threshold is that figure loosened by 10 %.
    gelu: |fc1 pre-activation| up to 15.3 / 18.9 / 27.1 in blocks 1 / 4 / 6, about 1000 of a sequence's 32 x 1024 beyond 10.5 in each.
    sharp: logits up to |57|, median top softmax probability 0.92 (block 2; 0.83 in block 5).
    massive: the residual stream reaches |115|, four channels stay beyond |80| at every token of all eight blocks and carry most of LayerNorm's variance.
    shifted: a token's mean^2 / variance reaches 547 after block 0 and 98 after block 7."""
    sd, _, taps = _oracle("gelu")
    for (blk, _), reach in zip(ow.GELU_BLOCKS, (15.3, 18.9, 27.1)):
        r = ow.block_ranges(sd, taps[f"h{blk}"], blk)
        print("gelu, block", blk, r)
        assert r["fc1"] >= 0.9 * reach and r["fc1_beyond"] >= 0.9 * 1000
    sd, _, taps = _oracle("sharp")
    r2, r5 = (ow.block_ranges(sd, taps[f"h{b}"], b) for b in ow.SHARP_BLOCKS)
    print("sharp, blocks 2 and 5:", r2, r5)
    assert r2["logit"] >= 0.9 * 57 and r2["top_prob"] >= 0.9 * 0.92 and r5["logit"] >= 0.9 * 40 and r5["top_prob"] >= 0.9 * 0.82
    sd, _, taps = _oracle("massive")
    streams = [ow.stream_ranges(taps[f"h{i + 1}"]) for i in range(8)]
    print("massive:", streams[0], streams[7])
    assert max(s["abs"] for s in streams) >= 0.9 * 115 and all(s["abs"] >= 100 and s["outlier_channels"] == 4 and s["outlier_share"] > 0.5 for s in streams)
    sd, _, taps = _oracle("shifted")
    s1, s8 = ow.stream_ranges(taps["h1"]), ow.stream_ranges(taps["h8"])
    print("shifted:", s1, s8)
    assert s1["mean2_over_var"] >= 0.9 * 547 and s8["mean2_over_var"] >= 0.9 * 98
