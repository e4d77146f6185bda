"""CPU pins of tests/train_stack_ref.py (no GPU): the fragment layout, the sliced metric, the hand-written DropPath table, that every hazard case
reaches its range from this test's input, the float64 block and its backward in two independent formulations, and every cap of
tests/test_gpu_train_stack.py that can be checked without the kernels - each against a float32 restatement of the kernels' own scalar code."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import outlier_weights as ow
from tests import train_stack_ref as R


def test_unpack_xt_inverts_a_pack_written_from_the_layout_sentence():
    """[F / 16][M / 32][64 lanes] x 8 bf16: lane 16 g + lr of fragment (nf, tile) holds X[32 tile + 8 g + e][16 nf + lr], e = 0 .. 7."""
    Fd, M = 48, 96
    X = torch.randn(M, Fd, generator=torch.Generator().manual_seed(1)).bfloat16()
    buf = torch.zeros(Fd // 16, M // 32, 64, 8, dtype=torch.bfloat16)
    for nf in range(Fd // 16):
        for tile in range(M // 32):
            for lane in range(64):
                g, lr = lane // 16, lane % 16
                for e in range(8):
                    buf[nf, tile, lane, e] = X[32 * tile + 8 * g + e, 16 * nf + lr]
    assert torch.equal(R.unpack_xt(buf.reshape(-1), Fd, M), X)
    assert torch.equal(R.unpack_xt(buf.reshape(-1).view(torch.uint8), Fd, M), X)            # the byte buffers the kernels are handed


def test_sliced_rel_l2_sees_one_wrong_workgroup():
    g = torch.Generator().manual_seed(2)
    want = torch.randn(64 * 32, 512, generator=g)
    got = want.clone()
    got[5 * 32:6 * 32, 256:384] *= 1.3                          # one head of one sequence, 30 % off
    whole = float((got - want).norm() / want.norm())
    assert whole < 3e-2 and abs(R.sliced_rel_l2(got, want) - 0.3) < 1e-6, whole             # the whole-tensor gate of 3e-2 lets it through
    e = R.slice_errors(got, want)
    assert e.shape == (64, 4) and int((e > 0).sum()) == 1 and e[5, 2] > 0.29
    # a slice that must be zero: exactly zero, or infinitely wrong; -0.0 is zero; a NaN never passes
    want[0:32, 0:128] = 0
    got = want.clone()
    assert R.sliced_rel_l2(got, want) == 0
    got[3, 7] = -0.0
    assert R.sliced_rel_l2(got, want) == 0
    got[3, 7] = 1e-30
    assert R.sliced_rel_l2(got, want) == math.inf
    got = want.clone()
    got[40, 300] = math.nan
    assert R.sliced_rel_l2(got, want) == math.inf
    # part segments: one sequence's row x 128 columns
    assert R.slice_errors(torch.ones(4, 512), torch.ones(4, 512), 1, 128).shape == (4, 4)


def test_bf16_steps_counts_representable_values():
    a = torch.tensor([1.0, 1.0, -1.0, 0.0, 2.0 ** -133], dtype=torch.bfloat16)
    b = torch.tensor([1.0078125, 0.99609375, -1.0078125, -0.0, -(2.0 ** -133)], dtype=torch.bfloat16)
    assert R.bf16_steps(a, b).tolist() == [1, 1, 1, 0, 2]


def test_drop_path_table_is_the_one_written_down():
    dp = R.drop_path_table(4)
    assert dp.shape == (16, 4) and dp.dtype is torch.float32
    zeros = {(int(r), int(s)) for r, s in (dp == 0).nonzero().tolist()}
    assert zeros == {(4, 0), (5, 0), (10, 1), (7, 2)}                   # block 2 both / block 5 attention / block 3 MLP
    assert int((dp == 1.25).sum()) == 64 - 4 and bool((dp[:, 3] == 1.25).all())
    one = R.drop_path_table(1)                                          # a single sequence carries all three
    assert one.shape == (16, 1) and {int(r) for r, _ in (one == 0).nonzero().tolist()} == {4, 5, 10, 7}
    assert {(int(r), int(s)) for r, s in (R.drop_path_table(64) == 0).nonzero().tolist()} == zeros


def test_weights_are_the_synthetic_blocks_with_layernorm_moved():
    from tests.refmodel import synth_state_dict
    base, sd = synth_state_dict("beatx"), R.state_dict("plain")
    assert len(sd) == 8 * 11
    for l in range(8):
        p = f"mytimmblocks.{l}."
        assert torch.equal(sd[p + "attn.qkv.weight"], base[p + "attn.qkv.weight"]) and torch.equal(sd[p + "mlp.fc1.bias"], base[p + "mlp.fc1.bias"])
        for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"):
            d = sd[p + n] - base[p + n]
            assert 0.07 < float(d.std()) < 0.13
        assert float((sd[p + "norm1.weight"] - 1).abs().mean()) > 0.05 and float(sd[p + "norm1.bias"].abs().mean()) > 0.05
    hz = R.state_dict("gelu")
    assert float((hz["mytimmblocks.4.mlp.fc1.bias"] - sd["mytimmblocks.4.mlp.fc1.bias"]).abs().max()) == 16.0
    assert torch.equal(hz["mytimmblocks.4.norm2.weight"], sd["mytimmblocks.4.norm2.weight"])      # the same LayerNorm edit in every case


# ---- the hazard ranges are reached from this test's input ------------------------------------------------------------------------------------------
N_HAZ = 4           # sequences of the hazard runs of tests/test_gpu_train_stack.py


@functools.lru_cache(maxsize=None)
def _chain(case):
    with torch.no_grad():
        return R.chain_exact(R.state_dict(case), R.h0(N_HAZ))


def _ranges(case):
    sd = {k: v.double() for k, v in R.state_dict(case).items()}
    hs = _chain(case)
    return [ow.block_ranges(sd, hs[i], i) for i in range(8)], [ow.stream_ranges(hs[i + 1]) for i in range(8)]


def test_plain_weights_never_leave_the_quiet_range():
    blocks, streams = _ranges("plain")
    assert max(b["fc1"] for b in blocks) < 6 and sum(b["fc1_beyond"] for b in blocks) == 0
    assert max(b["top_prob"] for b in blocks) < 0.2 and max(s["mean2_over_var"] for s in streams) < 0.02


def test_every_hazard_case_reaches_its_range_from_h0():
    """The conditions of tests/test_ranges_host.py::test_every_hazard_case_reaches_its_range (there: one sequence of the sampling path; the count of
    pre-activations beyond 10.5 is per sequence), on the float64 chain from `h0(4)`.  Measured: gelu 16.6 / 19.0 / 27.1 with 3778 / 4096 / 4096
    beyond 10.5; sharp logits 75.7 / 72.9, median top probability 0.98 / 0.98; massive |h| 112 .. 116, four channels, share 0.85 .. 0.98;
    shifted mean^2 / var 724 after block 0, 143 after block 7."""
    blocks, _ = _ranges("gelu")
    for (blk, _), reach in zip(ow.GELU_BLOCKS, (15.3, 18.9, 27.1)):
        print("gelu, block", blk, blocks[blk])
        assert blocks[blk]["fc1"] >= 0.9 * reach and blocks[blk]["fc1_beyond"] >= 0.9 * 1000 * N_HAZ
    blocks, _ = _ranges("sharp")
    r2, r5 = (blocks[b] for b in ow.SHARP_BLOCKS)
    print("sharp, blocks 2 and 5:", r2, r5)
    assert r2["logit"] >= 0.9 * 57 and r2["top_prob"] >= 0.9 * 0.92 and r5["logit"] >= 0.9 * 40 and r5["top_prob"] >= 0.9 * 0.82
    _, streams = _ranges("massive")
    print("massive:", streams[0], streams[7])
    assert max(s["abs"] for s in streams) >= 0.9 * 115 and all(s["abs"] >= 100 and s["outlier_channels"] == 4 and s["outlier_share"] > 0.5 for s in streams)
    _, streams = _ranges("shifted")
    print("shifted:", streams[0], streams[7])
    assert streams[0]["mean2_over_var"] >= 0.9 * 547 and streams[7]["mean2_over_var"] >= 0.9 * 98


# ---- caps of the GPU test, against float32 restatements of the kernels' scalar code ----------------------------------------------------------------
def _rows_of(case):
    """Residual-stream rows of a case, as the kernel sees them (fp32): all nine taps of the chain."""
    return torch.cat([h.float().reshape(-1, 512) for h in _chain(case)])


@pytest.mark.parametrize("case", ["plain", "shifted", "massive"])
def test_one_pass_statistics_stay_inside_their_gate(case):
    """`row_stats` restated in float32 with its summation order, against float64 statistics of the same rows.  Measured, as a share of the gate:
    mean 0.03 (plain) / 0.19 (shifted) / 0.21 (massive); rstd 0.11 / 0.12 / 0.13, i.e. 1.0 x 2^-23 (1 + mean^2 / var): the factor 8 is room for
    another summation order, not for another algorithm."""
    h = _rows_of(case)
    mean, rstd = R.row_stats_restated(h.numpy())
    m64, r64, _ = R.row_stats64(h)
    em = float(((torch.from_numpy(mean).double() - m64).abs() / R.mean_gate(h)).max())
    er = float(((torch.from_numpy(rstd).double() / r64 - 1).abs() / R.rstd_gate(h)).max())
    print(f"{case}: restated row_stats, worst share of the gate: mean {em:.3f}, rstd {er:.3f}")
    assert em <= 0.5 and er <= 0.25
    # a two-term slip in the restated algorithm (a dropped lane) is far outside: the gate has teeth
    bad = h.clone()
    bad[:, 17] = 0
    mb, rb = R.row_stats_restated(bad.numpy())
    assert float(((torch.from_numpy(mb).double() - m64).abs() / R.mean_gate(h)).max()) > 10


@pytest.mark.parametrize("case", ["plain", "shifted", "massive"])
def test_layernorm_formula_flips_few_bf16_roundings(case):
    """bf16((h - mean) rstd g + b) evaluated in float64 against the same formula in fp32 (torch, no fma), both with the fp32 statistics the kernel
    would save: every difference is one bf16 step (`layer_norm_bf16_check`: at the magnitude of what was added), on at most 1e-4 of the elements
    (the GPU test allows 4e-4 against the device, whose compiler may contract the last two operations).  Measured 7e-6 .. 4e-5.  Counted in steps
    of the RESULT a difference reaches 12 where x-hat g and b cancel: that is why the step is not taken there."""
    h = _rows_of(case)
    sd = R.state_dict(case)
    g, b = sd["mytimmblocks.3.norm1.weight"], sd["mytimmblocks.3.norm1.bias"]
    mean, rstd = (torch.from_numpy(v) for v in R.row_stats_restated(h.numpy()))
    y64 = ((h.double() - mean.double()[:, None]) * rstd.double()[:, None] * g.double() + b.double()).float().bfloat16()
    share, steps = R.layer_norm_bf16_check(y64, h, mean, rstd, g, b)
    print(f"{case}: fp32 LayerNorm formula, share of bf16 outputs off: {share:.2e}, largest difference {steps:.3f} steps")
    assert steps <= 1.0 and share <= 1e-4
    off = y64.clone()
    i = int(off[5].float().abs().argmax())
    off[5, i] = off[5, i] * 1.02                                        # three to five steps of one element: seen
    assert R.layer_norm_bf16_check(off, h, mean, rstd, g, b)[1] > 1.0


def test_abramowitz_stegun_gelu_and_its_derivative_stay_inside_half_their_gates():
    """`gelu_erf` / `gelu_grad` restated in fp32 (exact reciprocal and exp2) against float64 over [-30, 30].  Measured: gelu worst
    |err| / max(1, |x|) 1.85e-7, worst |err| 4.7e-7; gelu_grad worst |err| 2.8e-7.  The GPU gates (4e-7 max(1, |pre|), 6e-7 |da|) double these
    for the hardware's v_rcp_f32 / v_exp_f32."""
    x = np.linspace(-30.0, 30.0, 2000001).astype(np.float32)
    xd = torch.from_numpy(x).double()
    e = np.abs(R.gelu_as(x).astype(np.float64) - R.gelu64(xd).numpy())
    rel = float((e / np.maximum(1.0, np.abs(x))).max())
    eg = float(np.abs(R.gelu_grad_as(x).astype(np.float64) - R.gelu_grad64(xd).numpy()).max())
    print(f"A&S gelu: worst |err| / max(1, |x|) {rel:.3e}, worst |err| {e.max():.3e}; gelu_grad worst |err| {eg:.3e}")
    assert rel <= 2e-7 and e.max() <= 5e-7 and eg <= 3e-7
    # the float64 forms themselves, against torch's
    xs = torch.linspace(-30, 30, 4001, dtype=torch.float64).requires_grad_(True)
    ref = F.gelu(xs)
    assert float((R.gelu64(xs.detach()) - ref.detach()).abs().max()) < 1e-14
    assert float((R.gelu_grad64(xs.detach()) - torch.autograd.grad(ref.sum(), xs)[0]).abs().max()) < 1e-14
    # and the gates: bf16 rounding plus the floor covers the restatement everywhere, |pre| > 10.5 included
    want = R.gelu64(xd)
    got = torch.from_numpy(R.gelu_as(x)).bfloat16().double()
    assert bool(((got - want).abs() <= R.gelu_gate(xd, want)).all())


# ---- the float64 block and its backward ---------------------------------------------------------------------------------------------------------
def _block_case(case="plain", l=3, n=3, seed=5):
    P = R.block_params(R.state_dict(case), l)
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n * 32, 512, generator=g, dtype=torch.float64)
    dh = torch.randn(n * 32, 512, generator=g, dtype=torch.float64)
    fa, fm = torch.tensor([1.25, 0.0, 1.25][:n]), torch.tensor([1.25, 1.25, 0.0][:n])
    return P, h, dh, fa, fm


def test_exact_block_equals_torch_functional_and_its_autograd():
    P, h, dh, fa, fm = _block_case()
    x = h.clone().requires_grad_(True)
    par = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    z = F.layer_norm(x, (512,), par["g1"], par["b1"], 1e-5)
    q, k, v = F.linear(z, par["wqkv"]).reshape(3, 32, 3, 4, 128).permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(96, 512)
    hm = x + fa.double().repeat_interleave(32)[:, None] * F.linear(o, par["wproj"], par["bproj"])
    z2 = F.layer_norm(hm, (512,), par["g2"], par["b2"], 1e-5)
    out = hm + fm.double().repeat_interleave(32)[:, None] * F.linear(F.gelu(F.linear(z2, par["w1"], par["bfc1"])), par["w2"], par["bfc2"])
    out.backward(dh)
    got_out, _ = R.block_forward_exact(P, h, fa, fm)
    ex = R.block_backward_exact(P, h, dh, fa, fm)
    close = lambda a, b: float((a - b).norm() / b.norm()) < 1e-12
    assert close(got_out, out.detach()) and close(ex["dh_in"], x.grad)
    for seg, name in (("ln2_g", "g2"), ("ln2_b", "b2"), ("fc2_b", "bfc2"), ("fc1_b", "bfc1"), ("ln1_g", "g1"), ("ln1_b", "b1"), ("proj_b", "bproj")):
        c0, w = R.PART[seg]
        assert close(ex["part"][:, c0:c0 + w].sum(0), par[name].grad), seg                # the per-sequence partials add up to the parameter gradient
    # the transposed gradients are the left operands of the weight gradients
    assert close(ex["dyt_qkv"].T @ z.detach(), par["wqkv"].grad) and close(ex["dyt_fc1"].T @ z2.detach(), par["w1"].grad)
    assert close(ex["dyt_proj"].T @ o.detach(), par["wproj"].grad)
    # dropped branches: exactly zero
    assert not ex["dyt_fc2"][64:96].any() and not ex["dyt_fc1"][64:96].any() and not ex["dyt_proj"][32:64].any() and not ex["dyt_qkv"][32:64].any()


def test_backward_model_without_rounding_is_the_autograd():
    """The hand-written backward of `block_backward_model` (the kernel's formulas) with no rounding reproduces float64 autograd in every output."""
    for case, l in (("plain", 3), ("sharp", 2), ("shifted", 1)):
        P, h, dh, fa, fm = _block_case(case, l)
        if case == "shifted":
            h = h + 30.0
        ex, mo = R.block_backward_exact(P, h, dh, fa, fm), R.block_backward_model(P, h, dh, fa, fm, rounded=False)
        for k in ex:
            e = R.sliced_rel_l2(mo[k], ex[k], 1 if k == "part" else 32, 128)
            assert e < 1e-9, (case, k, e)


def test_backward_model_takes_the_saved_tensors_it_would_compute():
    P, h, dh, fa, fm = _block_case("gelu", 4)
    saved = R.block_forward_model(P, h, fa)
    assert set(saved) == set(R.SAVED)
    own, fed = R.block_backward_model(P, h, dh, fa, fm), R.block_backward_model(P, h, dh, fa, fm, saved={k: v.clone() for k, v in saved.items()})
    assert all(torch.equal(own[k], fed[k]) for k in own)
    # and they matter: the fc1 pre-activation of another block's weights is another gradient
    saved["pre"] = saved["pre"].flip(0)
    assert R.sliced_rel_l2(R.block_backward_model(P, h, dh, fa, fm, saved=saved)["dyt_fc1"], own["dyt_fc1"]) > 0.1


def test_backward_model_error_is_bf16_class():
    """E_model (rounded model against autograd) per stage: a fraction of a percent, the design's bf16 operands (measured 2.3e-3 .. 7.6e-3 on this
    block); the model passes both gates against itself, and its first rounding point is where the kernel's is."""
    P, h, dh, fa, fm = _block_case("plain", 3)
    ex, mo = R.block_backward_exact(P, h, dh, fa, fm), R.block_backward_model(P, h, dh, fa, fm)
    gates = R.backward_gates(mo, ex, mo)
    for st, (em, de, dm, r_exact, r_model) in gates.items():
        print(f"plain block 3, {st}: E_model {em:.2e}")
        assert 1e-4 < em < 1.5e-2 and dm == 0 and r_exact <= 1.0 + 1e-12, st
    assert torch.equal(mo["dyt_fc2"], R.bf16(R._factor_rows(fm, 96) * dh))
