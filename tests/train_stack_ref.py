"""References for the persistent training kernels of the eight transformer blocks (`k_stack_train`, `k_stack_train_bwd`, `syn_train_stack_wgrad`:
csrc/syn_stack_train.inc).  Importable without a GPU; every function takes tensors of any device and works in float64.

The forward kernel writes out every bf16 operand it feeds to a GEMM, so each stage can be checked from the kernel's OWN saved input of that stage
("teacher-forced"): nothing compounds, and a stage's tolerance is that stage's arithmetic.  tests/test_train_stack_host.py pins these helpers on the
CPU, tests/test_gpu_train_stack.py holds the kernels against them.

Layouts (include/syn_hip.h, ABI 7): activations are rows [M = 32 n_seq][features]; `qkv` columns are [3][4 heads][128]; the transposed gradients
`dyt_*` are [features][M] bf16; `part` is [n_seq][4096] with the segments of PART below; the `xt_*` buffers are MFMA fragments (`unpack_xt`)."""
import functools
import math

import numpy as np
import torch

from tests import outlier_weights as ow
from tests.refmodel import synth_state_dict

D, FF, HEADS, HD, T, LAYERS = 512, 1024, 4, 128, 32, 8
CASES = ("plain",) + ow.CASES
SCL = HD ** -0.5
PART = {"ln2_g": (0, 512), "ln2_b": (512, 512), "fc2_b": (1024, 512), "fc1_b": (1536, 1024), "ln1_g": (2560, 512), "ln1_b": (3072, 512),
        "proj_b": (3584, 512)}                                      # name -> (first column, width) of a row of `part` (kP* of syn_stack_train.inc)
PART_COLS = 4096
H0_SCALE = 1.0                                                      # the residual stream the blocks start from: H0_SCALE * randn (see `h0`)
KEEP = 1.0 / 0.8                                                    # DropPath's factor of a branch that is kept (drop probability 0.2)


# ---- layouts and the metric -------------------------------------------------------------------------------------------------------------------
def unpack_xt(buf, F, M):
    """The [M][F] bf16 matrix X held by a fragment buffer of X^T: [F / 16][M / 32][64 lanes] x 8 bf16, lane 16 g + lr of fragment (nf, tile) holding
    X[32 tile + 8 g + e][16 nf + lr] for e = 0 .. 7 (what `xt_frag` of syn_stack_train.inc writes).  `buf`: uint8 bytes or bf16 elements."""
    v = buf.view(torch.bfloat16) if buf.dtype is torch.uint8 else buf
    assert v.dtype is torch.bfloat16 and v.numel() == F * M and F % 16 == 0 and M % 32 == 0, (v.dtype, v.numel(), F, M)
    return v.reshape(F // 16, M // 32, 4, 16, 8).permute(1, 2, 4, 0, 3).reshape(M, F)


def slice_errors(got, want, rows=32, cols=128):
    """Per slice (one sequence's `rows` rows x one group of `cols` columns: what one workgroup produces) of [M][F] tensors: |got - want| / |want| in
    float64, as a [M / rows][F / cols] tensor.  A slice with want == 0 gives 0 if got is exactly 0 there and inf otherwise."""
    g, w = got.double(), want.double()
    assert g.shape == w.shape and g.dim() == 2 and g.shape[0] % rows == 0 and g.shape[1] % cols == 0, (g.shape, w.shape, rows, cols)
    cut = lambda x: x.reshape(g.shape[0] // rows, rows, g.shape[1] // cols, cols)
    num, den = cut(g - w).pow(2).sum((1, 3)).sqrt(), cut(w).pow(2).sum((1, 3)).sqrt()
    num = torch.where(torch.isnan(num), torch.full_like(num, math.inf), num)                  # a NaN in `got` never passes
    return torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, math.inf)), num / den.clamp_min(1e-300))


def sliced_rel_l2(got, want, rows=32, cols=128):
    """The largest `slice_errors` entry: a whole-tensor rel-L2 divides one wrong workgroup's error by the norm of all 4 n_seq of them."""
    return float(slice_errors(got, want, rows, cols).max())


def bf16_steps(a, b):
    """Distance of two bf16 tensors in representable values (+0 and -0 coincide), as int32."""
    def ordered(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7FFF))
    return (ordered(a) - ordered(b)).abs()


def bf16_spacing(x):
    """Distance between neighbouring bf16 values at the magnitude of x (float64; normal range)."""
    return torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126))) - 7)


def layer_norm_bf16_check(got, h, mean, rstd, g, b):
    """A LayerNorm output `got` (bf16 [M][512]) against bf16(((h - mean) rstd) g + b) evaluated in fp32 with the given fp32 statistics.
    -> (share of elements that differ, largest difference in units of one bf16 step).  The step is taken at the magnitude of the larger of the
    result and the two summands (x-hat g and b): where they cancel, the fp32 roundings of the formula's own operations - fused into one fma by
    the device compiler or not - are several bf16 steps of the small RESULT, yet still far below one step of what was added."""
    t = (h.float() - mean.float()[:, None]) * rstd.float()[:, None] * g.float()
    want = (t + b.float()).bfloat16()
    diff = (got.double() - want.double()).abs()
    scale = torch.maximum(torch.maximum(t.abs(), b.float().abs().expand_as(t)), want.float().abs())
    return float((diff != 0).double().mean()), float((diff / bf16_spacing(scale)).max())


def bf16(x):
    """Round as the kernels do: the fp32 value of x to bf16 (nearest even), returned in float64."""
    return x.float().bfloat16().double()


# ---- weights, inputs, DropPath ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_dict(case):
    """`synth_state_dict("beatx")` (case "plain") or one of `outlier_weights.hazard_state_dict`, with the blocks' LayerNorm gains moved off 1 and their
    shifts off 0 by a further 0.1 * randn each (one generator, seed 77).  Shared and cached: do not write to it."""
    assert case in CASES, case
    sd = synth_state_dict("beatx") if case == "plain" else ow.hazard_state_dict(case)
    sd = {k: v.clone() for k, v in sd.items() if k.startswith("mytimmblocks.")}
    g = torch.Generator().manual_seed(77)
    for l in range(LAYERS):
        for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"):
            sd[f"mytimmblocks.{l}.{n}"] += 0.1 * torch.randn(512, generator=g)
    return sd


NAMES = {"g1": "norm1.weight", "b1": "norm1.bias", "wqkv": "attn.qkv.weight", "wproj": "attn.proj.weight", "bproj": "attn.proj.bias",
         "g2": "norm2.weight", "b2": "norm2.bias", "w1": "mlp.fc1.weight", "bfc1": "mlp.fc1.bias", "w2": "mlp.fc2.weight", "bfc2": "mlp.fc2.bias"}


def block_params(sd, l, device="cpu", dtype=torch.float64):
    return {k: sd[f"mytimmblocks.{l}.{n}"].to(device=device, dtype=dtype) for k, n in NAMES.items()}


def h0(n_seq, seed=11):
    """The blocks' input (n_seq, 32, 512) fp32: H0_SCALE * randn.  With unit scale every hazard case reaches its range from it
    (tests/test_train_stack_host.py pins that), as it does from the sampling path's embedded input."""
    return H0_SCALE * torch.randn(n_seq, T, D, generator=torch.Generator().manual_seed(seed + 1000 * n_seq))


DROP_BOTH, DROP_ATTN, DROP_MLP = 2, 5, 3          # the block whose two branches / attention branch / MLP branch one sequence loses


def drop_path_table(n_seq):
    """DropPath factors [16][n_seq] fp32 (row 2 l: attention branch of block l, 2 l + 1: its MLP branch), written out by hand: sequence 0 loses
    both branches of block 2, sequence 1 the attention branch of block 5, sequence 2 the MLP branch of block 3 (sequence min(i, n_seq - 1) where
    there are fewer); every other factor is 1 / 0.8."""
    dp = torch.full((2 * LAYERS, n_seq), KEEP, dtype=torch.float32)
    s = lambda i: min(i, n_seq - 1)
    dp[2 * DROP_BOTH, s(0)] = 0.0
    dp[2 * DROP_BOTH + 1, s(0)] = 0.0
    dp[2 * DROP_ATTN, s(1)] = 0.0
    dp[2 * DROP_MLP + 1, s(2)] = 0.0
    return dp


# ---- the operations in float64 ----------------------------------------------------------------------------------------------------------------
def row_stats64(h):
    """mean, rstd (biased variance, eps 1e-5) and mean^2 / var of each row, float64."""
    h = h.double()
    mean, var = h.mean(-1), h.var(-1, unbiased=False)
    return mean, (var + 1e-5).rsqrt(), mean * mean / var


def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))          # (erfc: no cancellation for strongly negative x)


def gelu_grad64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _heads(x):                                     # [M][4 * 128] -> [n_seq][4][32][128]
    return x.reshape(-1, T, HEADS, HD).transpose(1, 2)


def _rows(x):                                      # back
    return x.transpose(1, 2).reshape(-1, HEADS * HD)


def _layer_norm(h, g, b):
    mean, rstd, _ = row_stats64(h)
    xh = (h - mean[:, None]) * rstd[:, None]
    return xh * g + b, xh, rstd[:, None]


def attention_exact(qkv):
    """softmax(q k^T / sqrt(128)) v per sequence and head of qkv [M][1536] -> [M][512], float64, nothing rounded."""
    q, k, v = (_heads(qkv.double()[:, i * D:(i + 1) * D]) for i in range(3))
    return _rows(torch.softmax(q @ k.transpose(-1, -2) * SCL, -1) @ v)


def attention_model(qkv, rounded=True, internals=False):
    """The attention as `k_stack_train` runs it, in float64: q, k, v rounded to bf16, numerators exp(s - max) rounded to bf16, normalised by the sum
    of the ROUNDED numerators after the product with v, the output rounded to bf16 (it is the proj GEMM's operand, saved as `xt_attn`)."""
    r = bf16 if rounded else (lambda x: x)
    q, k, v = (r(_heads(qkv.double()[:, i * D:(i + 1) * D])) for i in range(3))
    s = q @ k.transpose(-1, -2)
    pn = r(torch.exp((s - s.amax(-1, keepdim=True)) * SCL))
    inv = 1.0 / pn.sum(-1, keepdim=True)
    o = r((pn @ v) * inv)
    return (_rows(o), (q, k, v, pn, inv)) if internals else _rows(o)


def _seq_sums(x):                                  # [M][F] -> [n_seq][F]: the 32-row column sums of each sequence
    return x.reshape(-1, T, x.shape[-1]).sum(1)


def _factor_rows(f, M):
    return f.double().reshape(-1, 1).expand(M // T, T).reshape(M, 1)


def _part(n_seq, ref, **seg):
    part = torch.zeros(n_seq, PART_COLS, dtype=torch.float64, device=ref.device)
    for name, v in seg.items():
        c0, w = PART[name]
        part[:, c0:c0 + w] = _seq_sums(v)
    return part


def block_forward_exact(P, h, fa, fm):
    """One pre-LN block in float64: h [M][512], P = block_params(...), fa / fm = the DropPath factors [n_seq] of its attention / MLP branch.
    -> (output, {the intermediates by the names of the kernel's saved tensors})."""
    h = h.double()
    M = h.shape[0]
    z1, _, _ = _layer_norm(h, P["g1"], P["b1"])
    qkv = z1 @ P["wqkv"].T
    o = attention_exact(qkv)
    hm = h + _factor_rows(fa, M) * (o @ P["wproj"].T + P["bproj"])
    z2, _, _ = _layer_norm(hm, P["g2"], P["b2"])
    pre = z2 @ P["w1"].T + P["bfc1"]
    out = hm + _factor_rows(fm, M) * (gelu64(pre) @ P["w2"].T + P["bfc2"])
    return out, {"z1": z1, "qkv": qkv, "o": o, "h_mlp": hm, "z2": z2, "pre": pre}


def chain_exact(sd, h, dp=None):
    """The eight blocks in float64 from h (n_seq, 32, 512): [h_attn of block 0 .. 7, h_out], each (n_seq, 32, 512)."""
    n = h.shape[0]
    hs, x = [h.double()], h.double().reshape(n * T, D)
    one = torch.ones(n, dtype=torch.float64)
    for l in range(LAYERS):
        x, _ = block_forward_exact(block_params(sd, l), x, one if dp is None else dp[2 * l], one if dp is None else dp[2 * l + 1])
        hs.append(x.reshape(n, T, D))
    return hs


def block_backward_exact(P, h, dh_out, fa, fm):
    """float64 autograd of one block from its input h [M][512] and the gradient dh_out at its output.  -> dict of [M][features] tensors
    `dh_in`, `dyt_fc2`, `dyt_fc1`, `dyt_proj`, `dyt_qkv` (the gradients at the four Linears' outputs, NOT transposed) and `part` [n_seq][4096]
    (per-sequence sums of the bias / LayerNorm parameter gradients, segments of PART)."""
    with torch.enable_grad():
        h = h.detach().double().requires_grad_(True)
        M = h.shape[0]
        z1, xh1, _ = _layer_norm(h, P["g1"], P["b1"])
        qkv = z1 @ P["wqkv"].T
        yp = attention_exact(qkv) @ P["wproj"].T + P["bproj"]
        hm = h + _factor_rows(fa, M) * yp
        z2, xh2, _ = _layer_norm(hm, P["g2"], P["b2"])
        pre = z2 @ P["w1"].T + P["bfc1"]
        y2 = gelu64(pre) @ P["w2"].T + P["bfc2"]
        out = hm + _factor_rows(fm, M) * y2
        dh, dy2, dpre, dyp, dqkv, dz2, dz1 = torch.autograd.grad(out, [h, y2, pre, yp, qkv, z2, z1], dh_out.double())
    part = _part(M // T, h, ln2_g=dz2 * xh2.detach(), ln2_b=dz2, fc2_b=dy2, fc1_b=dpre, ln1_g=dz1 * xh1.detach(), ln1_b=dz1, proj_b=dyp)
    return {"dh_in": dh, "dyt_fc2": dy2, "dyt_fc1": dpre, "dyt_proj": dyp, "dyt_qkv": dqkv, "part": part}


SAVED = ("qkv", "h_mlp", "pre", "mean_attn", "rstd_attn", "mean_mlp", "rstd_mlp")       # what `k_stack_train_bwd` reads of a block besides h_attn


def block_forward_model(P, h, fa, rounded=True):
    """What `k_stack_train` saves of one block for the backward, from the block's input h, in float64 with the forward kernel's rounding points:
    {qkv, h_mlp, pre, mean_attn, rstd_attn, mean_mlp, rstd_mlp} (statistics [M])."""
    r = bf16 if rounded else (lambda x: x)
    h = h.double()
    z1, _, _ = _layer_norm(h, P["g1"], P["b1"])
    qkv = r(z1) @ r(P["wqkv"]).T
    hm = h + _factor_rows(fa, h.shape[0]) * (attention_model(qkv, rounded) @ r(P["wproj"]).T + P["bproj"])
    z2, _, _ = _layer_norm(hm, P["g2"], P["b2"])
    pre = r(z2) @ r(P["w1"]).T + P["bfc1"]
    (ma, ra, _), (mm, rm, _) = row_stats64(h), row_stats64(hm)
    return {"qkv": qkv, "h_mlp": hm, "pre": pre, "mean_attn": ma, "rstd_attn": ra, "mean_mlp": mm, "rstd_mlp": rm}


def block_backward_model(P, h, dh_out, fa, fm, rounded=True, saved=None):
    """`block_backward_exact` with the kernels' rounding points, everything else in float64; `rounded=False` rounds nowhere and must reproduce the
    autograd (that is how the formulas below are pinned).

    `saved`: what the backward kernel READS of the forward - qkv, h_mlp, pre and the four statistics, as `block_forward_model` returns them and as
    `k_stack_train` saved them.  Against the device the device's own saved tensors go here (teacher-forced, like the forward's stages): the
    forward's roundings are then shared value by value.  A model that recomputes them from h differs from the device in a share of the
    forward's bf16 roundings (a rounding decided the other way is a full bf16 step), which the backward then carries as an error of the size
    of E_model itself - most of all on a shifted stream, where the fp32 statistics move the LayerNorm outputs by 1e-4 of their size.

    bf16 roundings, read off csrc/syn_stack_train.inc:
    forward (`k_stack_train`, which produced what the backward reads; `block_forward_model`)
      * all four weight matrices (the packed fragment sets);
      * LayerNorm outputs (line 168: the qkv and fc1 GEMMs' operands);
      * q, k, v (216-218), the softmax numerators exp(s - max) (254), normalised by the sum of the rounded numerators (256, 260), the attention
        output (270); `qkv` and `pre` themselves are saved in fp32 and not rounded.
    backward (`k_stack_train_bwd`)
      * bf16(f dh) rows at the start of either branch (525): the operand of the W2 / Wproj GEMM and `dyt_fc2` / `dyt_proj`;
      * bf16(da gelu'(pre)) (632): the operand of the W1 GEMM and `dyt_fc1`; the fc1-bias partial sums the UNROUNDED products (631);
      * q, k, v of the saved qkv and do = (f dh) Wproj (689);
      * the numerators as in the forward (724, 776), P = numerator / sum kept in fp32 for Sum dP P (734) and for dS;
      * dS = P (dP - Sum dP P) / sqrt(128) (742, 778): the operand of the dq and dk products;
      * P itself (777): the operand of the dv product;
      * dq, dk, dv (751, 792, 793): the operands of the Wqkv GEMM and `dyt_qkv`.
    Not rounded: both LayerNorm backwards (x-hat from the saved h and the saved statistics), the exchanges, dh, every partial sum."""
    r = bf16 if rounded else (lambda x: x)
    h, dh_out = h.double(), dh_out.double()
    M = h.shape[0]
    fa_r, fm_r = _factor_rows(fa, M), _factor_rows(fm, M)
    wqkv, wproj, w1, w2 = r(P["wqkv"]), r(P["wproj"]), r(P["w1"]), r(P["w2"])
    S = {k: v.double() for k, v in (saved if saved is not None else block_forward_model(P, h, fa, rounded)).items()}
    _, (q, k, v, pn, inv) = attention_model(S["qkv"], rounded, internals=True)
    xh1, rstd1 = (h - S["mean_attn"][:, None]) * S["rstd_attn"][:, None], S["rstd_attn"][:, None]
    xh2, rstd2 = (S["h_mlp"] - S["mean_mlp"][:, None]) * S["rstd_mlp"][:, None], S["rstd_mlp"][:, None]

    def ln_backward(dz, xh, rstd, g):
        t = dz * g
        s1, s2 = t.mean(-1, keepdim=True), (t * xh).mean(-1, keepdim=True)
        return (t - s1 - xh * s2) * rstd
    # ---- MLP branch ----
    d2 = fm_r * dh_out
    dpre = (r(d2) @ w2) * gelu_grad64(S["pre"])
    dz2 = r(dpre) @ w1
    dhm = dh_out + ln_backward(dz2, xh2, rstd2, P["g2"])
    # ---- attention branch ----
    d1 = fa_r * dhm
    do = _heads(r(r(d1) @ wproj))
    p = pn * inv
    dP = do @ v.transpose(-1, -2)
    ds = r(p * (dP - (dP * p).sum(-1, keepdim=True)) * SCL)
    dq, dk, dv = r(ds @ k), r(ds.transpose(-1, -2) @ q), r(r(p).transpose(-1, -2) @ do)
    dqkv = torch.cat([_rows(dq), _rows(dk), _rows(dv)], 1)
    dz1 = dqkv @ wqkv
    dh = dhm + ln_backward(dz1, xh1, rstd1, P["g1"])
    part = _part(M // T, h, ln2_g=dz2 * xh2, ln2_b=dz2, fc2_b=d2, fc1_b=dpre, ln1_g=dz1 * xh1, ln1_b=dz1, proj_b=d1)
    return {"dh_in": dh, "dyt_fc2": r(d2), "dyt_fc1": r(dpre), "dyt_proj": r(d1), "dyt_qkv": dqkv, "part": part}


DOWNSTREAM = ("dyt_proj", "dyt_qkv", "dh_in", "ln2_g", "ln2_b", "ln1_g", "ln1_b", "proj_b")       # what the model gates (the rest has closed forms)


def stage_view(res, stage):
    """(tensor, rows, cols) of one DOWNSTREAM stage of a backward result: a `part` segment is sliced per sequence (1 row) x 128 columns."""
    if stage in PART:
        c0, w = PART[stage]
        return res["part"][:, c0:c0 + w], 1, 128
    return res[stage], T, 128


def backward_gates(dev, exact, model):
    """Per DOWNSTREAM stage: (E_model, device vs exact, device vs model, worst device-vs-exact / E_model, worst device-vs-model / E_model), the first
    three as the largest slice, the ratios slice by slice (0 / 0 = 0: a slice that is exactly zero everywhere; where the model rounds nothing - a
    bias partial behind a dropped branch is a plain sum of f dh - E_model is taken as SUM_TOL, the fp32 summation the device still does)."""
    out = {}
    for st in DOWNSTREAM:
        (d, rows, cols), (e, _, _), (m, _, _) = stage_view(dev, st), stage_view(exact, st), stage_view(model, st)
        em, de, dm = slice_errors(m, e, rows, cols), slice_errors(d, e, rows, cols), slice_errors(d, m, rows, cols)
        ratio = lambda a: float(torch.where(a == 0, torch.zeros_like(a), a / em.clamp_min(SUM_TOL)).max())
        out[st] = (float(em.max()), float(de.max()), float(dm.max()), ratio(de), ratio(dm))
    return out


# ---- fp32 restatements of the kernels' scalar code (numpy, for the CPU pins of the caps) ----------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)     # (the product of two floats is exact in double)


def row_stats_restated(h):
    """`row_stats` of syn_kernels.hip in float32, summation order included: rows [R][512] -> (mean, rstd).  A lane (wave, g) of a row sums its 16
    values (columns 64 wave + 16 nf + 4 g + r, nf outer) and fmas their squares, the four g meet by xor 16 then 32, the eight waves pairwise."""
    x = np.asarray(h, np.float32).reshape(-1, 8, 4, 4, 4)            # [row][wave][nf][g][r]
    s = np.zeros(x.shape[:2] + (4,), np.float32)
    q = np.zeros_like(s)
    for nf in range(4):
        for r in range(4):
            v = x[:, :, nf, :, r]
            s = s + v
            q = _fma32(v, v, q)
    tree = lambda a: (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])                        # xor 16: (g0+g1), (g2+g3); xor 32: their sum
    s, q = tree(s), tree(q)                                                                  # [row][wave]
    pair = lambda a: ((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])) + ((a[:, 4] + a[:, 5]) + (a[:, 6] + a[:, 7]))
    S, Q = pair(s), pair(q)
    mean = S * np.float32(1.0 / 512.0)
    var = np.maximum(Q * np.float32(1.0 / 512.0) - mean * mean, np.float32(0))
    return mean, (1.0 / np.sqrt((var + np.float32(1e-5)).astype(np.float64))).astype(np.float32)


def _as_erf_parts(x):
    f = np.float32
    z = np.abs(x) * f(0.70710678118654752440)
    t = (f(1.0) / _fma32(np.full_like(z, f(0.3275911)), z, np.ones_like(z))).astype(np.float32)
    p = _fma32(np.full_like(t, f(1.061405429)), t, np.full_like(t, f(-1.453152027)))
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = _fma32(p, t, np.full_like(t, f(c)))
    e = np.exp2((-z * z * f(1.4426950408889634)).astype(np.float64)).astype(np.float32)
    return _fma32(-p * t, e, np.ones_like(z)), e


def gelu_as(x):
    """`gelu_erf` of syn_kernels.hip (erf by Abramowitz & Stegun 7.1.26) in float32, with exact reciprocal and exp2."""
    x = np.asarray(x, np.float32)
    erf_abs, _ = _as_erf_parts(x)
    return np.float32(0.5) * x * (np.float32(1.0) + np.copysign(erf_abs, x))


def gelu_grad_as(x):
    """`gelu_grad` of syn_stack_train.inc in float32."""
    x = np.asarray(x, np.float32)
    erf_abs, e = _as_erf_parts(x)
    return np.float32(0.5) * (np.float32(1.0) + np.copysign(erf_abs, x)) + x * e * np.float32(0.3989422804014327)


# ---- the gates (one definition, used by the CPU pins and by the GPU test) ---------------------------------------------------------------------------
EPS32 = 2.0 ** -23
GEMM_TOL = 2e-6                    # identical bf16 operands, fp32 against float64 accumulation: the project's GEMM gate
WGRAD_TOL = 3e-6                   # tests/test_gpu_kernels.py::test_linear_pair_on_128_column_shapes
SUM_TOL = 1e-6                     # an fp32 sum of 32 rows against float64
LN_FLIP_SHARE = 4e-4               # share of LayerNorm outputs that may sit one bf16 step off the fp32 formula


def mean_gate(h):
    """|mean error| allowed per row: 4 * 2^-23 * rms(row)."""
    return 4 * EPS32 * h.double().pow(2).mean(-1).sqrt()


def rstd_gate(h):
    """|rstd / rstd64 - 1| allowed per row: 8 * 2^-23 * (1 + mean^2 / var), the conditioning of the one-pass variance E[x^2] - mean^2."""
    return 8 * EPS32 * (1 + row_stats64(h)[2])


def gelu_gate(pre, want):
    """2^-8 |want| (bf16 rounding plus one flip) + 4e-7 max(1, |pre|) (twice the A&S formula's own error, for hardware rcp / exp2)."""
    return 2.0 ** -8 * want.abs() + 4e-7 * pre.double().abs().clamp_min(1.0)


def dgelu_gate(da, want, da_terms, dgelu):
    """2^-8 |want| + 6e-7 |da| (twice the A&S gelu_grad's own absolute error of 2.8e-7) + 2^-23 |gelu'| Sum |terms of da|.
    The last term is the fp32 accumulation of da itself, the GEMM gate (2e-6 of a typical |da| = Sum |terms| / 18 at K = 512) put element by
    element: the first two terms vanish with |da|, and of 4 M sums of 512 signed products about a thousand cancel to below 3e-4 of the typical
    size, where the accumulation's rounding is all there is.  It is 1e-3 of the first term at a typical element."""
    return 2.0 ** -8 * want.abs() + 6e-7 * da.abs() + 2.0 ** -23 * dgelu.abs() * da_terms
