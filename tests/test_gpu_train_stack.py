"""The persistent training kernels of the eight blocks (`syn_train_stack_fwd` / `_bwd` / `_wgrad`, csrc/syn_stack_train.inc) stage by stage: the three
entry points are driven through ctypes the way `training.StackFn` fills their structs, every output is pre-filled with NaN, and every saved tensor,
transposed gradient, partial sum and weight gradient is held against a float64 reference (tests/train_stack_ref.py, on the device) computed from
the kernel's OWN saved input of that stage - so nothing compounds and each gate is that stage's arithmetic, not the 3e-2 of eight blocks.
All figures are per slice (one sequence's 32 rows x 128 columns: what one workgroup produces).  The gates and the caps behind them are pinned on the
CPU in tests/test_train_stack_host.py."""
import ctypes as C
import functools

import pytest
import torch

from tests import outlier_weights as ow
from tests import train_stack_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAVE_F32 = {"h_attn": 512, "mean_attn": 0, "rstd_attn": 0, "qkv": 1536, "h_mlp": 512, "mean_mlp": 0, "rstd_mlp": 0, "pre": 1024}      # name -> columns (0: [M])
SAVE_XT = {"xt_ln1": 512, "xt_attn": 512, "xt_ln2": 512, "xt_gelu": 1024}
DYT = {"dyt_fc2": 512, "dyt_fc1": 1024, "dyt_proj": 512, "dyt_qkv": 1536}
DW = {"dw_fc2": (512, 1024), "dw_fc1": (1024, 512), "dw_proj": (512, 512), "dw_qkv": (1536, 512)}
DSMALL = {"d_ln2_g": "ln2_g", "d_ln2_b": "ln2_b", "d_fc2_b": "fc2_b", "d_fc1_b": "fc1_b", "d_ln1_g": "ln1_g", "d_ln1_b": "ln1_b", "d_proj_b": "proj_b"}
WEIGHTS = (("wqkv", "w_qkv"), ("wproj", "w_proj"), ("w1", "w_fc1"), ("w2", "w_fc2"))
VECS = (("g1", "ln1_g"), ("b1", "ln1_b"), ("bproj", "b_proj"), ("g2", "ln2_g"), ("b2", "ln2_b"), ("bfc1", "b_fc1"), ("bfc2", "b_fc2"))


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


@functools.lru_cache(maxsize=None)
def _weights(case):
    """Per block: fp32 parameters on the device, their float64 copies with the matrices rounded to bf16 (what the fragment sets hold), and the
    packed fragment sets (W, W^T) made the way `training.StackFn` gets them."""
    from syntalker_amd import training
    sd = R.state_dict(case)
    p32 = [{k: v.contiguous() for k, v in R.block_params(sd, l, DEV, torch.float32).items()} for l in range(R.LAYERS)]
    p64 = [{k: (R.bf16(v) if v.dim() == 2 else v.double()) for k, v in p.items()} for p in p32]
    exact = [{k: v.double() for k, v in p.items()} for p in p32]
    packs = [{k: training._packs_of(p[k]) for k, _ in WEIGHTS} for p in p32]
    return p32, p64, exact, packs


class Stack:
    """One `syn_train_stack` with everything it points to; `forward()` launches it."""

    def __init__(self, case, n_seq, drop):
        from syntalker_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.case, self.n, self.M = case, n_seq, 32 * n_seq
        self.p32, self.p64, self.exact, self.packs = _weights(case)
        self.h_in = R.h0(n_seq).to(DEV).reshape(self.M, 512).contiguous()
        self.dp = R.drop_path_table(n_seq).to(DEV).contiguous() if drop else None
        self.h_out = _nan(self.M, 512)
        self.sync = torch.zeros(320, dtype=torch.int32, device=DEV)
        self.xch = _nan(n_seq, 8, 32 * 512)
        self.saves = []
        a = self.a = _lib.SynTrainStack()
        a.h_in, a.h_out, a.n_seq, a.drop_path = self.h_in.data_ptr(), self.h_out.data_ptr(), n_seq, _lib.ptr(self.dp)
        a.sync, a.xch = self.sync.data_ptr(), self.xch.data_ptr()
        for l in range(R.LAYERS):
            for k, f in VECS:
                setattr(a.layer[l], f, self.p32[l][k].data_ptr())
            for k, f in WEIGHTS:
                setattr(a.layer[l], f, self.packs[l][k][0].data_ptr())
            sv = {k: (_nan(self.M, c) if c else _nan(self.M)) for k, c in SAVE_F32.items()}
            sv.update({k: torch.full((c * self.M * 2,), 255, dtype=torch.uint8, device=DEV) for k, c in SAVE_XT.items()})      # 0xFFFF: a bf16 NaN
            for k, v in sv.items():
                setattr(a.save[l], k, v.data_ptr())
            self.saves.append(sv)

    def stream(self):
        return self._lib.current_stream(torch.device(DEV))

    def forward(self):
        self._lib.check(self.lib.syn_train_stack_fwd(C.byref(self.a), self.stream()), "syn_train_stack_fwd")
        torch.cuda.synchronize()
        return self

    def factors(self, l):
        """(fa, fm) [n_seq] of block l, fp32 on the device."""
        one = torch.ones(self.n, device=DEV)
        return (one, one) if self.dp is None else (self.dp[2 * l], self.dp[2 * l + 1])

    def rows(self, f):
        return f.reshape(-1, 1).expand(self.n, 32).reshape(self.M, 1)

    def xt(self, l, name):
        return R.unpack_xt(self.saves[l][name], SAVE_XT[name], self.M)

    def sync_is_zero(self):
        return not bool(self.sync.any())


class Grad:
    """One `syn_train_stack_grad` on a Stack, every output NaN."""

    def __init__(self, s, dh_out):
        self.s = s
        g = self.g = s._lib.SynTrainStackGrad()
        g.fwd = C.pointer(s.a)
        self.dh_out, self.dh_in, self.stash = dh_out.contiguous(), _nan(s.M, 512), _nan(s.n, 4, 32 * 512)
        g.dh_out, g.dh_in, g.stash = self.dh_out.data_ptr(), self.dh_in.data_ptr(), self.stash.data_ptr()
        self.out = []
        for l in range(R.LAYERS):
            for k, f in WEIGHTS:
                setattr(g.layer_t[l], f, s.packs[l][k][1].data_ptr())
            g.layer_t[l].ln1_g, g.layer_t[l].ln2_g = s.p32[l]["g1"].data_ptr(), s.p32[l]["g2"].data_ptr()
            t = {k: _nan(c, s.M, dtype=torch.bfloat16) for k, c in DYT.items()}
            t["part"] = _nan(s.n, R.PART_COLS)
            t.update({k: _nan(*shp) for k, shp in DW.items()})
            t.update({k: _nan(R.PART[seg][1]) for k, seg in DSMALL.items()})
            for k, v in t.items():
                setattr(g.grad[l], k, v.data_ptr())
            self.out.append(t)

    def refill(self):
        self.dh_in.fill_(float("nan"))
        for t in self.out:
            for v in t.values():
                v.fill_(float("nan"))

    def backward(self, first, last, dh_out=None, dh_in=None):
        g, s = self.g, self.s
        g.first_block, g.last_block = first, last
        g.dh_out = (self.dh_out if dh_out is None else dh_out).data_ptr()
        g.dh_in = (self.dh_in if dh_in is None else dh_in).data_ptr()
        s._lib.check(s.lib.syn_train_stack_bwd(C.byref(g), s.stream()), "syn_train_stack_bwd")
        torch.cuda.synchronize()

    def wgrad(self, first, last):
        g, s = self.g, self.s
        g.first_block, g.last_block = first, last
        s._lib.check(s.lib.syn_train_stack_wgrad(C.byref(g), s.stream()), "syn_train_stack_wgrad")
        torch.cuda.synchronize()

    def device_result(self, l):
        """Block l's outputs in the reference's form ([M][features], float64)."""
        t = self.out[l]
        res = {k: t[k].T.double() for k in DYT}
        res["dh_in"], res["part"] = self.dh_in.double(), t["part"].double()
        return res


@functools.lru_cache(maxsize=None)
def _forward(case, n_seq, drop):
    return Stack(case, n_seq, drop).forward()


def _dh_out(s, seed, zero_seq=None):
    d = torch.randn(s.M, 512, generator=torch.Generator().manual_seed(seed)).to(DEV)
    if zero_seq is not None:
        d[32 * zero_seq:32 * (zero_seq + 1)] = 0
    return d


def test_unpack_xt_inverts_the_library_pack():
    from syntalker_amd import training
    for Fd, M in ((512, 128), (1024, 32 * 9)):
        X = torch.randn(M, Fd, generator=torch.Generator().manual_seed(Fd + M)).to(DEV).bfloat16()
        assert torch.equal(R.unpack_xt(training._pack_t(X, Fd, M), Fd, M), X)


# ---- forward --------------------------------------------------------------------------------------------------------------------------------------
FWD_CASES = [("plain", n, drop) for n in (1, 4, 9, 12, 64) for drop in (False, True)] + [(c, 4, False) for c in ow.CASES]


@pytest.mark.parametrize("case,n_seq,drop", FWD_CASES)
def test_forward_every_saved_tensor_of_every_block(case, n_seq, drop):
    """Per block: (1) h_attn is bitwise the previous residual; (2) mean / rstd against float64 statistics of the saved h; (3) the LayerNorm operands
    against the fp32 formula on the saved statistics; (4) qkv, pre and (5) both residuals against float64 products of the kernel's own saved bf16
    operands; (6) the GELU operand against float64 gelu of the saved pre; (7) the attention operand against float64 attention of the saved qkv,
    within twice the distance of the kernel's rounding model from it; (8) sync zero, no NaN sentinel left."""
    s = _forward(case, n_seq, drop)
    M, fails, worst = s.M, [], {}

    def gate(stage, l, value, bound):
        worst[stage] = max(worst.get(stage, 0.0), value / bound)
        if not value <= bound:
            fails.append(f"block {l} {stage}: {value:.3e} > {bound:.3e}")
    model_dist = 0.0
    prev = s.h_in
    for l in range(R.LAYERS):
        sv, P = s.saves[l], s.p64[l]
        fa, fm = (s.rows(f).double() for f in s.factors(l))
        if not _same_bits(sv["h_attn"], prev):
            fails.append(f"block {l}: h_attn is not bitwise the previous residual")
        for br, (g, b) in (("attn", ("g1", "b1")), ("mlp", ("g2", "b2"))):
            h, mean, rstd = sv[f"h_{br}"], sv[f"mean_{br}"], sv[f"rstd_{br}"]
            m64, r64, _ = R.row_stats64(h)
            gate(f"mean_{br}", l, float(((mean.double() - m64).abs() / R.mean_gate(h)).max()), 1.0)
            gate(f"rstd_{br}", l, float(((rstd.double() / r64 - 1).abs() / R.rstd_gate(h)).max()), 1.0)
            share, steps = R.layer_norm_bf16_check(s.xt(l, "xt_ln1" if br == "attn" else "xt_ln2"), h, mean, rstd, s.p32[l][g], s.p32[l][b])
            gate(f"ln_{br} share", l, share, R.LN_FLIP_SHARE)
            gate(f"ln_{br} steps", l, steps, 1.0)
        x1, xo, x2, xa = (s.xt(l, k).double() for k in ("xt_ln1", "xt_attn", "xt_ln2", "xt_gelu"))
        gate("qkv", l, R.sliced_rel_l2(sv["qkv"], x1 @ P["wqkv"].T), R.GEMM_TOL)
        gate("pre", l, R.sliced_rel_l2(sv["pre"], x2 @ P["w1"].T + P["bfc1"]), R.GEMM_TOL)
        nxt = s.saves[l + 1]["h_attn"] if l + 1 < R.LAYERS else s.h_out
        # the residuals, on the branch term: a branch with factor 0 is a slice that must be exactly zero, i.e. the residual bitwise its input
        gate("h_mlp", l, R.sliced_rel_l2(sv["h_mlp"].double() - sv["h_attn"].double(), fa * (xo @ P["wproj"].T + P["bproj"])), R.GEMM_TOL)
        gate("h_next", l, R.sliced_rel_l2(nxt.double() - sv["h_mlp"].double(), fm * (xa @ P["w2"].T + P["bfc2"])), R.GEMM_TOL)
        pre = sv["pre"].double()
        want = R.gelu64(pre)
        gate("gelu", l, float(((xa - want).abs() / R.gelu_gate(pre, want)).max()), 1.0)
        if case == "gelu" and l in (1, 4, 6):
            assert float(pre.abs().max()) > 10.5 and int((pre.abs() > 10.5).sum()) >= 900 * n_seq, (l, float(pre.abs().max()))
        exact, model = R.attention_exact(sv["qkv"]), R.attention_model(sv["qkv"])
        E = R.slice_errors(model, exact)
        gate("attention / 2E", l, float((R.slice_errors(xo, exact) / E).max()), 2.0)
        model_dist = max(model_dist, R.sliced_rel_l2(xo, model))
        prev = nxt
    print(f"forward {case} n_seq {n_seq} DropPath {drop}: worst share of each gate: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; attention operand against its rounding model {model_dist:.2e}")
    if drop:        # the dropped branches left the residual bitwise alone
        s0, s1, s2 = (min(i, n_seq - 1) for i in range(3))
        rows = lambda t, q: t[32 * q:32 * (q + 1)]
        assert _same_bits(rows(s.saves[R.DROP_BOTH]["h_mlp"], s0), rows(s.saves[R.DROP_BOTH]["h_attn"], s0))
        assert _same_bits(rows(s.saves[R.DROP_BOTH + 1]["h_attn"], s0), rows(s.saves[R.DROP_BOTH]["h_attn"], s0))
        assert _same_bits(rows(s.saves[R.DROP_ATTN]["h_mlp"], s1), rows(s.saves[R.DROP_ATTN]["h_attn"], s1))
        assert _same_bits(rows(s.saves[R.DROP_MLP + 1]["h_attn"], s2), rows(s.saves[R.DROP_MLP]["h_mlp"], s2))
    assert s.sync_is_zero(), s.sync.nonzero().flatten().tolist()
    assert not bool(torch.isnan(s.h_out).any())
    for l, sv in enumerate(s.saves):
        for k, v in sv.items():
            assert not bool(torch.isnan(v.view(torch.bfloat16) if k in SAVE_XT else v).any()), (l, k)
    assert not fails, "\n".join(fails)


# ---- backward -------------------------------------------------------------------------------------------------------------------------------------
BWD_BLOCKS = {"plain": (7, 3, 0), "gelu": (1, 4, 6), "sharp": (2, 5), "massive": (0, 1), "shifted": (0, 1)}
N_BWD, ZERO_SEQ = 4, 3


@pytest.mark.parametrize("case", R.CASES)
def test_backward_one_block_at_a_time(case):
    """`syn_train_stack_bwd` with first_block = last_block = l on a random dh_out whose last sequence is zero, from the saved tensors of the forward
    (plain: with the DropPath table - block 3 is the one whose MLP branch sequence 2 lost).  dyt_fc2, dyt_fc1 and the two bias partials have closed
    forms; everything downstream is held against float64 autograd from the saved h_attn[l] (within 2 E_model) and against the rounding model
    fed with the forward's saved tensors, as the kernel is (within E_model / 4).  The three figures of a stage are `sliced_rel_l2` values (the worst
    slice of each); device-vs-exact is also held to 2 E_model slice by slice.

    Measured on an MI355X, worst block of each case, as E_model | device-vs-exact | device-vs-model:
      stage      plain                     gelu                      sharp                     massive                   shifted
      dyt_proj   3.1e-3 3.1e-3 1.9e-4     2.5e-3 2.5e-3 2.4e-4     3.4e-3 3.4e-3 2.3e-4     1.7e-3 1.7e-3 6.7e-5     2.5e-3 2.5e-3 5.6e-5
      dyt_qkv    7.6e-3 7.6e-3 1.5e-3     1.2e-2 1.3e-2 2.9e-3     7.1e-2 7.1e-2 3.2e-3     7.4e-3 7.4e-3 4.0e-4     8.1e-3 8.1e-3 1.6e-3
      dh_in      4.0e-3 4.0e-3 3.7e-4     2.9e-3 2.9e-3 3.2e-4     4.1e-2 4.1e-2 1.3e-3     2.7e-3 2.7e-3 1.1e-4     3.4e-3 3.4e-3 2.8e-4
      ln2_g      4.9e-3 4.9e-3 5.1e-5     4.8e-3 4.8e-3 2.7e-5     1.3e-2 1.3e-2 5.8e-5     8.5e-3 8.5e-3 1.0e-4     5.0e-3 5.0e-3 1.5e-5
      ln2_b      4.3e-3 4.3e-3 4.8e-5     4.5e-3 4.5e-3 2.4e-5     8.9e-3 8.9e-3 5.4e-5     4.1e-3 4.1e-3 9.3e-5     4.7e-3 4.7e-3 1.2e-5
      ln1_g      7.3e-3 7.4e-3 8.2e-4     6.9e-3 6.9e-3 8.5e-4     5.5e-2 5.5e-2 1.8e-3     7.6e-3 7.6e-3 3.1e-4     7.3e-3 7.3e-3 7.1e-4
      ln1_b      4.6e-3 4.7e-3 4.3e-4     5.1e-3 5.1e-3 5.0e-4     4.9e-2 4.9e-2 2.3e-3     4.2e-3 4.2e-3 1.6e-4     5.2e-3 5.2e-3 4.5e-4
      proj_b     1.7e-3 1.7e-3 1.7e-5     1.1e-3 1.1e-3 6.1e-6     3.2e-3 3.2e-3 2.0e-5     3.1e-4 3.1e-4 8.2e-6     2.2e-3 2.2e-3 5.7e-6
    The MLP stages sit 100 x below E_model, dyt_proj 10 - 40 x, dyt_qkv only 4 - 20 x (0.23 E_model for gelu block 6): it lies behind four bf16
    roundings in a row (f dh, do, dS, dq / dk / dv), and a rounding decided the other way is a full bf16 step, so each of them multiplies what the
    fp32 arithmetic before it differs by.  One float32 rounding (6e-8) of noise on the model's own inputs moves its dyt_qkv by 0.2 E_model on the CPU.
    A model that recomputes qkv / pre / the statistics from h instead of taking the saved ones misses the gate (0.3 - 0.9 E_model on every
    stage of the shifted stream): the backward kernel reads the forward's roundings, so the model has to."""
    s = _forward(case, N_BWD, case == "plain")
    gr = Grad(s, _dh_out(s, 21, ZERO_SEQ))
    fails = []
    for l in BWD_BLOCKS[case]:
        gr.refill()
        gr.backward(l, l)
        assert s.sync_is_zero()
        sv, P, t = s.saves[l], s.p64[l], gr.out[l]
        fa, fm = s.factors(l)
        dev = gr.device_result(l)
        for k, v in dev.items():
            assert not bool(torch.isnan(v).any()), (l, k)
        for other in range(R.LAYERS):
            if other != l:
                assert all(bool(torch.isnan(v).all()) for v in gr.out[other].values()), (l, other)       # no other block's buffers were touched
        # ---- closed forms
        d2 = gr.dh_out * s.rows(fm)                                   # fp32, as the kernel multiplies
        assert _same_bits(t["dyt_fc2"], d2.bfloat16().T.contiguous()), l
        c0, w = R.PART["fc2_b"]
        sums = lambda x: x.double().reshape(s.n, 32, -1).sum(1)
        e = float(((dev["part"][:, c0:c0 + w] - sums(d2)).abs() / (1e-6 * sums(d2.abs())).clamp_min(1e-300)).max())
        print(f"backward {case} block {l}: fc2-bias partial, worst share of 1e-6 {e:.3f}")
        if not e <= 1.0:
            fails.append(f"block {l} fc2-bias partial {e:.3f} of its gate")
        da, dg = dev["dyt_fc2"] @ P["w2"], R.gelu_grad64(sv["pre"].double())
        want = da * dg
        e = float(((dev["dyt_fc1"] - want).abs() / R.dgelu_gate(da, want, dev["dyt_fc2"].abs() @ P["w2"].abs(), dg).clamp_min(1e-300)).max())
        c0, w = R.PART["fc1_b"]
        eb = float(((dev["part"][:, c0:c0 + w] - sums(want)).abs() / (2.0 ** -8 * sums(want).abs() + 6e-7 * sums(da.abs())).clamp_min(1e-300)).max())
        print(f"backward {case} block {l}: dyt_fc1 worst share of its gate {e:.3f}, fc1-bias partial {eb:.3f}")
        if not (e <= 1.0 and eb <= 1.0):
            fails.append(f"block {l} dyt_fc1 {e:.3f} / fc1-bias partial {eb:.3f} of their gates")
        # ---- downstream: exact, model, device
        h = sv["h_attn"].double()
        exact = R.block_backward_exact(s.exact[l], h, gr.dh_out, fa, fm)
        model = R.block_backward_model(s.exact[l], h, gr.dh_out, fa, fm, saved={k: sv[k] for k in R.SAVED})      # what the kernel read
        for st, (em, de, dm, r_exact, r_model) in R.backward_gates(dev, exact, model).items():
            print(f"TABLE {case} block {l} {st}: E_model {em:.2e} device-vs-exact {de:.2e} device-vs-model {dm:.2e} (worst slice: {r_exact:.2f} E, {r_model:.3f} E)")
            floor = max(em, R.SUM_TOL)
            if not (de <= 2 * floor and dm <= floor / 4 and r_exact <= 2.0):
                fails.append(f"block {l} {st}: E_model {em:.2e}, device-vs-exact {de:.2e} (gate 2 E; slice by slice {r_exact:.2f} E), "
                             f"device-vs-model {dm:.2e} (gate E / 4)")
        # ---- the sequence without an output gradient: exactly nothing
        z = slice(32 * ZERO_SEQ, 32 * (ZERO_SEQ + 1))
        assert not bool(gr.dh_in[z].any()) and not bool(t["part"][ZERO_SEQ].any()) and all(not bool(t[k][:, z].any()) for k in DYT), l
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n_seq", [4, 12])
def test_backward_chain_cut_in_pieces_is_the_one_launch_bitwise(n_seq):
    s = _forward("plain", n_seq, True)
    gr = Grad(s, _dh_out(s, 22))
    gr.backward(7, 0)
    whole = (gr.dh_in.clone(), [{k: t[k].clone() for k in (*DYT, "part")} for t in gr.out])
    gr.refill()
    mid = _nan(s.M, 512)
    gr.backward(7, 4, dh_in=mid)
    assert bool(torch.isnan(gr.dh_in).all()) and all(bool(torch.isnan(gr.out[l]["part"]).all()) for l in range(4))
    gr.backward(3, 0, dh_out=mid)
    assert s.sync_is_zero() and not bool(torch.isnan(gr.dh_in).any())
    assert _same_bits(gr.dh_in, whole[0])
    for l in range(R.LAYERS):
        for k in (*DYT, "part"):
            assert _same_bits(gr.out[l][k], whole[1][l][k]), (l, k)


# ---- weight gradients -----------------------------------------------------------------------------------------------------------------------------
XT_OF = {"dw_fc2": ("dyt_fc2", "xt_gelu"), "dw_fc1": ("dyt_fc1", "xt_ln2"), "dw_proj": ("dyt_proj", "xt_attn"), "dw_qkv": ("dyt_qkv", "xt_ln1")}


@pytest.mark.parametrize("n_seq", [4, 12, 64])
def test_weight_gradients_against_the_kernels_own_operands(n_seq):
    """dW = dyt . unpack(xt) of the same run in float64 (rel-L2 3e-6: identical bf16 operands), the seven small gradients against the in-order fp32
    sum of `part` over the sequences (1e-6)."""
    s = _forward("plain", n_seq, True)
    gr = Grad(s, _dh_out(s, 23))
    gr.backward(7, 0)
    gr.wgrad(7, 0)
    assert s.sync_is_zero()
    worst_w = worst_s = 0.0
    for l in range(R.LAYERS):
        t = gr.out[l]
        for k, (dy, xt) in XT_OF.items():
            want = t[dy].double() @ s.xt(l, xt).double()
            worst_w = max(worst_w, float((t[k].double() - want).norm() / want.norm()))
        acc = torch.zeros(R.PART_COLS, device=DEV)
        for q in range(n_seq):
            acc = acc + t["part"][q]                                  # fp32, in sequence order, as k_part_sums adds
        for k, seg in DSMALL.items():
            c0, w = R.PART[seg]
            want = acc[c0:c0 + w].double()
            worst_s = max(worst_s, float((t[k].double() - want).norm() / want.norm()))
    print(f"weight gradients, n_seq {n_seq}: worst dW rel-L2 {worst_w:.2e}, worst small gradient {worst_s:.2e}")
    assert worst_w <= R.WGRAD_TOL and worst_s <= 1e-6


def test_weight_gradients_of_a_block_range_leave_the_other_blocks_alone():
    s = _forward("plain", 4, True)
    gr = Grad(s, _dh_out(s, 24))
    gr.backward(7, 0)
    gr.wgrad(5, 2)
    for l in range(R.LAYERS):
        for k in (*DW, *DSMALL):
            v = gr.out[l][k]
            assert bool(torch.isnan(v).all()) if (l < 2 or l > 5) else not bool(torch.isnan(v).any()), (l, k)
    t = gr.out[4]
    want = t["dyt_qkv"].double() @ s.xt(4, "xt_ln1").double()
    assert float((t["dw_qkv"].double() - want).norm() / want.norm()) <= R.WGRAD_TOL


# ---- argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_argument_checks():
    """Every refused call returns non-zero with a message and launches nothing: all outputs keep their NaN fill, sync stays zero."""
    s = Stack("plain", 4, True)                                     # never launched
    gr = Grad(s, _dh_out(s, 25))
    lib, st = s.lib, s.stream()

    def refused(rc, word):
        assert rc != 0 and word in lib.syn_last_error().decode(), (rc, word, lib.syn_last_error())

    def fwd(**edit):
        a = type(s.a).from_buffer_copy(s.a)
        for k, v in edit.items():
            o, f = (a, k) if "." not in k else (getattr(a, k.split(".")[0])[5], k.split(".")[1])
            setattr(o, f, v)
        return a

    def grad(a=None, **edit):
        g = type(gr.g).from_buffer_copy(gr.g)
        g.fwd = C.pointer(s.a if a is None else a)
        g.first_block, g.last_block = 7, 0
        for k, v in edit.items():
            o, f = (g, k) if "." not in k else (getattr(g, k.split(".")[0])[5], k.split(".")[1])
            setattr(o, f, v)
        return g
    keep = []

    def call(fn, struct):
        keep.append(struct)
        return fn(C.byref(struct), st)
    # forward
    for n in (0, 65, -4):
        refused(call(lib.syn_train_stack_fwd, fwd(n_seq=n)), "1 .. 64")
    for f in ("h_in", "h_out", "sync", "xch"):
        refused(call(lib.syn_train_stack_fwd, fwd(**{f: None})), "non-null")
    refused(lib.syn_train_stack_fwd(None, st), "non-null")
    for f in ("ln1_g", "ln1_b", "w_qkv", "w_proj", "b_proj", "ln2_g", "ln2_b", "w_fc1", "b_fc1", "w_fc2", "b_fc2"):
        refused(call(lib.syn_train_stack_fwd, fwd(**{"layer." + f: None})), "weights are incomplete")
    for f in (*SAVE_F32, *SAVE_XT):
        refused(call(lib.syn_train_stack_fwd, fwd(**{"save." + f: None})), "saved tensors are incomplete")
    # backward
    refused(lib.syn_train_stack_bwd(None, st), "null")
    for f in ("dh_out", "dh_in", "stash"):
        refused(call(lib.syn_train_stack_bwd, grad(**{f: None})), "null")
    g = grad()
    g.fwd = None
    refused(call(lib.syn_train_stack_bwd, g), "null")
    for n in (0, 65):
        a = fwd(n_seq=n)
        keep.append(a)
        refused(call(lib.syn_train_stack_bwd, grad(a)), "1 .. 64")
    for f in ("sync", "xch"):
        a = fwd(**{f: None})
        keep.append(a)
        refused(call(lib.syn_train_stack_bwd, grad(a)), "sync / xch")
    for first, last in ((3, 4), (0, 7), (3, -1), (-1, -1), (8, 0), (8, 8)):
        refused(call(lib.syn_train_stack_bwd, grad(first_block=first, last_block=last)), "first_block >= last_block")
        refused(call(lib.syn_train_stack_wgrad, grad(first_block=first, last_block=last)), "first_block >= last_block")
    for f in ("ln1_g", "w_qkv", "w_proj", "ln2_g", "w_fc1", "w_fc2"):
        refused(call(lib.syn_train_stack_bwd, grad(**{"layer_t." + f: None})), "transposed weights")
    for f in (*DYT, "part"):
        refused(call(lib.syn_train_stack_bwd, grad(**{"grad." + f: None})), "outputs are incomplete")
    # weight gradients
    refused(lib.syn_train_stack_wgrad(None, st), "null")
    g = grad()
    g.fwd = None
    refused(call(lib.syn_train_stack_wgrad, g), "null")
    for n in (0, 65, 6, 1, 9):
        a = fwd(n_seq=n)
        keep.append(a)
        refused(call(lib.syn_train_stack_wgrad, grad(a)), "multiple of 128")
    for f in (*DW, *DSMALL):
        refused(call(lib.syn_train_stack_wgrad, grad(**{"grad." + f: None})), "gradient buffers are incomplete")
    torch.cuda.synchronize()
    assert s.sync_is_zero()
    assert bool(torch.isnan(s.h_out).all()) and bool(torch.isnan(gr.dh_in).all()) and bool(torch.isnan(s.xch).all()) and bool(torch.isnan(gr.stash).all())
    for sv in s.saves:
        assert all(bool(torch.isnan(v.view(torch.bfloat16) if k in SAVE_XT else v).all()) for k, v in sv.items())
    for t in gr.out:
        assert all(bool(torch.isnan(v).all()) for v in t.values())
