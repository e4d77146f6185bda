"""The kernels of csrc/syn_rvq_train.inc one at a time, through the C ABI, against fp64 or - where a kernel's result is a single rounding - bit
for bit.  tests/test_gpu_rvq_train.py judges these kernels only through whole-step gradients at 3e-2 rel-L2; their operands are exact bf16 or
their result is one rounding, so each is held here to a bound thousands of times tighter:
  k_wgrad / k_colsum   |got - want| <= 2 K 2^-24 sum |dy x| per element (products of bf16 are exact in fp32, K u bounds any order of the sum, the
                       factor 2 leaves room for the matrix unit's internal order), on every geometry the trainer issues (ref.WGRAD_CASES)
  k_pack_jobs, k_ew, k_cast_pad, k_pairsum, k_stuff        bit for bit
  k_recons             gradient rows = the bf16 rounding of the fp64 value, parts within K u of fp64
  k_scalars            1e-6 relative
and the argument checks of the entry points refuse what they say they refuse.  What wrong kernels these comparisons would catch is shown on the
CPU, by tests/test_rvq_train_host.py; measured values: DESIGN.md 16.5."""
import numpy as np
import pytest
import torch

from syntalker_amd import _lib
from syntalker_amd.rvqvae import _up
from tests import rvq_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(fn, *args):
    """One entry point on the current stream, checked, and waited for; tensors are passed as their device pointers (and stay referenced until
    the kernel is done)."""
    _lib.check(fn(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], _lib.current_stream()), fn.__name__)
    torch.cuda.synchronize()


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def guarded(n, dtype, fill):
    """A device buffer of n elements and 64 more behind it that no kernel may touch."""
    return torch.full((n + 64,), fill, dtype=dtype, device=DEV)


def guard_intact(buf, n, fill):
    return bool((buf[n:].float().cpu() == fill).all())


# ---- C1. the weight gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.WGRAD_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[3]}-{c[5]}x{c[6]}")
def test_wgrad_against_fp64(lib, case):
    geo, cout, ldy, cin, ldx, clips, t_out = case
    taps, stride, dil, pad, up, relu_in = ref.WGRAD_GEOMETRY[geo]
    dy, x, t_in = ref.wgrad_operands(case)
    k = clips * t_out
    dw, db = guarded(cout * cin * taps, torch.float32, 7.0), guarded(cout, torch.float32, 7.0)
    call(lib.syn_vq_train_wgrad, dy.to(BF).to(DEV), ldy, x.to(BF).to(DEV), ldx, dw, db, clips, t_in, t_out,
         cout, cin, taps, stride, dil, pad, up, relu_in)
    assert guard_intact(dw, cout * cin * taps, 7.0) and guard_intact(db, cout, 7.0)
    want, mag, want_b, mag_b = ref.wgrad_ref(dy[..., :cout], x[..., :cin], taps, stride, dil, pad, up, relu_in)
    err = (dw[:cout * cin * taps].cpu().double().view(cout, cin, taps) - want).abs()
    err_b = (db[:cout].cpu().double() - want_b).abs()
    bound, bound_b = ref.wgrad_bound(mag, k), ref.wgrad_bound(mag_b, k)
    live = bound > 0
    print(f"{case}: K {k}, worst error / bound: dW {float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0:.4f}, "
          f"db {float((err_b / bound_b).max()):.4f}; elements with a zero bound {int((~live).sum())}")
    assert bool((err <= bound).all()) and bool((err_b <= bound_b).all())
    if geo == "dil9" and t_out == 1:                                      # one-frame clips: both off-centre taps read padding, never the neighbouring clip
        assert int((~live).sum()) >= 2 * cout * cin and float(dw[:cout * cin * taps].view(cout, cin, taps)[:, :, [0, 2]].abs().max()) == 0.0


# ---- C2. fragment packing --------------------------------------------------------------------------------------------------------------------
def fragments(w, cout_p, cin_p, kind):
    """include/syn_hip.h, syn_vq_train_pack: [tap][cout_p / 16][cin_p / 32][lane = 16 g + r][8] with co = 16 f + r, ci = 32 ks + 8 g + e; kind 1 is the
    tap-flipped transpose W'[ci][co][taps - 1 - tap] = W[co][ci][tap], kind 3 the remainder bf16(w - float(bf16(w))); zero in every padded lane."""
    src = w.permute(1, 0, 2).flip(-1) if kind == 1 else w
    if kind == 3:
        src = src - src.to(BF).float()
    taps = w.shape[2]
    full = torch.zeros(cout_p, cin_p, taps)
    full[:src.shape[0], :src.shape[1]] = src
    fr = full.permute(2, 0, 1).reshape(taps, cout_p // 16, 16, cin_p // 32, 4, 8)       # tap, f, r, ks, g, e
    return fr.permute(0, 1, 3, 4, 2, 5).reshape(taps, cout_p // 16, cin_p // 32, 64, 8).to(BF)


def test_pack_jobs_write_the_documented_layout(lib):
    g = torch.Generator().manual_seed(5)
    jobs, want, keep, max_units = [], [], [], 0
    for cout, cin, taps in ((512, 57, 3), (57, 512, 3), (512, 512, 4)):
        w, bias = torch.randn(cout, cin, taps, generator=g), torch.randn(cout, generator=g)
        wd, bd = w.to(DEV), bias.to(DEV)
        keep += [wd, bd]
        for kind, cout_p, cin_p in ((0, _up(cout, 128), _up(cin, 32)), (3, _up(cout, 128), _up(cin, 32)), (1, _up(cin, 128), _up(cout, 32))):
            ref_frag = fragments(w, cout_p, cin_p, kind)
            out = guarded(ref_frag.numel(), BF, 3.0)
            jobs.append((wd.data_ptr(), out.data_ptr(), cout, cin, taps, cout_p, cin_p, kind))
            want.append((out, ref_frag.reshape(-1), (cout, cin, taps, kind)))
            max_units = max(max_units, ref_frag.numel() // 8)
        cout_p = _up(cout, 128)
        out = guarded(cout_p, torch.float32, 3.0)
        jobs.append((bd.data_ptr(), out.data_ptr(), cout, 0, 0, cout_p, 0, 2))
        want.append((out, torch.cat([bias, torch.zeros(cout_p - cout)]), (cout, 0, 0, 2)))
    table = (_lib.SynVqTrainPackJob * len(jobs))(*[_lib.SynVqTrainPackJob(*j) for j in jobs])
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    call(lib.syn_vq_train_pack, table_dev, len(jobs), max_units)
    for out, expect, what in want:
        n = expect.numel()
        assert guard_intact(out, n, 3.0), what
        assert torch.equal(bits(out[:n]), bits(expect)), what
    assert any(bool((e == 0).any()) for _, e, w_ in want if w_[3] != 2)   # padded lanes exist in this table


# ---- C3. the element-wise kernel --------------------------------------------------------------------------------------------------------------
def ew_ref(v, resid, relu_src, keep, sv, sr, lo_relu):
    """out = sr * resid + sv * [relu_src > 0] * keep * v in fp32 with one multiply and one add, each rounded, as k_ew pins them."""
    x = v.clone()
    if relu_src is not None:
        x = torch.where(relu_src.float() > 0, x, torch.zeros(()))
    if keep is not None:
        x = torch.where(keep != 0, x, torch.zeros(()))
    x = torch.tensor(sv, dtype=torch.float32) * x
    if resid is not None:
        x = torch.tensor(sr, dtype=torch.float32) * resid + x
    hi = x.to(BF)
    lo = x - hi.float()
    if lo_relu:
        lo = torch.where(hi.float() > 0, lo, torch.zeros(()))
    return x, hi, lo.to(BF)


# (resid, relu_src, keep, sv, sr, out_f, out_b, out_lo, lo_relu): every combination RVQTrainer.forward_backward issues; out_f is the resid buffer
# itself wherever resid and out_f are both given, as in the trainer
EW_COMBOS = [(0, 0, 0, 1.0, 1.0, 0, 1, 1, 0), (0, 0, 0, 1.0, 1.0, 0, 1, 1, 1), (0, 0, 0, 1.0, 1.0, 1, 1, 1, 1), (1, 0, 1, 1.25, 1.0, 1, 1, 1, 1),
             (1, 0, 1, 1.25, 1.0, 1, 1, 1, 0), (0, 0, 1, 1.25, 1.0, 0, 1, 0, 0), (0, 1, 0, 1.0, 1.0, 0, 1, 0, 0), (1, 1, 0, 1.0, 1.0, 1, 1, 0, 0),
             (1, 0, 0, 6.0, 0.02 * 2.0 / (6 * 2048 * 512), 0, 1, 0, 0)]


@pytest.mark.parametrize("n", [4, 1020, 1024, 1028])
def test_ew_bit_for_bit(lib, n):
    g = torch.Generator().manual_seed(n)
    for combo in EW_COMBOS:
        has_r, has_m, has_k, sv, sr, has_f, has_b, has_lo, lo_relu = combo
        v, resid = torch.randn(n, generator=g), torch.randn(n, generator=g) * (1e4 if sr < 1e-3 else 1.0)
        relu_src = torch.randn(n, generator=g).to(BF)
        relu_src[0], relu_src[1], relu_src[2], relu_src[3] = 0.0, -0.0, -1.0, 0.5
        keep = (torch.rand(n, generator=g) >= 0.2).to(torch.uint8)
        want_f, want_b, want_lo = ew_ref(v, resid if has_r else None, relu_src if has_m else None, keep if has_k else None, sv, sr, lo_relu)
        resid_d = guarded(n, torch.float32, 9.0)
        resid_d[:n] = resid.to(DEV)
        out_f = resid_d if has_r and has_f else guarded(n, torch.float32, 9.0)
        out_b, out_lo = guarded(n, BF, 9.0), guarded(n, BF, 9.0)
        call(lib.syn_vq_train_ew, v.to(DEV), resid_d if has_r else None, relu_src.to(DEV) if has_m else None,
             keep.to(DEV) if has_k else None, sv, sr, out_f if has_f else None, out_b if has_b else None,
             out_lo if has_lo else None, lo_relu, n)
        assert guard_intact(out_f, n, 9.0) and guard_intact(out_b, n, 9.0) and guard_intact(out_lo, n, 9.0), combo
        if has_f:
            assert torch.equal(bits(out_f[:n]), bits(want_f)), combo
        assert torch.equal(bits(out_b[:n]), bits(want_b)), combo
        if has_lo:
            got_b, got_lo = out_b[:n].cpu().float(), out_lo[:n].cpu().float()
            assert torch.equal(bits(out_lo[:n]), bits(want_lo)), combo
            cut = (got_b <= 0) if lo_relu else torch.zeros(n, dtype=torch.bool)
            assert bool((got_lo[cut] == 0).all()) and (not lo_relu or bool(cut.any()) or n == 4), combo
            # the two halves give the fp32 value back to within one bf16 ulp (2^-7 relative) of the low half
            miss = (want_f.double() - got_b.double() - got_lo.double()).abs()[~cut]
            assert bool((miss <= 2.0 ** -7 * got_lo.double().abs()[~cut] + 1e-38).all()), combo
        if has_m and not has_r:
            assert float(out_b[:3].float().abs().max()) == 0.0 and float(out_b[3].float()) != 0.0, combo     # +0, -0 and a negative all cut


# ---- C4. cast, pair sum, zero stuffing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dp,rows", [(57, 64, 4), (57, 64, 5), (57, 64, 37), (180, 192, 1), (180, 192, 4), (180, 192, 11)])
@pytest.mark.parametrize("with_lo", [0, 1])
def test_cast_pads_and_splits(lib, dim, dp, rows, with_lo):
    """rows x dp elements: one workgroup exactly (4 x 64), one and a quarter, several with a part-filled last one; under one (1 x 192)."""
    x = torch.randn(rows, dim, generator=torch.Generator().manual_seed(rows + dim)) * 3.0
    out, lo = guarded(rows * dp, BF, 9.0), guarded(rows * dp, BF, 9.0)
    call(lib.syn_vq_train_cast, x.to(DEV), rows, dim, dp, out, lo if with_lo else None)
    full = torch.zeros(rows, dp)
    full[:, :dim] = x
    hi = full.to(BF)
    assert guard_intact(out, rows * dp, 9.0) and guard_intact(lo, rows * dp, 9.0)
    assert torch.equal(bits(out[:rows * dp]), bits(hi.reshape(-1)))
    if with_lo:
        assert torch.equal(bits(lo[:rows * dp]), bits((full - hi.float()).to(BF).reshape(-1)))
    else:
        assert bool((lo.float().cpu() == 9.0).all())


@pytest.mark.parametrize("clips,t,channels", [(2, 128, 4), (1, 257, 4), (2, 3, 512)])
def test_pairsum_and_stuff_respect_the_clips(lib, clips, t, channels):
    """(clips, t) frames of the coarse side; 4 / 8 channels make one thread per frame: 256 frames are one workgroup, 257 one more element."""
    g = torch.Generator().manual_seed(t)
    du = torch.randn(clips, 2 * t, channels, generator=g)
    out = guarded(clips * t * channels, torch.float32, 9.0)
    call(lib.syn_vq_train_pairsum, du.to(DEV), out, clips * t, channels)
    want = du[:, 0::2] + du[:, 1::2]                                      # per clip: frame r of clip n gets frames 2 r, 2 r + 1 of clip n
    assert guard_intact(out, want.numel(), 9.0) and torch.equal(bits(out[:want.numel()]), bits(want.reshape(-1)))
    ch8 = 2 * channels if channels == 4 else channels
    dy = torch.randn(clips, t, ch8, generator=g).to(BF)
    out = guarded(clips * 2 * t * ch8, BF, 9.0)
    call(lib.syn_vq_train_stuff, dy.to(DEV), out, clips * t, ch8)
    want = torch.zeros(clips, 2 * t, ch8, dtype=BF)
    want[:, 0::2] = dy                                                    # a clip's last frame is followed by its own zero row, then the next clip's first
    assert guard_intact(out, want.numel(), 9.0) and torch.equal(bits(out[:want.numel()]), bits(want.reshape(-1)))


# ---- C5. the loss kernels -----------------------------------------------------------------------------------------------------------------
# rows x dp = 4095, 4096, 4097 (a workgroup takes 4096; element 4096 of the last shape is a padded channel), and 8320: a third, part-filled
# workgroup with real channels in it
@pytest.mark.parametrize("rows,dim,dp", [(819, 3, 5), (64, 57, 64), (241, 13, 17), (130, 57, 64)])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_reconstruction_loss_and_its_gradient(lib, rows, dim, dp, kind):
    g = torch.Generator().manual_seed(rows + kind)
    gt = torch.randn(rows, dim, generator=g)
    diff = torch.randn(rows, dim, generator=g) * torch.where(torch.rand(rows, dim, generator=g) < 0.5, 0.3, 3.0)     # |diff| on both sides of 1
    rec = gt + diff
    rec[::7] = gt[::7]                                                    # and exactly 0
    n_parts = int(lib.syn_vq_train_loss_parts(rows, dp))
    assert n_parts == (rows * dp + 4095) // 4096
    d_rec, parts = guarded(rows * dp, BF, 9.0), guarded(n_parts, torch.float32, 9.0)
    call(lib.syn_vq_train_loss, rec.to(DEV), gt.to(DEV), rows, dim, dp, kind, d_rec, parts)
    assert guard_intact(d_rec, rows * dp, 9.0) and guard_intact(parts, n_parts, 9.0)
    d = rec.double() - gt.double()
    assert bool((d == 0).any()) and bool((d.abs() > 1).any()) and bool(((d.abs() < 1) & (d != 0)).any())
    term = [d * d, d.abs(), torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)][kind]
    grad = [2 * d, d.sign(), torch.where(d.abs() < 1, d, d.sign())][kind] / (rows * dim)
    got = d_rec[:rows * dp].cpu().float().view(rows, dp)
    assert float(got[:, dim:].abs().max()) == 0.0                          # padded channels
    # the kernel's fp32 value (difference, factor, 1 / count: three roundings) lies within 4 u of the fp64 one and bf16 rounding is monotonic
    lo, hi = (grad - 4 * U * grad.abs()).float().to(BF).float(), (grad + 4 * U * grad.abs()).float().to(BF).float()
    assert bool(((got[:, :dim] >= lo) & (got[:, :dim] <= hi)).all())
    assert float((lo != hi).double().mean()) < 1e-3                       # ... which leaves a choice of two bf16 values for next to no element
    flat = torch.zeros(rows, dp, dtype=torch.float64)
    flat[:, :dim] = term
    flat = torch.cat([flat.reshape(-1), torch.zeros(n_parts * 4096 - rows * dp, dtype=torch.float64)]).view(n_parts, 4096)
    err = (parts[:n_parts].cpu().double() - flat.sum(-1)).abs()
    print(f"kind {kind}, {rows} x {dp}: parts {parts[:n_parts].cpu().tolist()} error / bound {(err / ((4096 + 8) * U * flat.sum(-1))).tolist()}")
    assert bool((err <= (4096 + 8) * U * flat.sum(-1)).all())


@pytest.mark.parametrize("groups", [1, 65])
@pytest.mark.parametrize("n_active", [1, 3, 6])
def test_scalars_against_fp64(lib, groups, n_active):
    g = torch.Generator().manual_seed(groups + n_active)
    rows, count, commit_w = 16 * groups - 10, 1030 * 57, 0.02
    parts = torch.rand(3, generator=g) * 900.0
    sqerr = torch.rand(6, groups, generator=g) * 40.0
    bcount = torch.stack([torch.bincount(torch.randint(0, 512, (rows,), generator=g) % (64 + 75 * q), minlength=512) for q in range(6)]).float()
    out4 = guarded(4, torch.float32, 9.0)
    call(lib.syn_vq_train_scalars, parts.to(DEV), 3, count, sqerr.to(DEV), groups, bcount.to(DEV), n_active, rows,
         commit_w, out4)
    p = bcount[:n_active].double() / rows
    recons = float(parts.double().sum()) / count
    commit = float((sqerr[:n_active].double().sum(-1) / (rows * 512.0)).mean())
    perp = float(torch.exp(-(p * torch.log(p + 1e-7)).sum(-1)).mean())
    want = np.array([recons + commit_w * commit, recons, commit, perp])
    got = out4[:4].cpu().double().numpy()
    print(f"groups {groups}, n_active {n_active}: {got} vs {want}, relative {np.abs(got - want) / np.abs(want)}")
    assert guard_intact(out4, 4, 9.0) and bool((np.abs(got - want) <= 1e-6 * np.abs(want)).all())


# ---- C6. what the entry points refuse ---------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_document(lib):
    """Argument checks only: each call below returns non-zero with a message and launches nothing (every output keeps its fill)."""
    f32, bf = lambda n: torch.full((n,), 9.0, device=DEV), lambda n: torch.full((n,), 9.0, dtype=BF, device=DEV)
    st = _lib.current_stream()
    x, cb, cbt, cc, acc, rsum, sq = f32(16 * 512), f32(512 * 512), f32(512 * 512), f32(512), f32(16 * 512), f32(16 * 512), f32(4)
    idx = torch.zeros(16, 6, dtype=torch.int32, device=DEV)
    outs = [x, cb, cbt, cc, acc, rsum, sq]
    refused = [
        ("x_out == x_in", lib.syn_vq_train_quantize(x.data_ptr(), cb.data_ptr(), cbt.data_ptr(), cc.data_ptr(), None, 0.5, x.data_ptr(), acc.data_ptr(), None,
                                                    rsum.data_ptr(), idx.data_ptr(), sq.data_ptr(), 0, 1, 16, st)),
        ("ldy % 8", lib.syn_vq_train_wgrad(bf(4 * 68).data_ptr(), 68, bf(4 * 64).data_ptr(), 64, acc.data_ptr(), None, 1, 4, 4, 57, 57, 1, 1, 1, 0, 0, 0, st)),
        ("ldx % 8", lib.syn_vq_train_wgrad(bf(4 * 64).data_ptr(), 64, bf(4 * 60).data_ptr(), 60, acc.data_ptr(), None, 1, 4, 4, 57, 57, 1, 1, 1, 0, 0, 0, st)),
        ("pitch < cout", lib.syn_vq_train_wgrad(bf(4 * 64).data_ptr(), 56, bf(4 * 64).data_ptr(), 64, acc.data_ptr(), None, 1, 4, 4, 57, 57, 1, 1, 1, 0, 0, 0, st)),
        ("channels % 4", lib.syn_vq_train_pairsum(x.data_ptr(), acc.data_ptr(), 4, 6, st)),
        ("channels % 8", lib.syn_vq_train_stuff(bf(64).data_ptr(), acc.data_ptr(), 4, 12, st)),
        ("n % 4", lib.syn_vq_train_ew(x.data_ptr(), None, None, None, 1.0, 1.0, acc.data_ptr(), None, None, 0, 6, st)),
        ("tile: 511 rows, no noise", lib.syn_vq_train_tile(x.data_ptr(), 511, None, cb.data_ptr(), cbt.data_ptr(), cc.data_ptr(), st)),
        ("update: 511 rows, no noise", lib.syn_vq_train_codebook_update(x.data_ptr(), idx.data_ptr(), 0, 511, None, 0.99, 0.01, cb.data_ptr(), cbt.data_ptr(),
                                                                         cc.data_ptr(), rsum.data_ptr(), st)),
        ("cast: dim_padded < dim", lib.syn_vq_train_cast(x.data_ptr(), 4, 57, 56, acc.data_ptr(), None, st)),
        ("loss: dim_padded < dim", lib.syn_vq_train_loss(x.data_ptr(), cb.data_ptr(), 4, 57, 56, 0, acc.data_ptr(), sq.data_ptr(), st)),
        ("loss: kind", lib.syn_vq_train_loss(x.data_ptr(), cb.data_ptr(), 4, 57, 64, 3, acc.data_ptr(), sq.data_ptr(), st)),
        ("scalars: n_active", lib.syn_vq_train_scalars(sq.data_ptr(), 1, 1, sq.data_ptr(), 1, cb.data_ptr(), 7, 16, 0.02, cc.data_ptr(), st)),
    ]
    torch.cuda.synchronize()
    for what, rc in refused:
        assert rc != 0, what
    assert lib.syn_last_error()
    assert all(bool((t == 9.0).all()) for t in outs)
    assert int(lib.syn_vq_train_loss_parts(0, 64)) == -1
