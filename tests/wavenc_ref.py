"""Per-layer float64 reference of the WavEncoder forward (csrc/syn_wavenc.inc) and a per-element comparator.

The eleven launches of syn_wav_encode are restated one by one as F.conv1d in float64 on the model's own geometry (stride, padding, which
tensors a layer reads and writes - conditioning.fold_wav_encoder's blocks), with the folded fp32 weights rounded to bf16 and the fp32 bias, as
the kernels hold them.  The regrouping of the strided convolutions (conditioning.wav_gemm_weight) is NOT used here: it is part of what is under
test.  A layer's reference is computed from the DEVICE's own input to that layer, read back from the workspace (bf16 values are exact), so an
element's error is that of one launch and nothing is chained - `chain()` feeds the layers their own rounded outputs instead and stands in for the
device where there is none.

What the kernels do to a value, and what the acceptance interval of an element is made of:
  * bf16 x bf16 products are exact in fp32; a 16x16x32 MFMA step adds 32 of them to the accumulator, K / 32 steps per output (K = taps x cin),
    taps outermost, blocks of 32 input channels inside (the zero taps that a strided layer's row groups add change nothing); then come the bias,
    the residual and the LeakyReLU's multiplication, one fp32 rounding each.  The flat bound: one rounding per step and S = conv(|w|, |x|) +
    |bias| + |residual| give (K / 32 + 3) 2^-24 S; how the matrix pipe rounds INSIDE a step is not documented, so it carries a factor of two,
    E_flat = c 2^-24 S, c = 2 (K / 32 + 4)   (`c_of`: 68 ... 248 for K = 960 ... 3840, 70 for block 0).
  * E_flat is too blunt to test with: the sums cancel (|value| is a few per cent of S), and on 1 - 4 % of a layer's elements the interval it
    gives holds more than two bf16 values, at any waveform scale.  A step's rounding is relative to what the step adds up, not to S: with
    a_k the exact accumulator going into step k, a step is off by at most C_ACC 2^-24 (|a_k| + sum of the step's |products|) - C_ACC = 2
    roundings per step, the same factor of two - and the three roundings behind the loop by 2^-24 S each:
        E = 2^-24 (C_ACC sum_k |a_k| + 5 S)  <=  E_flat  (|a_k| <= S; asserted by the host test),
    so what this comparator accepts the flat one accepts.  `_steps` walks the steps in float64 to get the a_k.  C_ACC is the one number
    that may have to move if the hardware rounds more than twice per step; the GPU tests print, per layer, how far the device's values are
    from the reference in units of 2^-24 S and of E (`Ref.measured`), and their docstring records the maxima.
  * LeakyReLU is monotone, and so is rounding to bf16 (to nearest even): a bf16 output is accepted iff
        bf16(lrelu(pre - E)) <= got <= bf16(lrelu(pre + E)),
    pre = the exact pre-activation value.  (The activation is applied to the END POINTS: the error of a negative value shrinks with it.)
    The fp32 output is accepted iff lrelu(pre - E) - ulp32 <= got <= lrelu(pre + E) + ulp32.
  * k_block0's conv1 output never leaves LDS.  It is restated as z = lrelu(conv + b) with its own interval [z_lo, z_hi] in bf16; conv2's reference
    reads bf16(z), and conv(|w2|, max(z_hi - bf16(z), bf16(z) - z_lo)) joins E: zero wherever conv1's rounding is unambiguous.
An interval that holds more than two adjacent bf16 values says little; `Ref.wide` counts them (the tests bound their share by 1 % per layer).
"""
import collections

import torch
import torch.nn.functional as F

SLOPE = float(torch.tensor(0.01, dtype=torch.float32))      # the kernels' 0.01f
U = 2.0 ** -24

LAYOUT_WORDS = ("L1", "L2", "L3", "L4", "per_clip", "x1", "z1", "s1", "x2", "z2", "x3", "z3", "s3", "x4", "z4", "x5", "z5", "s5", "halo", "slack")
# tensor -> (channels, the level whose length it has, whether `halo` zero rows lie in front of its row 0)
TENSORS = {"x1": (64, "L1", False), "z1": (64, "L2", True), "s1": (64, "L2", False), "x2": (64, "L2", True), "z2": (64, "L2", True),
           "x3": (64, "L2", False), "z3": (128, "L3", True), "s3": (128, "L3", False), "x4": (128, "L3", True), "z4": (128, "L3", True),
           "x5": (128, "L3", False), "z5": (256, "L4", True), "s5": (256, "L4", False)}
# rows per workgroup of the launches that write a level (syn_wav_encode's template arguments: WM x RF x 16)
TILES = {"L1": (512,), "L2": (64, 256), "L3": (64, 128), "L4": (64,)}

# Clip lengths of the GPU tests: the smallest at which each tile edge exists (15 ... 34185), 4365 and 8625 (257 and 65 rows: one past a single
# 256- / 64-row tile) and the shortest clips with 255 - 257 rows at level 3 and 127 - 129 at level 4 (several 128- / 64-row tiles); `covers`
LENGTHS = (15, 1730, 1735, 4305, 4335, 4365, 8160, 8265, 8445, 8625, 11985, 12015, 12050, 19885, 20135, 20290, 24765, 33105, 33645, 34185,
           42825, 43005, 43185, 67665, 68205, 68745)

Layer = collections.namedtuple("Layer", "name block kind src res outs")
# in launch order; kind: block0 | c1sc (conv1 and the shortcut conv of a down-sampling block, one launch) | c1 | c2 (+ residual, activation)
LAYERS = (
    Layer("b0", 0, "block0", "wav", None, ("x1",)),
    Layer("b1.conv1|sc", 1, "c1sc", "x1", None, ("z1", "s1")), Layer("b1.conv2", 1, "c2", "z1", "s1", ("x2",)),
    Layer("b2.conv1", 2, "c1", "x2", None, ("z2",)), Layer("b2.conv2", 2, "c2", "z2", "x2", ("x3",)),
    Layer("b3.conv1|sc", 3, "c1sc", "x3", None, ("z3", "s3")), Layer("b3.conv2", 3, "c2", "z3", "s3", ("x4",)),
    Layer("b4.conv1", 4, "c1", "x4", None, ("z4",)), Layer("b4.conv2", 4, "c2", "z4", "x4", ("x5",)),
    Layer("b5.conv1|sc", 5, "c1sc", "x5", None, ("z5", "s5")), Layer("b5.conv2", 5, "c2", "z5", "s5", ("out",)),
)


def lengths(n):
    """Positions after blocks 0, 1 (= 2), 3 (= 4), 5 of an n-sample clip: Conv1d(k = 15) with stride 5 / padding 1700, then strides 6, 6, 3 unpadded."""
    L1 = (n + 3385) // 5 + 1
    L2 = (L1 - 15) // 6 + 1
    L3 = (L2 - 15) // 6 + 1
    return L1, L2, L3, (L3 - 15) // 3 + 1


def layout(n):
    """syn_wav_layout(n) as a dict (host only: no GPU)."""
    import ctypes
    from syntalker_amd import _lib
    words = (ctypes.c_int64 * len(LAYOUT_WORDS))()
    _lib.check(_lib.load().syn_wav_layout(n, ctypes.cast(words, ctypes.c_void_p)), "syn_wav_layout")
    return dict(zip(LAYOUT_WORDS, (int(v) for v in words)))


def regions(lay):
    """{tensor: (first element, one past the last)} of the rows [0, L) that syn_wav_encode writes inside a clip's workspace."""
    out = {}
    for name, (ch, level, halo) in TENSORS.items():
        first = lay[name] + (lay["halo"] * ch if halo else 0)
        out[name] = (first, first + lay[level] * ch)
    return out


def read(ws, lay, name):
    """Tensor `name` of every clip out of ws [clips][per_clip] bf16 -> [clips][L][channels] bf16."""
    first, last = regions(lay)[name]
    return ws[:, first:last].reshape(ws.shape[0], -1, TENSORS[name][0])


def stray(ws, lay):
    """Indices (clip, element) of the non-zero bf16 elements OUTSIDE the written regions: halos in front and behind, slack rows, alignment gaps."""
    keep = torch.ones(lay["per_clip"], dtype=torch.bool)
    for first, last in regions(lay).values():
        keep[first:last] = False
    return ((ws.view(torch.int16) & 0x7FFF) != 0).logical_and(keep).nonzero()


# ---- bf16 as an ordered set ---------------------------------------------------------------------------------------------------------------
def bf16(x):
    """float64 -> nearest bf16 (through fp32: monotone, which is all the comparator needs), as float64."""
    return x.to(torch.bfloat16).double()


def bf16_ord(x):
    """Position of a bf16-representable value on the bf16 number line (+-0 -> 0, neighbours differ by 1)."""
    i = x.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7FFF))


def bf16_at(o):
    bits = torch.where(o >= 0, o, (-o) | 0x8000)
    return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.bfloat16).double()


def lrelu(v):
    return torch.where(v > 0, v, SLOPE * v)


def c_of(steps):
    """The constant of the flat bound c 2^-24 S for an output behind `steps` MFMA steps (module docstring)."""
    return 2.0 * (steps + 4)


C_ACC = 2.0     # roundings, in units of 2^-24 of |accumulator| + sum |products|, that one MFMA step is allowed (module docstring)


class Ref:
    """One output tensor of one launch: pre-activation reference, its error bound, the acceptance interval.  Channels-last [clips][L][C] float64."""

    def __init__(self, name, pre, S, A, steps, act, extra=None, fp32=False, c_acc=None):
        self.name, self.pre, self.S, self.A, self.steps, self.act, self.fp32 = name, pre, S, A, steps, act, fp32
        self.extra = torch.zeros_like(S) if extra is None else extra
        self.E = U * ((C_ACC if c_acc is None else c_acc) * A + 5 * S) + self.extra
        self.E_flat = c_of(steps) * U * S + self.extra
        f = lrelu if act else (lambda v: v)
        self.ref, self.lo64, self.hi64 = f(pre), f(pre - self.E), f(pre + self.E)
        if fp32:
            ulp = torch.maximum(self.ref.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64))
            ulp = 2.0 ** (torch.floor(torch.log2(ulp)) - 23)
            self.lo, self.hi = self.lo64 - ulp, self.hi64 + ulp
            self.wide = torch.zeros_like(S, dtype=torch.bool)
        else:
            self.lo, self.hi = bf16(self.lo64), bf16(self.hi64)
            self.wide = bf16_ord(self.hi) - bf16_ord(self.lo) > 1            # more than two adjacent bf16 values

    def value(self):
        """What a kernel without accumulation error would store (the chain's next input)."""
        return self.ref.float().double() if self.fp32 else bf16(self.ref)

    def bad(self, got):
        """Mask of the elements of `got` (bf16 or fp32 tensor) outside their interval; NaN is outside."""
        g = got.double()
        return ~((g >= self.lo) & (g <= self.hi))

    def distance(self, got):
        """Per element, the distance before the activation from the reference to the set of values that round to `got` (block 0's extra term
        taken off): what the accumulation must at least have been off by.  distance / (2^-24 S) is the smallest flat c that accepts the element,
        distance / (E - extra) the share of the bound in use - the figures the test modules' docstrings record."""
        g = got.double()
        if self.fp32:
            half = (self.hi - self.hi64) / 2
            cell_lo, cell_hi = g - half, g + half
        else:
            o = bf16_ord(g)
            cell_lo, cell_hi = (g + bf16_at(o - 1)) / 2, (g + bf16_at(o + 1)) / 2
        if self.act:
            inv = lambda y: torch.where(y > 0, y, y / SLOPE)
            cell_lo, cell_hi = inv(cell_lo), inv(cell_hi)
        d = torch.maximum(cell_lo - self.pre, self.pre - cell_hi).clamp_min(0)
        return (d - self.extra).clamp_min(0)

    def measured(self, got):
        """(max distance / (2^-24 S), max distance / (E - extra)) over the tensor."""
        d = self.distance(got)
        return float((d / (U * self.S).clamp_min(2.0 ** -200)).max()), float((d / (self.E - self.extra).clamp_min(2.0 ** -200)).max())


def _steps(x, w, b, stride, pad, acc0=None):
    """F.conv1d in float64, and beside it the same sum the way the kernels accumulate it: one MFMA step per (tap, block of 32 input channels), taps outermost (the zero taps a
    strided layer's row groups add change nothing).  x [clips][L][cin] float64, w (cout, cin, 15), acc0: the accumulators' initial value.
    -> (conv + acc0, sum |products| + |acc0|, sum over the steps of |accumulator going in|), channels-last."""
    xp = F.pad(x.transpose(1, 2), (pad, pad))
    n_out = (xp.shape[2] - 15) // stride + 1
    acc = x.new_zeros(x.shape[0], w.shape[0], n_out) if acc0 is None else acc0.transpose(1, 2).clone()
    S, A, wa = acc.abs(), torch.zeros_like(acc), w.abs()
    blk = min(32, w.shape[1] * 15)                                           # block 0's first layer: all taps x channels are ONE step
    for t in range(15):
        xs = xp[:, :, t: t + (n_out - 1) * stride + 1: stride]
        for c0 in range(0, w.shape[1], 32):
            if blk == 32 or t == 0:
                A += acc.abs()
            acc = acc + torch.einsum("oc,bcl->bol", w[:, c0:c0 + 32, t], xs[:, c0:c0 + 32])
            S += torch.einsum("oc,bcl->bol", wa[:, c0:c0 + 32, t], xs[:, c0:c0 + 32].abs())
    # the value itself comes from F.conv1d; the walk above only has to agree with it (float64 round-off) to vouch for S and the a_k
    y = F.conv1d(x.transpose(1, 2), w, None, stride=stride, padding=pad) + (0 if acc0 is None else acc0.transpose(1, 2))
    assert y.shape == acc.shape and float((y - acc).abs().max()) <= 1e-12 * float(S.max()), "step walk and F.conv1d disagree"
    if b is not None:
        y, S = y + b[None, :, None], S + b.abs()[None, :, None]
    return y.transpose(1, 2), S.transpose(1, 2), A.transpose(1, 2)


def _wb(pair):
    return pair[0].to(torch.bfloat16).double(), pair[1].double()


def layer_refs(blocks, layer, get, c_acc=None):
    """The Refs of one launch.  get(name) -> the launch's input tensor `name` [clips][L][C] ("wav": [clips][n][cin] fp32), any float type."""
    blk = blocks[layer.block]
    x = get(layer.src).double()
    if layer.kind == "block0":
        x = bf16(x if x.dim() == 3 else x.unsqueeze(-1))                      # k_block0 rounds the waveform window to bf16
        (w1, b1), (w2, b2), (wsc, bsc) = _wb(blk["c1"]), _wb(blk["c2"]), _wb(blk["sc"])
        z = Ref("b0.z", *_steps(x, w1, b1, blk["stride"], blk["pad"]), 1, True, c_acc=c_acc)
        zb = z.value()
        sc, s_sc, _ = _steps(x, wsc, bsc, blk["stride"], blk["pad"])          # stays fp32: the initial value of conv2's accumulators
        y, s, a = _steps(zb, w2, b2, 1, 7, acc0=sc)
        extra = _steps(torch.maximum(z.hi - zb, zb - z.lo), w2.abs(), None, 1, 7)[0]
        return [Ref("x1", y, s + s_sc - sc.abs(), a, 1 + 15 * 64 // 32, True, extra=extra, c_acc=c_acc)]
    steps = 15 * x.shape[2] // 32
    if layer.kind in ("c1", "c1sc"):
        out = [Ref(layer.outs[0], *_steps(x, *_wb(blk["c1"]), blk["stride"], blk["pad"]), steps, True, c_acc=c_acc)]
        if layer.kind == "c1sc":
            out.append(Ref(layer.outs[1], *_steps(x, *_wb(blk["sc"]), blk["stride"], blk["pad"]), steps, False, c_acc=c_acc))
        return out
    r = get(layer.res).double()
    y, s, a = _steps(x, *_wb(blk["c2"]), 1, 7)
    return [Ref(layer.outs[0], y + r, s + r.abs(), a + y.abs(), steps, True, fp32=layer.outs[0] == "out", c_acc=c_acc)]


def chain(blocks, wav, c_acc=None):
    """Every layer fed the rounded output of the one before: {tensor: Ref} in launch order.  The stand-in for the device on a host without one."""
    vals, refs = {"wav": wav}, collections.OrderedDict()
    for layer in LAYERS:
        for r in layer_refs(blocks, layer, vals.__getitem__, c_acc):
            refs[r.name] = r
            vals[r.name] = r.value()
    return refs


def chain_out(blocks, wav):
    """The chain's final output alone, by F.conv1d in float64 (no bounds: a fraction of chain()'s cost, for many clips at once).  Sums in another
    order than chain(), so a bf16 rounding on the way may fall the other way: equal to it to ~1e-3 in rel-L2, not bitwise."""
    x = bf16((wav if wav.dim() == 3 else wav.unsqueeze(-1)).double()).transpose(1, 2)
    for i, blk in enumerate(blocks):
        conv = lambda v, pair, stride, pad: F.conv1d(v, *_wb(pair), stride=stride, padding=pad)
        z = bf16(lrelu(conv(x, blk["c1"], blk["stride"], blk["pad"])))
        r = conv(x, blk["sc"], blk["stride"], blk["pad"]) if blk["sc"] is not None else x
        x = lrelu(conv(z, blk["c2"], 1, 7) + (r if i == 0 else bf16(r)))
        x = x.float().double() if i == 5 else bf16(x)
    return x.transpose(1, 2).float()


def single_channel(blocks):
    """The same encoder for a one-channel waveform: block 0's conv1 and shortcut keep their first input channel."""
    b0 = dict(blocks[0])
    for k in ("c1", "sc"):
        b0[k] = (blocks[0][k][0][:, :1].contiguous(), blocks[0][k][1])
    return [b0] + list(blocks[1:])


def covers(ns):
    """The edge classes a set of clip lengths has to hit, from the length formula alone -> list of the classes it MISSES (empty: all covered).
    Per level: length = 0, 1, 15 mod 16 (full / one-row / all-but-one last 16-row fragment); for every tile size MW of the level the lengths
    k MW - 1, k MW, k MW + 1 both with k = 1 (one workgroup, where the shortest legal clip leaves the level that short) and with k >= 2; every
    residue of L1 mod 6, L2 mod 6 and L3 mod 3 (the row-group tails of the strided layers); the shortest legal clip, 15 samples."""
    ls = [lengths(n) for n in ns]
    shortest = lengths(15)
    missing = [] if 15 in ns else ["n = 15"]
    for i, level in enumerate(("L1", "L2", "L3", "L4")):
        have = {l[i] for l in ls}
        missing += [f"{level} = {r} mod 16" for r in (0, 1, 15) if not any(v % 16 == r for v in have)]
        for mw in TILES[level]:
            for d in (-1, 0, 1):
                if shortest[i] <= mw + d and mw + d not in have:
                    missing.append(f"{level} = {mw}{d:+d} (one tile)")
                if not any(v > mw + 1 and (v - d) % mw == 0 for v in have):
                    missing.append(f"{level} = k {mw}{d:+d}, k >= 2")
    for i, m in ((0, 6), (1, 6), (2, 3)):
        missing += [f"L{i + 1} = {r} mod {m}" for r in range(m) if not any(l[i] % m == r for l in ls)]
    return missing
