"""WavEncoder forward on the device (csrc/syn_wavenc.inc: k_block0 + ten k_conv launches), every layer per element at tile-edge lengths.

syn_wav_encode is called directly, on a workspace and an output buffer the test owns; every intermediate is read back at the offsets
syn_wav_layout gives and held, element by element, against the float64 restatement of its own launch computed from the DEVICE's input to that
launch (tests/wavenc_ref.py: the acceptance interval, why it is the per-step bound and not the flat c 2^-24 S, and what `wide` means).  Beside the
values: everything outside the written rows of the workspace stays zero (halos, slack rows, alignment gaps), the output buffer is written exactly
over its span, a workspace that served another waveform gives the same bits, a clip's bits do not depend on its batch mates, and a batch above
HipWavEncoder.CHUNK is cut correctly.  The clip lengths are wavenc_ref.LENGTHS; tests/test_wavenc_host.py asserts from the length formula that they
put every level at, one below and one above its tile sizes, as one tile and as several.

Measured on an MI355X, maxima over every length, clip and channel count of this module.  `distance` = how far the exact value of an element is
from the set of values that round to what the device stored, before the activation; first in units of 2^-24 S (the smallest flat c that would
accept every element, beside the flat c = 2 (K / 32 + 4)), then as a share of the bound E in use (C_ACC = 2):
    b0 -> x1        2.14  (c  70)   0.157        b3.conv1|sc -> z3   0.62  (c  68)   0.071
    b1.conv1|sc z1  0.85  (c  68)   0.090        b3.conv1|sc -> s3   0.58  (c  68)   0.071
    b1.conv1|sc s1  0.57  (c  68)   0.070        b3.conv2 -> x4      0.63  (c 128)   0.063
    b1.conv2 -> x2  0.76  (c  68)   0.088        b4.conv1 -> z4      0.67  (c 128)   0.072
    b2.conv1 -> z2  0.84  (c  68)   0.089        b4.conv2 -> x5      0.56  (c 128)   0.055
    b2.conv2 -> x3  0.99  (c  68)   0.111        b5.conv1|sc -> z5   0.81  (c 128)   0.080
    b5.conv1|sc s5  0.79  (c 128)   0.074        b5.conv2 -> out     2.69  (c 248)   0.166   (fp32: the one layer whose error is seen directly)
No element of any layer was outside its interval, on the first run and since; C_ACC and c stay as derived: twice the largest measured share
(0.166, the fp32 output) is 0.33 of the bound, and twice the largest flat figure (2.69) is 5.4 beside c = 248.
Intervals of more than two bf16 values: at most 0.57 % of a layer (x1; limit 1 %).
What the module sees that a norm over the output does not, tried once on a library built with two wrong row counts in syn_wav_encode (block 1's
launch without the last, partial 6-row group of x1; block 2's conv1 without the last row of x2): every case here fails, naming row L2 - 1 of z1 / s1
(lengths with L1 mod 6 >= 3: the others never read that group, and x5's partial 3-row group is read at no length) and the last 8 rows of z2, while
test_wav_encoder_vs_torch and test_wav_encoder_single_channel pass on that library.
"""
import ctypes as C

import pytest
import torch

from syntalker_amd import _lib, conditioning
from tests import refmodel, wavenc_ref as R
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENTINEL = 4, -12345.625          # frames of sentinel behind the output's span
ONE_CHANNEL = (15, 4335, 12015)          # lengths that also run with a one-channel waveform


@pytest.fixture(scope="module")
def encoders():
    """{cin: (folded blocks, HipWavEncoder)}: the synthetic state dict as it is; one channel = block 0 restricted to its first input channel."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    two = conditioning.fold_wav_encoder(refmodel.synth_state_dict("beatx"))
    one = R.single_channel(two)
    return {cin: (b, conditioning.HipWavEncoder(b, torch.device(DEV))) for cin, b in ((1, one), (2, two))}


def waveform(clips, n, cin, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(clips, n, cin, generator=g) if cin == 2 else torch.randn(clips, n, generator=g)


def encode(enc, wav, ws=None):
    """One syn_wav_encode call -> (workspace [clips][per_clip] bf16 on the device, out [clips][L4][256] fp32 on the host).  The output buffer is NaN
    inside its span with GUARD frames of SENTINEL behind it: asserted here that the span is fully written and nothing behind it is."""
    lib = _lib.load()
    clips, n = wav.shape[:2]
    lay = R.layout(n)
    assert lay["per_clip"] * 2 * clips == lib.syn_wav_workspace_bytes(clips, n)
    if ws is None:
        ws = torch.zeros(clips, lay["per_clip"], dtype=torch.bfloat16, device=DEV)
    assert ws.shape == (clips, lay["per_clip"]) and ws.is_contiguous()
    frames = clips * lay["L4"]
    out = torch.full((frames + GUARD, 256), float("nan"), device=DEV)
    out[frames:] = SENTINEL
    wd = wav.to(DEV).contiguous()
    _lib.check(lib.syn_wav_encode(C.byref(enc.c), wd.data_ptr(), clips, n, ws.data_ptr(), out.data_ptr(), _lib.current_stream(wd.device)), "syn_wav_encode")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[frames:] == SENTINEL).all()), "written behind the output's span"
    assert not bool(torch.isnan(out[:frames]).any()), "output rows left unwritten"
    return ws, out[:frames].reshape(clips, lay["L4"], 256)


def tensors(ws, out, lay):
    """Every tensor of a run on the host: {name: [clips][L][C]} (bf16; "out": fp32)."""
    w = ws.cpu()
    return {**{name: R.read(w, lay, name) for name in R.TENSORS}, "out": out}


def check_layers(blocks, wav, ws, out, lay, tag):
    """The comparator over every launch, each fed the device's own input; the sharpness condition; the untouched rows."""
    got = {"wav": wav, **tensors(ws, out, lay)}
    failures = []
    for layer in R.LAYERS:
        for r in R.layer_refs(blocks, layer, got.__getitem__):
            g = got[r.name]
            flat, share = r.measured(g)
            wide = float(r.wide.double().mean())
            print(f"wavenc {tag} {layer.name} -> {r.name}: max distance {flat:.2f} x 2^-24 S (flat c {R.c_of(r.steps):.0f}), {share:.3f} of E; wide {wide:.4f}")
            assert wide <= 0.01, (tag, r.name, wide)
            bad = r.bad(g).nonzero()
            if len(bad):
                i = tuple(bad[0].tolist())
                failures.append(f"{layer.name} -> {r.name}: {len(bad)} of {g.numel()} elements, first (clip, row, channel) = {i}: got {float(g[i])!r}, "
                                f"interval [{float(r.lo[i])!r}, {float(r.hi[i])!r}], rows hit {sorted(set(bad[:, 1].tolist()))[:8]} of {g.shape[1]}")
    assert not failures, f"{tag}: " + "; ".join(failures)
    stray = R.stray(ws.cpu(), lay)
    assert stray.numel() == 0, f"{tag}: {len(stray)} non-zero elements outside the written rows, first (clip, element) = {stray[0].tolist()}"


@pytest.mark.parametrize("n,cin", [(n, 2) for n in R.LENGTHS] + [(n, 1) for n in ONE_CHANNEL])
def test_every_layer_per_element(encoders, n, cin):
    """2 clips with different waveforms: every launch against its float64 restatement per element, untouched rows, output bounds; each clip alone gives
    the bits it has in the pair, into an output buffer of its own with its own guard frames."""
    blocks, enc = encoders[cin]
    lay = R.layout(n)
    wav = waveform(2, n, cin, seed=n + cin)
    ws, out = encode(enc, wav)
    check_layers(blocks, wav, ws, out, lay, f"n={n} cin={cin}")
    for i in range(2):
        ws1, out1 = encode(enc, wav[i:i + 1])
        assert torch.equal(out1[0], out[i]) and torch.equal(ws1[0].view(torch.int16), ws[i].view(torch.int16)), (n, cin, i)


@pytest.mark.parametrize("n", [1735, 12050])
def test_a_used_workspace_gives_the_same_bits(encoders, n):
    """Waveform A, then waveform B on the same workspace: B's output and every intermediate are bitwise what a freshly zeroed workspace gives, and the
    rows nobody writes are zero after both (a stray write of A's run would sit in B's halos: re-running the SAME waveform cannot show that)."""
    blocks, enc = encoders[2]
    lay = R.layout(n)
    a, b = waveform(2, n, 2, seed=1), 3.0 * waveform(2, n, 2, seed=2)
    ws, _ = encode(enc, a)
    assert R.stray(ws.cpu(), lay).numel() == 0
    ws, out = encode(enc, b, ws)
    assert R.stray(ws.cpu(), lay).numel() == 0
    ws_fresh, out_fresh = encode(enc, b)
    assert torch.equal(out, out_fresh) and torch.equal(ws.view(torch.int16), ws_fresh.view(torch.int16))
    check_layers(blocks, b, ws, out, lay, f"n={n} reused")


@pytest.mark.parametrize("n", [15, 20135])
def test_a_clip_does_not_depend_on_its_batch_mates(encoders, n):
    """Clip i of a 5-clip call = the 1-clip call, bitwise, intermediates included: at the shortest clip (112 / 17 / 1 rows behind block 0) and at one of several tiles per level."""
    _, enc = encoders[2]
    wav = waveform(5, n, 2, seed=7)
    ws, out = encode(enc, wav)
    for i in range(5):
        ws1, out1 = encode(enc, wav[i:i + 1])
        assert torch.equal(out1[0], out[i]) and torch.equal(ws1[0].view(torch.int16), ws[i].view(torch.int16)), (n, i)


def test_batches_above_the_chunk_size(encoders):
    """HipWavEncoder cuts a batch into calls of CHUNK clips: CHUNK + 1 shortest clips, every one equal to its own 1-clip result bitwise, and the whole
    against the chained reference at the encoder tests' 2e-2."""
    blocks, enc = encoders[2]
    clips = enc.CHUNK + 1
    assert clips == 257
    wav = waveform(clips, 15, 2, seed=3)
    got = enc(wav.to(DEV)).cpu()
    assert got.shape == (clips, 1, 256) and bool(torch.isfinite(got).all())
    ws = torch.zeros(1, R.layout(15)["per_clip"], dtype=torch.bfloat16, device=DEV)
    for i in range(clips):
        assert torch.equal(encode(enc, wav[i:i + 1], ws)[1][0], got[i]), i
    e = rel_l2(got, R.chain_out(blocks, wav))
    print(f"wavenc {clips} clips of 15 samples: rel-L2 vs the chained reference {e:.3e}")
    assert e < 2e-2
