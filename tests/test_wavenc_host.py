"""WavEncoder forward, the host side of its per-element tests (no GPU): the layout query syn_wav_layout, the clip lengths the GPU tests run at, and
the reference machinery of tests/wavenc_ref.py checked on itself - the chained float64 reference stands in for the device.

Recorded here because the GPU tests rest on it (20135 samples, 2 clips, waveform ~ N(0, 1), the synthetic state dict):
  * with the flat bound E = c 2^-24 S, c = 2 (K / 32 + 4), 0.7 - 3.7 % of a layer's elements have an interval of more than two bf16 values (the
    sums cancel: |value| is a few per cent of S), at any waveform scale from 0.03 to 3: the 1 % condition cannot be met with it;
  * with the per-step bound of wavenc_ref (never wider than the flat one: asserted below) the share is 0.07 - 0.55 %.
The perturbations of `test_the_comparator_sees_what_a_norm_cannot` (20135 samples): two bf16 ulps on one element of the last row of x2 move the
final output by rel-L2 4.3e-4; the same on x3 by nothing at all (the stride-6 layer behind it never reads its last five rows); one value of 0.5
in the halo row in front of x2 by 7.4e-4.  The encoder tests' threshold is 2e-2; the comparator and the untouched-rows check reject all three.
"""
import ctypes

import pytest
import torch

from syntalker_amd import _lib, conditioning
from tests import refmodel, wavenc_ref as R
from tests.conftest import rel_l2

LENGTHS = R.LENGTHS
CHAIN_LENGTHS = (15, 4335, 20135)


@pytest.fixture(scope="module")
def blocks():
    return conditioning.fold_wav_encoder(refmodel.synth_state_dict("beatx"))


@pytest.fixture(scope="module")
def chains(blocks):
    torch.set_num_threads(min(8, torch.get_num_threads()))
    out = {}
    for n in CHAIN_LENGTHS:
        wav = torch.randn(2, n, 2, generator=torch.Generator().manual_seed(n))
        out[n] = (wav, R.chain(blocks, wav))
    return out


def test_layout_query_matches_the_formula_and_the_size_queries():
    lib = _lib.load()
    for n in LENGTHS + (16, 68224, 68266):
        lay = R.layout(n)
        assert (lay["L1"], lay["L2"], lay["L3"], lay["L4"]) == R.lengths(n) and lay["L4"] == lib.syn_wav_out_frames(n)
        assert (lay["halo"], lay["slack"]) == (7, 16)
        for clips in (1, 3):
            assert lay["per_clip"] * 2 * clips == lib.syn_wav_workspace_bytes(clips, n)
        # what a tensor owns: its rows, the halos of a padded one with the slack behind, the slack of a row-grouped one (x1, x3, x5)
        spans = []
        for name, (ch, level, halo) in R.TENSORS.items():
            rows = lay[level] + (2 * lay["halo"] + lay["slack"] if halo else lay["slack"] if name in ("x1", "x3", "x5") else 0)
            assert lay[name] % 64 == 0, (n, name)
            spans.append((lay[name], lay[name] + rows * ch, name))
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] <= lay["per_clip"] and lay["per_clip"] % 64 == 0
        for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
            assert end <= start, (n, a, b)
        # the rows a strided layer's last row group reads lie inside the slack
        for name, level, s in (("x1", "L1", 6), ("x3", "L2", 6), ("x5", "L3", 3)):
            assert -(-lay[level] // s) * s <= lay[level] + lay["slack"]
        written = R.regions(lay)
        assert all(lay[name] <= written[name][0] < written[name][1] for name in R.TENSORS)


def test_layout_query_refuses_null_and_short_clips():
    lib = _lib.load()
    words = (ctypes.c_int64 * len(R.LAYOUT_WORDS))(*([-7] * len(R.LAYOUT_WORDS)))
    assert lib.syn_wav_layout(68224, None) != 0 and b"syn_wav_layout" in lib.syn_last_error()
    for n in (14, 0, -1):
        assert lib.syn_wav_layout(n, ctypes.cast(words, ctypes.c_void_p)) != 0 and b"syn_wav_layout" in lib.syn_last_error()
    assert list(words) == [-7] * len(R.LAYOUT_WORDS)                       # a refusal writes nothing
    assert lib.syn_wav_layout(15, ctypes.cast(words, ctypes.c_void_p)) == 0 and words[3] == 1
    assert _lib.PROTOTYPES["syn_wav_layout"] == (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p]) and "syn_wav_layout" in _lib.EXPORTS


def test_the_length_set_covers_every_edge_class():
    assert R.covers(LENGTHS) == []
    # the check itself is sharp: each of these drops exactly the classes it alone holds
    assert R.covers([n for n in LENGTHS if n != 15]) != []
    assert any("L2 = 256+1" in m for m in R.covers([n for n in LENGTHS if n != 4365]))
    assert any("L4 = k 64+0" in m for m in R.covers([n for n in LENGTHS if n != 68205]))
    assert R.lengths(15) == (681, 112, 17, 1) and R.lengths(1730) == (1024, 169, 26, 4) and R.lengths(33645)[3] == 64


def test_chained_reference_agrees_with_the_model(blocks, chains):
    """The per-layer restatement, chained, is the folded model: same shapes, rel-L2 < 2e-2 (bf16 activations through eleven layers)."""
    for n, (wav, refs) in chains.items():
        want = refmodel.wav_features(blocks, wav)
        got = refs["out"].value().float()
        assert got.shape == want.shape == (2, R.lengths(n)[3], 256)
        assert rel_l2(got, want) < 2e-2, (n, rel_l2(got, want))
        lay = R.layout(n)
        for name, (ch, level, _) in R.TENSORS.items():
            assert refs[name].ref.shape == (2, lay[level], ch), (n, name)
    one = R.single_channel(blocks)
    wav = torch.randn(2, 4335, generator=torch.Generator().manual_seed(1))
    assert rel_l2(R.chain(one, wav)["out"].value().float(), refmodel.wav_features(one, wav)) < 2e-2


def test_intervals_are_sharp_and_never_wider_than_the_flat_bound(chains):
    """At most 1 % of a layer's elements have an acceptance interval of more than two adjacent bf16 values, and every element's bound lies inside
    the flat c 2^-24 S, c = 2 (K / 32 + 4): whatever this comparator accepts, that one accepts."""
    for n, (_, refs) in chains.items():
        for name, r in refs.items():
            assert bool((r.E <= r.E_flat).all()), (n, name)
            assert float(r.wide.double().mean()) <= 0.01, (n, name, float(r.wide.double().mean()))
            assert not r.bad(r.value().float() if r.fp32 else r.value().to(torch.bfloat16)).any()      # the reference passes its own check
            assert r.measured(r.value())[0] <= 1.0        # (not 0: float64 -> bf16 goes through fp32, which can move a near-tie by 2^-24 |value|)


def _rest(blocks, vals, start):
    """The chain from launch `start` on, over given values -> final output."""
    vals = dict(vals)
    for layer in R.LAYERS[start:]:
        for r in R.layer_refs(blocks, layer, vals.__getitem__):
            vals[r.name] = r.value()
    return vals["out"].float()


def test_the_comparator_sees_what_a_norm_cannot(blocks, chains):
    n = 20135
    wav, refs = chains[n]
    lay = R.layout(n)
    vals = {"wav": wav, **{k: r.value() for k, r in refs.items()}}
    out = vals["out"].float()
    # one element of the last row of the last tile (782 rows: tiles of 64 and 256), two bf16 ulps off: in x2, which the next launch reads to its
    # last row, and in x3, whose last rows the stride-6 layer behind it never reads (782 = 6 * 127 + 15 + 5) - no test of the output can see those
    for name, start in (("x2", 3), ("x3", 5)):
        r = refs[name]
        at = (1, lay["L2"] - 1, 37)
        got = r.value().clone()
        got[at] = R.bf16_at(R.bf16_ord(got[at]) + (2 if got[at] >= 0 else -2))
        bad = r.bad(got.to(torch.bfloat16))
        assert bad[at] and int(bad.sum()) == 1
        assert rel_l2(got.float(), r.value().float()) < 1e-3
        e = rel_l2(_rest(blocks, {**vals, name: got}, start), out)
        print(f"two bf16 ulps on {name}{at}: final output moves by rel-L2 {e:.2e}")
        assert (0 < e < 1e-3) if name == "x2" else e == 0
    # one non-zero value in the halo row in front of x2: the untouched-rows check finds it; what the next launch reads moves the output by < 1e-3
    ws = torch.zeros(2, lay["per_clip"], dtype=torch.bfloat16)
    for name, (first, last) in R.regions(lay).items():
        ws[:, first:last] = refs[name].value().to(torch.bfloat16).reshape(2, -1)
    assert R.stray(ws, lay).numel() == 0
    assert torch.equal(R.read(ws, lay, "z3").double(), refs["z3"].value())
    spot = lay["x2"] + (lay["halo"] - 1) * 64 + 5                           # last halo row in front of x2, channel 5
    ws[1, spot] = 0.5
    assert R.stray(ws, lay).tolist() == [[1, spot]]
    x2 = torch.nn.functional.pad(vals["x2"], (0, 0, 7, 7))
    x2[1, 6, 5] = 0.5
    w, b = R._wb(blocks[2]["c1"])
    z2 = R.bf16(R.lrelu(R._steps(x2, w, b, 1, 0)[0]))
    assert z2.shape == vals["z2"].shape and not torch.equal(z2, vals["z2"])
    e = rel_l2(_rest(blocks, {**vals, "z2": z2}, 4), out)
    print(f"0.5 in the halo row in front of x2: final output moves by rel-L2 {e:.2e}")
    assert 0 < e < 1e-3
