"""The input / output stages of the wave-per-sequence step kernel k_seq (csrc/syn_seq.inc) and the generator its output stage
draws from (philox_round / randn4, csrc/syn_kernels.hip): the shapes at which waves idle or a workgroup is ragged, crossed with
the three noise terms of the update and with single-step / persistent launches, plus the generator against a NumPy restatement.

The generator's integer stage has no output of its own in the C ABI (syn_randn returns normals), so it is pinned from both sides:
the NumPy Philox4x32-10 below must reproduce the published known-answer vectors exactly, and the device's normals must be the
Box-Muller transform of exactly those words - one wrong word among the 4096 values moves the rel-L2 figure to ~1e-2, four orders
above the bound (only a flip below the fp32 rounding of a word, i.e. in its low 8 bits, cannot be seen through a float)."""
import numpy as np
import pytest
import torch

from syntalker_amd import synth
from tests.conftest import rel_l2
from tests.refmodel import synth_state_dict
from tests.test_gpu_parity import DEV, FWD_TOL, LOOP_TOL, _model

gpu = pytest.mark.gpu          # (per test: the known-answer check of the NumPy generator needs no GPU and runs in the CPU suite too)

T, CH = 32, 1536
# first clip of the generator's index space: clip 0 of every batch below covers elements 2^34 - 16384 .. 2^34 + 32767, so the
# Philox counter (element index / 4) carries into its high word inside the clip every test has
FIRST_CLIP = (1 << 34) // (T * CH)
assert FIRST_CLIP * T * CH < (1 << 34) < (FIRST_CLIP + 1) * T * CH


# ---- Philox4x32-10 + Box-Muller in NumPy ----------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: (N, 4) uint32 counters, key: (k0, k1).  Salmon et al. 2011; the key is bumped after every round."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).astype(np.uint32)


def randn_words(n, seed, stream_id, first_index):
    idx4 = np.arange(n // 4, dtype=np.uint64) + np.uint64(first_index // 4)
    sid = np.full_like(idx4, stream_id)
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    ctr = np.stack([idx4 & m32, idx4 >> s32, sid & m32, sid >> s32], 1).astype(np.uint32)
    return ctr, philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def box_muller(words):
    """fp64 Box-Muller of the uniforms the device forms in fp32: u = (float(word) + 0.5) 2^-32, pairs (words 0, 1), (2, 3)."""
    u = (words.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    u = u.astype(np.float64)
    z = np.empty(words.shape, np.float64)
    for p in range(2):
        rad = np.sqrt(-2.0 * np.log(u[:, 2 * p]))
        z[:, 2 * p] = rad * np.cos(2.0 * np.pi * u[:, 2 * p + 1])
        z[:, 2 * p + 1] = rad * np.sin(2.0 * np.pi * u[:, 2 * p + 1])
    return z.reshape(-1)


def test_numpy_philox_reproduces_the_known_answer_vectors():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert [int(v) for v in got] == list(want), (ctr, key, [hex(int(v)) for v in got])


@gpu
@pytest.mark.parametrize("seed", [9, 0xC0FFEE1234567])
@pytest.mark.parametrize("step", [0, 731])
@pytest.mark.parametrize("first", [(1 << 32) - 2048, (1 << 34) - 2048], ids=["element-index-crosses-2^32", "counter-high-word-sets"])
def test_syn_randn_vs_numpy_philox_box_muller(seed, step, first):
    """4096 values whose element index crosses 2^32, and whose Philox counter (index / 4) crosses 2^32 (the high counter word goes
    from 0 to 1 in the middle of the buffer).  Integer stage: see the module docstring.  Normals: 1e-6 relative (rel-L2, the
    figure this suite uses throughout) to the fp64 transform - the device uses v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32.
    And no single value off: |delta| <= 2e-6 everywhere, i.e. 1e-6 of the largest magnitude the transform reaches here
    (sqrt(-2 ln 2^-33) = 6.8, so 1e-6 relative to the value range is 6.8e-6; 2e-6 is four fp32 ulps of a value in [2, 4),
    what three chained hardware transcendentals of about one ulp each and the final product may leave)."""
    from syntalker_amd import _lib
    n = 4096
    ctr, words = randn_words(n, seed, step, first)
    if first == (1 << 34) - 2048:
        assert ctr[0, 1] == 0 and ctr[-1, 1] == 1 and ctr[512, 0] == 0           # the carry sits at element 2048
    want = box_muller(words)
    buf = torch.empty(n, device=DEV)
    _lib.check(_lib.load().syn_randn(buf.data_ptr(), n, seed, step, first, _lib.current_stream()), "syn_randn")
    got = buf.cpu().double().numpy()
    assert np.isfinite(got).all()
    e, worst = rel_l2(got, want), float(np.abs(got - want).max())
    print(f"syn_randn seed={seed:#x} step={step} first={first}: rel-L2 {e:.3e}, max |delta| {worst:.3e}, std {got.std():.4f}")
    assert e < 1e-6 and worst <= 2e-6


# ---- k_seq steps --------------------------------------------------------------------------------------------------------------
TS = [500, 463, 426]
SEED = 5


@pytest.fixture(scope="module")
def beatx():
    return _model("beatx")


@pytest.fixture(scope="module")
def steps_cache():
    return {}


def _inputs(B):
    return synth.synth_clip_inputs(B, seed=70 + B), synth.synth_latent(B, seed=70 + B)


def _run(cache, beatx, B, noise, persistent):
    """Three DDPM steps at TS on k_seq; returns x0_hat and x after the first step (single steps only), x and the bf16 shadow
    after the third."""
    key = (B, noise, persistent)
    if key in cache:
        return cache[key]
    from syntalker_amd import engine
    from syntalker_amd.process import create_gaussian_diffusion
    y, xT = _inputs(B)
    pm = beatx.packed()
    coef = engine.posterior_coefs(create_gaussian_diffusion().tables(), DEV)
    sb = engine.StepBuffers(B, 1, DEV, want_x0=True, layer_mode=5)
    assert sb.fragment
    sb.cond.copy_(beatx.variant_conds(synth.to_device(y, DEV), [(False, False, None)]).reshape(-1, 512))
    sb.load_x(xT.to(DEV)); sb.set_rng(SEED, FIRST_CLIP)
    use, fused = noise != "none", noise == "drawn"
    first = None
    if persistent:
        rows_m = torch.tensor(TS, dtype=torch.int32, device=DEV).view(-1, 1).repeat(1, B).contiguous()
        rows_c = rows_m.clone()
        try:
            sb.c.t_model, sb.c.t_coef = rows_m.data_ptr(), rows_c.data_ptr()
            engine.run_step(pm, sb, coef, use, fused_rng=fused, steps=len(TS))
        finally:
            sb.c.t_model, sb.c.t_coef = sb.t_model.data_ptr(), sb.t_coef.data_ptr()
    else:
        for i, t in enumerate(TS):
            sb.t_model.fill_(t); sb.t_coef.fill_(t)
            if noise == "read":
                sb.draw_noise(SEED, t, first_clip=FIRST_CLIP)
            engine.run_step(pm, sb, coef, use, fused_rng=fused)
            if i == 0:
                first = (sb.read(sb.x0).cpu(), sb.read(sb.x).cpu())
    torch.cuda.synchronize()
    cache[key] = (first, sb.read(sb.x).cpu(), sb.xb.clone().cpu())
    return cache[key]


def _oracle(cache, B, noisy):
    """The same three steps on the CPU oracle, fed the noise syn_randn draws for (SEED, t, FIRST_CLIP)."""
    key = ("oracle", B, noisy)
    if key in cache:
        return cache[key]
    from oracle import denoiser_ref as dr
    from oracle.process_ref import RefProcess
    from syntalker_amd import _lib
    y, x = _inputs(B)
    sd = synth_state_dict("beatx")
    ref = RefProcess(False)
    out = []
    with torch.no_grad():
        for t in TS:
            eps = torch.zeros(B, CH, 1, T)
            if noisy:
                buf = torch.empty(B, T, CH, device=DEV)
                _lib.check(_lib.load().syn_randn(buf.data_ptr(), buf.numel(), SEED, t, FIRST_CLIP * T * CH, _lib.current_stream()), "syn_randn")
                eps = buf.transpose(1, 2).reshape(B, CH, 1, T).cpu()
            x, x0 = ref.p_sample(lambda a, b, c: dr.mdm_forward(sd, a, b, c), x, torch.full((B,), t, dtype=torch.long), y, eps)
            out.append((x0, x))
    cache[key] = out
    return out


@gpu
@pytest.mark.parametrize("noise", ["none", "read", "drawn"])
@pytest.mark.parametrize("B", [1, 5, 6])
def test_steps_at_idle_and_ragged_shapes(beatx, steps_cache, B, noise):
    """B = 1: three waves idle; 5: a second workgroup with one live wave; 6: two waves of the second workgroup idle.  One step
    and three steps against the oracle; the 3-step persistent launch against three launches, bitwise (injected noise is per
    step, so that combination has no persistent form); drawn against injected noise, bitwise, in x and in the bf16 shadow."""
    first, x3, xb3 = _run(steps_cache, beatx, B, noise, False)
    want = _oracle(steps_cache, B, noise != "none")
    e0, e1, e3 = rel_l2(first[0], want[0][0]), rel_l2(first[1], want[0][1]), rel_l2(x3, want[2][1])
    print(f"k_seq B={B} noise={noise}: x0_hat {e0:.3e}, x after 1 step {e1:.3e}, after 3 steps {e3:.3e} (rel-L2 vs oracle)")
    assert torch.isfinite(x3).all()
    assert e0 < FWD_TOL and e1 < LOOP_TOL and e3 < LOOP_TOL
    if noise != "read":
        _, xp, xbp = _run(steps_cache, beatx, B, noise, True)
        assert torch.equal(xp, x3) and torch.equal(xbp, xb3)
    if noise == "drawn":
        fr, xr, xbr = _run(steps_cache, beatx, B, "read", False)
        assert torch.equal(fr[1], first[1]) and torch.equal(xr, x3) and torch.equal(xbr, xb3)
        # and the noise did something: the deterministic update is somebody else
        assert not torch.equal(_run(steps_cache, beatx, B, "none", False)[1], x3)


@gpu
def test_guided_two_variants_three_clips():
    """V = 2, B = 3: two clips per workgroup, the second workgroup half empty.  One noisy guided step against the token-resident
    kernel (x0_hat and x within 1.5e-2, as in tests/test_gpu_seq.py), and one 3-step persistent launch against three launches."""
    from syntalker_amd import engine
    from syntalker_amd.process import create_gaussian_diffusion
    V, B = 2, 3
    m = _model("h3d")
    pm = m.packed()
    coef = engine.posterior_coefs(create_gaussian_diffusion().tables(), DEV)
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(V * B * 32, 512, generator=g).to(DEV) * 0.5
    w = torch.tensor([[2.5, -1.5], [1.0, 0.0], [0.5, 0.5]])               # every row sums to 1, as every guidance formula does
    xT = synth.synth_latent(B, seed=61).to(DEV)
    tm = (torch.arange(V * B) % B * 97 + 300).int().to(DEV)               # a clip's variants share its timestep

    def run(mode, steps=1, replays=1, want_x0=False):
        sb = engine.StepBuffers(B, V, DEV, want_x0=want_x0, layer_mode=mode)
        sb.cond.copy_(cond); sb.cfg_w.copy_(w.to(DEV)); sb.set_rng(11, FIRST_CLIP)
        if steps == 1 and replays == 1:
            sb.load_x(xT); sb.t_model.copy_(tm); sb.t_coef.copy_(tm[:B])
            engine.run_step(pm, sb, coef, True, fused_rng=True)
        else:
            gr = engine.StepGraph(pm, sb, coef, True, fused_rng=True, scheduled=True, steps=steps)
            sb.load_x(xT)
            ts = [500 - 41 * i for i in range(steps * replays)]
            gr.set_schedule(ts, ts)
            for _ in range(replays):
                gr.replay()
        return sb.read(sb.x).cpu(), (sb.read(sb.x0).cpu() if want_x0 else None), sb.xb.clone().cpu()

    x5, x05, _ = run(5, want_x0=True)
    x4, x04, _ = run(4, want_x0=True)
    e0, e = rel_l2(x05, x04), rel_l2(x5, x4)
    print(f"guided V={V} B={B}: k_seq vs k_stack rel-L2 x0_hat {e0:.3e}, x {e:.3e}")
    assert e0 < 1.5e-2 and e < 1.5e-2
    a, _, ab = run(5, steps=1, replays=3)
    b, _, bb = run(5, steps=3, replays=1)
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(ab, bb)
