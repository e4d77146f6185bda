"""The denoising-step kernels at the ranges trained checkpoints reach and the synthetic weights never do (tests/outlier_weights.py: fc1
pre-activations up to |27|, softmaxes with a median top probability of 0.92, residual-stream channels at |115|, a residual stream with
mean^2 / variance = 547): one model evaluation per test on every step kernel, against the fp64 CPU oracle, under the bound every other
evaluation here is held to (tests/test_gpu_parity.FWD_TOL).  tests/test_ranges_host.py holds the kernels' arithmetic to half that bound on the CPU."""
import pytest
import torch

from oracle import denoiser_ref as dr
from syntalker_amd import synth
from tests.conftest import rel_l2
from tests.outlier_weights import CASES, hazard_state_dict
from tests.test_gpu_parity import DEV, FWD_TOL

pytestmark = pytest.mark.gpu
N_CLIPS = 9                      # the largest batch below; the smaller ones are its first clips


def _f64(y):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in y.items()}


def _load(variant, sd):
    if variant == "h3d":
        from syntalker_amd.denoiser_h3d import MDM
    else:
        from syntalker_amd.denoiser import MDM
    m = MDM(synth.default_args()).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(DEV)


@pytest.fixture(scope="module")
def inputs():
    return synth.synth_clip_inputs(N_CLIPS, seed=5), synth.synth_latent(N_CLIPS, seed=5), (torch.arange(N_CLIPS) * 53 + 1) % 1000


@pytest.fixture(scope="module")
def hazard(inputs):
    """case -> (model on the hazard weights, fp64 oracle's evaluation of the nine clips): built on first use, once per case."""
    cache = {}

    def get(case):
        if case not in cache:
            sd = hazard_state_dict(case)
            y, x, t = inputs
            with torch.no_grad():
                want = dr.mdm_forward(dr.cast_sd(sd, torch.float64), x.double(), t, _f64(y))
            cache[case] = (_load("beatx", sd), want)
        return cache[case]

    yield get
    cache.clear()


# (layer_mode, clips): k_seq with fewer sequences than waves, and two workgroups with a ragged second one; k_stack on whole tiles with a ragged
# 64-row tile; k_stack at the smallest batch whose tiles plan_step splits over an XCD; k_lat with fewer clips than XCD groups, and uneven groups;
# the per-operation path k_stack is pinned to bit for bit
KERNELS = [(5, 1), (5, 5), (4, 3), (0, 9), (3, 1), (3, 5), (1, 2)]
KERNEL_IDS = ["k_seq-1", "k_seq-5", "k_stack-whole-tiles-3", "k_stack-split-tiles-9", "k_lat-1", "k_lat-5", "per-operation-2"]


@pytest.mark.parametrize("mode,B", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", CASES)
def test_forward_on_hazard_weights_vs_fp64_oracle(hazard, inputs, case, mode, B):
    model, want = hazard(case)
    y, x, t = inputs
    yb = synth.to_device({k: (v[:B] if torch.is_tensor(v) else v) for k, v in y.items()}, DEV)
    model.layer_mode = mode
    try:
        sb = model.step_buffers(B, 1)
        assert sb.fragment == (mode == 5)
        if mode == 0:                     # split tiles exchange partial residual streams through ws_xch, and nothing else touches it
            sb.xch.fill_(-12345.0)
        with torch.no_grad():
            got = model(x[:B].to(DEV), t[:B].to(DEV), yb).cpu()
        if mode == 0:
            assert bool((sb.xch != -12345.0).any()), "plan_step did not split the tiles of this batch"
    finally:
        model.layer_mode = 0
    e = rel_l2(got.double(), want[:B])
    print(f"{case} weights, layer_mode {mode}, {B} clips: rel-L2 vs fp64 oracle {e:.3e}")
    assert torch.isfinite(got).all() and e < FWD_TOL


def test_guided_forward_on_gelu_hazard_weights_vs_fp64_oracle():
    """The text-prompt variant, two clips x two conditioning variants on the wave-per-sequence kernel (a clip's variants are waves of one
    workgroup and meet in the output stage): x0_hat against the fp64 recombination of the oracle's folded forward on the same cond rows."""
    from syntalker_amd import engine
    B, V = 2, 2
    sd = hazard_state_dict("gelu", "h3d")
    m = _load("h3d", sd)
    g = torch.Generator().manual_seed(5)
    cond = torch.randn(V * B * 32, 512, generator=g) * 0.5
    w = torch.tensor([[2.5, -1.5]] * 3)
    x, t = synth.synth_latent(B, seed=5), (torch.arange(B) * 53 + 1) % 1000
    sb = engine.StepBuffers(B, V, DEV, want_x0=True, layer_mode=5)
    assert sb.fragment
    sb.cond.copy_(cond); sb.cfg_w.copy_(w.to(DEV)); sb.load_x(x.to(DEV))
    sb.t_model.copy_(t.int().repeat(V)); sb.t_coef.zero_()               # a clip's variants share its timestep
    engine.run_step(m.packed(), sb, engine.identity_coefs(DEV), False)
    x0 = sb.read(sb.x0).cpu()
    sd64 = dr.cast_sd(sd, torch.float64)
    fw = dr.fold_weights(sd64, variant="h3d")
    want = torch.zeros(B, 1536, 1, 32, dtype=torch.float64)
    with torch.no_grad():
        te = dr.time_table(sd64, fw)
        for v in range(V):
            xv = dr.mdm_forward_folded(sd64, fw, cond.double().view(V, B, 32, 512)[v], te, x.double(), t)
            for c in range(3):
                want[:, 512 * c:512 * (c + 1)] += float(w[c, v]) * xv[:, 512 * c:512 * (c + 1)]
    e = rel_l2(x0.double(), want)
    print(f"guided, gelu weights, V = {V}, {B} clips on k_seq: x0_hat rel-L2 vs fp64 recombination {e:.3e}")
    assert torch.isfinite(x0).all() and e < FWD_TOL
