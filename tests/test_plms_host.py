"""PLMS sampler, host side (no GPU): `engine.plms_coefs` against the reference's update written out from the recorded tables, the launch
tables executed in numpy against the generic path, the ValueErrors and the signatures."""
import inspect
import os

import numpy as np
import pytest
import torch

from syntalker_amd import engine, process

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
AB = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


def ref_tables():
    g = np.load(os.path.join(GOLD, "tables.npz"))
    return {k[len("ddim."):]: g[k] for k in g.files if k.startswith("ddim.")}


def ref_update(tab, t, x, x0, olds, cur_order):
    """gaussian_diffusion.py:1047, 1064-1078 as written: olds = earlier estimates, newest last."""
    eps = (tab["sqrt_recip_alphas_cumprod"][t] * x - x0) / tab["sqrt_recipm1_alphas_cumprod"][t]
    es = list(olds) + [eps]
    a = AB[cur_order]
    eps_prime = sum(a[k] * es[-1 - k] for k in range(cur_order))
    pred = tab["sqrt_recip_alphas_cumprod"][t] * x - tab["sqrt_recipm1_alphas_cumprod"][t] * eps_prime
    abp = tab["alphas_cumprod_prev"][t]
    return pred * np.sqrt(abp) + np.sqrt(1 - abp) * eps_prime, eps


def relerr(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize("order", [2, 3, 4])
def test_plms_coefs_match_the_reference_update_at_every_step(order):
    tab = ref_tables()
    n = len(tab["betas"])
    assert n == 50
    c = engine.plms_coefs(tab, order, n)
    assert c["coef"].dtype == np.float64 and len(c["coef"]) == n + 1
    worst = 0.0
    # the Euler start (:1054-1061) over the basis (x_T, x0_hat of call 1, x0_hat of call 2)
    t0, I = n - 1, np.eye(3)
    eps1 = (tab["sqrt_recip_alphas_cumprod"][t0] * I[0] - I[1]) / tab["sqrt_recipm1_alphas_cumprod"][t0]
    abp = tab["alphas_cumprod_prev"][t0]
    mid = I[1] * np.sqrt(abp) + np.sqrt(1 - abp) * eps1
    eps2 = (tab["sqrt_recip_alphas_cumprod"][t0 - 1] * mid - I[2]) / tab["sqrt_recipm1_alphas_cumprod"][t0 - 1]
    ep = (eps1 + eps2) / 2
    want = (tab["sqrt_recip_alphas_cumprod"][t0] * I[0] - tab["sqrt_recipm1_alphas_cumprod"][t0] * ep) * np.sqrt(abp) + np.sqrt(1 - abp) * ep
    y = c["coef"][0, 0] * I[1] + c["coef"][0, 1] * I[0]
    h0 = c["hist"][0]
    e_kept = (h0[0] * I[0] - I[1]) * h0[1]
    H = h0[2] * I[0] + h0[3] * e_kept
    got = c["coef"][1, 0] * I[2] + c["coef"][1, 1] * y + c["coef"][1, 2] * H
    worst = max(worst, relerr(got, want), relerr(y, mid), relerr(e_kept, eps1))
    assert c["coef"][0, 2] == 0 and list(c["t"][:2]) == [t0, t0 - 1] and c["store"][0] == 0 and c["store"][1] == -1
    assert not c["hist"][1, 2:4].any()                      # launch 1 keeps nothing and takes nothing from its own registers
    # every later step over the basis (x_t, x0_hat, e_-1, e_-2, e_-3); the ring's contents are followed by estimate number
    ring = {0: 0}                                           # slot -> estimate (0: the start's e_1, j: step j's)
    for j in range(1, n):
        t, row, cur = n - 1 - j, j + 1, min(order, j + 1)
        assert c["t"][row] == t and c["order"][row] == cur
        I = np.eye(5)
        olds = [I[1 + k] for k in range(cur - 1, 0, -1)]                      # oldest first; I[2] = e_{j-1}
        want, _ = ref_update(tab, t, I[0], I[1], olds, cur)
        if t == 0:
            want = I[1]                                                         # nonzero_mask (:1083-1084): the sample is pred_xstart
        # H as the PREVIOUS update left it: weights by ring slot + the estimate that was still in its registers (step j - 1's)
        prev = c["hist"][row - 1]
        H = np.zeros(5)
        if prev[3] != 0:
            assert j >= 2
            H += prev[3] * I[2]
        for slot in range(3):
            if prev[4 + slot] != 0:
                k = j - ring[slot]                                              # that slot holds e_{j-k}
                assert 1 <= k <= 3 and not (k == 1 and j >= 2), (j, slot, ring)
                H += prev[4 + slot] * I[1 + k]
        got = c["coef"][row, 0] * I[1] + c["coef"][row, 1] * I[0] + c["coef"][row, 2] * H
        mask = want != 0
        assert not got[~mask].any(), (j, got, want)
        worst = max(worst, relerr(got[mask], want[mask]))
        if t == 0:
            assert tuple(c["coef"][row]) == (1.0, 0.0, 0.0, 0.0)
        # the row's own (r, 1 / m) and where its estimate goes
        assert c["hist"][row, 0] == tab["sqrt_recip_alphas_cumprod"][t] and abs(c["hist"][row, 1] * tab["sqrt_recipm1_alphas_cumprod"][t] - 1) < 1e-15
        if c["store"][row] >= 0:
            assert c["store"][row] == j % 3
            ring[int(c["store"][row])] = j
    print(f"order {order}: worst relative error on a coefficient {worst:.3e}")
    assert worst <= 1e-12
    # the current order ramps 1 (Euler), 2, 3, 4 and stays
    assert list(c["order"][:6]) == [1, 1] + [min(order, k) for k in (2, 3, 4, 5)]
    if order == 4:                                          # three estimates live: the slots rotate with the step counter
        assert list(c["store"][2:8]) == [1, 2, 0, 1, 2, 0]
    if order == 2:                                          # the one earlier estimate never leaves the update's registers
        assert (c["store"][1:] == -1).all()


def test_first_order_row_without_history_is_the_ddim_row():
    """a_0 = 1, H = 0 is DDIM with eta = 0: launch 0 of any loop is that row (the start's first model call is a DDIM step)."""
    tab = ref_tables()
    ddim = engine.ddim_coefs(tab, 0.0, "cpu").double().numpy()
    for n in (2, 10, 50):
        c = engine.plms_coefs(tab, 3, n)
        assert np.allclose(c["coef"][0, :2], ddim[n - 1, :2], rtol=2e-7, atol=0) and c["coef"][0, 2] == 0
    r, m = tab["sqrt_recip_alphas_cumprod"], tab["sqrt_recipm1_alphas_cumprod"]
    p, q = np.sqrt(tab["alphas_cumprod_prev"]), np.sqrt(1 - tab["alphas_cumprod_prev"])
    beta = q - p * m
    assert np.allclose(np.stack([-beta / m, r * (p + beta / m)], 1)[1:], ddim[1:, :2], rtol=2e-7, atol=1e-9)


class Toy(torch.nn.Module):
    def forward(self, x, t, y=None):
        return 0.8 * torch.tanh(x) + 0.0005 * t.view(-1, 1, 1, 1).to(x.dtype)


def run_tables(c, model, tmap, x):
    """The launches of a loop as the device runs them: step kernel row, then the history update; the steps ping-pong between two
    latents (numpy, fp64)."""
    lat, ring, H = [x.numpy(), None], [None] * 3, 0.0
    samples = []
    for L in range(len(c["store"])):
        src = L if L < 2 else L % 2
        xt = lat[src]
        x0 = model(torch.from_numpy(xt), torch.full((x.shape[0],), int(tmap[c["t"][L]]))).numpy()
        lat[1 - src] = c["coef"][L, 0] * x0 + c["coef"][L, 1] * xt + c["coef"][L, 2] * H
        h = c["hist"][L]
        if c["store"][L] >= 0 or h[2:].any():
            e = (h[0] * xt - x0) * h[1]
            H = h[2] * xt + h[3] * e + sum(h[4 + k] * ring[k] for k in range(3) if h[4 + k] != 0)
            if c["store"][L] >= 0:
                ring[c["store"][L]] = e
        if L >= 1:
            samples.append(lat[1 - src])
    return samples


@pytest.mark.parametrize("order,skip", [(2, 0), (3, 0), (4, 0), (4, 44), (3, 48)])
def test_launch_tables_run_like_the_generic_path(order, skip):
    """Both in fp64 (the generic path's table gather made fp64 for this test: near t = 0 its fp32 eps = (r x - x0) / m cancels)."""
    d = process.create_gaussian_diffusion(use_ddim=True)
    d._tab = lambda name, t, like: torch.from_numpy(getattr(d, name))[t].view(-1, *([1] * (like.dim() - 1)))
    torch.manual_seed(3)
    x = torch.randn(2, 8, 1, 4, dtype=torch.float64)
    n = d.num_timesteps - skip
    want, old, img = [], None, x
    for i in range(n - 1, -1, -1):
        old = d.plms_sample(Toy(), img, torch.full((2,), i), clip_denoised=False, order=order, old_out=old)
        img = old["sample"]
        want.append(img.numpy())
    got = run_tables(engine.plms_coefs(d.tables(), order, n), Toy(), d.timestep_map, x)
    assert len(got) == len(want) == n
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b), k


def test_generic_step_returns_the_reference_dictionary():
    d = process.create_gaussian_diffusion(use_ddim=True)
    x = torch.randn(1, 8, 1, 4)
    outs = list(d.plms_sample_loop_progressive(Toy(), x.shape, noise=x, clip_denoised=False, device="cpu", order=3, skip_timesteps=44))
    assert all(set(o) == {"sample", "pred_xstart", "old_eps"} for o in outs)
    assert len(outs[-1]["old_eps"]) == 2                    # (one list, extended and trimmed in place like the reference's)
    assert torch.equal(outs[-1]["sample"], outs[-1]["pred_xstart"])
    assert torch.equal(d.plms_sample_loop(Toy(), x.shape, noise=x, clip_denoised=False, device="cpu", order=3, skip_timesteps=44), outs[-1]["sample"])
    assert d.last_path == "generic"


def test_invalid_order_raises_value_error():
    d = process.create_gaussian_diffusion(use_ddim=True)
    x = torch.zeros(1, 8, 1, 4)
    for bad in (0, 5, -1, 2.5, "2", None):
        with pytest.raises(ValueError, match="order is invalid"):
            d.plms_sample_loop(Toy(), x.shape, noise=x, device="cpu", order=bad)
        with pytest.raises(ValueError, match="order is invalid"):
            d.plms_sample(Toy(), x, torch.tensor([5]), order=bad)
        with pytest.raises(ValueError, match="order is invalid"):
            next(d.plms_sample_loop_progressive(Toy(), x.shape, noise=x, device="cpu", order=bad))


def test_order_one_raises_value_error_naming_the_reference_line():
    d = process.create_gaussian_diffusion(use_ddim=True)
    x = torch.zeros(1, 8, 1, 4)
    with pytest.raises(ValueError, match=r"gaussian_diffusion\.py:1064"):
        d.plms_sample_loop(Toy(), x.shape, noise=x, device="cpu", order=1)
    with pytest.raises(ValueError, match=r"gaussian_diffusion\.py:1064"):
        d.plms_sample(Toy(), x, torch.tensor([5]), order=1)


def test_loop_of_fewer_than_two_steps_raises_value_error():
    d = process.create_gaussian_diffusion(use_ddim=True)
    x = torch.zeros(1, 8, 1, 4)
    for skip in (49, 50):
        with pytest.raises(ValueError, match="at least 2 steps"):
            d.plms_sample_loop(Toy(), x.shape, noise=x, device="cpu", order=2, skip_timesteps=skip)
        with pytest.raises(ValueError, match="at least 2 steps"):
            next(d.plms_sample_loop_progressive(Toy(), x.shape, noise=x, device="cpu", order=2, skip_timesteps=skip))
    with pytest.raises(ValueError):
        engine.plms_coefs(d.tables(), 2, 1)
    with pytest.raises(ValueError):
        engine.plms_coefs(d.tables(), 1, 10)
    with pytest.raises(NotImplementedError):
        d.plms_sample_loop(Toy(), x.shape, noise=x, device="cpu", cond_fn=lambda *a, **k: 0)


def test_signatures_equal_the_reference_parameters_plus_keyword_only_extras():
    want = {s.split("(", 1)[0]: s.split("(", 1)[1][:-1] for s in np.load(os.path.join(GOLD, "plms_outputs.npz"))["signatures"]}
    extras = {"plms_sample": [], "plms_sample_loop_progressive": [], "plms_sample_loop": ["seed", "first_clip"]}
    for name, ref in want.items():
        ps = [p for p in inspect.signature(getattr(process.SpacedDiffusion, name)).parameters.values() if p.name != "self"]
        pos = [p for p in ps if p.kind is p.POSITIONAL_OR_KEYWORD]
        assert ",".join(p.name + ("" if p.default is p.empty else "=" + repr(p.default)) for p in pos) == ref, name
        assert [p.name for p in ps if p.kind is p.KEYWORD_ONLY] == extras[name] and len(ps) == len(pos) + len(extras[name])


def test_a_call_that_does_not_bind_is_a_type_error_that_still_names_the_reference_line():
    d = process.create_gaussian_diffusion()
    for name in ("plms_sample", "plms_sample_loop", "plms_sample_loop_progressive"):
        for exc in (TypeError, NotImplementedError):
            with pytest.raises(exc, match=r"gaussian_diffusion\.py:1\d\d\d.*missing"):
                getattr(d, name)(None)
        with pytest.raises(TypeError, match="unexpected keyword"):
            getattr(d, name)(None, None, None, steps=3)


def test_update_entry_point_refuses_bad_arguments():
    import ctypes
    from syntalker_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.SynPlmsRow) == 32 and _lib.SynPlmsRow.store.offset == 28
    ok = dict(table=256, n_rows=4, counter=256, back=1, x=256, x0=256, ring=256, h=256, n=64)
    for k, v in (("table", None), ("n_rows", 0), ("counter", None), ("back", -1), ("x", None), ("x0", None), ("ring", None), ("h", None),
                 ("n", 0), ("n", 6), ("x", 260)):
        a = dict(ok, **{k: v})
        assert lib.syn_plms_update(a["table"], a["n_rows"], a["counter"], a["back"], a["x"], a["x0"], a["ring"], a["h"], a["n"], None) != 0, k
        assert b"syn_plms_update" in lib.syn_last_error()
