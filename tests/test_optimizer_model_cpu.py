"""``tests/optimizer_model.py`` on the CPU: the float64 model is torch's clipped AdamW, and the float32 twin of the
kernel's statements stays within HALF of ``bound`` on every input of the table -- the condition that fixes the bound
before any kernel is held to it (``tests/test_gpu_optimizer_epoch.py``)."""
import numpy as np
import pytest
import torch

import optimizer_model as om

N = 9372                    # parameters of maf3 at D = 10


@pytest.mark.parametrize("kind", om.STATES)
@pytest.mark.parametrize("lr,wd,max_norm", [(1e-3, 0.01, 1.0), (2e-4, 0.0, 0.0), (1e-3, 0.01, 1e9), (1e-6, 0.01, 1e-3)])
def test_step64_is_torch_clip_and_adamw_in_float64(kind, lr, wd, max_norm):
    """Five consecutive steps of ``clip_grad_norm_`` + ``torch.optim.AdamW`` on float64 tensors with the float32-rounded
    hyper-parameters: 1e-12 relative.  (torch takes the bias corrections from those betas in double, so the model gets
    them unrounded here; rounding them to float32 as the launcher does moves the step by a float32 rounding, below.)"""
    f32 = lambda x: float(np.float32(x))
    p, g, m, v = (a.astype(np.float64) for a in om.state(kind, N, seed=1))
    pt = torch.tensor(p, requires_grad=True)
    opt = torch.optim.AdamW([pt], lr=f32(lr), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(wd))
    rng = np.random.default_rng(3)
    m, v = np.zeros(N), np.zeros(N)                                   # torch starts its moments at zero
    for step in range(1, 6):
        gs = g * rng.uniform(0.5, 1.5, size=N)            # (one sign per entry: a moment that cancels has no relative error)
        pt.grad = torch.tensor(gs)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], f32(max_norm))
        opt.step()
        sc = om.scalars(step, f32(lr), f32(wd), f32(max_norm), f32(0.9), f32(0.999), f32(1e-8), rounded=False)
        p, m, v = om.step64(p, gs, m, v, sc)
        st = opt.state[pt]
        for got, want in ((p, pt.detach().numpy()), (m, st["exp_avg"].numpy()), (v, st["exp_avg_sq"].numpy())):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # the launcher's scalars: the same six hyper-parameters; its corrections come from the double betas, as torch's own
    # float32 optimizer takes them (1 - 0.999 against 1 - float32(0.999): 4.7e-5 apart at step 1)
    for step in (1, 2, 10, 10000):
        a = om.scalars(step, lr, wd, max_norm)
        assert a[:6] == om.scalars(step, f32(lr), f32(wd), f32(max_norm), f32(0.9), f32(0.999), f32(1e-8), rounded=False)[:6]
        assert a.bc1 == f32(1.0 - 0.9 ** step) and a.bc2 == f32(1.0 - 0.999 ** step)


def test_the_partials_stand_in_for_the_squared_gradient():
    p, g, m, v = om.state("mixed", N)
    sc = om.scalars(3, 1e-3, 0.01, 1.0)
    part = np.add.reduceat(g.astype(np.float64) ** 2, np.arange(0, N, 100))
    for a, b in zip(om.step64(p, g, m, v, sc), om.step64(p, g, m, v, sc, partials=part)):
        np.testing.assert_allclose(a, b, rtol=1e-13)
    # a double-counted partial shortens the step: the model notices what the suite is there to notice
    twice = np.concatenate([part, part[:1]])
    assert om.coefficient64(g, sc, twice) < om.coefficient64(g, sc, part)
    assert om.coefficient64(g, om.scalars(3, 1e-3, 0.01, 0.0)) == 1.0 == om.coefficient64(g, om.scalars(3, 1e-3, 0.01, 1e9))


def test_the_twins_sums_add_what_the_kernels_add():
    rng = np.random.default_rng(0)
    for n in (1, 58, 256, 257, 425, 862):
        part = rng.uniform(0.0, 3.0, size=n).astype(np.float32)
        exact = part.astype(np.float64).sum()
        assert abs(float(om.sum_partials32(part)) - exact) <= (n / 256 + 8) * om.U * exact
    for n in (5, 65536, 65537, 313944):
        g = rng.normal(size=n).astype(np.float32)
        for fused in (False, True):
            part = om.sq_partials32(g, fused)
            assert part.shape == (256,) and part.dtype == np.float32
            exact = (g.astype(np.float64) ** 2).sum()
            assert abs(part.astype(np.float64).sum() - exact) <= om.sq_depth(n) * om.U * exact


RATIOS = {}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", om.STATES)
@pytest.mark.parametrize("n,seed", [(9372, 0), (9372, 1), (70000, 0)])
def test_both_twins_stay_within_half_of_the_bound(kind, n, seed, fused):
    """Every input of the table, with the device-style partials (the twin's own float32 partials handed to the model) and
    without (the model squares the gradient itself)."""
    p, g, m, v = om.state(kind, n, seed)
    worst = 0.0
    for step, lr, wd, max_norm in om.HYPER:
        sc = om.scalars(step, lr, wd, max_norm)
        part = om.sq_partials32(g, fused)
        for partials, extra in ((part, 0), (None, om.sq_depth(n))):
            got = om.step32(p, g, m, v, sc, partials=part, fused=fused)
            want = om.step64(p, g, m, v, sc, partials)
            bnd = om.bound(p, g, m, v, sc, partials, n_part=part.size, sq_roundings=extra)
            r = om.worst_ratio(got, want, bnd)
            assert r <= 0.5, (kind, n, step, lr, wd, max_norm, fused, partials is None, r)
            worst = max(worst, r)
    RATIOS[(kind, n, seed, fused)] = worst
    print(f"twin/bound {kind} n={n} seed={seed} fused={int(fused)}: {worst:.3f}")


def test_a_wrong_step_leaves_the_bound():
    """What the bound is for: a partial counted twice, a stale bias correction and a skipped weight decay all leave it."""
    p, g, m, v = om.state("mixed", N)
    sc = om.scalars(10, 1e-3, 0.01, 1.0)
    part = om.sq_partials32(g)
    want, bnd = om.step64(p, g, m, v, sc, part), om.bound(p, g, m, v, sc, part)
    assert om.worst_ratio(om.step32(p, g, m, v, sc, part), want, bnd) <= 0.5
    twice = part.copy()
    twice[np.argmax(part)] *= 2
    assert om.worst_ratio(om.step32(p, g, m, v, sc, twice), want, bnd) > 1.0
    assert om.worst_ratio(om.step32(p, g, m, v, om.scalars(9, 1e-3, 0.01, 1.0), part), want, bnd) > 1.0
    assert om.worst_ratio(om.step32(p, g, m, v, om.scalars(10, 1e-3, 0.0, 1.0), part), want, bnd) > 1.0
