"""Distribution tests of the counter-based generator the throughput path (and bench.py) runs.

The reference draws from numpy's sequential legacy stream -- ``np.random.gamma`` per walker
(``pocomc/mcmc.py:80``), ``np.random.randn(D)`` per walker (``:85``), ``np.random.rand(N)`` (``:137``) -- which
a parallel kernel cannot reproduce by seed: trajectories are pinned in replay mode, and
the Philox draws are pinned HERE as distributions: Kolmogorov-Smirnov against the exact laws at N >= 1e5,
moments, and independence between seeds / steps / walkers / variate families.

``pmc_rng_fill`` writes exactly the variates the kernels draw inline for the same (seed, step, offset)
(``test_gpu_mcmc.py::test_variates_drawn_ahead_equal_inline_draws``), so these are the kernels' numbers.
Everything is deterministic (fixed seeds): the KS thresholds are p > 1e-3 for every one of the fixed draws.

The laws are pinned here; the VALUES -- which number a (seed, step, walker, stream, draw) yields: the cipher, the
counter layout, the conversions -- are pinned by the host model ``tests/philox_model.py``
(``tests/test_philox_model_cpu.py``, ``tests/test_gpu_philox_model.py``).
"""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats

pytestmark = pytest.mark.gpu

N = 200_000
P_MIN = 1e-3


def fill(seed, step, offset, n, D, gamma_shape=0.0, want_uniform=True):
    from pocomc_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    r = _lib.pmc_rng_t(gamma=None, normal=None, uniform=None, seed=seed, step=step, offset=offset)
    z = torch.empty(n, D, dtype=torch.float64, device="cuda")
    g = torch.empty(n, dtype=torch.float64, device="cuda") if gamma_shape > 0 else None
    u = torch.empty(n, dtype=torch.float64, device="cuda") if want_uniform else None
    _lib.check(lib.pmc_rng_fill(C.byref(r), float(gamma_shape), _lib.ptr(z), _lib.ptr(g) if g is not None else None,
                                _lib.ptr(u) if u is not None else None, n, D, _lib.stream_handle()), "pmc_rng_fill")
    torch.cuda.synchronize()
    return (z.cpu().numpy(), None if g is None else g.cpu().numpy(), None if u is None else u.cpu().numpy())


# shape = (D + nu) / 2 (mcmc.py:80): D=32, nu=5 (bench) -> 18.5; nu clamped to 1e6 (geometry.py:58-59) -> 500016;
# D=2, nu=1 -> 1.5; below one (Marsaglia-Tsang boost branch) 0.5 -- not reachable from mcmc.py (D >= 2), kept honest;
# the ends of a Student-t EM fit's nu (Geometry(student="em")): D=2 and D=5 at the lower clamp 0.1 -> 1.05, 2.55; D=10 at 1e4 -> 5005
@pytest.mark.parametrize("shape", [18.5, 500016.0, 1.5, 21.0, 0.5, 1.05, 2.55, 5005.0])
def test_gamma_draws_follow_the_gamma_law(shape):
    _, g, _ = fill(seed=20240928, step=3, offset=0, n=N, D=2, gamma_shape=shape)
    assert np.isfinite(g).all() and (g > 0).all()
    ks = stats.kstest(g, stats.gamma(a=shape).cdf)
    assert ks.pvalue > P_MIN, (shape, ks)
    # first three moments: mean = var = shape, skewness 2/sqrt(shape)
    se_mean = np.sqrt(shape / N)
    assert abs(g.mean() - shape) < 5 * se_mean
    assert abs(g.var() / shape - 1) < 5 * np.sqrt((2 + 6 / shape) / N)
    assert abs(stats.skew(g) - 2 / np.sqrt(shape)) < 5 * np.sqrt(6.0 / N) + 0.02
    # the scale draw of the step: s = 1 / (2/(nu+delta) * g)  ->  1/s ~ Gamma(shape, 2/(nu+delta)) (mcmc.py:80)
    if shape == 18.5:
        nu, delta = 5.0, 27.0
        inv_s = (2.0 / (nu + delta)) * g
        assert stats.kstest(inv_s, stats.gamma(a=shape, scale=2.0 / (nu + delta)).cdf).pvalue > P_MIN


@pytest.mark.parametrize("D", [2, 5, 32])
def test_normal_draws_are_standard_normal(D):
    n = max(N // D, 20_000)
    z, _, _ = fill(seed=7, step=11, offset=12345, n=n, D=D, want_uniform=False)
    flat = z.ravel()
    assert stats.kstest(flat, "norm").pvalue > P_MIN
    # every coordinate on its own (Box-Muller pairs: even = r cos, odd = r sin)
    for j in range(D):
        assert stats.kstest(z[:, j], "norm").pvalue > P_MIN / D, j
    m = flat.size
    assert abs(flat.mean()) < 5 / np.sqrt(m)
    assert abs(flat.var() - 1) < 5 * np.sqrt(2.0 / m)
    assert abs(stats.kurtosis(flat)) < 5 * np.sqrt(24.0 / m)
    # coordinates of one walker are uncorrelated (also inside a Box-Muller pair), and so are neighbouring walkers
    c = np.corrcoef(z.T)
    off = c[~np.eye(D, dtype=bool)]
    assert np.abs(off).max() < 5 / np.sqrt(n)
    assert abs(np.corrcoef(z[:-1, 0], z[1:, 0])[0, 1]) < 5 / np.sqrt(n)
    # r^2 = z0^2 + z1^2 of a pair is chi2(2) and its angle uniform
    r2 = z[:, 0] ** 2 + z[:, 1] ** 2
    assert stats.kstest(r2, stats.chi2(2).cdf).pvalue > P_MIN
    ang = (np.arctan2(z[:, 1], z[:, 0]) / (2 * np.pi)) % 1.0
    assert stats.kstest(ang, "uniform").pvalue > P_MIN


def test_uniform_draws_are_uniform():
    _, _, u = fill(seed=99, step=0, offset=0, n=N, D=2)
    assert (u > 0).all() and (u < 1).all()
    assert stats.kstest(u, "uniform").pvalue > P_MIN
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / N)
    assert abs(np.corrcoef(u[:-1], u[1:])[0, 1]) < 5 / np.sqrt(N)
    # chi-square over 256 equal bins
    cnt = np.bincount((u * 256).astype(int), minlength=256)
    assert stats.chisquare(cnt).pvalue > P_MIN
    # accept decisions u < alpha happen at the right rate for any alpha
    for a in (0.01, 0.234, 0.9):
        assert abs((u < a).mean() - a) < 5 * np.sqrt(a * (1 - a) / N)


def test_streams_are_independent_across_seeds_steps_families_and_shards():
    n, D = 100_000, 4
    za, ga, ua = fill(seed=1, step=5, offset=0, n=n, D=D, gamma_shape=18.5)
    zb, gb, ub = fill(seed=2, step=5, offset=0, n=n, D=D, gamma_shape=18.5)       # another engine (seed)
    zc, gc, uc = fill(seed=1, step=6, offset=0, n=n, D=D, gamma_shape=18.5)       # the next step
    lim = 5 / np.sqrt(n)
    corr = lambda a, b: abs(np.corrcoef(a, b)[0, 1])
    for other_z, other_g, other_u in ((zb, gb, ub), (zc, gc, uc)):
        assert corr(za[:, 0], other_z[:, 0]) < lim and corr(ga, other_g) < lim and corr(ua, other_u) < lim
        assert not np.array_equal(za, other_z)
        # two-sample KS: same law
        assert stats.ks_2samp(ga, other_g).pvalue > P_MIN
    # families of one (seed, step, walker) do not see each other
    assert corr(za[:, 0], ga) < lim and corr(za[:, 0], ua) < lim and corr(ga, ua) < lim
    assert corr(za[:, 0] ** 2, ga) < lim
    # keyed by the GLOBAL walker index: a shard that starts at walker 1000 draws walkers 1000.. of the whole set
    zs, gs, us = fill(seed=1, step=5, offset=1000, n=5000, D=D, gamma_shape=18.5)
    assert np.array_equal(zs, za[1000:6000]) and np.array_equal(gs, ga[1000:6000]) and np.array_equal(us, ua[1000:6000])
    # deterministic
    z2, g2, u2 = fill(seed=1, step=5, offset=0, n=n, D=D, gamma_shape=18.5)
    assert np.array_equal(z2, za) and np.array_equal(g2, ga) and np.array_equal(u2, ua)


def test_philox_step_accept_rate_and_scale_law():
    """The proposal of a whole Philox step: the t-scale s_k recovered from theta' follows 1/Gamma((D+nu)/2, 2/(nu+delta_k))
    (KS on the probability-integral transform, walker by walker) and the whitened noise is N(0, I)."""
    from pocomc_amd import Flow, Reparameterize
    from pocomc_amd.mcmc import StepEngine
    D, n, nu, sigma = 8, 100_000, 5.0, 0.4
    rng = np.random.default_rng(3)
    bounds = np.tile(np.array([[-10.0, 10.0]]), (D, 1))
    sc = Reparameterize(D, bounds=bounds)
    x = rng.uniform(-9, 9, size=(n, D))
    sc.fit(x)
    u = sc.forward(x)
    flow = Flow(D, "maf3", seed=0)
    A = rng.normal(size=(D, D)) * 0.3
    cov = np.eye(D) + A @ A.T
    mu = rng.normal(size=D) * 0.1
    eng = StepEngine("preconditioned_pcn", n, D, flow, sc, seed=424242)
    eng.load_state(u, x, sc.inverse(u)[1], np.zeros(n), np.zeros(n))
    eng.set_geometry(mu=mu, cov=cov)
    eng.propose(sigma, nu)
    torch.cuda.synchronize()
    theta = eng.theta32.cpu().numpy().astype(np.float64)
    tp = eng.p_theta64.cpu().numpy()
    L = np.linalg.cholesky(cov)
    diff = theta - mu
    delta = np.einsum("ki,ij,kj->k", diff, np.linalg.inv(cov), diff)
    np.testing.assert_allclose(eng.quad.cpu().numpy(), delta, rtol=1e-10)
    w = np.linalg.solve(L, (tp - mu - (1 - sigma ** 2) ** 0.5 * diff).T).T / sigma         # sqrt(s_k) z_k
    # |w_k|^2 = s_k |z_k|^2 with |z|^2 ~ chi2(D) and 1/s_k ~ Gamma(a, 2/(nu+delta_k)):  |w|^2 (nu+delta)/ (D * ... ) is an
    # F-type ratio:  (|z|^2 / D) / (2 g_k / (2a))  with g_k ~ Gamma(a, 1)  ->  (|w|^2 / D) * (nu+delta)/(2a) * ... ~ F(D, 2a)
    a = (D + nu) / 2
    f = (np.sum(w ** 2, axis=1) / D) * (2.0 / (nu + delta)) * a        # = (chi2_D / D) / (gamma(a,1)/a)  ~  F(D, 2a)
    assert stats.kstest(f, stats.f(D, 2 * a).cdf).pvalue > P_MIN
    # directions are uniform on the sphere: normalised coordinates have mean 0, second moment 1/D
    dirn = w / np.linalg.norm(w, axis=1, keepdims=True)
    assert np.abs(dirn.mean(axis=0)).max() < 5 / np.sqrt(n * D)
    assert np.abs((dirn ** 2).mean(axis=0) - 1 / D).max() < 5 * np.sqrt(2.0 / n) / D * 1.5
