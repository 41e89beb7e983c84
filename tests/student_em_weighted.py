"""Float64 numpy / scipy restatement of the weighted Student-t EM fit that ``pmc_student_em_weighted``
(``csrc/student.hip``) runs on the device, as ``include/pocomc_amd.h`` states it, and the seeded weight regimes of its
tests (``tests/test_student_em_weighted_cpu.py``, ``tests/test_gpu_student_em_weighted.py``).

With ``P = {r : w_r > 0}``, ``W = sum_P w_r`` and ``pi_r = w_r / W`` one iteration is

    L = chol(Sigma);  delta_r = |L^-1 (x_r - mu)|^2;  omega_r = (nu + D) / (nu + delta_r)
    nu <- root of  [log(nu/2) - psi(nu/2)] - [log((nu+D)/2) - psi((nu+D)/2)] + sum_P pi_r (log omega_r - omega_r + 1)
    Sigma <- sum_P pi_r omega_r d_r d_r^T  (about the old mu);   mu <- sum_P pi_r omega_r x_r / sum_P pi_r omega_r

from ``nu = 20`` with the bracket, the ``nu = inf`` / lower-clamp rules and the stop rule of ``tests/student_em.py``.
It shares no code with the device path: ``scipy.special.psi``, ``scipy.optimize.brentq`` on ``log nu``,
``np.linalg.cholesky`` and a triangular solve, plain numpy sums.
"""
from __future__ import annotations

import numpy as np
from scipy import linalg, optimize, special

import student_em as se

try:                                    # one BLAS thread: the matrices are small (a pool of threads is ten times slower on
    from threadpoolctl import threadpool_limits      # them), and the order of BLAS's sums, hence the recorded noise, depends
except ImportError:                                  # on the number of threads
    from contextlib import nullcontext as threadpool_limits

REGIMES = ("uniform", "lognormal1", "lognormal3", "zeros5", "half_mass", "integer", "chunk_zero")


def weights(regime, n, seed=0):
    """Seeded weights [n] of a regime, not normalised."""
    rng = np.random.default_rng(1000 + seed)
    if regime == "uniform":
        return np.ones(n)
    if regime == "lognormal1":
        return np.exp(rng.normal(size=n))
    if regime == "lognormal3":
        return np.exp(3.0 * rng.normal(size=n))
    if regime == "zeros5":                                   # 5 % exact zeros (one at least)
        w = np.exp(rng.normal(size=n))
        w[rng.permutation(n)[:max(1, n // 20)]] = 0.0
        return w
    if regime == "half_mass":                                # one row holds half the mass
        w = rng.uniform(0.5, 1.5, size=n)
        k = int(rng.integers(n))
        w[k] = 0.0
        w[k] = w.sum()
        return w
    if regime == "integer":
        return rng.integers(0, 4, size=n).astype(np.float64)
    if regime == "chunk_zero":                               # every row of one of the 64 row chunks of the device's sums
        w = np.exp(rng.normal(size=n))
        per = (n + 63) // 64
        c = int(rng.integers((n + per - 1) // per))
        w[c * per:(c + 1) * per] = 0.0
        return w
    raise ValueError(regime)


def ess(w):
    return float(w.sum() ** 2 / (w * w).sum())


def start_values(rows, w):
    """What ``Geometry(student="em_weighted")`` starts from: the weighted mean and the ML-normalised weighted scatter."""
    x = np.asarray(rows, dtype=np.float64)
    p = w / w.sum()
    m = p @ x
    d = x - m
    return m, (p[:, None] * d).T @ d


def f_nu(nu, delta, D, p):
    om = (nu + D) / (nu + delta)
    return ((np.log(nu / 2) - special.psi(nu / 2)) - (np.log((nu + D) / 2) - special.psi((nu + D) / 2))
            + np.sum(p * (np.log(om) - om + 1)))


def update_nu(delta, D, p, xtol=1e-13):
    if f_nu(se.NU_HI, delta, D, p) >= 0:
        return np.inf
    if f_nu(se.NU_LO, delta, D, p) <= 0:
        return se.NU_LO
    t = optimize.brentq(lambda t: f_nu(np.exp(t), delta, D, p), np.log(se.NU_LO), np.log(se.NU_HI), xtol=xtol,
                        rtol=4 * np.finfo(float).eps)
    return float(np.exp(t))


def fit(rows, w, mu, sigma, tol=1e-6, max_iter=100, xtol=1e-13):
    """The weighted EM loop from the given start values.  Returns ``dict(mu, sigma, nu, iterations, status, steps,
    rows_positive, ess)``; rows of weight zero are dropped before anything is computed."""
    with threadpool_limits(1):
        return _fit(rows, w, mu, sigma, tol, max_iter, xtol)


def _fit(rows, w, mu, sigma, tol, max_iter, xtol):
    w = np.asarray(w, dtype=np.float64)
    keep = w > 0
    x = np.asarray(rows, dtype=np.float64)[keep]
    p = w[keep] / w[keep].sum()
    D = x.shape[1]
    mu, sigma = np.array(mu, dtype=np.float64), np.array(sigma, dtype=np.float64)
    nu, last_nu, i, steps = 20.0, 0.0, 0, []
    status = None
    while abs(last_nu - nu) > tol and i < max_iter:
        i += 1
        d = x - mu
        try:
            L = np.linalg.cholesky(sigma)
        except np.linalg.LinAlgError:
            status = "not_pd"
            break
        y = linalg.solve_triangular(L, d.T, lower=True)
        delta = np.sum(y * y, axis=0)
        last_nu = nu
        nu = update_nu(delta, D, p, xtol)
        if nu == np.inf:
            status = "nu_inf"
            break
        pw = p * (nu + D) / (nu + delta)
        sigma = (pw[:, None] * d).T @ d
        mu = (pw[:, None] * x).sum(axis=0) / pw.sum()
        steps.append(abs(last_nu - nu))
    if status is None:
        status = "lower_clamp" if nu == se.NU_LO else "converged" if not abs(last_nu - nu) > tol else "max_iter"
    return dict(mu=mu, sigma=sigma, nu=nu, iterations=i, status=status, steps=steps, rows_positive=int(keep.sum()),
                ess=ess(w[keep]))


def reorder_noise(rows, w, mu, sigma, perms=3, **kw):
    """``tests/student_em.py: reorder_noise`` for the weighted fit: ``(d_nu, d_mu, d_sigma)``, how far the restatement's own
    result moves when rows and weights come in another order and its root tolerance is 1e-11 instead of 1e-13; the largest
    over ``perms`` seeded permutations.  ``se.tolerances`` turns it into the bound of the device tests."""
    a = fit(rows, w, mu, sigma, **kw)
    d = [0.0, 0.0, 0.0]
    for k in range(perms):
        q = np.random.default_rng(k).permutation(rows.shape[0])
        b = fit(rows[q], w[q], mu, sigma, xtol=1e-11, **kw)
        assert np.isfinite(a["nu"]) and np.isfinite(b["nu"])
        d[0] = max(d[0], abs(a["nu"] - b["nu"]) / a["nu"])
        d[1] = max(d[1], np.abs(a["mu"] - b["mu"]).max() / np.abs(a["mu"]).max())
        d[2] = max(d[2], np.abs(a["sigma"] - b["sigma"]).max() / np.abs(a["sigma"]).max())
    return tuple(d)


def systematic_indices(n, w, offset):
    """The systematic resample of ``n`` indices at a given offset in [0, 1) (``pocomc/tools.py``: positions
    ``(arange(n) + offset) / n`` against the cumulative weights)."""
    c = np.cumsum(w / w.sum())
    return np.minimum(np.searchsorted(c, (np.arange(n) + offset) / n), n - 1)


# (n, D) of the device parity: the tile edges of em_mom2_kernel, the last width of pmc_student_em, the first width of the
# 32-row instance of em_delta_kernel (129), a width past 160 KiB of LDS for 64 rows in the issue's count (143), the limit
SHAPES = [(40, 3), (65, 1), (130, 15), (130, 16), (130, 17), (300, 64), (200, 128), (200, 129), (260, 143), (220, 157)]
LENGTHS = [(0.0, 1), (0.0, 4), (0.0, 10), (1e-6, 100)]          # (tol, max_iter): three fixed lengths, and run to the end


def case_rows(n, D, f32=False):
    """t_3 rows of a shape, seeded by it (``se.edge_rows`` without the selection)."""
    return se.mvt_rows(300 + D, n, D, 3.0, dtype=np.float32 if f32 else np.float64)


def case_weights(n, D, regime):
    """The weights of a parity case: ``weights(regime, n, seed)`` with the first seed of D, D + 1000, ... that leaves more
    rows of positive weight than dimensions (220 x 157 with integer weights: a quarter of the rows are at zero)."""
    for k in range(16):
        w = weights(regime, n, seed=D + 1000 * k)
        if int((w > 0).sum()) > D:
            return w
    raise AssertionError((n, D, regime))


# ``reorder_noise`` (three permutations, float64 rows) of the cases where a component reaches 2e-12 -- ``(n, D, regime, index
# into LENGTHS) -> (d_nu, d_mu, d_sigma)``; every other case is below 2e-12 and gets the 1e-9 floor of ``se.tolerances``.
# ``tests/test_student_em_weighted_cpu.py`` re-measures all of them.  Below D = 128 the figures are the measured ones times
# 1.3.  The log-normal sigma = 3 weights at D >= 128 leave a Kish ESS of 1.2 to 3.7 on 200 to 260 rows: the fit is at the lower
# clamp after two iterations, its scatter matrix is a few rows' outer products, and the restatement's noise there moves by
# a factor of 2.4 with the number of BLAS threads of the process (Sigma: 2.1e-11 ... 4.9e-11 at 220 x 157, 1.4e-12 ...
# 3.3e-12 at 260 x 143); recorded is twice the largest seen.
NOISE = {
    (40, 3, "uniform", 0): (1.1e-11, 5.2e-14, 3.0e-13),
    (40, 3, "uniform", 1): (3.3e-12, 4.2e-14, 2.6e-13),
    (40, 3, "lognormal1", 2): (3.4e-12, 3.8e-14, 2.6e-13),
    (40, 3, "lognormal1", 3): (3.0e-12, 4.3e-14, 2.8e-13),
    (40, 3, "integer", 1): (3.2e-12, 2.7e-14, 1.7e-13),
    (65, 1, "lognormal3", 3): (7.8e-13, 3.0e-16, 8.1e-12),
    (130, 17, "zeros5", 3): (3.5e-12, 2.1e-13, 7.8e-13),
    (130, 17, "integer", 2): (3.1e-12, 4.3e-14, 5.5e-14),
    (200, 128, "zeros5", 0): (2.9e-12, 2.1e-14, 1.2e-13),
    (220, 157, "integer", 1): (3.0e-12, 5.2e-15, 7.5e-14),
}
for _k in (1, 2, 3):
    NOISE[(200, 128, "lognormal3", _k)] = (0.0, 9.4e-14, 1.0e-10)
    NOISE[(260, 143, "lognormal3", _k)] = (0.0, 6.0e-13, 6.6e-12)
    NOISE[(220, 157, "lognormal3", _k)] = (0.0, 1.8e-12, 9.8e-11)


def tolerances(n, D, regime, k):
    """``(tol_nu, tol_mu, tol_sigma)`` of a device case: ``se.tolerances`` of its recorded noise (1e-9 where none is)."""
    return se.tolerances(NOISE.get((n, D, regime, k), (0.0, 0.0, 0.0)))


# The four synthetic pools on which the resample-based fit was compared with the weighted one:
# (seed, n, D, nu of the rows, sigma of the log-normal weights); 5 % of the weights are exact zeros
POOLS = [(4, 2048, 6, 4.0, 1.0), (5, 2048, 6, 4.0, 2.0), (6, 4096, 32, 5.0, 1.5), (7, 1024, 2, 3.0, 3.0)]


def pool(seed, n, D, nu, s_lw):
    x = se.mvt_rows(seed, n, D, nu)
    rng = np.random.default_rng(100 + seed)
    w = np.exp(s_lw * rng.normal(size=n))
    w[rng.random(n) < 0.05] = 0.0
    return x, w
