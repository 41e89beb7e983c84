"""Float64 numpy / scipy restatement of the Student-t EM fit that ``pmc_student_em`` (``csrc/student.hip``) runs on the
device, as ``include/pocomc_amd.h`` states it, and a seeded generator of correlated multivariate-t rows
(``tests/test_student_em_cpu.py``, ``tests/test_gpu_student_em.py``).

The restatement shares no code with the device path: ``scipy.special.psi`` for the digamma function,
``scipy.optimize.brentq`` on ``log nu`` for the root, ``np.linalg.cholesky`` and a triangular solve for the Mahalanobis
distances, plain numpy sums for the weighted moments.
"""
from __future__ import annotations

import numpy as np
from scipy import linalg, optimize, special

NU_LO, NU_HI = 0.1, 1e4
STATUS = ("converged", "max_iter", "nu_inf", "lower_clamp", "not_pd", "nonfinite")      # PMC_STUDENT_* in this order


def mvt_rows(seed, n, D, nu, dtype=np.float64):
    """``n`` draws of a ``D``-variate t with ``nu`` degrees of freedom (``nu = inf``: normal), correlated columns of
    unequal scale, a location away from zero.  The mixing matrix is the identity plus a dense perturbation: its scatter
    matrix stays well conditioned at every ``D`` (a random triangular one does not: its condition number grows like ``2^D``,
    and at ``D = 128`` the restatement itself then moves by 1e-3 under a permutation of the rows)."""
    rng = np.random.default_rng(seed)
    A = (np.eye(D) + 0.5 * rng.normal(size=(D, D)) / np.sqrt(D)) * np.linspace(0.5, 2.0, D)[:, None]
    loc = rng.normal(size=D) * 3.0
    z = rng.normal(size=(n, D)) @ A.T
    if np.isfinite(nu):
        z = z / np.sqrt(rng.chisquare(nu, size=n) / nu)[:, None]
    return np.ascontiguousarray(loc + z, dtype=dtype)


def start_values(rows):
    """``mu, Sigma`` that ``Geometry.fit`` forms for the rows it fits: the column medians (in the rows' precision) and
    ``S / n + diag(var) / n``, ``var`` rounded to float32 for float32 rows."""
    n = rows.shape[0]
    x = rows.astype(np.float64)
    d = x - x.mean(axis=0)
    S = d.T @ d
    var = np.diag(S) / n
    if rows.dtype == np.float32:
        var = var.astype(np.float32)
    return np.median(rows, axis=0).astype(np.float64), S / n + (1 / n) * np.diag(var)


def f_nu(nu, delta, D):
    w = (nu + D) / (nu + delta)
    return (np.log(nu / 2) - special.psi(nu / 2) + np.mean(np.log(w) - w) + 1 + special.psi((nu + D) / 2)
            - np.log((nu + D) / 2))


def update_nu(delta, D, xtol=1e-13):
    if f_nu(NU_HI, delta, D) >= 0:
        return np.inf
    if f_nu(NU_LO, delta, D) <= 0:
        return NU_LO
    t = optimize.brentq(lambda t: f_nu(np.exp(t), delta, D), np.log(NU_LO), np.log(NU_HI), xtol=xtol, rtol=4 * np.finfo(float).eps)
    return float(np.exp(t))


def fit(rows, mu, sigma, tol=1e-6, max_iter=100, xtol=1e-13):
    """The EM loop from the given start values.  Returns ``dict(mu, sigma, nu, iterations, status, steps)``;
    ``steps`` lists ``|last_nu - nu|`` of every completed iteration."""
    x = np.asarray(rows, dtype=np.float64)
    n, D = x.shape
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
        nu = update_nu(delta, D, xtol)
        if nu == np.inf:
            status = "nu_inf"
            break
        w = (nu + D) / (nu + delta)
        sigma = (w[:, None] * d).T @ d / n
        mu = (w[:, None] * x).sum(axis=0) / w.sum()
        steps.append(abs(last_nu - nu))
    if status is None:
        status = "lower_clamp" if nu == NU_LO else "converged" if not abs(last_nu - nu) > tol else "max_iter"
    return dict(mu=mu, sigma=sigma, nu=nu, iterations=i, status=status, steps=steps)


# ---------------------------------------------------------------------------------------------------------------------
# What the edge tests share (``tests/test_student_em_cpu.py`` holds the conditions on the CPU,
# ``tests/test_gpu_student_em_edges.py`` compares the device): the noise of the restatement itself, and inputs whose
# first-iteration root of f(nu) lies where the test wants it.
# ---------------------------------------------------------------------------------------------------------------------
def first_deltas(rows, mu, sigma):
    """The squared Mahalanobis distances of the first iteration."""
    L = np.linalg.cholesky(np.asarray(sigma, dtype=np.float64))
    y = linalg.solve_triangular(L, (np.asarray(rows, dtype=np.float64) - mu).T, lower=True)
    return np.sum(y * y, axis=0)


def reorder_noise(rows, mu, sigma, perms=3, **kw):
    """``(d_nu, d_mu, d_sigma)``: how far the restatement's own result moves when the rows come in another order and its
    root tolerance is 1e-11 instead of 1e-13 -- nu relative to itself, mu to max|mu|, Sigma to max|Sigma|; the largest
    over ``perms`` seeded permutations (one alone can land on the same root by luck: above nu of about 1000 f(nu) is flat
    to the rounding of ``psi`` and ``log``, and a root finder stops anywhere inside that band).  The procedure behind
    every tolerance of the device tests: 500 times this, and never below 1e-9."""
    a = fit(rows, mu, sigma, **kw)
    d = [0.0, 0.0, 0.0]
    for k in range(perms):
        b = fit(rows[np.random.default_rng(k).permutation(rows.shape[0])], mu, sigma, xtol=1e-11, **kw)
        assert np.isfinite(a["nu"]) and np.isfinite(b["nu"])
        d[0] = max(d[0], abs(a["nu"] - b["nu"]) / a["nu"])
        d[1] = max(d[1], np.abs(a["mu"] - b["mu"]).max() / np.abs(a["mu"]).max())
        d[2] = max(d[2], np.abs(a["sigma"] - b["sigma"]).max() / np.abs(a["sigma"]).max())
    return tuple(d)


def tolerances(d, floor=1e-9, margin=500.0):
    """``(tol_nu, tol_mu, tol_sigma)`` from a recorded ``reorder_noise``."""
    return tuple(max(floor, margin * v) for v in d)


def scaled_start(rows, c):
    """``start_values`` with the scatter matrix times ``c``: every distance of the first iteration divided by ``c``, which
    moves the first root of f(nu) along the nu axis without touching the rows."""
    mu, sigma = start_values(rows)
    return mu, c * sigma


def collinear_rows(seed=0, n=200, D=8):
    """Rows in a two-dimensional subspace of ``R^D`` with heavy tails; column 1 is exactly twice column 0.  Sigma after one
    EM iteration has rank 3 (the plane, and the offset of the column medians the fit starts from, which do not lie in it):
    its Cholesky factorisation meets, after three pivots, a 5 x 5 block that holds rounding only
    -- about as likely to be positive definite as a random symmetric matrix of that size, whatever the order of the sums.
    (Two columns alone, ``x[:, 1] = 2 x[:, 0]``, leave ONE such pivot, ``4 (s - fl(fl(s / r)^2))``: zero or an ulp of either
    sign, decided by the last bit of ``s``.  The restatement survives it on one seed in four of a trial and then fails an iteration
    later; a device that adds in another order need not agree.)"""
    rng = np.random.default_rng(seed)
    f = rng.standard_t(3, size=(n, 2)) * np.array([1.5, 0.6]) + np.array([0.7, -0.2])
    mix = rng.normal(size=(2, D))
    mix[:, 0] = (1.0, 0.0)
    x = f @ mix
    x[:, 1] = 2.0 * x[:, 0]
    return np.ascontiguousarray(x)


# (n, D) of the fixed-length edge cases: fewer rows than one wavefront and than the 64 row chunks of the weighted sums;
# D = 1; 63 / 64 / 65 rows; D across the 16-wide tiles; D = 127 (the remainder loop of the substitution) and the LDS limit
EDGE_SHAPES = [(40, 3), (63, 1), (65, 1), (64, 5), (130, 15), (130, 16), (130, 17), (300, 127), (200, 128)]


def edge_rows(n, D, f32, indexed):
    """``(x, idx, rows)`` of an edge shape: the pool, the selection (None: all rows) and the selected rows as the
    restatement sees them; t3 rows, so that f(nu) has a root at every one of the shapes."""
    x = mvt_rows(300 + D, n + (11 if indexed else 0), D, 3.0, dtype=np.float32 if f32 else np.float64)
    if not indexed:
        return x, None, x
    idx = np.random.default_rng(n).integers(0, x.shape[0], size=n)       # repeats, out of order
    return x, idx, x[idx]


# The nu axis, one iteration (``tol = 0, max_iter = 1``): ``(mvt_rows arguments, c, root, (d_nu, d_mu, d_sigma))`` with the
# start values ``scaled_start(rows, c)``, the restatement's first root of f(nu) to six digits and its ``reorder_noise``
# rounded up to two digits -- both re-measured by ``tests/test_student_em_cpu.py``.  One root or more in every decade of
# [0.1, 1e4], and one within a factor of two of either end.
#   * c = 1e-6 on the Cauchy rows: every distance is above D (all w < 1, |u| up to 1); c = 0.1: distances from 1e-4 to
#     6.8e3 around a root of 0.65, rows far on either side of |u| = 1/2; the D = 128 rows: all |u| < 0.42 at every nu.
#   * c = 1.00175 on the t_3000 rows is the search's answer for the top decade (1.002: 9474, 1.004: no root below 1e4).
#   * NOT here: the c = 1 roots of (1, 4096, 4, 1000) and (2, 4096, 4, 1000), 977.68 and 1215.24.  Their ``reorder_noise``
#     reads 0 over 16 permutations, and not because the restatement is exact there: its f(nu) is a staircase of 8.9e-16
#     (one ulp of log(nu / 2) and psi(nu / 2), both about 6) that is flat to two steps over 3e-8 of nu, brentq meets a
#     value of exactly 0.0 and returns it, and a permutation moves the mean by less than a step.  The rule would hand
#     these inputs 1e-9 where the restatement itself is good to 2e-8 (``test_a_plateau_hides_the_restatements_noise``).
NU_AXIS = [
    ((4, 1024, 3, 1), 1e-06, 0.197682, (1.5e-16, 1.4e-15, 1.6e-15)),
    ((4, 1024, 3, 1), 0.1, 0.64821, (2.9e-13, 2.5e-15, 4.3e-14)),
    ((3, 65, 1, 1), 1.0, 4.83408, (1.8e-14, 8.5e-16, 6.3e-15)),
    ((2, 40, 3, 4), 1.0, 9.08295, (2.2e-13, 1.2e-14, 2.1e-14)),
    ((2, 63, 1, 3), 1.0, 54.6534, (4.5e-12, 2e-14, 1.6e-13)),
    ((5, 300, 128, 100), 0.9, 201.447, (9.9e-13, 2e-15, 2.4e-14)),
    ((1, 4096, 4, 100), 1.0, 279.179, (0.0, 1.6e-15, 1.2e-15)),
    ((1, 4096, 4, 300), 1.0, 595.81, (5.1e-09, 4.1e-13, 1.7e-11)),
    ((2, 4096, 4, 3000), 1.0, 2020.79, (1.5e-07, 1.6e-12, 1.5e-10)),
    ((2, 4096, 4, 3000), 1.00175, 6488.91, (6e-06, 2e-11, 1.9e-09)),
]
NU_AXIS_STRADDLE, NU_AXIS_NEAR_ONE = NU_AXIS[1], NU_AXIS[5]      # |u| far on both sides of 1/2; all |u| < 1/2

# Large-nu fits run to the end (default ``tol``, ``max_iter``): ``(mvt_rows arguments, nu, (d_nu, d_mu, d_sigma))``
LARGE_NU = [
    ((1, 4096, 4, 300), 356.764, (7.9e-10, 5.5e-14, 4.2e-12)),
    ((1, 4096, 4, 1000), 588.259, (7.6e-09, 3.1e-13, 2.5e-11)),
    ((1, 4096, 4, 3000), 598.277, (3.7e-09, 1.5e-13, 1.2e-11)),
    ((2, 4096, 4, 3000), 1291.43, (6.1e-08, 1.1e-12, 9.6e-11)),
]
