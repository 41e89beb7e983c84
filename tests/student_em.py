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
