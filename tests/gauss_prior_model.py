"""The arithmetic of ``csrc/gauss_prior.hip`` (``pmc_gauss_blocks_logpdf``, include/pocomc_amd.h), stated in numpy: float64,
loops over i and j with the rows vectorised, every product and every sum a numpy operation of its own (numpy contracts
nothing into an FMA) in the order the header fixes.  The kernel must equal it bit for bit.

    d_j = x[cols[j]] - mean[j]
    y_i = (((0.0 + Linv[i,0] d_0) + Linv[i,1] d_1) + ...) + Linv[i,i] d_i
    q   = ((0.0 + y_0 y_0) + y_1 y_1) + ...
    g   = -0.5 q - logc;   -inf where an x[cols[j]] is not finite or g is NaN
"""
import numpy as np


def constants(mean, cov):
    """``(mean, linv_packed, logc)``: what ``GaussianPrior`` computes on the host, by the issue's formulas."""
    from scipy.linalg import solve_triangular
    mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    k = len(mean)
    L = np.linalg.cholesky(cov)
    Linv = solve_triangular(L, np.eye(k), lower=True)
    packed = np.concatenate([Linv[i, :i + 1] for i in range(k)])
    logc = np.sum(np.log(np.diag(L))) + 0.5 * k * np.log(2 * np.pi)
    return mean, packed, float(logc)


def gauss_block_model(xb, mean, linv_packed, logc):
    """``g`` of every row of ``xb`` ``(n, k)``, the block's gathered columns."""
    xb = np.asarray(xb, dtype=np.float64)
    n, k = xb.shape
    assert len(mean) == k and len(linv_packed) == k * (k + 1) // 2
    with np.errstate(all="ignore"):
        d = [xb[:, j] - mean[j] for j in range(k)]
        q = np.zeros(n)
        for i in range(k):
            row = linv_packed[i * (i + 1) // 2:]
            y = np.zeros(n)
            for j in range(i + 1):
                y = y + row[j] * d[j]
            q = q + y * y
        g = -0.5 * q - logc
    bad = ~np.isfinite(xb).all(axis=1) | np.isnan(g)
    return np.where(bad, -np.inf, g)


def gauss_blocks_model(x, blocks, start=None):
    """``start + g_0 + g_1 + ...`` left to right (``start=None``: ``g_0 + g_1 + ...``), ``blocks`` a list of
    ``(cols, mean, linv_packed, logc)``; -inf where the sum is not finite."""
    x = np.asarray(x, dtype=np.float64)
    v = None if start is None else np.array(start, dtype=np.float64)
    with np.errstate(all="ignore"):
        for cols, mean, packed, logc in blocks:
            g = gauss_block_model(x[:, np.asarray(cols)], mean, packed, logc)
            v = g if v is None else v + g
    return np.where(np.isfinite(v), v, -np.inf)


def random_cov(k, cond, rng):
    """A covariance with a random orthogonal basis and eigenvalues log-spaced from 1 down to 1 / cond, exactly symmetric."""
    Q, _ = np.linalg.qr(rng.normal(size=(k, k)))
    lam = np.logspace(0.0, -np.log10(cond), k) if k > 1 else np.ones(1)
    c = (Q * lam) @ Q.T
    return 0.5 * (c + c.T)


def draws(mean, cov, n, width, rng):
    """``n`` rows of N(mean, width^2 cov)."""
    L = np.linalg.cholesky(cov)
    return mean + width * (rng.normal(size=(n, len(mean))) @ L.T)
