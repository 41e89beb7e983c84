"""The value of ``pmc_gauss_box_logpdf`` (``pocomc_amd.TruncatedGaussianPrior``, include/pocomc_amd.h), stated in numpy on top of
``tests/gauss_prior_model.py``: a row's value is ``gauss_block_model(x, mean, linv_packed, logc_box)`` where every
``lo_j <= x_j <= hi_j`` holds (a NaN fails the test) and -inf elsewhere; several blocks go through ``gauss_blocks_model``, with
-inf for a row that violates any block's box.  The kernel must equal it bit for bit.

Also the fixture of ``tests/test_gpu_gauss_box_prior.py``: ``tests/test_gpu_gauss_prior.py``'s recipe with a box on the columns
{0, 7, 8, k - 1}."""
import numpy as np

import gauss_prior_model as gpm


def in_box(xb, lo, hi):
    """Every ``lo_j <= x_j <= hi_j`` of a row, written so that a NaN fails it."""
    with np.errstate(all="ignore"):
        return ((xb >= lo) & (xb <= hi)).all(axis=1)


def gauss_box_model(xb, mean, linv_packed, logc_box, lo, hi):
    """The truncated block's value of every row of ``xb`` ``(n, k)``, the block's gathered columns."""
    xb = np.asarray(xb, dtype=np.float64)
    g = gpm.gauss_block_model(xb, mean, linv_packed, logc_box)
    return np.where(in_box(xb, lo, hi), g, -np.inf)


def gauss_box_blocks_model(x, blocks, start=None):
    """``gauss_blocks_model`` over ``blocks``, a list of ``(cols, mean, linv_packed, logc, lo, hi)`` with ``lo = hi = None`` for a
    block without a box; -inf for a row that violates any block's box."""
    x = np.asarray(x, dtype=np.float64)
    v = gpm.gauss_blocks_model(x, [b[:4] for b in blocks], start)
    ok = np.ones(len(x), dtype=bool)
    for cols, _, _, _, lo, hi in blocks:
        if lo is not None:
            ok &= in_box(x[:, np.asarray(cols)], lo, hi)
    return np.where(ok, v, -np.inf)


def bounded_columns(k):
    """{0, 7, 8, k - 1} in [0, k): 7 and 8 are where the element stage wraps from wavefront 7 to wavefront 0, k - 1 is the
    ragged end."""
    return sorted({0, 7, 8, k - 1} & set(range(k)))


def box_of(mean, cov):
    """``(k, 2)`` bounds: ``lo = mean - 1.5 sd`` on every bounded column, ``hi = mean + 1.5 sd`` on the 1st and 3rd of them and
    +inf on the others -- both one-sided and two-sided limits occur."""
    k = len(mean)
    sd = np.sqrt(np.diag(cov))
    b = np.stack([np.full(k, -np.inf), np.full(k, np.inf)], axis=1)
    for i, j in enumerate(bounded_columns(k)):
        b[j, 0] = mean[j] - 1.5 * sd[j]
        if i % 2 == 0:
            b[j, 1] = mean[j] + 1.5 * sd[j]
    return b


def fixture(k, cond=100.0):
    """``(mean, cov, bounds, x)``: ``rng = default_rng(7 k + 1)``, ``mean = 3 normal``, ``cov = 2.5 random_cov(k, cond)``, 150
    rows of width 1 and 50 of width 10 -- the rows of ``tests/test_gpu_gauss_prior.py`` -- and ``box_of``'s bounds."""
    rng = np.random.default_rng(7 * k + 1)
    mean = rng.normal(size=k) * 3.0
    cov = gpm.random_cov(k, cond, rng) * 2.5
    x = np.concatenate([gpm.draws(mean, cov, 150, 1.0, rng), gpm.draws(mean, cov, 50, 10.0, rng)])
    return mean, cov, box_of(mean, cov), x
