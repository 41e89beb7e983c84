"""The joint prior restated in numpy and scipy (test infrastructure): the density ``pocomc_amd.JointPrior`` evaluates on the
device,

    ``log p(x) = flow_prior_model(x[:, flow_cols]) + sum_m dists[m].logpdf(x[:, rest_cols[m]])``,

from ``tests/flow_prior_model.py`` (the oracle's scaler and flow) and the frozen scipy factors themselves, with -inf wherever
the result is not finite: a NaN or an inf in the row, the flow block on or beyond a scaler bound, a rest column outside its
factor's support, a pole of a factor."""
import numpy as np

from flow_prior_model import flow_prior_model


def rest_dists(Dr):
    """``Dr`` frozen scipy factors: uniform, norm, gamma, beta, truncnorm and lognorm, cycled."""
    from scipy import stats
    kinds = [stats.uniform(-2.0, 5.0), stats.norm(0.5, 1.5), stats.gamma(2.5, loc=-1.0, scale=0.8),
             stats.beta(2.0, 3.5, loc=-1.0, scale=4.0), stats.truncnorm(-1.5, 2.0, loc=0.3, scale=1.2),
             stats.lognorm(0.6, loc=-0.5, scale=1.1)]
    return [kinds[m % len(kinds)] for m in range(Dr)]


def rest_rows(dists, n, rng):
    """``(n, Dr)`` rows inside every factor's support: between its 1e-3 and 1 - 1e-3 quantiles."""
    p = rng.uniform(1e-3, 1.0 - 1e-3, size=(n, len(dists)))
    return np.stack([d.ppf(p[:, m]) for m, d in enumerate(dists)], axis=1)


def flow_rows(bounds, n, rng):
    """``(n, Df)`` rows strictly inside ``bounds``: across a two-sided range, up to 6 units from a one-sided bound, 3 units
    either way where there is none."""
    p = rng.uniform(0.02, 0.98, size=(n, len(bounds)))
    lo, hi = bounds[:, 0], bounds[:, 1]
    both, left, right = np.isfinite(lo) & np.isfinite(hi), np.isfinite(lo) & ~np.isfinite(hi), ~np.isfinite(lo) & np.isfinite(hi)
    x = 6.0 * (p - 0.5)
    for j in range(len(bounds)):
        if both[j]:
            x[:, j] = lo[j] + (hi[j] - lo[j]) * p[:, j]
        elif left[j]:
            x[:, j] = lo[j] + 6.0 * p[:, j]
        elif right[j]:
            x[:, j] = hi[j] - 6.0 * p[:, j]
    return x


def interleaved_columns(Df, Dr, seed=0):
    """Positions of the flow block in the joint x: spread evenly from the first to the last of the Df + Dr columns (rest
    columns lie between them), then shuffled (not sorted)."""
    rng = np.random.default_rng(seed)
    cols = np.round(np.linspace(0, Df + Dr - 1, Df)).astype(np.int64)
    assert len(np.unique(cols)) == Df
    while Df > 1 and np.array_equal(cols, np.sort(cols)):
        cols = rng.permutation(cols)
    return [int(c) for c in cols]


def layout(columns, D):
    """``(flow_cols, rest_cols)``: the model's own statement of ``JointPrior.layout`` (valid input only)."""
    flow_cols = np.asarray(columns, dtype=np.int64)
    return flow_cols, np.array([j for j in range(D) if j not in set(flow_cols.tolist())], dtype=np.int64)


def joint_prior_model(scaler, maf, dists, columns, x):
    """``(logp, flow_logp, rest_terms)`` of the rows of ``x`` (float64 ``(n, Df + Dr)``): ``logp`` float64, -inf wherever the
    sum is not finite; ``flow_logp`` the flow block's ``flow_prior_model`` value; ``rest_terms`` ``(n, Dr)`` the factors'
    ``logpdf``.  The flow block is evaluated one row at a time: a row's bits then do not depend on which other rows are in
    the call (numpy's matrix products round differently at different row counts)."""
    x = np.asarray(x, dtype=np.float64)
    flow_cols, rest_cols = layout(columns, x.shape[1])
    flow_logp = np.array([flow_prior_model(scaler, maf, x[r:r + 1, flow_cols])[0][0] for r in range(len(x))])
    with np.errstate(all="ignore"):
        terms = np.stack([d.logpdf(x[:, j]) for d, j in zip(dists, rest_cols)], axis=1)
        v = flow_logp + terms.sum(axis=1)
        v = np.where(np.isfinite(x).all(axis=1), v, -np.inf)
    return np.where(np.isfinite(v), v, -np.inf), flow_logp, terms
