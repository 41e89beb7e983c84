"""The blocks form of the joint prior restated in numpy and scipy (test infrastructure): the density
``pocomc_amd.JointPrior([fp_0, fp_1, ...], [cols_0, cols_1, ...], rest)`` evaluates on the device,

    ``log p(x) = sum_b flow_prior_model_b(x[:, cols_b]) + sum_m dists[m].logpdf(x[:, rest_cols[m]])``,

the blocks' terms added left to right in float64, then the factors' -- from ``tests/flow_prior_model.py`` (the oracle's scaler
and flow) and ``tests/joint_prior_model.py`` (the factors and their rows), with -inf wherever the sum, or any x of the row, is
not finite."""
import numpy as np

from flow_prior_model import flow_prior_model
from joint_prior_model import rest_dists, rest_rows  # noqa: F401  (the fixtures of the single form serve this one too)


def interleaved_blocks(dims, Dr, seed=0):
    """Column lists for blocks of ``dims`` columns and ``Dr`` rest columns: a shuffle of all positions dealt out block after
    block, so that every block's columns are interleaved with the others' and with the rest's, and no list is sorted."""
    D = sum(dims) + Dr
    rng = np.random.default_rng(seed + 1000 * D)
    while True:
        perm = rng.permutation(D)
        lists, o = [], 0
        for d in dims:
            lists.append([int(c) for c in perm[o:o + d]])
            o += d
        if all(l != sorted(l) for l in lists):
            return lists


def layout_blocks(columns, D):
    """``(block_cols, rest_cols)``: the model's own statement of ``JointPrior.layout_blocks`` (valid input only)."""
    maps = [np.asarray(c, dtype=np.int64) for c in columns]
    taken = set(int(c) for m in maps for c in m)
    return maps, np.array([j for j in range(D) if j not in taken], dtype=np.int64)


def joint_blocks_model(scalers, mafs, dists, columns, x):
    """``(logp, block_logp, rest_terms)`` of the rows of ``x`` (float64 ``(n, D)``): ``logp`` float64, -inf wherever the sum
    or an x of the row is not finite; ``block_logp`` ``(B, n)`` every block's ``flow_prior_model`` value; ``rest_terms``
    ``(n, Dr)`` the factors' ``logpdf`` (``dists`` empty or None: no table).  Every block is evaluated one row at a time, as
    ``joint_prior_model`` does: a row's bits do not depend on which other rows are in the call."""
    x = np.asarray(x, dtype=np.float64)
    dists = list(dists or [])
    maps, rest_cols = layout_blocks(columns, x.shape[1])
    assert len(rest_cols) == len(dists) and len(maps) == len(scalers) == len(mafs)
    block_logp = np.array([[flow_prior_model(s, m, x[r:r + 1, cols])[0][0] for r in range(len(x))]
                           for s, m, cols in zip(scalers, mafs, maps)])
    with np.errstate(all="ignore"):
        terms = (np.stack([d.logpdf(x[:, j]) for d, j in zip(dists, rest_cols)], axis=1) if dists
                 else np.zeros((len(x), 0)))
        v = block_logp[0].copy()
        for b in range(1, len(maps)):
            v = v + block_logp[b]
        if dists:                                                 # (the table's own sum, from 0.0, then added)
            lp = np.zeros(len(x))
            for m in range(len(dists)):
                lp = lp + terms[:, m]
            v = v + lp
        v = np.where(np.isfinite(x).all(axis=1), v, -np.inf)
    return np.where(np.isfinite(v), v, -np.inf), block_logp, terms
