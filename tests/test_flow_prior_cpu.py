"""The float64 restatement of the flow prior (``tests/flow_prior_model.py``) is a normalised density: it integrates to one
over the scaler's box, for an affine and a spline flow under both transforms, and it is -inf off the support.  A wrong sign
on the scaler's log-determinant misses the first by orders of magnitude.  No GPU."""
import numpy as np
import pytest

import cases
import flow_prior_model as fpm
from oracle.maf import OracleMAF
from pocomc_amd.maf_spec import MAFSpec


def _parts(univariate, transform):
    spec = MAFSpec(2, 3, univariate=univariate)
    maf = OracleMAF(spec, cases.flow_params(spec, 5))
    return fpm.oracle_scaler(fpm.NORM_BOUNDS, transform, fpm.norm_fit_rows()), maf


@pytest.mark.parametrize("transform", ["probit", "logit"])
@pytest.mark.parametrize("univariate", ["affine", "rqs"])
def test_the_model_integrates_to_one(univariate, transform):
    """Midpoint rule on a 600 x 600 grid.  Measured: affine 0.9983 (probit) / 0.9998 (logit), rqs 1.0004 / 1.0001."""
    scaler, maf = _parts(univariate, transform)
    x, cell = fpm.norm_grid()
    logp, ldj, inside = fpm.flow_prior_model(scaler, maf, x)
    assert inside.all() and np.isfinite(logp).all()
    total = fpm.integral(logp, cell)
    print(f"{univariate} {transform}: integral {total:.4f}")
    assert abs(total - 1.0) <= fpm.NORM_BOUND, total
    # the sign of the log-determinant is what normalises it: with the other sign the integral is nowhere near one
    u = scaler.forward(x)
    wrong = maf.log_prob(u.astype(np.float32)).astype(np.float64) + ldj
    assert abs(fpm.integral(wrong, cell) - 1.0) > 100 * fpm.NORM_BOUND


@pytest.mark.parametrize("transform", ["probit", "logit"])
def test_rows_off_the_support_are_minus_infinity(transform):
    scaler, maf = _parts("affine", transform)
    x = np.array([[0.5, 2.5],             # inside
                  [-1.0, 2.5],            # on the lower bound
                  [0.5, 5.0],             # on the upper bound
                  [2.5, 2.5],             # beyond the upper bound
                  [0.5, -0.1],            # below the lower bound
                  [np.nan, 2.5],
                  [0.5, np.inf],
                  [-np.inf, 2.5],
                  [1.9, 0.1]])            # inside
    logp, ldj, inside = fpm.flow_prior_model(scaler, maf, x)
    want = np.array([True] + [False] * 7 + [True])
    assert np.array_equal(inside, want)
    assert np.isfinite(logp[want]).all() and np.isfinite(ldj[want]).all()
    assert np.isneginf(logp[~want]).all()
    assert not np.isnan(logp).any()
    # row-wise: the good rows alone give the same values
    alone = fpm.flow_prior_model(scaler, maf, x[want])[0]
    assert np.array_equal(alone, logp[want])
