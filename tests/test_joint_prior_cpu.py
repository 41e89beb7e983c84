"""``JointPrior.layout`` (pure numpy) and the float64 restatement of the joint prior (``tests/joint_prior_model.py``): the
column maps round-trip, every bad ``columns`` is refused, and the model is -inf exactly on the rows that are off the support
of either part, row by row.  No GPU."""
import numpy as np
import pytest

import cases
import flow_prior_model as fpm
import joint_prior_model as jpm
from oracle.maf import OracleMAF
from parity import TOL
from pocomc_amd.maf_spec import MAFSpec
from pocomc_amd.prior import JointPrior


@pytest.mark.parametrize("Df,Dr", [(2, 1), (3, 4), (17, 16), (156, 1), (2, 155)])
def test_layout_round_trips_a_shuffled_columns(Df, Dr):
    D = Df + Dr
    rng = np.random.default_rng(D)
    columns = rng.permutation(D)[:Df]
    flow_cols, rest_cols = JointPrior.layout(columns.tolist(), Df, Dr)
    assert flow_cols.dtype == np.int32 and rest_cols.dtype == np.int32
    assert np.array_equal(flow_cols, columns)                            # the order given, not sorted
    assert len(rest_cols) == Dr and np.all(np.diff(rest_cols) > 0)      # the other positions, increasing
    assert np.array_equal(np.sort(np.concatenate([flow_cols, rest_cols])), np.arange(D))
    # a joint row taken apart by the maps and put together again is the row
    x = rng.normal(size=(5, D))
    y = np.empty_like(x)
    y[:, flow_cols] = x[:, flow_cols]
    y[:, rest_cols] = x[:, rest_cols]
    assert np.array_equal(x, y)
    # numpy integers and arrays are columns too, and the model's own statement of the layout agrees
    again = JointPrior.layout(np.asarray(columns, dtype=np.int16), Df, Dr)
    assert np.array_equal(again[0], flow_cols) and np.array_equal(again[1], rest_cols)
    mf, mr = jpm.layout(columns, D)
    assert np.array_equal(mf, flow_cols) and np.array_equal(mr, rest_cols)


@pytest.mark.parametrize("columns,what", [([0, 2, 2], "distinct"), ([0, 2, 5], "lie in"), ([0, -1, 2], "lie in"),
                                          ([0, 1.0, 2], "integers"), ([0.5, 1, 2], "integers"), ([0, 1], "columns for"),
                                          ([0, 1, 2, 3], "columns for"), ([[0, 1, 2]], "integers"), ("012", "integers"),
                                          ([True, False, True], "integers"), ([0, None, 2], "integers"), (3, "integers")])
def test_layout_refuses_bad_columns(columns, what):
    with pytest.raises(ValueError, match=what):
        JointPrior.layout(columns, 3, 2)


def _parts(Df=3, Dr=4, uni="affine", transform="probit"):
    spec = MAFSpec(Df, 3, univariate=uni)
    maf = OracleMAF(spec, cases.flow_params(spec, 5))
    b = np.array([[-1.0, 2.0], [0.5, np.inf], [-np.inf, 3.0]])[:Df]
    scaler = fpm.oracle_scaler(b, transform, jpm.flow_rows(b, 500, np.random.default_rng(11)))
    return scaler, maf, jpm.rest_dists(Dr), jpm.interleaved_columns(Df, Dr), b


def _rows(b, dists, columns, n, seed):
    rng = np.random.default_rng(seed)
    D = len(b) + len(dists)
    flow_cols, rest_cols = jpm.layout(columns, D)
    x = np.empty((n, D))
    x[:, flow_cols] = jpm.flow_rows(b, n, rng)
    x[:, rest_cols] = jpm.rest_rows(dists, n, rng)
    return x, flow_cols, rest_cols


@pytest.mark.parametrize("uni", ["affine", "rqs"])
def test_the_model_is_the_sum_of_its_parts_and_minus_infinity_off_the_support(uni):
    """Flow feature 0 is two-sided on (-1, 2), 1 bounded below at 0.5; rest factor 0 is uniform on [-2, 3], 2 a gamma with
    loc -1.  One bad value per row; every other row keeps its bits."""
    scaler, maf, dists, columns, b = _parts(uni=uni)
    x, flow_cols, rest_cols = _rows(b, dists, columns, 40, 3)
    good, flow_logp, terms = jpm.joint_prior_model(scaler, maf, dists, columns, x)
    assert np.isfinite(good).all()
    assert np.array_equal(good, flow_logp + terms.sum(axis=1))
    # (the oracle's flow is float32 numpy: one call on all rows rounds its matrix products differently from a call per row)
    np.testing.assert_allclose(flow_logp, fpm.flow_prior_model(scaler, maf, x[:, flow_cols])[0], rtol=TOL)
    bad = {1: (flow_cols[0], np.nan), 4: (rest_cols[1], np.nan), 7: (flow_cols[2], np.inf), 9: (rest_cols[1], -np.inf),
           12: (flow_cols[0], -1.0), 15: (flow_cols[0], 2.0), 18: (flow_cols[1], 0.5),          # on a scaler bound
           21: (rest_cols[0], 3.5), 24: (rest_cols[2], -1.5), 27: (rest_cols[3], 3.5)}          # outside a factor's support
    y = x.copy()
    for r, (j, v) in bad.items():
        y[r, j] = v
    got = jpm.joint_prior_model(scaler, maf, dists, columns, y)[0]
    rows = np.array(sorted(bad))
    keep = np.setdiff1d(np.arange(len(x)), rows)
    assert np.isneginf(got[rows]).all(), got[rows]
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    assert np.array_equal(got[keep].view(np.int64), good[keep].view(np.int64))
    # row-wise: the good rows alone give the same values
    alone = jpm.joint_prior_model(scaler, maf, dists, columns, y[keep])[0]
    assert np.array_equal(alone.view(np.int64), good[keep].view(np.int64))


def test_a_pole_of_a_factor_is_minus_infinity():
    """gamma(0.5) at its loc: scipy's logpdf is +inf there; the joint prior's value is -inf (the step rejects the row)."""
    from scipy import stats
    scaler, maf, _, _, b = _parts(Df=2, Dr=1)
    dists = [stats.gamma(0.5, loc=1.0)]
    x, flow_cols, rest_cols = _rows(b, dists, [2, 0], 6, 1)
    assert np.isfinite(jpm.joint_prior_model(scaler, maf, dists, [2, 0], x)[0]).all()
    x[3, rest_cols[0]] = 1.0
    assert np.isposinf(dists[0].logpdf(1.0))
    got = jpm.joint_prior_model(scaler, maf, dists, [2, 0], x)[0]
    assert np.isneginf(got[3]) and np.isfinite(np.delete(got, 3)).all()
