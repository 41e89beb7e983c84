"""``tests/pool_regimes.py`` pinned against the oracle without a GPU, so that ``tests/test_gpu_pool_regimes.py`` cannot be
vacuous: in every regime x size the float64 oracle itself meets the criterion against the exact reference, the exact
trim ratios reproduce the oracle's bin wherever the case is no knife edge, and the knife edges are listed and capped."""
import mpmath
import numpy as np
import pytest

import pool_regimes as pr
from oracle import tools as otools


@pytest.mark.parametrize("regime", pr.REGIMES)
def test_oracle_statistics_meet_the_criterion(regime):
    for P in pr.SIZES:
        lw, ex, env = pr.stats_case(regime, P)
        with np.errstate(invalid="ignore"):
            o = pr.oracle_stats(lw)
        assert np.max(lw) == ex["max"]
        for k, q in pr.STAT_BOUND.items():
            e = pr.err(o[k], ex[k])
            assert e <= pr.allowed(q, ex[k], env[k]), (regime, P, k, e, env[k])
        if regime == "one_hot":
            assert o["ess"] == 1.0 and o["logz"] == 0.0 and ex["ess"] == 1 and ex["logz"] == 0
        if regime == "equal":
            assert ex["ess"] == P and o["s1"] == P == o["s2"]     # (the oracle's ESS divides by P first: 1/P rounds)


@pytest.mark.parametrize("regime", ["gauss", "very_wide", "holes", "shifted_down"])
def test_extended_precision_reference_equals_the_50_digit_one(regime):
    """Above ``MP_MAX`` elements the reference is summed in extended precision: at ``MP_MAX`` both exist and agree to
    1e-17 of the value, a hundred times below the smallest bound in use (1e-13 relative, one float64 rounding)."""
    lw = pr.logw(regime, pr.MP_MAX)
    a, b = pr.exact_stats(lw, force="mp"), pr.exact_stats(lw, force="ld")
    for k in ("s1", "s2", "ess", "logz"):
        assert abs(a[k] - b[k]) <= 1e-17 * abs(a[k]), (k, float(abs(a[k] - b[k]) / abs(a[k])))


def test_uss_reference_is_the_float64_definition():
    """USS is compared as the reference defines it in float64; its exact value is reported next to it."""
    for regime in ("gauss", "near_equal", "wide"):
        w = pr.weights(regime, 4097)
        for k in (1, 64, 4097, 40970):
            ref, env, exact = pr.uss_reference(w, k)
            assert ref == otools.unique_sample_size(w.copy(), k)
            print(f"uss {regime} k={k}: float64 {ref:.17g} exact {exact:.17g} envelope {env:.2e}")
            assert 0 < ref <= 4097 and abs(ref - exact) <= 1e-6 * exact + 4097 * 2.0 ** -53 * k


@pytest.mark.parametrize("T", pr.HISTORY_T)
@pytest.mark.parametrize("width", [4, 300])
def test_mixture_reference_and_oracle(T, width):
    logl, beta, logz = pr.history(T, 257, width, holes=True)
    for bf in (0.0, 0.41, 1.0):
        ex = pr.exact_mixture(logl, beta, logz, bf)
        flat = logl.reshape(-1)
        for e in range(0, flat.size, max(flat.size // 48, 1)):        # the extended-precision reference against 50 digits
            if np.isfinite(flat[e]):
                with mpmath.workdps(50):
                    m = pr.mixture_mp(flat[e], beta, logz, bf)
                    assert abs(pr._mpf(ex[e]) - m) <= 1e-17 * (1 + abs(m))
        with np.errstate(invalid="ignore"):
            lw, _ = otools.compute_logw_and_logz(logl, beta, logz, bf, normalize=False)
        assert np.array_equal(np.isnan(lw), np.isneginf(flat))        # -inf * beta[0] = NaN
        assert np.array_equal(np.isnan(lw), np.isnan(ex.astype(np.float64)))
        env = pr.mixture_envelope(logl, beta, logz, bf, ex)
        ok = np.isfinite(flat)
        e = np.abs((lw.astype(np.longdouble) - ex).astype(np.float64))[ok]
        lim = np.maximum(pr.BOUND["logw"] * (1 + np.abs(ex[ok].astype(np.float64))), pr.C * env[ok])
        assert (e <= lim).all(), (T, width, bf, float((e / lim).max()))


KNIFE = []
TRIM_CASES = [(r, P) for r in pr.REGIMES for P in pr.SORT_SIZES]


@pytest.mark.parametrize("regime", pr.REGIMES)
def test_exact_trim_ratios_reproduce_the_oracles_bin(regime):
    for P in pr.SORT_SIZES:
        w = pr.weights(regime, P)
        w /= np.sum(w)
        tr = pr.trim_exact(w)
        ob = pr.oracle_trim_bin(w)
        assert ob in tr["valid"], (regime, P, ob, tr["valid"])
        if tr["knife"]:
            KNIFE.append((regime, P, ob, tr["bin"], tr["knife"]))
        else:
            assert ob == tr["bin"], (regime, P, ob, tr["bin"])
        if P <= 100_000:                                              # the oracle itself: same kept set as that bin's
            idx, wt = otools.trim_weights(np.arange(P), w.copy())
            np.testing.assert_array_equal(idx, np.nonzero(w >= tr["thr"][ob])[0])
        if regime == "equal" or tr["thr"][ob] == 0.0:                 # (one_hot from P = 101: the 99th percentile is 0.0)
            assert np.count_nonzero(w >= tr["thr"][ob]) == P


def test_knife_edges_are_few_and_where_expected():
    """Runs after the regimes above (file order).  A knife edge is a case where a bin's exact ESS ratio equals ``ess`` to
    within rounding: dropping exactly 1 % of nearly equal weights gives 0.99 up to the last bit."""
    assert len(KNIFE) > 0, "run the whole file: the trim cases fill the list"
    print(f"knife-edge trim cases: {len(KNIFE)} of {len(TRIM_CASES)} ({100.0 * len(KNIFE) / len(TRIM_CASES):.1f} %)")
    for regime, P, ob, eb, bins in KNIFE:
        print(f"  {regime} P={P}: oracle bin {ob}, exact-arithmetic bin {eb}, bins on the edge {bins}")
    assert len(KNIFE) <= 0.05 * len(TRIM_CASES)
    assert not [c for c in KNIFE if c[0] in pr.NO_KNIFE_EDGE]
    assert {("near_equal", 100), ("near_equal", 1000)} <= {(c[0], c[1]) for c in KNIFE}


def test_resampling_reference_is_the_oracles_loop():
    """``systematic_reference`` is the oracle's loop vectorised; where a position lies above the last cdf entry the
    oracle raises, and the reference reports it."""
    for regime in pr.REGIMES:
        for P in (1, 2, 17, 1000):
            w = pr.weights(regime, P)
            w = w / np.sum(w)
            for n_out in (1, max(P // 3, 1), P, 4 * P):
                for off in (0.0, 0.37, pr.ONE_BELOW):
                    idx, over = pr.systematic_reference(n_out, w, off)
                    if over.any():
                        with pytest.raises(IndexError):
                            otools.systematic_resample(n_out, w, offset=off)
                    else:
                        np.testing.assert_array_equal(idx, otools.systematic_resample(n_out, w, offset=off))


def test_exact_moments_small_case_against_fractions():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    x = 1e8 + rng.normal(size=(5, 2))
    w = rng.uniform(0.1, 1, 5)
    mean, S, v1, v2 = pr.exact_moments(x, w)
    fw = [Fraction(float(v)) for v in w]
    fx = [[Fraction(float(v)) for v in r] for r in x]
    m0 = sum(a * r[0] for a, r in zip(fw, fx)) / sum(fw)
    s00 = sum(a * (r[0] - m0) ** 2 for a, r in zip(fw, fx))
    hi = float(mean[0])
    assert abs(Fraction(hi) + Fraction(float(mean[0] - np.longdouble(hi))) - m0) <= 1e-18 * m0
    assert abs(float(S[0, 0]) - float(s00)) <= 1e-14 * float(s00)


def test_bootstrap_reference():
    lw = pr.logw("holes", 64)
    holes = np.nonzero(np.isneginf(lw))[0]
    out = pr.exact_bootstrap(lw, [np.arange(64), np.resize(holes, 64)])
    with mpmath.workdps(50):
        assert abs(out[0] - (pr.exact_stats(lw)["logz"] - mpmath.log(64))) < 1e-40 and out[1] == -mpmath.inf
