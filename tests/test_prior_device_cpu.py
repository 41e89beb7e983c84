"""``Prior(dists, device=...)`` and its host-side table (``Prior.device_table``): family codes, shapes, loc / scale and
the log-normalisers the device reads, the choice of where the prior runs, and pickling.  No GPU."""
import pickle

import numpy as np
import pytest
import scipy.special as sp
from scipy import stats as ss

from pocomc_amd.prior import DEVICE_FAMILIES, NPAR, Prior

# (frozen distribution, family code, shapes as the device reads them (p0, p1), loc, scale, family constant p2)
CASES = [
    (ss.truncnorm(-1, 2), 3, (-1, 2), 0.0, 1.0, None),
    (ss.truncnorm(a=5, b=8, loc=1, scale=2), 3, (5, 8), 1.0, 2.0, None),
    (ss.loguniform(1e-3, 10), 4, (1e-3, 10), 0.0, 1.0, np.log(np.log(10) - np.log(1e-3))),
    (ss.reciprocal(a=0.5, b=2, scale=3), 4, (0.5, 2), 0.0, 3.0, np.log(np.log(2) - np.log(0.5))),
    (ss.lognorm(0.5), 5, (0.5, 0.5), 0.0, 1.0, 0.0),
    (ss.lognorm(s=1.7, loc=-1, scale=2), 5, (1.7, 2 * 1.7 ** 2), -1.0, 2.0, 0.0),
    (ss.halfnorm(), 6, (0, 0), 0.0, 1.0, 0.5 * np.log(2 / np.pi)),
    (ss.halfnorm(1, 0.3), 6, (0, 0), 1.0, 0.3, 0.5 * np.log(2 / np.pi)),
    (ss.expon(loc=-2, scale=5), 7, (0, 0), -2.0, 5.0, 0.0),
    (ss.gamma(2.0), 8, (1.0, 0), 0.0, 1.0, 0.0),
    (ss.gamma(a=2.0, loc=-3), 8, (1.0, 0), -3.0, 1.0, 0.0),
    (ss.gamma(0.5, 1, 2), 8, (-0.5, 0), 1.0, 2.0, np.log(np.sqrt(np.pi))),
    (ss.invgamma(3, scale=2), 9, (4.0, 0), 0.0, 2.0, np.log(2.0)),
    (ss.beta(2, 5, 0, 1), 10, (1.0, 4.0), 0.0, 1.0, np.log(1 / 30)),
    (ss.beta(a=0.5, b=0.5, loc=-1, scale=2), 10, (-0.5, -0.5), -1.0, 2.0, np.log(np.pi)),
    (ss.cauchy(3, 0.1), 11, (0, 0), 3.0, 0.1, np.log(np.pi)),
    (ss.halfcauchy(scale=4), 12, (0, 0), 0.0, 4.0, np.log(2 / np.pi)),
    (ss.laplace(0.2, 0.7), 13, (0, 0), 0.2, 0.7, 0.0),
    (ss.t(1), 14, (1.0, 1.0), 0.0, 1.0, -np.log(np.pi)),
    (ss.t(df=30, loc=1, scale=2), 14, (30.0, 15.5), 1.0, 2.0, None),
    (ss.uniform(-1, 3), 1, None, -1.0, 3.0, None),
    (ss.norm(scale=2), 2, None, 0.0, 2.0, None),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_table_of_each_family(i):
    d, fam, shapes, loc, scale, c = CASES[i]
    tab = Prior([d, ss.gamma(3.0)], device=True).device_table()
    assert tab["family"].dtype == np.int32 and list(tab["family"]) == [fam, 8]
    assert tab["loc"][0] == loc and tab["scale"][0] == scale
    par = tab["par"]
    assert par.shape == (NPAR, 2) and par.dtype == np.float64
    assert par[3, 0] == pytest.approx(np.log(scale), abs=1e-15)
    if shapes is not None:
        np.testing.assert_allclose(par[:2, 0], shapes, rtol=1e-15)
    if c is not None:
        assert par[2, 0] == pytest.approx(c, rel=1e-14, abs=1e-14)
    assert par[2, 1] == pytest.approx(np.log(2.0), rel=1e-14)          # gamma(3): gammaln(3) = log 2


def test_truncnorm_and_t_normalisers_against_scipy():
    """truncnorm: the log-mass is what truncnorm.logpdf subtracts from the normal's at an interior point (far tail
    included); t: log(poch(df/2, 1/2)) - (log df + log pi) / 2 is t.logpdf(0)."""
    for a, b in [(-1, 2), (5, 8), (-np.inf, 0.3), (-30, -25), (0, np.inf)]:
        d = ss.truncnorm(a, b)
        c = Prior([d], device=True).device_table()["par"][2, 0]
        z = 0.5 * (a + b) if np.isfinite(a + b) else (b - 0.5 if np.isfinite(b) else a + 0.5)
        assert c == pytest.approx(ss.norm.logpdf(z) - d.logpdf(z), rel=1e-12, abs=1e-12), (a, b)
    for df in (1.0, 2.5, 30.0):
        tab = Prior([ss.t(df)], device=True).device_table()
        assert tab["par"][2, 0] == pytest.approx(ss.t(df).logpdf(0.0), rel=1e-13)
        assert tab["par"][2, 0] == pytest.approx(sp.gammaln((df + 1) / 2) - sp.gammaln(df / 2)
                                                 - 0.5 * np.log(df * np.pi), rel=1e-10)
    for a, b in [(2.0, 5.0), (0.3, 0.7)]:
        assert Prior([ss.beta(a, b)], device=True).device_table()["par"][2, 0] == \
            pytest.approx(sp.gammaln(a) + sp.gammaln(b) - sp.gammaln(a + b), rel=1e-13)
    for a in (0.5, 3.7):
        assert Prior([ss.invgamma(a)], device=True).device_table()["par"][2, 0] == pytest.approx(sp.gammaln(a), rel=1e-14)


def test_every_family_name_has_a_code():
    assert set(DEVICE_FAMILIES.values()) == set(range(1, 15))
    assert DEVICE_FAMILIES["loguniform"] == DEVICE_FAMILIES["reciprocal"]


def test_unsupported_factor_raises_naming_it():
    for bad, word in [(ss.chi2(3), "chi2"), (ss.vonmises(1.0), "vonmises"), (object(), "object")]:
        with pytest.raises(ValueError, match=rf"dimension 2: .*{word}"):
            Prior([ss.norm(), ss.gamma(2.0), bad], device=True)
    with pytest.raises(ValueError, match="dimension 0"):
        Prior([ss.norm(0, -1)], device=True)                            # invalid parameters
    with pytest.raises(ValueError, match="device"):
        Prior([ss.norm()], device="yes")


def test_auto_and_false():
    """"auto" is the two-family rule (a gamma factor keeps the prior on the host); False never gives a table."""
    assert Prior([ss.uniform(-1, 2), ss.gamma(2.0)]).device_table() is None
    assert Prior([ss.uniform(-1, 2), ss.gamma(2.0)]).device_descriptor() is None
    tab = Prior([ss.uniform(-1, 2), ss.norm(1, 3)]).device_table()
    assert list(tab["family"]) == [1, 2] and tab["par"] is None
    assert list(tab["loc"]) == [-1, 1] and list(tab["scale"]) == [2, 3]
    for dists in ([ss.uniform(-1, 2)], [ss.gamma(2.0)]):
        p = Prior(dists, device=False)
        assert p.device_table() is None and p.device_descriptor() is None
    # device=True with uniform / normal factors only: the same table as "auto" (no parameter table)
    t2 = Prior([ss.uniform(-1, 2), ss.norm(1, 3)], device=True).device_table()
    assert all(np.array_equal(tab[k], t2[k]) for k in ("family", "loc", "scale")) and t2["par"] is None


def test_host_logpdf_is_unchanged():
    dists = [ss.gamma(2.0, loc=-1), ss.beta(2, 3), ss.uniform(0, 1)]
    x = np.random.default_rng(0).uniform(-0.5, 1.5, size=(200, 3))
    want = sum(d.logpdf(x[:, j]) for j, d in enumerate(dists))
    for dev in ("auto", True, False):
        assert np.array_equal(Prior(dists, device=dev).logpdf(x), want)


@pytest.mark.parametrize("device", ["auto", True, False])
def test_pickle_keeps_the_choice(device):
    p = Prior([ss.loguniform(0.1, 10), ss.norm()], device=device)
    p._ddesc, p._dtensors = object(), [object()]           # stand-ins for the uploaded descriptor
    q = pickle.loads(pickle.dumps(p))
    assert q.device == device and not hasattr(q, "_ddesc") and not hasattr(q, "_dtensors")
    tq, tp = q.device_table(), Prior([ss.loguniform(0.1, 10), ss.norm()], device=device).device_table()
    assert (tq is None) == (tp is None)
    if tq is not None:
        assert all(np.array_equal(tq[k], tp[k]) for k in ("family", "loc", "scale", "par"))
    old = Prior([ss.norm()])
    st = old.__getstate__()
    st.pop("device")                                        # a state saved before the choice existed
    r = Prior.__new__(Prior)
    r.__setstate__(st)
    assert r.device == "auto"
