"""``pocomc_amd.TruncatedGaussianPrior`` without a GPU: the box's log mass against exact references (``truncnorm``, a product of
them, ``dblquad``) and against a counting estimate, the special cases, determinism, the constructor's refusals, the rest of the
prior protocol, and the new entry's ABI and refusals, which come before any launch."""
import ctypes as C
import pickle

import numpy as np
import pytest

import gauss_box_model as gbm
import gauss_prior_model as gpm

INF = np.inf


def free(k):
    return np.stack([np.full(k, -INF), np.full(k, INF)], axis=1)


def truncnorm_log_mass(a, b):
    """log of the normal mass of [a, b] as ``scipy.stats.truncnorm`` itself has it: log phi(z) - truncnorm.logpdf(z)."""
    from scipy.stats import norm, truncnorm
    z = 0.5 * (a + b) if np.isfinite(a) and np.isfinite(b) else (a + 1.0 if np.isfinite(a) else b - 1.0)
    return float(norm.logpdf(z) - truncnorm.logpdf(z, a, b))


def model_values(prior, x):
    blk = prior.device_block()
    return gbm.gauss_box_model(x, blk["mean"], blk["linv_packed"], float(blk["logc"]), blk["lo"], blk["hi"])


# ------------------------------------------------------------------------------------------------------------------
# log_mass against exact references
# ------------------------------------------------------------------------------------------------------------------
def test_one_column_is_scipys_truncnorm():
    import pocomc_amd as pc
    from scipy.stats import truncnorm
    m, sd, lo, hi = 0.7, 1.3, -0.4, 2.9
    prior = pc.TruncatedGaussianPrior([m], [[sd * sd]], [[lo, hi]])
    a, b = (lo - m) / sd, (hi - m) / sd
    want = truncnorm_log_mass(a, b)
    assert abs(prior.log_mass - want) <= 1e-12 * abs(want) and prior.log_mass_spread == 0.0
    x = np.random.default_rng(0).uniform(lo - 0.5, hi + 0.5, size=(200, 1))
    x[0], x[1] = lo, hi
    got, ref = model_values(prior, x), truncnorm.logpdf(x[:, 0], a, b, loc=m, scale=sd)
    inside = (x[:, 0] >= lo) & (x[:, 0] <= hi)
    assert inside[:2].all() and 20 < inside.sum() < 190
    assert np.isneginf(got[~inside]).all() and np.isneginf(ref[~inside]).all()
    assert (np.abs(got[inside] - ref[inside]) <= 1e-12 * np.maximum(1.0, np.abs(ref[inside]))).all()


def test_a_diagonal_covariance_is_a_product_of_truncnorms():
    import pocomc_amd as pc
    from scipy.stats import truncnorm
    rng = np.random.default_rng(6)
    k = 6
    mean, sd = rng.normal(size=k) * 2.0, rng.uniform(0.5, 3.0, size=k)
    lo, hi = mean - rng.uniform(0.5, 2.5, size=k) * sd, mean + rng.uniform(0.5, 2.5, size=k) * sd
    hi[2], lo[4] = INF, -INF
    prior = pc.TruncatedGaussianPrior(mean, np.diag(sd * sd), np.stack([lo, hi], axis=1))
    a, b = (lo - mean) / sd, (hi - mean) / sd
    want = sum(truncnorm_log_mass(a[j], b[j]) for j in range(k))
    print(f"k = 6, diagonal: log_mass {prior.log_mass!r}, the truncnorm masses' {want!r}")
    assert abs(prior.log_mass - want) <= 1e-12 * abs(want) and prior.log_mass_spread == 0.0
    x = mean + rng.normal(size=(200, k)) * sd * 0.8
    ref = sum(truncnorm.logpdf(x[:, j], a[j], b[j], loc=mean[j], scale=sd[j]) for j in range(k))
    got = model_values(prior, x)
    inside = np.isfinite(ref)
    assert 30 < inside.sum() < 190 and np.array_equal(np.isfinite(got), inside) and np.isneginf(got[~inside]).all()
    assert (np.abs(got[inside] - ref[inside]) <= 1e-12 * np.maximum(1.0, np.abs(ref[inside]))).all()


def test_two_correlated_columns_against_dblquad():
    import pocomc_amd as pc
    from scipy.integrate import dblquad
    from scipy.stats import multivariate_normal
    mean, cov = np.array([0.3, -0.2]), np.array([[1.5, 0.9], [0.9, 1.1]])
    lo, hi = np.array([-0.8, -1.5]), np.array([1.9, 0.7])
    prior = pc.TruncatedGaussianPrior(mean, cov, np.stack([lo, hi], axis=1))
    pdf = multivariate_normal(mean, cov).pdf
    want, err = dblquad(lambda y, x: pdf([x, y]), lo[0], hi[0], lo[1], hi[1], epsabs=1e-13, epsrel=1e-13)
    print(f"k = 2: mass {np.exp(prior.log_mass)!r}, dblquad {want!r} +- {err:.1e}, spread {prior.log_mass_spread!r}")
    assert 0.1 < want < 0.9 and abs(np.exp(prior.log_mass) - want) <= 1e-9 * want
    assert prior.log_mass_spread <= 1e-3


# ------------------------------------------------------------------------------------------------------------------
# log_mass against a counting estimate
# ------------------------------------------------------------------------------------------------------------------
def counting_case(k, bounded, half_width):
    rng = np.random.default_rng(100 + k)
    mean, cov = rng.normal(size=k), gpm.random_cov(k, 30.0, rng) * 2.0
    sd = np.sqrt(np.diag(cov))
    b = free(k)
    for i, j in enumerate(bounded):
        b[j] = mean[j] - half_width * sd[j], mean[j] + half_width * sd[j]
        if i == 1:
            b[j, 1] = INF                                                 # one of them one-sided
    return mean, cov, b, rng


@pytest.mark.parametrize("k,bounded,half_width", [(3, [0, 1, 2], 1.5), (5, [0, 1, 2, 3, 4], 2.0), (33, [0, 7, 8, 32], 1.6)])
def test_a_correlated_box_against_counting(k, bounded, half_width):
    """4e6 draws of N(mean, cov): the share inside the box is within 5 binomial standard errors sqrt(p (1 - p) / N) of
    exp(log_mass)."""
    import pocomc_amd as pc
    mean, cov, b, rng = counting_case(k, bounded, half_width)
    prior = pc.TruncatedGaussianPrior(mean, cov, b)
    assert prior.log_mass_spread is not None and prior.log_mass_spread <= 1e-3
    S = np.array(bounded)
    LS = np.linalg.cholesky(cov)[S]                                       # the bounded columns of mean + z @ L.T
    N, inside = 4_000_000, 0
    for _ in range(20):
        xs = mean[S] + rng.standard_normal((N // 20, k)) @ LS.T
        inside += int(((xs >= b[S, 0]) & (xs <= b[S, 1])).all(axis=1).sum())
    p, mass = inside / N, float(np.exp(prior.log_mass))
    se = np.sqrt(p * (1 - p) / N)
    print(f"k = {k}, {len(S)} bounded: mass {mass:.8f}, counted {p:.8f} +- {se:.1e}, spread {prior.log_mass_spread:.2e}")
    assert 0.1 < p < 0.9
    assert abs(mass - p) <= 5 * se
    # the marginal on the bounded columns carries all of it: the same bits as the 4-column prior
    marginal = pc.TruncatedGaussianPrior(mean[S], cov[np.ix_(S, S)], b[S])
    assert marginal.log_mass == prior.log_mass and marginal.log_mass_spread == prior.log_mass_spread


def test_the_integration_agrees_with_scipys():
    """The constructor's own integration (three and more correlated bounded columns) against scipy's Genz routine, whose
    spread between calls is 3e-8 (3 columns) to 1e-5 (12 columns): 1e-4 covers both errors with a factor of 5."""
    import pocomc_amd as pc
    from scipy.stats import multivariate_normal
    for k in (3, 6):
        mean, cov, b, _ = counting_case(k, list(range(k)), 1.7)
        prior = pc.TruncatedGaussianPrior(mean, cov, b)
        ref = float(multivariate_normal.cdf(b[:, 1], mean, cov, maxpts=1000000 * k, abseps=1e-9, releps=1e-7, lower_limit=b[:, 0]))
        print(f"k = {k}: log_mass {prior.log_mass!r}, scipy {np.log(ref)!r}")
        assert abs(prior.log_mass - np.log(ref)) <= 1e-4


# ------------------------------------------------------------------------------------------------------------------
# special cases, determinism
# ------------------------------------------------------------------------------------------------------------------
def test_all_infinite_bounds_are_the_gaussian_prior():
    import pocomc_amd as pc
    rng = np.random.default_rng(5)
    mean, cov = rng.normal(size=5), gpm.random_cov(5, 100.0, rng)
    prior, plain = pc.TruncatedGaussianPrior(mean, cov, free(5)), pc.GaussianPrior(mean, cov)
    assert prior.log_mass == 0.0 and np.signbit(prior.log_mass) == False and prior.logc_box == plain.logc   # noqa: E712
    blk, pblk = prior.device_block(), plain.device_block()
    for key in pblk:
        assert np.array_equal(blk[key], pblk[key]), key
    x = gpm.draws(mean, cov, 50, 3.0, rng)
    x[3, 2] = np.nan
    want = gpm.gauss_block_model(x, pblk["mean"], pblk["linv_packed"], float(pblk["logc"]))
    assert np.array_equal(model_values(prior, x).view(np.int64), want.view(np.int64))


def test_one_sided_limits():
    import pocomc_amd as pc
    from scipy.stats import norm
    rng = np.random.default_rng(8)
    mean, cov = rng.normal(size=3), gpm.random_cov(3, 30.0, rng)
    sd = np.sqrt(np.diag(cov))
    for a in (-0.5, 1.0):
        b = free(3)
        b[1, 0] = mean[1] + a * sd[1]
        prior = pc.TruncatedGaussianPrior(mean, cov, b)
        want = np.log(1.0 - norm.cdf(a))
        assert abs(prior.log_mass - want) <= 1e-12 * abs(want), (a, prior.log_mass, want)
        b = free(3)
        b[1, 1] = mean[1] + a * sd[1]
        assert abs(pc.TruncatedGaussianPrior(mean, cov, b).log_mass - np.log(norm.cdf(a))) <= 1e-12 * abs(np.log(norm.cdf(a)))


def test_the_constructor_is_deterministic_and_leaves_numpys_generator_alone():
    import pocomc_amd as pc
    mean, cov, b, _ = counting_case(4, [0, 1, 2, 3], 1.5)
    np.random.seed(3)
    before = np.random.get_state()
    first = pc.TruncatedGaussianPrior(mean, cov, b)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    np.random.standard_normal(5)                                          # (whatever else the process draws in between)
    second = pc.TruncatedGaussianPrior(mean, cov, b)
    assert first.log_mass == second.log_mass and first.log_mass_spread == second.log_mass_spread
    assert 0.0 < first.log_mass_spread <= 1e-3


# ------------------------------------------------------------------------------------------------------------------
# the constructor's refusals
# ------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    import pocomc_amd as pc
    mean, cov = np.zeros(3), np.eye(3) + 0.3
    T = pc.TruncatedGaussianPrior

    def refused(text, *args, **kw):
        with pytest.raises(ValueError, match=text):
            T(*args, **kw)
    b = free(3)
    b[1, 0] = np.nan
    refused("column 1 hold a NaN", mean, cov, b)
    b = free(3)
    b[2] = 1.0, 1.0
    refused(r"column 2: lo = 1.0 is not below hi = 1.0", mean, cov, b)
    b[2] = 2.0, -2.0
    refused(r"column 2: lo = 2.0 is not below hi = -2.0", mean, cov, b)
    b[2] = INF, INF
    refused("column 2", mean, cov, b)
    refused(r"bounds must have shape \(3, 2\), got \(2, 2\)", mean, cov, free(2))
    refused(r"bounds must have shape \(3, 2\), got \(2, 3\)", mean, cov, free(3).T)
    refused(r"bounds must have shape \(3, 2\), got \(6,\)", mean, cov, free(3).ravel())
    refused("bounds must be a", mean, cov, [["a", "b"]] * 3)
    # GaussianPrior's checks, in its words
    refused(r"GaussianPrior: mean\[1\] is not finite", [0.0, np.nan, 0.0], cov, free(3))
    refused("GaussianPrior: cov is not positive definite", mean, -np.eye(3), free(3))
    refused(r"mean has 158 dimensions \(1 <= k <= 157\)", np.zeros(158), np.eye(158), free(158))
    for bad in (1e-3, INF, -INF, np.nan):
        refused("log_mass must be a finite float <= 0", mean, cov, free(3), log_mass=bad)
    refused("log_mass must be a finite float <= 0", mean, cov, free(3), log_mass="x")
    # 13 correlated bounded columns
    rng = np.random.default_rng(13)
    m13, c13 = rng.normal(size=13), gpm.random_cov(13, 30.0, rng)
    b13 = np.stack([m13 - 2.0, m13 + 2.0], axis=1)
    assert pc.prior.MAX_CORRELATED_BOUNDS == 12
    refused(r"13 correlated bounded columns.*MAX_CORRELATED_BOUNDS = 12.*log_mass= takes a value computed elsewhere", m13, c13, b13)
    given = T(m13, c13, b13, log_mass=-2.5)
    assert given.log_mass == -2.5 and given.log_mass_spread is None and given.logc_box == given.logc + -2.5
    assert T(m13, np.diag(np.diag(c13)), b13).log_mass < 0.0              # (a diagonal covariance: any number of columns)
    # a box at mean + 40 sd on two correlated columns: the mass underflows
    c2 = np.array([[1.0, 0.5], [0.5, 1.0]])
    refused(r"not positive and finite.*log_mass= takes a value computed elsewhere", np.zeros(2), c2, [[40.0, 41.0], [40.0, 41.0]])
    assert T(np.zeros(2), c2, [[40.0, 41.0], [40.0, 41.0]], log_mass=-1650.0).log_mass == -1650.0
    # mean need not lie in the box
    assert T(np.zeros(2), c2, [[1.0, 3.0], [0.5, INF]]).log_mass < np.log(0.2)


def test_a_spread_above_the_limit_is_refused(monkeypatch):
    import pocomc_amd as pc
    mean, cov, b, _ = counting_case(3, [0, 1, 2], 1.5)
    monkeypatch.setattr(pc.prior, "MASS_POINTS", 4)                        # 12 points per seed: the two integrations disagree
    monkeypatch.setattr(pc.prior, "MASS_SHIFTS", 1)
    assert pc.prior.MAX_LOG_MASS_SPREAD == 1e-3
    with pytest.raises(ValueError, match=r"differ by .* in the log.*log_mass= takes a value computed elsewhere"):
        pc.TruncatedGaussianPrior(mean, cov, b)


# ------------------------------------------------------------------------------------------------------------------
# the protocol
# ------------------------------------------------------------------------------------------------------------------
def test_rvs_bounds_dim_and_pickling():
    """The draws' moments: column means and covariance of 2e5 draws of ``rvs`` against those of 2e6 rejection draws made here
    with another generator.  Each difference is held to 5 of its standard errors: for a mean sqrt(var_j (1 / n1 + 1 / n2)),
    for a covariance sqrt((E[(x_i - m_i)^2 (x_j - m_j)^2] - c_ij^2) (1 / n1 + 1 / n2)), the variances taken from the larger
    sample."""
    import pocomc_amd as pc
    mean, cov, b, rng = counting_case(4, [0, 2], 1.2)
    prior = pc.TruncatedGaussianPrior(mean, cov, b)
    assert prior.dim == 4 and not hasattr(prior, "device_descriptor") and not hasattr(prior, "step_stage")
    assert isinstance(prior, pc.GaussianPrior) and callable(prior.logpdf_device) and callable(prior.logpdf)
    assert np.array_equal(prior.bounds, b) and prior.bounds is not prior.bounds
    prior.bounds[0, 0] = 99.0                                             # a copy: the prior does not move
    assert np.array_equal(prior.bounds, b)
    np.random.seed(11)
    a = prior.rvs(7)
    np.random.seed(11)
    assert a.shape == (7, 4) and a.dtype == np.float64 and np.array_equal(prior.rvs(7), a) and not np.array_equal(prior.rvs(7), a)
    # rejection from mean + z @ L.T, in draw order
    np.random.seed(11)
    m = int(np.ceil(1.2 * 7 / np.exp(prior.log_mass))) + 16
    raw = mean + np.random.standard_normal((m, 4)) @ np.linalg.cholesky(cov).T
    raw = raw[((raw >= b[:, 0]) & (raw <= b[:, 1])).all(axis=1)]
    assert len(raw) >= 7 and np.array_equal(raw[:7], a)
    assert prior.rvs().shape == (1, 4) and prior.rvs(0).shape == (0, 4)
    np.random.seed(12)
    n1, n2 = 200_000, 2_000_000
    x1 = prior.rvs(n1)
    assert x1.shape == (n1, 4) and ((x1 >= b[:, 0]) & (x1 <= b[:, 1])).all()
    L, x2 = np.linalg.cholesky(cov), []
    while sum(len(v) for v in x2) < n2:
        v = mean + rng.standard_normal((500_000, 4)) @ L.T
        x2.append(v[((v >= b[:, 0]) & (v <= b[:, 1])).all(axis=1)])
    x2 = np.concatenate(x2)[:n2]
    m2, c2 = x2.mean(axis=0), np.cov(x2.T)
    d2 = x2 - m2
    f = 1.0 / n1 + 1.0 / n2
    assert (np.abs(x1.mean(axis=0) - m2) <= 5 * np.sqrt(np.diag(c2) * f)).all()
    c1 = np.cov(x1.T)
    for i in range(4):
        for j in range(i + 1):
            se = np.sqrt((np.mean(d2[:, i] ** 2 * d2[:, j] ** 2) - c2[i, j] ** 2) * f)
            assert abs(c1[i, j] - c2[i, j]) <= 5 * se, (i, j, c1[i, j], c2[i, j], se)
    assert abs(c2[0, 0] - cov[0, 0]) > 0.1 * cov[0, 0]                    # (the box does move the moments)
    # the state
    back = pickle.loads(pickle.dumps(prior))
    assert type(back) is pc.TruncatedGaussianPrior and back is not prior
    st, st2 = prior.__getstate__(), back.__getstate__()
    assert set(st) == {"mean", "cov", "L", "linv_packed", "logc", "bounds", "log_mass", "log_mass_spread"}
    for key in st:
        assert not hasattr(st[key], "device") or isinstance(st[key], np.ndarray), key
        assert np.array_equal(st[key], st2[key]), key
    blk, blk2 = prior.device_block(), back.device_block()
    assert set(blk) == {"mean", "linv_packed", "logc", "lo", "hi"}
    for key in blk:
        assert blk[key].dtype == np.float64 and np.array_equal(blk[key].view(np.int64), blk2[key].view(np.int64)), key
    assert float(blk["logc"]) == prior.logc + prior.log_mass == prior.logc_box
    assert np.array_equal(blk["lo"], b[:, 0]) and np.array_equal(blk["hi"], b[:, 1])
    assert set(pc.GaussianPrior(mean, cov).__getstate__()) == {"mean", "cov", "L", "linv_packed", "logc"}
    assert set(pc.GaussianPrior(mean, cov).device_block()) == {"mean", "linv_packed", "logc"}
    assert "TruncatedGaussianPrior" in pc.__all__


def test_rvs_refuses_a_hopeless_box_before_drawing():
    import pocomc_amd as pc
    prior = pc.TruncatedGaussianPrior([0.0], [[1.0]], [[6.0, INF]])       # a mass of 1e-9
    np.random.seed(1)
    before = np.random.get_state()
    with pytest.raises(RuntimeError, match="draws of the untruncated normal"):
        prior.rvs(1)
    assert np.array_equal(before[1], np.random.get_state()[1]) and before[2] == np.random.get_state()[2]


# ------------------------------------------------------------------------------------------------------------------
# the ABI and the entry's refusals: nothing is launched (there is no device here, every array address is a fake)
# ------------------------------------------------------------------------------------------------------------------
def test_the_abi_grew_by_one_entry_and_one_struct():
    import os
    from pocomc_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    hdr = open(os.path.join(root, "include", "pocomc_amd.h")).read()
    for text in ("#define PMC_ABI_VERSION 9", "typedef struct pmc_gauss_box {", "const double* lo[PMC_GAUSS_BLOCKS_MAX];",
                 "const double* hi[PMC_GAUSS_BLOCKS_MAX];", "} pmc_gauss_box_t;",
                 "int pmc_gauss_box_logpdf(const pmc_gauss_blocks_t* g, const pmc_gauss_box_t* box, const double* x, "
                 "int64_t row_stride,\n                         int64_t col_stride, int64_t n, const double* base, double* logp, "
                 "void* stream);"):
        assert text in hdr, text
    assert lib.pmc_abi_version() == 9 and hasattr(lib, "pmc_gauss_box_logpdf")
    assert C.sizeof(_lib.pmc_gauss_box_t) == 128 and _lib.pmc_gauss_box_t.hi.offset == 64
    assert C.sizeof(_lib.pmc_gauss_blocks_t) == 312


def entry_refusals(call, lib, descriptor, box_of):
    """Every refusal of ``pmc_gauss_box_logpdf`` by its text; ``call(g, box, **arguments)`` makes the call (``g`` / ``box`` None:
    a NULL pointer), ``descriptor(**kw)`` gives ``(g, rest)`` and ``box_of(g)`` a full box for it."""
    seen = set()

    def refused(word, change=None, null=False, **kw):
        args = {a: kw.pop(a) for a in ("x", "n", "rs", "cs", "base", "logp") if a in kw}
        g, rest = descriptor(**kw)
        box = box_of(g)
        if change:
            box = change(g, rest, box)
        rc = call(None if null else g, box, **args)
        msg = lib.pmc_last_error().decode()
        assert rc != 0 and msg.startswith("pmc_gauss_box_logpdf: ") and word in msg, (word, rc, msg)
        seen.add(msg)
        return box

    def keep(f):
        return lambda g, r, box: (f(g, r, box), box)[1]
    refused("bad descriptor", null=True)
    for nb in (0, -1, 9):
        refused("n_blocks must lie in 1 .. 8", keep(lambda g, r, box: setattr(g, "n_blocks", nb)))
    for field in ("cols", "mean", "linv"):
        refused("bad block descriptor", keep(lambda g, r, box: getattr(g, field).__setitem__(1, None)))
    refused("at least 1 column", dims=(3, 0))
    refused("n_dim too large (D <= 157)", dims=(3, 4), D=158)
    refused("more columns than x", dims=(3, 4), D=6)
    refused("rest and rest_cols go together", keep(lambda g, r, box: setattr(g, "rest_cols", None)), Dr=2)
    refused("rest and rest_cols go together", keep(lambda g, r, box: setattr(g, "rest", None)), Dr=2)
    refused("bad prior descriptor", keep(lambda g, r, box: setattr(r, "family", None)), Dr=2)
    refused("parameter table", keep(lambda g, r, box: setattr(r, "par", None)), Dr=2)
    refused("base and rest exclude each other", Dr=2, base=True)
    refused("bad box descriptor", lambda g, r, box: None)
    refused("lo and hi of a block go together", keep(lambda g, r, box: box.lo.__setitem__(1, None)))
    refused("lo and hi of a block go together", keep(lambda g, r, box: box.hi.__setitem__(0, None)))
    for kw in (dict(x=None), dict(logp=None), dict(n=-1), dict(rs=-1), dict(cs=-1)):
        refused("bad argument", **kw)
    refused("too many rows", n=64 * 2 ** 31)
    assert len(seen) == 14                                                # texts of their own
    # a NULL pair is no refusal (the block has no box), and entries behind n_blocks are not read
    def pair(g, r, box):
        box.lo[1] = box.hi[1] = None
        box.lo[2], box.hi[3] = 0x10, 0x20
        return box
    refused("bad argument", pair, x=None)
    return seen


def descriptor(dims=(3, 4), D=9, Dr=0):
    from pocomc_amd import _lib
    g = _lib.pmc_gauss_blocks_t(n_blocks=len(dims), D=D)
    for b, k in enumerate(dims):
        g.dim[b], g.logc[b] = k, 1.0
        g.cols[b], g.mean[b], g.linv[b] = 0x1000 + 0x100 * b, 0x2000 + 0x100 * b, 0x3000 + 0x1000 * b
    rest = _lib.pmc_prior_t(family=0x70, loc=0x80, scale=0x90, D=max(Dr, 1), par=0xA0, n_extended=1)
    if Dr:
        g.rest, g.rest_cols = C.addressof(rest), 0x5000
    return g, rest


def fake_box(g):
    from pocomc_amd import _lib
    box = _lib.pmc_gauss_box_t()
    for b in range(max(min(g.n_blocks, 8), 0)):
        box.lo[b], box.hi[b] = 0x8000 + 0x100 * b, 0x9000 + 0x100 * b
    return box


def test_the_entry_refuses_before_any_launch():
    from pocomc_amd import _lib
    lib = _lib.load()

    def call(g, box, x=0x6000, n=21, rs=9, cs=1, base=None, logp=0x7000):
        return lib.pmc_gauss_box_logpdf(None if g is None else C.byref(g), None if box is None else C.byref(box), x, rs, cs, n,
                                        0xB000 if base else None, logp, None)
    entry_refusals(call, lib, descriptor, fake_box)
    # n == 0 returns 0 and reads nothing; a bad descriptor or a NULL box is refused at n == 0 as well
    g, rest = descriptor()
    box = fake_box(g)
    assert lib.pmc_gauss_box_logpdf(C.byref(g), C.byref(box), None, 9, 1, 0, None, None, None) == 0
    assert lib.pmc_gauss_box_logpdf(C.byref(g), None, None, 9, 1, 0, None, None, None) != 0
    # the old entry keeps its texts under its own name
    assert lib.pmc_gauss_blocks_logpdf(None, 0x6000, 9, 1, 21, None, 0x7000, None) != 0
    assert lib.pmc_last_error().decode() == "pmc_gauss_blocks_logpdf: bad descriptor"
