"""``pocomc_amd.GaussianPrior`` without a GPU: the numpy statement of the kernel's arithmetic (``tests/gauss_prior_model.py``)
against ``scipy.stats.multivariate_normal``, the host-side constants, the constructor's refusals, the rest of the prior
protocol, and the entry's refusals, which come before any launch."""
import ctypes as C
import pickle

import numpy as np
import pytest

import gauss_prior_model as gpm

KS = [1, 2, 5, 33, 64, 157]
CONDS = [1.0, 1e3]


def case(k, cond):
    import pocomc_amd as pc
    rng = np.random.default_rng(1000 * k + int(cond))
    mean = rng.normal(size=k) * 3.0
    cov = gpm.random_cov(k, cond, rng) * 2.5
    return pc.GaussianPrior(mean, cov), mean, cov, rng


# ------------------------------------------------------------------------------------------------------------------
# the model against scipy
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", CONDS)
@pytest.mark.parametrize("k", KS)
def test_the_model_matches_scipy(k, cond):
    """200 rows at 1x and 200 at 10x the distribution's width.  The bound is the rounding of k-term sums amplified by the
    factor's conditioning, ``8 k cond 2^-53 max(1, |scipy|)``.  Measured over these inputs: at condition number 1 between
    0 (k = 1) and 1.3e-14 (k = 157), the closest a factor of 3.6 inside the bound (k = 2: 4.9e-16 of 1.8e-15); at 1e3 at
    most 2.0e-13 (k = 5), a factor of 22 inside it."""
    from scipy.stats import multivariate_normal
    prior, mean, cov, rng = case(k, cond)
    blk = prior.device_block()
    ref = multivariate_normal(mean, cov)
    worst = 0.0
    for width in (1.0, 10.0):
        x = gpm.draws(mean, cov, 200, width, rng)
        want = np.atleast_1d(ref.logpdf(x))
        got = gpm.gauss_block_model(x, blk["mean"], blk["linv_packed"], float(blk["logc"]))
        assert got.shape == (200,) and np.isfinite(got).all()
        scale = np.maximum(1.0, np.abs(want))
        worst = max(worst, float((np.abs(got - want) / scale).max()))
        assert (np.abs(got - want) <= 8 * k * cond * 2.0 ** -53 * scale).all(), (k, cond, width, worst)
    print(f"k={k} cond={cond:g}: model against scipy, max relative difference {worst:.3e} (bound {8 * k * cond * 2.0 ** -53:.3e})")


def test_the_model_marks_bad_rows():
    prior, mean, cov, rng = case(5, 1e3)
    blk = prior.device_block()
    x = gpm.draws(mean, cov, 12, 1.0, rng)
    good = gpm.gauss_block_model(x, blk["mean"], blk["linv_packed"], float(blk["logc"]))
    x[1, 0], x[3, 4], x[5, 2] = np.nan, np.inf, -np.inf
    x[7], x[8] = 1e300, -1e300
    x[9] = 1e300 * np.array([1, -1, 1, -1, 1])
    got = gpm.gauss_block_model(x, blk["mean"], blk["linv_packed"], float(blk["logc"]))
    bad = [1, 3, 5, 7, 8, 9]
    keep = np.setdiff1d(np.arange(12), bad)
    assert np.isneginf(got[bad]).all() and not np.isnan(got).any() and np.array_equal(got[keep], good[keep])
    # the blocks' sum: left to right, on top of a start or of nothing
    two = [([3, 0], *gpm.constants(mean[:2], cov[:2, :2])), ([1, 4, 2], *gpm.constants(mean[2:], cov[2:, 2:]))]
    y = gpm.draws(mean, cov, 12, 1.0, rng)
    g0 = gpm.gauss_block_model(y[:, [3, 0]], *two[0][1:])
    g1 = gpm.gauss_block_model(y[:, [1, 4, 2]], *two[1][1:])
    assert np.array_equal(gpm.gauss_blocks_model(y, two), g0 + g1)
    start = rng.normal(size=12)
    assert np.array_equal(gpm.gauss_blocks_model(y, two, start), (start + g0) + g1)
    start[4] = -np.inf
    assert np.isneginf(gpm.gauss_blocks_model(y, two, start)[4])


# ------------------------------------------------------------------------------------------------------------------
# the constants
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 33])
def test_device_block_is_the_models_input(k):
    prior, mean, cov, _ = case(k, 1e3)
    blk = prior.device_block()
    assert set(blk) == {"mean", "linv_packed", "logc"}
    m, packed, logc = gpm.constants(mean, cov)
    assert blk["mean"].dtype == np.float64 and blk["linv_packed"].dtype == np.float64 and blk["logc"].dtype == np.float64
    assert np.array_equal(blk["mean"], m) and blk["linv_packed"].shape == (k * (k + 1) // 2,)
    assert np.array_equal(blk["linv_packed"], packed) and float(blk["logc"]) == logc
    # packed by rows: row i at i (i + 1) / 2, and it is the inverse of the Cholesky factor
    Linv = np.zeros((k, k))
    for i in range(k):
        Linv[i, :i + 1] = blk["linv_packed"][i * (i + 1) // 2: i * (i + 1) // 2 + i + 1]
    L = np.linalg.cholesky(cov)
    np.testing.assert_allclose(Linv @ L, np.eye(k), atol=1e-9)
    assert logc == np.sum(np.log(np.diag(L))) + 0.5 * k * np.log(2 * np.pi)
    blk["mean"][0] = 99.0                                                 # a copy: the prior does not move
    assert prior.device_block()["mean"][0] == m[0]


# ------------------------------------------------------------------------------------------------------------------
# the constructor
# ------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    import pocomc_amd as pc
    ok_mean, ok_cov = np.zeros(3), np.eye(3)
    assert pc.GaussianPrior(ok_mean, ok_cov).dim == 3 and pc.GaussianPrior.MAX_DIM == 157
    assert pc.GaussianPrior([0.5], [[2.0]]).dim == 1
    wide = pc.GaussianPrior(np.zeros(157), np.eye(157))
    assert wide.dim == 157 and wide.device_block()["linv_packed"].shape == (157 * 158 // 2,)

    def refused(text, mean, cov):
        with pytest.raises(ValueError, match=text):
            pc.GaussianPrior(mean, cov)
    for bad in (np.nan, np.inf, -np.inf):
        refused(r"mean\[1\] is not finite", [0.0, bad, 0.0], ok_cov)
        c = np.eye(3)
        c[2, 1] = c[1, 2] = bad
        refused(r"cov\[1, 2\] is not finite", ok_mean, c)
    refused(r"cov must have shape \(3, 3\), got \(3, 4\)", ok_mean, np.zeros((3, 4)))
    refused(r"cov must have shape \(3, 3\), got \(2, 2\)", ok_mean, np.eye(2))
    refused(r"cov must have shape \(3, 3\), got \(9,\)", ok_mean, np.eye(3).ravel())
    c = np.eye(3)
    c[0, 2] = 1e-17
    refused(r"cov is not symmetric \(cov\[0, 2\]", ok_mean, c)
    refused("not positive definite", ok_mean, np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    refused("not positive definite", ok_mean, np.zeros((3, 3)))
    refused("not positive definite", ok_mean, -np.eye(3))
    refused(r"mean must have shape \(k,\), got \(3, 1\)", np.zeros((3, 1)), ok_cov)
    refused(r"mean must have shape \(k,\), got \(\)", 0.0, [[1.0]])
    refused(r"cov must have shape \(2, 2\)", np.zeros(2), ok_cov)
    refused("mean has 0 dimensions", np.zeros(0), np.zeros((0, 0)))
    refused(r"mean has 158 dimensions \(1 <= k <= 157\)", np.zeros(158), np.eye(158))
    refused("mean must be a", ["a", "b"], np.eye(2))
    refused("cov must be a", np.zeros(2), [["a", "b"], ["c", "d"]])


# ------------------------------------------------------------------------------------------------------------------
# the protocol
# ------------------------------------------------------------------------------------------------------------------
def test_rvs_bounds_dim_and_pickling():
    import pocomc_amd as pc
    prior, mean, cov, _ = case(5, 1e3)
    assert prior.dim == 5 and not hasattr(prior, "device_descriptor") and not hasattr(prior, "step_stage")
    assert callable(prior.logpdf_device) and callable(prior.logpdf)
    b = prior.bounds
    assert b.shape == (5, 2) and np.isneginf(b[:, 0]).all() and np.isposinf(b[:, 1]).all()
    np.random.seed(11)
    a = prior.rvs(7)
    np.random.seed(11)
    z = np.random.standard_normal((7, 5))
    assert a.shape == (7, 5) and a.dtype == np.float64 and np.array_equal(a, mean + z @ np.linalg.cholesky(cov).T)
    np.random.seed(11)
    assert np.array_equal(prior.rvs(7), a) and not np.array_equal(prior.rvs(7), a)
    assert prior.rvs().shape == (1, 5)
    big = prior.rvs(40000)
    np.testing.assert_allclose(big.mean(axis=0), mean, atol=0.05)
    np.testing.assert_allclose(np.cov(big.T), cov, atol=0.08)
    back = pickle.loads(pickle.dumps(prior))
    assert isinstance(back, pc.GaussianPrior) and back is not prior and back.dim == 5
    st, st2 = prior.__getstate__(), back.__getstate__()
    assert set(st) == {"mean", "cov", "L", "linv_packed", "logc"}
    for key in st:
        assert not hasattr(st[key], "device") or isinstance(st[key], np.ndarray), key      # plain arrays, no tensors
        assert np.array_equal(st[key], st2[key]), key
    for key, v in back.device_block().items():
        assert np.array_equal(v, prior.device_block()[key]), key
    np.random.seed(11)
    assert np.array_equal(back.rvs(7), a)                                 # (an unpickled copy draws from the global generator too)
    # the sources do not move the prior
    mean[0] += 1.0
    assert prior.mean[0] == back.mean[0]


def test_layout_blocks_takes_a_block_of_one_column():
    import pocomc_amd as pc
    one, three = pc.GaussianPrior([0.0], [[1.0]]), pc.GaussianPrior(np.zeros(3), np.eye(3))
    maps, rest_cols = pc.JointPrior.layout_blocks([[4], [1, 5, 0]], [one.dim, three.dim], 2)
    assert [m.tolist() for m in maps] == [[4], [1, 5, 0]] and rest_cols.tolist() == [2, 3]
    assert all(m.dtype == np.int32 for m in maps) and rest_cols.dtype == np.int32
    maps, rest_cols = pc.JointPrior.layout_blocks([[0], [1]], [1, 1], 0)
    assert [m.tolist() for m in maps] == [[0], [1]] and len(rest_cols) == 0
    with pytest.raises(ValueError, match="blocks 0 and 1 overlap"):
        pc.JointPrior.layout_blocks([[4], [1, 4, 0]], [1, 3], 2)


# ------------------------------------------------------------------------------------------------------------------
# the ABI and the entry's refusals: nothing is launched (there is no device here, every array address is a fake)
# ------------------------------------------------------------------------------------------------------------------
def test_the_abi_grew_by_one_entry_and_one_struct():
    import os
    from pocomc_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    hdr = open(os.path.join(root, "include", "pocomc_amd.h")).read()
    for text in ("#define PMC_ABI_VERSION 9", "#define PMC_GAUSS_BLOCKS_MAX 8", "} pmc_gauss_blocks_t;",
                 "int pmc_gauss_blocks_logpdf(const pmc_gauss_blocks_t* g, const double* x, int64_t row_stride, int64_t col_stride"):
        assert text in hdr, text
    assert lib.pmc_abi_version() == 9 and _lib.PMC_GAUSS_BLOCKS_MAX == 8 and hasattr(lib, "pmc_gauss_blocks_logpdf")
    G, J = _lib.pmc_gauss_blocks_t, _lib.pmc_joint_blocks_t
    # two int32, 8 int32, 3 x 8 pointers, 8 doubles, 2 pointers
    assert C.sizeof(G) == 2 * 4 + 8 * 4 + 3 * 8 * 8 + 8 * 8 + 2 * 8 == 312
    assert [getattr(G, f).offset for f in ("n_blocks", "D", "dim", "cols", "mean", "linv", "logc", "rest", "rest_cols")] == \
        [0, 4, 8, 40, 104, 168, 232, 296, 304]
    assert C.sizeof(J) == 152 and J.D.offset == 4 and J.scaler.offset == 8       # (its reserved word, named)


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


def test_the_entry_refuses_before_any_launch():
    from pocomc_amd import _lib
    lib = _lib.load()
    seen = set()

    def refused(word, change=None, null=False, x=0x6000, n=21, rs=9, cs=1, base=None, logp=0x7000, **kw):
        g, rest = descriptor(**kw)
        if change:
            change(g, rest)
        rc = lib.pmc_gauss_blocks_logpdf(None if null else C.byref(g), x, rs, cs, n, base, logp, None)
        msg = lib.pmc_last_error().decode()
        assert rc != 0 and msg.startswith("pmc_gauss_blocks_logpdf: ") and word in msg, (word, rc, msg)
        seen.add(msg)
    refused("bad descriptor", null=True)
    for nb in (0, -1, 9):
        refused("n_blocks must lie in 1 .. 8", lambda g, r: setattr(g, "n_blocks", nb))
    for field in ("cols", "mean", "linv"):
        refused("bad block descriptor", lambda g, r: getattr(g, field).__setitem__(1, None))
    refused("at least 1 column", dims=(3, 0))
    refused("at least 1 column", dims=(-2, 4))
    refused("n_dim too large (D <= 157)", dims=(3, 4), D=158)
    refused("more columns than x", dims=(3, 4), D=6)
    refused("more columns than x", dims=(3, 4), D=9, Dr=3)
    refused("rest and rest_cols go together", lambda g, r: setattr(g, "rest_cols", None), Dr=2)
    refused("rest and rest_cols go together", lambda g, r: setattr(g, "rest", None), Dr=2)
    for field in ("family", "loc", "scale"):
        refused("bad prior descriptor", lambda g, r: setattr(r, field, None), Dr=2)
    refused("bad prior descriptor", lambda g, r: setattr(r, "n_extended", -1), Dr=2)
    refused("parameter table", lambda g, r: setattr(r, "par", None), Dr=2)
    refused("base and rest exclude each other", Dr=2, base=0x8000)
    for kw in (dict(x=None), dict(logp=None), dict(n=-1), dict(rs=-1), dict(cs=-1)):
        refused("bad argument", **kw)
    refused("too many rows", n=64 * 2 ** 31)
    assert len(seen) == 12                                                # texts of their own
    # the widest descriptors pass the check: they are refused for their arguments
    refused("bad argument", dims=(157,), D=157, x=None)
    refused("bad argument", dims=(1,) * 8, D=157, Dr=149, x=None)
    # n == 0 returns 0 and reads nothing; a bad descriptor is refused at n == 0 as well
    g, rest = descriptor()
    assert lib.pmc_gauss_blocks_logpdf(C.byref(g), None, 9, 1, 0, None, None, None) == 0
    g.n_blocks = 0
    assert lib.pmc_gauss_blocks_logpdf(C.byref(g), None, 9, 1, 0, None, None, None) != 0
