"""``pocomc_amd.GaussianMixturePrior`` without a GPU: the constructor and its texts, the host-side constants, the rest of the
prior protocol, the numpy statement of the kernel's arithmetic (``tests/gauss_mix_model.py``) against scipy, the draws, the EM
fit, and the entry's refusals, which come before any launch."""
import ctypes as C
import pickle

import numpy as np
import pytest

import gauss_mix_model as gmm
import gauss_prior_model as gpm


def mixture(Cn, k, seed=0, **kw):
    import pocomc_amd as pc
    w, m, c = gmm.random_mixture(Cn, k, seed, **kw)
    return pc.GaussianMixturePrior(w, m, c), w, m, c


# ------------------------------------------------------------------------------------------------------------------
# the constructor
# ------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    import pocomc_amd as pc
    G = pc.GaussianMixturePrior
    assert G.MAX_COMPONENTS == 32 and G.MAX_DIM == 64 and "GaussianMixturePrior" in pc.__all__
    w, m, c = np.array([1.0, 3.0]), np.zeros((2, 3)), np.stack([np.eye(3)] * 2)
    assert G(w, m, c).dim == 3 and G([2.0], [[0.5]], [[[2.0]]]).dim == 1
    assert G(np.ones(32), np.zeros((32, 64)), np.stack([np.eye(64)] * 32)).components == 32

    def refused(text, *args):
        with pytest.raises(ValueError, match=text):
            G(*args)
    refused(r"weights must have shape \(C,\) with C >= 1, got \(2, 1\)", w[:, None], m, c)
    refused(r"weights must have shape \(C,\) with C >= 1, got \(0,\)", [], np.zeros((0, 3)), np.zeros((0, 3, 3)))
    refused(r"33 components \(1 <= C <= 32\)", np.ones(33), np.zeros((33, 2)), np.stack([np.eye(2)] * 33))
    refused(r"means must have shape \(2, k\) with k >= 1, got \(3, 3\)", w, np.zeros((3, 3)), c)
    refused(r"means must have shape \(2, k\) with k >= 1, got \(3,\)", w, np.zeros(3), c)
    refused(r"means have 65 dimensions \(1 <= k <= 64\)", w, np.zeros((2, 65)), np.stack([np.eye(65)] * 2))
    refused(r"covs must have shape \(2, 3, 3\), got \(3, 3\)", w, m, np.eye(3))
    refused(r"covs must have shape \(2, 3, 3\), got \(2, 3, 4\)", w, m, np.zeros((2, 3, 4)))
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(r"weights\[1\] = .* is not finite and strictly positive", [1.0, bad], m, c)
    refused("weights must be a", ["a", "b"], m, c)
    refused("means must be a", w, [["a"] * 3] * 2, c)
    refused("covs must be a", w, m, "no")
    # GaussianPrior's checks on every component, in its words behind the component's number
    bad = np.array(m)
    bad[1, 2] = np.nan
    refused(r"^GaussianMixturePrior: component 1: mean\[2\] is not finite", w, bad, c)
    cc = np.array(c)
    cc[0, 0, 2] = 1e-17
    refused(r"^GaussianMixturePrior: component 0: cov is not symmetric \(cov\[0, 2\]", w, m, cc)
    cc = np.array(c)
    cc[1] = -np.eye(3)
    refused(r"^GaussianMixturePrior: component 1: cov is not positive definite", w, m, cc)
    cc = np.array(c)
    cc[1, 1, 1] = np.inf
    refused(r"^GaussianMixturePrior: component 1: cov\[1, 1\] is not finite", w, m, cc)


def test_weights_are_normalised_and_one_component_has_logw_zero():
    import pocomc_amd as pc
    for weight in (1.0, 3.7, 1e-300, 1e300):
        one = pc.GaussianMixturePrior([weight], [[0.0, 1.0]], [np.eye(2)])
        assert one.logw.shape == (1,) and one.logw[0] == 0.0 and not np.signbit(one.logw[0])
    prior = pc.GaussianMixturePrior([1.0, 3.0], np.zeros((2, 2)), np.stack([np.eye(2)] * 2))
    assert np.array_equal(prior.logw, np.log(np.array([1.0, 3.0]) / 4.0)) and np.array_equal(prior.weights, [1.0, 3.0])


@pytest.mark.parametrize("Cn,k", [(1, 1), (2, 5), (7, 33), (32, 64)])
def test_device_block_is_every_components_gaussian_block(Cn, k):
    import pocomc_amd as pc
    prior, w, m, c = mixture(Cn, k, seed=Cn + k)
    blk = prior.device_block()
    assert set(blk) == {"logw", "mean", "linv_packed", "logc"}
    assert blk["logw"].shape == (Cn,) and blk["mean"].shape == (Cn, k) and blk["logc"].shape == (Cn,)
    assert blk["linv_packed"].shape == (Cn, k * (k + 1) // 2) and all(v.dtype == np.float64 for v in blk.values())
    assert np.array_equal(blk["logw"], np.log(w / w.sum()))
    for j in range(Cn):
        one = pc.GaussianPrior(m[j], c[j]).device_block()
        assert np.array_equal(blk["mean"][j], one["mean"]) and np.array_equal(blk["linv_packed"][j], one["linv_packed"])
        assert blk["logc"][j] == float(one["logc"])
    blk["mean"][0, 0] = 99.0                                              # a copy: the prior does not move
    assert prior.device_block()["mean"][0, 0] == m[0, 0]


def test_the_protocol_and_pickling():
    import pocomc_amd as pc
    prior, w, m, c = mixture(3, 4, seed=5, wmin=0.05)
    assert prior.dim == 4 and prior.components == 3
    assert not hasattr(prior, "device_descriptor") and not hasattr(prior, "step_stage")
    assert callable(prior.logpdf_device) and callable(prior.logpdf) and prior.fit_info is None
    b = prior.bounds
    assert b.shape == (4, 2) and np.isneginf(b[:, 0]).all() and np.isposinf(b[:, 1]).all()
    back = pickle.loads(pickle.dumps(prior))
    assert type(back) is pc.GaussianMixturePrior and back is not prior and back.dim == 4 and back._dev is None
    st, st2 = prior.__getstate__(), back.__getstate__()
    assert set(st) == {"weights", "means", "covs", "logw", "L", "linv_packed", "logc", "fit_info"}
    for key in st:
        if key != "fit_info":
            assert isinstance(st[key], np.ndarray) and np.array_equal(st[key], st2[key]), key
    np.random.seed(11)
    a = prior.rvs(9)
    np.random.seed(11)
    assert np.array_equal(back.rvs(9), a)
    m[0, 0] += 1.0                                                        # the sources do not move the prior
    assert prior.means[0, 0] == back.means[0, 0] != m[0, 0]
    # a JointPrior's constructor refuses other block types in the words it had, the new class behind them
    with pytest.raises(ValueError, match="block 1 must be a pocomc_amd.FlowPrior or GaussianPrior or GaussianMixturePrior, got"):
        pc.JointPrior([prior, object()], [[0, 1, 2, 3], [4]])
    with pytest.raises(ValueError, match=r"9 blocks \(0 flow blocks, 0 Gaussian blocks, 9 mixture blocks; 1 <= blocks <= 8\)"):
        pc.JointPrior([pc.GaussianMixturePrior([1.0], [[0.0]], [[[1.0]]])] * 9, [[j] for j in range(9)])


# ------------------------------------------------------------------------------------------------------------------
# the model against scipy
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", [1.0, 1e3])
@pytest.mark.parametrize("Cn,k", [(1, 1), (2, 2), (2, 5), (7, 33), (32, 64)])
def test_the_model_matches_scipy(Cn, k, cond):
    """200 rows at 1x and 200 at 10x the components' widths, against ``logsumexp_c(log w_c + multivariate_normal.logpdf)``.
    The bound is the one ``tests/test_gauss_prior_cpu.py`` holds the one-component model to, ``8 k cond 2^-53 max(1, |scipy|)``,
    at its condition numbers: a mixture's value is a log-sum-exp of such values, which moves by no more than its largest
    term does."""
    prior, w, m, c = mixture(Cn, k, seed=100 * Cn + k, cond=cond, spread=3.0, wmin=1e-6)
    rng = np.random.default_rng(k)
    worst = 0.0
    for width in (1.0, 10.0):
        x = gmm.mixture_draws(w, m, c, 200, width, rng)
        want = gmm.scipy_logpdf(x, w, m, c)
        got = gmm.block_model(prior, x)
        assert got.shape == (200,) and np.isfinite(got).all()
        scale = np.maximum(1.0, np.abs(want))
        worst = max(worst, float((np.abs(got - want) / scale).max()))
        assert (np.abs(got - want) <= 8 * k * cond * 2.0 ** -53 * scale).all(), (Cn, k, cond, width, worst)
    print(f"C={Cn} k={k} cond={cond:g}: model against scipy, max relative difference {worst:.3e} "
          f"(bound {8 * k * cond * 2.0 ** -53:.3e})")


def test_the_model_at_its_edges():
    prior, w, m, c = mixture(3, 4, seed=2, spread=2.0, wmin=1e-3)
    rng = np.random.default_rng(0)
    x = gmm.mixture_draws(w, m, c, 12, 1.0, rng)
    good = gmm.block_model(prior, x)
    x[1, 0], x[3, 3], x[5, 2] = np.nan, np.inf, -np.inf
    x[7] = 1e200
    x[8] = 1e300 * np.array([1, -1, 1, -1])
    far = m[0] + 1e3 * np.sqrt(np.diag(c[0]))                             # 1e3 widths away: a naive log(sum(exp)) is -inf
    x[9] = far
    got = gmm.block_model(prior, x)
    bad = [1, 3, 5, 7, 8]
    keep = np.setdiff1d(np.arange(12), bad + [9])
    assert np.isneginf(got[bad]).all() and not np.isnan(got).any() and np.array_equal(got[keep], good[keep])
    assert np.isfinite(got[9]) and got[9] < -1e4
    with np.errstate(all="ignore"):
        naive = np.log(np.exp(gmm.mix_t_model(x[9:10], *[prior.device_block()[f] for f in ("logw", "mean", "linv_packed", "logc")])).sum())
    assert np.isneginf(naive)
    assert abs(got[9] - gmm.scipy_logpdf(x[9:10], w, m, c)[0]) <= 1e-9 * abs(got[9])
    # one component with logw = 0.0 is the Gaussian model, bit for bit
    one, w1, m1, c1 = mixture(1, 5, seed=4)
    y = gmm.mixture_draws(w1, m1, c1, 50, 3.0, rng)
    blk = one.device_block()
    assert np.array_equal(gmm.block_model(one, y), gpm.gauss_block_model(y, blk["mean"][0], blk["linv_packed"][0], blk["logc"][0]))
    # on top of a start: one float64 addition, -inf stays -inf
    start = rng.normal(size=12)
    start[0] = -np.inf
    on = gmm.block_model(prior, x, start)
    assert np.array_equal(on[keep[1:]], (start + got)[keep[1:]]) and np.isneginf(on[[0] + bad]).all()


# ------------------------------------------------------------------------------------------------------------------
# draws
# ------------------------------------------------------------------------------------------------------------------
def test_rvs_draws_the_components_by_their_weights_then_one_block_of_normals():
    import pocomc_amd as pc
    weights = np.array([0.2, 0.5, 0.3])
    means = np.array([[-20.0, 0.0], [0.0, 20.0], [20.0, 0.0]])            # far apart: a row shows its component
    covs = np.stack([gpm.random_cov(2, 10.0, np.random.default_rng(s)) for s in range(3)])
    prior = pc.GaussianMixturePrior(weights * 4.0, means, covs)
    n = 40000
    np.random.seed(5)
    x = prior.rvs(n)
    assert x.shape == (n, 2) and x.dtype == np.float64 and prior.rvs().shape == (1, 2)
    # the stated order of the two draws, from the global generator
    np.random.seed(5)
    comp = np.random.choice(3, size=n, p=np.exp(prior.logw))
    z = np.random.standard_normal((n, 2))
    L = np.linalg.cholesky(covs)
    assert np.array_equal(x, means[comp] + np.einsum("rj,rij->ri", z, L[comp]))
    np.random.seed(5)
    assert np.array_equal(prior.rvs(n), x) and not np.array_equal(prior.rvs(n), x)
    nearest = np.argmin(((x[:, None, :] - means[None]) ** 2).sum(axis=2), axis=1)
    assert np.array_equal(nearest, comp)
    for j in range(3):
        nj = int((comp == j).sum())
        assert abs(nj / n - weights[j]) <= 5.0 * np.sqrt(weights[j] * (1.0 - weights[j]) / n), j
        se = np.sqrt(np.diag(covs[j]) / nj)
        assert (np.abs(x[comp == j].mean(axis=0) - means[j]) <= 5.0 * se).all(), j


# ------------------------------------------------------------------------------------------------------------------
# the EM fit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_from_samples_fits_the_two_component_case(weighted):
    """Two components in 3-D, 4000 rows, uniform weights and gamma(0.5) weights.  The conditions are the issue's: the same
    bits twice and an untouched global generator; no step of the weighted mean log-density falls by more than 1e-10; the
    final one is not below the generating mixture's on the same rows (a maximum-likelihood fit cannot be); the sorted weights
    are within 0.04 of (0.3, 0.7), a sampling-noise condition."""
    import pocomc_amd as pc
    x, w_true, m_true, c_true = gmm.em_case()
    sw = np.random.default_rng(8).gamma(0.5, size=len(x)) if weighted else None
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    prior = pc.GaussianMixturePrior.from_samples(x, sw, n_components=2)
    again = pc.GaussianMixturePrior.from_samples(x, sw, n_components=2)
    assert np.array_equal(np.random.get_state()[1], before)
    for key in ("weights", "means", "covs", "logw", "linv_packed", "logc"):
        assert np.array_equal(getattr(prior, key), getattr(again, key)), key
    info = prior.fit_info
    assert set(info) == {"iterations", "converged", "loglik"} and info["converged"] and info["iterations"] == len(info["loglik"])
    assert np.array_equal(info["loglik"], again.fit_info["loglik"]) and 2 <= info["iterations"] <= 500
    steps = np.diff(info["loglik"])
    print(f"weighted={weighted}: {info['iterations']} E-steps, smallest step {steps.min():.3e}")
    assert (steps >= -1e-10).all(), steps.min()
    wn = np.full(len(x), 1.0 / len(x)) if sw is None else sw / sw.sum()
    fitted = float(wn @ gmm.scipy_logpdf(x, prior.weights, prior.means, prior.covs))
    truth = float(wn @ gmm.scipy_logpdf(x, w_true, m_true, c_true))
    print(f"weighted={weighted}: weighted mean log-density {fitted:.6f} (fit) against {truth:.6f} (generating mixture)")
    assert abs(fitted - info["loglik"][-1]) <= 1e-12 * abs(fitted)
    assert fitted >= truth
    got = np.sort(np.exp(prior.logw))
    print(f"weighted={weighted}: fitted weights {got}")
    assert (np.abs(got - [0.3, 0.7]) <= 0.04).all()
    back = pickle.loads(pickle.dumps(prior))
    assert back.fit_info["iterations"] == info["iterations"] and np.array_equal(back.fit_info["loglik"], info["loglik"])
    other = pc.GaussianMixturePrior.from_samples(x, sw, n_components=2, seed=1)
    assert other.fit_info["converged"]


def test_from_samples_refusals():
    import pocomc_amd as pc
    F = pc.GaussianMixturePrior.from_samples
    rng = np.random.default_rng(0)
    x = rng.normal(size=(12, 2))
    with pytest.raises(ValueError, match=r"component \d+ has collapsed.*use fewer components"):
        F(x, n_components=8)
    with pytest.raises(ValueError, match=r"x must have shape \(n, k\)"):
        F(np.zeros(5))
    with pytest.raises(ValueError, match=r"x\[3, 1\] is not finite"):
        y = np.array(x)
        y[3, 1] = np.nan
        F(y)
    with pytest.raises(ValueError, match=r"weights must have shape \(12,\)"):
        F(x, np.ones(5))
    with pytest.raises(ValueError, match="weights must be finite, not negative and not all zero"):
        F(x, -np.ones(12))
    with pytest.raises(ValueError, match=r"n_components = 33 \(1 <= C <= 32\)"):
        F(x, n_components=33)
    with pytest.raises(ValueError, match=r"x has 65 columns"):
        F(np.zeros((100, 65)))
    one = F(rng.normal(size=(200, 3)), n_components=1)                    # one component: the weighted moments
    assert one.components == 1 and one.logw[0] == 0.0 and one.fit_info["converged"]

    class Unfinished:
        walkers = {"beta": 0.5}
    with pytest.raises(ValueError, match="has not run to beta = 1"):
        pc.GaussianMixturePrior.from_sampler(Unfinished(), columns=[0, 1])


# ------------------------------------------------------------------------------------------------------------------
# the ABI and the entry's refusals: nothing is launched (there is no device here, every array address is a fake)
# ------------------------------------------------------------------------------------------------------------------
def descriptor(n_comp=3, dim=4, D=9, Dr=0):
    from pocomc_amd import _lib
    g = _lib.pmc_gauss_mix_t(n_comp=n_comp, dim=dim, D=D, cols=0x1000, logw=0x2000, mean=0x3000, linv=0x4000, logc=0x5000)
    rest = _lib.pmc_prior_t(family=0x70, loc=0x80, scale=0x90, D=max(Dr, 1), par=0xA0, n_extended=1)
    if Dr:
        g.rest, g.rest_cols = C.addressof(rest), 0x6000
    return g, rest


def test_the_abi_grew_by_one_entry_and_one_struct():
    import os
    from pocomc_amd import _lib
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    hdr = open(os.path.join(root, "include", "pocomc_amd.h")).read()
    for text in ("#define PMC_ABI_VERSION 9", "#define PMC_GAUSS_MIX_MAX_COMPONENTS 32", "#define PMC_GAUSS_MIX_MAX_DIM 64",
                 "} pmc_gauss_mix_t;", "int pmc_gauss_mix_logpdf(const pmc_gauss_mix_t* g, const double* x, int64_t row_stride, "
                 "int64_t col_stride, int64_t n,"):
        assert text in hdr, text
    assert lib.pmc_abi_version() == 9 and hasattr(lib, "pmc_gauss_mix_logpdf")
    assert _lib.PMC_GAUSS_MIX_MAX_COMPONENTS == 32 and _lib.PMC_GAUSS_MIX_MAX_DIM == 64
    G = _lib.pmc_gauss_mix_t
    assert C.sizeof(G) == 4 * 4 + 7 * 8 == 72
    assert [getattr(G, f).offset for f in ("n_comp", "dim", "D", "reserved", "cols", "logw", "mean", "linv", "logc", "rest",
                                           "rest_cols")] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert C.sizeof(_lib.pmc_gauss_blocks_t) == 312                       # (the entries before it have not moved)


def test_the_entry_refuses_before_any_launch():
    from pocomc_amd import _lib
    lib = _lib.load()
    seen = set()

    def refused(word, change=None, null=False, x=0x7000, n=21, rs=9, cs=1, base=None, logp=0x8000, **kw):
        g, rest = descriptor(**kw)
        if change:
            change(g, rest)
        rc = lib.pmc_gauss_mix_logpdf(None if null else C.byref(g), x, rs, cs, n, base, logp, None)
        msg = lib.pmc_last_error().decode()
        assert rc != 0 and msg.startswith("pmc_gauss_mix_logpdf: ") and word in msg, (word, rc, msg)
        seen.add(msg)
    refused("bad descriptor", null=True)
    for field in ("cols", "logw", "mean", "linv", "logc"):
        refused("a NULL array", lambda g, r: setattr(g, field, None))
    for nc in (0, -1, 33):
        refused("n_comp must lie in 1 .. 32", n_comp=nc)
    for k in (0, -2, 65):
        refused("dim must lie in 1 .. 64", dim=k, D=100)
    refused("n_dim too large (D <= 157)", D=158)
    refused("more columns than x", dim=4, D=3)
    refused("more columns than x", dim=4, D=9, Dr=6)
    refused("rest and rest_cols go together", lambda g, r: setattr(g, "rest_cols", None), Dr=2)
    refused("rest and rest_cols go together", lambda g, r: setattr(g, "rest", None), Dr=2)
    for field in ("family", "loc", "scale"):
        refused("bad prior descriptor", lambda g, r: setattr(r, field, None), Dr=2)
    refused("parameter table", lambda g, r: setattr(r, "par", None), Dr=2)
    refused("base and rest exclude each other", Dr=2, base=0x9000)
    refused("a NULL x or logp", x=None)
    refused("a NULL x or logp", logp=None)
    for kw in (dict(n=-1), dict(rs=-1), dict(cs=-1)):
        refused("a negative count or stride", **kw)
    refused("too many rows", n=64 * 2 ** 31)
    assert len(seen) == 13                                                # texts of their own
    # the widest descriptor passes the check: it is refused for its arguments
    refused("a NULL x or logp", n_comp=32, dim=64, D=157, Dr=93, x=None)
    # n == 0 returns 0 and reads nothing; a bad descriptor is refused at n == 0 as well
    g, rest = descriptor()
    assert lib.pmc_gauss_mix_logpdf(C.byref(g), None, 9, 1, 0, None, None, None) == 0
    g.n_comp = 0
    assert lib.pmc_gauss_mix_logpdf(C.byref(g), None, 9, 1, 0, None, None, None) != 0
