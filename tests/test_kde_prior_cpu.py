"""``pocomc_amd.KDEPrior`` without a GPU: the constructor and its texts, the bandwidths against ``scipy.stats.gaussian_kde``, the
numpy statement of the kernel's arithmetic (``tests/kde_model.py``) against scipy and by quadrature, the rest of the prior
protocol, the draws, the ``JointPrior`` texts, and the entry's refusals, which come before any launch."""
import ctypes as C
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

import gauss_prior_model as gpm
import kde_model as km


# ------------------------------------------------------------------------------------------------------------------
# the constructor
# ------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    import pocomc_amd as pc
    K = pc.KDEPrior
    assert K.MAX_DIM == 16 and K.MAX_SAMPLES == 65536 and "KDEPrior" in pc.__all__
    s = km.banana(40, 3, 0)
    assert K(s).dim == 3 and K(s[:, :1]).dim == 1 and K(s, np.ones(40), "silverman").n_samples == 40
    assert K(np.zeros((65536, 1)) + np.arange(65536)[:, None]).n_samples == 65536

    def refused(text, *args, **kw):
        with pytest.raises(ValueError, match=text):
            K(*args, **kw)
    refused("samples must be an", [["a", "b"]])
    refused(r"samples must have shape \(M, k\) with M >= 1 and k >= 1, got \(40,\)", s[:, 0])
    refused(r"samples must have shape \(M, k\) with M >= 1 and k >= 1, got \(0, 3\)", np.zeros((0, 3)))
    refused(r"samples have 17 columns \(1 <= k <= 16\): choose fewer columns", np.zeros((40, 17)))
    refused(r"65537 samples of weight above zero \(1 <= M <= 65536\): thin the chain", np.zeros((65537, 1)))
    refused("weights must be an", s, ["a"] * 40)
    refused(r"weights must have shape \(40,\), got \(39,\)", s, np.ones(39))
    for bad in (-1.0, np.nan, np.inf):
        w = np.ones(40)
        w[7] = bad
        refused(r"weights\[7\] = .* is not finite and non-negative", s, w)
    refused("every weight is zero", s, np.zeros(40))
    bad = np.array(s)
    bad[5, 1] = np.nan
    refused(r"samples\[5, 1\] is not finite", bad)
    refused("bandwidth must be 'scott', 'silverman', a positive float or a", s, bandwidth="scot")
    refused("bandwidth must be 'scott', 'silverman', a positive float or a", s, bandwidth=None)
    for f in (0.0, -0.5, np.inf, np.nan):
        refused("the bandwidth factor must be finite and positive", s, bandwidth=f)
    refused(r"a matrix bandwidth must have shape \(3, 3\), got \(2, 2\)", s, bandwidth=np.eye(2))
    # too few distinct rows for a covariance: the text names the way out
    refused("not positive definite .too few distinct rows.: a matrix bandwidth=H takes an H from elsewhere", s[:1])
    refused("not positive definite .too few distinct rows.: a matrix bandwidth=H", s[:3])
    refused("not positive definite .too few distinct rows.: a matrix bandwidth=H", np.repeat(s[:1], 9, axis=0))
    assert K(s[:1], bandwidth=np.eye(3)).n_samples == 1
    # GaussianPrior's checks on (center, H), in its words behind the class's name
    H = np.eye(3)
    H[0, 2] = 1e-17
    refused(r"^KDEPrior: cov is not symmetric \(cov\[0, 2\]", s, bandwidth=H)
    refused(r"^KDEPrior: cov is not positive definite", s, bandwidth=-np.eye(3))
    H = np.eye(3)
    H[1, 1] = np.inf
    refused(r"^KDEPrior: cov\[1, 1\] is not finite", s, bandwidth=H)
    refused("too far apart for the bandwidth: a whitened sample is not finite", s * 1e150, bandwidth=np.eye(3) * 1e-320)


def test_zero_weight_rows_are_dropped_before_anything_else():
    import pocomc_amd as pc
    s = km.banana(30, 2, 1)
    w = np.linspace(0.0, 1.0, 30)
    w[[0, 4, 9]] = 0.0
    junk = np.array(s)
    junk[[0, 4, 9]] = np.nan                                              # what is dropped is not looked at
    a, b = pc.KDEPrior(junk, w), pc.KDEPrior(s[w > 0], w[w > 0])
    assert a.n_samples == 27 and np.array_equal(a.samples, s[w > 0]) and np.array_equal(a.weights, w[w > 0])
    for key, v in a.__getstate__().items():
        assert np.array_equal(v, b.__getstate__()[key]), key
    many = np.zeros((70000, 1))
    many[:, 0] = np.arange(70000)
    assert pc.KDEPrior(many, (np.arange(70000) < 65536).astype(float)).n_samples == 65536     # the limit counts what is kept


def test_weights_are_normalised_and_one_sample_has_logw_zero():
    import pocomc_amd as pc
    for weight in (1.0, 3.7, 1e-300, 1e300):
        one = pc.KDEPrior([[0.5, 1.0]], [weight], np.eye(2))
        assert one.logw.shape == (1,) and one.logw[0] == 0.0 and not np.signbit(one.logw[0])
        assert np.array_equal(one.center, [0.5, 1.0]) and np.array_equal(one.t, np.zeros((1, 2)))
    s = km.banana(4, 2, 2)
    prior = pc.KDEPrior(s, [1.0, 3.0, 2.0, 2.0], 0.5)
    assert np.array_equal(prior.logw, np.log(np.array([1.0, 3.0, 2.0, 2.0]) / 8.0))
    assert np.array_equal(prior.weights, [1.0, 3.0, 2.0, 2.0]) and prior.factor == 0.5


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", [1, 3, 5, 16])
def test_the_bandwidth_is_scipys(k, weighted):
    """The factor exactly, the covariance to 1e-14 (relative to its largest entry)."""
    import pocomc_amd as pc
    s = km.bimodal(300, k, k)
    w = km.log_weights(300, k, wmin=1e-3) if weighted else None
    for bw in ("scott", "silverman", 0.37):
        ref = km.scipy_kde(s, w, bw)
        prior = pc.KDEPrior(s, w, bw)
        assert prior.factor == ref.factor, (bw, prior.factor, ref.factor)
        assert np.array_equal(prior.H, prior.H.T)
        err = np.abs(prior.H - ref.covariance).max() / np.abs(ref.covariance).max()
        print(f"k={k} {bw}: covariance differs from scipy's by {err:.2e}")
        assert err <= 1e-14
        assert abs(1.0 / np.sum((prior.weights / prior.weights.sum()) ** 2) - ref.neff) <= 1e-12 * ref.neff
    H = gpm.random_cov(k, 30.0, np.random.default_rng(k))
    prior = pc.KDEPrior(s, w, H)
    assert prior.factor is None and np.array_equal(prior.H, H)


@pytest.mark.parametrize("k,M", [(1, 9), (3, 513), (16, 200)])
def test_device_block_is_the_issues_constants(k, M):
    import pocomc_amd as pc
    s, w = km.bimodal(M, k, 3), km.log_weights(M, 4, wmin=1e-6)
    prior = pc.KDEPrior(s, w, "silverman")
    blk = prior.device_block()
    assert set(blk) == {"center", "linv_packed", "t", "logw", "logc"} and all(v.dtype == np.float64 for v in blk.values())
    assert blk["center"].shape == (k,) and blk["linv_packed"].shape == (k * (k + 1) // 2,) and blk["t"].shape == (M, k)
    assert blk["logw"].shape == (M,) and blk["logc"].shape == ()
    wn = w / w.sum()
    assert np.array_equal(blk["logw"], np.log(wn))
    assert np.allclose(blk["center"], np.average(s, axis=0, weights=w), rtol=1e-14, atol=0)
    one = pc.GaussianPrior(prior.center, prior.H).device_block()
    assert np.array_equal(blk["linv_packed"], one["linv_packed"]) and float(blk["logc"]) == float(one["logc"])
    assert np.isclose(float(blk["logc"]), 0.5 * k * np.log(2 * np.pi) + 0.5 * np.linalg.slogdet(prior.H)[1], rtol=1e-13)
    Linv = np.zeros((k, k))
    Linv[np.tril_indices(k)] = blk["linv_packed"]
    assert np.array_equal(blk["t"], (s - prior.center) @ Linv.T)
    assert np.allclose(Linv @ prior.H @ Linv.T, np.eye(k), atol=1e-9)
    blk["t"][0, 0] = 99.0                                                 # a copy: the prior does not move
    assert prior.device_block()["t"][0, 0] != 99.0


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", [1, 3, 5, 16])
def test_the_model_matches_scipys_gaussian_kde(k, weighted):
    """A bimodal set centred near 70, rows at the samples' scale and ten times it, at ``1e-12 max(1, |v|)`` (3e-14 measured
    with scipy 1.15.3: the margin covers scipy's different summation)."""
    import pocomc_amd as pc
    M = 400
    s = km.bimodal(M, k, 10 + k)
    w = km.log_weights(M, k, wmin=1e-4) if weighted else None
    prior = pc.KDEPrior(s, w, "scott")
    ref = km.scipy_kde(s, w, "scott")
    rng = np.random.default_rng(k)
    x = np.concatenate([s[rng.integers(M, size=100)] + rng.normal(size=(100, k)) * 0.3,
                        70.0 + rng.normal(size=(100, k)) * 30.0])
    want = ref.logpdf(x.T)
    got = km.block_model(prior, x)
    assert got.shape == (200,) and np.isfinite(got).all() and np.isfinite(want).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"k={k} weighted={weighted}: model against scipy {err.max():.2e} relative, |v| up to {np.abs(want).max():.3g}")
    assert err.max() <= 1e-12
    # the slices of the kernel's sum stay far inside the tolerance of the sequential statement
    split = km.block_model(prior, x, chunks=8)
    assert (np.abs(split - got) <= 0.25 * km.tolerance(M, got, prior.logc)).all()


def test_the_model_is_normalised():
    import pocomc_amd as pc
    s = km.banana(60, 2, 5)
    w = km.log_weights(60, 6, wmin=1e-2)
    one = pc.KDEPrior(s[:, :1], w, "silverman")
    g = np.linspace(s[:, 0].min() - 12.0, s[:, 0].max() + 12.0, 40001)
    p = np.exp(km.block_model(one, g[:, None]))
    assert abs(np.sum(0.5 * (p[1:] + p[:-1]) * np.diff(g)) - 1.0) < 1e-9
    two = pc.KDEPrior(s, w, "scott")
    gx = np.linspace(s[:, 0].min() - 8.0, s[:, 0].max() + 8.0, 501)
    gy = np.linspace(s[:, 1].min() - 8.0, s[:, 1].max() + 8.0, 501)
    X, Y = np.meshgrid(gx, gy, indexing="ij")
    p = np.exp(km.block_model(two, np.stack([X.ravel(), Y.ravel()], axis=1))).reshape(501, 501)
    assert abs(p.sum() * (gx[1] - gx[0]) * (gy[1] - gy[0]) - 1.0) < 1e-6


@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_one_sample_is_the_gaussian_prior_bit_for_bit_in_the_model(k):
    import pocomc_amd as pc
    rng = np.random.default_rng(k)
    s0, H = rng.normal(size=k) * 3.0, gpm.random_cov(k, 100.0, rng) * 2.5
    prior = pc.KDEPrior(s0[None, :], None, H)
    plain = pc.GaussianPrior(s0, H).device_block()
    x = np.concatenate([gpm.draws(s0, H, 150, 1.0, rng), gpm.draws(s0, H, 50, 10.0, rng), s0[None, :]])
    want = gpm.gauss_block_model(x, plain["mean"], plain["linv_packed"], float(plain["logc"]))
    got = km.block_model(prior, x)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    base = rng.normal(size=len(x)) * 10.0
    assert np.array_equal(km.block_model(prior, x, base).view(np.int64), (base + want).view(np.int64))


def test_the_models_edges():
    import pocomc_amd as pc
    s = km.banana(9, 2, 7)
    prior = pc.KDEPrior(s, km.log_weights(9, 8), "scott")
    sd = np.sqrt(np.diag(prior.H))
    x = np.stack([s[3], s.max(axis=0) + 1e3 * sd, np.full(2, 1e160), [np.nan, 0.0], [0.0, np.inf], [-np.inf, 0.0]])
    v = km.block_model(prior, x)
    assert np.isfinite(v[:2]).all() and v[1] < -1e4 and np.isneginf(v[2:]).all()
    with np.errstate(all="ignore"):
        blk = prior.device_block()
        naive = np.log(np.exp(km.kde_e_model(x[1:2], blk["center"], blk["linv_packed"], blk["t"], blk["logw"])).sum())
    assert np.isneginf(naive)                                             # (what the maximum is taken out for)


# ------------------------------------------------------------------------------------------------------------------
# the protocol
# ------------------------------------------------------------------------------------------------------------------
def test_the_protocol_and_pickling():
    import pocomc_amd as pc
    s, w = km.banana(50, 4, 9), km.log_weights(50, 9, wmin=0.01)
    prior = pc.KDEPrior(s, w)
    assert prior.dim == 4 and prior.n_samples == 50
    assert not hasattr(prior, "device_descriptor") and not hasattr(prior, "step_stage")
    assert callable(prior.logpdf_device) and callable(prior.logpdf)
    b = prior.bounds
    assert b.shape == (4, 2) and np.isneginf(b[:, 0]).all() and np.isposinf(b[:, 1]).all()
    back = pickle.loads(pickle.dumps(prior))
    assert type(back) is pc.KDEPrior and back is not prior and back.dim == 4 and back._dev is None
    st, st2 = prior.__getstate__(), back.__getstate__()
    assert set(st) == {"samples", "weights", "H", "center", "L", "linv_packed", "t", "logw", "logc", "factor"}
    for key in st:
        assert np.array_equal(st[key], st2[key]), key
    np.random.seed(11)
    a = prior.rvs(9)
    np.random.seed(11)
    assert np.array_equal(back.rvs(9), a)
    s[0, 0] += 1.0                                                        # the sources do not move the prior
    assert prior.samples[0, 0] == back.samples[0, 0] != s[0, 0]


def test_rvs_draws_the_estimate():
    import pocomc_amd as pc
    s, w = km.banana(200, 3, 12), km.log_weights(200, 12, wmin=1e-2)
    prior = pc.KDEPrior(s, w, "silverman")
    np.random.seed(3)
    r = prior.rvs(40000)
    assert r.shape == (40000, 3) and np.isfinite(r).all() and prior.rvs(1).shape == (1, 3)
    # the two draws, in the documented order, from numpy's global generator
    np.random.seed(3)
    idx = np.random.choice(200, size=40000, p=w / w.sum())
    z = np.random.standard_normal((40000, 3))
    assert np.array_equal(r, s[idx] + z @ prior.L.T)
    # the estimate's first two moments are center and C + H, C the samples' weighted covariance (not divided by 1 - sum w^2)
    wn = w / w.sum()
    C_ = ((s - prior.center).T * wn) @ (s - prior.center)
    V = C_ + prior.H
    se_mean = np.sqrt(np.diag(V) / 40000)
    assert (np.abs(r.mean(axis=0) - prior.center) <= 5 * se_mean).all()
    d = r - prior.center
    prod = d[:, :, None] * d[:, None, :]
    se_cov = prod.std(axis=0) / np.sqrt(40000)
    assert (np.abs(prod.mean(axis=0) - V) <= 5 * se_cov).all()


def test_from_samples_selects_columns_and_from_sampler_needs_a_finished_run():
    import pocomc_amd as pc
    x = km.banana(80, 5, 13)
    w = km.log_weights(80, 13, wmin=0.1)
    a, b = pc.KDEPrior.from_samples(x, w, columns=[4, 0, 2], bandwidth="silverman"), pc.KDEPrior(x[:, [4, 0, 2]], w, "silverman")
    for key, v in a.__getstate__().items():
        assert np.array_equal(v, b.__getstate__()[key]), key
    assert pc.KDEPrior.from_samples(x).dim == 5
    with pytest.raises(ValueError, match="columns are not distinct"):
        pc.KDEPrior.from_samples(x, columns=[1, 1])
    with pytest.raises(ValueError, match=r"columns must lie in \[0, 5\)"):
        pc.KDEPrior.from_samples(x, columns=[1, 5])
    with pytest.raises(ValueError, match=r"x must have shape \(n, d\)"):
        pc.KDEPrior.from_samples(x[:, 0])

    class Unfinished:
        walkers = {"beta": 0.5}
    with pytest.raises(ValueError, match="has not run to beta = 1"):
        pc.KDEPrior.from_sampler(Unfinished(), columns=[0, 1])


def test_the_constructor_imports_no_torch():
    code = ("import sys, numpy as np, pocomc_amd as pc\n"
            "p = pc.KDEPrior(np.random.default_rng(0).normal(size=(50, 3)), None, 'scott')\n"
            "p.device_block(); p.rvs(3); p.bounds; p.__getstate__()\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


# ------------------------------------------------------------------------------------------------------------------
# JointPrior: what needs no device
# ------------------------------------------------------------------------------------------------------------------
def test_joint_prior_texts_with_kde_blocks():
    import pocomc_amd as pc
    kde = pc.KDEPrior(km.banana(30, 3, 1))
    # the texts the constructor had, to the letter; the new kind behind them, or only where a KDE block is there
    with pytest.raises(ValueError, match="block 1 must be a pocomc_amd.FlowPrior or GaussianPrior or GaussianMixturePrior, got "
                                         r"object \(a KDEPrior is taken as well\)"):
        pc.JointPrior([kde, object()], [[0, 1, 2], [3]])
    one = pc.KDEPrior(np.arange(5.0)[:, None])
    with pytest.raises(ValueError, match=r"9 blocks \(0 flow blocks, 0 Gaussian blocks, 9 KDE blocks; 1 <= blocks <= 8\)"):
        pc.JointPrior([one] * 9, [[j] for j in range(9)])
    mix = pc.GaussianMixturePrior([1.0], [[0.0]], [[[1.0]]])
    with pytest.raises(ValueError, match=r"9 blocks \(0 flow blocks, 1 Gaussian blocks, 3 mixture blocks, 5 KDE blocks; "
                                         r"1 <= blocks <= 8\)"):
        pc.JointPrior([one] * 5 + [mix] * 3 + [pc.GaussianPrior([0.0], [[1.0]])], [[j] for j in range(9)])
    with pytest.raises(ValueError, match=r"9 blocks \(0 flow blocks, 0 Gaussian blocks, 9 mixture blocks; 1 <= blocks <= 8\)"):
        pc.JointPrior([mix] * 9, [[j] for j in range(9)])
    # the layout is the blocks form's: a KDE block's columns in any order, the rest in increasing order
    maps, rest = pc.JointPrior.layout_blocks([[4, 0, 2]], [kde.dim], 3)
    assert maps[0].tolist() == [4, 0, 2] and rest.tolist() == [1, 3, 5]
    assert pc.JointPrior.kde_priors == ()
    # step_stage and step_prior refuse a prior with a KDE block, each in words of its own
    stub = types.SimpleNamespace(kde_priors=(kde,), mixture_priors=(), gaussian_priors=(), blocks=1)
    with pytest.raises(ValueError, match="JointPrior.step_stage: a prior with a KDE block is not evaluated inside the step"):
        pc.JointPrior.step_stage(stub, 64)

    class WithKde:
        kde_priors = (kde,)
        dim = 3
        bounds = kde.bounds

        def step_stage(self, n, device=None):
            raise AssertionError("not reached")

        def logpdf(self, x):
            return kde.logpdf(x)

        def rvs(self, size=1):
            return kde.rvs(size)
    with pytest.raises(ValueError, match="step_prior=True does not take a JointPrior with a KDE block"):
        pc.Sampler(prior=WithKde(), likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)


# ------------------------------------------------------------------------------------------------------------------
# the ABI and the entry's refusals: nothing is launched (there is no device here, every array address is a fake)
# ------------------------------------------------------------------------------------------------------------------
def descriptor(n_samples=9, dim=4, D=9, Dr=0):
    from pocomc_amd import _lib
    g = _lib.pmc_kde_t(n_samples=n_samples, dim=dim, D=D, cols=0x1000, center=0x2000, linv=0x3000, t=0x4000, logw=0x5000,
                       logc=1.5)
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
    for text in ("#define PMC_ABI_VERSION 9", "#define PMC_KDE_MAX_DIM 16", "#define PMC_KDE_MAX_SAMPLES 65536", "} pmc_kde_t;",
                 "int pmc_kde_logpdf(const pmc_kde_t* g, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,"):
        assert text in hdr, text
    assert lib.pmc_abi_version() == 9 and hasattr(lib, "pmc_kde_logpdf")
    assert _lib.PMC_KDE_MAX_DIM == 16 and _lib.PMC_KDE_MAX_SAMPLES == 65536
    G = _lib.pmc_kde_t
    assert C.sizeof(G) == 4 * 4 + 8 * 8 == 80
    assert [getattr(G, f).offset for f in ("n_samples", "dim", "D", "reserved", "cols", "center", "linv", "t", "logw", "logc",
                                           "rest", "rest_cols")] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72]
    assert C.sizeof(_lib.pmc_gauss_mix_t) == 72 and C.sizeof(_lib.pmc_gauss_blocks_t) == 312      # (nothing before it moved)


def test_the_entry_refuses_before_any_launch():
    from pocomc_amd import _lib
    lib = _lib.load()
    seen = set()

    def refused(word, change=None, null=False, x=0x7000, n=21, rs=9, cs=1, base=None, logp=0x8000, **kw):
        g, rest = descriptor(**kw)
        if change:
            change(g, rest)
        rc = lib.pmc_kde_logpdf(None if null else C.byref(g), x, rs, cs, n, base, logp, None)
        msg = lib.pmc_last_error().decode()
        assert rc != 0 and msg.startswith("pmc_kde_logpdf: ") and word in msg, (word, rc, msg)
        seen.add(msg)
    refused("bad descriptor", null=True)
    for field in ("cols", "center", "linv", "t", "logw"):
        refused("bad KDE descriptor (a NULL array)", lambda g, r: setattr(g, field, None))
    for M in (0, -1, 65537):
        refused("n_samples must lie in 1 .. 65536", n_samples=M)
    for k in (0, -2, 17):
        refused("dim must lie in 1 .. 16", dim=k, D=100)
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
    refused("a NULL x or logp", n_samples=65536, dim=16, D=157, Dr=141, x=None)
    # n == 0 returns 0 and reads nothing; a bad descriptor is refused at n == 0 as well
    g, rest = descriptor()
    assert lib.pmc_kde_logpdf(C.byref(g), None, 9, 1, 0, None, None, None) == 0
    g.n_samples = 0
    assert lib.pmc_kde_logpdf(C.byref(g), None, 9, 1, 0, None, None, None) != 0
