"""``pocomc_amd.KDEPrior`` and the KDE blocks of ``pocomc_amd.JointPrior`` on the device: one launch of ``pmc_kde_logpdf``
(``csrc/kde_prior.hip``) per estimate.

With one sample the statement is bit for bit against ``GaussianPrior`` (``pmc_gauss_blocks_logpdf``).  With more the yardstick
is ``tests/kde_model.py``, the statement of a row in numpy with a sequential sum, to ``kde_model.tolerance``:
``(M + 8) 2^-52 + 2^-50 (|v| + |logc|)``, derived there and not measured.  Among themselves the layouts, the row counts and the
rows' places give the same bits.  The sample counts are the edges of the kernel's eight-way slicing (2, 7, 8, 9), of a 64-wide
chunk (63, 65), several hundred kernels a slice (513, 4099) and the limit (65536, once); the row counts one row, one short of
a 64-row tile, a tile, one more, several tiles."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import gauss_prior_model as gpm
import joint_prior_model as jpm
import kde_model as km
from .test_gpu_flow_prior import bits, bounds_of, gauss_at, make as make_flow, rows_in
from .test_gpu_gauss_prior import layouts, up
from .test_gpu_joint_prior import table_logp

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 200]
_made = {}


def make(k, M, weighted, seed=None):
    """``(prior, 200 rows, the model's values of them, the special rows' indices)``, built once per case.  The rows: around the
    samples at a third of their scatter, and across ten times it; row 5 exactly on a sample, row 6 1e3 bandwidths beyond every
    sample in every column."""
    import pocomc_amd as pc
    key = (k, M, weighted)
    if key not in _made:
        seed = 100 * k + M if seed is None else seed
        s = km.banana(M, k, seed)
        w = km.log_weights(M, seed + 1) if weighted else None             # from 1 down to 1e-12
        H = None
        if M <= k + 1:                                                    # too few rows for a covariance: an H from elsewhere
            H = gpm.random_cov(k, 20.0, np.random.default_rng(seed)) * 0.3
        prior = pc.KDEPrior(s, w, "scott" if H is None else H)
        rng = np.random.default_rng(seed + 2)
        x = np.concatenate([s[rng.integers(M, size=150)] + rng.normal(size=(150, k)) * 0.3 * s.std(axis=0).clip(0.1),
                            s.mean(axis=0) + rng.normal(size=(50, k)) * 10.0 * s.std(axis=0).clip(0.1)])
        x[5] = s[M // 2]
        x[6] = s.max(axis=0) + 1e3 * np.sqrt(np.diag(prior.H))
        want = km.block_model(prior, x)
        assert np.isfinite(want).all() and want[6] < -1e4
        want.setflags(write=False)
        x.setflags(write=False)
        _made[key] = (prior, x, want)
    return _made[key]


def close(got, want, prior, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    tol = km.tolerance(prior.n_samples, want[fin], prior.logc)
    print(f"{what} M={prior.n_samples} k={prior.dim}: largest difference to the model {err.max() if fin.any() else 0.0:.3e}, "
          f"largest share of the tolerance {(err / tol).max() if fin.any() else 0.0:.3f}")
    return np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]) and bool((err <= tol).all())


# ------------------------------------------------------------------------------------------------------------------
# 1. one sample: pmc_gauss_blocks_logpdf's bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_one_sample_has_the_gaussian_priors_bits(k):
    import pocomc_amd as pc
    rng = np.random.default_rng(7 * k + 1)
    s0, H = rng.normal(size=k) * 3.0, gpm.random_cov(k, 100.0, rng) * 2.5
    prior = pc.KDEPrior(s0[None, :], None, H)
    assert prior.logw[0] == 0.0 and not prior.t.any()
    plain = pc.GaussianPrior(s0, H)
    x = np.concatenate([gpm.draws(s0, H, 150, 1.0, rng), gpm.draws(s0, H, 49, 10.0, rng), s0[None, :]])
    xt = up(x)
    for n in NS:
        ref = bits(plain.logpdf_device(xt[:n].contiguous()))              # one launch of pmc_gauss_blocks_logpdf
        for other in layouts(xt[:n].contiguous()):
            got = prior.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
            assert np.array_equal(bits(got), ref), (k, n, other.stride())
    want = km.block_model(prior, x)
    assert np.array_equal(bits(prior.logpdf_device(xt)), want.view(np.int64))               # (and the model's)
    assert np.array_equal(prior.logpdf(x).view(np.int64), want.view(np.int64))
    assert prior.logpdf_device(torch.zeros(0, k, dtype=torch.float64, device="cuda")).shape == (0,)
    for bad in (torch.zeros(3, k, device="cuda"), torch.zeros(3, k + 1, dtype=torch.float64, device="cuda"),
                torch.zeros(3, k, dtype=torch.float64), np.zeros((3, k))):
        with pytest.raises(ValueError, match="KDEPrior.logpdf_device"):
            prior.logpdf_device(bad)


# ------------------------------------------------------------------------------------------------------------------
# 2. several samples: the model within the derived tolerance, the same bits among layouts, row counts and places
# ------------------------------------------------------------------------------------------------------------------
CASES = [(1, 2, False), (2, 7, True), (5, 8, False), (16, 9, True), (1, 63, True), (2, 65, False), (5, 513, True),
         (16, 4099, False), (2, 4099, True), (16, 513, True), (1, 8, True), (5, 2, True)]


@pytest.mark.parametrize("k,M,weighted", CASES)
def test_the_kernel_matches_the_model_within_the_derived_tolerance(k, M, weighted):
    prior, x, want = make(k, M, weighted)
    if weighted:
        assert prior.weights.max() / prior.weights.min() >= 0.99e12       # weights from 1 down to 1e-12
    xt = up(x)
    first = None
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = prior.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64
            if first is None or len(first) < n:
                assert close(got, want[:n], prior, f"n={n}"), (k, M, weighted, n)
                assert first is None or np.array_equal(bits(got)[:len(first)], first)
                first = bits(got)
            else:
                assert np.array_equal(bits(got), first[:n]), (k, M, weighted, n, other.stride())
    # the same rows alone, at the head and at the tail of a longer call
    some = xt[60:70].contiguous()
    assert np.array_equal(bits(prior.logpdf_device(some)), first[60:70])
    assert np.array_equal(bits(prior.logpdf_device(torch.cat([some, xt[:130]]))[:10]), first[60:70])
    assert np.array_equal(bits(prior.logpdf_device(torch.cat([xt[100:], some]))[-10:]), first[60:70])
    assert np.array_equal(bits(prior.logpdf_device(xt[37:38].contiguous())), first[37:38])
    assert np.array_equal(prior.logpdf(np.array(x)).view(np.int64), first)


def test_the_most_samples():
    prior, x, want = make(5, 65536, True)
    xt = up(x[:64])
    got = prior.logpdf_device(xt)
    assert close(got, want[:64], prior, "n=64")
    assert np.array_equal(bits(prior.logpdf_device(xt.t().contiguous().t())), bits(got))


def test_eight_or_fewer_samples_are_summed_in_the_models_order():
    """One sample a slice: the eight partial sums in slice order are the sequential sum, so the only differences left are
    ``exp``'s and ``log``'s."""
    prior, x, want = make(5, 8, False)
    assert np.array_equal(km.block_model(prior, x, chunks=8).view(np.int64), want.view(np.int64))
    assert close(prior.logpdf_device(up(x)), want, prior, "one sample a slice")


# ------------------------------------------------------------------------------------------------------------------
# 3. edges
# ------------------------------------------------------------------------------------------------------------------
HOLES = [0, 63, 64, 69]                  # first row, a tile's last, the next tile's first, the call's last


@pytest.mark.parametrize("k,M", [(2, 9), (16, 513)])
def test_far_rows_are_finite_and_bad_rows_are_minus_infinity(k, M):
    prior, x, want = make(k, M, True)
    n = 70
    clean = prior.logpdf_device(up(x[:n]))
    assert close(clean, want[:n], prior)
    clean = bits(clean)
    keep = np.setdiff1d(np.arange(n), HOLES)
    sd = np.sqrt(np.diag(prior.H))
    signs = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    for what, v in {"on a sample": prior.samples[3], "far": prior.samples.max(axis=0) + 1e3 * sd, "NaN": np.nan, "+inf": np.inf,
                    "-inf": -np.inf, "1e160": 1e160, "+-1e300": 1e300 * signs}.items():
        y = np.array(x[:n])
        if np.ndim(v) == 0 and not np.isfinite(v):
            y[HOLES, k // 2] = v                                          # one bad column is enough
        else:
            y[HOLES] = v
        model = km.block_model(prior, y)
        for other in layouts(up(y)):
            got = prior.logpdf_device(other).cpu().numpy()
            assert not np.isnan(got).any() and not np.isposinf(got).any(), what
            assert np.array_equal(got[keep].view(np.int64), clean[keep]), what      # the bad rows move nothing else
            assert close(got, model, prior, what), what
            if what == "on a sample":
                assert np.isfinite(got[HOLES]).all()
            elif what == "far":                                           # 1e3 bandwidths from every sample: finite
                assert np.isfinite(got[HOLES]).all() and (got[HOLES] < -1e4).all()
            else:
                assert np.isneginf(got[HOLES]).all(), (what, got[HOLES])


# ------------------------------------------------------------------------------------------------------------------
# 4. the entry through ctypes
# ------------------------------------------------------------------------------------------------------------------
class Entry:
    """An estimate of ``M`` samples on the columns ``cols`` of a ``D``-column x; ``rest``: a ``Prior`` on ``rest_cols``."""

    def __init__(self, D=12, cols=(7, 0, 10, 2), M=65, rest=None, rest_cols=(3, 6), real_cols=None):
        import pocomc_amd as pc
        from pocomc_amd import _lib
        k = len(cols)
        self.D, self.cols, self.k = D, list(cols), k
        real = self.cols if real_cols is None else list(real_cols)       # (where x carries the block when cols has a bad entry)
        self.prior = pc.KDEPrior(km.banana(M, k, 77), km.log_weights(M, 78, wmin=1e-6))
        blk = self.prior.device_block()
        self.keep = [up(np.array(cols, dtype=np.int32))] + [up(blk[f]) for f in ("center", "linv_packed", "t", "logw")]
        p = [t.data_ptr() for t in self.keep]
        self.g = _lib.pmc_kde_t(n_samples=M, dim=k, D=D, cols=p[0], center=p[1], linv=p[2], t=p[3], logw=p[4],
                                logc=float(blk["logc"]))
        self.rest = rest
        rng = np.random.default_rng(10)
        self.x = rng.normal(size=(200, D)) * 1.5
        self.x[:, real] = self.prior.samples[rng.integers(M, size=200)] + rng.normal(size=(200, k)) * 0.5
        if rest is not None:
            self.rdesc = rest.device_descriptor()
            self.rest_cols = up(np.array(rest_cols, dtype=np.int32))
            self.g.rest, self.g.rest_cols = C.addressof(self.rdesc), self.rest_cols.data_ptr()
            self.x[:, list(rest_cols)] = jpm.rest_rows(rest.dists, 200, rng)

    def call(self, xt, n, base=None, out=None, strides=None):
        from pocomc_amd import _lib
        out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda") if out is None else out
        rs, cs = strides if strides is not None else (self.D, 1)
        _lib.check(_lib.load().pmc_kde_logpdf(C.byref(self.g), C.c_void_p(xt.data_ptr()), rs, cs, n, _lib.ptr(base),
                                              _lib.ptr(out), _lib.stream_handle()), "pmc_kde_logpdf")
        return out


@pytest.mark.parametrize("shape", ["D=k", "D=12", "D=157"])
def test_columns_strides_a_base_in_place_and_a_table(shape):
    import pocomc_amd as pc
    from scipy.stats import gamma, uniform
    if shape == "D=k":
        kw, rest_cols = dict(D=5, cols=(3, 0, 4, 1, 2), M=9), None
    elif shape == "D=12":
        kw, rest_cols = dict(D=12, cols=(7, 0, 10, 2), M=65), (3, 6)      # interleaved with the table's and nobody's columns
    else:
        kw, rest_cols = dict(D=157, cols=tuple(range(150, 0, -10)) + (156,), M=513), (3, 155)
    e = Entry(**kw)
    D, cols, k = e.D, e.cols, e.k
    assert k == (16 if D == 157 else len(cols))
    xt = up(e.x)
    own = e.prior.logpdf_device(xt[:, cols].contiguous()).cpu().numpy()   # the block's own value on its gathered columns
    assert np.isfinite(own).all() and close(own, km.block_model(e.prior, e.x[:, cols]), e.prior, shape)
    base = np.random.default_rng(3).normal(size=200) * 10.0
    base[[5, 64]] = -np.inf                                               # a row another part has put outside its support
    with np.errstate(all="ignore"):
        on_base = np.where(np.isfinite(base + own), base + own, -np.inf)
    for n in NS:
        xc = xt[:n].contiguous()
        assert np.array_equal(bits(e.call(xc, n)), own[:n].view(np.int64)), n
        assert np.array_equal(bits(e.call(xc.t().contiguous(), n, strides=(1, n))), own[:n].view(np.int64)), n
        # rows three doubles longer than D, and every other double of a row twice as long and three: an odd stride
        wide = torch.full((n, D + 3), np.nan, dtype=torch.float64, device="cuda")
        wide[:, :D] = xc
        assert np.array_equal(bits(e.call(wide, n, strides=(D + 3, 1))), own[:n].view(np.int64)), n
        odd = torch.full((n, 2 * D + 3), np.nan, dtype=torch.float64, device="cuda")
        odd[:, 1:2 * D + 1:2] = xc
        assert np.array_equal(bits(e.call(odd[:, 1:], n, strides=(2 * D + 3, 2))), own[:n].view(np.int64)), n
        b = up(base[:n])
        assert np.array_equal(bits(e.call(xc, n, base=b)), on_base[:n].view(np.int64)), n
        assert np.array_equal(bits(b), base[:n].view(np.int64))
        got = e.call(xc, n, base=b, out=b)                                # in place
        assert got is b and np.array_equal(bits(b), on_base[:n].view(np.int64)), n
    if rest_cols is None:
        return
    y = np.array(e.x)                                                     # the columns that are nobody's are not read
    y[:, np.setdiff1d(np.arange(D), cols)] = np.nan
    assert np.array_equal(bits(e.call(up(y), 200)), own.view(np.int64))
    # with a table: pmc_prior_logpdf's bits on the gathered rest, then one addition
    rest = pc.Prior([uniform(-2.0, 5.0), gamma(0.5, loc=1.0)], device=True)
    e = Entry(rest=rest, rest_cols=rest_cols, **kw)
    x = e.x
    x[7, rest_cols[1]] = 1.0               # the gamma(0.5) pole: +inf in the table's own sum
    x[9, rest_cols[0]] = 3.5               # beyond the uniform factor
    x[11, rest_cols[1]] = np.nan
    x[13, cols[2]] = np.inf                # a block column
    xt = up(x)
    table = table_logp(rest, xt[:, list(rest_cols)].contiguous())
    own = e.prior.logpdf_device(xt[:, cols].contiguous()).cpu().numpy()
    with np.errstate(all="ignore"):
        want = np.where(np.isfinite(table + own), table + own, -np.inf)
    want[11] = -np.inf
    for n in NS:
        assert np.array_equal(bits(e.call(xt[:n].contiguous(), n)), want[:n].view(np.int64)), n
        assert np.array_equal(bits(e.call(xt[:n].t().contiguous(), n, strides=(1, n))), want[:n].view(np.int64)), n
    assert np.isneginf(want[[7, 9, 11, 13]]).all() and np.isfinite(np.delete(want, [7, 9, 11, 13])).all()


def test_a_column_outside_x_is_not_followed():
    for cols in ([7, 12, 10, 2], [7, 0, -1, 2]):                          # 12 and -1 are no columns of x
        e = Entry(cols=cols, real_cols=[7, 0, 10, 2])
        assert np.isneginf(e.call(up(e.x[:70]), 70).cpu().numpy()).all()


def test_the_entry_refuses_and_writes_nothing():
    import pocomc_amd as pc
    from pocomc_amd import _lib
    from scipy.stats import gamma
    lib = _lib.load()
    e = Entry()
    n, D = 4, e.D
    xt = up(e.x[:n])
    out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    base = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    st = _lib.stream_handle()

    def copy_of(**fields):
        c = type(e.g).from_buffer_copy(e.g)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def refused(text, g=None, x=xt, count=n, rs=D, cs=1, b=None, o=out):
        g = e.g if g is None else g
        rc = lib.pmc_kde_logpdf(None if g is False else C.byref(g), _lib.ptr(x), rs, cs, count, _lib.ptr(b), _lib.ptr(o), st)
        msg = lib.pmc_last_error()
        assert rc != 0 and msg.startswith(b"pmc_kde_logpdf: ") and text in msg, (text, rc, msg)
    refused(b"bad descriptor", g=False)
    for field in ("cols", "center", "linv", "t", "logw"):
        refused(b"bad KDE descriptor (a NULL array)", g=copy_of(**{field: None}))
    refused(b"n_samples must lie in 1 .. 65536", g=copy_of(n_samples=0))
    refused(b"n_samples must lie in 1 .. 65536", g=copy_of(n_samples=65537))
    refused(b"dim must lie in 1 .. 16", g=copy_of(dim=0))
    refused(b"dim must lie in 1 .. 16", g=copy_of(dim=17, D=100))
    refused(b"n_dim too large (D <= 157)", g=copy_of(D=158))
    refused(b"more columns than x", g=copy_of(D=3))
    ext = pc.Prior([gamma(2.0), gamma(3.0)], device=True).device_descriptor()
    cols2 = up(np.array([3, 6], dtype=np.int32))
    refused(b"more columns than x", g=copy_of(D=5, rest=C.addressof(ext), rest_cols=cols2.data_ptr()))
    refused(b"rest and rest_cols go together", g=copy_of(rest=C.addressof(ext)))
    refused(b"rest and rest_cols go together", g=copy_of(rest_cols=cols2.data_ptr()))
    no_par = type(ext).from_buffer_copy(ext)
    no_par.par = None
    refused(b"parameter table", g=copy_of(rest=C.addressof(no_par), rest_cols=cols2.data_ptr()))
    refused(b"base and rest exclude each other", g=copy_of(rest=C.addressof(ext), rest_cols=cols2.data_ptr()), b=base)
    refused(b"bad argument (a NULL x or logp)", x=None)
    refused(b"bad argument (a NULL x or logp)", o=None)
    refused(b"bad argument (a negative count or stride)", count=-1)
    refused(b"bad argument (a negative count or stride)", rs=-1)
    refused(b"bad argument (a negative count or stride)", cs=-1)
    refused(b"too many rows", count=64 * 2 ** 31)
    assert lib.pmc_kde_logpdf(C.byref(e.g), None, D, 1, 0, None, None, st) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (base == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------
# 5. KDE blocks in a JointPrior, D = 12: the KDE blocks' columns are the last ones, so that the first columns are the x of
#    the same prior without its KDE blocks
# ------------------------------------------------------------------------------------------------------------------
D12 = 12
_joint = {}


def gauss_of(k, seed):
    import pocomc_amd as pc
    rng = np.random.default_rng(seed)
    return pc.GaussianPrior(rng.normal(size=k), gpm.random_cov(k, 50.0, rng) * 1.5)


def mix_of(Cn, k, seed):
    import gauss_mix_model as gmm
    import pocomc_amd as pc
    return pc.GaussianMixturePrior(*gmm.random_mixture(Cn, k, seed, spread=2.0, wmin=1e-4))


def kde_of(M, k, seed):
    import pocomc_amd as pc
    return pc.KDEPrior(km.banana(M, k, seed), km.log_weights(M, seed, wmin=1e-4), "silverman")


def joint_case(name):
    """``(joint, the same prior without its KDE blocks or None, parts, columns, rest columns, rows)``, built once."""
    import gauss_mix_model as gmm
    import pocomc_amd as pc
    if name in _joint:
        return _joint[name]
    rng = np.random.default_rng(len(name))
    if name == "flow+gauss+mix+kde+table":
        flow = make_flow(3, 3, "affine")[0]
        parts = [flow, gauss_of(2, 1), mix_of(3, 2, 2), kde_of(65, 3, 3)]
        columns, Dr, head = [[4, 0, 2], [1, 5], [6, 3], [11, 9, 10]], 2, 3
    elif name == "kde+gauss+kde+table":                                   # the KDE blocks around the Gaussian block in the list
        parts, columns, Dr, head = [kde_of(9, 2, 2), gauss_of(3, 1), kde_of(513, 3, 4)], [[8, 7], [1, 5, 6], [11, 9, 10]], 4, None
    elif name == "kde+table":
        parts, columns, Dr, head = [kde_of(65, 5, 5)], [[11, 2, 9, 0, 10]], 7, None
    else:
        assert name == "kde+kde"
        parts, columns, Dr, head = [kde_of(8, 5, 6), kde_of(63, 7, 7)], [[8, 0, 3, 5, 11], [2, 7, 1, 6, 4, 9, 10]], 0, None
    dists = jpm.rest_dists(Dr)
    rest = pc.Prior(dists, device=True) if Dr else None
    joint = pc.JointPrior(parts, columns, rest)
    without = pc.JointPrior(parts[:head], columns[:head], rest) if head else None           # on the first 9 columns
    x = np.empty((200, D12))
    for p, c in zip(parts, columns):
        if isinstance(p, pc.FlowPrior):
            x[:, c] = rows_in(bounds_of(3), 200, rng)
        elif isinstance(p, pc.GaussianPrior):
            x[:, c] = gpm.draws(p.mean, p.cov, 200, 1.0, rng)
        elif isinstance(p, pc.GaussianMixturePrior):
            x[:, c] = gmm.mixture_draws(p.weights, p.means, p.covs, 200, 1.0, rng)
        else:
            x[:, c] = p.samples[rng.integers(p.n_samples, size=200)] + rng.normal(size=(200, p.dim)) * 0.4
    rest_cols = np.setdiff1d(np.arange(D12), np.concatenate(columns))
    if Dr:
        x[:, rest_cols] = jpm.rest_rows(dists, 200, rng)
    _joint[name] = (joint, without, parts, columns, rest_cols, x)
    return _joint[name]


def sum_of_parts(joint, without, parts, columns, rest_cols, xt, model=False, partials=None):
    """The documented order: the same prior without its KDE blocks (flow blocks in list order, the table, Gaussian blocks in
    list order, mixture blocks in list order: each part by itself on its gathered columns), then every KDE block's own
    ``logpdf_device`` (``model``: the numpy statement's ``v`` instead) in list order, added left to right in float64; -inf where
    that is not finite.  ``partials``: a list that takes the sum behind every KDE block's addition."""
    import pocomc_amd as pc
    v = None
    for p, c in zip(parts, columns):
        if isinstance(p, pc.FlowPrior):
            part = p.logpdf_device(xt[:, c].contiguous()).cpu().numpy()
            v = part if v is None else v + part
    if joint.rest is not None:
        t = table_logp(joint.rest, xt[:, rest_cols.tolist()].contiguous())
        v = t if v is None else v + t
    with np.errstate(all="ignore"):
        for kind in (pc.GaussianPrior, pc.GaussianMixturePrior):
            for p, c in zip(parts, columns):
                if isinstance(p, kind):
                    part = p.logpdf_device(xt[:, c].contiguous()).cpu().numpy()
                    v = part if v is None else v + part
                    if kind is pc.GaussianPrior:
                        v = np.where(np.isfinite(v), v, -np.inf)          # (the Gaussian launch's own closing test)
        if without is not None:                                           # the same prior without its KDE blocks, as a prior
            head = without.logpdf_device(xt[:, :without.dim].contiguous()).cpu().numpy()
            assert np.array_equal(head.view(np.int64), np.where(np.isfinite(v), v, -np.inf).view(np.int64))
        for p, c in zip(parts, columns):
            if isinstance(p, pc.KDEPrior):
                part = km.block_model(p, xt[:, c].cpu().numpy()) if model else p.logpdf_device(xt[:, c].contiguous()).cpu().numpy()
                v = part if v is None else v + part
                if partials is not None:
                    partials.append(np.array(v))
    return np.where(np.isfinite(v), v, -np.inf)


@pytest.mark.parametrize("name", ["flow+gauss+mix+kde+table", "kde+gauss+kde+table", "kde+table", "kde+kde"])
def test_a_joint_prior_is_the_sum_of_its_parts_in_the_documented_order(name):
    import pocomc_amd as pc
    joint, without, parts, columns, rest_cols, x = joint_case(name)
    kdes = [p for p in parts if isinstance(p, pc.KDEPrior)]
    n_flow = sum(isinstance(p, pc.FlowPrior) for p in parts)
    assert joint.dim == D12 and joint.blocks == len(parts) and len(joint.flow_priors) == n_flow
    assert isinstance(joint.kde_priors, tuple) and len(joint.kde_priors) == len(kdes) == len(joint._kdescs)
    assert all(type(g) is pc.KDEPrior and g is not p for g in joint.kde_priors for p in parts)        # owned copies
    # the table goes through the first KDE launch only where nothing precedes it
    nothing_before = n_flow == 0 and not joint.gaussian_priors and not joint.mixture_priors
    assert bool(joint._kdescs[0].rest) == (joint.rest is not None and nothing_before)
    assert not any(d.rest for d in joint._kdescs[1:])
    xt = up(x)
    want = sum_of_parts(joint, without, parts, columns, rest_cols, xt)
    assert np.isfinite(want).all()
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = joint.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64
            assert np.array_equal(bits(got), want[:n].view(np.int64)), (name, n, other.stride())
    assert np.array_equal(joint.logpdf(x).view(np.int64), want.view(np.int64))
    assert joint.logpdf_device(torch.zeros(0, D12, dtype=torch.float64, device="cuda")).shape == (0,)
    # against the numpy statement: the same prior without its KDE blocks (the same numbers on both sides) plus every KDE
    # block's v, each within its tolerance; an addition rounds its sum once on each side, 2^-53 of the sum each
    partials = []
    model = sum_of_parts(joint, without, parts, columns, rest_cols, xt, model=True, partials=partials)
    tol = sum(km.tolerance(p.n_samples, km.block_model(p, x[:, c]), p.logc) for p, c in zip(parts, columns)
              if isinstance(p, pc.KDEPrior)) + 2.0 ** -52 * sum(np.abs(v) for v in partials)
    err = np.abs(want - model)
    print(f"{name}: largest share of the tolerance {(err / tol).max():.3f}")
    assert (err <= tol).all()
    st = joint.__getstate__()
    assert st["kinds"] == ["flow" if isinstance(p, pc.FlowPrior) else "gmix" if isinstance(p, pc.GaussianMixturePrior)
                           else "kde" if isinstance(p, pc.KDEPrior) else "gauss" for p in parts]
    back = pickle.loads(pickle.dumps(joint))
    assert back.blocks == joint.blocks and back.dim == D12 and np.array_equal(back.bounds, joint.bounds)
    assert len(back.kde_priors) == len(kdes) and len(back.flow_priors) == n_flow
    assert np.array_equal(bits(back.logpdf_device(xt)), want.view(np.int64))
    with pytest.raises(ValueError, match="KDE block"):
        joint.step_stage(64)
    # outside any part's support: -inf, never NaN
    y = np.array(x[:70])
    y[3, columns[0][0]] = np.nan
    y[64, columns[-1][-1]] = np.inf
    y[66, columns[-1]] = 1e160
    if joint.rest is not None:
        y[5, rest_cols[0]] = 3.5                                          # beyond the uniform factor
    got = joint.logpdf_device(up(y)).cpu().numpy()
    bad = [3, 64, 66] + ([5] if joint.rest is not None else [])
    keep = np.setdiff1d(np.arange(70), bad)
    assert not np.isnan(got).any()
    assert np.isneginf(got[bad]).all() and np.array_equal(got[keep].view(np.int64), want[:70][keep].view(np.int64))
    # bounds and draws go by list order
    b = joint.bounds
    for p, c in zip(parts, columns):
        assert np.array_equal(b[c], p.bounds)
    torch.manual_seed(2)
    np.random.seed(2)
    r = joint.rvs(50)
    assert r.shape == (50, D12) and np.isfinite(joint.logpdf(r)).all()
    torch.manual_seed(2)
    np.random.seed(2)
    assert np.array_equal(back.rvs(50), r)


def test_a_joint_prior_without_a_kde_block_is_untouched():
    import gauss_mix_model as gmm
    import pocomc_amd as pc
    g3, m2 = gauss_of(3, 1), mix_of(3, 2, 2)
    dists = jpm.rest_dists(3)
    joint = pc.JointPrior([g3, m2], [[1, 5, 6], [7, 0]], pc.Prior(dists, device=True))
    assert joint.kde_priors == () and joint._kdescs == [] and joint.__getstate__()["kinds"] == ["gauss", "gmix"]
    rng = np.random.default_rng(4)
    x = np.empty((130, 8))
    x[:, [1, 5, 6]], x[:, [7, 0]], x[:, [2, 3, 4]] = gpm.draws(g3.mean, g3.cov, 130, 1.0, rng), \
        gmm.mixture_draws(m2.weights, m2.means, m2.covs, 130, 1.0, rng), jpm.rest_rows(dists, 130, rng)
    xt = up(x)
    got = joint.logpdf_device(xt)
    assert torch.isfinite(got).all() and np.array_equal(bits(got), bits(joint._logpdf_device_mix(xt)))
    # a state without the kind still loads
    st = joint.__getstate__()
    assert "kde" not in st["kinds"]
    back = pc.JointPrior.__new__(pc.JointPrior)
    back.__setstate__(st)
    assert back.kde_priors == () and np.array_equal(bits(back.logpdf_device(xt)), bits(got))
    flow = make_flow(3, 3, "affine")[0]
    flows = pc.JointPrior([flow], [[4, 0, 2]], pc.Prior(jpm.rest_dists(6), device=True))
    assert "kinds" not in flows.__getstate__() and flows.kde_priors == () and flows._jdesc.D == 0
    assert flows.step_stage(64) is not None


# ------------------------------------------------------------------------------------------------------------------
# 6. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
KW = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)


def test_the_samplers_two_routes_agree(tmp_path):
    import pocomc_amd as pc
    from scipy.stats import norm, uniform
    kde = pc.KDEPrior(km.banana(200, 2, 12) * 0.5 + 0.3)
    prior = pc.JointPrior([kde], [[0, 2]], pc.Prior([norm(0.5, 2.0), uniform(-6.0, 12.0)]))
    assert prior.dim == 4 and len(prior.kde_priors) == 1

    def run(on_device):
        s = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=on_device, **KW)
        s.run(n_total=256, n_evidence=0, progress=False)
        return s
    dev, host = run(True), run(False)
    assert dev.device_prior is True and host.device_prior is False
    for a, b in zip(dev.posterior(), host.posterior()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert dev.evidence() == host.evidence() and dev.calls == host.calls
    rd = dev.results
    assert np.isfinite(np.asarray(rd["logp"])).all() and np.asarray(rd["beta"])[-1] == 1.0
    xs = np.asarray(rd["x"]).reshape(-1, 4)
    assert np.array_equal(prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    # a checkpoint carries the estimate through its state
    dev.save_state(tmp_path / "kde.state")
    t = pc.Sampler(prior=pc.KDEPrior(np.zeros((1, 4)), None, np.eye(4)), likelihood=gauss_at(0.8), random_state=7,
                   device_prior=True, **KW)
    t.load_state(tmp_path / "kde.state")
    assert type(t.prior) is pc.JointPrior and t.prior is not prior and t.prior.kde_priors[0].n_samples == 200
    assert np.array_equal(t.prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    with pytest.raises(ValueError, match="needs a prior with a step_stage method"):
        pc.Sampler(prior=kde, likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)
    with pytest.raises(ValueError, match="KDE block"):
        pc.Sampler(prior=prior, likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)
