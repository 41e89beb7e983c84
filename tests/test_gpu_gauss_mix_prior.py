"""``pocomc_amd.GaussianMixturePrior`` and the mixture blocks of ``pocomc_amd.JointPrior`` on the device: one launch of
``pmc_gauss_mix_logpdf`` (``csrc/gauss_mix_prior.hip``) per mixture.

With one component the statement is bit for bit against ``GaussianPrior``.  With more the yardstick is
``tests/gauss_mix_model.py``, the kernel's arithmetic in numpy, to ``gauss_mix_model.tolerance``: the ``t_c`` are the model's
bits, the device's ``exp`` and ``log`` are not numpy's.  The ROCm toolchain ships no document that states an ulp bound for the
two functions, so the factor ``C + 8`` stands as derived (a 1-ulp ``exp`` and ``log``).  Among themselves the
layouts and the row counts give the same bits.  n = 70 is a full 64-row tile and a tail of 6, n = 257 five tiles."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import gauss_mix_model as gmm
import gauss_prior_model as gpm
import joint_prior_model as jpm
from .test_gpu_flow_prior import bits, bounds_of, gauss_at, make as make_flow, rows_in
from .test_gpu_gauss_prior import layouts, up
from .test_gpu_joint_prior import table_logp

pytestmark = pytest.mark.gpu

NS = [70, 257]
_made = {}


def make(Cn, k, spread):
    """``(prior, weights, means, covs, 257 rows, the model's values of them)``, built once per case: 200 rows at the
    components' widths and 57 at five times them, each from a component chosen uniformly."""
    import pocomc_amd as pc
    key = (Cn, k, spread)
    if key not in _made:
        w, m, c = gmm.random_mixture(Cn, k, 1000 * Cn + k + int(spread), spread=spread)
        prior = pc.GaussianMixturePrior(w, m, c)
        rng = np.random.default_rng(Cn + k)
        x = np.concatenate([gmm.mixture_draws(w, m, c, 200, 1.0, rng), gmm.mixture_draws(w, m, c, 57, 5.0, rng)])
        want = gmm.block_model(prior, x)
        assert np.isfinite(want).all()
        want.setflags(write=False)
        x.setflags(write=False)
        _made[key] = (prior, w, m, c, x, want)
    return _made[key]


def close(got, want, Cn):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    tol = gmm.tolerance(Cn, want[fin])
    print(f"C={Cn}: largest difference to the model {err.max() if fin.any() else 0.0:.3e}, "
          f"largest share of the tolerance {(err / tol).max() if fin.any() else 0.0:.3f}")
    return np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]) and (err <= tol).all()


# ------------------------------------------------------------------------------------------------------------------
# 1. one component: GaussianPrior's bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 33, 64])
def test_one_component_has_the_gaussian_priors_bits(k):
    import pocomc_amd as pc
    prior, w, m, c, x, want = make(1, k, 1.0)
    assert prior.logw[0] == 0.0
    plain = pc.GaussianPrior(m[0], c[0])
    xt = up(x)
    for n in NS:
        ref = bits(plain.logpdf_device(xt[:n].contiguous()))
        for other in layouts(xt[:n].contiguous()):
            got = prior.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
            assert np.array_equal(bits(got), ref), (k, n, other.stride())
    assert np.array_equal(bits(plain.logpdf_device(xt)), want.view(np.int64))               # (and the model's)
    assert np.array_equal(prior.logpdf(np.array(x)).view(np.int64), want.view(np.int64))
    assert prior.logpdf_device(torch.zeros(0, k, dtype=torch.float64, device="cuda")).shape == (0,)
    for bad in (torch.zeros(3, k, device="cuda"), torch.zeros(3, k + 1, dtype=torch.float64, device="cuda"),
                torch.zeros(3, k, dtype=torch.float64), np.zeros((3, k))):
        with pytest.raises(ValueError, match="GaussianMixturePrior.logpdf_device"):
            prior.logpdf_device(bad)


# ------------------------------------------------------------------------------------------------------------------
# 2. several components: the model within the derived tolerance, the same bits among layouts and row counts
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [1.0, 30.0])                           # overlapping, well separated
@pytest.mark.parametrize("Cn,k", [(2, 5), (7, 33), (32, 64), (32, 3)])
def test_the_kernel_matches_the_model_within_the_derived_tolerance(Cn, k, spread):
    prior, w, m, c, x, want = make(Cn, k, spread)
    assert w.max() / w.min() >= 0.99e12                                   # weights from 1 down to 1e-12
    xt = up(x)
    first = None
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = prior.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64
            if first is None or len(first) < n:
                assert close(got, want[:n], Cn), (Cn, k, spread, n)
                assert first is None or np.array_equal(bits(got)[:len(first)], first)
                first = bits(got)
            else:
                assert np.array_equal(bits(got), first[:n]), (Cn, k, spread, n, other.stride())
    # a row's bits do not depend on its place either
    assert np.array_equal(bits(prior.logpdf_device(xt[64:].contiguous())), first[64:])
    assert np.array_equal(bits(prior.logpdf_device(xt[37:38].contiguous())), first[37:38])


# ------------------------------------------------------------------------------------------------------------------
# 3. edges
# ------------------------------------------------------------------------------------------------------------------
HOLES = [0, 63, 64, 69]                  # first row, a tile's last, the next tile's first, the call's last


@pytest.mark.parametrize("Cn,k", [(2, 5), (7, 33)])
def test_far_rows_are_finite_and_bad_rows_are_minus_infinity(Cn, k):
    prior, w, m, c, x, want = make(Cn, k, 1.0)
    n = 70
    clean = prior.logpdf_device(up(x[:n]))
    assert close(clean, want[:n], Cn)
    clean = bits(clean)
    keep = np.setdiff1d(np.arange(n), HOLES)
    sd = np.sqrt(np.diag(c[0]))
    signs = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    for what, v in {"far": m[0] + 1e3 * sd, "NaN": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e200": 1e200,
                    "+-1e300": 1e300 * signs}.items():
        y = np.array(x[:n])
        if np.ndim(v) == 0 and not np.isfinite(v):
            y[HOLES, k // 2] = v                                          # one bad column is enough
        else:
            y[HOLES] = v
        model = gmm.block_model(prior, y)
        for other in layouts(up(y)):
            got = prior.logpdf_device(other).cpu().numpy()
            assert not np.isnan(got).any() and not np.isposinf(got).any(), what
            assert np.array_equal(got[keep].view(np.int64), clean[keep]), what      # the bad rows move nothing else
            assert close(got, model, Cn), what
            if what == "far":                                             # 1e3 widths from every component: finite
                assert np.isfinite(got[HOLES]).all() and (got[HOLES] < -1e4).all()
                blk = prior.device_block()
                with np.errstate(all="ignore"):
                    naive = np.log(np.exp(gmm.mix_t_model(y[HOLES], blk["logw"], blk["mean"], blk["linv_packed"],
                                                          blk["logc"])).sum(axis=0))
                assert np.isneginf(naive).all()
            else:
                assert np.isneginf(got[HOLES]).all(), (what, got[HOLES])


@pytest.mark.parametrize("k", [2, 33])
def test_identical_components_agree_with_the_one_component_value(k):
    import pocomc_amd as pc
    _, _, m, c, x, want = make(1, k, 1.0)
    xt = up(x[:70])
    for copies in (2, 4):                                                 # weights 1/2 and 1/4
        prior = pc.GaussianMixturePrior(np.ones(copies), np.stack([m[0]] * copies), np.stack([c[0]] * copies))
        assert np.array_equal(prior.logw, np.full(copies, np.log(1.0 / copies)))
        assert close(prior.logpdf_device(xt), want[:70], copies), (k, copies)


# ------------------------------------------------------------------------------------------------------------------
# 4. the entry through ctypes
# ------------------------------------------------------------------------------------------------------------------
D9 = 9
COLS = [7, 0, 4, 2]                      # permuted; columns 3 and 6 are the table's, or nobody's


class Entry:
    """A three-component mixture on four permuted columns of a 9-column x; ``rest``: a ``Prior`` on columns 3 and 6."""

    def __init__(self, rest=None, cols=COLS):
        import pocomc_amd as pc
        from pocomc_amd import _lib
        w, m, c = gmm.random_mixture(3, 4, 77, spread=2.0, wmin=1e-3)
        self.prior = pc.GaussianMixturePrior(w, m, c)
        blk = self.prior.device_block()
        self.keep = [up(np.array(cols, dtype=np.int32))] + [up(blk[f]) for f in ("logw", "mean", "linv_packed", "logc")]
        p = [t.data_ptr() for t in self.keep]
        self.g = _lib.pmc_gauss_mix_t(n_comp=3, dim=4, D=D9, cols=p[0], logw=p[1], mean=p[2], linv=p[3], logc=p[4])
        self.rest = rest
        rng = np.random.default_rng(10)
        self.x = rng.normal(size=(257, D9)) * 1.5
        self.x[:, COLS] = gmm.mixture_draws(w, m, c, 257, 1.5, rng)
        if rest is not None:
            self.rdesc = rest.device_descriptor()
            self.rest_cols = up(np.array([3, 6], dtype=np.int32))
            self.g.rest, self.g.rest_cols = C.addressof(self.rdesc), self.rest_cols.data_ptr()
            self.x[:, [3, 6]] = jpm.rest_rows(rest.dists, 257, rng)

    def call(self, xt, base=None, out=None, strides=None):
        from pocomc_amd import _lib
        n = xt.shape[0] if strides is None else xt.shape[1]               # (strides: the [D][n] column-major array)
        out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda") if out is None else out
        rs, cs = strides if strides is not None else (D9, 1)
        _lib.check(_lib.load().pmc_gauss_mix_logpdf(C.byref(self.g), C.c_void_p(xt.data_ptr()), rs, cs, n, _lib.ptr(base),
                                                    _lib.ptr(out), _lib.stream_handle()), "pmc_gauss_mix_logpdf")
        return out


def test_permuted_columns_alone_on_a_base_in_place_and_with_a_table():
    import pocomc_amd as pc
    from scipy.stats import gamma, uniform
    e = Entry()
    xt = up(e.x)
    own = e.prior.logpdf_device(xt[:, COLS].contiguous()).cpu().numpy()   # the block's own value on its gathered columns
    assert np.isfinite(own).all() and close(own, gmm.block_model(e.prior, e.x[:, COLS]), 3)
    base = np.random.default_rng(3).normal(size=257) * 10.0
    base[[5, 64]] = -np.inf                                               # a row another part has put outside its support
    with np.errstate(all="ignore"):
        on_base = np.where(np.isfinite(base + own), base + own, -np.inf)
    for n in NS:
        xc = xt[:n].contiguous()
        assert np.array_equal(bits(e.call(xc)), own[:n].view(np.int64)), n
        assert np.array_equal(bits(e.call(xc.t().contiguous(), strides=(1, n))), own[:n].view(np.int64)), n
        b = up(base[:n])
        assert np.array_equal(bits(e.call(xc, base=b)), on_base[:n].view(np.int64)), n
        assert np.array_equal(bits(b), base[:n].view(np.int64))
        got = e.call(xc, base=b, out=b)                                   # in place
        assert got is b and np.array_equal(bits(b), on_base[:n].view(np.int64)), n
    y = np.array(e.x)                                                     # the columns that are nobody's are not read
    y[:, [1, 3, 5, 6, 8]] = np.nan
    assert np.array_equal(bits(e.call(up(y))), own.view(np.int64))
    # with a table: pmc_prior_logpdf's bits on the gathered rest, then one addition
    rest = pc.Prior([uniform(-2.0, 5.0), gamma(0.5, loc=1.0)], device=True)
    e = Entry(rest)
    x = e.x
    x[7, 6] = 1.0                          # the gamma(0.5) pole: +inf in the table's own sum
    x[9, 3] = 3.5                          # beyond the uniform factor
    x[11, 6] = np.nan
    x[13, 2] = np.inf                      # a block column
    xt = up(x)
    table = table_logp(rest, xt[:, [3, 6]].contiguous())
    own = e.prior.logpdf_device(xt[:, COLS].contiguous()).cpu().numpy()
    with np.errstate(all="ignore"):
        want = np.where(np.isfinite(table + own), table + own, -np.inf)
    want[11] = -np.inf
    for n in NS:
        assert np.array_equal(bits(e.call(xt[:n].contiguous())), want[:n].view(np.int64)), n
        assert np.array_equal(bits(e.call(xt[:n].t().contiguous(), strides=(1, n))), want[:n].view(np.int64)), n
    assert np.isneginf(want[[7, 9, 11, 13]]).all() and np.isfinite(np.delete(want, [7, 9, 11, 13])).all()


def test_a_column_outside_x_is_not_followed():
    for cols in ([7, 9, 4, 2], [7, 0, -1, 2]):                            # 9 and -1 are no columns of x
        e = Entry(cols=cols)
        assert np.isneginf(e.call(up(e.x[:70])).cpu().numpy()).all()


def test_the_entry_refuses_and_writes_nothing():
    import pocomc_amd as pc
    from pocomc_amd import _lib
    from scipy.stats import gamma
    lib = _lib.load()
    e = Entry()
    n = 4
    xt = up(e.x[:n])
    out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    base = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    st = _lib.stream_handle()

    def copy_of(**fields):
        c = type(e.g).from_buffer_copy(e.g)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def refused(text, g=None, x=xt, count=n, rs=D9, cs=1, b=None, o=out):
        g = e.g if g is None else g
        rc = lib.pmc_gauss_mix_logpdf(None if g is False else C.byref(g), _lib.ptr(x), rs, cs, count, _lib.ptr(b),
                                      _lib.ptr(o), st)
        msg = lib.pmc_last_error()
        assert rc != 0 and msg.startswith(b"pmc_gauss_mix_logpdf: ") and text in msg, (text, rc, msg)
    refused(b"bad descriptor", g=False)
    for field in ("cols", "logw", "mean", "linv", "logc"):
        refused(b"bad mixture descriptor (a NULL array)", g=copy_of(**{field: None}))
    refused(b"n_comp must lie in 1 .. 32", g=copy_of(n_comp=0))
    refused(b"n_comp must lie in 1 .. 32", g=copy_of(n_comp=33))
    refused(b"dim must lie in 1 .. 64", g=copy_of(dim=0))
    refused(b"dim must lie in 1 .. 64", g=copy_of(dim=65, D=100))
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
    assert lib.pmc_gauss_mix_logpdf(C.byref(e.g), None, D9, 1, 0, None, None, st) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (base == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------
# 5. mixture blocks in a JointPrior, D = 12: the mixtures' columns are the last ones, so that the first columns are the x of
#    the same prior without its mixture blocks
# ------------------------------------------------------------------------------------------------------------------
D12 = 12
_joint = {}


def gauss_of(k, seed):
    import pocomc_amd as pc
    rng = np.random.default_rng(seed)
    return pc.GaussianPrior(rng.normal(size=k), gpm.random_cov(k, 50.0, rng) * 1.5)


def mix_of(Cn, k, seed):
    import pocomc_amd as pc
    return pc.GaussianMixturePrior(*gmm.random_mixture(Cn, k, seed, spread=2.0, wmin=1e-4))


def joint_case(name):
    """``(joint, the same prior without its mixture blocks or None, parts, columns, rest or None, rows)``, built once."""
    import pocomc_amd as pc
    if name in _joint:
        return _joint[name]
    rng = np.random.default_rng(len(name))
    if name == "flow+gauss+mix+table":
        flow = make_flow(3, 3, "affine")[0]
        parts, columns, Dr, head = [flow, gauss_of(3, 1), mix_of(3, 3, 2)], [[4, 0, 2], [1, 5, 6], [11, 9, 10]], 3, 2
    elif name == "mix+gauss+mix+table":                                   # the mixtures around the Gaussian block in the list
        parts, columns, Dr, head = [mix_of(3, 2, 2), gauss_of(3, 1), mix_of(2, 3, 4)], [[8, 7], [1, 5, 6], [11, 9, 10]], 4, None
    elif name == "mix+table":
        parts, columns, Dr, head = [mix_of(4, 5, 5)], [[11, 2, 9, 0, 10]], 7, None
    else:
        assert name == "mix+mix"
        parts, columns, Dr, head = [mix_of(3, 5, 6), mix_of(2, 7, 7)], [[8, 0, 3, 5, 11], [2, 7, 1, 6, 4, 9, 10]], 0, None
    dists = jpm.rest_dists(Dr)
    rest = pc.Prior(dists, device=True) if Dr else None
    joint = pc.JointPrior(parts, columns, rest)
    without = pc.JointPrior(parts[:head], columns[:head], rest) if head else None           # on the first 9 columns
    x = np.empty((257, D12))
    for p, c in zip(parts, columns):
        if isinstance(p, pc.FlowPrior):
            x[:, c] = rows_in(bounds_of(3), 257, rng)
        elif isinstance(p, pc.GaussianPrior):
            x[:, c] = gpm.draws(p.mean, p.cov, 257, 1.0, rng)
        else:
            x[:, c] = gmm.mixture_draws(p.weights, p.means, p.covs, 257, 1.0, rng)
    rest_cols = np.setdiff1d(np.arange(D12), np.concatenate(columns))
    if Dr:
        x[:, rest_cols] = jpm.rest_rows(dists, 257, rng)
    _joint[name] = (joint, without, parts, columns, rest_cols, x)
    return _joint[name]


def sum_of_parts(joint, without, parts, columns, rest_cols, xt):
    """The documented order: the same prior without its mixture blocks (flow blocks in list order, the table, Gaussian blocks
    in list order: each part by itself on its gathered columns), then every mixture block's own ``logpdf_device`` in list
    order, added left to right in float64; -inf where that is not finite."""
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
        if without is not None:
            head = without.logpdf_device(xt[:, :without.dim].contiguous()).cpu().numpy()
            for p, c in zip(parts, columns):
                if isinstance(p, pc.GaussianMixturePrior):
                    head = head + p.logpdf_device(xt[:, c].contiguous()).cpu().numpy()
            assert np.array_equal(np.where(np.isfinite(head), head, -np.inf).view(np.int64),
                                  np.where(np.isfinite(v), v, -np.inf).view(np.int64))
    return np.where(np.isfinite(v), v, -np.inf)


@pytest.mark.parametrize("name", ["flow+gauss+mix+table", "mix+gauss+mix+table", "mix+table", "mix+mix"])
def test_a_joint_prior_is_the_sum_of_its_parts_in_the_documented_order(name):
    import pocomc_amd as pc
    joint, without, parts, columns, rest_cols, x = joint_case(name)
    n_mix = sum(isinstance(p, pc.GaussianMixturePrior) for p in parts)
    n_flow = sum(isinstance(p, pc.FlowPrior) for p in parts)
    assert joint.dim == D12 and joint.blocks == len(parts) and len(joint.flow_priors) == n_flow
    assert isinstance(joint.mixture_priors, tuple) and len(joint.mixture_priors) == n_mix == len(joint._mdescs)
    assert len(joint.gaussian_priors) == len(parts) - n_flow - n_mix
    assert all(type(g) is pc.GaussianMixturePrior and g is not p for g in joint.mixture_priors for p in parts)      # owned copies
    # the table goes through the first mixture launch only where nothing precedes it
    assert bool(joint._mdescs[0].rest) == (joint.rest is not None and n_flow == 0 and not joint.gaussian_priors)
    assert not any(d.rest for d in joint._mdescs[1:])
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
    st = joint.__getstate__()
    assert st["kinds"] == ["flow" if isinstance(p, pc.FlowPrior) else "gmix" if isinstance(p, pc.GaussianMixturePrior)
                           else "gauss" for p in parts]
    back = pickle.loads(pickle.dumps(joint))
    assert back.blocks == joint.blocks and back.dim == D12 and np.array_equal(back.bounds, joint.bounds)
    assert len(back.mixture_priors) == n_mix and len(back.flow_priors) == n_flow
    assert np.array_equal(bits(back.logpdf_device(xt)), want.view(np.int64))
    with pytest.raises(ValueError, match="mixture block"):
        joint.step_stage(64)
    # outside any part's support: -inf, never NaN
    y = np.array(x[:70])
    y[3, columns[0][0]] = np.nan
    y[64, columns[-1][-1]] = np.inf
    y[66, columns[-1]] = 1e200
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


def test_a_joint_prior_without_a_mixture_block_is_untouched():
    import pocomc_amd as pc
    flow, g3 = make_flow(3, 3, "affine")[0], gauss_of(3, 1)
    dists = jpm.rest_dists(3)
    joint = pc.JointPrior([flow, g3], [[4, 0, 2], [1, 5, 6]], pc.Prior(dists, device=True))
    assert joint.mixture_priors == () and joint._mdescs == [] and joint.__getstate__()["kinds"] == ["flow", "gauss"]
    rng = np.random.default_rng(4)
    x = np.empty((130, 9))
    x[:, [4, 0, 2]], x[:, [1, 5, 6]], x[:, [3, 7, 8]] = rows_in(bounds_of(3), 130, rng), gpm.draws(g3.mean, g3.cov, 130, 1.0, rng), \
        jpm.rest_rows(dists, 130, rng)
    xt = up(x)
    got = joint.logpdf_device(xt)
    assert torch.isfinite(got).all() and np.array_equal(bits(got), bits(joint._logpdf_device_gauss(xt)))
    blk = g3.device_block()
    parts = (flow.logpdf_device(xt[:, [4, 0, 2]].contiguous()).cpu().numpy()
             + table_logp(joint.rest, xt[:, [3, 7, 8]].contiguous()))
    want = gpm.gauss_blocks_model(x, [([1, 5, 6], blk["mean"], blk["linv_packed"], float(blk["logc"]))], parts)
    assert np.array_equal(bits(got), want.view(np.int64))
    # a state without the kind still loads
    st = joint.__getstate__()
    assert "gmix" not in st["kinds"]
    back = pc.JointPrior.__new__(pc.JointPrior)
    back.__setstate__(st)
    assert back.mixture_priors == () and np.array_equal(bits(back.logpdf_device(xt)), bits(got))
    flows = pc.JointPrior([flow], [[4, 0, 2]], pc.Prior(jpm.rest_dists(6), device=True))
    assert "kinds" not in flows.__getstate__() and flows.mixture_priors == () and flows._jdesc.D == 0
    assert flows.step_stage(64) is not None


# ------------------------------------------------------------------------------------------------------------------
# 6. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
KW = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)


def test_a_bimodal_prior_in_the_sampler(tmp_path):
    import pocomc_amd as pc
    rng = np.random.default_rng(12)
    means = np.array([[-1.5, 0.0, 0.5, 0.0], [1.5, 0.5, -0.5, 1.0]])
    covs = np.stack([gpm.random_cov(4, 20.0, rng) * 1.5, gpm.random_cov(4, 20.0, rng) * 1.5])
    prior = pc.GaussianMixturePrior([0.4, 0.6], means, covs)
    assert prior.dim == 4
    s = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=True, **KW)
    s.run(n_total=256, n_evidence=0, progress=False)
    assert s.device_prior is True
    rd = s.results
    assert np.isfinite(np.asarray(rd["logp"])).all() and np.asarray(rd["beta"])[-1] == 1.0
    xs = np.asarray(rd["x"]).reshape(-1, 4)
    assert np.array_equal(prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    # a checkpoint carries the prior through its state
    s.save_state(tmp_path / "mix.state")
    t = pc.Sampler(prior=pc.GaussianMixturePrior([1.0], [np.zeros(4)], [np.eye(4)]), likelihood=gauss_at(0.8), random_state=7,
                   device_prior=True, **KW)
    t.load_state(tmp_path / "mix.state")
    assert type(t.prior) is pc.GaussianMixturePrior and t.prior is not prior and t.prior.components == 2
    assert np.array_equal(t.prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    with pytest.raises(ValueError, match="needs a prior with a step_stage method"):
        pc.Sampler(prior=prior, likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)
    joint = pc.JointPrior([prior], [[0, 1, 2, 3]])
    with pytest.raises(ValueError, match="mixture block"):
        pc.Sampler(prior=joint, likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)
