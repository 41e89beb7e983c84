"""``pocomc_amd.GaussianPrior`` and the Gaussian blocks of ``pocomc_amd.JointPrior`` on the device: one launch of
``pmc_gauss_blocks_logpdf`` (``csrc/gauss_prior.hip``).

The yardstick is ``tests/gauss_prior_model.py``, the kernel's arithmetic in numpy, and the statement is bit for bit: every
width class, the 64-row tile's edges, both coalesced layouts and a slice, bad rows, the entry through ctypes (on top of a base,
in place, with a table), the joint prior as the sum of its parts in the documented order, and the Sampler's two routes."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import gauss_prior_model as gpm
import joint_prior_model as jpm
from .test_gpu_flow_prior import bits, bounds_of, gauss_at, make as make_flow, rows_in
from .test_gpu_joint_prior import table_logp

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 33, 157]                  # one column, the crossing of 32 (four rows a lane x eight wavefronts), the limit
NS = [1, 63, 64, 65, 200]
_made = {}


def make(k, cond=100.0):
    """``(prior, mean, cov, 200 rows, the model's values of them)``, built once per width."""
    import pocomc_amd as pc
    if k not in _made:
        rng = np.random.default_rng(7 * k + 1)
        mean = rng.normal(size=k) * 3.0
        cov = gpm.random_cov(k, cond, rng) * 2.5
        prior = pc.GaussianPrior(mean, cov)
        x = np.concatenate([gpm.draws(mean, cov, 150, 1.0, rng), gpm.draws(mean, cov, 50, 10.0, rng)])
        blk = prior.device_block()
        want = gpm.gauss_block_model(x, blk["mean"], blk["linv_packed"], float(blk["logc"]))
        assert np.isfinite(want).all()
        want.setflags(write=False)
        x.setflags(write=False)
        _made[k] = (prior, mean, cov, x, want)
    return _made[k]


def up(a):
    return torch.from_numpy(np.array(a)).cuda()


def layouts(xc):
    """The C-contiguous tensor, its column-major view and a slice that is neither."""
    n, D = xc.shape
    colmajor = xc.t().contiguous().t()
    wide = torch.zeros(n, 2 * D + 3, dtype=torch.float64, device=xc.device)
    wide[:, 1:2 * D + 1:2] = xc
    sliced = wide[:, 1:2 * D + 1:2]
    assert xc.is_contiguous() and (n == 1 or D == 1 or colmajor.stride() == (1, n))
    assert (n == 1 and D == 1) or not sliced.is_contiguous()
    return xc, colmajor, sliced


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel is the model
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_the_kernel_equals_the_model_bit_for_bit(k):
    prior, _, _, x, want = make(k)
    xt = up(x)
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = prior.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
            assert np.array_equal(bits(got), want[:n].view(np.int64)), (k, n, other.stride())
    assert np.array_equal(prior.logpdf(np.array(x)).view(np.int64), want.view(np.int64))
    assert prior.logpdf_device(torch.zeros(0, k, dtype=torch.float64, device="cuda")).shape == (0,)
    for bad in (torch.zeros(3, k, device="cuda"), torch.zeros(3, k + 1, dtype=torch.float64, device="cuda"),
                torch.zeros(3, k, dtype=torch.float64), np.zeros((3, k))):
        with pytest.raises(ValueError):
            prior.logpdf_device(bad)


@pytest.mark.parametrize("k", KS)
def test_a_rows_bits_do_not_depend_on_n_its_place_or_the_layout(k):
    prior, mean, cov, x, want = make(k)
    row = x[17:18]
    alone = bits(prior.logpdf_device(up(row)))
    assert alone[0] == want[17:18].view(np.int64)[0]
    y = np.array(x)
    y[0], y[199] = row, row
    for other in layouts(up(y))[:2]:
        got = bits(prior.logpdf_device(other))
        assert got[0] == alone[0] and got[199] == alone[0] and got[17] == alone[0]
        assert np.array_equal(got[1:199], want[1:199].view(np.int64))
        assert np.array_equal(bits(prior.logpdf_device(other[37:])), got[37:])
        assert np.array_equal(bits(prior.logpdf_device(other[64:])), got[64:])


# ------------------------------------------------------------------------------------------------------------------
# 2. bad rows
# ------------------------------------------------------------------------------------------------------------------
HOLES = [0, 63, 64, 129]                 # first row, a tile's last, the next tile's first, the call's last


@pytest.mark.parametrize("k", [1, 5, 33])
def test_bad_rows_are_minus_infinity_and_move_nothing_else(k):
    prior, mean, cov, x, want = make(k)
    blk = prior.device_block()
    n = 130
    good = want[:n].view(np.int64)
    signs = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    for what, v in {"NaN": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e300": 1e300, "-1e300": -1e300,
                    "+-1e300": 1e300 * signs, "1.7e308": 1.7e308}.items():
        y = np.array(x[:n])
        if np.ndim(v) == 0 and not np.isfinite(v):
            y[HOLES, k // 2] = v                                          # one bad column is enough
        else:
            y[HOLES] = v
        model = gpm.gauss_block_model(y, blk["mean"], blk["linv_packed"], float(blk["logc"]))
        assert np.isneginf(model[HOLES]).all()
        keep = np.setdiff1d(np.arange(n), HOLES)
        for other in layouts(up(y)):
            got = prior.logpdf_device(other).cpu().numpy()
            assert np.isneginf(got[HOLES]).all(), (what, got[HOLES])
            assert not np.isnan(got).any() and not np.isposinf(got).any(), what
            assert np.array_equal(got[keep].view(np.int64), good[keep]), what
            assert np.array_equal(got.view(np.int64), model.view(np.int64)), what


# ------------------------------------------------------------------------------------------------------------------
# 3. the entry through ctypes
# ------------------------------------------------------------------------------------------------------------------
D9 = 9
COLS9 = [[7, 0, 4], [2, 8, 1, 5]]        # two blocks, permuted and interleaved; columns 3 and 6 are nobody's, or the table's


class Entry:
    """Two blocks at D = 9 with their device arrays and descriptor; ``rest``: a ``Prior`` on columns 3 and 6, or None."""

    def __init__(self, rest=None, cols=COLS9):
        import pocomc_amd as pc
        from pocomc_amd import _lib
        rng = np.random.default_rng(9)
        self.blocks, self.keep = [], []
        g = _lib.pmc_gauss_blocks_t(n_blocks=len(cols), D=D9)
        for b, c in enumerate(cols):
            k = len(c)
            mean = rng.normal(size=k)
            mean_, packed, logc = gpm.constants(mean, gpm.random_cov(k, 50.0, rng) * 1.5)
            self.blocks.append((c, mean_, packed, logc))
            t = [up(np.array(c, dtype=np.int32)), up(mean_), up(packed)]
            self.keep.append(t)
            g.dim[b], g.logc[b] = k, logc
            g.cols[b], g.mean[b], g.linv[b] = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
        self.rest = rest
        if rest is not None:
            self.rdesc = rest.device_descriptor()
            self.rest_cols = up(np.array([3, 6], dtype=np.int32))
            g.rest, g.rest_cols = C.addressof(self.rdesc), self.rest_cols.data_ptr()
        self.g = g
        self.x = np.random.default_rng(10).normal(size=(200, D9)) * 1.5
        if rest is not None:
            self.x[:, [3, 6]] = jpm.rest_rows(rest.dists, 200, rng)

    def call(self, xt, base=None, out=None, strides=None):
        from pocomc_amd import _lib
        n = xt.shape[0] if strides is None else xt.shape[1]               # (strides: the [D][n] column-major array)
        out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda") if out is None else out
        rs, cs = strides if strides is not None else (D9, 1)
        _lib.check(_lib.load().pmc_gauss_blocks_logpdf(C.byref(self.g), C.c_void_p(xt.data_ptr()), rs, cs, n, _lib.ptr(base),
                                                       _lib.ptr(out), _lib.stream_handle()), "pmc_gauss_blocks_logpdf")
        return out


def test_two_blocks_on_permuted_columns_alone_on_a_base_and_in_place():
    e = Entry()
    want = gpm.gauss_blocks_model(e.x, e.blocks)
    g0 = gpm.gauss_block_model(e.x[:, COLS9[0]], *e.blocks[0][1:])
    g1 = gpm.gauss_block_model(e.x[:, COLS9[1]], *e.blocks[1][1:])
    assert np.isfinite(want).all() and np.array_equal(want, g0 + g1)
    xt = up(e.x)
    base = np.random.default_rng(3).normal(size=200) * 10.0
    base[[5, 64]] = -np.inf                                               # a row another part has put outside its support
    on_base = gpm.gauss_blocks_model(e.x, e.blocks, base)
    assert np.array_equal(on_base[6:64], ((base + g0) + g1)[6:64]) and np.isneginf(on_base[[5, 64]]).all()
    for n in NS:
        xc = xt[:n].contiguous()
        assert np.array_equal(bits(e.call(xc)), want[:n].view(np.int64)), n
        colmajor = xc.t().contiguous()
        assert np.array_equal(bits(e.call(colmajor, strides=(1, n))), want[:n].view(np.int64)), n
        b = up(base[:n])
        assert np.array_equal(bits(e.call(xc, base=b)), on_base[:n].view(np.int64)), n
        assert np.array_equal(bits(b), base[:n].view(np.int64))
        got = e.call(xc, base=b, out=b)                                   # in place
        assert got is b and np.array_equal(bits(b), on_base[:n].view(np.int64)), n
    # the columns that are nobody's are not read: a NaN there moves nothing
    y = np.array(e.x)
    y[:, [3, 6]] = np.nan
    assert np.array_equal(bits(e.call(up(y))), want.view(np.int64))


def test_with_a_table_the_value_is_pmc_prior_logpdf_plus_the_model():
    import pocomc_amd as pc
    from scipy.stats import gamma, uniform
    rest = pc.Prior([uniform(-2.0, 5.0), gamma(0.5, loc=1.0)], device=True)
    e = Entry(rest)
    x = e.x
    x[7, 6] = 1.0                          # the gamma(0.5) pole: +inf in the table's own sum
    x[9, 3] = 3.5                          # beyond the uniform factor
    x[11, 6] = np.nan
    x[13, 2] = np.inf                      # a block column
    xt = up(x)
    table = table_logp(rest, xt[:, [3, 6]].contiguous())
    assert np.isposinf(table[7]) and np.isneginf(table[9]) and np.isfinite(np.delete(table, [7, 9, 11, 13])).all()
    want = gpm.gauss_blocks_model(x, e.blocks, table)
    for n in NS:
        got = e.call(xt[:n].contiguous())
        assert np.array_equal(bits(got), want[:n].view(np.int64)), n
        colmajor = xt[:n].t().contiguous()
        assert np.array_equal(bits(e.call(colmajor, strides=(1, n))), want[:n].view(np.int64)), n
    got = e.call(xt).cpu().numpy()
    assert np.isneginf(got[[7, 9, 11, 13]]).all() and np.isfinite(np.delete(got, [7, 9, 11, 13])).all()


def test_a_column_outside_x_is_not_followed():
    e = Entry(cols=[[7, 0, 4], [2, 9, 1, 5]])                             # 9 is no column of x
    got = e.call(up(e.x[:70])).cpu().numpy()
    assert np.isneginf(got).all()
    e = Entry(cols=[[7, 0, -1], [2, 8, 1, 5]])
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
        rc = lib.pmc_gauss_blocks_logpdf(None if g is False else C.byref(g), _lib.ptr(x), rs, cs, count, _lib.ptr(b),
                                         _lib.ptr(o), st)
        assert rc != 0 and text in lib.pmc_last_error(), (text, rc, lib.pmc_last_error())
    refused(b"bad descriptor", g=False)
    refused(b"n_blocks must lie in 1 .. 8", g=copy_of(n_blocks=0))
    refused(b"n_blocks must lie in 1 .. 8", g=copy_of(n_blocks=9))
    for field in ("cols", "mean", "linv"):
        g = copy_of()
        getattr(g, field)[1] = None
        refused(b"bad block descriptor", g=g)
    g = copy_of()
    g.dim[0] = 0
    refused(b"at least 1 column", g=g)
    refused(b"n_dim too large", g=copy_of(D=158))
    refused(b"more columns than x", g=copy_of(D=6))
    ext = pc.Prior([gamma(2.0), gamma(3.0)], device=True).device_descriptor()
    cols2 = up(np.array([3, 6], dtype=np.int32))
    refused(b"rest and rest_cols go together", g=copy_of(rest=C.addressof(ext)))
    refused(b"rest and rest_cols go together", g=copy_of(rest_cols=cols2.data_ptr()))
    no_par = type(ext).from_buffer_copy(ext)
    no_par.par = None
    refused(b"parameter table", g=copy_of(rest=C.addressof(no_par), rest_cols=cols2.data_ptr()))
    refused(b"base and rest exclude each other", g=copy_of(rest=C.addressof(ext), rest_cols=cols2.data_ptr()), b=base)
    refused(b"bad argument", x=None)
    refused(b"bad argument", o=None)
    refused(b"bad argument", count=-1)
    refused(b"bad argument", rs=-1)
    refused(b"bad argument", cs=-1)
    refused(b"too many rows", count=64 * 2 ** 31)
    assert lib.pmc_gauss_blocks_logpdf(C.byref(e.g), None, D9, 1, 0, None, None, st) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (base == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. Gaussian blocks in a JointPrior, D = 9
# ------------------------------------------------------------------------------------------------------------------
def gauss_of(k, seed):
    import pocomc_amd as pc
    rng = np.random.default_rng(seed)
    mean = rng.normal(size=k)
    return pc.GaussianPrior(mean, gpm.random_cov(k, 50.0, rng) * 1.5)


_joint = {}


def joint_case(name):
    """``(joint, blocks in list order, columns, dists, rows)`` of a case, built once."""
    import pocomc_amd as pc
    if name in _joint:
        return _joint[name]
    rng = np.random.default_rng(len(name))
    flow = make_flow(3, 3, "affine")[0]
    if name == "flow+gauss+table":
        parts, columns, dists = [flow, gauss_of(3, 1)], [[4, 0, 2], [1, 5, 6]], jpm.rest_dists(3)
    elif name == "gauss+flow+table":                                      # the same prior, the Gaussian block first in the list
        parts, columns, dists = [gauss_of(3, 1), flow], [[1, 5, 6], [4, 0, 2]], jpm.rest_dists(3)
    elif name == "gauss+table":
        parts, columns, dists = [gauss_of(3, 1)], [[1, 5, 6]], jpm.rest_dists(6)
    else:
        assert name == "gauss+gauss"
        parts, columns, dists = [gauss_of(4, 2), gauss_of(5, 3)], [[8, 0, 3, 5], [2, 7, 1, 6, 4]], []
    joint = pc.JointPrior(parts, columns, pc.Prior(dists, device=True) if dists else None)
    n = 200
    x = np.empty((n, D9))
    for p, c in zip(parts, columns):
        x[:, c] = rows_in(bounds_of(3), n, rng) if isinstance(p, pc.FlowPrior) else gpm.draws(p.mean, p.cov, n, 1.0, rng)
    rest_cols = np.setdiff1d(np.arange(D9), np.concatenate(columns))
    if dists:
        x[:, rest_cols] = jpm.rest_rows(dists, n, rng)
    _joint[name] = (joint, parts, columns, dists, rest_cols, x)
    return _joint[name]


def sum_of_parts(joint, parts, columns, rest_cols, xt):
    """The documented order: the flow blocks in list order, the table, then the Gaussian blocks in list order -- every part
    evaluated on its gathered columns by itself, the Gaussian blocks by the model."""
    import pocomc_amd as pc
    v = None
    for p, c in zip(parts, columns):
        if isinstance(p, pc.FlowPrior):
            part = p.logpdf_device(xt[:, c].contiguous()).cpu().numpy()
            v = part if v is None else v + part
    if joint.rest is not None:
        t = table_logp(joint.rest, xt[:, rest_cols.tolist()].contiguous())
        v = t if v is None else v + t
    x = xt.cpu().numpy()
    blocks = []
    for p, c in zip(parts, columns):
        if isinstance(p, pc.GaussianPrior):
            blk = p.device_block()
            blocks.append((c, blk["mean"], blk["linv_packed"], float(blk["logc"])))
            assert np.array_equal(bits(p.logpdf_device(xt[:, c].contiguous())),
                                  gpm.gauss_block_model(x[:, c], *blocks[-1][1:]).view(np.int64))
    return gpm.gauss_blocks_model(x, blocks, v)


@pytest.mark.parametrize("name", ["flow+gauss+table", "gauss+flow+table", "gauss+table", "gauss+gauss"])
def test_a_joint_prior_is_the_sum_of_its_parts_in_the_documented_order(name):
    import pocomc_amd as pc
    joint, parts, columns, dists, rest_cols, x = joint_case(name)
    n_flow = sum(isinstance(p, pc.FlowPrior) for p in parts)
    assert joint.dim == D9 and joint.blocks == len(parts) and len(joint.flow_priors) == n_flow
    assert isinstance(joint.gaussian_priors, tuple) and len(joint.gaussian_priors) == len(parts) - n_flow
    assert all(g is not p for g in joint.gaussian_priors for p in parts)                    # owned copies
    xt = up(x)
    want = sum_of_parts(joint, parts, columns, rest_cols, xt)
    assert np.isfinite(want).all()
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = joint.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64
            assert np.array_equal(bits(got), want[:n].view(np.int64)), (name, n, other.stride())
    assert np.array_equal(joint.logpdf(x).view(np.int64), want.view(np.int64))
    back = pickle.loads(pickle.dumps(joint))
    assert back.blocks == joint.blocks and back.dim == D9 and np.array_equal(back.bounds, joint.bounds)
    assert len(back.gaussian_priors) == len(joint.gaussian_priors) and len(back.flow_priors) == n_flow
    assert np.array_equal(bits(back.logpdf_device(xt)), want.view(np.int64))
    with pytest.raises(ValueError, match="Gaussian block"):
        joint.step_stage(64)
    # outside any part's support: -inf, never NaN
    y = np.array(x[:70])
    y[3, columns[0][0]] = np.nan
    y[64, columns[-1][-1]] = np.inf
    if dists:
        y[5, rest_cols[0]] = 3.5                                          # beyond the uniform factor
    got = joint.logpdf_device(up(y)).cpu().numpy()
    bad = [3, 64] + ([5] if dists else [])
    keep = np.setdiff1d(np.arange(70), bad)
    assert np.isneginf(got[bad]).all() and np.array_equal(got[keep].view(np.int64), want[:70][keep].view(np.int64))
    # bounds and draws go by list order
    b = joint.bounds
    for p, c in zip(parts, columns):
        assert np.array_equal(b[c], p.bounds)
    torch.manual_seed(2)
    np.random.seed(2)
    r = joint.rvs(50)
    assert r.shape == (50, D9) and np.isfinite(joint.logpdf(r)).all()
    torch.manual_seed(2)
    np.random.seed(2)
    assert np.array_equal(back.rvs(50), r)


def test_the_list_order_of_the_two_kinds_does_not_move_the_value():
    a, _, _, _, _, x = joint_case("flow+gauss+table")
    b = joint_case("gauss+flow+table")[0]
    xt = up(x)
    assert np.array_equal(bits(a.logpdf_device(xt)), bits(b.logpdf_device(xt)))


def test_joint_refusals_with_gaussian_blocks():
    import pocomc_amd as pc
    from scipy.stats import norm
    g3, flow = gauss_of(3, 1), make_flow(3, 3, "affine")[0]
    with pytest.raises(ValueError, match="9 blocks"):
        pc.JointPrior([gauss_of(1, s) for s in range(9)], [[c] for c in range(9)])
    with pytest.raises(ValueError, match="block 1 must be a pocomc_amd.FlowPrior or GaussianPrior"):
        pc.JointPrior([g3, pc.Prior([norm()])], [[0, 1, 2], [3]])
    with pytest.raises(ValueError, match="blocks 0 and 1 overlap"):
        pc.JointPrior([g3, flow], [[0, 1, 2], [2, 3, 4]])
    with pytest.raises(ValueError, match="too large"):
        pc.JointPrior([gauss_of(100, 1), gauss_of(58, 2)], [list(range(100)), list(range(100, 158))])
    eight = pc.JointPrior([gauss_of(1, s) for s in range(8)], [[c] for c in range(8)])       # one column each, the most blocks
    assert eight.blocks == 8 and eight.dim == 8 and eight.flow_priors == ()
    x = np.random.default_rng(0).normal(size=(65, 8))
    blocks = [([c], *[g.device_block()[f] for f in ("mean", "linv_packed")], float(g.device_block()["logc"]))
              for c, g in enumerate(eight.gaussian_priors)]
    assert np.array_equal(bits(eight.logpdf_device(up(x))), gpm.gauss_blocks_model(x, blocks).view(np.int64))


def test_a_joint_prior_of_flow_blocks_alone_is_untouched():
    import pocomc_amd as pc
    a, b = make_flow(3, 3, "affine")[0], make_flow(2, 3, "rqs", seed=6)[0]
    dists = jpm.rest_dists(2)
    joint = pc.JointPrior([a, b], [[4, 0, 2], [6, 1]], pc.Prior(dists, device=True))
    assert joint.blocks == 2 and joint.gaussian_priors == () and joint._gdesc is None and joint._jdesc.D == 0
    rng = np.random.default_rng(4)
    x = np.empty((130, 7))
    x[:, [4, 0, 2]], x[:, [6, 1]], x[:, [3, 5]] = rows_in(bounds_of(3), 130, rng), rows_in(bounds_of(2), 130, rng), \
        jpm.rest_rows(dists, 130, rng)
    xt = up(x)
    got = joint.logpdf_device(xt)
    assert torch.isfinite(got).all() and np.array_equal(bits(got), bits(joint._logpdf_device_blocks(xt)))
    parts = (a.logpdf_device(xt[:, [4, 0, 2]].contiguous()).cpu().numpy()
             + b.logpdf_device(xt[:, [6, 1]].contiguous()).cpu().numpy()) + table_logp(joint.rest, xt[:, [3, 5]].contiguous())
    assert np.array_equal(bits(got), parts.view(np.int64))
    assert "kinds" not in joint.__getstate__()
    assert joint.step_stage(64) is not None


# ------------------------------------------------------------------------------------------------------------------
# 5. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
KW = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)


@pytest.mark.parametrize("which", ["gaussian", "joint"])
def test_the_samplers_two_routes_agree(which):
    import pocomc_amd as pc
    from scipy.stats import norm, uniform
    rng = np.random.default_rng(12)
    if which == "gaussian":
        prior = pc.GaussianPrior(rng.normal(size=4) * 0.3, gpm.random_cov(4, 20.0, rng) * 4.0)
    else:
        prior = pc.JointPrior([pc.GaussianPrior(rng.normal(size=2) * 0.3, gpm.random_cov(2, 20.0, rng) * 4.0)], [[0, 2]],
                              pc.Prior([norm(0.5, 2.0), uniform(-6.0, 12.0)]))
    assert prior.dim == 4

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
    with pytest.raises(ValueError):
        pc.Sampler(prior=prior, likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)
