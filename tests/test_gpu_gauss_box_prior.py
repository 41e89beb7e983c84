"""``pocomc_amd.TruncatedGaussianPrior`` and the truncated Gaussian blocks of ``pocomc_amd.JointPrior`` on the device: one launch
of ``pmc_gauss_box_logpdf`` (``csrc/gauss_prior.hip``, the instance of the blocks' kernel with the box test).

The yardstick is ``tests/gauss_box_model.py`` and the statement is bit for bit, as in ``tests/test_gpu_gauss_prior.py``: every
width class, the 64-row tile's edges, both coalesced layouts and a slice; rows inside the box have the old entry's bits; the
bound itself and the first float beyond it; bad rows; the entry through ctypes; the joint prior as the sum of its parts; the
Sampler's two routes."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import gauss_box_model as gbm
import gauss_prior_model as gpm
import joint_prior_model as jpm
from .test_gauss_box_prior_cpu import entry_refusals
from .test_gpu_flow_prior import bits, bounds_of, gauss_at, make as make_flow, rows_in
from .test_gpu_gauss_prior import Entry, layouts, up
from .test_gpu_joint_prior import table_logp

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 33, 157]
NS = [1, 63, 64, 65, 200]
INF = np.inf
_made = {}


def i64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make(k):
    """``(prior, mean, cov, bounds, 200 rows, the model's values of them, which rows are inside)``, built once per width; the
    fixture splits the rows into two classes of at least 50, with at least 20 inside rows in each of the first two tiles."""
    import pocomc_amd as pc
    if k not in _made:
        mean, cov, b, x = gbm.fixture(k)
        prior = pc.TruncatedGaussianPrior(mean, cov, b)
        blk = prior.device_block()
        want = gbm.gauss_box_model(x, blk["mean"], blk["linv_packed"], float(blk["logc"]), blk["lo"], blk["hi"])
        inside = gbm.in_box(x, b[:, 0], b[:, 1])
        assert inside.sum() >= 50 and (~inside).sum() >= 50, (k, int(inside.sum()))
        assert inside[:64].sum() >= 20 and inside[64:128].sum() >= 20, (k, int(inside[:64].sum()), int(inside[64:128].sum()))
        assert np.isfinite(want[inside]).all() and np.isneginf(want[~inside]).all()
        for a in (want, x, inside):
            a.setflags(write=False)
        _made[k] = (prior, mean, cov, b, x, want, inside)
    return _made[k]


def old_entry(blk, xt):
    """``pmc_gauss_blocks_logpdf`` for the same descriptor: one block on the columns in order, ``logc`` = ``logc_box``."""
    from pocomc_amd import _lib
    n, k = xt.shape
    keep = [up(np.arange(k, dtype=np.int32)), up(blk["mean"]), up(blk["linv_packed"])]
    g = _lib.pmc_gauss_blocks_t(n_blocks=1, D=k)
    g.dim[0], g.logc[0] = k, float(blk["logc"])
    g.cols[0], g.mean[0], g.linv[0] = (t.data_ptr() for t in keep)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().pmc_gauss_blocks_logpdf(C.byref(g), C.c_void_p(xt.data_ptr()), k, 1, n, None, _lib.ptr(out),
                                                   _lib.stream_handle()), "pmc_gauss_blocks_logpdf")
    return out


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel is the model
# ------------------------------------------------------------------------------------------------------------------
def test_the_fixture_splits_the_rows_as_stated():
    """The split of the 200 rows that the fixture's statement gives: (inside, outside) per width."""
    got = {k: (int(make(k)[6].sum()), int((~make(k)[6]).sum())) for k in KS}
    assert got == {1: (134, 66), 2: (130, 70), 5: (128, 72), 33: (96, 104), 157: (102, 98)}, got


@pytest.mark.parametrize("k", KS)
def test_the_kernel_equals_the_model_bit_for_bit(k):
    prior, _, _, _, x, want, inside = make(k)
    xt = up(x)
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = prior.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
            assert np.array_equal(bits(got), i64(want[:n])), (k, n, other.stride())
    assert np.array_equal(i64(prior.logpdf(np.array(x))), i64(want))
    assert prior.logpdf_device(torch.zeros(0, k, dtype=torch.float64, device="cuda")).shape == (0,)
    for bad in (torch.zeros(3, k, device="cuda"), torch.zeros(3, k + 1, dtype=torch.float64, device="cuda"),
                torch.zeros(3, k, dtype=torch.float64), np.zeros((3, k))):
        with pytest.raises(ValueError, match="TruncatedGaussianPrior.logpdf_device"):
            prior.logpdf_device(bad)
    with pytest.raises(ValueError, match="TruncatedGaussianPrior.logpdf"):
        prior.logpdf(np.zeros((3, k + 1)))


@pytest.mark.parametrize("k", KS)
def test_inside_rows_have_the_old_entrys_bits(k):
    prior, _, _, _, x, want, inside = make(k)
    xt = up(x)
    old = old_entry(prior.device_block(), xt).cpu().numpy()
    got = prior.logpdf_device(xt).cpu().numpy()
    assert np.isfinite(old).all()
    assert np.array_equal(i64(got[inside]), i64(old[inside])) and np.isneginf(got[~inside]).all()


@pytest.mark.parametrize("k", KS)
def test_all_infinite_bounds_are_the_gaussian_prior(k):
    import pocomc_amd as pc
    _, mean, cov, _, x, _, _ = make(k)
    free = np.stack([np.full(k, -INF), np.full(k, INF)], axis=1)
    prior, plain = pc.TruncatedGaussianPrior(mean, cov, free), pc.GaussianPrior(mean, cov)
    assert prior.log_mass == 0.0
    y = np.array(x)
    y[5, k // 2], y[70, 0] = np.nan, INF
    for other in layouts(up(y)):
        got, want = prior.logpdf_device(other), plain.logpdf_device(other)
        assert np.array_equal(bits(got), bits(want))
    assert np.isneginf(got.cpu().numpy()[[5, 70]]).all() and torch.isfinite(got).sum() == 198


@pytest.mark.parametrize("k", KS)
def test_a_rows_bits_do_not_depend_on_n_its_place_or_the_layout(k):
    prior, _, _, _, x, want, inside = make(k)
    for src in (int(np.flatnonzero(inside)[5]), int(np.flatnonzero(~inside)[5])):      # a row inside and a row outside
        row = x[src:src + 1]
        alone = bits(prior.logpdf_device(up(row)))
        assert alone[0] == i64(want[src:src + 1])[0]
        y = np.array(x)
        y[0], y[199] = row, row
        for other in layouts(up(y))[:2]:
            got = bits(prior.logpdf_device(other))
            assert got[0] == alone[0] and got[199] == alone[0] and got[src] == alone[0]
            assert np.array_equal(got[1:199], i64(want[1:199]))
            assert np.array_equal(bits(prior.logpdf_device(other[37:])), got[37:])
            assert np.array_equal(bits(prior.logpdf_device(other[64:])), got[64:])


# ------------------------------------------------------------------------------------------------------------------
# 2. the bound itself, bad rows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_the_value_on_a_bound_is_finite_and_the_first_float_beyond_it_is_minus_infinity(k):
    prior, _, _, b, x, want, inside = make(k)
    blk = prior.device_block()
    n = 130
    places = [0, 63, 64, n - 1]
    donor = x[int(np.flatnonzero(inside)[3])]
    for j in gbm.bounded_columns(k):
        for side in (0, 1):
            if not np.isfinite(b[j, side]):
                continue
            beyond = np.nextafter(b[j, side], -INF if side == 0 else INF)
            for value, finite in ((b[j, side], True), (beyond, False)):
                y = np.array(x[:n])
                y[places] = donor
                y[places, j] = value
                model = gbm.gauss_box_model(y, blk["mean"], blk["linv_packed"], float(blk["logc"]), blk["lo"], blk["hi"])
                assert np.isfinite(model[places]).all() if finite else np.isneginf(model[places]).all()
                keep = np.setdiff1d(np.arange(n), places)
                for other in layouts(up(y)):
                    got = prior.logpdf_device(other).cpu().numpy()
                    assert np.array_equal(i64(got), i64(model)), (k, j, side, finite)
                    assert np.isfinite(got[places]).all() if finite else np.isneginf(got[places]).all()
                    assert np.array_equal(i64(got[keep]), i64(want[:n][keep]))
                    assert not np.isnan(got).any() and not np.isposinf(got).any()


HOLES = [0, 63, 64, 129]                 # first row, a tile's last, the next tile's first, the call's last


@pytest.mark.parametrize("k", [1, 5, 33])
def test_bad_rows_are_minus_infinity_and_move_nothing_else(k):
    prior, _, _, b, x, want, inside = make(k)
    blk = prior.device_block()
    n = 130
    good = i64(want[:n])
    bounded = gbm.bounded_columns(k)
    unbounded = [j for j in range(k) if j not in bounded]
    signs = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    columns = [("a bounded column", bounded[-1])] + ([("an unbounded column", unbounded[len(unbounded) // 2])] if unbounded else [])
    for where, j in columns:
        for what, v in {"NaN": np.nan, "+inf": INF, "-inf": -INF, "1e300": 1e300, "-1e300": -1e300,
                        "+-1e300": 1e300 * signs, "1.7e308": 1.7e308}.items():
            y = np.array(x[:n])
            if np.ndim(v) == 0:
                y[HOLES, j] = v                                           # one bad column is enough
            else:
                y[HOLES] = v
            model = gbm.gauss_box_model(y, blk["mean"], blk["linv_packed"], float(blk["logc"]), blk["lo"], blk["hi"])
            assert np.isneginf(model[HOLES]).all(), (where, what)
            keep = np.setdiff1d(np.arange(n), HOLES)
            for other in layouts(up(y)):
                got = prior.logpdf_device(other).cpu().numpy()
                assert np.isneginf(got[HOLES]).all(), (where, what, got[HOLES])
                assert not np.isnan(got).any() and not np.isposinf(got).any(), (where, what)
                assert np.array_equal(i64(got[keep]), good[keep]), (where, what)
                assert np.array_equal(i64(got), i64(model)), (where, what)


# ------------------------------------------------------------------------------------------------------------------
# 3. the entry through ctypes, D = 9
# ------------------------------------------------------------------------------------------------------------------
class BoxEntry(Entry):
    """``tests/test_gpu_gauss_prior.py``'s two blocks on permuted, interleaved columns; block 0 has a box (two-sided on its 1st
    column, one-sided on its 3rd), block 1 a NULL pair."""

    def __init__(self, rest=None):
        from pocomc_amd import _lib
        super().__init__(rest)
        k = len(self.blocks[0][0])
        lo, hi = np.full(k, -INF), np.full(k, INF)
        lo[0], hi[0], lo[2] = -1.2, 1.6, -0.9
        self.lo, self.hi = lo, hi
        self.box_keep = [up(lo), up(hi)]
        self.box = _lib.pmc_gauss_box_t()
        self.box.lo[0], self.box.hi[0] = self.box_keep[0].data_ptr(), self.box_keep[1].data_ptr()
        self.model_blocks = [self.blocks[0] + (lo, hi), self.blocks[1] + (None, None)]

    def call(self, xt, base=None, out=None, strides=None):
        from pocomc_amd import _lib
        n = xt.shape[0] if strides is None else xt.shape[1]
        out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda") if out is None else out
        rs, cs = strides if strides is not None else (xt.shape[1], 1)
        _lib.check(_lib.load().pmc_gauss_box_logpdf(C.byref(self.g), C.byref(self.box), C.c_void_p(xt.data_ptr()), rs, cs, n,
                                                    _lib.ptr(base), _lib.ptr(out), _lib.stream_handle()), "pmc_gauss_box_logpdf")
        return out


def test_two_blocks_one_with_a_box_alone_on_a_base_and_in_place():
    e = BoxEntry()
    cols0 = e.blocks[0][0]
    want = gbm.gauss_box_blocks_model(e.x, e.model_blocks)
    inside = gbm.in_box(e.x[:, cols0], e.lo, e.hi)
    assert inside.sum() >= 50 and (~inside).sum() >= 50
    plain = gpm.gauss_blocks_model(e.x, e.blocks)
    assert np.array_equal(i64(want[inside]), i64(plain[inside])) and np.isneginf(want[~inside]).all()
    xt = up(e.x)
    base = np.random.default_rng(3).normal(size=200) * 10.0
    base[[5, 64]] = -INF
    on_base = gbm.gauss_box_blocks_model(e.x, e.model_blocks, base)
    for n in [1, 63, 64, 65, 200]:
        xc = xt[:n].contiguous()
        assert np.array_equal(bits(e.call(xc)), i64(want[:n])), n
        assert np.array_equal(bits(e.call(xc.t().contiguous(), strides=(1, n))), i64(want[:n])), n
        b = up(base[:n])
        assert np.array_equal(bits(e.call(xc, base=b)), i64(on_base[:n])), n
        assert np.array_equal(bits(b), i64(base[:n]))
        got = e.call(xc, base=b, out=b)                                   # in place
        assert got is b and np.array_equal(bits(b), i64(on_base[:n])), n
    # the block with the NULL pair has no box: its columns may lie anywhere
    y = np.array(e.x)
    y[:, e.blocks[1][0][0]] += 50.0
    got = e.call(up(y)).cpu().numpy()
    assert np.array_equal(i64(got), i64(gbm.gauss_box_blocks_model(y, e.model_blocks))) and np.isfinite(got[inside]).all()


def test_with_a_table_a_row_outside_either_support_is_minus_infinity():
    import pocomc_amd as pc
    from scipy.stats import gamma, uniform
    rest = pc.Prior([uniform(-2.0, 5.0), gamma(0.5, loc=1.0)], device=True)
    e = BoxEntry(rest)
    x = e.x
    cols0 = e.blocks[0][0]
    x[:40, cols0[0]], x[:40, cols0[2]] = 0.2, 0.1                         # the first 40 rows inside the box
    x[9, 3] = 3.5                          # beyond the uniform factor only
    x[11, cols0[0]] = 1.7                  # beyond the box only
    x[13, cols0[2]] = np.nextafter(-0.9, -INF)
    x[15, 6] = np.nan
    xt = up(x)
    table = table_logp(rest, xt[:, [3, 6]].contiguous())
    want = gbm.gauss_box_blocks_model(x, e.model_blocks, table)
    assert np.isneginf(want[[9, 11, 13, 15]]).all() and np.isfinite(np.delete(want[:40], [9, 11, 13, 15])).all()
    for n in [1, 63, 64, 65, 200]:
        assert np.array_equal(bits(e.call(xt[:n].contiguous())), i64(want[:n])), n
        assert np.array_equal(bits(e.call(xt[:n].t().contiguous(), strides=(1, n))), i64(want[:n])), n


def test_the_entry_refuses_and_writes_nothing():
    from pocomc_amd import _lib
    lib = _lib.load()
    e = BoxEntry()
    n = 4
    xt = up(e.x[:n])
    out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    base_t = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    rdev = [up(np.array([1, 1], dtype=np.int32)), up(np.zeros(2)), up(np.ones(2)), up(np.zeros(8)), up(np.array([3, 6], dtype=np.int32)),
            up(np.zeros(4)), up(np.ones(4))]

    def descriptor(dims=(3, 4), D=9, Dr=0):
        g = type(e.g).from_buffer_copy(e.g)
        g.D = D
        for b, k in enumerate(dims):
            g.dim[b] = k
        rest = _lib.pmc_prior_t(family=rdev[0].data_ptr(), loc=rdev[1].data_ptr(), scale=rdev[2].data_ptr(), D=max(Dr, 1),
                                par=rdev[3].data_ptr(), n_extended=1)
        if Dr:
            g.rest, g.rest_cols = C.addressof(rest), rdev[4].data_ptr()
        return g, rest

    def box_of(g):
        box = _lib.pmc_gauss_box_t()
        for b in range(2):
            box.lo[b], box.hi[b] = rdev[5].data_ptr(), rdev[6].data_ptr()
        return box

    def call(g, box, x=True, n=n, rs=9, cs=1, base=False, logp=True):
        return lib.pmc_gauss_box_logpdf(None if g is None else C.byref(g), None if box is None else C.byref(box),
                                        _lib.ptr(xt) if x else None, rs, cs, n, _lib.ptr(base_t) if base else None,
                                        _lib.ptr(out) if logp else None, _lib.stream_handle())
    entry_refusals(call, lib, descriptor, box_of)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (base_t == 7.0).all()
    assert lib.pmc_gauss_box_logpdf(C.byref(e.g), C.byref(e.box), None, 9, 1, 0, None, None, _lib.stream_handle()) == 0


# ------------------------------------------------------------------------------------------------------------------
# 4. truncated blocks in a JointPrior, D = 9
# ------------------------------------------------------------------------------------------------------------------
D9 = 9


def gauss_of(k, seed):
    import pocomc_amd as pc
    rng = np.random.default_rng(seed)
    mean = rng.normal(size=k)
    return pc.GaussianPrior(mean, gpm.random_cov(k, 50.0, rng) * 1.5)


def truncated_of(k, seed):
    """A box of 1.5 sd below on the first column and 1.2 sd either way on the last (k = 1: both on the one column)."""
    import pocomc_amd as pc
    g = gauss_of(k, seed)
    sd = np.sqrt(np.diag(g.cov))
    b = np.stack([np.full(k, -INF), np.full(k, INF)], axis=1)
    b[0, 0] = g.mean[0] - 1.5 * sd[0]
    b[k - 1] = max(b[k - 1, 0], g.mean[k - 1] - 1.2 * sd[k - 1]), g.mean[k - 1] + 1.2 * sd[k - 1]
    return pc.TruncatedGaussianPrior(g.mean, g.cov, b)


_joint = {}


def joint_case(name):
    """``(joint, blocks in list order, columns, dists, rest_cols, rows)`` of a case, built once."""
    import pocomc_amd as pc
    if name in _joint:
        return _joint[name]
    rng = np.random.default_rng(len(name))
    if name == "flow+truncated":
        parts, columns, dists = [make_flow(3, 3, "affine")[0], truncated_of(3, 1)], [[4, 0, 2], [1, 5, 6]], jpm.rest_dists(3)
    elif name == "truncated+table":
        parts, columns, dists = [truncated_of(3, 1)], [[1, 5, 6]], jpm.rest_dists(6)
    elif name == "gaussian+truncated":
        parts, columns, dists = [gauss_of(4, 2), truncated_of(5, 3)], [[8, 0, 3, 5], [2, 7, 1, 6, 4]], []
    else:
        assert name == "truncated+truncated"
        parts, columns, dists = [truncated_of(4, 2), truncated_of(5, 3)], [[8, 0, 3, 5], [2, 7, 1, 6, 4]], []
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
    """The documented order: the flow blocks in list order, the table, then ``+ g_b`` for every Gaussian block of either kind
    in list order, ``g_b`` the block's own ``logpdf_device`` on its gathered columns (which is the model's value)."""
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
    with np.errstate(all="ignore"):
        for p, c in zip(parts, columns):
            if isinstance(p, pc.GaussianPrior):
                g = p.logpdf_device(xt[:, c].contiguous()).cpu().numpy()
                blk = p.device_block()
                if isinstance(p, pc.TruncatedGaussianPrior):
                    model = gbm.gauss_box_model(x[:, c], blk["mean"], blk["linv_packed"], float(blk["logc"]), blk["lo"], blk["hi"])
                else:
                    model = gpm.gauss_block_model(x[:, c], blk["mean"], blk["linv_packed"], float(blk["logc"]))
                assert np.array_equal(i64(g), i64(model))
                v = g if v is None else v + g
    return np.where(np.isfinite(v), v, -INF)


@pytest.mark.parametrize("name", ["flow+truncated", "truncated+table", "gaussian+truncated", "truncated+truncated"])
def test_a_joint_prior_is_the_sum_of_its_parts_in_the_documented_order(name):
    import pocomc_amd as pc
    joint, parts, columns, dists, rest_cols, x = joint_case(name)
    n_flow = sum(isinstance(p, pc.FlowPrior) for p in parts)
    assert joint.dim == D9 and joint.blocks == len(parts) and len(joint.flow_priors) == n_flow
    assert len(joint.gaussian_priors) == len(parts) - n_flow and joint._gbox is not None
    assert [type(g) for g in joint.gaussian_priors] == [type(p) for p in parts if isinstance(p, pc.GaussianPrior)]
    assert all(g is not p for g in joint.gaussian_priors for p in parts)                    # owned copies
    xt = up(x)
    want = sum_of_parts(joint, parts, columns, rest_cols, xt)
    inside = np.isfinite(want)
    assert inside.sum() >= 40 and (~inside).sum() >= 40 and np.isneginf(want[~inside]).all(), (name, int(inside.sum()))
    for n in NS:
        for other in layouts(xt[:n].contiguous()):
            got = joint.logpdf_device(other)
            assert got.shape == (n,) and got.dtype == torch.float64
            assert np.array_equal(bits(got), i64(want[:n])), (name, n, other.stride())
    assert np.array_equal(i64(joint.logpdf(x)), i64(want))
    # the whole row is -inf as soon as any block's box is violated, and only then
    ok = np.ones(len(x), dtype=bool)
    for p, c in zip(parts, columns):
        if isinstance(p, pc.TruncatedGaussianPrior):
            ok &= gbm.in_box(x[:, c], p.bounds[:, 0], p.bounds[:, 1])
    assert np.array_equal(ok, inside)
    # bounds are merged by position
    b = joint.bounds
    for p, c in zip(parts, columns):
        assert np.array_equal(b[c], p.bounds)
    if dists:
        assert np.array_equal(b[rest_cols], joint.rest.bounds)
    # pickling
    st = joint.__getstate__()
    assert st["kinds"] == ["flow" if isinstance(p, pc.FlowPrior) else "gauss_box" if isinstance(p, pc.TruncatedGaussianPrior)
                           else "gauss" for p in parts]
    back = pickle.loads(pickle.dumps(joint))
    assert back.blocks == joint.blocks and back.dim == D9 and np.array_equal(back.bounds, joint.bounds)
    assert len(back.gaussian_priors) == len(joint.gaussian_priors) and len(back.flow_priors) == n_flow
    assert np.array_equal(bits(back.logpdf_device(xt)), i64(want))
    with pytest.raises(ValueError, match="Gaussian block"):
        joint.step_stage(64)
    # draws stay inside every part's support
    torch.manual_seed(2)
    np.random.seed(2)
    r = joint.rvs(50)
    assert r.shape == (50, D9) and np.isfinite(joint.logpdf(r)).all()
    assert ((r >= b[:, 0]) & (r <= b[:, 1])).all()
    torch.manual_seed(2)
    np.random.seed(2)
    assert np.array_equal(back.rvs(50), r)


def test_a_joint_prior_without_a_truncated_block_calls_the_old_entry_as_before():
    import pocomc_amd as pc
    from pocomc_amd import _lib
    a, b = gauss_of(4, 2), gauss_of(5, 3)
    columns = [[8, 0, 3, 5], [2, 7, 1, 6, 4]]
    joint = pc.JointPrior([a, b], columns)
    assert joint._gbox is None and joint.__getstate__()["kinds"] == ["gauss", "gauss"]
    rng = np.random.default_rng(1)
    x = np.empty((130, D9))
    x[:, columns[0]], x[:, columns[1]] = gpm.draws(a.mean, a.cov, 130, 1.0, rng), gpm.draws(b.mean, b.cov, 130, 1.0, rng)
    xt = up(x)
    keep = []
    g = _lib.pmc_gauss_blocks_t(n_blocks=2, D=D9)
    for i, (p, c) in enumerate(zip((a, b), columns)):
        blk = p.device_block()
        t = [up(np.array(c, dtype=np.int32)), up(blk["mean"]), up(blk["linv_packed"])]
        keep.append(t)
        g.dim[i], g.logc[i] = p.dim, float(blk["logc"])
        g.cols[i], g.mean[i], g.linv[i] = (v.data_ptr() for v in t)
    out = torch.empty(130, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().pmc_gauss_blocks_logpdf(C.byref(g), C.c_void_p(xt.data_ptr()), D9, 1, 130, None, _lib.ptr(out),
                                                   _lib.stream_handle()), "pmc_gauss_blocks_logpdf")
    got = joint.logpdf_device(xt)
    assert torch.isfinite(got).all() and np.array_equal(bits(got), bits(out))
    # a state pickled before the truncated kind existed knows "flow" and "gauss" only, and still loads
    st = joint.__getstate__()
    assert set(st) == {"flow_priors", "columns", "rest", "kinds"} and set(st["kinds"]) == {"gauss"}
    old = pc.JointPrior.__new__(pc.JointPrior)
    old.__setstate__(st)
    assert np.array_equal(bits(old.logpdf_device(xt)), bits(out))


# ------------------------------------------------------------------------------------------------------------------
# 5. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
KW = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)


@pytest.mark.parametrize("which", ["truncated", "joint"])
def test_the_samplers_two_routes_agree(which):
    import pocomc_amd as pc
    from scipy.stats import norm, uniform
    rng = np.random.default_rng(12)
    if which == "truncated":
        mean, cov = rng.normal(size=4) * 0.3, gpm.random_cov(4, 20.0, rng) * 4.0
        b = np.stack([np.full(4, -INF), np.full(4, INF)], axis=1)
        b[1], b[3] = (0.0, INF), (-1.0, 2.5)
        prior = pc.TruncatedGaussianPrior(mean, cov, b)
    else:
        mean, cov = rng.normal(size=2) * 0.3, gpm.random_cov(2, 20.0, rng) * 4.0
        block = pc.TruncatedGaussianPrior(mean, cov, [[0.0, INF], [-1.0, 2.5]])
        prior = pc.JointPrior([block], [[0, 2]], pc.Prior([norm(0.5, 2.0), uniform(-6.0, 12.0)]))
        b = prior.bounds
        assert np.array_equal(b[[0, 2]], block.bounds) and np.array_equal(b[3], [-6.0, 6.0])
    assert prior.dim == 4

    def run(on_device):
        s = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=on_device, **KW)
        s.run(n_total=256, n_evidence=0, progress=False)
        return s
    dev, host = run(True), run(False)
    assert dev.device_prior is True and host.device_prior is False
    for a, c in zip(dev.posterior(), host.posterior()):
        assert np.array_equal(np.asarray(a), np.asarray(c))
    assert dev.evidence() == host.evidence() and dev.calls == host.calls
    rd = dev.results
    assert np.isfinite(np.asarray(rd["logp"])).all() and np.asarray(rd["beta"])[-1] == 1.0
    xs = np.asarray(rd["x"]).reshape(-1, 4)
    assert np.array_equal(prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    assert ((xs >= b[:, 0]) & (xs <= b[:, 1])).all()
    with pytest.raises(ValueError):
        pc.Sampler(prior=prior, likelihood=lambda x: -0.5 * np.sum(x ** 2, axis=1), vectorize=True, step_prior=True)
