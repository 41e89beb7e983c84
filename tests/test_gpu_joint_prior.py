"""``pocomc_amd.JointPrior``: a flow prior on some columns of x and scipy factors on the others, evaluated on the device by
``pmc_joint_prior_pre`` -> the flow's forward kernel -> ``pmc_joint_prior_post`` (``csrc/joint_prior.hip``); and the marginal
fit behind it, ``FlowPrior.from_samples`` / ``FlowPrior.from_sampler(columns=...)``.

The first yardstick is the pair of entries the kernel fuses: ``pmc_flow_prior_pre`` on the gathered flow columns and
``pmc_prior_logpdf`` on the gathered rest columns, bit for bit.  The second is the restatement of
``tests/joint_prior_model.py`` (the oracle's scaler and flow, scipy's own ``logpdf``), held to the tolerances of
``tests/test_gpu_flow_prior.py``.  Layout, row position, bad rows, ownership and the Sampler's two routes are bit-for-bit
statements."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import cases
import flow_prior_model as fpm
import joint_prior_model as jpm
from oracle.maf import OracleMAF
from parity import close_rel, TOL
from pocomc_amd.maf_spec import MAFSpec
from .test_gpu_flow import NSF_LADJ
from .test_gpu_flow_prior import bits, bounds_of, gauss_at, make, pre, rows_in

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, "affine"), (3, 4, "rqs"), (17, 16, "affine")]
NS = [1, 63, 64, 65, 200]


def build(Df, Dr, uni, T=3, dists=None, columns=None):
    """``(joint, flow prior, rest, oracle scaler, oracle flow, dists, flow_cols, rest_cols)``: the flow prior of
    ``test_gpu_flow_prior.make`` on columns that are interleaved with the rest's and not sorted."""
    import pocomc_amd as pc
    prior, oscaler, maf, _, _ = make(Df, T, uni)
    dists = jpm.rest_dists(Dr) if dists is None else dists
    columns = jpm.interleaved_columns(Df, len(dists)) if columns is None else columns
    rest = pc.Prior(dists, device=True)
    joint = pc.JointPrior(prior, columns, rest)
    flow_cols, rest_cols = jpm.layout(columns, Df + len(dists))
    assert not np.array_equal(flow_cols, np.sort(flow_cols)) and rest_cols.min() < flow_cols.max()
    return joint, prior, rest, oscaler, maf, dists, flow_cols, rest_cols


def rows(Df, dists, flow_cols, rest_cols, n, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, Df + len(dists)))
    x[:, flow_cols] = rows_in(bounds_of(Df), n, rng)
    x[:, rest_cols] = jpm.rest_rows(dists, n, rng)
    return x


def jpre(joint, xt):
    """``pmc_joint_prior_pre`` alone on a C-contiguous tensor: ``(u32, ldj, rest_logp, inside)`` as numpy."""
    from pocomc_amd import _lib
    n, D = xt.shape
    Df = joint.flow_prior.dim
    u32 = torch.empty(n, Df, dtype=torch.float32, device=xt.device)
    ldj = torch.empty(n, dtype=torch.float64, device=xt.device)
    rest_logp = torch.empty(n, dtype=torch.float64, device=xt.device)
    inside = torch.empty(n, dtype=torch.int32, device=xt.device)
    _lib.check(_lib.load().pmc_joint_prior_pre(C.byref(joint.flow_prior._sdesc), _lib.ptr(joint._dev["flow_cols"]),
                                               C.byref(joint._rdesc), _lib.ptr(joint._dev["rest_cols"]), _lib.ptr(xt), D, 1, n,
                                               _lib.ptr(u32), _lib.ptr(ldj), _lib.ptr(rest_logp), _lib.ptr(inside),
                                               _lib.stream_handle()), "pmc_joint_prior_pre")
    return u32.cpu().numpy(), ldj.cpu().numpy(), rest_logp.cpu().numpy(), inside.cpu().numpy()


def table_logp(rest, xr):
    """``pmc_prior_logpdf`` on a C-contiguous ``(n, Dr)`` tensor, every row marked finite."""
    from pocomc_amd import _lib
    n = xr.shape[0]
    fin = torch.ones(n, dtype=torch.int32, device=xr.device)
    out = torch.empty(n, dtype=torch.float64, device=xr.device)
    _lib.check(_lib.load().pmc_prior_logpdf(C.byref(rest.device_descriptor()), _lib.ptr(xr), _lib.ptr(fin), _lib.ptr(out), n,
                                            _lib.stream_handle()), "pmc_prior_logpdf")
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# 1. the parts' bits
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Df,Dr,uni", SHAPES)
def test_the_fused_kernel_gives_the_bits_of_its_two_parts(Df, Dr, uni):
    joint, prior, rest, _, _, dists, flow_cols, rest_cols = build(Df, Dr, uni)
    xt = torch.from_numpy(rows(Df, dists, flow_cols, rest_cols, max(NS), Df)).cuda()
    fc, rc = torch.from_numpy(flow_cols).cuda(), torch.from_numpy(rest_cols).cuda()
    for n in NS:
        x = xt[:n].contiguous()
        xf, xr = x[:, fc].contiguous(), x[:, rc].contiguous()
        u32, ldj, rest_logp, inside = jpre(joint, x)
        fu32, fldj, finside = pre(prior, xf)
        assert inside.all() and finside.all()
        assert np.array_equal(u32.view(np.int32), fu32.view(np.int32)), n
        assert np.array_equal(ldj.view(np.int64), fldj.view(np.int64)), n
        want_rest = table_logp(rest, xr)
        assert np.isfinite(want_rest).all()
        assert np.array_equal(rest_logp.view(np.int64), want_rest.view(np.int64)), n
        got = joint.logpdf_device(x)
        assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
        want = prior.logpdf_device(xf).cpu().numpy() + want_rest
        assert np.isfinite(want).all() and np.array_equal(bits(got), want.view(np.int64)), n


# ------------------------------------------------------------------------------------------------------------------
# 2. values against the model
# ------------------------------------------------------------------------------------------------------------------
def against_the_model(joint, oscaler, maf, dists, flow_cols, x, tol, what):
    """``close_rel`` of ``joint.logpdf_device(x)`` against the model, measured against the size of the sum's terms: those of
    the flow's log-determinant and the scaler's (as ``test_gpu_flow_prior`` builds them) plus the rest terms' absolute values."""
    want, _, terms = jpm.joint_prior_model(oscaler, maf, dists, flow_cols, x)
    assert np.isfinite(want).all()
    xf = x[:, flow_cols]
    want_ldj = fpm.flow_prior_model(oscaler, maf, xf)[1]
    cancel = maf.ladj_abs_terms(oscaler.forward(xf).astype(np.float32)) + np.abs(want_ldj) + np.abs(terms).sum(axis=1)
    got = joint.logpdf_device(torch.from_numpy(x).cuda())
    worst = close_rel(got.cpu().numpy(), want, 1.0, f"{what} measured", cancel=cancel)
    print(f"{what}: log p max relative error {worst:.3e} (bound {tol:g})")
    close_rel(got.cpu().numpy(), want, tol, what, cancel=cancel)
    return got


@pytest.mark.parametrize("Df,Dr,uni", SHAPES)
def test_values_match_the_model(Df, Dr, uni):
    """200 rows (several blocks and a partial one).  Measured on the MI355X, relative to the size of the sum's terms: 1.8e-7
    (2 + 1, affine), 8.1e-7 (3 + 4, spline), 4.5e-7 (17 + 16, affine)."""
    joint, _, _, oscaler, maf, dists, flow_cols, rest_cols = build(Df, Dr, uni)
    x = rows(Df, dists, flow_cols, rest_cols, max(NS), Df)
    tol = TOL if uni == "affine" else NSF_LADJ
    against_the_model(joint, oscaler, maf, dists, flow_cols, x, tol, f"joint prior log p ({Df} + {Dr} {uni})")


# ------------------------------------------------------------------------------------------------------------------
# 3. the widest priors, and what the entries refuse
# ------------------------------------------------------------------------------------------------------------------
def wide(Df, Dr):
    import pocomc_amd as pc
    bounds = bounds_of(Df)
    spec = MAFSpec(Df, 2, 160)
    flat = cases.flow_params(spec, 5)
    flow = pc.Flow(Df, spec)
    flow.set_params(flat)
    train = rows_in(bounds, 500, np.random.default_rng(11))
    scaler = pc.Reparameterize(Df, bounds=bounds)
    scaler.fit(train)
    dists = jpm.rest_dists(Dr)
    columns = jpm.interleaved_columns(Df, Dr)
    joint = pc.JointPrior(pc.FlowPrior(flow, scaler), columns, pc.Prior(dists, device=True))
    return joint, fpm.oracle_scaler(bounds, "probit", train), OracleMAF(spec, flat), dists, columns


@pytest.mark.parametrize("Df,Dr", [(2, 155), (156, 1)])
def test_the_widest_priors_match_the_model(Df, Dr):
    """D = 157 both ways: the tile takes up to 121,204 bytes of LDS (beyond the 48 KiB a launch gets without asking).  65 rows:
    a full block and a row.  Measured on the MI355X: 1.3e-7 (2 + 155), 8.7e-8 (156 + 1)."""
    n = 65
    joint, oscaler, maf, dists, columns = wide(Df, Dr)
    assert joint.dim == 157
    flow_cols, rest_cols = jpm.layout(columns, 157)
    x = rows(Df, dists, flow_cols, rest_cols, n, Df)
    got = against_the_model(joint, oscaler, maf, dists, flow_cols, x, TOL, f"joint prior log p ({Df} + {Dr})")
    xt = torch.from_numpy(x).cuda()
    assert np.array_equal(bits(joint.logpdf_device(xt.t().contiguous().t())), bits(got))


def test_refusals():
    import pocomc_amd as pc
    from pocomc_amd import _lib
    from scipy.stats import gamma, norm, uniform
    lib = _lib.load()
    joint, prior, rest, _, _, dists, flow_cols, rest_cols = build(3, 4, "affine")
    # the class
    with pytest.raises(ValueError, match=r"Prior\(dists, device=True\)"):
        pc.JointPrior(prior, flow_cols.tolist(), pc.Prior([gamma(2.0)] * 4))
    with pytest.raises(ValueError, match=r"Prior\(dists, device=True\)"):
        pc.JointPrior(prior, flow_cols.tolist(), pc.Prior([norm()] * 4, device=False))
    with pytest.raises(ValueError, match="at least one factor"):
        pc.JointPrior(prior, [0, 1, 2], pc.Prior([]))
    with pytest.raises(ValueError, match="FlowPrior"):
        pc.JointPrior(rest, flow_cols.tolist(), rest)
    with pytest.raises(ValueError, match="pocomc_amd.Prior"):
        pc.JointPrior(prior, flow_cols.tolist(), prior)
    with pytest.raises(ValueError, match="distinct"):
        pc.JointPrior(prior, [0, 0, 1], rest)
    with pytest.raises(ValueError, match="columns for"):
        pc.JointPrior(prior, [0, 1], rest)
    two = make(2, 2, "affine")[0]
    W = pc.JointPrior.MAX_DIM + 1
    assert W == 158
    many = pc.Prior([uniform(-1.0, 2.0)] * (W - 2))
    with pytest.raises(ValueError, match="too large"):
        pc.JointPrior(two, [0, 1], many)
    assert not hasattr(joint, "device_descriptor")
    # the device function's own contract
    for bad in (torch.zeros(3, 7, device="cuda"), torch.zeros(3, 6, dtype=torch.float64, device="cuda"),
                torch.zeros(3, 7, dtype=torch.float64), np.zeros((3, 7))):
        with pytest.raises(ValueError):
            joint.logpdf_device(bad)
    assert joint.logpdf_device(torch.zeros(0, 7, dtype=torch.float64, device="cuda")).shape == (0,)

    # the entry: nothing is launched or written, and every refusal has its own text
    n = 4
    xt = torch.zeros(n, W, dtype=torch.float64, device="cuda")
    u32 = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    outs = [torch.full((n,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    ins = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    cols = torch.arange(W, dtype=torch.int32, device="cuda")
    st = _lib.stream_handle()

    def refused(text, s=None, r=None, x=xt, count=n, fcols=cols, rcols=cols, out_u=u32, stride=W):
        s = joint.flow_prior._sdesc if s is None else s
        r = joint._rdesc if r is None else r
        rc = lib.pmc_joint_prior_pre(None if s is False else C.byref(s), _lib.ptr(fcols), None if r is False else C.byref(r),
                                     _lib.ptr(rcols), _lib.ptr(x), stride, 1, count, _lib.ptr(out_u), _lib.ptr(outs[0]),
                                     _lib.ptr(outs[1]), _lib.ptr(ins), st)
        assert rc != 0 and text in lib.pmc_last_error(), (text, rc, lib.pmc_last_error())

    def copy_of(desc, **fields):
        c = type(desc).from_buffer_copy(desc)
        for k, v in fields.items():
            setattr(c, k, v)
        return c
    many_desc = many.device_descriptor()
    refused(b"n_dim too large", s=two._sdesc, r=many_desc)                                 # 2 + 156 = 158
    refused(b"bad scaler descriptor", s=False)
    refused(b"bad scaler descriptor", fcols=None)
    refused(b"bad prior descriptor", r=False)
    refused(b"bad prior descriptor", rcols=None)
    refused(b"bad prior descriptor", r=copy_of(joint._rdesc, loc=None))
    one = pc.Reparameterize(1, bounds=np.array([[-1.0, 1.0]]))
    one.fit(np.random.default_rng(0).uniform(-0.9, 0.9, size=(64, 1)))
    refused(b"at least 2 columns", s=one.device_descriptor())
    refused(b"at least 1 factor", r=copy_of(joint._rdesc, D=0))
    assert joint._rdesc.n_extended > 0
    refused(b"parameter table", r=copy_of(joint._rdesc, par=None))
    refused(b"needs mu and sigma", s=copy_of(joint.flow_prior._sdesc, mu=None))
    refused(b"bad argument", x=None)
    refused(b"bad argument", out_u=None)
    refused(b"bad argument", count=-1)
    refused(b"bad argument", stride=-1)
    refused(b"too many rows", count=64 * 2 ** 31)
    post = lambda *a: lib.pmc_joint_prior_post(*a)
    lp32 = torch.zeros(n, dtype=torch.float32, device="cuda")
    assert post(None, _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(ins), _lib.ptr(outs[0]), n, st) != 0
    assert b"pmc_joint_prior_post: bad argument" in lib.pmc_last_error()
    assert post(_lib.ptr(lp32), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(ins), _lib.ptr(outs[0]), 256 * 2 ** 31, st) != 0
    assert b"pmc_joint_prior_post: too many rows" in lib.pmc_last_error()
    # n == 0 is no error, and reads nothing
    assert lib.pmc_joint_prior_pre(C.byref(joint.flow_prior._sdesc), _lib.ptr(cols), C.byref(joint._rdesc), _lib.ptr(cols),
                                   None, 7, 1, 0, None, None, None, None, st) == 0
    assert post(None, None, None, None, None, 0, st) == 0
    torch.cuda.synchronize()
    assert (u32 == 7.0).all() and (outs[0] == 7.0).all() and (outs[1] == 7.0).all() and (ins == 7).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. layouts and row position
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Df,Dr,uni", [(3, 4, "rqs"), (17, 16, "affine")])
@pytest.mark.parametrize("n", [1, 65, 200])
def test_every_layout_gives_the_same_bits(Df, Dr, uni, n):
    joint, _, _, _, _, dists, flow_cols, rest_cols = build(Df, Dr, uni)
    D = Df + Dr
    x = torch.from_numpy(rows(Df, dists, flow_cols, rest_cols, n, n)).cuda()
    colmajor = x.t().contiguous().t()
    wide_ = torch.zeros(n, 2 * D + 3, dtype=torch.float64, device="cuda")
    wide_[:, 1:2 * D + 1:2] = x
    sliced = wide_[:, 1:2 * D + 1:2]
    assert x.is_contiguous() and (n == 1 or colmajor.stride() == (1, n)) and torch.equal(sliced, x)
    a = joint.logpdf_device(x)
    assert torch.isfinite(a).all()
    for other in (colmajor, sliced, x):
        assert np.array_equal(bits(joint.logpdf_device(other)), bits(a))
    # ... and a row does not depend on its place in the call or on n
    if n > 64:
        assert np.array_equal(bits(joint.logpdf_device(x[37:])), bits(a[37:]))
        assert np.array_equal(bits(joint.logpdf_device(colmajor[64:])), bits(a[64:]))
    assert np.array_equal(joint.logpdf(x.cpu().numpy()).view(np.int64), bits(a))


# ------------------------------------------------------------------------------------------------------------------
# 5. bad rows
# ------------------------------------------------------------------------------------------------------------------
HOLES = [0, 63, 64, 129]                 # first row, a block's last, the next block's first, the call's last


def test_bad_rows_are_minus_infinity_and_move_nothing_else():
    """130 rows, Df = 5 (feature 0 two-sided on (-1, 2), 1 bounded below at 0.5, 2 bounded above at 3, 3 unbounded), the rest
    uniform on [-2, 3], norm, gamma(2.5, loc=-1), ..., and a gamma(0.5, loc=1) whose logpdf is +inf at 1.  Every kind of bad
    row at every one of HOLES, then one of each kind in one call: exactly -inf there, every other row the bits of the call
    without bad rows, in both layouts.  ``inside`` is 0 for what the flow block and the finiteness test refuse and stays 1
    where only a factor's support or pole speaks."""
    from scipy.stats import gamma
    Df, n = 5, 130
    dists = jpm.rest_dists(5) + [gamma(0.5, loc=1.0)]
    joint, _, _, _, _, _, fc, rc = build(Df, len(dists), "rqs", dists=dists)
    x = rows(Df, dists, fc, rc, n, 3)
    good = bits(joint.logpdf_device(torch.from_numpy(x).cuda()))
    assert np.isfinite(good.view(np.float64)).all()
    # what: (column, value, inside)
    kinds = {"NaN in a flow column": (fc[3], np.nan, 0), "+inf in a flow column": (fc[1], np.inf, 0),
             "-inf in a flow column": (fc[3], -np.inf, 0), "NaN in a rest column": (rc[1], np.nan, 0),
             "+inf in a rest column": (rc[1], np.inf, 0), "-inf in a rest column": (rc[4], -np.inf, 0),
             "on the lower bound": (fc[0], -1.0, 0), "on the upper bound": (fc[0], 2.0, 0),
             "on a bound below": (fc[1], 0.5, 0), "on a bound above": (fc[2], 3.0, 0),
             "beyond the uniform factor": (rc[0], 3.5, 1), "below the gamma factor": (rc[2], -1.5, 1),
             "the gamma(0.5) pole": (rc[5], 1.0, 1)}

    def check(y, bad, what, inside_want):
        keep = np.setdiff1d(np.arange(n), bad)
        for yt in (torch.from_numpy(y).cuda(), torch.from_numpy(y).cuda().t().contiguous().t()):
            got = joint.logpdf_device(yt).cpu().numpy()
            assert np.isneginf(got[bad]).all(), (what, got[bad])
            assert not np.isnan(got).any() and not np.isposinf(got).any(), what
            assert np.array_equal(got[keep].view(np.int64), good[keep]), what
        u32, ldj, rest_logp, ins = jpre(joint, torch.from_numpy(y).cuda())
        assert np.array_equal(ins[bad], inside_want) and ins[keep].all(), (what, ins[bad])
        out = np.asarray(bad)[np.asarray(inside_want) == 0]
        assert not u32[out].any() and np.isfinite(u32).all() and np.isneginf(rest_logp[out]).all(), what
        assert np.isfinite(rest_logp[keep]).all(), what
    for what, (j, v, ins) in kinds.items():
        y = x.copy()
        y[HOLES, j] = v
        check(y, HOLES, what, [ins] * len(HOLES))
    y = x.copy()
    bad = HOLES + [100, 65, 1, 2, 30, 62, 66, 127, 128]
    assert len(bad) == len(kinds)
    for r, (j, v, _) in zip(bad, kinds.values()):
        y[r, j] = v
    check(y, bad, "one of each", [k[2] for k in kinds.values()])
    # the pole is +inf in the table's own sum; the join maps it
    y = x.copy()
    y[7, rc[5]] = 1.0
    assert np.isposinf(jpre(joint, torch.from_numpy(y).cuda())[2][7])


# ------------------------------------------------------------------------------------------------------------------
# 6. bounds, dim, pickling, ownership, rvs
# ------------------------------------------------------------------------------------------------------------------
def test_bounds_dim_pickling_ownership_and_rvs():
    import pocomc_amd as pc
    Df, Dr = 5, 6
    joint, prior, rest, _, _, dists, fc, rc = build(Df, Dr, "rqs")
    assert joint.dim == Df + Dr
    b = joint.bounds
    assert b.shape == (Df + Dr, 2) and np.array_equal(b[fc], prior.bounds) and np.array_equal(b[rc], rest.bounds)
    x = torch.from_numpy(rows(Df, dists, fc, rc, 100, 1)).cuda()
    a = bits(joint.logpdf_device(x))
    back = pickle.loads(pickle.dumps(joint))
    assert isinstance(back, pc.JointPrior) and back.dim == joint.dim and np.array_equal(back.bounds, b)
    assert np.array_equal(bits(back.logpdf_device(x)), a)
    # the source flow prior's flow changes: the source moves, the joint prior does not
    before = bits(prior.logpdf_device(x[:, torch.from_numpy(fc).cuda()].contiguous()))
    prior.flow.set_params(cases.flow_params(MAFSpec(Df, 3, univariate="rqs"), 9))
    assert not np.array_equal(bits(prior.logpdf_device(x[:, torch.from_numpy(fc).cuda()].contiguous())), before)
    assert np.array_equal(bits(joint.logpdf_device(x)), a)
    rest.dists[1] = dists[0]
    assert np.array_equal(bits(joint.logpdf_device(x)), a) and np.array_equal(bits(back.logpdf_device(x)), a)
    # draws
    torch.manual_seed(3)
    np.random.seed(3)
    r = joint.rvs(300)
    assert r.shape == (300, Df + Dr) and r.dtype == np.float64
    assert (r[:, fc] > b[fc, 0]).all() and (r[:, fc] < b[fc, 1]).all()
    assert (r[:, rc] >= b[rc, 0]).all() and (r[:, rc] <= b[rc, 1]).all()
    assert np.isfinite(joint.logpdf(r)).all()
    assert joint.rvs(1).shape == (1, Df + Dr)


# ------------------------------------------------------------------------------------------------------------------
# 7. the marginal fit
# ------------------------------------------------------------------------------------------------------------------
BOX = np.array([[-5.0, 5.0], [-6.0, 4.0]])
CENTRE, COV = np.array([1.0, -1.5]), np.array([[1.0, 0.8], [0.8, 1.0]])


def weighted_rows(n, seed):
    """A broad proposal (uniform on most of BOX) weighted to a correlated Gaussian: ``(rows, weights)``."""
    rng = np.random.default_rng(seed)
    x = BOX[:, 0] + (BOX[:, 1] - BOX[:, 0]) * rng.uniform(0.05, 0.95, size=(n, 2))
    d = x - CENTRE
    return x, np.exp(-0.5 * np.einsum("ni,ij,nj->n", d, np.linalg.inv(COV), d))


def test_from_samples_fits_the_weighted_density():
    """Measured on the MI355X: mu and sigma 2.2e-16 from the oracle's moments; weighted mean log p of the held-out rows -2.43
    after the fit against -6.10 with the untrained flow."""
    import pocomc_amd as pc
    x, w = weighted_rows(2000, 0)
    torch.manual_seed(0)
    prior = pc.FlowPrior.from_samples(x, w, bounds=BOX, train_config={"epochs": 200})
    assert isinstance(prior, pc.FlowPrior) and prior.dim == 2 and np.array_equal(prior.bounds, BOX)
    assert prior.flow.spec.univariate == "rqs" and prior.flow.spec.n_transforms == 6 and prior.scaler.transform == "probit"
    # the scaler: the weighted moments of the oracle's unscaled transform
    t = fpm.oracle_scaler(BOX, "probit")._forward(x)
    wn = w / w.sum()
    mu = (wn[:, None] * t).sum(axis=0)
    sigma = np.sqrt((wn[:, None] * (t - mu) ** 2).sum(axis=0))
    err = max(np.abs(prior.scaler.mu / mu - 1.0).max(), np.abs(prior.scaler.sigma / sigma - 1.0).max())
    print(f"from_samples: mu, sigma max relative error {err:.3e} (bound 1e-12)")
    assert err <= 1e-12
    # the fit: held-out rows are more probable than under the same scaler with an untrained flow
    y, wy = weighted_rows(500, 1)
    untrained = pc.FlowPrior(pc.Flow(2, "nsf6", seed=0), prior.scaler)
    lp, lp0 = prior.logpdf(y), untrained.logpdf(y)
    assert np.isfinite(lp).all() and np.isfinite(lp0).all()
    fitted, base = float(np.sum(wy * lp) / wy.sum()), float(np.sum(wy * lp0) / wy.sum())
    print(f"from_samples: weighted mean log p on 500 held-out rows {fitted:.4f}, untrained flow {base:.4f}")
    assert fitted > base
    # uniform weights and no bounds are defaults
    free = pc.FlowPrior.from_samples(x[:200], flow="maf3", train_config={"epochs": 2})
    assert free.dim == 2 and np.isinf(free.bounds).all() and np.isfinite(free.logpdf(y)).all()
    np.testing.assert_allclose(free.scaler.mu, x[:200].mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(free.scaler.sigma, x[:200].std(axis=0), rtol=1e-12)


def test_from_samples_refusals():
    import pocomc_amd as pc
    x, w = weighted_rows(100, 0)
    kw = dict(bounds=BOX, train_config={"epochs": 1})
    for j, v in ((0, 5.0), (1, -6.5), (0, np.nan)):
        y = x.copy()
        y[17, j] = v
        with pytest.raises(ValueError, match="outside the bounds"):
            pc.FlowPrior.from_samples(y, w, **kw)
    for k, v in ((3, -1.0), (3, np.nan), (3, np.inf)):
        bad = w.copy()
        bad[k] = v
        with pytest.raises(ValueError, match="weights must be"):
            pc.FlowPrior.from_samples(x, bad, **kw)
    with pytest.raises(ValueError, match="weights must be"):
        pc.FlowPrior.from_samples(x, np.zeros(100), **kw)
    with pytest.raises(ValueError, match="weights must have shape"):
        pc.FlowPrior.from_samples(x, w[:50], **kw)
    with pytest.raises(ValueError, match="at least 2 dimensions"):
        pc.FlowPrior.from_samples(x[:, :1], w, bounds=BOX[:1])
    with pytest.raises(ValueError, match="too large"):
        pc.FlowPrior.from_samples(np.zeros((10, 158)))
    with pytest.raises(ValueError, match="bounds must have shape"):
        pc.FlowPrior.from_samples(x, w, bounds=BOX[:1])
    with pytest.raises(ValueError, match="train_config has no key"):
        pc.FlowPrior.from_samples(x, w, bounds=BOX, train_config={"epoch": 1})


# ------------------------------------------------------------------------------------------------------------------
# 8. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
def test_a_block_of_run_a_as_part_of_the_prior_of_run_b_on_both_routes(tmp_path):
    """Run A: a 4-D Gaussian under a uniform prior (3 shared parameters and a nuisance parameter).  The marginal flow fitted on
    its first three columns is the prior of run B's columns 4, 0, 2; B's own columns 1 and 3 get a normal and a uniform
    factor.  B once with the prior inside the step and once through ``logpdf`` on the host route: the same bits."""
    import pocomc_amd as pc
    from scipy.stats import norm, uniform
    kw = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)
    a = pc.Sampler(prior=pc.Prior([uniform(-10.0, 20.0)] * 4), likelihood=gauss_at(0.3), random_state=3, **kw)
    with pytest.raises(ValueError, match="has not run"):
        pc.FlowPrior.from_sampler(a, columns=[0, 1, 2])
    a.run(n_total=256, n_evidence=0, progress=False)
    # columns=None is what it was: the sampler's own flow and scaler
    whole, same = pc.FlowPrior.from_sampler(a), pc.FlowPrior(a.flow, a.scaler)
    xa = np.asarray(a.results["x"]).reshape(-1, 4)[:100]
    assert whole.dim == 4 and np.array_equal(whole.logpdf(xa).view(np.int64), same.logpdf(xa).view(np.int64))
    with pytest.raises(ValueError, match="lie in"):
        pc.FlowPrior.from_sampler(a, columns=[0, 1, 4])
    torch.manual_seed(5)
    block = pc.FlowPrior.from_sampler(a, columns=[0, 1, 2], flow="maf3", train_config={"epochs": 30})
    assert block.dim == 3 and np.array_equal(block.bounds, np.array([[-10.0, 10.0]] * 3))
    assert block.flow.spec.univariate == "affine" and block.flow.spec.n_transforms == 3
    D = 5
    prior = pc.JointPrior(block, [4, 0, 2], pc.Prior([norm(0.5, 2.0), uniform(-4.0, 9.0)]))
    assert prior.dim == D
    assert np.array_equal(prior.bounds, np.array([[-10.0, 10.0], [-np.inf, np.inf], [-10.0, 10.0], [-4.0, 5.0], [-10.0, 10.0]]))

    def run_b(on_device, **extra):
        s = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=on_device, **kw, **extra)
        s.run(n_total=256, n_evidence=0, progress=False)
        return s
    dev, host = run_b(True, output_dir=tmp_path), run_b(False)
    assert dev.device_prior is True and host.device_prior is False
    rd, rh = dev.results, host.results
    for k in ("x", "logp", "logl", "logz", "beta"):
        assert np.array_equal(np.asarray(rd[k]), np.asarray(rh[k])), k
    assert dev.evidence() == host.evidence() and dev.calls == host.calls
    assert np.isfinite(np.asarray(rd["logp"])).all() and np.asarray(rd["beta"])[-1] == 1.0
    xs = np.asarray(rd["x"]).reshape(-1, D)
    assert np.array_equal(prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    path = tmp_path / "b.state"
    dev.save_state(path)
    res = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=True, **kw)
    res.load_state(path)
    assert isinstance(res.prior, pc.JointPrior) and res.prior is not prior
    for k in ("x", "logp", "logl", "logz"):
        assert np.array_equal(np.asarray(res.results[k]), np.asarray(rd[k])), k
    assert np.array_equal(res.prior.logpdf(xs[:70]), prior.logpdf(xs[:70]))
    assert isinstance(pickle.loads(pickle.dumps(dev.prior)), pc.JointPrior)
