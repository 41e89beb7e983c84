"""``pocomc_amd.FlowPrior``: a finished run's flow and scaler as a prior, evaluated on the device by ``pmc_flow_prior_pre`` ->
the flow's forward kernel -> ``pmc_flow_prior_post`` (``csrc/flow_prior.hip``).

The yardstick is the float64 restatement of ``tests/flow_prior_model.py`` (the oracle's scaler and flow).  ``log p`` is held
to the tolerances the flow's own ``log_prob`` is held to (``tests/test_gpu_flow.py``: ``TOL`` affine, ``NSF_LADJ`` spline, per
row, measured against the size of the sum's terms); the scaler's log-determinant, float64 on both sides, to ``LDJ_BOUND``
below.  Layout, row position, bad rows, ownership and the Sampler's two routes are bit-for-bit statements."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import cases
import flow_prior_model as fpm
from oracle.maf import OracleMAF
from parity import close_rel, TOL
from pocomc_amd.maf_spec import MAFSpec
from .test_gpu_flow import NSF_INV, NSF_LADJ

pytestmark = pytest.mark.gpu

# Largest |ldj(device) - ldj(model)| over every case of test 1, measured on the MI355X: LDJ_MEASURED.  The two sides add the
# same float64 terms (the device in index order, numpy pairwise) of maps whose erfinv / log differ in their last bits between
# libm and the device, and the model takes the terms at mu + sigma * u where the device takes them at the unscaled value
# itself.  The bound is ten times the measurement, floored at 1e-12.
LDJ_MEASURED = 1.137e-13
LDJ_BOUND = max(10.0 * LDJ_MEASURED, 1e-12)

SHAPES = [(2, 3, "affine"), (5, 3, "rqs"), (17, 2, "affine"), (33, 2, "rqs")]
NS = [1, 63, 64, 65, 200]
EDGE = 1e-6


def bounds_of(D):
    """Two-sided, lower only, upper only, unbounded, and round again."""
    kinds = [[-1.0, 2.0], [0.5, np.inf], [-np.inf, 3.0], [-np.inf, np.inf]]
    return np.array([kinds[j % 4] for j in range(D)])


def rows_in(bounds, n, rng):
    """Rows from EDGE to 1 - EDGE of each side's range: a two-sided feature across its width, its first rows at the two ends;
    a one-sided feature from EDGE above (below) its bound to a few units away; an unbounded one a few units either way."""
    D = len(bounds)
    p = rng.uniform(EDGE, 1.0 - EDGE, size=(n, D))
    p[0::7] = np.where(rng.uniform(size=p[0::7].shape) < 0.5, EDGE, 1.0 - EDGE)
    x = np.empty((n, D))
    for j, (lo, hi) in enumerate(bounds):
        if np.isfinite(lo) and np.isfinite(hi):
            x[:, j] = lo + (hi - lo) * p[:, j]
        elif np.isfinite(lo):
            x[:, j] = lo + 8.0 * p[:, j]
        elif np.isfinite(hi):
            x[:, j] = hi - 8.0 * p[:, j]
        else:
            x[:, j] = 8.0 * (p[:, j] - 0.5)
    return x


def make(D, T, uni, transform="probit", bounds=None, train=None, seed=5):
    """``(prior, oracle scaler, oracle flow, source flow, source scaler)`` on ``bounds``, both scalers fitted on the same rows
    (``train``; 500 rows of ``rows_in`` by default)."""
    import pocomc_amd as pc
    bounds = bounds_of(D) if bounds is None else np.asarray(bounds, dtype=np.float64)
    spec = MAFSpec(D, T, univariate=uni)
    flat = cases.flow_params(spec, seed)
    flow = pc.Flow(D, spec)
    flow.set_params(flat)
    train = rows_in(bounds, 500, np.random.default_rng(11)) if train is None else train
    scaler = pc.Reparameterize(D, bounds=bounds, transform=transform)
    scaler.fit(train)
    oscaler = fpm.oracle_scaler(bounds, transform, train)
    return pc.FlowPrior(flow, scaler), oscaler, OracleMAF(spec, flat), flow, scaler


def pre(prior, xt):
    """``pmc_flow_prior_pre`` alone on a C-contiguous tensor: ``(u32, ldj, inside)`` as numpy."""
    from pocomc_amd import _lib
    n, D = xt.shape
    u32 = torch.empty(n, D, dtype=torch.float32, device=xt.device)
    ldj = torch.empty(n, dtype=torch.float64, device=xt.device)
    inside = torch.empty(n, dtype=torch.int32, device=xt.device)
    _lib.check(_lib.load().pmc_flow_prior_pre(C.byref(prior._sdesc), _lib.ptr(xt), D, 1, n, _lib.ptr(u32), _lib.ptr(ldj),
                                              _lib.ptr(inside), _lib.stream_handle()), "pmc_flow_prior_pre")
    return u32.cpu().numpy(), ldj.cpu().numpy(), inside.cpu().numpy()


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# 1. values
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", ["probit", "logit"])
@pytest.mark.parametrize("D,T,uni", SHAPES)
def test_values_match_the_model(D, T, uni, transform):
    """Every n of NS (one row, one short of a block, a block, one more, several blocks) on the first n of the same 200 rows:
    the model is evaluated once.  Measured on the MI355X: log p 5.6e-7 (affine) / 1.4e-6 (spline) of the terms' size, the
    log-determinant 1.137e-13 (D = 33, logit, |ldj| up to 218)."""
    prior, oscaler, maf, _, _ = make(D, T, uni, transform)
    x = rows_in(bounds_of(D), max(NS), np.random.default_rng(D))
    want, want_ldj, inside = fpm.flow_prior_model(oscaler, maf, x)
    assert inside.all() and np.isfinite(want).all()
    u = oscaler.forward(x).astype(np.float32)
    cancel = maf.ladj_abs_terms(u) + np.abs(want_ldj)
    tol = TOL if uni == "affine" else NSF_LADJ
    xt = torch.from_numpy(x).cuda()
    for n in NS:
        got = prior.logpdf_device(xt[:n])
        assert got.shape == (n,) and got.dtype == torch.float64 and got.is_cuda
        u32, ldj, ins = pre(prior, xt[:n].contiguous())
        assert ins.all()
        err = float(np.abs(ldj - want_ldj[:n]).max())
        worst = close_rel(got.cpu().numpy(), want[:n], 1.0, f"flow prior log p ({uni}) measured", cancel=cancel[:n])
        print(f"D={D} {uni} {transform} n={n}: ldj max abs error {err:.3e} (bound {LDJ_BOUND:.1e}), "
              f"log p max relative error {worst:.3e} (bound {tol:g})")
        close_rel(u32, u[:n], 2e-7, "flow prior u32")               # float32 roundings of float64 values that agree to ~1e-15
        assert err <= LDJ_BOUND, (err, LDJ_BOUND)
        close_rel(got.cpu().numpy(), want[:n], tol, f"flow prior log p ({uni})", cancel=cancel[:n])


def test_the_widest_prior_matches_the_model():
    """D = 157, the width limit: the pre kernel's tile takes 120,832 bytes of LDS (beyond the 48 KiB a launch gets without
    asking) and its row length D | 1 is D itself.  70 rows: a full block and a partial one.  ``log p`` against the model at the
    affine tolerance, both layouts the same bits, one bad row.  Measured on the MI355X: log p 1.7e-7; the log-determinant
    (printed, held by the values test at its own widths) 8.0e-13 with |ldj| up to 755."""
    D, n = 157, 70
    prior, oscaler, maf, _, _ = make(D, 2, "affine")
    x = rows_in(bounds_of(D), n, np.random.default_rng(D))
    want, want_ldj, inside = fpm.flow_prior_model(oscaler, maf, x)
    assert inside.all() and np.isfinite(want).all()
    cancel = maf.ladj_abs_terms(oscaler.forward(x).astype(np.float32)) + np.abs(want_ldj)
    xt = torch.from_numpy(x).cuda()
    got = prior.logpdf_device(xt)
    u32, ldj, ins = pre(prior, xt)
    worst = close_rel(got.cpu().numpy(), want, 1.0, "flow prior log p (D = 157) measured", cancel=cancel)
    print(f"D={D}: ldj max abs error {np.abs(ldj - want_ldj).max():.3e} (|ldj| up to {np.abs(want_ldj).max():.0f}), "
          f"log p max relative error {worst:.3e} (bound {TOL:g})")
    assert ins.all()
    close_rel(got.cpu().numpy(), want, TOL, "flow prior log p (D = 157)", cancel=cancel)
    assert np.array_equal(bits(prior.logpdf_device(xt.t().contiguous().t())), bits(got))
    y = x.copy()
    y[64, 156] = np.nan
    bad = prior.logpdf_device(torch.from_numpy(y).cuda()).cpu().numpy()
    keep = np.arange(n) != 64
    assert np.isneginf(bad[64]) and np.array_equal(bad[keep].view(np.int64), bits(got)[keep])


# ------------------------------------------------------------------------------------------------------------------
# 2. layout
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,uni", [(5, 3, "rqs"), (17, 2, "affine")])
@pytest.mark.parametrize("n", [1, 65, 200])
def test_every_layout_gives_the_same_bits(D, T, uni, n):
    prior = make(D, T, uni)[0]
    x = torch.from_numpy(rows_in(bounds_of(D), n, np.random.default_rng(n))).cuda()
    colmajor = x.t().contiguous().t()
    wide = torch.zeros(n, 2 * D + 3, dtype=torch.float64, device="cuda")
    wide[:, 1:2 * D + 1:2] = x
    sliced = wide[:, 1:2 * D + 1:2]
    assert x.is_contiguous() and (n == 1 or colmajor.stride() == (1, n)) and torch.equal(sliced, x)
    a = prior.logpdf_device(x)
    assert torch.isfinite(a).all()
    for other in (colmajor, sliced, x):
        assert np.array_equal(bits(prior.logpdf_device(other)), bits(a))
    # ... and a row does not depend on its place in the call or on n
    if n > 64:
        assert np.array_equal(bits(prior.logpdf_device(x[37:])), bits(a[37:]))
        assert np.array_equal(bits(prior.logpdf_device(colmajor[64:])), bits(a[64:]))
    assert np.array_equal(prior.logpdf(x.cpu().numpy()).view(np.int64), bits(a))


# ------------------------------------------------------------------------------------------------------------------
# 3. holes
# ------------------------------------------------------------------------------------------------------------------
HOLES = [0, 63, 64, 129]                 # first row, a block's last, the next block's first, the call's last


@pytest.mark.parametrize("transform", ["probit", "logit"])
def test_bad_rows_are_minus_infinity_and_move_nothing_else(transform):
    """130 rows.  Feature 0 is two-sided, 1 bounded below, 2 bounded above, 3 unbounded.  Every kind of bad row at every one of
    HOLES, then one of each kind in one call: exactly -inf there, every other row the bits of the call without bad rows, in
    both layouts; and the flow is handed zeros for them."""
    D, n = 5, 130
    prior = make(D, 3, "rqs", transform)[0]
    x = rows_in(bounds_of(D), n, np.random.default_rng(3))
    good = bits(prior.logpdf_device(torch.from_numpy(x).cuda()))
    assert np.isfinite(good.view(np.float64)).all()
    kinds = {"on the lower bound": (0, -1.0), "beyond the upper bound": (0, 2.5), "NaN": (3, np.nan), "+inf": (1, np.inf),
             "-inf": (3, -np.inf), "on a one-sided bound": (1, 0.5), "beyond a one-sided bound": (2, 3.5)}

    def check(y, bad, what):
        keep = np.setdiff1d(np.arange(n), bad)
        for yt in (torch.from_numpy(y).cuda(), torch.from_numpy(y).cuda().t().contiguous().t()):
            got = prior.logpdf_device(yt).cpu().numpy()
            assert np.isneginf(got[bad]).all(), (what, got[bad])
            assert np.array_equal(got[keep].view(np.int64), good[keep]), what
        u32, ldj, ins = pre(prior, torch.from_numpy(y).cuda())
        assert not ins[bad].any() and ins[keep].all() and not u32[bad].any() and np.isfinite(u32).all(), what
    for what, (j, v) in kinds.items():
        y = x.copy()
        y[HOLES, j] = v
        check(y, HOLES, what)
    y = x.copy()
    rows = HOLES + [100, 65, 1]
    for r, (j, v) in zip(rows, kinds.values()):
        y[r, j] = v
    check(y, rows, "one of each")


# ------------------------------------------------------------------------------------------------------------------
# 4. normalisation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", ["probit", "logit"])
@pytest.mark.parametrize("uni", ["affine", "rqs"])
def test_the_device_density_integrates_to_one(uni, transform):
    """The grid of ``tests/test_flow_prior_cpu.py`` in one call of 360,000 rows.  Measured on the MI355X: the model's figures,
    affine 0.9983 (probit) / 0.9998 (logit), rqs 1.0004 / 1.0001."""
    prior = make(2, 3, uni, transform, bounds=fpm.NORM_BOUNDS, train=fpm.norm_fit_rows())[0]
    x, cell = fpm.norm_grid()
    logp = prior.logpdf_device(torch.from_numpy(x).cuda())
    assert torch.isfinite(logp).all()
    total = float(torch.exp(logp).sum().item() * cell)
    print(f"{uni} {transform}: integral {total:.4f}")
    assert abs(total - 1.0) <= fpm.NORM_BOUND, total


# ------------------------------------------------------------------------------------------------------------------
# 5. ownership
# ------------------------------------------------------------------------------------------------------------------
def test_the_prior_owns_its_flow_and_scaler_and_pickles():
    D = 5
    prior, _, _, flow, scaler = make(D, 3, "rqs")
    x = torch.from_numpy(rows_in(bounds_of(D), 100, np.random.default_rng(1))).cuda()
    a = bits(prior.logpdf_device(x))
    spec = MAFSpec(D, 3, univariate="rqs")
    flow.set_params(cases.flow_params(spec, 9))
    scaler.fit(rows_in(bounds_of(D), 300, np.random.default_rng(2)))
    assert np.array_equal(bits(prior.logpdf_device(x)), a)
    import pocomc_amd as pc
    moved = pc.FlowPrior(flow, scaler)
    assert not np.array_equal(bits(moved.logpdf_device(x)), a)             # (the source did change)
    back = pickle.loads(pickle.dumps(prior))
    assert isinstance(back, pc.FlowPrior) and back.dim == D and np.array_equal(back.bounds, prior.bounds)
    assert np.array_equal(bits(back.logpdf_device(x)), a)
    assert not hasattr(prior, "device_descriptor")


# ------------------------------------------------------------------------------------------------------------------
# 6. rvs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,T,uni", [(2, 3, "affine"), (5, 3, "rqs")])
def test_rvs_draws_from_the_density(D, T, uni):
    """Seed 3: none of the 200 rows needs a redraw at these shapes (asserted: the rows are those of ONE base draw; the probit
    argument of the two-sided features stays below 5.8 / 7.4 where 8.3 saturates), so the density of the draws is
    ``Flow.sample``'s log q of the same base draw minus the scaler's log-determinant.  Seed 4 at D = 2 does need redraws
    (an argument of 10): its rows are inside all the same."""
    prior, oscaler, maf, _, _ = make(D, T, uni)
    b = prior.bounds
    for seed in (4, 3):
        torch.manual_seed(seed)
        x = prior.rvs(200)
        assert x.shape == (200, D) and x.dtype == np.float64
        assert (x > b[:, 0]).all() and (x < b[:, 1]).all()
        torch.manual_seed(seed)
        assert np.array_equal(prior.rvs(200), x)
    assert prior.rvs(1).shape == (1, D)
    torch.manual_seed(3)
    z = torch.randn(200, D, dtype=torch.float32)
    u, lq = prior.flow.sample(200, z=z)
    x1, ldj = prior.scaler.inverse(u.numpy().astype(np.float64))
    assert np.array_equal(x1, x)                                         # no redraw
    want = lq.numpy().astype(np.float64) - ldj
    tol = 10 * TOL if uni == "affine" else 10 * NSF_INV
    cancel = maf.ladj_abs_terms(u.numpy()) + np.abs(ldj)
    worst = close_rel(prior.logpdf(x), want, tol, f"flow prior rvs round trip ({uni})", cancel=cancel)
    print(f"D={D} {uni}: logpdf(rvs) against log q - ldj: max relative error {worst:.3e} (bound {tol:g})")


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import pocomc_amd as pc
    from scipy.stats import uniform
    D = 4
    flow = pc.Flow(D, "maf3", seed=0)
    b = np.array([[-1.0, 1.0]] * D)
    rows = np.random.default_rng(0).uniform(-0.9, 0.9, size=(200, D))
    with pytest.raises(ValueError, match="not fitted"):
        pc.FlowPrior(flow, pc.Reparameterize(D, bounds=b))
    full = pc.Reparameterize(D, bounds=b, diagonal=False)
    full.fit(rows)
    with pytest.raises(ValueError, match="diagonal"):
        pc.FlowPrior(flow, full)
    other = pc.Reparameterize(D + 1, bounds=np.array([[-1.0, 1.0]] * (D + 1)))
    other.fit(np.random.default_rng(0).uniform(-0.9, 0.9, size=(200, D + 1)))
    with pytest.raises(ValueError, match="dimensions"):
        pc.FlowPrior(flow, other)
    s = pc.Sampler(prior=pc.Prior([uniform(-1, 2)] * D), likelihood=lambda x: -0.5 * (x * x).sum(dim=1), vectorize=True,
                   flow="maf3", n_active=64, n_effective=128, random_state=0, device_likelihood=True)
    with pytest.raises(ValueError, match="has not run"):
        pc.FlowPrior.from_sampler(s)
    # one dimension past the widest MCMC step: refused by the class, and by the entry before anything is launched
    W = pc.FlowPrior.MAX_DIM + 1
    assert W == 158
    wide = pc.Reparameterize(W, bounds=np.array([[-1.0, 1.0]] * W))
    wide.fit(np.random.default_rng(0).uniform(-0.9, 0.9, size=(64, W)))
    with pytest.raises(ValueError, match="too large"):
        pc.FlowPrior(pc.Flow(W, MAFSpec(W, 2, 160), seed=0), wide)
    from pocomc_amd import _lib
    xt = torch.zeros(4, W, dtype=torch.float64, device="cuda")
    out = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    rc = _lib.load().pmc_flow_prior_pre(C.byref(wide.device_descriptor()), _lib.ptr(xt), W, 1, 4, _lib.ptr(xt.float()),
                                        _lib.ptr(out), _lib.ptr(torch.zeros(4, dtype=torch.int32, device="cuda")), None)
    assert rc != 0 and b"n_dim too large" in _lib.load().pmc_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # the device function's own contract
    prior = make(5, 3, "affine")[0]
    for bad in (torch.zeros(3, 5, device="cuda"), torch.zeros(3, 4, dtype=torch.float64, device="cuda"),
                torch.zeros(3, 5, dtype=torch.float64), np.zeros((3, 5))):
        with pytest.raises(ValueError):
            prior.logpdf_device(bad)
    assert prior.logpdf_device(torch.zeros(0, 5, dtype=torch.float64, device="cuda")).shape == (0,)


# ------------------------------------------------------------------------------------------------------------------
# 8. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
def gauss_at(c):
    def f(x):
        acc = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
        for j in range(x.shape[1]):
            acc = acc + (x[:, j] - c) ** 2
        return -0.5 * acc
    return f


def test_run_a_as_the_prior_of_run_b_on_both_routes(tmp_path):
    """Run A: a 4-D Gaussian under a uniform prior.  Its flow and scaler are run B's prior (a shifted Gaussian), once evaluated
    inside the step (``device_prior=True``) and once through ``logpdf`` on the host route: the same rows in another layout,
    at another n, at other places in the call -- and the same bits, as ``tests/test_gpu_device_prior_callable.py`` states it
    for ``DevicePrior``."""
    import pocomc_amd as pc
    from scipy.stats import uniform
    D = 4
    kw = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)
    a = pc.Sampler(prior=pc.Prior([uniform(-10.0, 20.0)] * D), likelihood=gauss_at(0.3), random_state=3, **kw)
    with pytest.raises(ValueError, match="has not run"):
        pc.FlowPrior.from_sampler(a)
    a.run(n_total=256, n_evidence=0, progress=False)
    prior = pc.FlowPrior.from_sampler(a)
    assert prior.dim == D and np.array_equal(prior.bounds, np.array([[-10.0, 10.0]] * D))

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
    # B's pool carries A's density: its logp is the prior's value of its x
    xs = np.asarray(rd["x"]).reshape(-1, D)
    assert np.array_equal(prior.logpdf(xs), np.asarray(rd["logp"]).reshape(-1))
    path = tmp_path / "b.state"
    dev.save_state(path)
    res = pc.Sampler(prior=prior, likelihood=gauss_at(0.8), random_state=7, device_prior=True, **kw)
    res.load_state(path)
    assert isinstance(res.prior, pc.FlowPrior) and res.prior is not prior
    for k in ("x", "logp", "logl", "logz"):
        assert np.array_equal(np.asarray(res.results[k]), np.asarray(rd[k])), k
    assert np.array_equal(res.prior.logpdf(xs[:70]), prior.logpdf(xs[:70]))
    assert isinstance(pickle.loads(pickle.dumps(dev.prior)), pc.FlowPrior)
