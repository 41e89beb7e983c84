"""The scipy.stats families beyond uniform / normal on the device (``Prior(dists, device=True)``, pmc_prior_t.par):
the kernel against scipy on grids over the supports' edges, bulk and far tails (classification exact, values to
1e-12 relative to the value and the dimension's log-normaliser), the scaler launch against pmc_prior_logpdf, the MCMC
step against the host prior, x' staying on the device with a device likelihood, and a Sampler run against quadrature."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats as ss

pytestmark = pytest.mark.gpu

SETTINGS = {
    "truncnorm": [ss.truncnorm(-1, 2, loc=0.5, scale=1.5), ss.truncnorm(5, 8), ss.truncnorm(-np.inf, 0.3, scale=2)],
    "loguniform": [ss.loguniform(1e-3, 10), ss.reciprocal(0.5, 2, loc=1, scale=3)],
    "lognorm": [ss.lognorm(0.5), ss.lognorm(s=1.7, loc=-1, scale=2)],
    "halfnorm": [ss.halfnorm(), ss.halfnorm(loc=1, scale=0.3)],
    "expon": [ss.expon(), ss.expon(loc=-2, scale=5)],
    "gamma": [ss.gamma(0.5), ss.gamma(1.0, loc=-3), ss.gamma(a=3.5, scale=2), ss.gamma(2.0)],
    "invgamma": [ss.invgamma(0.7), ss.invgamma(a=3, loc=1, scale=2)],
    "beta": [ss.beta(0.5, 0.5), ss.beta(2, 5, 0, 1), ss.beta(a=1, b=0.3, loc=-1, scale=2), ss.beta(1, 1)],
    "cauchy": [ss.cauchy(), ss.cauchy(loc=3, scale=0.1)],
    "halfcauchy": [ss.halfcauchy(), ss.halfcauchy(loc=-1, scale=4)],
    "laplace": [ss.laplace(), ss.laplace(loc=2, scale=0.5)],
    "t": [ss.t(1), ss.t(30, loc=1, scale=2), ss.t(2.5)],
}


def _lognormaliser(tab, j):
    """|log-normaliser| of dimension j for the tolerance: the family constant and log(scale) of the table (lognorm's
    log(s sqrt(2 pi)) is not in the table: the device takes the log of s x sqrt(2 pi) as scipy does)."""
    c = abs(tab["par"][2, j]) + abs(tab["par"][3, j])
    if tab["family"][j] == 5:
        c += abs(np.log(tab["par"][0, j] * np.sqrt(2 * np.pi)))
    return c


def _grid(d):
    """Support edges, one ulp inside and outside them, the bulk and far tails, in x."""
    lo, hi = d.support()
    _, loc, scale = d.dist._parse_args(*d.args, **d.kwds)
    pts = [loc, loc - scale * 1e-300, np.nextafter(float(loc), np.inf), np.nextafter(float(loc), -np.inf)]
    for e in (lo, hi):
        if np.isfinite(e):
            pts += [e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), np.nextafter(np.nextafter(e, np.inf), np.inf)]
    q = d.ppf(np.linspace(1e-6, 1 - 1e-6, 97))
    pts += list(q[np.isfinite(q)])
    for t in (0.5, 3.0, 30.0, 1e3, 1e8, 1e150, 1e300):
        pts += [loc + scale * t, loc - scale * t]
    x = np.unique(np.array(pts, float))
    return x[np.isfinite(x)]


def dev_logpdf(prior, x, fin=None):
    from pocomc_amd import _lib
    desc = prior.device_descriptor()
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    out = torch.empty(len(x), dtype=torch.float64, device="cuda")
    fd = None if fin is None else torch.from_numpy(fin.astype(np.int32)).cuda()
    _lib.check(_lib.load().pmc_prior_logpdf(C.byref(desc), _lib.ptr(xd), _lib.ptr(fd) if fd is not None else None,
                                           _lib.ptr(out), len(x), _lib.stream_handle()), "pmc_prior_logpdf")
    return out.cpu().numpy()


def _same_class(a, b):
    return (np.isfinite(a) == np.isfinite(b)).all() and (np.isposinf(a) == np.isposinf(b)).all() and \
        (np.isneginf(a) == np.isneginf(b)).all()


@pytest.mark.parametrize("family", sorted(SETTINGS))
def test_kernel_matches_scipy_on_the_grid(family):
    import pocomc_amd as pc
    worst = 0.0
    for d in SETTINGS[family]:
        prior = pc.Prior([d], device=True)
        tab = prior.device_table()
        assert tab["par"] is not None and tab["family"][0] > 2
        x = _grid(d)
        with np.errstate(all="ignore"):
            want = d.logpdf(x)
        got = dev_logpdf(prior, x[:, None])
        bad = ~((np.isfinite(got) == np.isfinite(want)) & (np.isposinf(got) == np.isposinf(want)) &
                (np.isneginf(got) == np.isneginf(want)))
        assert not bad.any(), (family, d.args, d.kwds, x[bad], got[bad], want[bad])
        ok = np.isfinite(want)
        assert ok.sum() > 50
        tol = 1e-12 * (1 + np.abs(want[ok]) + _lognormaliser(tab, 0))
        err = np.abs(got[ok] - want[ok]) / tol
        worst = max(worst, float(err.max()))
        assert (err <= 1).all(), (family, d.args, d.kwds, x[ok][err > 1], got[ok][err > 1], want[ok][err > 1])
    print(f"{family}: worst |device - scipy| = {worst:.2e} of the tolerance")


def test_documented_edge_values():
    import pocomc_amd as pc
    cases = [(ss.gamma(1), 0.0, 0.0), (ss.gamma(0.5), 0.0, np.inf), (ss.gamma(2), 0.0, -np.inf),
             (ss.beta(0.5, 0.5), 0.0, np.inf), (ss.beta(0.5, 0.5), 1.0, np.inf), (ss.lognorm(1.0), 0.0, -np.inf),
             (ss.expon(), 0.0, 0.0), (ss.invgamma(2), 0.0, -np.inf), (ss.halfcauchy(), 1e200, -np.inf)]
    for d, x, v in cases:
        got = dev_logpdf(pc.Prior([d], device=True), np.array([[x]]))[0]
        assert got == v and float(d.logpdf(x)) == v, (d.dist.name, d.args, x, got)


def test_mixed_prior_row_sums():
    """D = 12, one factor of each family: row sums against the reference's loop over dimensions; a finite mask gates
    rows to -inf; without a mask a non-finite x gives a non-finite logp."""
    import pocomc_amd as pc
    dists = [SETTINGS[f][-1] for f in sorted(SETTINGS)]
    prior = pc.Prior(dists, device=True)
    tab = prior.device_table()
    rng = np.random.default_rng(0)
    x = np.column_stack([rng.choice(_grid(d), 2000) for d in dists])
    x[:1000] = np.column_stack([d.rvs(1000, random_state=rng) for d in dists])
    with np.errstate(all="ignore"):
        terms = np.column_stack([d.logpdf(x[:, j]) for j, d in enumerate(dists)])
        want = prior.logpdf(x)
    got = dev_logpdf(prior, x)
    assert _same_class(got, want)
    ok = np.isfinite(want)
    assert ok.sum() > 1000
    tol = 1e-12 * (1 + np.abs(terms[ok]) + np.array([_lognormaliser(tab, j) for j in range(12)])).sum(axis=1)
    err = np.abs(got[ok] - want[ok]) / tol
    print(f"D = 12 row sums: worst |device - scipy| = {err.max():.2e} of the summed tolerance")
    assert (err <= 1).all()
    fin = np.ones(len(x), bool)
    fin[::7] = False
    gated = dev_logpdf(prior, x, fin)
    assert np.isneginf(gated[~fin]).all() and np.array_equal(gated[fin], got[fin])
    xn = x[:8].copy()
    xn[:, 3] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf]
    assert not np.isfinite(dev_logpdf(prior, xn)).any()


def test_uniform_and_normal_factors_keep_their_bits():
    """Uniform / normal factors in a prior with an extended factor: the same bits as the two-family evaluation (the
    gamma(1) factor at 0 adds exactly 0)."""
    import pocomc_amd as pc
    un = [ss.uniform(-2.0, 5.0), ss.norm(0.5, 1.7), ss.uniform(0.0, 1.0), ss.norm(-3.0, 0.2)]
    rng = np.random.default_rng(4)
    x = rng.normal(size=(3000, 4)) * 2.0
    xe = np.column_stack([x, np.zeros(len(x))])
    ext = pc.Prior(un + [ss.gamma(1.0)], device=True)
    assert ext.device_table()["par"] is not None and pc.Prior(un, device=True).device_table()["par"] is None
    assert np.array_equal(dev_logpdf(ext, xe), dev_logpdf(pc.Prior(un), x))


def test_descriptor_without_the_table_is_refused():
    import pocomc_amd as pc
    from pocomc_amd import _lib
    prior = pc.Prior([ss.gamma(2.0), ss.norm()], device=True)
    desc = prior.device_descriptor()
    bad = _lib.pmc_prior_t(family=desc.family, loc=desc.loc, scale=desc.scale, D=2, reserved=0, par=None,
                           n_extended=1, reserved2=0)
    x = torch.ones(4, 2, dtype=torch.float64, device="cuda")
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    lib = _lib.load()
    assert lib.pmc_prior_logpdf(C.byref(bad), _lib.ptr(x), None, _lib.ptr(out), 4, _lib.stream_handle()) != 0
    assert b"par" in lib.pmc_last_error()


def _mixed(D):
    base = [ss.loguniform(0.1, 10), ss.truncnorm(-1, 2, loc=0.5, scale=1.5), ss.beta(2, 3, loc=-1, scale=4),
            ss.gamma(2.0, loc=-1), ss.halfnorm(loc=-2, scale=2), ss.t(5, loc=0.3), ss.laplace(0.2, 0.7),
            ss.expon(loc=-1.5, scale=2)]
    return [base[j % len(base)] for j in range(D)]


def test_scaler_launch_writes_the_bits_of_pmc_prior_logpdf():
    """pmc_scaler_inverse_prior with an extended prior: its logp' is pmc_prior_logpdf's on its x', bit for bit."""
    import pocomc_amd as pc
    from pocomc_amd import _lib
    lib = _lib.load()
    D, n = 8, 777
    prior = pc.Prior(_mixed(D), device=True)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    scaler.fit(prior.rvs(3000))
    rng = np.random.default_rng(2)
    u32 = torch.from_numpy((rng.normal(size=(n, D)) * 2.0).astype(np.float32)).cuda()
    u32[5, 1] = float("nan")
    sd, pd = scaler.device_descriptor(), prior.device_descriptor()
    mk = lambda *s, dt=torch.float64: torch.empty(*s, dtype=dt, device="cuda")
    uo, x, ldj, fin, lp, lp2 = mk(n, D), mk(n, D), mk(n), mk(n, dt=torch.int32), mk(n), mk(n)
    _lib.check(lib.pmc_scaler_inverse_prior(C.byref(sd), C.byref(pd), _lib.ptr(u32), None, _lib.ptr(uo), _lib.ptr(x),
                                            None, _lib.ptr(ldj), _lib.ptr(fin), _lib.ptr(lp), None, None, None, n,
                                            _lib.stream_handle()))
    _lib.check(lib.pmc_prior_logpdf(C.byref(pd), _lib.ptr(x), _lib.ptr(fin), _lib.ptr(lp2), n, _lib.stream_handle()))
    a, b = lp.cpu().numpy(), lp2.cpu().numpy()
    assert np.array_equal(a, b) and np.isneginf(a[5]) and np.isfinite(a).sum() > n // 2
    xs, f = x.cpu().numpy(), fin.cpu().numpy().astype(bool)
    with np.errstate(all="ignore"):
        want = prior.logpdf(xs[f])
    assert _same_class(a[f], want)
    ok = np.isfinite(want)
    np.testing.assert_allclose(a[f][ok], want[ok], rtol=1e-11, atol=1e-11)


KINDS = ["preconditioned_pcn", "preconditioned_rwm", "pcn", "rwm"]


def _problem(D, N, flow_name, seed):
    import pocomc_amd as pc
    from pocomc_amd.geometry import Geometry
    dists = _mixed(D)
    prior = pc.Prior(dists, device=True)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    rng = np.random.default_rng(seed)
    x = np.column_stack([d.rvs(N, random_state=rng) for d in dists])
    scaler.fit(x)
    u = scaler.forward(x)
    flow = pc.Flow(D, flow_name, seed=0)
    flow.set_params(0.25 * flow.params.cpu())
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    geo.normal_cov = np.cov(u.T)
    return dists, prior, scaler, flow, geo, x, u


def f_torch(x):
    acc = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    for j in range(x.shape[1]):
        acc = acc + ((x[:, j] - 0.3) / 1.5) ** 2
    return -0.5 * acc


def _call(kind, prob, device_prior, device_like=False, n_max=6):
    from pocomc_amd import mcmc as pmcmc
    dists, prior, scaler, flow, geo, x, u = prob
    D = x.shape[1]
    if device_like:
        like = lambda xt: (f_torch(xt), None)
    else:
        like = lambda xx: (f_torch(torch.from_numpy(xx).cuda()).cpu().numpy(), None)
    logl0 = f_torch(torch.from_numpy(x).cuda()).cpu().numpy()
    state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0, logp=prior.logpdf(x), beta=0.5,
                 blobs=None)
    funcs = dict(loglike=like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo, u_geometry=geo)
    opts = dict(n_max=n_max, n_steps=10 ** 6, progress_bar=None, proposal_scale=0.5 / D ** 0.5, seed=11,
                device_prior=device_prior)
    opts.update(dict(device_likelihood=True) if device_like else dict(x_order="F"))
    return getattr(pmcmc, kind)(state, funcs, opts)


@pytest.mark.parametrize("flow_name", ["maf3", "nsf3"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_with_the_device_prior_follows_the_host_prior(kind, flow_name):
    """Same seed, prior on the device against the host's scipy: the logp' differ by rounding only, so the accept
    decisions, calls, x, u and logdetj agree (a decision could flip only where the uniform variate lands within
    ~1e-13 of alpha); logp agrees to the prior's tolerance."""
    if not kind.startswith("preconditioned") and flow_name != "maf3":
        pytest.skip("pcn / rwm use no flow: covered once")
    D, N = 8, 1024
    prob = _problem(D, N, flow_name, seed=3)
    a = _call(kind, prob, device_prior=False)
    b = _call(kind, prob, device_prior=True)
    assert a["steps"] == b["steps"] == 6 and a["calls"] == b["calls"]
    assert b["accept"] == pytest.approx(a["accept"], rel=1e-12)           # (the mean of alpha: rounding of logp')
    for k in ("x", "u", "logdetj", "logl"):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(b["logp"], a["logp"], rtol=1e-11, atol=1e-11)
    assert not np.array_equal(b["x"], prob[5])


def test_x_prime_stays_on_the_device(monkeypatch):
    """Device likelihood with an extended device prior: the engine's pinned host x' and finite mask keep a sentinel
    through a whole call (a host prior would need x' on the host)."""
    from pocomc_amd import mcmc as pmcmc
    seen = []
    orig = pmcmc.StepEngine.set_device_likelihood

    def spy(self):
        orig(self)
        self.h_x.fill_(float("nan"))
        self.h_fin.fill_(-7)
        seen.append(self)
    monkeypatch.setattr(pmcmc.StepEngine, "set_device_likelihood", spy)
    prob = _problem(8, 1024, "maf3", seed=1)
    b = _call("preconditioned_pcn", prob, device_prior=True, device_like=True, n_max=8)
    assert b["steps"] == 8 and len(seen) == 1 and seen[0].prior_desc is not None
    assert torch.isnan(seen[0].h_x).all() and (seen[0].h_fin == -7).all()
    a = _call("preconditioned_pcn", prob, device_prior=False, device_like=True, n_max=8)
    assert a["calls"] == b["calls"] and np.array_equal(a["x"], b["x"])


def _reference_logz(dists, mu, sig):
    from scipy.integrate import quad
    total = 0.0
    for d, m, s in zip(dists, mu, sig):
        lo, hi = d.support()
        lo, hi = max(lo, m - 12 * s), min(hi, m + 12 * s)
        f = lambda t: np.exp(d.logpdf(t) - 0.5 * ((t - m) / s) ** 2 - np.log(s * np.sqrt(2 * np.pi)))
        v, _ = quad(f, lo, hi, points=[m], limit=200, epsabs=0, epsrel=1e-10)
        total += np.log(v)
    return total


def test_sampler_evidence_against_quadrature(tmp_path):
    """4-D loguniform x truncnorm x beta x gamma prior, separable normal likelihood: logZ with a host and with a device
    likelihood within 3 of its reported errors (+ 0.05) of the sum of 1-D quadratures; a save / resume round trip."""
    import pocomc_amd as pc
    dists = [ss.loguniform(0.05, 20), ss.truncnorm(-1, 3, loc=0.5, scale=1.5), ss.beta(2, 3), ss.gamma(2.0, loc=-1)]
    mu, sig = np.array([2.0, 1.0, 0.35, 0.5]), np.array([0.8, 0.7, 0.15, 0.6])
    ref = _reference_logz(dists, mu, sig)
    norm_c = -np.log(sig * np.sqrt(2 * np.pi)).sum()

    def like_np(x):
        return -0.5 * (((x - mu) / sig) ** 2).sum(axis=1) + norm_c
    mu_t, sig_t = torch.tensor(mu, device="cuda"), torch.tensor(sig, device="cuda")

    def like_t(x):
        return -0.5 * (((x - mu_t) / sig_t) ** 2).sum(dim=1) + norm_c
    for device in (False, True):
        prior = pc.Prior(dists, device=True)
        s = pc.Sampler(prior=prior, likelihood=like_t if device else like_np, vectorize=True, n_active=256,
                       n_effective=512, random_state=5, train_config={"epochs": 50}, device_likelihood=device,
                       output_dir=tmp_path / str(device), output_label="r")
        s.run(progress=False, n_total=2048, n_evidence=4096, save_every=2)
        logz, err = s.evidence()
        assert np.isfinite(logz) and abs(logz - ref) <= 3 * err + 0.05, (device, logz, err, ref)
        mid = sorted((tmp_path / str(device)).glob("r_[0-9]*.state"), key=lambda p: int(p.stem.split("_")[1]))
        assert mid
        r = pc.Sampler(prior=pc.Prior(dists, device=True), likelihood=like_t if device else like_np, vectorize=True,
                       n_active=256, n_effective=512, random_state=5, train_config={"epochs": 50},
                       device_likelihood=device)
        r.run(progress=False, n_total=2048, n_evidence=4096, resume_state_path=mid[-1])
        assert r.prior.device is True and r.prior.device_table()["par"] is not None
        logz2, err2 = r.evidence()
        assert np.isfinite(logz2) and abs(logz2 - ref) <= 3 * err2 + 0.05, (device, logz2, err2, ref)
