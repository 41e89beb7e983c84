"""The MCMC step with a likelihood on the GPU (``option_dict["device_likelihood"]``, ``Sampler(device_likelihood=True)``):
x' is written for the likelihood on the device, the accept gates logl' itself (``pmc_step_t.lik_x``), and the result is
the host path's bit for bit -- walkers, sums, adaptation, call counts.  The host comparator is the pipelined host call
(``x_order='F'``), which adapts sigma / mu on the device as the device-likelihood call does; it hands the same torch
likelihood the host's x' (``lambda x: (f(torch.from_numpy(x).cuda()).cpu().numpy(), None)``)."""
import numpy as np
import pytest
import torch

KINDS = ["preconditioned_pcn", "preconditioned_rwm", "pcn", "rwm"]


def f_torch(x):
    """Row-wise, independent of the batch a row is in and of the layout of ``x``: a column after column accumulation."""
    acc = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    for j in range(x.shape[1]):
        acc = acc + (x[:, j] - 0.3) ** 2
    return -0.5 * acc


def host_like(f):
    return lambda x: (f(torch.from_numpy(x).cuda()).cpu().numpy(), None)


def device_like(f):
    return lambda xt: (f(xt), None)


def _problem(D, N, flow_name, seed, prior=None, bounds=10.0):
    """Walkers inside a narrow uniform prior (|x| <= 3) whose scaler box is wider: proposals can leave the support."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd.geometry import Geometry
    prior = prior or pc.Prior([uniform(-3, 6)] * D)
    rng = np.random.default_rng(seed)
    scaler = pc.Reparameterize(D, bounds=np.array([[-bounds, bounds]] * D))
    x = 0.5 * rng.uniform(-2.0, 2.0, size=(N, D))
    x[: N // 64] = rng.uniform(2.9, 2.99, size=(N // 64, D))          # a few walkers at the edge of the support
    scaler.fit(x)
    u = scaler.forward(x)
    flow = pc.Flow(D, flow_name, seed=0)
    flow.set_params(0.25 * flow.params.cpu())
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    geo.normal_cov = np.cov(u.T)
    return prior, scaler, flow, geo, x, u


def _call(kind, prob, loglike, logl0, device, n_max=8, scale=None, **extra):
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    D = x.shape[1]
    state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x),
                 beta=0.5, blobs=None)
    funcs = dict(loglike=loglike, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo, u_geometry=geo)
    opts = dict(n_max=n_max, n_steps=10 ** 6, progress_bar=None, proposal_scale=(scale or 0.25) / D ** 0.5, seed=5,
                **extra)
    if device:
        opts["device_likelihood"] = True
    else:
        opts["x_order"] = "F"
    return getattr(pmcmc, kind)(state, funcs, opts)


def _assert_same(a, b):
    for k in ("u", "x", "logl", "logp", "logdetj"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("steps", "calls", "proposal_scale", "accept"):
        assert a[k] == b[k], (k, a[k], b[k])


FLOWS = [("maf3", 6), ("nsf3", 6), ("maf6", 50)]       # fused affine sweep, spline sweep, lane sweep + scaler launch


@pytest.mark.gpu
@pytest.mark.parametrize("flow_name,D", FLOWS)
@pytest.mark.parametrize("kind", KINDS)
def test_device_likelihood_call_equals_the_host_call_bit_for_bit(kind, flow_name, D):
    if not kind.startswith("preconditioned") and flow_name != "maf3":
        pytest.skip("pcn / rwm use no flow: covered once")
    from pocomc_amd import _lib
    import ctypes
    N = 1024
    prob = _problem(D, N, flow_name, seed=D)
    if flow_name == "maf6":
        assert _lib.load().pmc_maf_inverse_auto_is_lane(ctypes.byref(prob[2]._desc)) == 1
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    a = _call(kind, prob, host_like(f_torch), logl0, device=False)
    b = _call(kind, prob, device_like(f_torch), logl0, device=True)
    _assert_same(a, b)
    assert b["steps"] == 8 and b["calls"] < 8 * N                         # some proposals left the support
    assert b["evaluations"] == 8 * N                                       # ... yet every step handed over all rows
    assert not np.array_equal(b["x"], prob[4])


@pytest.mark.gpu
@pytest.mark.parametrize("no_fuse", [0, 2])
@pytest.mark.parametrize("kind", ["preconditioned_pcn", "rwm"])
def test_gated_rows_never_reach_the_device_likelihood(kind, no_fuse, monkeypatch):
    """A wide proposal scale sends many proposals out of the prior's support: the likelihood only ever sees finite rows
    inside it (the rejected rows carry the walkers' current x), the result and the count of rows that reached the
    likelihood equal the host path's.  ``no_fuse=2``: the scaler + prior as a launch of their own."""
    monkeypatch.setenv("PMC_NO_FUSE", str(no_fuse))
    D, N = 5, 1024
    prob = _problem(D, N, "maf3", seed=3)

    def strict(xt):
        assert bool(torch.isfinite(xt).all()) and float(xt.abs().max()) <= 3.0
        return f_torch(xt)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    a = _call(kind, prob, host_like(f_torch), logl0, device=False, scale=2.38)
    b = _call(kind, prob, device_like(strict), logl0, device=True, scale=2.38)
    _assert_same(a, b)
    assert b["calls"] < (0.9 if kind == "rwm" else 1.0) * 8 * N        # (tpCN caps sigma at 0.99: fewer leave)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["preconditioned_pcn", "pcn"])
def test_nan_from_the_device_likelihood_is_never_accepted(kind):
    """NaN logl' gives alpha = 0 (``mcmc.py:134``), as on the host path."""
    D, N = 5, 1024
    prob = _problem(D, N, "maf3", seed=9)

    def holes(x):
        ll = f_torch(x)
        return torch.where(x[:, 1] < -0.4, torch.full_like(ll, float("nan")), ll)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    a = _call(kind, prob, host_like(holes), logl0, device=False, scale=1.0)
    b = _call(kind, prob, device_like(holes), logl0, device=True, scale=1.0)
    _assert_same(a, b)
    assert np.isfinite(b["logl"]).all()
    moved = ~(b["x"] == prob[4]).all(axis=1)
    assert moved.any() and (b["x"][moved, 1] >= -0.4).all()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["gamma", "device_prior_off"])
@pytest.mark.parametrize("kind", ["preconditioned_pcn", "rwm"])
def test_host_prior_fallback_equals_the_host_call(kind, how):
    """A prior the device does not evaluate (a gamma factor), or ``device_prior=False``: x' goes to the host for
    Prior.logpdf only, logp' is uploaded, the likelihood stays on the device -- the same call bit for bit."""
    from scipy.stats import gamma, uniform
    import pocomc_amd as pc
    D, N = 5, 1024
    extra = {}
    if how == "gamma":
        prior = pc.Prior([uniform(-3, 6)] * (D - 1) + [gamma(2.0, loc=-3.0)])
        assert prior.device_descriptor(torch.device("cuda", 0)) is None
    else:
        prior = pc.Prior([uniform(-3, 6)] * D)
        extra = dict(device_prior=False)
    prob = _problem(D, N, "maf3", seed=4, prior=prior)

    def strict(xt):
        assert bool(torch.isfinite(xt).all())
        if how != "gamma":
            assert float(xt.abs().max()) <= 3.0
        return f_torch(xt)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    a = _call(kind, prob, host_like(f_torch), logl0, device=False, scale=1.0, **extra)
    b = _call(kind, prob, device_like(strict), logl0, device=True, scale=1.0, **extra)
    _assert_same(a, b)
    assert b["calls"] < 8 * N


@pytest.mark.gpu
def test_x_prime_stays_on_the_device(monkeypatch):
    """With a device prior the pre-step hands x' to nobody but the likelihood: the engine's pinned host x' and finite
    mask keep a sentinel through a whole call."""
    from pocomc_amd import mcmc as pmcmc
    seen = []
    orig = pmcmc.StepEngine.set_device_likelihood

    def spy(self):
        orig(self)
        self.h_x.fill_(float("nan"))
        self.h_fin.fill_(-7)
        seen.append(self)
    monkeypatch.setattr(pmcmc.StepEngine, "set_device_likelihood", spy)
    D, N = 6, 1024
    prob = _problem(D, N, "maf3", seed=1)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    b = _call("preconditioned_pcn", prob, device_like(f_torch), logl0, device=True)
    assert b["steps"] == 8 and len(seen) == 1
    assert torch.isnan(seen[0].h_x).all() and (seen[0].h_fin == -7).all()


@pytest.mark.gpu
def test_device_likelihood_contract_errors():
    """A result of the wrong shape, dtype or device, a numpy result, blobs: ValueError naming the problem."""
    D, N = 4, 256
    prob = _problem(D, N, "maf3", seed=2)
    logl0 = f_torch(torch.from_numpy(prob[4]).cuda()).cpu().numpy()
    bad = [(lambda xt: (f_torch(xt)[:-1], None), "shape"), (lambda xt: (f_torch(xt).to(torch.float16), None), "dtype"),
           (lambda xt: (f_torch(xt).cpu(), None), "device"), (lambda xt: (f_torch(xt).cpu().numpy(), None), "ndarray")]
    for fn, word in bad:
        with pytest.raises(ValueError, match=word):
            _call("preconditioned_pcn", prob, fn, logl0, device=True, n_max=2)
    # float32 is widened on the device
    r32 = _call("rwm", prob, lambda xt: (f_torch(xt).float(), None), logl0, device=True, n_max=3)
    r64 = _call("rwm", prob, lambda xt: (f_torch(xt).float().double(), None), logl0, device=True, n_max=3)
    _assert_same(r32, r64)
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    state = dict(u=u, x=x, logdetj=scaler.inverse(u)[1], logl=logl0, logp=prior.logpdf(x), beta=0.5,
                 blobs=np.zeros(N))
    with pytest.raises(ValueError, match="blobs"):
        pmcmc.rwm(state, dict(loglike=device_like(f_torch), logprior=prior.logpdf, scaler=scaler, u_geometry=geo),
                  dict(n_max=2, n_steps=10, progress_bar=None, proposal_scale=0.5, device_likelihood=True))


@pytest.mark.gpu
def test_sampler_constructor_contract():
    from scipy.stats import uniform
    import pocomc_amd as pc
    prior = pc.Prior([uniform(-5, 10)] * 3)
    with pytest.raises(ValueError, match="vectorize"):
        pc.Sampler(prior=prior, likelihood=f_torch, device_likelihood=True, random_state=0)
    with pytest.raises(ValueError, match="blobs"):
        pc.Sampler(prior=prior, likelihood=f_torch, vectorize=True, blobs_dtype=float, device_likelihood=True,
                   random_state=0)


def _sampler(device, **kw):
    from scipy.stats import uniform
    import pocomc_amd as pc
    D = 5
    prior = pc.Prior([uniform(-5, 10)] * D)
    like = f_torch if device else (lambda x: f_torch(torch.from_numpy(x).cuda()).cpu().numpy())
    opts = {} if device else dict(mcmc_options=dict(x_order="F"))
    return pc.Sampler(prior=prior, likelihood=like, vectorize=True, n_active=256, n_effective=512, random_state=7,
                      train_config={"epochs": 30}, device_likelihood=device, **opts, **kw)


@pytest.mark.gpu
def test_sampler_with_a_device_likelihood_equals_the_host_sampler(tmp_path):
    """Default flow (nsf6), D = 5: posterior samples and weights, evidence and likelihood calls are the host sampler's bit
    for bit; a run resumed from a mid-run checkpoint matches the host sampler resumed from its own."""
    out = []
    for device in (False, True):
        s = _sampler(device, output_dir=tmp_path / str(device), output_label="r")
        s.run(progress=False, n_total=1024, n_evidence=1024, save_every=2)
        x, w, logl, logp = s.posterior()
        out.append((x, w, logl, s.evidence(), s.calls))
    (xa, wa, la, za, ca), (xb, wb, lb, zb, cb) = out
    assert np.array_equal(xa, xb) and np.array_equal(wa, wb) and np.array_equal(la, lb)
    assert za == zb and ca == cb and np.isfinite(zb[0])
    res = []
    for device in (False, True):
        mid = sorted((tmp_path / str(device)).glob("r_[0-9]*.state"), key=lambda p: int(p.stem.split("_")[1]))
        assert len(mid) >= 2
        s = _sampler(device)
        s.run(progress=False, n_total=1024, n_evidence=1024, resume_state_path=mid[1])
        assert s.device_likelihood is device
        x, w, _, _ = s.posterior()
        res.append((x, w, s.evidence(), s.calls))
    assert all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for p, q in zip(*res))


def test_device_likelihood_result_is_checked():
    """What the device likelihood returns (no GPU needed for the checks that come before the device's)."""
    from pocomc_amd.mcmc import device_logl
    ok = torch.zeros(4, dtype=torch.float64)
    assert device_logl((ok, None), 4, "cpu") is ok
    assert device_logl(ok.float(), 4, "cpu").dtype == torch.float32
    for out, word in ((np.zeros(4), "ndarray"), (torch.zeros(3, dtype=torch.float64), r"shape \(4,\), got \(3,\)"),
                      (torch.zeros(4, 1, dtype=torch.float64), "shape"), (torch.zeros(4, dtype=torch.int64), "int64"),
                      (ok, "device cuda:0, got one on cpu")):
        with pytest.raises(ValueError, match=word):
            device_logl(out, 4, "cuda:0")
