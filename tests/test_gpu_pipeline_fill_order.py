"""The pipelined step enqueues the lanes' pre-steps back to back and the variates of the next step behind the last of
them (``pipeline_enqueue_pre`` in ``csrc/step.hip``, ``LanedEngine._propose_lanes``).  The fills write the other parity's
buffers and nothing reads them before the next step, so the order must not show in any result: the C pipeline, the Python
pipeline and the Python pipeline with every lane's fill inline in its own ``pmc_step_pre`` (the order before the change,
and what a ``StepEngine`` on its own still does) leave the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D = 96, 6
KINDS = ["preconditioned_pcn", "pcn", "preconditioned_rwm"]
# (C pipeline, fills inline in every lane's pmc_step_pre)
VARIANTS = [("1", False), ("0", False), ("0", True)]


def _problem(seed):
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd.geometry import Geometry
    import torch
    prior = pc.Prior([uniform(-5, 10)] * D)
    rng = np.random.default_rng(seed)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    scaler.fit(prior.rvs(2000))
    x = rng.uniform(-4, 4, size=(N, D))
    u = scaler.forward(x)
    flow = pc.Flow(D, "maf3", seed=0)
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    geo.normal_cov = np.cov(u.T)
    return prior, scaler, flow, geo, x, u


def _like(xx):
    l = -0.5 * np.sum(xx ** 2, axis=1)
    l[xx[:, 0] > 3.5] = -np.inf
    return l, None


def _inline_fills(monkeypatch):
    """Every lane's pre-step fills the next step's variates itself, as a lone ``StepEngine`` does."""
    from pocomc_amd import mcmc as pmcmc
    real = pmcmc.StepEngine.propose
    calls = []

    def propose(self, sigma, nu=0.0, replay=None, step=None, defer_fill=False):
        calls.append(defer_fill)
        return real(self, sigma, nu, replay=replay, step=step, defer_fill=False)
    monkeypatch.setattr(pmcmc.StepEngine, "propose", propose)
    monkeypatch.setattr(pmcmc.StepEngine, "fill_next", lambda self, nu=0.0: None)
    return calls


def _run(kind, lanes, prob, drains=(), steps=12):
    from pocomc_amd.mcmc import LanedEngine, Adaptation
    prior, scaler, flow, geo, x, u = prob
    pre = kind.startswith("preconditioned")
    tpcn = kind.endswith("pcn")
    beta, nu = 0.5, 5.0
    g_mu, g_cov = (geo.t_mean, geo.t_cov) if tpcn else (None, geo.normal_cov)
    eng = LanedEngine(kind, N, D, flow if pre else None, scaler, lanes=lanes, seed=77, x_order="F", streams=False)
    assert eng.set_device_prior(prior)
    eng.load_state(u, x, scaler.inverse(u)[1], _like(x)[0], prior.logpdf(x))
    eng.set_geometry(mu=g_mu, cov=g_cov)
    ad = Adaptation(kind, D, N, n_steps=10 ** 9, n_max=10 ** 9, sigma0=2.38 / D ** 0.5, mu0=g_mu, logp2_0=-np.inf)
    assert eng.can_pipeline()
    eng.start_pipeline(float(ad.sigma), ad.mu, nu)
    all_sums = []
    for k in range(1, steps + 1):
        last = k in drains or k == steps
        _, sums = eng.step_pipelined(beta, nu, ad.coefficients(), N, prior.logpdf, _like, more=not last)
        all_sums.append(np.array(sums, copy=True))
        ad.update(all_sums[-1])
        if k in drains:
            eng.finish_pipeline()
            eng.resume_pipeline(nu)
    eng.finish_pipeline()
    used_c = bool(eng._pipe)
    mu = None if ad.mu is None else np.array(ad.mu, copy=True)
    return eng.download(), np.array(all_sums), float(ad.sigma), mu, used_c


def _same(a, b):
    (sa, ua, ga, ma, _), (sb, ub, gb, mb, _) = a, b
    for k in ("u", "x", "logl", "logp", "logdetj"):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    np.testing.assert_array_equal(ua, ub, err_msg="sums")
    assert ga == gb
    assert (ma is None and mb is None) or np.array_equal(ma, mb)


@pytest.mark.parametrize("lanes", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_twelve_pipelined_steps_do_not_depend_on_where_the_fills_sit(kind, lanes, monkeypatch):
    prob = _problem(lanes)
    out = []
    for c_pipe, inline in VARIANTS:
        with monkeypatch.context() as mp:
            mp.setenv("PMC_C_PIPELINE", c_pipe)
            calls = _inline_fills(mp) if inline else None
            out.append(_run(kind, lanes, prob))
            assert out[-1][4] == (c_pipe == "1")
            if inline:
                assert calls and all(calls)          # (the pipeline asked for deferred fills; this variant filled inline)
    _same(out[0], out[1])
    _same(out[0], out[2])
    assert not np.array_equal(out[0][0]["x"], prob[4])          # (walkers did move)


@pytest.mark.parametrize("lanes", [2, 3])
def test_a_drained_and_resumed_pipeline_does_not_depend_on_where_the_fills_sit(lanes, monkeypatch):
    """``resume_pipeline`` enqueues the pre-steps and the fills in the new order too: drained behind steps 3 and 8, every
    variant equals the twelve steps in one go with the fills inline."""
    prob = _problem(10 + lanes)
    with monkeypatch.context() as mp:
        mp.setenv("PMC_C_PIPELINE", "0")
        _inline_fills(mp)
        ref = _run("preconditioned_pcn", lanes, prob)
    for c_pipe in ("1", "0"):
        with monkeypatch.context() as mp:
            mp.setenv("PMC_C_PIPELINE", c_pipe)
            _same(ref, _run("preconditioned_pcn", lanes, prob, drains=(3, 8)))


@pytest.mark.parametrize("kind", ["preconditioned_pcn", "pcn"])
def test_a_plateau_stop_with_a_pre_step_in_flight_does_not_depend_on_where_the_fills_sit(kind, monkeypatch):
    """The stop rule fires while the next pre-steps (and, behind them, their fills) are enqueued: the whole call returns
    the same state, and the next call starts from variates it draws itself."""
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, _, _ = _problem(5)
    x = np.random.default_rng(3).normal(size=(N, D)) * 0.3              # already at the mode: logP stops improving at once
    u = scaler.forward(x)
    res = []
    for c_pipe, inline in VARIANTS:
        with monkeypatch.context() as mp:
            mp.setenv("PMC_C_PIPELINE", c_pipe)
            if inline:
                _inline_fills(mp)
            two = []
            for _ in range(2):                           # (the second call follows a call that left a fill in flight)
                state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=_like(x)[0], logp=prior.logpdf(x),
                             beta=1.0, blobs=None)
                funcs = dict(loglike=_like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo,
                             u_geometry=geo)
                opts = dict(n_max=500, n_steps=2, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=5, lanes=2,
                            x_order="F")
                two.append(getattr(pmcmc, kind)(state, funcs, opts))
            res.append(two)
    a = res[0][0]
    assert 1 < a["steps"] < 500
    for two in res:
        for b in two:
            assert a["steps"] == b["steps"] and a["calls"] == b["calls"]
            for k in ("u", "x", "logl", "logp", "logdetj"):
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
            assert a["proposal_scale"] == b["proposal_scale"] and a["accept"] == b["accept"]
