"""The tpCN step at the degrees of freedom a Student-t EM fit hands over (``Geometry(student="em")``): the lower clamp
nu = 0.1, a converged heavy-tailed fit (0.9057), a large-nu fit (588.26) and the upper end of the fit's bracket (1e4) --
the golden and teacher-forced cases of ``cases.MCMC_CASES`` use nu in {3.5, 4, 5, 7.5, 1e6}.

The reference is the float64 oracle (``oracle/mcmc.py``), teacher-forced step by step exactly as
``tests/test_gpu_mcmc.py::test_step_teacher_forced`` does it, with that test's criteria (``tols(case)``): theta', u', x' and
the log-determinants per walker, alpha against mcmc.py:124-134 applied to what the device holds (the reference's own
``log(1 + q / nu)``), decisions ``== (u < alpha)`` with flips inside the alpha gap only.  The cases are
``cases.NU_RANGE_CASES``; they need no vectors from the reference.

Two of that test's criteria cannot hold on proposals this far out, whatever computes them, and ``teacher_forced`` replaces
them for cases handed to it as a dict (the reasons and the figures are next to the code there): x' is an exponential of
u' on a half-bounded coordinate (|u'| reaches 1e7 here), so it is held to the oracle's scaler applied to the device's own
u' at 1e-10, and the moved state and the sums to the device's own proposal exactly; u' of the affine flows is held per
walker to 1e-5 or, where the exact inverse itself moves by more than 2.5e-6 per float32 ulp of theta', to four such ulps."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats

import cases
import student_em as se
from oracle import mcmc as omcmc
from test_gpu_mcmc import oracle_case, product_case, teacher_forced

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------- a, b. teacher-forced, fused and as separate launches
@pytest.mark.parametrize("no_fuse", [0, 3], ids=["fused", "separate"])
@pytest.mark.parametrize("name", list(cases.NU_RANGE_CASES))
def test_step_teacher_forced_at_the_fits_nu(name, no_fuse, monkeypatch):
    """``PMC_NO_FUSE = 3``: proposal, sweep and scaler as separate launches.  At nu = 0.1 with the half-bounded prior the
    oracle alone rejects a proposal outright in some step (x' or its log-determinant not finite, or outside the prior's
    support) while more than half stay finite: the finite / prior gating of ``scaler_body.h`` and the accept kernel's
    handling of -inf and NaN exponents see the regime the fit produces.  With the box prior and with the spline flow no
    seed of 300 gets there (``cases.NU_RANGE_CASES``): every proposal of those cases reaches the likelihood, which is
    asserted as well."""
    monkeypatch.setenv("PMC_NO_FUSE", str(no_fuse))
    c = cases.NU_RANGE_CASES[name]
    trace = teacher_forced(name, case=c)
    rejected = [int((~tr["finite"]).sum()) for tr in trace]
    print(f"{name}: proposals the oracle rejects before the likelihood, per step: {rejected}")
    if name in cases.NU_RANGE_REJECTING:
        assert 1 <= max(rejected) <= c["N"] // 2
    elif c["nu"] == 0.1:
        assert max(rejected) == 0


# ------------------------------------------------------------------------------------------------ c. Philox mode
def test_t_scale_follows_its_law_at_the_lower_clamp():
    """nu = 0.1, D = 2: the t-scale s = (nu + q) / (2 g) with g ~ Gamma((D + nu) / 2 = 1.05), drawn inline (Philox).  One
    proposal with L = I, mu = 0, cn_a = 0 and z = (1, 0) supplied gives theta'_0 = sigma sqrt(s); with q from the kernel,
    (nu + q) sigma^2 / theta'_0^2 = 2 g.  The criterion of ``test_gpu_rng.py::test_gamma_draws_follow_the_gamma_law``."""
    from pocomc_amd import _lib
    from pocomc_amd.mcmc import PMC_KIND_TPCN
    from test_gpu_rng import N, P_MIN
    lib = _lib.load()
    _lib.require_gpu()
    D, nu, sigma = 2, 0.1, 0.7
    shape = 0.5 * (D + nu)
    rng = np.random.default_rng(3)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    cur = up(rng.normal(size=(N, D)) * np.array([0.3, 3.0]))               # q from 1e-6 to about 100
    z = up(np.tile([1.0, 0.0], (N, 1)))
    eye, mu = up(np.eye(D)), up(np.zeros(D))
    t64, q = torch.empty(N, D, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    qp = torch.empty_like(q)
    r = _lib.pmc_rng_t(gamma=None, normal=z.data_ptr(), uniform=None, seed=20240928, step=3, offset=0)
    _lib.check(lib.pmc_propose(PMC_KIND_TPCN, None, _lib.ptr(cur), _lib.ptr(mu), _lib.ptr(eye), _lib.ptr(eye), nu, sigma, 0.0,
                               C.byref(r), _lib.ptr(t64), None, _lib.ptr(q), _lib.ptr(qp), N, D, _lib.stream_handle()),
               "pmc_propose")
    torch.cuda.synchronize()
    th, qn, qpn = t64.cpu().numpy(), q.cpu().numpy(), qp.cpu().numpy()
    np.testing.assert_allclose(qn, np.sum(cur.cpu().numpy() ** 2, axis=1), rtol=1e-14)
    assert np.all(th[:, 1] == 0.0) and np.all(th[:, 0] > 0) and np.isfinite(th).all()
    np.testing.assert_allclose(qpn, th[:, 0] ** 2, rtol=1e-14)
    g = 0.5 * (nu + qn) * sigma ** 2 / th[:, 0] ** 2
    print(f"t-scale at nu = 0.1: sqrt(s) from {th[:, 0].min() / sigma:.3g} to {th[:, 0].max() / sigma:.3g}, g from {g.min():.3g} to {g.max():.3g}")
    ks = stats.kstest(g, stats.gamma(a=shape).cdf)
    assert ks.pvalue > P_MIN, ks
    assert abs(g.mean() - shape) < 5 * np.sqrt(shape / N)
    assert abs(g.var() / shape - 1) < 5 * np.sqrt((2 + 6 / shape) / N)
    assert th[:, 0].max() / th[:, 0].min() > 1e3                           # (the scale spans decades)


# -------------------------------------------------------------------------------------------------- d. hand-over
def handover_case(geometry, D, seed):
    return dict(kind="preconditioned_pcn", N=96, D=D, T=3, beta=0.5, nu=None, prior="mixed", target="gauss", seed=seed,
                n_max=2, geometry=geometry)


def test_lower_clamp_fit_goes_into_the_step():
    """``Geometry(student="em")`` on t_0.3 rows ends at the lower clamp; the step takes ``nu`` from ``g.t_nu``."""
    from pocomc_amd.geometry import Geometry
    g = Geometry(student="em")
    g.fit(se.mvt_rows(4, 1024, 3, 0.3))
    assert g.student_info["status"] == "lower_clamp" and g.t_nu == se.NU_LO
    teacher_forced("handover_lower_clamp", case=handover_case(g, 3, 240))


def first_step(case):
    """The device's first step of a case on the oracle's variates: what the proposal and the accept launch wrote."""
    from pocomc_amd.mcmc import StepEngine
    state, funcs, opts, _ = oracle_case("handover", case)
    rng = omcmc.LegacyStream()
    np.random.seed(case["seed"])
    omcmc.preconditioned_pcn(state, funcs, dict(opts, n_max=1), rng=rng)
    pstate, pfuncs, popts, _ = product_case("handover", case)
    geo = pfuncs["theta_geometry"]
    eng = StepEngine("preconditioned_pcn", case["N"], case["D"], pfuncs["flow"], pfuncs["scaler"])
    eng.load_state(pstate["u"], pstate["x"], pstate["logdetj"], pstate["logl"], pstate["logp"])
    eng.set_geometry(mu=geo.t_mean, cov=geo.t_cov)
    rec = rng.record[0]
    eng.propose(min(popts["proposal_scale"], 0.99), float(geo.t_nu), dict(gamma=rec["gamma"], z=rec["z"], u=rec["u"]))
    eng.evaluate(pfuncs["logprior"], pfuncs["loglike"])
    sums = eng.accept_reduce(case["beta"], float(geo.t_nu), want_mask=True)
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in ("p_theta64", "p_u", "p_x", "p_logdetj", "quad", "p_quad", "alpha")}
    out["accept"] = eng.h_accept.numpy().copy()
    out["sums"] = np.array(sums, dtype=np.float64)
    out.update({"post_" + k: v for k, v in eng.download().items()})
    return out


def test_gaussian_fit_hands_over_the_reference_step():
    """Gaussian rows: the EM fit leaves at its first iteration (``nu_inf``), ``t_nu == 1e6``, and the step is the step of
    ``Geometry(student="reference")`` on the same rows, bit for bit."""
    from pocomc_amd.geometry import Geometry
    x = se.mvt_rows(3, 2048, 6, np.inf)
    out = {}
    for mode in ("reference", "em"):
        g = Geometry(student=mode)
        g.fit(x)
        assert g.t_nu == 1e6
        out[mode] = first_step(handover_case(g, 6, 241))
        if mode == "em":
            assert g.student_info["status"] == "nu_inf"
            teacher_forced("handover_nu_inf", case=handover_case(g, 6, 241))
    assert out["em"].keys() == out["reference"].keys()
    for k, v in out["em"].items():
        assert np.array_equal(v, out["reference"][k], equal_nan=True), k
