"""The scaler's element stage keeps a feature's constants in registers (``csrc/scaler_body.h``: ``ScalerFeat``): a thread of
the fused sweeps' epilogue and of ``scaler_inverse_kernel`` takes ONE feature, requests its constants once and walks its
rows.  Both users share the element code, so the fused pre-step
(``pmc_step_pre``) and the scaler launch of its own (``pmc_scaler_inverse_prior``) on the same u' must agree bit for bit, and
both must follow the float64 restatement (``oracle/scaler.py``, the round trip of ``oracle/mcmc.py``) within the tolerances
of ``tests/test_gpu_tools.py``.

D in {5, 8, 32, 33, 50, 64}: threads per workgroup a multiple of D and not, D a multiple of 8 and not (the pairwise sum's
tail); n in {1, 16, 17, 100}: a partly filled workgroup, more than one.  The features cycle through the four kinds of
bounds; periodic / reflective boundary conditions on some of them in half of the cases; logit and probit, with and without
the affine part; a prior of uniform and normal factors with one feature whose x' can leave its support; rows whose u' is
+-inf or NaN."""
import ctypes as C

import numpy as np
import pytest

DS = (5, 8, 32, 33, 50, 64)
NS = (1, 16, 17, 100)
SCALERS = {"probit-scaled": ("probit", True), "probit-unscaled": ("probit", False),
           "logit-scaled": ("logit", True), "logit-unscaled": ("logit", False)}
WIDE = 3                                       # the feature whose box is twice its prior's support
BAD = {3: np.inf, 5: np.nan, 7: -np.inf}       # rows whose theta (and with it u') is made non-finite
SKIPPED = []                                   # (D, scaler) whose fused leg the plan does not have


def _flow(D):
    import pocomc_amd as pc
    from pocomc_amd.maf_spec import MAFSpec
    # the flows whose fused sweep has the epilogue (the plan's answer, asserted below): the affine two-wave sweep up to its
    # 15 hidden tiles, the two-wave spline sweep at D = 64
    if D == 64:
        return pc.Flow(D, "nsf3", seed=0)
    return pc.Flow(D, MAFSpec(D, 3, 160) if D == 50 else "maf3", seed=0)


def _plan(flow, n):
    from pocomc_amd import _lib
    p = _lib.pmc_inverse_plan_t()
    _lib.check(_lib.load().pmc_maf_inverse_plan(C.byref(flow._desc), n, 0, 1, C.byref(p)), "pmc_maf_inverse_plan")
    return p


def _setup(D, with_bc):
    """bounds by kind j % 4 (none, low, high, both), the prior, the boundary conditions."""
    from scipy.stats import norm, uniform
    kinds = np.arange(D) % 4
    low = np.where((kinds == 1) | (kinds == 3), -5.0, -np.inf)
    high = np.where((kinds == 2) | (kinds == 3), 5.0, np.inf)
    low[WIDE], high[WIDE] = -10.0, 10.0
    dists = [uniform(-5, 10) if k == 3 else norm(0.5, 2.0) for k in kinds]
    both = [j for j in range(D) if kinds[j] == 3]
    periodic = both[0::2] if with_bc else None                 # (D = 5: one periodic feature, no reflective one)
    reflective = (both[1::2] or None) if with_bc else None
    return np.stack([low, high], axis=1), dists, periodic, reflective


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _fused(n, D, flow, scaler, prior, x, u):
    import torch
    from pocomc_amd.mcmc import StepEngine
    eng = StepEngine("preconditioned_pcn", n, D, flow, scaler, seed=9, x_order="F")
    assert eng.set_device_prior(prior)
    eng.load_state(u, x, scaler.inverse(u)[1], -0.5 * np.sum(x ** 2, axis=1), prior.logpdf(x))
    eng.set_geometry(mu=np.zeros(D), cov=np.eye(D))
    for r, v in BAD.items():
        if r < n:
            eng.theta32[r] = float(v)
    eng.propose(min(2.38 / D ** 0.5, 0.9), 5.0)
    assert eng._direct_now and eng._step.no_fuse == 0
    eng._wait_pre_step()
    torch.cuda.synchronize()
    out = {k: getattr(eng, "p_" + k).cpu().numpy().copy() for k in ("u", "x", "logdetj", "fin", "logp", "u32")}
    out.update(host_x=np.array(eng._np_x, copy=True), host_fin=eng._np_fin.copy(), host_logp=eng._np_logp.copy(),
               clean=int(eng._np_clean[0]), cur_x=eng.x.cpu().numpy().copy())
    return out


def _alone(n, D, scaler, prior, u32):
    """scaler_inverse_kernel on the same u' (float32, as the flow leaves it)."""
    import torch
    from pocomc_amd import _lib
    lib = _lib.load()
    sd, pd = scaler.device_descriptor(), prior.device_descriptor()
    mk = lambda *s, dt=torch.float64: torch.empty(*s, dtype=dt, device="cuda")
    ud = torch.from_numpy(u32).cuda()
    uo, x, xT, ldj, fin, lp = mk(n, D), mk(n, D), mk(D, n), mk(n), mk(n, dt=torch.int32), mk(n)
    _lib.check(lib.pmc_scaler_inverse_prior(C.byref(sd), C.byref(pd), _lib.ptr(ud), None, _lib.ptr(uo), _lib.ptr(x),
                                            _lib.ptr(xT), _lib.ptr(ldj), _lib.ptr(fin), _lib.ptr(lp), None, None, None, n,
                                            _lib.stream_handle()), "pmc_scaler_inverse_prior")
    torch.cuda.synchronize()
    return dict(u=uo.cpu().numpy(), x=x.cpu().numpy(), xT=xT.cpu().numpy(), logdetj=ldj.cpu().numpy(),
                fin=fin.cpu().numpy(), logp=lp.cpu().numpy())


def _restated(scaler, bounds, periodic, reflective, transform, scale, u):
    """mcmc.py:91-97 in float64 numpy (oracle/scaler.py with the fitted affine part)."""
    from oracle.mcmc import _scaler_step
    from oracle.scaler import Reparameterize as OracleScaler
    o = OracleScaler(len(bounds), bounds=bounds, periodic=periodic, reflective=reflective, transform=transform, scale=scale)
    o.mu, o.sigma = scaler.mu.copy(), scaler.sigma.copy()
    with np.errstate(all="ignore"):
        return _scaler_step(o, u)


@pytest.mark.gpu
@pytest.mark.parametrize("scaler_kind", list(SCALERS))
@pytest.mark.parametrize("D", DS)
def test_fused_epilogue_and_scaler_launch_agree_and_follow_the_restatement(D, scaler_kind):
    import pocomc_amd as pc
    transform, scale = SCALERS[scaler_kind]
    flow = _flow(D)
    seen = dict(bad=0, outside=0, tail=0)
    for n in NS:
        plan = _plan(flow, n)
        if plan.sweep == 0 or not plan.epilogue:
            SKIPPED.append((D, scaler_kind, n))
            continue
        with_bc = (n in (16, 100)) == (transform == "probit")       # both transforms with and without, full and partial groups
        bounds, dists, periodic, reflective = _setup(D, with_bc)
        prior = pc.Prior(dists)
        rng = np.random.default_rng(1000 * D + n)
        scaler = pc.Reparameterize(D, bounds=bounds, periodic=periodic, reflective=reflective, transform=transform, scale=scale)
        scaler.fit(rng.uniform(-4, 4, size=(2000, D)))
        x = rng.uniform(-4, 4, size=(n, D))
        odd = np.arange(n) % 2 == 1                  # every other walker starts outside the support of feature WIDE
        x[odd, WIDE] = rng.uniform(5.5, 9.0, size=odd.sum()) * np.where(np.arange(odd.sum()) % 2, 1.0, -1.0)
        u = scaler.forward(x)
        a = _fused(n, D, flow, scaler, prior, x, u)
        b = _alone(n, D, scaler, prior, a["u32"])
        tag = (D, scaler_kind, n, with_bc)
        # ---- the two users of the element code: bit for bit
        for k in ("u", "x", "logdetj", "fin", "logp"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)
        fin = a["fin"] != 0
        clean = fin & np.isfinite(a["logp"])
        assert np.array_equal(a["host_fin"], a["fin"]) and np.array_equal(_bits(a["host_logp"]), _bits(a["logp"])), tag
        assert np.array_equal(_bits(b["xT"].T), _bits(b["x"])), tag                      # the launch's column-major copy
        assert np.array_equal(_bits(a["host_x"][clean]), _bits(a["x"][clean])), tag      # the epilogue's, in host memory
        assert np.array_equal(_bits(a["host_x"][~clean]), _bits(a["cur_x"][~clean])), tag     # (fill_rejected)
        assert a["clean"] == (~clean).sum(), tag
        for r in BAD:
            if r < n:
                assert not fin[r] and np.isneginf(a["logp"][r]), (tag, r)
        assert np.isneginf(a["logp"][~fin]).all(), tag
        seen["bad"] += int((~fin).sum())
        seen["outside"] += int((fin & ~clean).sum())
        # ---- against the float64 restatement, on the rows whose u' is finite
        ok = np.isfinite(a["u32"]).all(axis=1)
        assert not fin[~ok].any(), tag
        u64 = a["u32"][ok].astype(np.float64)
        ur, xr, ldjr = _restated(scaler, bounds, periodic, reflective, transform, scale, u64)
        np.testing.assert_allclose(a["x"][ok], xr, rtol=1e-12, atol=1e-12, err_msg=str(tag))
        np.testing.assert_allclose(a["u"][ok], ur, rtol=1e-11, atol=1e-11, err_msg=str(tag))
        if not with_bc:
            assert np.array_equal(_bits(a["u"][ok]), _bits(u64)), tag
        # (far tails: log(1 - p) with p -> 1 amplifies the last bit of exp, tests/test_gpu_tools.py: the looser bound there)
        t = np.abs(scaler.mu + scaler.sigma * u64 if scale else u64).max(axis=1)
        near = t < 5.0
        seen["tail"] += int((~near).sum())
        okf = fin[ok]
        np.testing.assert_allclose(a["logdetj"][ok][near & okf], ldjr[near & okf], rtol=1e-12, atol=1e-11, err_msg=str(tag))
        np.testing.assert_allclose(a["logdetj"][ok][~near & okf], ldjr[~near & okf], rtol=1e-9, atol=1e-9, err_msg=str(tag))
        # Prior.logpdf of the device's x', factor after factor (scipy), on the rows that have one
        xs = a["x"][fin]
        ref = np.zeros(len(xs))
        with np.errstate(all="ignore"):
            for j, d in enumerate(dists):
                ref += d.logpdf(xs[:, j])
        got = a["logp"][fin]
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)), tag
        m = np.isfinite(ref)
        np.testing.assert_allclose(got[m], ref[m], rtol=1e-13, atol=1e-13, err_msg=str(tag))
    assert seen["bad"] >= 6 and seen["outside"] >= 1, (D, scaler_kind, seen)


@pytest.mark.gpu
def test_no_listed_width_skips_the_fused_leg():
    """Runs behind the cases above (file order): the plan gives every listed D (all <= 64) the fused sweep with the epilogue."""
    assert [s for s in SKIPPED if s[0] <= 64] == [], SKIPPED
