"""The row stage of the fused sweeps' scaler epilogue (``csrc/scaler_body.h``: ``scaler_epilogue_rows``) serves a walker
with eight lanes: lane i keeps numpy's accumulator r_i of the pairwise sum of the Jacobian terms, the group combines them in
numpy's tree, one lane adds the tail; another lane walks ``Prior.logpdf``'s sequential sum.  The scaler launch of its own
(``pmc_scaler_inverse_prior``: one thread per row, ``np_pairwise_sum``) is the reference: the same pre-step with the scaler
fused (``no_fuse = 0``) and as a launch of its own (``no_fuse = 2``), every result bit for bit."""
import numpy as np
import pytest

DS = [3, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 50, 61, 64]
# D = 61 is the largest D the fused sweep reaches: the D - 1 degree groups take a quad of hidden slots each, and from 16 hidden
# tiles on (D >= 62) the lane sweep runs, with the scaler as a launch of its own -- at D = 64 the two sequences compared below
# are that one launch twice
FUSED_MAX_D = 61


# ------------------------------------------------------------------------------------------------------------------
# CPU: the eight-lane order is numpy's
# ------------------------------------------------------------------------------------------------------------------
def eight_lane_sum(a):
    """What the epilogue's lanes compute for one row of n <= 128 terms."""
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    n8 = n - n % 8
    r = [np.float64(a[i]) for i in range(8)]
    for i in range(8):                                   # lane i: a[i], a[i + 8], ... in index order
        for k in range(i + 8, n8, 8):
            r[i] = r[i] + a[k]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(n8, n):
        res = res + a[k]
    return res


@pytest.mark.parametrize("D", DS)
def test_the_eight_lane_order_is_numpys_pairwise_sum(D):
    rng = np.random.default_rng(D)
    rows = rng.normal(size=(200, D)) * np.exp(rng.normal(size=(200, D)) * 8.0)      # (terms of very different size: order shows)
    want = np.add.reduce(rows, axis=1)
    got = np.array([eight_lane_sum(r) for r in rows])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if D >= 8:
        naive = np.array([sum(r.tolist()) for r in rows])
        assert not np.array_equal(naive, want)              # (the rows can tell the orders apart)


# ------------------------------------------------------------------------------------------------------------------
# GPU: fused epilogue against the scaler launch
# ------------------------------------------------------------------------------------------------------------------
SCALERS = {"probit-scaled": dict(transform="probit", scale=True), "probit-unscaled": dict(transform="probit", scale=False),
           "logit-scaled": dict(transform="logit", scale=True)}
BAD_ROW = 3              # its x' is made non-finite


def _flow(D):
    import pocomc_amd as pc
    from pocomc_amd.maf_spec import MAFSpec
    # (the default width of D >= 43 has 16 hidden tiles, which the lane sweep takes: these keep the fused two-wave sweep
    #  and leave its epilogue the LDS it needs)
    hidden = {50: 160, 61: 60, 64: 208}.get(D)
    return pc.Flow(D, MAFSpec(D, 3, hidden) if hidden else "maf3", seed=0)


def _pre_step(monkeypatch, no_fuse, n, D, flow, scaler, prior, x, u):
    import torch
    from pocomc_amd.mcmc import StepEngine
    monkeypatch.setenv("PMC_NO_FUSE", str(no_fuse))
    eng = StepEngine("preconditioned_pcn", n, D, flow, scaler, seed=9, x_order="F")
    assert eng.set_device_prior(prior)
    eng.load_state(u, x, scaler.inverse(u)[1], -0.5 * np.sum(x ** 2, axis=1), prior.logpdf(x))
    eng.set_geometry(mu=np.zeros(D), cov=np.eye(D))
    eng.theta32[BAD_ROW] = float("inf")                  # this walker's proposal, u' and x' are not finite
    eng.propose(min(2.38 / D ** 0.5, 0.9), 5.0)          # (tpCN: sigma < 1)
    assert eng._direct_now and eng._step.no_fuse == no_fuse
    eng._wait_pre_step()
    torch.cuda.synchronize()
    out = dict(u=eng.p_u, x=eng.p_x, logdetj=eng.p_logdetj, finite=eng.p_fin, logp=eng.p_logp, u32=eng.p_u32,
               ldjf=eng.p_ldjf, theta=eng.p_theta64)
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out.update(host_x=np.array(eng._np_x, copy=True), host_finite=eng._np_fin.copy(), host_logp=eng._np_logp.copy(),
               clean=eng._np_clean.copy(), done=eng.h_done.numpy().copy(), cur_x=eng.x.cpu().numpy().copy())
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.gpu
@pytest.mark.parametrize("scaler_kind", list(SCALERS))
@pytest.mark.parametrize("D", DS)
def test_fused_epilogue_rows_equal_the_scaler_launch_bit_for_bit(D, scaler_kind, monkeypatch):
    import ctypes
    from scipy.stats import uniform, norm
    import pocomc_amd as pc
    from pocomc_amd import _lib
    flow = _flow(D)
    assert _lib.load().pmc_maf_inverse_auto_is_lane(ctypes.byref(flow._desc)) == (0 if D <= FUSED_MAX_D else 1)
    if D <= FUSED_MAX_D:
        assert _lib.load().pmc_maf_inverse_auto_is_duo(ctypes.byref(flow._desc), 16) == 1
    seen_bad = seen_out = 0
    for prior_kind in ("uniform", "normal"):
        # dimension 0: the scaler's box is twice the prior's support and every other walker starts outside the support (the
        # tpCN proposal contracts towards the centre, so some come back and some do not: logp' = -inf); the normal factors
        # sit on unbounded dimensions
        if prior_kind == "uniform":
            prior = pc.Prior([uniform(-5, 10)] * D)
            bounds = np.array([[-10.0, 10.0]] + [[-5.0, 5.0]] * (D - 1))
        else:
            prior = pc.Prior([uniform(-5, 10)] + [norm(0.5, 2.0)] * (D - 1))
            bounds = np.array([[-10.0, 10.0]] + [[-np.inf, np.inf]] * (D - 1))
        for n in (16, 21):
            rng = np.random.default_rng(1000 * D + n)
            scaler = pc.Reparameterize(D, bounds=bounds, **SCALERS[scaler_kind])
            scaler.fit(rng.uniform(-4, 4, size=(2000, D)))
            x = rng.uniform(-4, 4, size=(n, D))
            odd = np.arange(n) % 2 == 1                   # (every other walker starts outside the support, on either side)
            x[odd, 0] = rng.uniform(5.5, 9.0, size=odd.sum()) * np.where(np.arange(odd.sum()) % 2, 1.0, -1.0)
            u = scaler.forward(x)
            a = _pre_step(monkeypatch, 0, n, D, flow, scaler, prior, x, u)
            b = _pre_step(monkeypatch, 2, n, D, flow, scaler, prior, x, u)
            for k in a:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, prior_kind, n)
            # what the rows went through
            fin = a["finite"] != 0
            out = fin & ~np.isfinite(a["logp"])
            assert not fin[BAD_ROW] and not np.isfinite(a["x"][BAD_ROW]).all()
            assert np.isneginf(a["logp"][~fin]).all()
            assert a["clean"][0] == (~fin | out).sum() and a["done"][0] == 1
            assert np.array_equal(a["host_x"][~fin | out], a["cur_x"][~fin | out])          # fill_rejected
            assert np.array_equal(a["host_x"][fin & ~out], a["x"][fin & ~out])
            assert np.array_equal(a["host_finite"], a["finite"]) and np.array_equal(_bits(a["host_logp"]), _bits(a["logp"]))
            seen_bad += int((~fin).sum())
            seen_out += int(out.sum())
    assert seen_bad >= 4 and seen_out >= 1, (seen_bad, seen_out)
