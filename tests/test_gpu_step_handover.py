"""One pre-step through every hand-over mode of ``pmc_step_pre`` (``csrc/step.hip``: ``step_handover``): copies on the
stream (``x_order="C"``, ``"F"`` without ``host_direct``), the kernels writing pinned host memory without and with the
completion word -- each with the scaler as the fused sweep's epilogue (``PMC_NO_FUSE`` 0) and as a launch of its own (2), with
and without a device prior.  The device results do not depend on the mode, the host's x' carries the walkers' current x
exactly where the decision says so, and the "every row is clean" word is the count or -1 as ``pmc_step_t.h_clean`` documents:
in particular the fused epilogue counts without a device prior and the launch of its own does not.

The engine's word is -1 from its constructor on, so every run starts its pre-step from a stale value (``STALE``) instead:
where the step holds the word (the spinning runs) it must write the count or the -1 itself, and where it does not (every
other run: ``h_clean`` is not in the descriptor) it must leave the word alone -- there the -1 a caller reads is the engine's own.

D = 5 on the fused two-wave sweep, n = 21: one full 16-row workgroup and a partial one."""
import ctypes as C

import numpy as np
import pytest

D, N = 5, 21
BAD_ROW = 3              # its x' is made non-finite
STALE = 12345            # the clean word before the pre-step: no count of N rows and not -1
#        name              x_order  host_direct  spin_wait
MODES = {"C":             ("C",     False,       True),
         "F-copies":      ("F",     False,       True),
         "F-direct-wait": ("F",     True,        False),
         "F-direct-spin": ("F",     True,        True)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _pre_step(monkeypatch, mode, no_fuse, with_prior, flow, scaler, prior, x, u):
    import torch
    from pocomc_amd.mcmc import StepEngine
    x_order, host_direct, spin_wait = MODES[mode]
    monkeypatch.setenv("PMC_NO_FUSE", str(no_fuse))
    eng = StepEngine("preconditioned_pcn", N, D, flow, scaler, seed=9, x_order=x_order)
    eng.configure(host_direct=host_direct, spin_wait=spin_wait)
    if with_prior:
        assert eng.set_device_prior(prior)
    eng.load_state(u, x, scaler.inverse(u)[1], -0.5 * np.sum(x ** 2, axis=1), prior.logpdf(x))
    eng.set_geometry(mu=np.zeros(D), cov=np.eye(D))
    eng.theta32[BAD_ROW] = float("inf")                  # this walker's proposal, u' and x' are not finite
    assert int(eng._np_clean[0]) == -1                   # the engine's own "not known", which the non-spinning runs keep
    eng._np_clean[0] = STALE
    eng.propose(min(2.38 / D ** 0.5, 0.9), 5.0)          # (tpCN: sigma < 1)
    assert eng._step.no_fuse == no_fuse and eng._direct_now == (mode == "F-direct-spin")
    eng._wait_pre_step()
    torch.cuda.synchronize()
    out = dict(u=eng.p_u, x=eng.p_x, logdetj=eng.p_logdetj, finite=eng.p_fin, logp=eng.p_logp, cur_x=eng.x)
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out.update(host_x=np.array(eng._np_x, copy=True), clean=int(eng._np_clean[0]), fill=bool(eng._step.fill_rejected))
    return out


@pytest.mark.gpu
def test_every_hand_over_mode_of_one_pre_step(monkeypatch):
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import _lib
    flow = pc.Flow(D, "maf3", seed=0)
    plan = _lib.pmc_inverse_plan_t()
    assert _lib.load().pmc_maf_inverse_plan(C.byref(flow._desc), N, flow.inverse_algo, 1, C.byref(plan)) == 0
    assert (plan.sweep, plan.fused, plan.epilogue) == (4, 1, 1)          # the fused two-wave sweep with the scaler as epilogue
    # dimension 0: the scaler's box is twice the prior's support and every other walker starts outside the support (the
    # tpCN proposal contracts towards the centre, so some come back and some do not: logp' = -inf)
    prior = pc.Prior([uniform(-5, 10)] * D)
    bounds = np.array([[-10.0, 10.0]] + [[-5.0, 5.0]] * (D - 1))
    rng = np.random.default_rng(1000 * D + N)
    scaler = pc.Reparameterize(D, bounds=bounds, transform="probit", scale=True)
    scaler.fit(rng.uniform(-4, 4, size=(2000, D)))
    x = rng.uniform(-4, 4, size=(N, D))
    odd = np.arange(N) % 2 == 1
    x[odd, 0] = rng.uniform(5.5, 9.0, size=odd.sum()) * np.where(np.arange(odd.sum()) % 2, 1.0, -1.0)
    u = scaler.forward(x)
    for with_prior in (True, False):
        ref = None
        for mode in MODES:
            for no_fuse in (0, 2):
                key = (mode, no_fuse, with_prior)
                a = _pre_step(monkeypatch, mode, no_fuse, with_prior, flow, scaler, prior, x, u)
                if ref is None:
                    ref = a
                # the device results: one answer for every mode and both scaler paths
                for k in ("u", "x", "logdetj", "finite") + (("logp",) if with_prior else ()):
                    assert np.array_equal(_bits(a[k]), _bits(ref[k])), (k, key)
                fin = a["finite"] != 0
                assert not fin[BAD_ROW] and not np.isfinite(a["x"][BAD_ROW]).all()
                # the rows that reach the likelihood, as far as the device knows
                reach = fin & np.isfinite(a["logp"]) if with_prior else fin
                if with_prior:
                    assert (fin & ~reach).sum() >= 1, "no walker ended outside the prior's support"
                # the fill and the count: with the completion word, by the fused epilogue always, by the launch of its own
                # only with a device prior
                spin = mode == "F-direct-spin"
                counts = spin and (with_prior or no_fuse == 0)
                assert a["fill"] == spin
                filled = ~reach if counts else np.zeros(N, dtype=bool)
                assert np.array_equal(_bits(a["host_x"][~filled]), _bits(a["x"][~filled])), key
                assert np.array_equal(_bits(a["host_x"][filled]), _bits(a["cur_x"][filled])), key
                # the clean word: written by the step where it holds it -- the count, or -1 over the stale value -- and
                # untouched elsewhere (the engine's -1 stands there)
                assert a["clean"] == (int((~reach).sum()) if counts else -1 if spin else STALE), key
