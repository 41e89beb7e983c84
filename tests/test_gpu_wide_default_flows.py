"""Default-width flows at n_dim >= 86 in float32 (H = 512 by the reference's width rule, ``flow.py:52``): the LEAN instances
of the forward / D-pass workgroup kernel (``csrc/maf_forward_wg.hip``) and of the trainer's chain kernel
(``csrc/maf_train.hip``), which keep two hidden-width activation arrays of 16 rows in LDS where the full ones keep three
and four, and the inverse plan's fallback to the lean D-pass kernel (``csrc/inverse_plan.hip``).

D = 86 is the first width the full instances refuse, 102 has the largest padded hidden width (Hp = 816, Dp = 112), 128 is
the BASELINE config-5 width whose spline training did not fit, 157 the widest MCMC step (Dp = 160).  T = 2: both feature
orders.  (a) lean == full bit for bit on small flows, forced by ``PMC_MAF_VARIANT_LEAN_LDS`` (``Flow.lean_lds``); (b)
forward / log_prob / AUTO's inverse against the oracle with the measures and tolerances of ``tests/test_gpu_flow.py``; (c)
loss and gradient against torch autograd on the oracle twin with the tolerances of ``tests/test_gpu_train.py``; (d) a fit
and a default ``Sampler`` run at D = 100."""
import functools

import numpy as np
import pytest
import torch

import cases
from oracle.maf import OracleMAF, torch_loss
from parity import close_rel, TOL
from pocomc_amd.maf_spec import MAFSpec, spec_by_name

pytestmark = pytest.mark.gpu

WIDE = (86, 102, 128, 157)
FAMILIES = ("affine", "rqs")
NSF_FWD, NSF_INV, NSF_LADJ = 2e-5, 5e-5, 1e-4        # tests/test_gpu_flow.py
S_LANE, S_NSF_SOLO, S_DPASS_LEAN = 5, 6, 8


@functools.lru_cache(maxsize=None)
def wide(D, uni):
    """One flow per (D, family) for the whole module: (Flow, spec, parameters, float32 oracle)."""
    from pocomc_amd import Flow
    spec = MAFSpec(D, 2, univariate=uni)
    assert spec.hidden == 512
    flat = cases.flow_params(spec, 3, gain=1.0)
    f = Flow(D, spec)
    f.set_params(flat)
    return f, spec, flat, OracleMAF(spec, flat)


def auto_sweep(f, n):
    import ctypes as C
    from pocomc_amd import _lib
    p = _lib.pmc_inverse_plan_t()
    _lib.check(f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, 0, 0, C.byref(p)))
    return p.sweep


# ------------------------------------------------------------------------------------------ which instance runs
def test_the_wide_flows_take_the_instances_the_plan_names():
    got = {(D, uni): {k: v[0] for k, v in wide(D, uni)[0].lds_plan().items()} for D in WIDE for uni in FAMILIES}
    L, F = "lean", "full"
    assert {k: v["train"] for k, v in got.items()} == {(86, "affine"): L, (102, "affine"): L, (128, "affine"): F, (157, "affine"): L,
                                                       (86, "rqs"): L, (102, "rqs"): L, (128, "rqs"): L, (157, "rqs"): L}
    assert {k: v["forward"] for k, v in got.items()} == {(86, "affine"): F, (102, "affine"): L, (128, "affine"): F, (157, "affine"): F,
                                                         (86, "rqs"): L, (102, "rqs"): L, (128, "rqs"): F, (157, "rqs"): L}
    for uni in FAMILIES:
        assert auto_sweep(wide(102, uni)[0], 33) == S_DPASS_LEAN
    assert auto_sweep(wide(128, "affine")[0], 33) == S_LANE and auto_sweep(wide(128, "rqs")[0], 33) == S_NSF_SOLO


# ------------------------------------------------------------------------------------------ (a) lean == full, bit for bit
@pytest.mark.parametrize("name", ["maf3", "nsf3"])
@pytest.mark.parametrize("D", [10, 32])
def test_forced_lean_instances_equal_the_full_ones_bit_for_bit(name, D):
    """``Flow.lean_lds`` forces the two-array instances on flows that fit both.  The lean forward kernel writes h2 over h0 and
    the lean trainer reads the relu' masks' operands from the scratch instead of LDS: the same operations in the same order,
    so z, the log-determinant, log_prob, the D-pass inverse, the loss and every gradient entry are the same bits.  (These
    small flows also take the trainer's partial-tile staging, which the wide ones do not.)  The affine flows' D-pass
    algorithm has no full instance of the workgroup kernel to compare with -- theirs is the lone-wave kernel, which adds a
    row's log-determinant in another order: held to the oracle tolerance of ``tests/test_gpu_flow.py`` instead."""
    from pocomc_amd import Flow
    from pocomc_amd.train import loss_and_grad, _train_state
    spec = spec_by_name(D, name)
    f = Flow(D, spec)
    f.set_params(cases.flow_params(spec, 7, gain=1.0))
    assert {v[0] for v in f.lds_plan().values()} == {"full"}
    _train_state(f).repack(f)
    rng = np.random.default_rng(D)

    def run(n):
        x = torch.from_numpy((rng.normal(size=(n, D)) * 2.0).astype(np.float32))
        w = torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32))
        out = {}
        for lean in (False, True):
            f.lean_lds = lean
            assert {v[0] for v in f.lds_plan().values()} == {"lean" if lean else "full"}
            z, ladj = f.forward(x)
            f.inverse_algo = 2                                   # the D-pass algorithm
            xi, li = f.inverse(z)
            f.inverse_algo = 0
            grads = []
            for wb in (None, w):
                loss = float(loss_and_grad(f, x.cuda(), None if wb is None else wb.cuda()))
                grads += [loss, f._train.grad.cpu().numpy().copy()]
            out[lean] = [z.numpy(), ladj.numpy(), f.log_prob(x).numpy(), xi.numpy(), li.numpy()] + grads
        f.lean_lds = False
        return out

    for n in (1, 17, 40):
        out = run(n)
        names = ("z", "ladj", "log_prob", "x (D-pass)", "ladj (D-pass)", "loss", "gradient", "weighted loss", "weighted gradient")
        for what, a, b in zip(names, out[False], out[True]):
            if name == "maf3" and "D-pass" in what:
                close_rel(b, a, TOL, f"lean D-pass vs lone-wave D-pass, {what}",
                          cancel=None if what.startswith("x") else OracleMAF(spec, f.params.cpu().numpy()).ladj_abs_terms(out[False][3]))
            else:
                assert np.array_equal(np.asarray(a), np.asarray(b)), (what, n)
        assert np.abs(out[True][6]).max() > 0 and np.isfinite(out[True][5])


# ------------------------------------------------------------------------------------------ (b) against the oracle
@pytest.mark.parametrize("uni", FAMILIES)
@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("n", [1, 33])
def test_forward_and_log_prob_match_the_oracle(D, uni, n):
    f, spec, flat, o = wide(D, uni)
    x = (np.random.default_rng(n + D).normal(size=(n, D)) * (2.5 if uni == "rqs" else 1.5)).astype(np.float32)
    z, ladj = f.forward(torch.from_numpy(x))
    zo, lo = o.forward(x)
    terms = o.ladj_abs_terms(x)
    tz, tl = (NSF_FWD, NSF_LADJ) if uni == "rqs" else (TOL, TOL)
    base = 0.5 * (zo.astype(np.float64) ** 2).sum(axis=1) + 0.5 * D * np.log(2 * np.pi)
    lp = f.log_prob(torch.from_numpy(x)).numpy()
    print(f"wide forward D={D} {uni} n={n}: z {close_rel(z.numpy(), zo, np.inf, 'wide z (measured)'):.2e} "
          f"ladj {close_rel(ladj.numpy(), lo, np.inf, 'wide ladj (measured)', cancel=terms):.2e} "
          f"log_prob {close_rel(lp, o.log_prob(x), np.inf, 'wide log_prob (measured)', cancel=terms + base):.2e}")
    close_rel(z.numpy(), zo, tz, "wide z")
    close_rel(ladj.numpy(), lo, tl, "wide ladj", cancel=terms)
    close_rel(lp, o.log_prob(x), tl, "wide log_prob", cancel=terms + base)


@pytest.mark.parametrize("uni", FAMILIES)
@pytest.mark.parametrize("D", [102, 128])
@pytest.mark.parametrize("n", [1, 33])
def test_auto_inverse_matches_the_oracles_dpass(D, uni, n):
    """D = 102: no sweep fits, AUTO falls back to the lean D-pass kernel; D = 128: the lane-per-walker / lone-wave spline
    sweep, as before."""
    f, spec, flat, o = wide(D, uni)
    assert auto_sweep(f, n) == (S_DPASS_LEAN if D == 102 else S_LANE if uni == "affine" else S_NSF_SOLO)
    z = (np.random.default_rng(7 + n + D).normal(size=(n, D)) * (1.5 if uni == "rqs" else 1.2)).astype(np.float32)
    xo, lo = o.inverse(z)                                    # the reference's D-pass algorithm
    terms = o.ladj_abs_terms(xo)
    x, l = f.inverse(torch.from_numpy(z))
    tx, tl = (NSF_INV, NSF_LADJ) if uni == "rqs" else (TOL, TOL)
    print(f"wide inverse D={D} {uni} n={n}: x {close_rel(x.numpy(), xo, np.inf, 'wide x (measured)'):.2e} "
          f"ladj {close_rel(l.numpy(), lo, np.inf, 'wide ladj inverse (measured)', cancel=terms):.2e}")
    close_rel(x.numpy(), xo, tx, "wide x, AUTO")
    close_rel(l.numpy(), lo, tl, "wide ladj inverse, AUTO", cancel=terms)


# ------------------------------------------------------------------------------------------ (c) against autograd
@pytest.mark.parametrize("uni", FAMILIES)
@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("n", [5, 40])
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_and_gradient_match_autograd(D, uni, n, weighted):
    from pocomc_amd.train import loss_and_grad, _train_state
    f, spec, flat, _ = wide(D, uni)
    rng = np.random.default_rng(n + D)
    x = (rng.normal(size=(n, D)) * (2.5 if uni == "rqs" else 1.3)).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    ft = torch.tensor(flat, requires_grad=True)
    lo = torch_loss(spec, ft, torch.from_numpy(x), None if w is None else torch.from_numpy(w))
    lo.backward()
    g_ref = ft.grad.numpy()
    _train_state(f).repack(f)
    loss = loss_and_grad(f, torch.from_numpy(x).cuda(), None if w is None else torch.from_numpy(w).cuda())
    g = f._train.grad.cpu().numpy()
    scale = np.abs(g_ref).max()
    rtol, atol = (2e-3, 1e-4 * scale) if uni == "rqs" else (1e-3, 5e-5 * scale)
    excess = (np.abs(g - g_ref) - rtol * np.abs(g_ref)).max() / scale
    print(f"wide gradient D={D} {uni} n={n} weighted={weighted}: loss rel {abs(float(loss) - float(lo.detach())) / abs(float(lo.detach())):.2e}, "
          f"max (|g - g_ref| - rtol |g_ref|) / max|g_ref| {excess:.2e} (allowed {atol / scale:.0e})")
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=5e-5)
    np.testing.assert_allclose(g, g_ref, rtol=rtol, atol=atol)
    assert not g[spec.mask_flat() == 0].any()                # masked weights never receive gradient


# ------------------------------------------------------------------------------------------ (d) end to end
def test_fit_and_round_trip_at_100_dimensions():
    from pocomc_amd import Flow
    torch.manual_seed(0)
    D = 100
    data = torch.randn(256, D) * 1.5
    flow = Flow(D, "maf6", seed=1)
    assert flow.lds_plan()["train"][0] == "lean" and flow.lds_plan()["forward"][0] == "lean"
    hist = flow.fit(data, epochs=3)
    assert len(hist["loss"]) == 3 and np.isfinite(hist["loss"]).all()
    z, _ = flow.forward(data)
    x, _ = flow.inverse(z)
    assert torch.isfinite(z).all()
    np.testing.assert_allclose(x.numpy(), data.numpy(), rtol=0, atol=1e-4)


def test_default_sampler_runs_at_100_dimensions():
    """``pc.Sampler(prior, likelihood)`` with its default flow (nsf6, H = 512) on a 100-dimensional problem: a likelihood so
    broad that beta reaches 1 in the first iterations, so the run is a warm-up, a few flow fits and preconditioned steps."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    D = 100

    def loglike(x):
        return -0.5 * np.sum((x / 50.0) ** 2, axis=1)

    prior = pc.Prior([uniform(-10, 20)] * D)
    s = pc.Sampler(prior=prior, likelihood=loglike, vectorize=True, n_active=64, n_effective=128, n_steps=1, n_max_steps=2,
                   train_config=dict(epochs=3), random_state=0)
    assert s.flow.spec.hidden == 512 and s.flow.spec.univariate == "rqs" and s.flow.spec.n_transforms == 6
    before = s.flow.params.cpu().numpy().copy()
    s.run(n_total=128, n_evidence=0, progress=False)
    assert float(s.particles.get("beta", index=-1)) == 1.0
    x, w, logl, logp = s.posterior()
    assert x.shape[1] == D and np.isfinite(x).all() and np.isfinite(w).all() and np.isfinite(logl).all() and np.isfinite(logp).all()
    assert not np.array_equal(s.flow.params.cpu().numpy(), before)
