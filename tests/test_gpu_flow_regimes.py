"""The flow kernels on TRAINED flows, on flows whose output layer is scaled up (the soft clip's ceiling), and at the
spline's edges, against the float64 oracle under the sensitivity criterion of ``tests/flow_regimes.py`` (``C`` = 16, the
median ``err/e`` <= 2, the suite's existing bounds as the floor).

* forward / log_prob and every inverse sweep the spec admits, on data rows, latent rows and the edge rows (inputs on the
  oracle's float32 knots and one ulp either side, +-5.0f and its neighbours, the ulp band between the computed end knot
  and 5.0f -- where a kernel may take either side: the criterion holds it to the oracle there);
* coordinates well outside the spline box come back bit-for-bit, with an exact zero log-determinant where the whole row is
  outside;
* rows with NaN / +-inf leave every other row of the batch bit-identical (same n: AUTO picks its sweep by n);
* loss and gradient of the trainer against float64 autograd, per parameter block, with the float32 twin's error as the
  envelope.

Flows trained here: ``Flow.fit`` with fixed seeds and data, 50 epochs like ``bench.py`` (config 5's flow: 10).  Where a
float32 evaluation of the same rows -- the numpy oracle, the same with sequential dot products (D <= 10), the kernels'
spline formulas -- fails the row criterion on some rows (tests/test_flow_regimes_cpu.py shows where: the inverse at gain
x4 / x16), the kernel is held to be as good a float32 evaluation as those (``check``).  The median bound follows the float32
evaluations of the same rows: the numpy oracle and, for spline flows, ``KernelSplineOracle`` -- the kernels' spline
formulas in float32 (reciprocals, exp2 of a rounded product, running-sum knots), whose median on a trained nsf6 inverse is
~1.9 against numpy's 1.5 (tests/test_flow_regimes_cpu.py): the kernels' ~2.0 there comes from those formulas."""
import functools

import numpy as np
import pytest
import torch

import flow_regimes as fr
import parity
from oracle.maf import OracleMAF, torch_loss
from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu

FITTED = {
    # name: spec, training rows
    "maf3-d10-fit": (lambda: MAFSpec(10, 3), lambda: fr.rosenbrock_draws(10, 2000, 1)),
    "maf3-d32-fit": (lambda: MAFSpec(32, 3), lambda: fr.rosenbrock_draws(32, 4000, 2)),
    "nsf6-d10-fit": (lambda: MAFSpec(10, 6, univariate="rqs"), lambda: fr.two_modes(10, 2000, 3)),
    "nsf3-d32-fit": (lambda: MAFSpec(32, 3, univariate="rqs"), lambda: fr.rosenbrock_draws(32, 4000, 4)),
    "maf6-d50-fit": (lambda: MAFSpec(50, 6), lambda: fr.bimodal_draws(50, 4000, 5)),
    "maf8-d128-fit": (lambda: MAFSpec(128, 8), lambda: config5_rows()),          # config 5: H = 512
}
EPOCHS = {"maf8-d128-fit": 10}      # config 5's validation loss is best near epoch 5 and diverges by 50 (bench.py)


# OPEN FINDING (asserted failing, test_open_finding_*): the on-device D-pass inverse (algorithm 2, the cross-check kernel;
# AUTO never takes it for these flows) on the affine flow with its output layer x16 misses C e_i on the inverse
# log-determinant on 15 of 192 rows (worst 0.09), where float32 evaluations in two other orders of addition miss up to 6
# (worst 0.09): the same magnitude, more than twice the rows.  Not explained yet.
OPEN_FINDINGS = {("maf3-d10-g16", 2)}


def config5_rows():
    """scripts/config5_flow_health.py: 5000 logit-transformed U(-30, 30) draws at D = 128."""
    from pocomc_amd import Reparameterize
    D = 128
    x = np.random.default_rng(7).uniform(-30.0, 30.0, size=(10000, D))
    sc = Reparameterize(D, bounds=np.array([[-30.0, 30.0]] * D))
    sc.fit(x)
    return np.asarray(sc.forward(x[:5000]), np.float32)
GAIN = {"maf3-d10-g4": (lambda: MAFSpec(10, 3), 4.0), "maf3-d10-g16": (lambda: MAFSpec(10, 3), 16.0),
        "nsf6-d10-g4": (lambda: MAFSpec(10, 6, univariate="rqs"), 4.0)}
FIXTURES = list(FITTED) + list(GAIN)
ROWS = {10: (384, 192), 32: (256, 96), 50: (256, 96), 128: (64, 8)}          # forward / inverse rows per D (float64 D-pass cost)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(spec, float32 parameters, data rows)."""
    from pocomc_amd import Flow
    if name in GAIN:
        mk, g = GAIN[name]
        spec = mk()
        return spec, fr.gain_params(spec, g), fr.two_modes(spec.n_dim, 1000, 9) * np.float32(1.3)
    mk, data = FITTED[name]
    spec, x = mk(), data()
    torch.manual_seed(0)
    f = Flow(spec.n_dim, spec, seed=0)
    f.fit(torch.from_numpy(x), epochs=EPOCHS.get(name, 50), batch_size=512, validation_split=0.5, patience=spec.n_dim, annealing=False, verbose=0)
    flat = f.params.cpu().numpy().astype(np.float32)
    assert np.isfinite(flat).all() and not np.array_equal(flat, spec.init_params(0))
    return spec, flat, x


def flow(spec, flat):
    from pocomc_amd import Flow
    f = Flow(spec.n_dim, spec, seed=0)
    f.set_params(flat)
    return f


def algorithms(spec):
    """Every inverse the spec admits (tests/test_gpu_flow.py), AUTO first."""
    if not spec.tri_ok:
        return [0, 2]
    if spec.univariate == "rqs":
        return [0, 1, 2, 6, 7]
    small = spec.nOT <= 8 and 2 * spec.Dp + 3 * spec.Hp + 176 <= 2560
    return [0, 1, 2, 8] + ([6, 7] if small else [])


def forward_inputs(spec, flat, data):
    n = ROWS[spec.n_dim][0]
    x = data[np.random.default_rng(11).choice(len(data), n, replace=False)]
    parts = [x]
    if spec.univariate == "rqs":
        parts += [fr.knot_rows(spec, flat, x)[0], fr.all_knot_rows(spec, flat, x[:16])[0], fr.box_rows(spec, flat, x)[0]]
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


def inverse_inputs(spec, flat, data, f):
    n = ROWS[spec.n_dim][1]
    rng = np.random.default_rng(12)
    x = data[rng.choice(len(data), n // 2, replace=False)]
    z = np.concatenate([f.forward(torch.from_numpy(x))[0].numpy(),                    # latent images of the flow's own rows
                        (rng.normal(size=(n - n // 2, spec.n_dim)) * 1.2).astype(np.float32)])
    parts = [z]
    if spec.univariate == "rqs":
        parts += [fr.knot_rows(spec, flat, z, inverse=True)[0], fr.box_rows(spec, flat, z, inverse=True)[0]]
    return np.ascontiguousarray(np.concatenate(parts), np.float32)


def check(R, q, got, what, f32):
    """The criterion on ``got``.  ``f32``: float32 evaluations of the same rows (numpy oracle first).  Where one of them
    fails the row criterion, the quantity is ill-conditioned beyond the envelope on these rows (tests/test_flow_regimes_cpu.py:
    BEYOND_F32), and WHICH rows a float32 evaluation misses depends on its order of additions (numpy and the sequential
    oracle miss different rows of the affine x16 inverse by the same ~0.12).  There the kernel is held to be as good a
    float32 evaluation as those: at most twice as many rows beyond ``C e_i`` as the worst of them, a worst error at most
    twice theirs, and the median criterion on the rows every evaluation meets."""
    lim = np.maximum(fr.bounds(R.spec)[q], fr.C * R.env[q])
    bad = [R.ok & ~(R.err(q, v) <= lim) for v in f32]
    beyond = np.logical_or.reduce(bad)
    if not beyond.any():
        s = R.check(q, got, what, f32=f32)
    else:
        held = np.flatnonzero(~beyond)
        s = R.check(q, got, what, rows=held, f32=f32, raise_=False)
        assert s["median_ratio"] <= s["median_bound"], (what, q, s)
        err = R.err(q, got)
        bad_k = R.ok & ~(err <= lim)
        n_e = max(int(b.sum()) for b in bad)
        worst_e = max(float(R.err(q, v)[b].max()) for v, b in zip(f32, bad) if b.any())
        worst_k = float(err[bad_k].max()) if bad_k.any() else 0.0
        key = f"{what.split(',')[0]} {q} rows beyond C e (kernel / float32)"
        print(f"{what} {q}: beyond C e_i on {int(bad_k.sum())} rows (worst err {worst_k:.3g}); float32 evaluations: up to "
              f"{n_e} rows (worst err {worst_e:.3g})")
        parity.MEASURED[key] = max(parity.MEASURED.get(key, 0.0), float(bad_k.sum()))
        assert bad_k.sum() <= 2 * n_e and worst_k <= 2 * worst_e, (what, q, int(bad_k.sum()), n_e, worst_k, worst_e)
    print(f"{what} {q}: worst err/e {s['worst_ratio']:.3g}, median {s['median_ratio']:.3g} (bound {s['median_bound']:.3g}), "
          f"worst err {s['worst']:.2e}, well-conditioned rows {s['worst_well']:.2e}")


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_log_prob_and_every_inverse_meet_the_criterion(name, only_algo=None):
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    o = OracleMAF(spec, flat)
    k = fr.KernelSplineOracle(spec, flat) if spec.univariate == "rqs" else None
    seq = fr.SequentialOracle(spec, flat) if spec.n_dim <= 10 else None          # (python loop per term: small flows only)
    x = forward_inputs(spec, flat, data)
    kp = min(fr.N_PERTURB, 4) if spec.n_dim >= 128 else fr.N_PERTURB          # (float64 D-pass cost at D = 128)
    R = fr.Reference(spec, flat, x, "forward", k=kp)
    z, l = (t.numpy() for t in f.forward(torch.from_numpy(x)))
    lp = f.log_prob(torch.from_numpy(x)).numpy()
    ev = [o] + [e for e in (k, seq) if e is not None]
    f32 = [dict(zip(("z", "ladj"), e.forward(x)), log_prob=e.log_prob(x)) for e in ev]
    for q, v in (("z", z), ("ladj", l), ("log_prob", lp)):
        check(R, q, v, f"forward, {name}", [d[q] for d in f32])
    u = inverse_inputs(spec, flat, data, f)
    R = fr.Reference(spec, flat, u, "inverse", k=kp)
    f32 = [dict(zip(("x", "ladj"), e.inverse(u))) for e in ev]
    for algo in algorithms(spec):
        if (only_algo is None) == ((name, algo) in OPEN_FINDINGS) or (only_algo is not None and algo != only_algo):
            continue
        f.inverse_algo = algo
        xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(u)))
        fam = f"inverse algorithm {algo}" if algo else "inverse AUTO"
        check(R, "x", xi, f"{fam}, {name}", [d["x"] for d in f32])
        check(R, "ladj", li, f"{fam}, {name}", [d["ladj"] for d in f32])


@pytest.mark.xfail(strict=True, reason="open finding: see OPEN_FINDINGS")
@pytest.mark.parametrize("name,algo", sorted(OPEN_FINDINGS))
def test_open_finding_the_criterion_on_the_listed_inverses(name, algo):
    """The listed (flow, inverse algorithm) pairs fail the criterion today; strict: the test fails once they meet it, so
    that the list stays true."""
    test_forward_log_prob_and_every_inverse_meet_the_criterion(name, only_algo=algo)


@pytest.mark.parametrize("name", [n for n in FIXTURES if n.startswith("nsf")])
def test_coordinates_outside_the_spline_box_come_back_bit_for_bit(name):
    """The spline is the identity outside its box in every transform, so a coordinate with |x| well beyond both the computed
    end knot and 5.0f (>= 5.0001) passes every transform unchanged: bit-for-bit from the forward and from every inverse,
    and a row that is outside in every coordinate has a log-determinant of exactly zero."""
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    x, out = fr.outside_rows(spec, data[:64])
    allout = out.all(axis=1)
    assert allout.sum() >= 4
    z, l = (t.numpy() for t in f.forward(torch.from_numpy(x)))
    np.testing.assert_array_equal(z[out], x[out])
    np.testing.assert_array_equal(l[allout], 0.0)
    for algo in algorithms(spec):
        f.inverse_algo = algo
        xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(x)))
        np.testing.assert_array_equal(xi[out], x[out], err_msg=f"algorithm {algo}")
        np.testing.assert_array_equal(li[allout], 0.0, err_msg=f"algorithm {algo}")


@pytest.mark.parametrize("name", ["maf3-d10-fit", "maf3-d32-fit", "nsf6-d10-fit", "nsf3-d32-fit", "maf6-d50-fit", "maf3-d10-g16"])
@pytest.mark.parametrize("n", [64, 4096])
def test_non_finite_rows_stay_in_their_rows(name, n):
    """NaN / +inf / -inf in one coordinate of rows 0, 15, 16, 17 and n-1: every other row is bit-identical to the same batch
    with those rows finite, for the forward, log_prob, AUTO and every inverse (same n: AUTO picks its sweep by n)."""
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    good = data[np.random.default_rng(n).choice(len(data), n, replace=n > len(data))]
    f.inverse_algo = 0
    lat = f.forward(torch.from_numpy(good))[0].numpy()
    for what, base in (("forward", good), ("inverse", lat)):
        bad, rows = fr.with_nonfinite(base)
        keep = np.setdiff1d(np.arange(n), rows)
        runs = [("forward", None), ("log_prob", None)] if what == "forward" else [("inverse", a) for a in algorithms(spec)]
        for kind, algo in runs:
            res = []
            for inp in (base, bad):
                t = torch.from_numpy(np.ascontiguousarray(inp))
                if kind == "forward":
                    res.append([v.numpy() for v in f.forward(t)])
                elif kind == "log_prob":
                    res.append([f.log_prob(t).numpy()])
                else:
                    f.inverse_algo = algo
                    res.append([v.numpy() for v in f.inverse(t)])
            for a, b in zip(*res):
                np.testing.assert_array_equal(b[keep], a[keep], err_msg=f"{name} n={n} {kind} algorithm {algo}")
    f.inverse_algo = 0


def _blocks(spec):
    for t in range(spec.n_transforms):
        for name, (off, sz) in spec.offsets.items():
            b = t * spec.params_per_transform + off
            yield f"t{t}.{name}", slice(b, b + sz)


@pytest.mark.parametrize("name", ["maf3-d10-fit", "nsf6-d10-fit", "maf3-d10-g4", "nsf6-d10-g4"])
@pytest.mark.parametrize("n", [5, 100, 512])
@pytest.mark.parametrize("weighted", [False, True])
def test_trainer_loss_and_gradient_per_block(name, n, weighted):
    """``pmc_maf_loss_grad`` (and the chain / dW kernels behind it) on a trained or gain-4 flow against float64 autograd
    of ``torch_loss``.  Per parameter block (``max |g - g64| / max |g64|``) and the loss (against ``sum |log_prob|``):
    ``err <= max(2e-5, C e)`` with ``e`` the float32 twin's error.  Spline flows: a quarter of the rows sit on the
    oracle's knots for the LOSS; the gradient is taken on rows off the knots, because the loss is not differentiable in
    the spline's parameters there -- the two one-sided gradients differ (measured: 1e-2 of the block t0.b3) and which one
    a float32 evaluation returns depends on which side of its own rounded knot the input falls."""
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    rng = np.random.default_rng(n + 31 * weighted)
    x = np.ascontiguousarray(data[rng.choice(len(data), n, replace=False)], np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    batches = [(x, True)]
    if spec.univariate == "rqs":
        batches.append((np.ascontiguousarray(np.concatenate([fr.knot_rows(spec, flat, x)[0][: max(n // 4, 1)], x])[:n]), False))
    for xb, grad in batches:
        _loss_and_gradient(spec, flat, f, xb, w, grad, f"trainer, {name} n={n} w={int(weighted)}{'' if grad else ' knots'}")


def _loss_and_gradient(spec, flat, f, x, w, grad, tag):
    from pocomc_amd.train import loss_and_grad, _train_state
    ref = {}
    for dt in (torch.float64, torch.float32):
        ft = torch.tensor(flat.astype(np.float64) if dt == torch.float64 else flat, dtype=dt, requires_grad=True)
        lo = torch_loss(spec, ft, torch.from_numpy(x).to(dt), None if w is None else torch.from_numpy(w).to(dt))
        lo.backward()
        ref[dt] = (float(lo.detach()), ft.grad.double().numpy())
        if dt == torch.float64:
            from oracle.maf import torch_log_prob
            lp_abs = float(torch_log_prob(spec, ft.detach(), torch.from_numpy(x).double()).abs().sum())
            if w is not None:
                lp_abs *= 1000.0 * float(w.max()) / float(w.sum())
    _train_state(f).repack(f)
    loss = float(loss_and_grad(f, torch.from_numpy(x).cuda(), None if w is None else torch.from_numpy(w).cuda()))
    g = f._train.grad.cpu().double().numpy()
    (l64, g64), (l32, g32) = ref[torch.float64], ref[torch.float32]
    el, e32 = abs(loss - l64) / max(abs(l64), lp_abs), abs(l32 - l64) / max(abs(l64), lp_abs)
    assert el <= max(fr.TRAIN_BOUND, fr.C * e32), f"{tag} loss: {el:.3e} > max({fr.TRAIN_BOUND}, {fr.C} x {e32:.3e})"
    parity.MEASURED["trainer loss err"] = max(parity.MEASURED.get("trainer loss err", 0.0), el)
    if not grad:
        print(f"{tag}: loss err {el:.2e} (twin {e32:.2e})")
        return
    worst, worst_ratio = 0.0, 0.0
    for blk, sl in _blocks(spec):
        s = max(np.abs(g64[sl]).max(), fr.TINY)
        eb, eb32 = np.abs(g[sl] - g64[sl]).max() / s, np.abs(g32[sl] - g64[sl]).max() / s
        assert eb <= max(fr.TRAIN_BOUND, fr.C * eb32), f"{tag} gradient block {blk}: {eb:.3e} > max({fr.TRAIN_BOUND}, {fr.C} x {eb32:.3e})"
        worst, worst_ratio = max(worst, eb), max(worst_ratio, eb / max(eb32, fr.EPS))
    for key, v in (("trainer gradient err/e", worst_ratio), ("trainer gradient err", worst)):
        parity.MEASURED[key] = max(parity.MEASURED.get(key, 0.0), v)
    print(f"{tag}: loss err {el:.2e} (twin {e32:.2e}); gradient worst block err {worst:.2e}, worst err/e {worst_ratio:.3g}")


STEP_FAMILIES = {       # sweep family: fixture, case (tests/golden/cases.py: tpCN, its N, D, T and likelihood)
    "lane (maf3, D=32, N=10000)": ("maf3-d32-fit", "tpcn_n10000_d32_corr"),
    "nsf2 (nsf6, D=10)": ("nsf6-d10-fit", "tpcn_n256_d10_nsf6"),
    "tri6 (maf6, D=50, N=10000)": ("maf6-d50-fit", "tpcn_n10000_d50_bimodal"),
}


@pytest.mark.parametrize("no_fuse", ["0", "3"])
@pytest.mark.parametrize("family", list(STEP_FAMILIES))
def test_one_teacher_forced_step_on_a_trained_flow(family, no_fuse, monkeypatch):
    """One tpCN step (fused, and PMC_NO_FUSE=3: proposal / sweep / scaler as separate launches) on the trained flow.  The
    oracle's step (oracle/mcmc.py) starts from the same state with the same variates; its flow's inverse hands back the
    device's u' (teacher forcing), so theta', x', the scaler's log-determinant and alpha are compared walker by walker, and
    accept decisions may differ only where u lies between the two alphas.  The device's u' and the flow's log-determinant
    of it are held to the float64 oracle under the criterion on a subsample of at most 512 rows."""
    from oracle import mcmc as omcmc
    from oracle.maf import TorchFlowAdapter
    from oracle.scaler import Reparameterize as OracleScaler
    from pocomc_amd import Reparameterize
    from pocomc_amd.mcmc import StepEngine
    import cases
    monkeypatch.setenv("PMC_NO_FUSE", no_fuse)
    fx, name = STEP_FAMILIES[family]
    spec, flat, _ = fixture(fx)
    monkeypatch.setattr(cases, "flow_params", lambda s, seed, gain=1.2: flat)
    c = cases.find_case(name)
    N, D = c["N"], c["D"]
    state, funcs, opts, aux = cases.build_case(name, Reparameterize)
    assert (aux["spec"].n_dim, aux["spec"].n_transforms, aux["spec"].univariate) == (spec.n_dim, spec.n_transforms, spec.univariate)
    f = flow(spec, flat)
    ostate, ofuncs, oopts, _ = cases.build_case(name, OracleScaler)
    omaf = OracleMAF(spec, flat)
    geo = funcs["theta_geometry"]
    nu, sigma, mu = float(geo.t_nu), min(float(opts["proposal_scale"]), 0.99), np.array(geo.t_mean, float)
    rs = np.random.RandomState(c["seed"])
    rec = dict(gamma=rs.standard_gamma((D + nu) / 2, N), z=rs.randn(N, D), u=rs.rand(N))
    eng = StepEngine("preconditioned_pcn", N, D, f, funcs["scaler"])
    eng.load_state(state["u"], state["x"], state["logdetj"], state["logl"], state["logp"])
    eng.set_geometry(mu=geo.t_mean, cov=geo.t_cov)
    eng.set_mu(mu)
    sub = np.arange(N)[:: max(1, N // ROWS[D][1])][: ROWS[D][1]]
    # theta = forward(u): the device's, under the criterion; then both steps start from the float32 oracle's
    th0, l0 = omcmc.flow_numpy_wrapper(TorchFlowAdapter(omaf)).forward(state["u"])
    R = fr.Reference(spec, flat, state["u"][sub].astype(np.float32), "forward")
    check(R, "z", eng.theta32.cpu().numpy()[sub], f"step theta = forward(u), {family}", [th0[sub]])
    eng.theta32.copy_(torch.from_numpy(th0.astype(np.float32)))
    eng.ldjf.copy_(torch.from_numpy(l0.astype(np.float32)))
    eng.propose(sigma, nu, rec)
    p_theta, p_u, p_ldjf = eng.p_theta64.cpu().numpy(), eng.p_u.cpu().numpy(), eng.p_ldjf.cpu().numpy()

    class DeviceInverse(TorchFlowAdapter):
        def inverse(self, theta):
            return torch.from_numpy(p_u.astype(np.float32)), torch.from_numpy(p_ldjf.astype(np.float32))

    ofuncs["flow"] = DeviceInverse(omaf)
    oopts = dict(oopts, n_max=1)
    trace = []
    omcmc.preconditioned_pcn(ostate, ofuncs, oopts, rng=omcmc.Replay([rec]), trace=trace)
    tr = trace[0]
    parity.close_rel(p_theta, tr["theta_prime"], 2e-7, f"step theta', {family}")
    t32 = p_theta[sub].astype(np.float32)
    R = fr.Reference(spec, flat, t32, "inverse")
    ev = omaf.inverse(t32)
    check(R, "x", p_u[sub], f"step u' = inverse(theta'), {family}", [ev[0]])
    check(R, "ladj", p_ldjf[sub], f"step u' = inverse(theta'), {family}", [ev[1]])
    parity.close_rel(eng.p_x.cpu().numpy(), tr["x_prime"], fr.AFFINE_BOUND["x"], f"step x', {family}")
    parity.close_rel(eng.p_logdetj.cpu().numpy(), tr["logdetj_prime"], fr.AFFINE_BOUND["ladj"], f"step scaler logdetj', {family}",
                     cancel=1.0 + np.sum(np.where(np.isfinite(p_u), p_u, 0.0) ** 2, axis=1))
    eng.evaluate(funcs["logprior"], funcs["loglike"])
    eng.accept_reduce(c["beta"], nu, want_mask=True)
    alpha, acc = eng.alpha.cpu().numpy(), eng.h_accept.numpy().astype(bool)
    np.testing.assert_allclose(alpha, tr["alpha"], rtol=2e-3, atol=2e-5)
    assert np.array_equal(acc, rec["u"] < alpha)
    flips = acc != tr["accept"]
    lo, hi = np.minimum(alpha, tr["alpha"]), np.maximum(alpha, tr["alpha"])
    assert ((rec["u"][flips] >= lo[flips]) & (rec["u"][flips] <= hi[flips])).all()
    print(f"step {family} PMC_NO_FUSE={no_fuse}: {int(flips.sum())} accept flips of {N}, all inside the alpha gap")
