"""``FlowPrior`` / ``JointPrior`` inside the step of a HOST likelihood (kernel option ``step_prior``,
``pmc_step_ext_t.prior_stage``): the prior's three launches run on the step's stream, on the device's copy of x', while the
host evaluates the likelihood, and the accept takes logp' from the device.

No tolerance appears: a row's prior value depends on the row's own values only (``tests/test_gpu_flow_prior.py``,
``tests/test_gpu_joint_prior.py``), so the call with ``step_prior=True`` is the call without it -- the host route, the
parent's behaviour -- bit for bit, in every mode a kernel call takes with a host likelihood."""
import ctypes as C

import numpy as np
import pytest
import torch

from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu

D, N, N_MAX, N_STEPS, SEED = 5, 200, 8, 4, 5         # 200 walkers: three 64-row blocks and a tail of 8
ARRAYS = ("x", "u", "logdetj", "logl", "logp")
SCALARS = ("calls", "steps", "accept", "proposal_scale", "efficiency")
MODES = {"plain": dict(x_order="C"),
         "pipelined": dict(x_order="F"),
         "pipelined-2-lanes": dict(x_order="F", lanes=2),                       # 112 + 88 rows
         "lanes-on-streams": dict(x_order="F", pipeline=False, lanes=2),
         "host-threads": dict(x_order="F", host_threads=2)}


def gauss(width, centre=0.2):
    """A numpy Gaussian, row-wise and independent of the batch and of the layout of ``x``: column after column."""
    def f(x):
        acc = np.zeros(x.shape[0])
        for j in range(x.shape[1]):
            acc = acc + (x[:, j] - centre) ** 2
        return -0.5 * acc / width ** 2
    return f


def rows_inside(half, sigma, n, cols, seed):
    """The first ``n`` of 4 n Gaussian rows that lie strictly inside (-half, half)^cols."""
    x = np.random.default_rng(seed).normal(0.0, sigma, size=(4 * n, cols))
    x = x[(np.abs(x) < half).all(axis=1)][:n]
    assert len(x) == n
    return x


def flow_prior(flow, half=3.0, sigma=0.5, cols=D, seed=1):
    """A ``FlowPrior`` on (-half, half)^cols, its flow trained by 30 epochs on 256 Gaussian rows."""
    import pocomc_amd as pc
    torch.manual_seed(seed)
    return pc.FlowPrior.from_samples(rows_inside(half, sigma, 256, cols, seed), bounds=np.array([[-half, half]] * cols),
                                     flow=flow, train_config={"epochs": 30})


def build_prior(name):
    import pocomc_amd as pc
    from scipy.stats import gamma, norm
    if name == "affine":
        return flow_prior(MAFSpec(D, 3, 32))
    if name == "spline":
        return flow_prior("nsf3")
    # Df = 3 on the columns 4, 0, 2; the factors on 1 and 3, the second an extended family with a pole at its loc
    return pc.JointPrior(flow_prior("maf3", cols=3), [4, 0, 2], pc.Prior([norm(0.2, 1.0), gamma(0.5, loc=-2.5, scale=2.0)],
                                                                        device=True))


def build_problem(prior, bounds, x):
    """``(prior, scaler, flow, geometry, x, u)``: walkers ``x`` in the step's ``Reparameterize`` on ``bounds``, a near-identity
    maf3 as the preconditioner."""
    import pocomc_amd as pc
    from pocomc_amd.geometry import Geometry
    scaler = pc.Reparameterize(D, bounds=np.asarray(bounds, dtype=np.float64))
    scaler.fit(x)
    u = scaler.forward(x)
    flow = pc.Flow(D, "maf3", seed=0)
    flow.set_params(0.25 * flow.params.cpu())
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    geo.normal_cov = np.cov(u.T)
    assert np.isfinite(prior.logpdf(x)).all()
    return prior, scaler, flow, geo, x, u


@pytest.fixture(scope="module")
def problems():
    """The three priors, each with walkers in a step whose scaler has the prior's own box (what a Sampler builds)."""
    out = {}
    for name in ("affine", "spline", "joint"):
        prior = build_prior(name)
        out[name] = build_problem(prior, prior.bounds, rows_inside(2.0, 0.5, N, D, 7))
    return out


def call(prob, f, kind, step_prior, logprior=None, blobs=None, scale=1.0, **extra):
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=f(x), logp=prior.logpdf(x), beta=0.5, blobs=blobs)
    loglike = (lambda v: (f(v), None)) if blobs is None else (lambda v: (f(v), 2.0 * f(v)))
    funcs = dict(loglike=loglike, logprior=logprior or prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo,
                 u_geometry=geo)
    opts = dict(n_max=N_MAX, n_steps=N_STEPS, progress_bar=None, proposal_scale=scale / D ** 0.5, seed=SEED, **extra)
    if step_prior is not None:
        opts["step_prior"] = step_prior
    return getattr(pmcmc, kind)(state, funcs, opts)


def assert_same(a, b, tag):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), (tag, k)
    for k in SCALARS:
        assert a[k] == b[k], (tag, k, a[k], b[k])


# ------------------------------------------------------------------------------------------------------------------
# 1. the same trajectory
# ------------------------------------------------------------------------------------------------------------------
CELLS = [("affine", "preconditioned_pcn", "plain"), ("affine", "preconditioned_pcn", "pipelined-2-lanes"),
         ("affine", "preconditioned_rwm", "pipelined"), ("affine", "pcn", "lanes-on-streams"),
         ("affine", "preconditioned_pcn", "host-threads"),
         ("spline", "preconditioned_pcn", "plain"), ("spline", "preconditioned_rwm", "pipelined-2-lanes"),
         ("spline", "preconditioned_pcn", "pipelined"),
         ("joint", "preconditioned_pcn", "plain"), ("joint", "pcn", "pipelined-2-lanes"),
         ("joint", "preconditioned_rwm", "lanes-on-streams")]


@pytest.mark.parametrize("name,kind,mode", CELLS)
def test_the_trajectory_is_the_host_routes(problems, name, kind, mode):
    prob, f = problems[name], gauss(0.8)
    on = call(prob, f, kind, True, **MODES[mode])
    # (host_threads: the host route would call FlowPrior.logpdf from two threads at once, which share the workspaces it keeps
    #  per row count -- the option asks for thread-safe black boxes; the stage calls nothing from the threads, and a row-wise
    #  likelihood gives the chunks the values of the whole block: the reference is the one-thread call)
    off = call(prob, f, kind, False, **MODES["pipelined" if mode == "host-threads" else mode])
    moved = int((on["x"] != prob[4]).any(axis=1).sum())
    print(f"{name} {kind} {mode}: steps {on['steps']}, calls {on['calls']} of {on['steps'] * N}, evaluations "
          f"{on['evaluations']} / {off['evaluations']}, moved {moved} of {N}")
    assert_same(on, off, (name, kind, mode))
    assert on["steps"] >= 2 and 0 < moved and np.isfinite(on["logp"]).all()
    assert np.array_equal(prob[0].logpdf(on["x"]), on["logp"])                # the walkers carry the prior's value of their x


def test_the_option_left_out_is_the_option_off(problems):
    prob, f = problems["affine"], gauss(0.8)
    assert_same(call(prob, f, "preconditioned_pcn", None, x_order="F"), call(prob, f, "preconditioned_pcn", False, x_order="F"),
                "default")


@pytest.mark.parametrize("mode,tensor", [("plain", False), ("pipelined-2-lanes", True)])
def test_blobs_of_a_host_likelihood_keep_their_route(problems, mode, tensor):
    """numpy blobs (the plain step's bookkeeping) and blobs as a device tensor (the pinned buffer and the move launch)."""
    prob, f = problems["joint"], gauss(0.8)
    start = np.full(N, -7.0)
    blobs = lambda: torch.from_numpy(start.copy()).cuda() if tensor else start.copy()
    on = call(prob, f, "preconditioned_pcn", True, blobs=blobs(), **MODES[mode])
    off = call(prob, f, "preconditioned_pcn", False, blobs=blobs(), **MODES[mode])
    assert_same(on, off, mode)
    assert np.array_equal(np.asarray(on["blobs"]), np.asarray(off["blobs"]))
    moved = (on["x"] != prob[4]).any(axis=1)
    assert moved.any() and np.array_equal(np.asarray(on["blobs"]).reshape(-1)[moved], 2.0 * f(on["x"])[moved])


# ------------------------------------------------------------------------------------------------------------------
# 2. the host prior is not called
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "pipelined-2-lanes"])
def test_the_host_prior_is_not_called(problems, mode, monkeypatch):
    """The route's point.  (Without the feature the option is not known and the prior is called on the host.)"""
    prob, f = problems["affine"], gauss(0.8)
    prior = prob[0]
    seen = []
    real = type(prior).logpdf

    def counted(self, x):
        seen.append(len(x))
        return real(self, x)
    for step_prior in (True, False):
        with monkeypatch.context() as m:
            m.setattr(type(prior), "logpdf", counted)
            del seen[:]
            res = call(prob, f, "preconditioned_pcn", step_prior, **MODES[mode])
        during = len(seen) - 1               # (call() takes the walkers' own logp through the counter, once, before the kernel)
        print(f"{mode} step_prior={step_prior}: {during} host calls of prior.logpdf during the kernel call")
        assert res["steps"] >= 2
        assert (during == 0) if step_prior else (during >= 1), (step_prior, during)


# ------------------------------------------------------------------------------------------------------------------
# 3. rows the prior rules out
# ------------------------------------------------------------------------------------------------------------------
NARROW_WIDTH = 1.0       # of the likelihood in the narrow-prior problem: broad, so that the walkers move (condition below)


@pytest.fixture(scope="module")
def narrow():
    """The prior's box is [-1, 1]^5, the step's ``Reparameterize`` has [-3, 3]^5: proposals leave the prior's box."""
    prior = flow_prior(MAFSpec(D, 3, 32), half=1.0, sigma=0.3)
    x = np.random.default_rng(3).uniform(-0.95, 0.95, size=(N, D))
    x[:, 0] = np.minimum(x[:, 0], 0.89)                 # (the walkers' own logl is finite: the likelihood below has a hole)
    return build_problem(prior, np.array([[-3.0, 3.0]] * D), x)


def nan_beyond(f):
    def g(x):
        out = f(x)
        out[x[:, 0] > 0.9] = np.nan
        return out
    return g


@pytest.mark.parametrize("kind,mode", [("preconditioned_pcn", "plain"), ("preconditioned_pcn", "pipelined-2-lanes"),
                                       ("preconditioned_rwm", "pipelined"), ("pcn", "lanes-on-streams")])
def test_rows_the_prior_rules_out(narrow, kind, mode):
    prior, f = narrow[0], nan_beyond(gauss(NARROW_WIDTH, centre=0.0))
    # the condition on the inputs, on the host route alone: what the prior returns there
    lp = []

    def recorded(x):
        out = prior.logpdf(x)
        lp.append(out)
        return out
    off = call(narrow, f, kind, False, logprior=recorded, scale=2.0, **MODES[mode])
    lp = np.concatenate(lp)
    ruled_out, proposals = int(np.isneginf(lp).sum()), off["steps"] * N
    moved = int((off["x"] != narrow[4]).any(axis=1).sum())
    print(f"{kind} {mode}: host route: logp' = -inf on {ruled_out} of {proposals} proposals, acceptance {off['accept']:.3f}, "
          f"moved {moved} of {N}, calls {off['calls']}")
    assert ruled_out >= 0.10 * proposals and off["accept"] >= 0.10
    on = call(narrow, f, kind, True, scale=2.0, **MODES[mode])
    assert_same(on, off, (kind, mode))
    assert on["calls"] < on["steps"] * N
    assert on["evaluations"] > off["evaluations"]              # the rows the prior rules out did reach the likelihood
    assert np.isfinite(on["logp"]).all() and np.isfinite(on["logl"]).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. / 5. the stage against the class
# ------------------------------------------------------------------------------------------------------------------
def one_pre_step(prob, n, kind="preconditioned_pcn", scale=2.0):
    """One ``pmc_step_pre`` of the first ``n`` walkers with the stage: ``(p_x, p_fin, p_logp, host words)``."""
    from pocomc_amd import mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    eng = pmcmc.StepEngine(kind, n, D, flow, scaler, seed=SEED, x_order="C")
    eng.load_state(u[:n], x[:n], scaler.inverse(u[:n])[1], np.zeros(n), prior.logpdf(x[:n]))
    eng.set_geometry(mu=geo.t_mean, cov=geo.t_cov)
    eng.set_step_prior(prior)
    eng.propose(scale / D ** 0.5, float(geo.t_nu))
    torch.cuda.synchronize()
    return eng.p_x.clone(), eng.p_fin.cpu().numpy().astype(bool), eng.p_logp.cpu().numpy(), eng._np_stage.copy()


def check_stage(prior, p_x, fin, logp, words):
    want = prior.logpdf_device(p_x).cpu().numpy()
    assert np.array_equal(logp[fin].view(np.int64), want[fin].view(np.int64))
    assert np.isneginf(logp[~fin]).all()
    count = int((fin & ~np.isfinite(logp)).sum())
    assert words[0] == count and words[1] == 0, (words, count)
    return count


@pytest.fixture(scope="module")
def wide(narrow):
    """The three priors under a step whose box is wider than theirs: a good part of the proposals is ruled out."""
    out = {"affine": narrow}
    x = np.random.default_rng(4).uniform(-2.4, 2.9, size=(N, D))
    for name in ("spline", "joint"):
        out[name] = build_problem(build_prior(name), np.array([[-6.0, 6.0]] * D), x)
    return out


@pytest.mark.parametrize("n", [1, 64, 65, 200])
@pytest.mark.parametrize("name", ["affine", "spline", "joint"])
def test_the_stage_is_the_class(wide, name, n):
    p_x, fin, logp, words = one_pre_step(wide[name], n)
    count = check_stage(wide[name][0], p_x, fin, logp, words)
    print(f"{name} n={n}: {int(fin.sum())} finite rows, {count} of them ruled out by the prior")
    assert n < 64 or (0 < count < n)


def test_a_bf16_flow_keeps_its_kernel():
    """The smallest flow ``Flow`` takes with ``precision="bf16"`` (affine: every width; two features, two transforms, one
    hidden tile): the stage launches ``pmc_maf_forward_bf16`` as ``FlowPrior.logpdf_device`` does, and gives its bits."""
    import pocomc_amd as pc
    d, n = 2, 200
    flow = pc.Flow(d, MAFSpec(d, 2, 16), seed=0, precision="bf16")
    x = np.random.default_rng(5).uniform(-0.95, 0.95, size=(n, d))
    fit = pc.Reparameterize(d, bounds=np.array([[-1.0, 1.0]] * d))
    fit.fit(x)
    prior = pc.FlowPrior(flow, fit)
    assert prior.flow.precision == "bf16"
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    scaler = pc.Reparameterize(d, bounds=np.array([[-3.0, 3.0]] * d))
    scaler.fit(x)
    u = scaler.forward(x)
    geo = Geometry()
    geo.fit(u)
    eng = pmcmc.StepEngine("pcn", n, d, None, scaler, seed=SEED, x_order="C")
    eng.load_state(u, x, scaler.inverse(u)[1], np.zeros(n), prior.logpdf(x))
    eng.set_geometry(mu=geo.t_mean, cov=geo.t_cov)
    eng.set_step_prior(prior)
    assert eng._stage.image16 and eng._stage.image_per_transform > 0
    eng.propose(0.9, float(geo.t_nu))
    torch.cuda.synchronize()
    fin, logp = eng.p_fin.cpu().numpy().astype(bool), eng.p_logp.cpu().numpy()
    count = check_stage(prior, eng.p_x, fin, logp, eng._np_stage.copy())
    f32 = pc.FlowPrior(pc.Flow(d, MAFSpec(d, 2, 16), seed=0), fit).logpdf_device(eng.p_x).cpu().numpy()
    assert 0 < count < n and not np.array_equal(f32[fin], logp[fin])          # (the bf16 kernel did run)


def test_the_entry_on_its_own(wide):
    """``pmc_step_prior_stage`` on a hand-filled struct: rows with ``p_fin == 0`` get -inf whatever their x' and are not
    counted; the count goes to the two host words in turn, and the device counter is zero again behind every launch."""
    from pocomc_amd import _lib
    prior = wide["joint"][0]
    n = 130
    x = np.random.default_rng(6).uniform(-3.4, 3.4, size=(n, D))
    x[5, 1] = np.nan
    fin = np.ones(n, dtype=np.int32)
    fin[[0, 5, 63, 64, 129]] = 0
    p_x, p_fin = torch.from_numpy(x).cuda(), torch.from_numpy(fin).cuda()
    p_logp = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    stage = prior.step_stage(n)
    s = _lib.pmc_step_ext_t(n=n, D=D, p_x=p_x.data_ptr(), p_fin=p_fin.data_ptr(), p_logp=p_logp.data_ptr(),
                            ext=_lib.PMC_STEP_EXT, prior_stage=C.cast(C.pointer(stage), C.c_void_p))
    lib = _lib.load()
    want = prior.logpdf_device(p_x).cpu().numpy()
    want[fin == 0] = -np.inf
    count = int(((fin != 0) & ~np.isfinite(want)).sum())
    assert 0 < count < n
    words = stage.counts.numpy()
    for launch in range(3):
        p_logp.fill_(7.0)
        words[launch & 1] = -1
        _lib.check(lib.pmc_step_prior_stage(C.byref(s), _lib.stream_handle()), "pmc_step_prior_stage")
        torch.cuda.synchronize()
        assert np.array_equal(p_logp.cpu().numpy().view(np.int64), want.view(np.int64))
        assert words[launch & 1] == count
        assert stage._keep[1]["count"].cpu().numpy().tolist() == [0, launch + 1]
    # a refusal leaves everything as it is
    s.prior_rows = 1
    p_logp.fill_(7.0)
    assert lib.pmc_step_prior_stage(C.byref(s), _lib.stream_handle()) != 0
    torch.cuda.synchronize()
    assert (p_logp == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------
# 6. in a Sampler
# ------------------------------------------------------------------------------------------------------------------
def gauss_t(c):
    def f(x):
        acc = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
        for j in range(x.shape[1]):
            acc = acc + (x[:, j] - c) ** 2
        return -0.5 * acc
    return f


@pytest.fixture(scope="module")
def run_a():
    """Run A of ``test_run_a_as_the_prior_of_run_b_on_both_routes``: a 4-D Gaussian under a uniform prior."""
    import pocomc_amd as pc
    from scipy.stats import uniform
    a = pc.Sampler(prior=pc.Prior([uniform(-10.0, 20.0)] * 4), likelihood=gauss_t(0.3), random_state=3, vectorize=True,
                   flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30}, device_likelihood=True)
    a.run(n_total=256, n_evidence=0, progress=False)
    return a


def sampler_prior(a, which):
    import pocomc_amd as pc
    from scipy.stats import norm, uniform
    if which == "flow":
        return pc.FlowPrior.from_sampler(a)
    torch.manual_seed(5)
    block = pc.FlowPrior.from_sampler(a, columns=[0, 1, 2], flow="maf3", train_config={"epochs": 30})
    return pc.JointPrior(block, [4, 0, 2], pc.Prior([norm(0.5, 2.0), uniform(-4.0, 9.0)]))      # 3 shared columns, 2 own


@pytest.mark.parametrize("which", ["flow", "joint"])
def test_run_b_with_a_host_likelihood_on_both_routes(run_a, which, tmp_path):
    import pocomc_amd as pc
    prior = sampler_prior(run_a, which)
    kw = dict(vectorize=True, flow="maf3", n_active=64, n_effective=128, train_config={"epochs": 30})

    def run_b(step_prior, **extra):
        s = pc.Sampler(prior=prior, likelihood=gauss(1.0, centre=0.8), random_state=7, step_prior=step_prior, **kw, **extra)
        s.run(n_total=256, n_evidence=0, progress=False)
        return s
    on, off = run_b(True, output_dir=tmp_path), run_b(False)
    assert on.step_prior is True and off.step_prior is False
    ra, rb = on.results, off.results
    for k in ("x", "logp", "logl", "logz", "beta"):
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    assert on.evidence() == off.evidence() and on.calls == off.calls
    assert np.isfinite(np.asarray(ra["logp"])).all() and np.asarray(ra["beta"])[-1] == 1.0
    # a checkpoint written by one run loads into the other
    path = tmp_path / "b.state"
    on.save_state(path)
    res = pc.Sampler(prior=prior, likelihood=gauss(1.0, centre=0.8), random_state=7, step_prior=False, **kw)
    res.load_state(path)
    for k in ("x", "logp", "logl", "logz"):
        assert np.array_equal(np.asarray(res.results[k]), np.asarray(ra[k])), k
