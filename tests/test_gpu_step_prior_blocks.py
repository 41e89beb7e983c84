"""The blocks form of ``JointPrior`` inside the step of a host likelihood (``pmc_step_ext2_t.blocks_stage``, kernel option
``step_prior``): ``pmc_joint_blocks_pre`` on the device's copy of x', every block's forward call and a closing kernel, on the
step's stream while the host evaluates the likelihood.

No tolerance appears: the stage is the class's ``logpdf_device`` gated by the finite mask, and a row's prior value depends on
the row's own values only (``tests/test_gpu_joint_blocks.py``), so the call with ``step_prior=True`` is the call without it."""
import ctypes as C

import numpy as np
import pytest
import torch

from .test_gpu_step_prior import (D, MODES, N, SEED, assert_same, build_problem, call, check_stage, flow_prior, gauss,
                                  nan_beyond, rows_inside)

pytestmark = pytest.mark.gpu


def blocks_prior(half=3.0, sigma=0.5, own=True):
    """Two blocks -- maf3 on the columns 4, 0 and nsf3 on 2, 1 -- and (``own``) a gamma(0.5) factor with a pole on column 3;
    without it a three-column spline block on 2, 1, 3."""
    import pocomc_amd as pc
    from scipy.stats import gamma
    a = flow_prior("maf3", half=half, sigma=sigma, cols=2, seed=1)
    if own:
        c = flow_prior("nsf3", half=half, sigma=sigma, cols=2, seed=2)
        return pc.JointPrior([a, c], [[4, 0], [2, 1]], pc.Prior([gamma(0.5, loc=-half, scale=2.0)], device=True))
    c = flow_prior("nsf3", half=half, sigma=sigma, cols=3, seed=2)
    return pc.JointPrior([a, c], [[4, 0], [2, 1, 3]])


@pytest.fixture(scope="module")
def problems():
    """The two priors with walkers in a step whose scaler has the prior's own box (what a Sampler builds)."""
    out = {}
    for name, own in (("table", True), ("bare", False)):
        prior = blocks_prior(own=own)
        assert prior.blocks == 2 and prior.dim == D
        out[name] = build_problem(prior, prior.bounds, rows_inside(2.0, 0.5, N, D, 7))
    return out


@pytest.fixture(scope="module")
def narrow():
    """The prior's box is [-1, 1]^5, the step's ``Reparameterize`` has [-3, 3]^5: proposals leave the prior's box."""
    prior = blocks_prior(half=1.0, sigma=0.3, own=False)
    x = np.random.default_rng(3).uniform(-0.95, 0.95, size=(N, D))
    x[:, 0] = np.minimum(x[:, 0], 0.89)                 # (the walkers' own logl is finite: the likelihood below has a hole)
    return build_problem(prior, np.array([[-3.0, 3.0]] * D), x)


# ------------------------------------------------------------------------------------------------------------------
# the stage against the class
# ------------------------------------------------------------------------------------------------------------------
def one_pre_step(prob, n, kind="preconditioned_pcn", scale=2.0):
    from pocomc_amd import _lib, mcmc as pmcmc
    prior, scaler, flow, geo, x, u = prob
    eng = pmcmc.StepEngine(kind, n, D, flow, scaler, seed=SEED, x_order="C")
    eng.load_state(u[:n], x[:n], scaler.inverse(u[:n])[1], np.zeros(n), prior.logpdf(x[:n]))
    eng.set_geometry(mu=geo.t_mean, cov=geo.t_cov)
    eng.set_step_prior(prior)
    assert isinstance(eng._stage, _lib.pmc_prior_blocks_stage_t) and eng._step.ext == _lib.PMC_STEP_EXT2
    assert eng._step.blocks_stage and not eng._step.prior_stage
    eng.propose(scale / D ** 0.5, float(geo.t_nu))
    torch.cuda.synchronize()
    return eng.p_x.clone(), eng.p_fin.cpu().numpy().astype(bool), eng.p_logp.cpu().numpy(), eng._np_stage.copy()


@pytest.fixture(scope="module")
def wide(narrow):
    """Both priors under a step whose box is wider than theirs: a good part of the proposals is ruled out."""
    x = np.random.default_rng(4).uniform(-2.4, 2.9, size=(N, D))
    return {"bare": narrow, "table": build_problem(blocks_prior(own=True), np.array([[-6.0, 6.0]] * D), x)}


@pytest.mark.parametrize("n", [1, 64, 65, 200])
@pytest.mark.parametrize("name", ["table", "bare"])
def test_the_stage_is_the_class(wide, name, n):
    p_x, fin, logp, words = one_pre_step(wide[name], n)
    count = check_stage(wide[name][0], p_x, fin, logp, words)
    print(f"{name} n={n}: {int(fin.sum())} finite rows, {count} of them ruled out by the prior")
    assert n < 64 or (0 < count < n)


def test_the_single_form_takes_its_own_field(problems):
    """A ``FlowPrior`` in the larger struct: ``prior_stage`` is set, ``blocks_stage`` stays NULL."""
    from pocomc_amd import _lib, mcmc as pmcmc
    prior, scaler, flow, geo, x, u = problems["table"]
    single = flow_prior("maf3", cols=D)
    eng = pmcmc.StepEngine("preconditioned_pcn", 70, D, flow, scaler, seed=SEED, x_order="C")
    assert isinstance(eng._step, _lib.pmc_step_ext2_t) and eng._step.ext == 2 and not eng._step.blocks_stage
    eng.load_state(u[:70], x[:70], scaler.inverse(u[:70])[1], np.zeros(70), single.logpdf(x[:70]))
    eng.set_geometry(mu=geo.t_mean, cov=geo.t_cov)
    eng.set_step_prior(single)
    assert eng._step.prior_stage and not eng._step.blocks_stage
    eng.propose(1.0 / D ** 0.5, float(geo.t_nu))
    torch.cuda.synchronize()
    check_stage(single, eng.p_x, eng.p_fin.cpu().numpy().astype(bool), eng.p_logp.cpu().numpy(), eng._np_stage.copy())


def test_the_entry_on_its_own(wide):
    """``pmc_step_prior_stage`` on a hand-filled ``pmc_step_ext2_t``: rows with ``p_fin == 0`` get -inf whatever their x' and
    are not counted; the count goes to the two host words in turn, and the device counter is zero again behind every launch."""
    from pocomc_amd import _lib
    prior = wide["table"][0]
    n = 130
    x = np.random.default_rng(6).uniform(-3.4, 3.4, size=(n, D))
    x[5, 1] = np.nan
    fin = np.ones(n, dtype=np.int32)
    fin[[0, 5, 63, 64, 129]] = 0
    p_x, p_fin = torch.from_numpy(x).cuda(), torch.from_numpy(fin).cuda()
    p_logp = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    stage = prior.step_stage(n)
    assert isinstance(stage, _lib.pmc_prior_blocks_stage_t) and stage.blocks.n_blocks == 2
    s = _lib.pmc_step_ext2_t(n=n, D=D, p_x=p_x.data_ptr(), p_fin=p_fin.data_ptr(), p_logp=p_logp.data_ptr(),
                             ext=_lib.PMC_STEP_EXT2, blocks_stage=C.cast(C.pointer(stage), C.c_void_p))
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
    # a refusal leaves everything as it is: both stages set, then a second prior
    other = flow_prior("maf3", cols=D).step_stage(n)
    p_logp.fill_(7.0)
    s.prior_stage = C.cast(C.pointer(other), C.c_void_p)
    assert lib.pmc_step_prior_stage(C.byref(s), _lib.stream_handle()) != 0 and b"both set" in lib.pmc_last_error()
    s.prior_stage = None
    s.prior_rows = 1
    assert lib.pmc_step_prior_stage(C.byref(s), _lib.stream_handle()) != 0
    torch.cuda.synchronize()
    assert (p_logp == 7.0).all()


# ------------------------------------------------------------------------------------------------------------------
# whole kernel calls
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["table", "bare"])
@pytest.mark.parametrize("mode", ["plain", "pipelined-2-lanes"])
def test_the_trajectory_is_the_host_routes(problems, name, mode):
    prob, f, kind = problems[name], gauss(0.8), "preconditioned_pcn"
    on = call(prob, f, kind, True, **MODES[mode])
    off = call(prob, f, kind, False, **MODES[mode])
    moved = int((on["x"] != prob[4]).any(axis=1).sum())
    print(f"{name} {mode}: steps {on['steps']}, calls {on['calls']} of {on['steps'] * N}, evaluations "
          f"{on['evaluations']} / {off['evaluations']}, moved {moved} of {N}")
    assert_same(on, off, (name, mode))
    assert on["steps"] >= 2 and 0 < moved and np.isfinite(on["logp"]).all()
    assert np.array_equal(prob[0].logpdf(on["x"]), on["logp"])                # the walkers carry the prior's value of their x


@pytest.mark.parametrize("mode", ["plain", "pipelined-2-lanes"])
def test_rows_the_prior_rules_out(narrow, mode):
    prior, f, kind = narrow[0], nan_beyond(gauss(1.0, centre=0.0)), "preconditioned_pcn"
    lp = []

    def recorded(x):
        out = prior.logpdf(x)
        lp.append(out)
        return out
    off = call(narrow, f, kind, False, logprior=recorded, scale=2.0, **MODES[mode])
    lp = np.concatenate(lp)
    ruled_out, proposals = int(np.isneginf(lp).sum()), off["steps"] * N
    print(f"{mode}: host route: logp' = -inf on {ruled_out} of {proposals} proposals, acceptance {off['accept']:.3f}, "
          f"calls {off['calls']}")
    assert ruled_out >= 0.10 * proposals and off["accept"] >= 0.10
    on = call(narrow, f, kind, True, scale=2.0, **MODES[mode])
    assert_same(on, off, mode)
    assert on["calls"] < on["steps"] * N                        # the stage did rule rows out ...
    assert on["evaluations"] > off["evaluations"]              # ... which reached the likelihood all the same
    assert np.isfinite(on["logp"]).all() and np.isfinite(on["logl"]).all()


# ------------------------------------------------------------------------------------------------------------------
# in a Sampler
# ------------------------------------------------------------------------------------------------------------------
def test_run_b_with_a_host_likelihood_on_both_routes(tmp_path):
    """Run B of ``test_gpu_joint_blocks``'s Sampler test (A's block on 4, 0, 2, C's on 1, 5, one own factor) with a numpy
    likelihood, the prior once inside the step and once on the host route: the same bits."""
    import pocomc_amd as pc
    from scipy.stats import norm
    from .test_gpu_joint_blocks import blocks_of_a_and_c
    block_a, block_c = blocks_of_a_and_c()
    prior = pc.JointPrior([block_a, block_c], [[4, 0, 2], [1, 5]], pc.Prior([norm(0.5, 2.0)]))
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
    path = tmp_path / "b.state"
    on.save_state(path)
    res = pc.Sampler(prior=prior, likelihood=gauss(1.0, centre=0.8), random_state=7, step_prior=False, **kw)
    res.load_state(path)
    for k in ("x", "logp", "logl", "logz"):
        assert np.array_equal(np.asarray(res.results[k]), np.asarray(ra[k])), k
