"""The workgroup inverse sweep of the affine flows (``csrc/maf_inverse_wg.hip``; ``PMC_INVERSE_TRIANGULAR_WG`` = 10, an
opt-in: ``Flow(inverse_sweep="workgroup")``): a right-looking triangular sweep that keeps two hidden-width arrays in LDS
and so fits the default-width flows at n_dim 92 - 114, which AUTO hands to the D-pass algorithm.

Against the oracle's D-pass inverse with the measures and the tolerance ``tests/test_gpu_wide_default_flows.py`` holds AUTO
to; against the device's own D-pass at more than one round of workgroups; what it writes and that it writes the same bits
twice; that a row of NaN leaves every other row's bits alone (the kernel's control flow reads no data); inside the MCMC
step; through ``Flow``, a pickle and a ``Sampler`` run.

Every flow here is default-initialised (``cases.flow_params``).  The sweep on trained and scaled-up flows -- the regime
criterion, the non-finite rows at 64 and 4096 rows, one teacher-forced step -- is in ``tests/test_gpu_flow_regimes.py``:
``algorithms`` lists algorithm 10 for every affine fixture the plan gives this sweep, from D = 10 to the default-width
flows at D = 102 (51 hidden tiles), where it is the only triangular sweep."""
import ctypes as C
import functools
import pickle

import numpy as np
import pytest
import torch

import cases
from oracle.maf import OracleMAF
from parity import close_rel, TOL
from pocomc_amd.maf_spec import MAFSpec, spec_by_name
from test_gpu_epilogue_rows import _bits, _pre_step
from test_gpu_inverse_plan import _inverse

pytestmark = pytest.mark.gpu

WG, NAIVE = 10, 2
S_WG = 9
SHAPES = {f"D{D}": (D, None) for D in (3, 10, 17, 33, 65, 92, 102, 114, 128, 157)}
SHAPES.update({"D10-maf3": (10, "maf3"), "D32-maf6": (32, "maf6")})
# beyond the fragments held in registers, where the kernel loads in place: 64 live hidden tiles (the hidden update past
# 8 * 7 + 1 tiles), and 25 output tiles over 13 x tiles (the output update past 3 * 8 tiles, layer 0 past 8 x tiles)
SHAPES.update({"D65-H1024": (65, MAFSpec(65, 2, hidden=1024)), "D193-H208": (193, MAFSpec(193, 2, hidden=208))})


def _spec(name):
    D, chain = SHAPES[name]
    if isinstance(chain, MAFSpec):
        return chain
    return spec_by_name(D, chain) if chain else MAFSpec(D, 2)


@functools.lru_cache(maxsize=None)
def flow_of(name):
    """One flow per shape for the whole module: (Flow with AUTO's inverse, spec, float32 oracle)."""
    from pocomc_amd import Flow
    spec = _spec(name)
    flat = cases.flow_params(spec, 3, gain=1.0)
    f = Flow(spec.n_dim, spec)
    f.set_params(flat)
    return f, spec, OracleMAF(spec, flat)


def latent(n, D, seed):
    return (np.random.default_rng(seed).normal(size=(n, D)) * 1.2).astype(np.float32)


def run(f, z, algo):
    rc, xb, lb = _inverse(f, torch.from_numpy(z).cuda(), algo)
    assert rc == 0, f.lib.pmc_last_error()
    return xb.view(np.float32), lb.view(np.float32)


# ------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_sweep_matches_the_oracles_dpass(name, n):
    f, spec, o = flow_of(name)
    D = spec.n_dim
    from pocomc_amd import _lib
    plan = _lib.pmc_inverse_plan_t()
    assert f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, WG, 0, C.byref(plan)) == 0 and plan.sweep == S_WG
    z = latent(n, D, 7 + n + D)
    xo, lo = o.inverse(z)                                    # the reference's D-pass algorithm
    terms = o.ladj_abs_terms(xo)
    x, l = run(f, z, WG)
    print(f"workgroup sweep {name} n={n}: x {close_rel(x, xo, np.inf, 'wg x (measured)'):.2e} "
          f"ladj {close_rel(l, lo, np.inf, 'wg ladj (measured)', cancel=terms):.2e}")
    close_rel(x, xo, TOL, "wg sweep x")
    close_rel(l, lo, TOL, "wg sweep ladj", cancel=terms)


def test_more_than_one_round_matches_the_devices_dpass():
    """4097 rows: 257 workgroups, the last with a single row."""
    f, spec, o = flow_of("D102")
    z = latent(4097, 102, 11)
    xd, ld = run(f, z, NAIVE)
    x, l = run(f, z, WG)
    terms = o.ladj_abs_terms(xd)
    print(f"workgroup sweep vs device D-pass, 4097 rows: x {close_rel(x, xd, np.inf, 'wg x vs dpass (measured)'):.2e} "
          f"ladj {close_rel(l, ld, np.inf, 'wg ladj vs dpass (measured)', cancel=terms):.2e}")
    close_rel(x, xd, TOL, "wg sweep x vs device D-pass")
    close_rel(l, ld, TOL, "wg sweep ladj vs device D-pass", cancel=terms)


def test_round_trip():
    f, spec, _ = flow_of("D102")
    z = latent(33, 102, 5)
    x, _ = run(f, z, WG)
    zz, _ = f.forward(torch.from_numpy(x))
    np.testing.assert_allclose(zz.numpy(), z, rtol=0, atol=1e-4)


# ------------------------------------------------------------------------------------------ writes, determinism, independence
@pytest.mark.parametrize("name", ["D33", "D102"])
def test_writes_and_determinism(name):
    from pocomc_amd import _lib
    f, spec, _ = flow_of(name)
    D, n = spec.n_dim, 33
    z = torch.from_numpy(latent(n + 16, D, 3)).cuda()

    def call(with_ladj=True):
        x = torch.full((n + 16, D), -7.0, dtype=torch.float32, device="cuda")
        ladj = torch.full((n + 16,), -7.0, dtype=torch.float32, device="cuda")
        rc = f.lib.pmc_maf_inverse(C.byref(f._desc), _lib.ptr(z), _lib.ptr(x), _lib.ptr(ladj) if with_ladj else None, n, WG,
                                   _lib.stream_handle())
        torch.cuda.synchronize()
        assert rc == 0
        return x.cpu().numpy(), ladj.cpu().numpy()

    x, l = call()
    assert np.isfinite(x[:n]).all() and not (x[:n] == -7.0).any() and np.isfinite(l[:n]).all() and not (l[:n] == -7.0).any()
    poison = _bits(np.float32([-7.0]))[0]
    assert (_bits(x[n:]) == poison).all() and (_bits(l[n:]) == poison).all()
    x2, l2 = call()
    assert np.array_equal(_bits(x), _bits(x2)) and np.array_equal(_bits(l), _bits(l2))
    x3, l3 = call(with_ladj=False)
    assert np.array_equal(_bits(x), _bits(x3)) and (_bits(l3) == poison).all()


def test_rows_are_independent():
    f, spec, _ = flow_of("D33")
    z = latent(33, 33, 9)
    x, l = run(f, z, WG)
    bad = z.copy()
    bad[5] = np.nan
    bad[20, 0] = np.inf
    xb, lb = run(f, bad, WG)                                 # (returns: _inverse synchronises)
    torch.cuda.synchronize()
    keep = np.ones(33, dtype=bool)
    keep[[5, 20]] = False
    assert np.array_equal(_bits(xb[keep]), _bits(x[keep])) and np.array_equal(_bits(lb[keep]), _bits(l[keep]))
    assert not np.isfinite(xb[5]).all() and not np.isfinite(xb[20]).all()


# ------------------------------------------------------------------------------------------ in the step
@pytest.mark.parametrize("D", [33, 102])
def test_the_step_launches_the_sweep_unfused(D, monkeypatch):
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd.mcmc import StepEngine
    spec = MAFSpec(D, 2)
    flow = pc.Flow(D, spec, seed=1)
    flow.inverse_algo = WG
    n = 21
    prior = pc.Prior([uniform(-5, 10)] * D)
    rng = np.random.default_rng(1000 * D + n)
    scaler = pc.Reparameterize(D, bounds=np.array([[-5.0, 5.0]] * D))
    scaler.fit(rng.uniform(-4, 4, size=(2000, D)))
    x = rng.uniform(-4, 4, size=(n, D))
    u = scaler.forward(x)
    engines, propose = [], StepEngine.propose

    def kept_propose(self, *args, **kw):
        self.p_theta32.fill_(-7.0)
        engines.append(self)
        return propose(self, *args, **kw)
    monkeypatch.setattr(StepEngine, "propose", kept_propose)
    a = _pre_step(monkeypatch, 0, n, D, flow, scaler, prior, x, u)
    theta32 = engines[0].p_theta32.clone()
    assert bool((theta32 != -7.0).any())                     # the proposal was a launch of its own: no fused instance
    rc, xb, lb = _inverse(flow, theta32, WG)
    assert rc == 0
    assert np.array_equal(_bits(a["u32"]), xb) and np.array_equal(_bits(a["ldjf"]), lb)
    b = _pre_step(monkeypatch, 1, n, D, flow, scaler, prior, x, u)
    for k in ("u32", "ldjf", "x", "finite", "theta"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["done"][0] == 1 and b["done"][0] == 1 and (a["finite"] != 0).sum() >= n - 1
    assert flow.inverse_algo == WG


# ------------------------------------------------------------------------------------------ the Flow surface
def test_flow_argument_and_pickle():
    from pocomc_amd import Flow
    f, spec, _ = flow_of("D102")
    assert f.inverse_algo == 0 and f.inverse_sweep == "auto"
    g = Flow(102, MAFSpec(102, 2), inverse_sweep="workgroup")
    g.set_params(f.params.cpu().numpy())
    assert g.inverse_algo == WG and g.inverse_sweep == "workgroup"
    z = latent(33, 102, 13)
    x, l = run(f, z, WG)
    xg, lg = g.inverse(torch.from_numpy(z))
    assert np.array_equal(_bits(xg.numpy()), _bits(x)) and np.array_equal(_bits(lg.numpy()), _bits(l))
    h = pickle.loads(pickle.dumps(g))
    assert h.inverse_algo == WG and h.inverse_sweep == "workgroup"
    xh, lh = h.inverse(torch.from_numpy(z))
    assert np.array_equal(_bits(xh.numpy()), _bits(x)) and np.array_equal(_bits(lh.numpy()), _bits(l))


def test_flow_argument_refusals():
    from pocomc_amd import Flow
    with pytest.raises(ValueError, match="inverse_sweep must be"):
        Flow(10, "maf3", inverse_sweep="lane")
    with pytest.raises(ValueError, match="spline flows know"):
        Flow(10, "nsf3", inverse_sweep="workgroup")
    with pytest.raises(ValueError, match="degree groups <= one tile"):
        Flow(2, "maf3", inverse_sweep="workgroup")
    with pytest.raises(ValueError, match="inverse_precision='f32'"):
        Flow(66, "maf3", inverse_precision="bf16", inverse_sweep="workgroup")
    assert Flow(10, "maf3").inverse_algo == 0


# ------------------------------------------------------------------------------------------ a run
def test_a_sampler_runs_with_the_workgroup_sweep_at_100_dimensions():
    """The prior, likelihood, sizes and assertions of ``test_default_sampler_runs_at_100_dimensions``
    (``tests/test_gpu_wide_default_flows.py``), with a ready maf6 flow that inverts with the workgroup sweep."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    D = 100

    def loglike(x):
        return -0.5 * np.sum((x / 50.0) ** 2, axis=1)

    prior = pc.Prior([uniform(-10, 20)] * D)
    flow = pc.Flow(D, "maf6", inverse_sweep="workgroup")
    s = pc.Sampler(prior=prior, likelihood=loglike, vectorize=True, n_active=64, n_effective=128, n_steps=1, n_max_steps=2,
                   train_config=dict(epochs=3), random_state=0, flow=flow)
    assert s.flow is flow and s.flow.spec.hidden == 512 and s.flow.spec.n_transforms == 6
    before = s.flow.params.cpu().numpy().copy()
    s.run(n_total=128, n_evidence=0, progress=False)
    assert float(s.particles.get("beta", index=-1)) == 1.0
    x, w, logl, logp = s.posterior()
    assert x.shape[1] == D and np.isfinite(x).all() and np.isfinite(w).all() and np.isfinite(logl).all() and np.isfinite(logp).all()
    assert not np.array_equal(s.flow.params.cpu().numpy(), before)
    assert np.isfinite(s.evidence()[0])
    assert s.flow.inverse_algo == WG
