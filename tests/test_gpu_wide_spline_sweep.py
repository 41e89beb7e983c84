"""The workgroup inverse sweep of the spline flows (``csrc/maf_inverse_wg_nsf.hip``; ``PMC_INVERSE_TRIANGULAR_WG_NSF`` = 11,
an opt-in: ``Flow(inverse_sweep="workgroup_spline")``): the affine flows' workgroup sweep with a left-looking output stage,
two hidden-width arrays in LDS, so that it fits the default-width spline flows at n_dim 97 - 108, which AUTO hands to the
D-pass algorithm.

Against the oracle's D-pass inverse with the measures and the tolerances the suite holds every spline inverse to
(``tests/test_gpu_flow.py``: ``NSF_INV`` on x, ``NSF_LADJ`` on the log-determinant); against the device's own D-pass at
more than one round of workgroups and against the lone-wave spline sweep; what it writes and that it writes the same bits
twice; that a non-finite row leaves every other row's bits alone (the kernel's control flow reads no data, the spline's bin
is picked by selects); outside the spline box; the regime criterion of ``tests/test_gpu_flow_regimes.py``; inside the MCMC
step; through ``Flow``, a pickle and a ``Sampler`` run.

The regime test of this file runs at D = 10 (2-3 hidden tiles: products that are never split by K range).  The split
products -- 16 K tiles and more, the partials added by wavefront 0 -- meet the criterion in
``tests/test_gpu_flow_regimes.py``, whose ``algorithms`` lists algorithm 11 for every spline fixture the plan gives this
sweep: scaled-up and trained flows at D = 102 (51 hidden tiles, 35 of them split; it is the only triangular sweep there),
D = 86 (43 tiles, 27 split, on the same rows as the lone-wave sweep) and D = 128 (33 tiles of three or four degree groups:
long products, none split), with the non-finite rows, the rows outside the box and one teacher-forced step."""
import ctypes as C
import functools
import pickle

import numpy as np
import pytest
import torch

import cases
import flow_regimes as fr
import test_gpu_flow_regimes as regimes
from oracle.maf import OracleMAF
from parity import close_rel
from pocomc_amd.maf_spec import MAFSpec, spec_by_name
from test_gpu_epilogue_rows import _bits, _pre_step
from test_gpu_inverse_plan import _inverse

pytestmark = pytest.mark.gpu

WG_NSF, NAIVE, NSF_SOLO = 11, 2, 6
S_WG_NSF = 10
NSF_INV, NSF_LADJ = 5e-5, 1e-4                           # tests/test_gpu_flow.py
SHAPES = {f"D{D}": (D, None) for D in (3, 10, 17, 33, 65, 86, 97, 102, 108, 128, 157)}
SHAPES.update({"D10-nsf3": (10, "nsf3"), "D32-nsf6": (32, "nsf6")})
# beyond the fragments held in registers, where the kernel loads in place: 64 live hidden tiles (the hidden update past
# 8 * 7 + 1 tiles)
SHAPES.update({"D65-H1024": (65, MAFSpec(65, 2, hidden=1024, univariate="rqs"))})


def _spec(name):
    D, chain = SHAPES[name]
    if isinstance(chain, MAFSpec):
        return chain
    return spec_by_name(D, chain) if chain else MAFSpec(D, 2, univariate="rqs")


@functools.lru_cache(maxsize=None)
def flow_of(name):
    """One flow per shape for the whole module: (Flow with AUTO's inverse, spec, float32 oracle)."""
    from pocomc_amd import Flow
    spec = _spec(name)
    flat = cases.flow_params(spec, 3, gain=1.0)
    f = Flow(spec.n_dim, spec)
    f.set_params(flat)
    return f, spec, OracleMAF(spec, flat)


def latent(n, D, seed, scale=1.5):
    return (np.random.default_rng(seed).normal(size=(n, D)) * scale).astype(np.float32)


def run(f, z, algo):
    rc, xb, lb = _inverse(f, torch.from_numpy(z).cuda(), algo)
    assert rc == 0, f.lib.pmc_last_error()
    return xb.view(np.float32), lb.view(np.float32)


def held(x, l, xr, lr, terms, what):
    print(f"{what}: x {close_rel(x, xr, np.inf, what + ' x (measured)'):.2e} "
          f"ladj {close_rel(l, lr, np.inf, what + ' ladj (measured)', cancel=terms):.2e}")
    close_rel(x, xr, NSF_INV, what + " x")
    close_rel(l, lr, NSF_LADJ, what + " ladj", cancel=terms)


# ------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_sweep_matches_the_oracles_dpass(name, n):
    f, spec, o = flow_of(name)
    D = spec.n_dim
    from pocomc_amd import _lib
    plan = _lib.pmc_inverse_plan_t()
    assert f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, WG_NSF, 0, C.byref(plan)) == 0 and plan.sweep == S_WG_NSF
    z = latent(n, D, 7 + n + D)
    xo, lo = o.inverse(z)                                    # the reference's D-pass algorithm
    x, l = run(f, z, WG_NSF)
    held(x, l, xo, lo, o.ladj_abs_terms(xo), f"workgroup spline sweep {name} n={n}")


def test_more_than_one_round_matches_the_devices_dpass():
    """4097 rows: 257 workgroups, the last with a single row."""
    f, spec, o = flow_of("D102")
    z = latent(4097, 102, 11)
    xd, ld = run(f, z, NAIVE)
    x, l = run(f, z, WG_NSF)
    held(x, l, xd, ld, o.ladj_abs_terms(xd), "workgroup spline sweep vs device D-pass, 4097 rows")


@pytest.mark.parametrize("name", ["D33", "D86", "D128"])
def test_the_sweep_matches_the_lone_wave_spline_sweep(name):
    f, spec, o = flow_of(name)
    z = latent(33, spec.n_dim, 21)
    xs, ls = run(f, z, NSF_SOLO)
    x, l = run(f, z, WG_NSF)
    held(x, l, xs, ls, o.ladj_abs_terms(xs), f"workgroup spline sweep vs lone-wave sweep {name}")


@pytest.mark.parametrize("name", ["D3", "D10", "D10-nsf3"])
def test_short_flows_give_the_lone_wave_sweeps_bits(name):
    """Products of fewer than 16 K tiles are not split by K range and add in the lone-wave sweep's order; with one x tile
    (D <= 16) layer 0 does too, and the two sweeps are the same arithmetic."""
    f, spec, _ = flow_of(name)
    assert spec.nT < 16 and spec.nXT == 1
    z = latent(33, spec.n_dim, 23)
    xs, ls = run(f, z, NSF_SOLO)
    x, l = run(f, z, WG_NSF)
    assert np.array_equal(_bits(x), _bits(xs)) and np.array_equal(_bits(l), _bits(ls))


def test_round_trip():
    f, spec, _ = flow_of("D102")
    z = latent(33, 102, 5)
    x, _ = run(f, z, WG_NSF)
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
        rc = f.lib.pmc_maf_inverse(C.byref(f._desc), _lib.ptr(z), _lib.ptr(x), _lib.ptr(ladj) if with_ladj else None, n, WG_NSF,
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
    """Every data-derived index of the kernel is select-based and stays in the row's own panel (``rqs_inverse_coop``)."""
    f, spec, _ = flow_of("D33")
    z = latent(33, 33, 9)
    x, l = run(f, z, WG_NSF)
    bad = z.copy()
    bad[5] = np.nan
    bad[20, 0] = np.inf
    xb, lb = run(f, bad, WG_NSF)
    keep = np.ones(33, dtype=bool)
    keep[[5, 20]] = False
    assert np.array_equal(_bits(xb[keep]), _bits(x[keep])) and np.array_equal(_bits(lb[keep]), _bits(l[keep]))
    assert not np.isfinite(xb[5]).all() and not np.isfinite(xb[20]).all()


# ------------------------------------------------------------------------------------------ the spline's box, the regimes
def test_coordinates_outside_the_spline_box_come_back_bit_for_bit():
    spec, flat, data = regimes.fixture("nsf6-d10-g4")
    f = regimes.flow(spec, flat)
    x, out = fr.outside_rows(spec, data[:64])
    allout = out.all(axis=1)
    assert allout.sum() >= 4
    f.inverse_algo = WG_NSF
    xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(x)))
    np.testing.assert_array_equal(xi[out], x[out])
    np.testing.assert_array_equal(li[allout], 0.0)


@pytest.mark.parametrize("name", ["nsf6-d10-g4", "nsf6-d10-fit"])
def test_the_sweep_meets_the_regime_criterion(name):
    """``tests/test_gpu_flow_regimes.py``'s criterion, inputs (latent rows, knot rows, box rows) and float32 evaluations."""
    spec, flat, data = regimes.fixture(name)
    f = regimes.flow(spec, flat)
    ev = [OracleMAF(spec, flat), fr.KernelSplineOracle(spec, flat), fr.SequentialOracle(spec, flat)]
    u = regimes.inverse_inputs(spec, flat, data, f)
    R = fr.Reference(spec, flat, u, "inverse", k=fr.N_PERTURB)
    f32 = [dict(zip(("x", "ladj"), e.inverse(u))) for e in ev]
    f.inverse_algo = WG_NSF
    xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(u)))
    regimes.check(R, "x", xi, f"inverse algorithm {WG_NSF}, {name}", [d["x"] for d in f32])
    regimes.check(R, "ladj", li, f"inverse algorithm {WG_NSF}, {name}", [d["ladj"] for d in f32])


# ------------------------------------------------------------------------------------------ in the step
@pytest.mark.parametrize("D", [33, 102])
def test_the_step_launches_the_sweep_unfused(D, monkeypatch):
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd.mcmc import StepEngine
    spec = MAFSpec(D, 2, univariate="rqs")
    flow = pc.Flow(D, spec, seed=1)
    flow.inverse_algo = WG_NSF
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
    rc, xb, lb = _inverse(flow, theta32, WG_NSF)
    assert rc == 0
    assert np.array_equal(_bits(a["u32"]), xb) and np.array_equal(_bits(a["ldjf"]), lb)
    b = _pre_step(monkeypatch, 1, n, D, flow, scaler, prior, x, u)
    for k in ("u32", "ldjf", "x", "finite", "theta"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["done"][0] == 1 and b["done"][0] == 1 and (a["finite"] != 0).sum() >= n - 1
    assert flow.inverse_algo == WG_NSF


# ------------------------------------------------------------------------------------------ the Flow surface
def test_flow_argument_and_pickle():
    from pocomc_amd import Flow
    f, spec, _ = flow_of("D102")
    assert f.inverse_algo == 0 and f.inverse_sweep == "auto"
    g = Flow(102, MAFSpec(102, 2, univariate="rqs"), inverse_sweep="workgroup_spline")
    g.set_params(f.params.cpu().numpy())
    assert g.inverse_algo == WG_NSF and g.inverse_sweep == "workgroup_spline"
    z = latent(33, 102, 13)
    x, l = run(f, z, WG_NSF)
    xg, lg = g.inverse(torch.from_numpy(z))
    assert np.array_equal(_bits(xg.numpy()), _bits(x)) and np.array_equal(_bits(lg.numpy()), _bits(l))
    h = pickle.loads(pickle.dumps(g))
    assert h.inverse_algo == WG_NSF and h.inverse_sweep == "workgroup_spline"
    xh, lh = h.inverse(torch.from_numpy(z))
    assert np.array_equal(_bits(xh.numpy()), _bits(x)) and np.array_equal(_bits(lh.numpy()), _bits(l))


def test_flow_argument_refusals():
    from pocomc_amd import Flow
    with pytest.raises(ValueError, match="inverse_sweep must be"):
        Flow(10, "nsf3", inverse_sweep="lane")
    with pytest.raises(ValueError, match="unknown algo"):
        Flow(10, "maf3", inverse_sweep="workgroup_spline")
    with pytest.raises(ValueError, match="degree groups <= one tile"):
        Flow(2, "nsf3", inverse_sweep="workgroup_spline")
    with pytest.raises(ValueError, match="built for 8 bins"):
        Flow(10, MAFSpec(10, 2, univariate="rqs", bins=16), inverse_sweep="workgroup_spline")
    assert Flow(10, "nsf3").inverse_algo == 0


# ------------------------------------------------------------------------------------------ a run
def test_a_sampler_runs_with_the_workgroup_spline_sweep_at_100_dimensions():
    """The prior, likelihood, sizes and assertions of ``test_a_sampler_runs_with_the_workgroup_sweep_at_100_dimensions``
    (``tests/test_gpu_wide_sweep.py``), with a ready nsf6 flow -- the default family -- that inverts with this sweep."""
    from scipy.stats import uniform
    import pocomc_amd as pc
    D = 100

    def loglike(x):
        return -0.5 * np.sum((x / 50.0) ** 2, axis=1)

    prior = pc.Prior([uniform(-10, 20)] * D)
    flow = pc.Flow(D, "nsf6", inverse_sweep="workgroup_spline")
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
    assert s.flow.inverse_algo == WG_NSF
