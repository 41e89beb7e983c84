"""The numpy / scipy restatement of the Student-t EM fit (``tests/student_em.py``) on inputs with a known answer, and the
parts of ``Geometry(student=...)`` that need no GPU."""
import functools
import pickle

import numpy as np
import pytest

import student_em as se


@pytest.mark.parametrize("seed,n,D,nu", [(1, 2048, 6, 4.0), (2, 1000, 32, 8.0)])
def test_restatement_recovers_nu(seed, n, D, nu):
    x = se.mvt_rows(seed, n, D, nu)
    r = se.fit(x, *se.start_values(x))
    print(f"t_{nu:g} rows {n} x {D}: nu = {r['nu']:.4f} after {r['iterations']} iterations ({r['status']})")
    assert r["status"] == "converged" and r["iterations"] < 100
    assert abs(r["nu"] - nu) < 0.15 * nu
    assert np.isfinite(r["mu"]).all() and np.linalg.eigvalsh(r["sigma"]).min() > 0


def test_restatement_leaves_gaussian_rows_at_the_first_iteration():
    x = se.mvt_rows(3, 2048, 6, np.inf)
    mu0, s0 = se.start_values(x)
    r = se.fit(x, mu0, s0)
    assert r["status"] == "nu_inf" and r["iterations"] == 1 and r["nu"] == np.inf
    assert np.array_equal(r["mu"], mu0) and np.array_equal(r["sigma"], s0)


def test_geometry_rejects_an_unknown_student_mode():
    from pocomc_amd.geometry import Geometry
    with pytest.raises(ValueError):
        Geometry(student="bogus")
    assert Geometry().student == "reference" and Geometry(student="em").student == "em"


def test_geometry_from_an_older_checkpoint_is_in_reference_mode():
    """A ``Geometry`` pickled before the attribute existed has no ``student`` in its state."""
    from pocomc_amd.geometry import Geometry
    g = Geometry()
    state = dict(g.__dict__)
    del state["student"], state["student_info"]
    old = Geometry.__new__(Geometry)
    old.__dict__.update(state)
    back = pickle.loads(pickle.dumps(old))
    assert "student" not in back.__dict__
    assert back.student == "reference" and back.student_info is None


# ------------------------------------------------------------------------------------------------------------------
# The conditions on the inputs of ``tests/test_gpu_student_em_edges.py``, held by the restatement: a change to
# ``mvt_rows`` or to the restatement cannot move an input out of its regime unnoticed.
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_fit(seed, n, D, nu, **kw):
    x = se.mvt_rows(seed, n, D, nu)
    return se.fit(x, *se.start_values(x), **kw)


def permuted_fit(seed, n, D, nu):
    x = se.mvt_rows(seed, n, D, nu)
    return se.fit(x[np.random.default_rng(99).permutation(n)], *se.start_values(x), xtol=1e-11)


@pytest.mark.parametrize("args,status,nu,iterations", [
    ((1, 4096, 4, 100), "converged", 166.22, 23), ((1, 4096, 4, 300), "converged", 356.76, None),
    ((1, 4096, 4, 1000), "converged", 588.26, None), ((2, 4096, 4, 1000), "converged", 764.30, 22),
    ((1, 4096, 4, 3000), "max_iter", 598.28, 100), ((2, 4096, 4, 3000), "max_iter", 1291.4, 100),
    ((2, 40, 3, 4), "converged", 3.169, 46), ((2, 63, 1, 3), "converged", 138.96, 40),
    ((3, 65, 1, 1), "converged", 0.8546, 68), ((4, 1024, 3, 1), "converged", 0.9057, 76),
    ((4, 1024, 3, 0.3), "lower_clamp", se.NU_LO, 2), ((4, 1024, 3, 0.5), "lower_clamp", se.NU_LO, 2),
    ((1, 3, 2, 4), "nu_inf", np.inf, 1), ((1, 7, 6, 4), "nu_inf", np.inf, 1), ((3, 129, 128, 5), "nu_inf", np.inf, 1)])
def test_the_inputs_are_in_their_regimes(args, status, nu, iterations):
    r = table_fit(*args)
    print(f"{args}: {r['status']}, nu = {r['nu']:.6g}, {r['iterations']} iterations, last steps {r['steps'][-2:]}")
    assert r["status"] == status
    assert r["nu"] == nu if not np.isfinite(nu) or nu == se.NU_LO else abs(r["nu"] - nu) < 1e-3 * nu
    assert iterations is None or r["iterations"] == iterations


def test_the_stopping_iteration_above_nu_1000_depends_on_rounding_and_nu_does_not():
    """t_3000 rows: the restatement runs to ``max_iter`` with |delta nu| stuck just above ``tol``; the same rows in another
    order converge in 22 iterations, at the same nu to 1e-7."""
    for args, stuck in (((1, 4096, 4, 3000), 1.36e-6), ((2, 4096, 4, 3000), None)):
        a, b = table_fit(*args), permuted_fit(*args)
        print(f"{args}: {a['iterations']} iterations (last step {a['steps'][-1]:.3e}), permuted {b['iterations']}; "
              f"nu differs by {abs(a['nu'] - b['nu']) / a['nu']:.1e}")
        assert a["status"] == "max_iter" and a["iterations"] == 100 and a["steps"][-1] > 1e-6
        assert stuck is None or abs(a["steps"][-1] - stuck) < 0.01e-6
        assert b["status"] == "converged" and b["iterations"] < 30
        assert abs(a["nu"] - b["nu"]) < 1e-7 * a["nu"]


def test_fixed_length_on_the_largest_d():
    x = se.mvt_rows(3, 200, 128, 5)
    r = se.fit(x, *se.start_values(x), tol=0.0, max_iter=5)
    assert r["status"] == "max_iter" and r["iterations"] == 5 and abs(r["nu"] - 7.959) < 1e-3


@pytest.mark.parametrize("n,D", se.EDGE_SHAPES)
def test_edge_shapes_run_their_fixed_length_and_the_restatement_is_quiet_there(n, D):
    """``tol = 0``: the fit has ``max_iter`` iterations (no Gaussian exit, every Cholesky succeeds), and the restatement's
    own reordering noise leaves the device tests' 1e-9 a factor of 100 or more."""
    for f32 in (False, True):
        for indexed in (False, True):
            rows = se.edge_rows(n, D, f32, indexed)[2]
            assert rows.shape == (n, D)
            start = se.start_values(rows)
            for max_iter in (1, 4):
                r = se.fit(rows, *start, tol=0.0, max_iter=max_iter)
                assert r["status"] == "max_iter" and r["iterations"] == max_iter
                assert se.NU_LO < r["nu"] < se.NU_HI
            if not f32:
                assert max(se.reorder_noise(rows, *start, perms=2, tol=0.0, max_iter=4)) < 1e-11


@pytest.mark.parametrize("args", [(1, 3, 2, 4), (1, 7, 6, 4), (3, 129, 128, 5)])
def test_one_row_more_than_dimensions_is_gaussian_to_the_fit(args):
    x = se.mvt_rows(*args)
    assert x.shape[0] == x.shape[1] + 1
    mu0, s0 = se.start_values(x)
    r = se.fit(x, mu0, s0)
    assert r["status"] == "nu_inf" and r["iterations"] == 1 and r["nu"] == np.inf
    assert np.array_equal(r["mu"], mu0) and np.array_equal(r["sigma"], s0)


@pytest.mark.parametrize("k", range(len(se.NU_AXIS)))
def test_nu_axis_roots_and_noise_are_the_recorded_ones(k):
    args, c, root, d = se.NU_AXIS[k]
    x = se.mvt_rows(*args)
    start = se.scaled_start(x, c)
    r = se.fit(x, *start, tol=0.0, max_iter=1)
    m = se.reorder_noise(x, *start, tol=0.0, max_iter=1)
    print(f"{args} c = {c}: first root {r['nu']:.6g}; reorder noise nu {m[0]:.2e} mu {m[1]:.2e} Sigma {m[2]:.2e}")
    assert r["status"] == "max_iter" and r["iterations"] == 1
    assert abs(r["nu"] - root) < 1e-5 * root
    assert all(a <= b for a, b in zip(m, d)), (m, d)                     # (the recorded figures bound the measured ones)
    assert all(b <= 2.0 * a + 1e-15 for a, b in zip(m, d)), (m, d)       # (and are no slack of their own)


def test_nu_axis_covers_every_decade_and_both_ends():
    roots = np.array([r for _, _, r, _ in se.NU_AXIS])
    for lo in (0.1, 1.0, 10.0, 100.0, 1000.0):
        assert ((roots >= lo) & (roots <= 10.0 * lo)).any(), lo
    assert roots.min() < 2.0 * se.NU_LO and roots.max() > 0.5 * se.NU_HI
    # rows far on either side of |u| = 1/2, u = (D - delta) / (nu + delta): delta << D and delta >> nu + D
    args, c, root, _ = se.NU_AXIS_STRADDLE
    x = se.mvt_rows(*args)
    delta = se.first_deltas(x, *se.scaled_start(x, c))
    assert delta.min() < 1e-3 * args[2] and delta.max() > 1e3 * (root + args[2])
    u = (args[2] - delta) / (root + delta)
    assert (np.abs(u) < 0.5).sum() >= 32 and (np.abs(u) >= 0.5).sum() >= 32
    # all |u| < 1/2 at every nu of the bracket (|u| falls with nu)
    args, c, root, _ = se.NU_AXIS_NEAR_ONE
    x = se.mvt_rows(*args)
    delta = se.first_deltas(x, *se.scaled_start(x, c))
    assert np.abs((args[2] - delta) / (se.NU_LO + delta)).max() < 0.5


@pytest.mark.parametrize("args,root", [((1, 4096, 4, 1000), 977.678), ((2, 4096, 4, 1000), 1215.24)])
def test_a_plateau_hides_the_restatements_noise(args, root):
    """Why these two roots are not on the nu axis of the device tests (``student_em.NU_AXIS``): brentq stops on a value of
    exactly zero, the permutations all find it again, and f(nu) stays within two ulp of log(nu / 2) over +-1e-8 of nu."""
    x = se.mvt_rows(*args)
    start = se.start_values(x)
    r = se.fit(x, *start, tol=0.0, max_iter=1)
    assert abs(r["nu"] - root) < 1e-5 * root
    delta = se.first_deltas(x, *start)
    assert se.f_nu(r["nu"], delta, args[2]) == 0.0
    assert se.reorder_noise(x, *start, perms=4, tol=0.0, max_iter=1)[0] == 0.0
    step = np.spacing(np.log(r["nu"] / 2))
    assert all(abs(se.f_nu(r["nu"] * (1 + e), delta, args[2])) <= 2 * step for e in (-1e-8, -5e-9, 5e-9, 1e-8))


@pytest.mark.parametrize("k", range(len(se.LARGE_NU)))
def test_large_nu_fits_and_their_noise_are_the_recorded_ones(k):
    args, nu, d = se.LARGE_NU[k]
    x = se.mvt_rows(*args)
    start = se.start_values(x)
    r = table_fit(*args)
    m = se.reorder_noise(x, *start)
    print(f"{args}: nu {r['nu']:.6g} ({r['status']}, {r['iterations']} iterations); reorder noise nu {m[0]:.2e} mu {m[1]:.2e} "
          f"Sigma {m[2]:.2e}")
    assert r["status"] in ("converged", "max_iter") and abs(r["nu"] - nu) < 1e-5 * nu
    assert all(a <= b for a, b in zip(m, d)), (m, d)
    assert all(b <= 2.0 * a for a, b in zip(m, d)), (m, d)


@pytest.mark.parametrize("args,iterations", [((4, 1024, 3, 1), 76), ((3, 65, 1, 1), 68)])
def test_heavy_tailed_fits_stop_clear_of_the_tolerance(args, iterations):
    r = table_fit(*args)
    assert r["status"] == "converged" and r["iterations"] == iterations and 0.8 < r["nu"] < 1.0
    assert all(not (0.99e-6 <= s <= 1.01e-6) for s in r["steps"][-2:])


def test_collinear_rows_end_the_fit_at_the_second_cholesky():
    x = se.collinear_rows()
    assert np.array_equal(x[:, 1], 2.0 * x[:, 0]) and np.linalg.matrix_rank(x - x.mean(axis=0)) == 2
    mu0, s0 = se.start_values(x)
    for sigma0 in (s0 + np.eye(x.shape[1]), s0):                         # the caller's + I; Geometry.fit's own start
        np.linalg.cholesky(sigma0)
        r = se.fit(x, mu0, sigma0)
        assert r["status"] == "not_pd" and r["iterations"] == 2 and len(r["steps"]) == 1
        one = se.fit(x, mu0, sigma0, max_iter=1)
        assert np.array_equal(one["sigma"], r["sigma"]) and np.array_equal(one["mu"], r["mu"])
        # rank 3 (the rows' plane and the way to the column medians, which do not lie in it): five eigenvalues are rounding
        ev = np.linalg.eigvalsh(r["sigma"])
        assert np.abs(ev[:-3]).max() < 1e-13 * ev[-1] and ev[-3] > 1e-6 * ev[-1]


# ------------------------------------------------------------------------------------------------------------------
# The conditions on the nu = 0.1 cases of ``tests/test_gpu_step_nu_range.py`` (``cases.NU_RANGE_CASES``), on the oracle alone
# ------------------------------------------------------------------------------------------------------------------
def oracle_trace(name):
    import cases
    from oracle import mcmc as omcmc
    from oracle.maf import OracleMAF, TorchFlowAdapter
    from oracle.scaler import Reparameterize as OracleScaler
    c = cases.NU_RANGE_CASES[name]
    state, funcs, opts, aux = cases.build_case(name, OracleScaler, c)
    funcs["flow"] = TorchFlowAdapter(OracleMAF(aux["spec"], aux["flat"]))
    trace = []
    np.random.seed(c["seed"])
    omcmc.preconditioned_pcn(state, funcs, opts, rng=omcmc.LegacyStream(), trace=trace)
    return c, trace


def nu_range_names(pred):
    import cases
    return [k for k, c in cases.NU_RANGE_CASES.items() if pred(k, c)]


def test_nu_range_cases_cover_what_they_say():
    import cases
    cs = cases.NU_RANGE_CASES.values()
    assert {c["nu"] for c in cs} == {0.1, 0.9057, 588.26, 1e4}
    assert {(c["N"], c["D"]) for c in cs} == {(96, 2), (80, 5), (128, 10)}
    assert {c["prior"] for c in cs} == {"uniform", "mixed"}
    assert any(c.get("flow") == "rqs" for c in cs) and any(c.get("periodic") and c.get("reflective") for c in cs)
    assert not set(cases.NU_RANGE_CASES) & (set(cases.MCMC_CASES) | set(cases.BIG_CASES) | set(cases.BIG_GOLDEN_CASES))
    assert all(cases.NU_RANGE_CASES[k]["nu"] == 0.1 for k in cases.NU_RANGE_REJECTING)


@pytest.mark.parametrize("name", nu_range_names(lambda k, c: c["nu"] == 0.1))
def test_the_oracle_at_the_lower_clamp_rejects_outright_where_the_prior_is_half_bounded(name):
    """Half-bounded coordinates, affine flow: in some step a proposal is not finite (x' or its log-determinant) or leaves the prior's
    support, and more than half stay finite.
    The box prior and the spline flow: every proposal reaches the likelihood."""
    import cases
    c, trace = oracle_trace(name)
    rejected = [int((~tr["finite"]).sum()) for tr in trace]
    print(f"{name}: rejected before the likelihood per step {rejected}; largest |theta'| "
          f"{max(float(np.abs(tr['theta_prime']).max()) for tr in trace):.3g}")
    assert len(trace) == c["n_max"]
    if name in cases.NU_RANGE_REJECTING:
        assert 1 <= max(rejected) <= c["N"] // 2
    else:
        assert max(rejected) == 0


def test_the_affine_inverse_is_ill_conditioned_on_the_farthest_proposals():
    """The figure behind ``test_gpu_mcmc.FLOW_ULPS``'s use: at nu = 0.1 the exact (float64) inverse of the float32 flow moves by
    more than 1e-5 when theta' moves by one float32 ulp, on a proposal that the step rejects outright -- and on all but a
    few walkers by less than 1e-6."""
    from oracle.maf import OracleMAF
    from test_gpu_mcmc import FLOW_ULPS, TOL, ulp_response
    import cases
    from oracle.scaler import Reparameterize as OracleScaler
    name = "tpcn_nu0p1_n128_d10_mixed"
    c, trace = oracle_trace(name)
    aux = cases.build_case(name, OracleScaler, c)[3]
    flow64 = OracleMAF(aux["spec"], aux["flat"], dtype=np.float64)
    r = np.array([ulp_response(flow64, tr["theta_prime"]) for tr in trace])
    fin = np.array([tr["finite"] for tr in trace])
    print(f"{name}: largest response to one ulp {r.max():.2e}; walkers above TOL / FLOW_ULPS per step {(FLOW_ULPS * r > TOL).sum(axis=1)}")
    assert 1e-5 < r.max() < 3e-5 and not fin.ravel()[r.argmax()]
    assert (FLOW_ULPS * r > TOL).sum(axis=1).max() <= 3 and np.median(r) < 1e-6
