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
import ctypes as C
import functools
import time

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
    # default width at D = 102: Hp = 816, 51 hidden tiles -- AUTO is the lean D-pass kernel, the workgroup sweeps (algorithms
    # 10 / 11) the only triangular ones.  maf6-d102-fit: the flow of test_a_sampler_runs_with_the_workgroup_sweep_at_100_dimensions
    "maf6-d102-fit": (lambda: MAFSpec(102, 6), lambda: fr.bimodal_draws(102, 4000, 6)),
    "nsf3-d102-fit": (lambda: MAFSpec(102, 3, univariate="rqs"), lambda: fr.two_modes(102, 4000, 7)),
}
EPOCHS = {"maf8-d128-fit": 10}      # config 5's validation loss is best near epoch 5 and diverges by 50 (bench.py)


# OPEN FINDING (asserted failing, test_open_finding_*): the on-device D-pass inverse (algorithm 2, the cross-check kernel;
# AUTO never takes it for these flows) on the affine flow with its output layer x16 misses C e_i on the inverse
# log-determinant on 15 of 192 rows (worst 0.09), where float32 evaluations in two other orders of addition miss up to 6
# (worst 0.09): the same magnitude, more than twice the rows.  Not explained yet.
#
# ("maf3-d10-g16", 10): the affine workgroup sweep on the same rows misses THE SAME 15 rows (worst 0.093; the float32
# evaluations: 6 rows, worst 0.093; limit 2 x 6).  Measured since: the numpy oracle, the sequential oracle and eight more
# float32 evaluations of the hyper-network on the host (bias first, terms in index order, reversed, six random orders) miss
# 4 to 6 rows each, every one of them among these 15; the register-chain and lane sweeps (algorithms 0, 1, 6, 7, 8) miss
# 2 or 3 of them.  What the D-pass kernel and the workgroup sweep share, and no other evaluation has, is the dense kernels'
# order -- bias first, K tiles ascending on two accumulators -- with the IEEE forms of the soft clip and the division.
# Which of the two it is, is not found.
#
# ("maf3-d102-g16", "forward z"): the lean forward kernel at 51 hidden tiles and gain 16 meets the row criterion on every
# row (worst err 2.3e-06, worst err/e 7.0) and misses the MEDIAN rule: median err/e 2.43 against 1.25 x the numpy
# oracle's 1.92 = 2.40 (32 rows, k = 4).  Over three envelope seeds and k = 4 / 8 the kernel's median is 1.21 - 1.35 x
# numpy's; the host's sequential float32 evaluation (one rounded product and one rounded sum per term) has 2.76 on the same
# rows, so the kernel lies between two float32 orders of addition.  The criterion takes only the numpy oracle here; at
# gain 2 and 3 the same kernel's median is below numpy's (1.51 / 1.73, 2.32 / 2.48).  ("maf3-d102-g16", "forward log_prob"):
# the same rows, the same rule, through -z^2 / 2 -- no row beyond (worst err 2.3e-06), median 2.45 against 1.25 x 1.92.
# The log-determinant meets the criterion (median 0.5).
OPEN_FINDINGS = {("maf3-d10-g16", 2), ("maf3-d10-g16", 10), ("maf3-d102-g16", "forward z"), ("maf3-d102-g16", "forward log_prob")}


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
FIXTURES = list(FITTED) + list(GAIN) + list(fr.WIDE_GAIN)
WIDE = ("maf6-d102-fit", "nsf3-d102-fit") + tuple(fr.WIDE_GAIN)          # default width, n_dim 86 / 102 / 128: the non-vacuity condition holds
FORWARD_ONLY = fr.WIDE_FORWARD_ONLY                                      # forward, log_prob and the trainer's loss only
ROWS = fr.ROWS                                                           # forward / inverse rows per D (float64 D-pass cost)

AUTO, NAIVE, WG, WG_NSF = 0, 2, 10, 11
S_NSF_SOLO, S_DPASS_LEAN, S_WG, S_WG_NSF = 6, 8, 9, 10                    # include/pocomc_amd.h PMC_SWEEP_*
DPASS_SWEEPS = (1, 2, S_DPASS_LEAN)
# what ``algorithms`` listed for each fixture before it asked the plan: it lists at least these
LISTED_BEFORE = {"maf3-d10-fit": [0, 1, 2, 8, 6, 7], "maf3-d32-fit": [0, 1, 2, 8, 6, 7], "nsf6-d10-fit": [0, 1, 2, 6, 7],
                 "nsf3-d32-fit": [0, 1, 2, 6, 7], "maf6-d50-fit": [0, 1, 2, 8, 6, 7], "maf8-d128-fit": [0, 1, 2, 8],
                 "maf3-d10-g4": [0, 1, 2, 8, 6, 7], "maf3-d10-g16": [0, 1, 2, 8, 6, 7], "nsf6-d10-g4": [0, 1, 2, 6, 7]}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(spec, float32 parameters, data rows)."""
    from pocomc_amd import Flow
    if name in fr.WIDE_GAIN:
        return fr.wide_gain_fixture(name)
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


def plan_of(f, n, algo, fused=0):
    """The plan of ``f``'s inverse of ``n`` rows with ``algo`` (csrc/inverse_plan.hip), or None where ``pmc_maf_inverse``
    refuses the call."""
    from pocomc_amd import _lib
    p = _lib.pmc_inverse_plan_t()
    return p if f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, algo, fused, C.byref(p)) == 0 else None


def algorithms(f, n=64):
    """Every inverse the plan admits for the flow ``f`` and a call of ``n`` rows, AUTO first: the candidates of
    tests/test_gpu_flow.py that the plan does not refuse (the default-width flows at D = 102 keep AUTO and NAIVE, both the
    lean D-pass kernel), and the workgroup sweep of the flow's family -- algorithm 10 / 11 -- where the plan gives it
    ``PMC_SWEEP_WG`` / ``PMC_SWEEP_WG_NSF``."""
    spec = f.spec
    if not spec.tri_ok:
        cand = [0, 2]
    elif spec.univariate == "rqs":
        cand = [0, 1, 2, 6, 7]
    else:
        small = spec.nOT <= 8 and 2 * spec.Dp + 3 * spec.Hp + 176 <= 2560
        cand = [0, 1, 2, 8] + ([6, 7] if small else [])
    out = [a for a in cand if plan_of(f, n, a) is not None]
    wg, sweep = (WG_NSF, S_WG_NSF) if spec.univariate == "rqs" else (WG, S_WG)
    p = plan_of(f, n, wg)
    if p is not None and p.sweep == sweep:
        out.append(wg)
    return out


def forward_inputs(spec, flat, data):
    return fr.forward_inputs(spec, flat, data)


def inverse_inputs(spec, flat, data, f):
    """(latent images: the device's forward map of the flow's own rows)"""
    return fr.inverse_inputs(spec, flat, data, lambda x: f.forward(torch.from_numpy(x))[0].numpy())


check = fr.check            # (the criterion with its float32 evaluations: tests/flow_regimes.py)


def evaluations(spec, flat):
    """The float32 evaluations ``check`` holds a kernel against: the numpy oracle, the kernels' spline formulas (spline
    flows), the sequential dot products (a python loop per term: D <= 10 only)."""
    ev = [OracleMAF(spec, flat)]
    if spec.univariate == "rqs":
        ev.append(fr.KernelSplineOracle(spec, flat))
    if spec.n_dim <= 10:
        ev.append(fr.SequentialOracle(spec, flat))
    return ev


def _evaluated(ev, inp, direction):
    if direction == "forward":
        return [dict(zip(("z", "ladj"), e.forward(inp)), log_prob=e.log_prob(inp)) for e in ev]
    return [dict(zip(("x", "ladj"), e.inverse(inp))) for e in ev]


@functools.lru_cache(maxsize=None)
def wide_reference(name, direction):
    """(rows, Reference, float32 evaluations) of a default-width fixture, once per session (the float64 D-pass inverse of a
    spline flow at D = 102 takes ~10 s of host time): its fixed rows do not pass through a kernel -- the latent images are
    the float32 oracle's -- and the non-vacuity condition is asserted on them before any kernel is judged."""
    spec, flat, data = fixture(name)
    t0 = time.perf_counter()
    inp = fr.forward_inputs(spec, flat, data) if direction == "forward" else fr.inverse_inputs(spec, flat, data, fr.oracle_latent(spec, flat))
    R = fr.Reference(spec, flat, inp, direction, k=fr.n_perturb(spec))
    shares = fr.assert_non_vacuous(R, name)
    f32 = _evaluated(evaluations(spec, flat), inp, direction)
    print(f"reference, {name} {direction}: {len(inp)} rows, {int(R.ok.sum())} counted, share with C e_i <= {fr.WELL:g}: "
          + ", ".join(f"{q} {s:.3f}" for q, s in shares.items()) + f"; {time.perf_counter() - t0:.1f} s of host time")
    return inp, R, f32


def reference(name, direction, f):
    if name in WIDE:
        return wide_reference(name, direction)
    spec, flat, data = fixture(name)
    inp = forward_inputs(spec, flat, data) if direction == "forward" else inverse_inputs(spec, flat, data, f)
    R = fr.Reference(spec, flat, inp, direction, k=fr.n_perturb(spec))
    return inp, R, _evaluated(evaluations(spec, flat), inp, direction)


def _assert_the_listed_sweeps(name, f, algos):
    """What the plan admits, by name: the old fixtures list at least what they listed before and their family's workgroup
    sweep; at D = 102 AUTO and NAIVE are the lean D-pass kernel and the workgroup sweep is the only triangular one; at
    D = 128 (spline) AUTO is the lone-wave sweep.  And which regime of ``output_partials`` (csrc/maf_inverse_wg_nsf.hip) a
    spline flow reaches: products of >= 16 K tiles, dealt by K range, need 17 hidden tiles."""
    spec = f.spec
    wg = WG_NSF if spec.univariate == "rqs" else WG
    assert algos[0] == AUTO and wg in algos, (name, algos)
    if name in LISTED_BEFORE:
        assert set(LISTED_BEFORE[name]) <= set(algos), (name, algos)
    if spec.n_dim == 102:
        assert algos == [AUTO, NAIVE, wg], (name, algos)
        assert plan_of(f, 64, AUTO).sweep == S_DPASS_LEAN and plan_of(f, 64, NAIVE).sweep == S_DPASS_LEAN
    if name in ("nsf3-d128-g2", "nsf3-d86-g2"):
        assert plan_of(f, 64, AUTO).sweep == S_NSF_SOLO and {NAIVE, WG_NSF} <= set(algos), (name, algos)
    if spec.univariate == "rqs":
        # 17 hidden tiles are needed for a product of 16 K tiles, and a tile of one or two degree groups for the split
        split = fr.k_split_tiles(spec)
        if spec.n_dim in (86, 102):
            assert spec.nT >= 17 and split >= 16, (name, spec.nT, split)
        if spec.n_dim == 10:
            assert spec.nT < 17 and split == 0, (name, spec.nT, split)
        if spec.n_dim == 128:
            assert spec.nT >= 17 and split == 0, (name, spec.nT, split)          # (long products, none of them split)


@pytest.mark.parametrize("name", FIXTURES)
def test_forward_log_prob_and_every_inverse_meet_the_criterion(name, only_algo=None):
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    x, R, f32 = reference(name, "forward", f)
    z, l = (t.numpy() for t in f.forward(torch.from_numpy(x)))
    lp = f.log_prob(torch.from_numpy(x)).numpy()
    for q, v in (("z", z), ("ladj", l), ("log_prob", lp)):
        if (only_algo is None) != ((name, f"forward {q}") in OPEN_FINDINGS) and only_algo in (None, f"forward {q}"):
            check(R, q, v, f"forward, {name}", [d[q] for d in f32])
    algos = algorithms(f, ROWS[spec.n_dim][1])
    _assert_the_listed_sweeps(name, f, algos)
    if name in FORWARD_ONLY or isinstance(only_algo, str):
        return
    u, R, f32 = reference(name, "inverse", f)
    assert algos == algorithms(f, len(u))
    for algo in algos:
        if (only_algo is None) == ((name, algo) in OPEN_FINDINGS) or (only_algo is not None and algo != only_algo):
            continue
        f.inverse_algo = algo
        xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(u)))
        fam = f"inverse algorithm {algo}" if algo else "inverse AUTO"
        check(R, "x", xi, f"{fam}, {name}", [d["x"] for d in f32])
        check(R, "ladj", li, f"{fam}, {name}", [d["ladj"] for d in f32])


@pytest.mark.parametrize("name", ["nsf3-d128-g2", "nsf3-d86-g2"])
def test_the_two_spline_sweeps_agree_on_the_same_rows(name):
    """The lone-wave spline sweep (AUTO) and the workgroup spline sweep on the same rows, at the two width classes where both
    run: D = 128 (33 hidden tiles, every output product unsplit) and D = 86 (43 tiles, 27 of them with their products dealt
    by K range and added by wavefront 0).  Each meets the criterion on the fixture's inverse rows; their distance from each
    other, by the criterion's own row measure, is recorded -- a measurement with no bound of its own."""
    spec, flat, _ = fixture(name)
    f = flow(spec, flat)
    u, R, f32 = wide_reference(name, "inverse")
    assert plan_of(f, len(u), AUTO).sweep == S_NSF_SOLO and plan_of(f, len(u), WG_NSF).sweep == S_WG_NSF and spec.nT >= 17
    assert (fr.k_split_tiles(spec) > 0) == (name == "nsf3-d86-g2")
    got = {}
    for algo in (AUTO, WG_NSF):
        f.inverse_algo = algo
        got[algo] = [t.numpy() for t in f.inverse(torch.from_numpy(u))]
        for q, v in zip(("x", "ladj"), got[algo]):
            check(R, q, v, f"two sweeps algorithm {algo}, {name}", [d[q] for d in f32])
    f.inverse_algo = AUTO
    dx = fr.row_err(got[WG_NSF][0], got[AUTO][0])[R.ok].max()
    dl = fr.row_err(got[WG_NSF][1], got[AUTO][1], R.cancel["ladj"])[R.ok].max()
    print(f"workgroup spline sweep vs lone-wave sweep, {name}: x {dx:.2e} ladj {dl:.2e} (row_err, {int(R.ok.sum())} rows)")
    for key, v in ((f"workgroup vs lone-wave spline sweep x ({name})", dx), (f"workgroup vs lone-wave spline sweep ladj ({name})", dl)):
        parity.MEASURED[key] = max(parity.MEASURED.get(key, 0.0), float(v))


@pytest.mark.xfail(strict=True, reason="open finding: see OPEN_FINDINGS")
@pytest.mark.parametrize("name,algo", sorted(OPEN_FINDINGS, key=lambda p: (p[0], str(p[1]).zfill(2))))
def test_open_finding_the_criterion_on_the_listed_inverses(name, algo):
    """The listed (flow, inverse algorithm) pairs -- and (flow, "forward <quantity>") -- fail the criterion today; strict:
    the test fails once they meet it, so that the list stays true."""
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
    algos = algorithms(f, len(x))
    assert WG_NSF in algos
    for algo in ([] if name in FORWARD_ONLY else algos):
        f.inverse_algo = algo
        xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(x)))
        np.testing.assert_array_equal(xi[out], x[out], err_msg=f"algorithm {algo}")
        np.testing.assert_array_equal(li[allout], 0.0, err_msg=f"algorithm {algo}")


@pytest.mark.parametrize("name", ["maf3-d10-fit", "maf3-d32-fit", "nsf6-d10-fit", "nsf3-d32-fit", "maf6-d50-fit", "maf3-d10-g16",
                                  "maf3-d102-g2", "nsf3-d102-g2", "maf6-d102-fit"])
@pytest.mark.parametrize("n", [64, 4096])
def test_non_finite_rows_stay_in_their_rows(name, n):
    """NaN / +inf / -inf in one coordinate of rows 0, 15, 16, 17 and n-1: every other row is bit-identical to the same batch
    with those rows finite, for the forward, log_prob, AUTO and every inverse (same n: AUTO picks its sweep by n).  At
    D = 102 the D-pass inverses (AUTO, NAIVE: 103 passes of a 51-tile network, the 300 ms class at 4096 rows) run at n = 64
    only; the forward and the workgroup sweep run at both."""
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    algos = algorithms(f, n)
    if spec.n_dim >= 102 and n > 64:
        algos = [a for a in algos if plan_of(f, n, a).sweep not in DPASS_SWEEPS]
        assert algos == [WG_NSF if spec.univariate == "rqs" else WG]
    assert (WG_NSF if spec.univariate == "rqs" else WG) in algos
    good = data[np.random.default_rng(n).choice(len(data), n, replace=n > len(data))]
    f.inverse_algo = 0
    lat = f.forward(torch.from_numpy(good))[0].numpy()
    for what, base in (("forward", good), ("inverse", lat)):
        bad, rows = fr.with_nonfinite(base)
        keep = np.setdiff1d(np.arange(n), rows)
        runs = [("forward", None), ("log_prob", None)] if what == "forward" else [("inverse", a) for a in algos]
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
    _trainer_case(name, n, weighted)


@pytest.mark.parametrize("name", ["maf3-d102-g2", "nsf3-d102-g2", "maf6-d102-fit", "nsf3-d102-fit", "maf3-d102-g16", "nsf3-d102-g4"])
@pytest.mark.parametrize("n", [5, 100])
@pytest.mark.parametrize("weighted", [False, True])
def test_trainer_loss_and_gradient_per_block_at_default_width(name, n, weighted):
    """The same test with the same envelope rule on the default-width flows at D = 102 (51 hidden tiles: the wide
    training instances), scaled up and trained.  The gain-16 / gain-4 flows are held on the loss only.  The rows are
    drawn off the ReLU kinks: with 3 x 512 x T pre-activations a row, one of 5 rows of ``nsf3-d102-g2`` has a layer-1
    pre-activation of -1.5e-7 (float64) that the float32 numpy oracle computes as +4.1e-7 -- the kernel and the twin took
    different sides, and that unit's bias gradient differed by 2.4e-3 of its block while every other unit agreed to 4e-6."""
    _trainer_case(name, n, weighted, gradient=name not in FORWARD_ONLY, off_kinks=True)


def _trainer_case(name, n, weighted, gradient=True, off_kinks=False):
    spec, flat, data = fixture(name)
    f = flow(spec, flat)
    rng = np.random.default_rng(n + 31 * weighted)
    x = np.ascontiguousarray(data[rng.choice(len(data), 2 * n + 8 if off_kinks else n, replace=False)], np.float32)
    if off_kinks:
        # like the knots below: the rows of the gradient stay off the ReLU kinks (fr.relu_margin), where the loss is not
        # differentiable in the parameters and the twin's error is no envelope of another float32 evaluation's
        keep = fr.relu_margin(spec, flat, x) > fr.RELU_MARGIN
        assert keep.sum() >= n, (name, n, int(keep.sum()))
        print(f"trainer, {name} n={n} w={int(weighted)}: {int((~keep[: np.flatnonzero(keep)[n - 1] + 1]).sum())} drawn rows on a ReLU kink replaced")
        x = np.ascontiguousarray(x[keep][:n])
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    batches = [(x, gradient)]
    if spec.univariate == "rqs":
        batches.append((np.ascontiguousarray(np.concatenate([fr.knot_rows(spec, flat, x)[0][: max(n // 4, 1)], x])[:n]), False))
    for i, (xb, grad) in enumerate(batches):
        _loss_and_gradient(spec, flat, f, xb, w, grad, f"trainer, {name} n={n} w={int(weighted)}{' knots' if i else ''}")


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
    # default width at D = 102, the flow inverting with its family's workgroup sweep (inverse algorithm 10 / 11; the step
    # launches proposal, sweep and scaler one by one whatever PMC_NO_FUSE says): a case of 64 walkers that is in no table
    "workgroup (maf6, D=102)": ("maf6-d102-fit", dict(kind="preconditioned_pcn", N=64, D=102, T=6, beta=0.5, nu=5.0, prior="uniform",
                                                      target="bimodal", seed=23, n_max=2), WG),
    "workgroup spline (nsf3, D=102)": ("nsf3-d102-fit", dict(kind="preconditioned_pcn", N=64, D=102, T=3, beta=1.0, nu=5.0, prior="normal",
                                                             target="gauss", seed=24, n_max=2, flow="rqs"), WG_NSF),
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
    fx, name, *algo = STEP_FAMILIES[family]
    spec, flat, _ = fixture(fx)
    monkeypatch.setattr(cases, "flow_params", lambda s, seed, gain=1.2: flat)
    c = name if isinstance(name, dict) else cases.find_case(name)
    name = family if isinstance(name, dict) else name                # (a case of its own: the name is a label)
    N, D = c["N"], c["D"]
    state, funcs, opts, aux = cases.build_case(name, Reparameterize, case=c)
    assert (aux["spec"].n_dim, aux["spec"].n_transforms, aux["spec"].univariate) == (spec.n_dim, spec.n_transforms, spec.univariate)
    f = flow(spec, flat)
    if algo:
        # the engine's sweep: the workgroup sweep of the flow's family, and no fused proposal + inverse instance
        f.inverse_algo = algo[0]
        plain, fused = plan_of(f, N, algo[0]), plan_of(f, N, algo[0], fused=1)
        assert plain.sweep == {WG: S_WG, WG_NSF: S_WG_NSF}[algo[0]] and plain.fused == 0
        assert fused is not None and fused.sweep == 0 and fused.fused == 0
    ostate, ofuncs, oopts, _ = cases.build_case(name, OracleScaler, case=c)
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
    R = fr.Reference(spec, flat, state["u"][sub].astype(np.float32), "forward", k=fr.n_perturb(spec))
    # (the float32 evaluations: the numpy oracle; the new families' spline flow: and the kernels' spline formulas, as in
    #  the criterion test -- on these 16 rows the forward kernel's median err/e is 4.0, the formulas' 3.6, numpy's 2.9)
    model = fr.KernelSplineOracle(spec, flat) if algo and spec.univariate == "rqs" else None
    extra = [] if model is None else [model.forward(state["u"][sub].astype(np.float32))[0]]
    check(R, "z", eng.theta32.cpu().numpy()[sub], f"step theta = forward(u), {family}", [th0[sub]] + extra)
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
    R = fr.Reference(spec, flat, t32, "inverse", k=fr.n_perturb(spec))
    ev = omaf.inverse(t32)
    evk = ([], []) if model is None else tuple([v] for v in model.inverse(t32))
    check(R, "x", p_u[sub], f"step u' = inverse(theta'), {family}", [ev[0]] + evk[0])
    check(R, "ladj", p_ldjf[sub], f"step u' = inverse(theta'), {family}", [ev[1]] + evk[1])
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
