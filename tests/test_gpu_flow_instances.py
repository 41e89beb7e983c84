"""Every instance of the float32 flow kernels that no other test launches (``tests/flow_instances.py`` has the table, the
CPU census in ``tests/test_flow_instances_cpu.py`` shows that nothing is left out):

(a) the four-wave forward kernel (calls of more than 16384 rows), all eight instances, against the eight-wave one on the
    same rows and against the oracle;
(b) the lean instances at 4 and 16 bins, with eight- and sixteen-wave trainers, and at one transform, forced on small
    flows where the full instances give the same bits;
(c) the lean trainer over several row-set chunks and through a row index;
(d) default-width 4- and 16-bin flows at the ends of the ranges where every kernel is lean, against the oracle and
    autograd -- and the widths a 16-bin flow is refused at;
(e) the lean D-pass fallback (D = 102) on rows outside the spline box and on non-finite rows.

Every bound is the one an existing test holds the same quantity to (``tests/test_gpu_flow.py``, ``tests/test_gpu_train.py``,
``tests/test_gpu_wide_default_flows.py``); the measured errors are printed before they are asserted."""
import functools

import numpy as np
import pytest
import torch

import cases
import flow_instances as fi
import flow_regimes as fr
from oracle.maf import OracleMAF, torch_loss
from parity import close_rel, TOL
from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu

NSF_FWD, NSF_INV, NSF_LADJ = 2e-5, 5e-5, 1e-4        # tests/test_gpu_flow.py


def ident(s):
    return "-".join(str(v) for v in s)


def takes(f, spec_arg, n, lean, **want):
    """The plan names what the case table says this call launches (asserted before anything is compared)."""
    got = fi.instances(f.lib, spec_arg, n, lean)
    assert {k: got[k] for k in want} == want, (spec_arg, n, lean, got)
    rows = [c for c in fi.CASES if c.spec == spec_arg and c.n == n and c.lean == lean and c.group != "suite"]
    assert rows and all(got[k] == v for c in rows for k, v in c.reaches.items()), (spec_arg, n, lean, got)


@functools.lru_cache(maxsize=None)
def flow_of(spec_arg, seed=3):
    """One flow per shape for the whole module: (Flow, spec, parameters, float32 oracle)."""
    from pocomc_amd import Flow
    spec = fi.make_spec(spec_arg)
    flat = cases.flow_params(spec, seed, gain=1.0)
    f = Flow(spec.n_dim, spec)
    f.set_params(flat)
    return f, spec, flat, OracleMAF(spec, flat)


def tolerances(spec):
    return (TOL, TOL, TOL) if spec.univariate == "affine" else (NSF_FWD, NSF_INV, NSF_LADJ)


# ------------------------------------------------------------------------------------------ (a) four waves against eight
@functools.lru_cache(maxsize=None)
def big_reference(spec_arg):
    """BIG rows of N(0, 2.5^2) -- inside and outside the spline box -- and the oracle's forward on them, computed once."""
    f, spec, flat, o = flow_of(spec_arg)
    x = (np.random.default_rng(fi.BIG).normal(size=(fi.BIG, spec.n_dim)) * 2.5).astype(np.float32)
    zo, lo = o.forward(x)
    terms = o.ladj_abs_terms(x)
    base = 0.5 * (zo.astype(np.float64) ** 2).sum(axis=1) + 0.5 * spec.n_dim * np.log(2 * np.pi)
    return x, zo, lo, o.log_prob(x), terms, base


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("spec_arg", fi.A_FLOWS, ids=ident)
def test_four_waves_give_what_eight_give(spec_arg, lean):
    """One call of 16391 rows takes ``maf_forward_wg_kernel<4, ...>``; the same rows as 16384 + 7 take the eight-wave
    instance (16384 is the last size that does).  A tile is one wavefront's work either way, so z is the same bits; the
    log-determinant is summed over the wavefronts in another order, so it and log_prob are held to the oracle, in both
    runs.  The big call's first row and its last (row 6 of a row set of 7) are also compared on their own.
    Measured on MI355X over the 16391 rows, the same figures from four and from eight wavefronts (the float32 oracle's own
    distance to the float64 evaluation of these rows in brackets), z / log-determinant / log_prob: maf3 8.4e-7 / 2.1e-7 /
    1.4e-6 (9.8e-7 / 1.7e-7 / 1.1e-6) against 1e-5; nsf3 9.3e-6 / 1.3e-5 / 1.7e-6 (5.2e-6 / 9.5e-6 / 1.5e-6), 4 bins
    2.5e-6 / 4.6e-6 / 7.7e-7 (1.7e-6 / 2.8e-6 / 6.1e-7), 16 bins 4.1e-6 / 2.4e-5 / 3.6e-6 (5.2e-6 / 2.6e-5 / 4.0e-6) against
    2e-5 / 1e-4 / 1e-4."""
    f, spec, flat, o = flow_of(spec_arg)
    x, zo, lo, lpo, terms, base = big_reference(spec_arg)
    u = fi.uni_of(spec)
    kind = fi.LEAN if lean else fi.FULL
    takes(f, spec_arg, fi.BIG, lean, forward=(4, u, kind))
    takes(f, spec_arg, fi.NW_ROWS, lean, forward=(8, u, kind))
    xt = torch.from_numpy(x)
    f.lean_lds = lean
    try:
        assert f.lds_plan()["forward"][0] == kind
        z4, l4 = (t.numpy() for t in f.forward(xt))
        lp4 = f.log_prob(xt).numpy()
        parts = [xt[:fi.NW_ROWS], xt[fi.NW_ROWS:]]
        assert [len(p) for p in parts] == [16384, 7]
        z8, l8 = (np.concatenate(v) for v in zip(*[[t.numpy() for t in f.forward(p)] for p in parts]))
        lp8 = np.concatenate([f.log_prob(p).numpy() for p in parts])
    finally:
        f.lean_lds = False
    assert np.array_equal(z4, z8), f"{int((z4 != z8).any(axis=1).sum())} rows of z differ between four and eight wavefronts"
    tz, _, tl = tolerances(spec)
    for nw, z, l, lp in ((4, z4, l4, lp4), (8, z8, l8, lp8)):
        print(f"{nw} waves {ident(spec_arg)} {kind}: z {close_rel(z, zo, np.inf, 'z (measured)'):.2e} "
              f"ladj {close_rel(l, lo, np.inf, 'ladj (measured)', cancel=terms):.2e} "
              f"log_prob {close_rel(lp, lpo, np.inf, 'log_prob (measured)', cancel=terms + base):.2e}")
    for nw, z, l, lp in ((4, z4, l4, lp4), (8, z8, l8, lp8)):
        close_rel(z, zo, tz, f"z, {nw} waves")
        close_rel(l, lo, tl, f"ladj, {nw} waves", cancel=terms)
        close_rel(lp, lpo, tl, f"log_prob, {nw} waves", cancel=terms + base)
    for r in (0, fi.BIG - 1):
        s = slice(r, r + 1)
        close_rel(z4[s], zo[s], tz, f"z, four waves, row {r}")
        close_rel(l4[s], lo[s], tl, f"ladj, four waves, row {r}", cancel=terms[s])
        close_rel(lp4[s], lpo[s], tl, f"log_prob, four waves, row {r}", cancel=(terms + base)[s])
    assert np.isfinite(z4).all() and np.isfinite(l4).all() and np.isfinite(lp4).all()


# ------------------------------------------------------------------------------------------ (b) lean == full, bit for bit
@pytest.mark.parametrize("spec_arg", fi.B_FLOWS, ids=ident)
def test_forced_lean_equals_full_bit_for_bit(spec_arg):
    """``tests/test_gpu_wide_default_flows.py::test_forced_lean_instances_equal_the_full_ones_bit_for_bit`` on the flows it
    leaves out: 4 and 16 bins with the eight-wave trainer (hidden width 64) and the sixteen-wave one (128), and flows of
    ONE transform -- the last transform's activations are the only ones a full trainer never reloads and the first a lean
    one does.  z, log-determinant, log_prob, the D-pass inverse, loss and gradient (unweighted, weighted): the same bits.
    The affine flow's D-pass has no full instance of the workgroup kernel (theirs is the lone-wave kernel, another order
    of additions): oracle tolerance there, as in that test."""
    from pocomc_amd.train import loss_and_grad, _train_state
    f, spec, flat, o = flow_of(spec_arg, seed=7)
    D, u = spec.n_dim, fi.uni_of(spec)
    for lean in (False, True):
        row = [c for c in fi.CASES if c.group == "b" and c.spec == spec_arg and c.lean == lean][0]
        takes(f, spec_arg, 40, lean, **row.reaches)
    assert {v[0] for v in f.lds_plan().values()} == {"full"}
    _train_state(f).repack(f)
    rng = np.random.default_rng(D + u)
    names = ("z", "ladj", "log_prob", "x (D-pass)", "ladj (D-pass)", "loss", "gradient", "weighted loss", "weighted gradient")
    for n in (1, 17, 40):
        x = torch.from_numpy((rng.normal(size=(n, D)) * 2.0).astype(np.float32))
        w = torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32))
        out = {}
        try:
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
        finally:
            f.lean_lds, f.inverse_algo = False, 0
        for what, a, b in zip(names, out[False], out[True]):
            if u == 0 and "D-pass" in what:
                close_rel(b, a, TOL, f"lean D-pass vs lone-wave D-pass, {what}",
                          cancel=None if what.startswith("x") else o.ladj_abs_terms(out[False][3]))
            else:
                assert np.array_equal(np.asarray(a), np.asarray(b)), (what, n)
        assert np.abs(out[True][6]).max() > 0 and np.isfinite(out[True][5]) and np.isfinite(out[True][6]).all()
        assert np.isfinite(out[True][0]).all() and np.isfinite(out[True][3]).all()
    # ... and the full side is right: forward and gradient of the last batch against the oracle and autograd
    tz, _, tl = tolerances(spec)
    zo, lo = o.forward(x.numpy())
    close_rel(out[False][0], zo, tz, "z, small flow")
    close_rel(out[False][1], lo, tl, "ladj, small flow", cancel=o.ladj_abs_terms(x.numpy()))
    ft = torch.tensor(flat, requires_grad=True)
    torch_loss(spec, ft, x, w).backward()
    g_ref = ft.grad.numpy()
    rtol, atol = (2e-3, 1e-4) if u else (1e-3, 5e-5)                 # tests/test_gpu_train.py
    np.testing.assert_allclose(out[False][8], g_ref, rtol=rtol, atol=atol * np.abs(g_ref).max())


# ------------------------------------------------------------------------------------------ (c) chunks and a row index
@pytest.mark.parametrize("spec_arg", fi.C_FLOWS, ids=ident)
def test_lean_trainer_in_chunks_and_through_an_index(spec_arg):
    """The shape of ``tests/test_gpu_train.py::test_large_batch_loops_over_row_sets``: 131 row sets through a scratch of 40,
    so the batch comes in four chunks (``set0`` = 0, 40, 80, 120) and the lean instance indexes its activation scratch per
    chunk.  Weighted.  Lean loss and gradient are the full ones' bits; the lean batch through a row-index list into a
    shuffled copy of the data is the contiguous lean batch's bits."""
    from pocomc_amd import Flow
    from pocomc_amd.train import loss_and_grad, _train_state
    spec = fi.make_spec(spec_arg)
    flat = cases.flow_params(spec, 1)
    f = Flow(spec.n_dim, spec)                               # (a flow of its own: the scratch cap is set before its first batch)
    f.set_params(flat)
    takes(f, spec_arg, fi.C_ROWS, True, **[c for c in fi.CASES if c.group == "c" and c.spec == spec_arg][0].reaches)
    ts = _train_state(f)
    ts.set_cap = 40
    assert ts.n_sets == 0
    n = fi.C_ROWS
    rng = np.random.default_rng(5)
    xd = torch.from_numpy((rng.normal(size=(n, spec.n_dim)) * (1.2 if spec.univariate == "affine" else 2.5)).astype(np.float32)).cuda()
    wd = torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32)).cuda()
    ts.repack(f)
    res = {}
    try:
        for lean in (False, True):
            f.lean_lds = lean
            assert f.lds_plan()["train"][0] == ("lean" if lean else "full")
            res[lean] = (float(loss_and_grad(f, xd, wd)), f._train.grad.cpu().numpy().copy())
        assert f._train.desc.max_sets == 40 and (n + 15) // 16 == 131
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n)
        loss_i = float(loss_and_grad(f, xd[perm.cuda()].contiguous(), wd[perm.cuda()].contiguous(), idx=inv.cuda()))
        grad_i = f._train.grad.cpu().numpy().copy()
    finally:
        f.lean_lds = False
    assert res[True][0] == res[False][0] and np.isfinite(res[True][0])
    assert np.array_equal(res[True][1], res[False][1]) and np.abs(res[True][1]).max() > 0
    assert loss_i == res[True][0]
    assert np.array_equal(grad_i, res[True][1])
    # the full side against autograd, with the bounds of the test this shape comes from (spline: tests/test_gpu_train.py's)
    ft = torch.tensor(flat, requires_grad=True)
    lo = torch_loss(spec, ft, xd.cpu(), wd.cpu())
    lo.backward()
    g_ref = ft.grad.numpy()
    rtol, atol = (5e-4, 5e-5) if spec.univariate == "affine" else (2e-3, 1e-4)
    np.testing.assert_allclose(res[False][0], float(lo.detach()), rtol=5e-5)
    np.testing.assert_allclose(res[False][1], g_ref, rtol=rtol, atol=atol * np.abs(g_ref).max())


# ------------------------------------------------------------------------------------------ (d) wide 4- and 16-bin flows
def auto_sweep(f, n):
    import ctypes as C
    from pocomc_amd import _lib
    p = _lib.pmc_inverse_plan_t()
    _lib.check(f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, 0, 0, C.byref(p)))
    return p.sweep


def wide_plan_is_lean(f, spec_arg, n):
    """What ``lds_plan()`` and the inverse plan name, on the live flow's own descriptor."""
    assert f.spec.hidden == 512
    assert {k: v[0] for k, v in f.lds_plan().items()} == {"forward": "lean", "dpass": "lean", "train": "lean"}
    assert auto_sweep(f, n) == 8                                           # PMC_SWEEP_DPASS_LEAN
    u = spec_arg[4]
    got = fi.instances(f.lib, spec_arg, n)
    assert got == {"forward": (8, u, fi.LEAN), "dpass": (u, fi.LEAN), "auto": "dpass_lean", "train": (16, u, fi.LEAN, False)}


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("spec_arg", fi.D_FLOWS, ids=ident)
def test_wide_forward_and_log_prob_match_the_oracle(spec_arg, n):
    """``tests/test_gpu_wide_default_flows.py::test_forward_and_log_prob_match_the_oracle`` at 4 bins (D = 92, 112: both ends
    of the widths where all three kernels are lean) and 16 bins (86, 95: the first width and the last before the refusals;
    112: the first after).  Measured maxima over these cases: z 1.5e-6 (bound 2e-5), log-determinant 2.0e-6 and log_prob
    3.2e-7 (1e-4); the inverse below: x 1.6e-6 (5e-5), log-determinant 1.5e-6 (1e-4); the gradient's excess over
    rtol |g_ref| at most 4.0e-6 max|g_ref| (1e-4), the loss within 2.5e-7 (5e-5)."""
    f, spec, flat, o = flow_of(spec_arg)
    wide_plan_is_lean(f, spec_arg, n)
    D = spec.n_dim
    x = (np.random.default_rng(n + D).normal(size=(n, D)) * 2.5).astype(np.float32)
    z, ladj = f.forward(torch.from_numpy(x))
    zo, lo = o.forward(x)
    terms = o.ladj_abs_terms(x)
    base = 0.5 * (zo.astype(np.float64) ** 2).sum(axis=1) + 0.5 * D * np.log(2 * np.pi)
    lp = f.log_prob(torch.from_numpy(x)).numpy()
    print(f"wide forward {ident(spec_arg)} n={n}: z {close_rel(z.numpy(), zo, np.inf, 'wide z (measured)'):.2e} "
          f"ladj {close_rel(ladj.numpy(), lo, np.inf, 'wide ladj (measured)', cancel=terms):.2e} "
          f"log_prob {close_rel(lp, o.log_prob(x), np.inf, 'wide log_prob (measured)', cancel=terms + base):.2e}")
    close_rel(z.numpy(), zo, NSF_FWD, "wide z")
    close_rel(ladj.numpy(), lo, NSF_LADJ, "wide ladj", cancel=terms)
    close_rel(lp, o.log_prob(x), NSF_LADJ, "wide log_prob", cancel=terms + base)


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("spec_arg", fi.D_FLOWS, ids=ident)
def test_wide_auto_inverse_matches_the_oracles_dpass(spec_arg, n):
    """The only inverse these flows have: AUTO falls back to the lean D-pass kernel, D + 1 passes per transform."""
    f, spec, flat, o = flow_of(spec_arg)
    wide_plan_is_lean(f, spec_arg, n)
    D = spec.n_dim
    z = (np.random.default_rng(7 + n + D).normal(size=(n, D)) * 1.5).astype(np.float32)
    xo, lo = o.inverse(z)                                    # the reference's D-pass algorithm
    terms = o.ladj_abs_terms(xo)
    x, l = f.inverse(torch.from_numpy(z))
    print(f"wide inverse {ident(spec_arg)} n={n}: x {close_rel(x.numpy(), xo, np.inf, 'wide x (measured)'):.2e} "
          f"ladj {close_rel(l.numpy(), lo, np.inf, 'wide ladj inverse (measured)', cancel=terms):.2e}")
    close_rel(x.numpy(), xo, NSF_INV, "wide x, AUTO")
    close_rel(l.numpy(), lo, NSF_LADJ, "wide ladj inverse, AUTO", cancel=terms)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("n", [5, 40])
@pytest.mark.parametrize("spec_arg", fi.D_FLOWS, ids=ident)
def test_wide_loss_and_gradient_match_autograd(spec_arg, n, weighted):
    """The sixteen-wave lean trainer at 4 and 16 bins against float32 autograd on the oracle twin, with the spline bounds of
    ``tests/test_gpu_train.py``: gradient rtol 2e-3 with atol 1e-4 max|g_ref|, loss rtol 5e-5.  No masked weight receives
    gradient."""
    from pocomc_amd.train import loss_and_grad, _train_state
    f, spec, flat, _ = flow_of(spec_arg)
    wide_plan_is_lean(f, spec_arg, n)
    D = spec.n_dim
    rng = np.random.default_rng(n + D)
    x = (rng.normal(size=(n, D)) * 2.5).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    ft = torch.tensor(flat, requires_grad=True)
    lo = torch_loss(spec, ft, torch.from_numpy(x), None if w is None else torch.from_numpy(w))
    lo.backward()
    g_ref = ft.grad.numpy()
    _train_state(f).repack(f)
    loss = loss_and_grad(f, torch.from_numpy(x).cuda(), None if w is None else torch.from_numpy(w).cuda())
    g = f._train.grad.cpu().numpy()
    scale = np.abs(g_ref).max()
    rtol, atol = 2e-3, 1e-4 * scale
    excess = (np.abs(g - g_ref) - rtol * np.abs(g_ref)).max() / scale
    print(f"wide gradient {ident(spec_arg)} n={n} weighted={weighted}: loss rel {abs(float(loss) - float(lo.detach())) / abs(float(lo.detach())):.2e}, "
          f"max (|g - g_ref| - rtol |g_ref|) / max|g_ref| {excess:.2e} (allowed {atol / scale:.0e})")
    np.testing.assert_allclose(float(loss), float(lo.detach()), rtol=5e-5)
    np.testing.assert_allclose(g, g_ref, rtol=rtol, atol=atol)
    assert not g[spec.mask_flat() == 0].any()                # masked weights never receive gradient
    assert np.abs(g).max() > 0


@pytest.mark.parametrize("spec_arg", fi.D_REFUSED, ids=ident)
def test_refused_widths_raise_the_launchers_errors(spec_arg):
    """16 bins at D = 100 and 104: no instance of any of the three kernels fits.  ``forward``, ``log_prob``, ``inverse`` and
    ``loss_and_grad`` raise the launcher's message; nothing is launched -- the gradient and the loss word stay as they were."""
    from pocomc_amd import Flow, _lib
    from pocomc_amd.train import loss_and_grad, _train_state
    spec = fi.make_spec(spec_arg)
    f = Flow(spec.n_dim, spec, seed=1)
    got = fi.instances(f.lib, spec_arg, 33)
    assert got == {"forward": fi.REFUSED_FORWARD, "dpass": fi.REFUSED_FORWARD, "auto": fi.REFUSED_FORWARD, "train": fi.REFUSED_TRAIN}
    with pytest.raises(_lib.PocomcAmdError, match="too wide for 160 KB of LDS"):
        f.lds_plan()
    x = torch.randn(33, spec.n_dim, generator=torch.Generator().manual_seed(1))
    for call in (f.forward, f.log_prob, f.inverse):
        with pytest.raises(_lib.PocomcAmdError, match="pmc_maf_forward: flow too wide for 160 KB of LDS"):
            call(x)
    ts = _train_state(f)
    ts.repack(f)
    ts.grad.fill_(7.0)
    with pytest.raises(_lib.PocomcAmdError, match="pmc_maf_loss_grad: flow too wide for the 160 KB LDS of one workgroup"):
        loss_and_grad(f, x.cuda())
    torch.cuda.synchronize()
    assert bool((ts.grad == 7.0).all()) and float(ts.scal[0]) == 0.0


# ------------------------------------------------------------------------------------------ (e) the fallback at the edge rows
def test_outside_coordinates_come_back_bit_for_bit_at_102_dimensions():
    """``tests/test_gpu_flow_regimes.py::test_coordinates_outside_the_spline_box_come_back_bit_for_bit`` through the lean
    forward kernel and AUTO's lean D-pass inverse (D = 102, 8 bins, n = 33): a coordinate well outside the box passes
    every transform unchanged, and a row outside in every coordinate has a log-determinant of exactly zero."""
    spec_arg = fi.E_FLOWS[1]
    f, spec, flat, o = flow_of(spec_arg)
    takes(f, spec_arg, 33, False, forward=(8, 8, fi.LEAN), auto="dpass_lean")
    base = (np.random.default_rng(102).normal(size=(33, 102)) * 2.5).astype(np.float32)
    x, out = fr.outside_rows(spec, base)
    allout = out.all(axis=1)
    assert allout.sum() >= 4 and not out.all() and (~out).any(axis=1).sum() >= 16
    z, l = (t.numpy() for t in f.forward(torch.from_numpy(x)))
    np.testing.assert_array_equal(z[out], x[out])
    np.testing.assert_array_equal(l[allout], 0.0)
    xi, li = (t.numpy() for t in f.inverse(torch.from_numpy(x)))
    np.testing.assert_array_equal(xi[out], x[out])
    np.testing.assert_array_equal(li[allout], 0.0)


@pytest.mark.parametrize("spec_arg", fi.E_FLOWS, ids=ident)
def test_non_finite_rows_stay_in_their_rows_at_102_dimensions(spec_arg):
    """``tests/test_gpu_flow_regimes.py::test_non_finite_rows_stay_in_their_rows`` on the lean forward kernel and the lean
    D-pass fallback: NaN / +inf / -inf in one coordinate of rows 0, 15, 16, 17 and 32 of 33 leave every other row of the
    same call bit-identical -- forward, log_prob and AUTO's inverse."""
    f, spec, flat, o = flow_of(spec_arg)
    u = fi.uni_of(spec)
    takes(f, spec_arg, 33, False, forward=(8, u, fi.LEAN), auto="dpass_lean")
    n = 33
    good = (np.random.default_rng(n).normal(size=(n, 102)) * (2.5 if u else 1.5)).astype(np.float32)
    lat = f.forward(torch.from_numpy(good))[0].numpy()
    assert np.isfinite(lat).all()
    for what, base in (("forward", good), ("inverse", lat)):
        bad, rows = fr.with_nonfinite(base)
        assert rows == [0, 15, 16, 17, 32]
        keep = np.setdiff1d(np.arange(n), rows)
        for kind in (("forward", "log_prob") if what == "forward" else ("inverse",)):
            res = []
            for inp in (base, bad):
                t = torch.from_numpy(np.ascontiguousarray(inp))
                res.append([f.log_prob(t).numpy()] if kind == "log_prob" else [v.numpy() for v in getattr(f, kind)(t)])
            for a, b in zip(*res):
                assert np.isfinite(a[keep]).all(), kind
                np.testing.assert_array_equal(b[keep], a[keep], err_msg=f"{ident(spec_arg)} {kind}")
