"""The bf16 matrix-core kernels (``csrc/maf_forward_bf16.hip``, ``csrc/maf_train_bf16.hip``) against the float64 evaluation
of a model that rounds where they round (``tests/bf16_model.py``), with the float32 evaluation of the same model as the
yardstick -- measured in the same test on the same rows, never a constant.  ``tests/test_bf16_model_cpu.py`` shows that
this criterion rejects each of six single defects that the plain-oracle bounds (3e-2; 2e-2 / 1e-1) let pass.

Forward, per quantity (z, ladj, log_prob) and row: ``b = max(8 x p75 of the float32 model's errors, 2^-20)``; the kernel's
75th percentile is at most ``b``, at most 25 % of its rows lie beyond ``b`` (flipped rows: a value within float32 noise
of a bf16 rounding boundary rounded the other way), at most 10 % of the float32 model's own rows do, and every row is
finite and within the suite's 3e-2 of the plain oracle -- except the seven (case, quantity) pairs of PLAIN_OPEN, where
the model itself is beyond the 3e-2 and the bound is asserted FAILING (an open finding about the bound), and the twin's
log_prob, decided from the model (PLAIN_BY_MODEL).  Outputs requested alone are bit-equal to the same outputs
requested together; a row's outputs do not depend on its position in the batch, on the ``idx`` gather or on the launch
shape (z bit for bit; the log-determinant bit for bit where the wave count is the same -- its per-wave partial sums are
grouped by wave -- and by the criterion above otherwise).

Trainer: relative error of the loss, relative L2 error of the gradient overall and of every canonical tensor, each at
most ``4 x`` the largest of four float32 model evaluations that differ in contraction order (floors 2^-20 / 1e-6);
masked entries exactly zero.

MEASURED on MI355X, 2026-10-18 (docs/LAB_NOTEBOOK.md has the same table).  Forward, flows at the default initialisation,
rows N(0, 1.2^2): 75th percentile of the per-row error against the float64 model, kernel / float32 model, and the share
of rows beyond the bound (kernel, float32 model):

    shape (D, T, H)   n      z                 ladj              log_prob          beyond b
    (2, 2, 32)        33     9.0e-8 / 1.1e-7   3.7e-8 / 2.9e-8   7.8e-8 / 1.1e-7   0 %, 0 %
    (2, 2, 32)        16389  8.1e-8 / 1.0e-7   3.2e-8 / 3.1e-8   7.7e-8 / 9.3e-8   0.2 %, 0.1 %   (worst row 9.4e-4 / 3.5e-4; eight waves, two row sets)
    (7, 2, 32)        33     7.6e-8 / 1.0e-7   3.0e-8 / 3.3e-8   6.7e-8 / 7.9e-8   0 %, 0 %
    (7, 2, 32)        4113   7.5e-8 / 1.1e-7   2.9e-8 / 2.8e-8   6.2e-8 / 7.2e-8   1 row, none    (that row 2.7e-5)
    (33, 2, 128)      33     7.5e-8 / 1.4e-7   1.6e-8 / 2.0e-8   4.6e-8 / 7.6e-8   0 %, 0 %
    (40, 2, 256)      33     9.8e-8 / 1.4e-7   1.6e-8 / 1.4e-8   4.0e-8 / 6.2e-8   3 %, 3 %       (4.8e-6 / 3.4e-5)
    (64, 3, 256)      33     1.0e-7 / 1.9e-7   9.7e-9 / 1.4e-8   4.8e-8 / 6.9e-8   0 %, 0 %
    (4, 2, 1024)      16389  8.4e-8 / 1.2e-7   7.0e-8 / 6.8e-8   6.6e-8 / 7.9e-8   3.4 %, 3.0 %   (1.3e-4 / 1.7e-4; the four-wave launch, 1541 rows modelled)
    (128, 8, 512)     33     1.7e-7 / 2.8e-7   6.7e-9 / 8.2e-9   4.7e-8 / 6.9e-8   9.1 %, 3.0 %   (1.5e-3 / 1.4e-3)
    maf3-d10-twin     384    1.6e-6 / 2.3e-6   4.7e-8 / 4.9e-8   1.6e-7 / 2.1e-7   0.3 %, 0.5 %   (1.9e-2 / 1.9e-2)
    maf3-d10-g4       384    1.9e-7 / 2.1e-7   1.9e-8 / 2.3e-8   1.7e-7 / 1.8e-7   0 %, 0 %
    maf3-d10-g16      384    4.9e-7 / 5.2e-7   2.1e-8 / 2.8e-8   9.7e-7 / 1.0e-6   0 %, 0 %

(the bounds ``b`` were 9.5e-7 .. 1.8e-5; the same outputs are 5e-4 .. 1.1e-2 from the plain oracle).  Every bit-for-bit
comparison held, the log-determinant and log_prob across row sets (n = 4113 and 16389 against 17 rows) included.  Trainer, kernel (largest of the four float32 orders):

    case (D, T, H, n, weighted)   loss                gradient L2         worst tensor             largest ratio
    (5, 3, 32, 1, no)             6.0e-9 (1.2e-7)     0 (0)               0 (0)                    0.03
    (5, 3, 32, 31, no)            3.1e-8 (2.7e-7)     2.3e-8 (2.7e-8)     5.6e-8 (5.6e-8)          0.22
    (5, 3, 32, 33, no)            3.5e-8 (3.5e-8)     7.2e-8 (7.6e-8)     t1.b0 9.8e-7 (9.8e-7)    1.00
    (16, 2, 64, 100, yes)         2.3e-8 (2.3e-8)     3.1e-8 (5.7e-8)     4.6e-8 (6.3e-8)          0.18
    (33, 2, 128, 513, yes)        9.6e-8 (9.6e-8)     6.2e-6 (2.8e-5)     t0.W2 1.5e-5 (4.0e-5)    0.40
    (50, 6, 256, 64, no)          3.1e-8 (3.1e-8)     3.0e-7 (2.0e-4)     3.6e-8 (5.2e-7)          0.13
    (128, 8, 512, 64, yes)        6.3e-6 (5.8e-6)     2.7e-3 (2.7e-3)     t0.b0 1.7e-3 (1.7e-3)    1.08
    maf3-d10-twin, 100, no        7.0e-8 (7.0e-8)     7.6e-5 (7.6e-5)     t1.b2 6.1e-5 (6.1e-5)    1.01
    maf3-d10-twin, 100, yes       7.8e-8 (1.5e-7)     1.7e-5 (1.7e-5)     t0.b3 1.5e-5 (1.5e-5)    1.00

(where a case shows the same figure on both sides, kernel and float32 model flipped the same value: that term dominates
both).  Open finding: PLAIN_OPEN below -- about the plain-oracle bound, not about a kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bf16_model as bm
import flow_regimes as fr
from oracle.maf import OracleMAF
from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 33)
# (D, T, hidden): extra row counts
FORWARD_SHAPES = {
    (2, 2, None): (16389,),        # tri_ok false, even tile count; 16389 rows: eight waves, two row sets, 513 workgroups
    (7, 2, None): (4113,),         # three hidden tiles: the odd half k-tile; n >= 4096: two row sets, the last workgroup's second set holds one row
    (33, 2, None): (),             # two input k-tiles, the second partly padding
    (40, 2, 256): (),              # 20 tiles: the sixteen-wave launch
    (64, 3, 256): (),              # 17 tiles, sixteen waves, eight output tiles
    (128, 8, 512): None,           # config 5's own flow: n = 33 only
}
# The four-wave launch is NOT among them: ``pmc_maf_forward_bf16`` picks four waves for n > 16384 but dispatches them only
# with one row set, and n >= 4096 takes two row sets unless their activations exceed 160 KB of LDS -- at H = 32 the 16389
# rows run eight waves with two row sets.  ``test_the_four_wave_launch`` reaches it with a flow of H = 1024.

# OPEN FINDING: where the suite's 3e-2 against the PLAIN float32 oracle cannot hold for a correct bf16 evaluation.  Listed
# per case and quantity with the distance of the rounding-exact model ITSELF (float64, on the CPU) from the plain oracle on
# the same rows; the kernel reproduces these figures and sits within float32 noise of the model on those rows.  The listed
# quantities are asserted failing (``test_open_finding_the_plain_oracle_bound``, strict, the figure in the reason); every
# other quantity of these cases, and every quantity of every other case, is asserted to hold the 3e-2.
#   * trained / saturated flows amplify the operand rounding like they amplify float32's (tests/flow_regimes.py), here
#     2^-9 instead of 2^-24;
#   * D = 2, 16389 rows: the error of z is relative to the row's own ``max_j |z_j|`` and 7 rows have their latent next to
#     the origin (the worst is z = (-0.0018, -0.035)).
# The twin is trained on the CPU and its parameters are not bit-reproducible across thread counts: its z was 1.3e-1 ..
# 3.4e-1 from the plain oracle on three machines (always beyond the bound), its log_prob 2.3e-2 .. 6.2e-2 -- that one is
# decided from the model on the parameters at hand (``test_the_plain_oracle_bound_on_the_twins_log_prob``).
PLAIN_OPEN = {
    "maf3-d10-twin": {"z": 1.3e-1},
    "maf3-d10-g4": {"z": 4.2e-2, "log_prob": 4.4e-2},
    "maf3-d10-g16": {"z": 3.3e-2, "ladj": 1.0e-1, "log_prob": 6.5e-2},
    "d2-n16389": {"z": 5.82e-2},
}
PLAIN_BY_MODEL = {"maf3-d10-twin": ("log_prob",)}


def plain_held(case):
    """The quantities of ``case`` that are asserted to hold the 3e-2 against the plain oracle."""
    return tuple(q for q in bm.FWD_QUANTITIES if q not in PLAIN_OPEN.get(case, {}) and q not in PLAIN_BY_MODEL.get(case, ()))


def default_params(spec, seed=3):
    return spec.init_params(seed).astype(np.float32)


def rows_for(D, n, seed=0, scale=1.2):
    return (np.random.default_rng(1000 * D + seed).normal(size=(n, D)) * scale).astype(np.float32)


def bf16_flow(spec, flat, engine=None):
    from pocomc_amd import Flow
    f = Flow(spec.n_dim, spec, precision="bf16", seed=0)
    if engine:
        f.train_engine = engine
    f.set_params(flat)
    return f


def forward_call(f, xd, n, want=("z", "ladj", "log_prob"), idx=None):
    """``pmc_maf_forward_bf16`` on the first ``n`` rows of the device tensor ``xd`` (or the rows ``idx`` of it) with exactly
    the outputs ``want``; the others are passed as null."""
    from pocomc_amd import _lib
    _, img, per_t = f._bf16_image()
    D = f.spec.n_dim
    out = {"z": torch.full((n, D), 7.0, dtype=torch.float32, device=xd.device) if "z" in want else None,
           "ladj": torch.full((n,), 7.0, dtype=torch.float32, device=xd.device) if "ladj" in want else None,
           "log_prob": torch.full((n,), 7.0, dtype=torch.float32, device=xd.device) if "log_prob" in want else None}
    with torch.cuda.device(xd.device):
        _lib.check(f.lib.pmc_maf_forward_bf16(C.byref(f._desc), _lib.ptr(img), per_t, _lib.ptr(xd), _lib.ptr(out["z"]),
                                              _lib.ptr(out["ladj"]), _lib.ptr(out["log_prob"]), n, _lib.ptr(idx),
                                              _lib.stream_handle()), "pmc_maf_forward_bf16")
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def plain_errors(spec, flat, x, got):
    """The three errors of ``tests/test_gpu_config.py`` against the plain float32 oracle, per row."""
    o = OracleMAF(spec, flat)
    with np.errstate(all="ignore"):
        zo, lo = o.forward(x)
        terms = o.ladj_abs_terms(x)
        lpo = o.log_prob(x)
        return {"z": np.abs(got["z"] - zo).max(axis=1) / np.abs(zo).max(axis=1),
                "ladj": np.abs(got["ladj"] - lo) / np.maximum(np.abs(lo), terms),
                "log_prob": np.abs(got["log_prob"] - lpo) / np.maximum(np.abs(lpo), terms + 0.5 * (zo.astype(np.float64) ** 2).sum(axis=1))}


def hold_forward(spec, flat, x, got, ref, f32, tag, plain=bm.FWD_QUANTITIES):
    """The forward criterion on the rows ``x`` (``ref`` / ``f32``: the float64 / float32 model on the same rows);
    ``plain``: the quantities held to the suite's 3e-2 against the plain float32 oracle (all, but for PLAIN_OPEN)."""
    for q in bm.FWD_QUANTITIES:
        assert np.isfinite(got[q]).all(), f"{tag} {q}: non-finite rows"
        v = bm.forward_verdict(bm.forward_row_err(q, got[q], ref), bm.forward_row_err(q, f32[q], ref))
        print(f"{tag} {q}: kernel p75 {v['p75']:.2e} worst {v['worst']:.2e} beyond {v['flipped']:.1%} | float32 model p75 "
              f"{v['p75_f32']:.2e} worst {v['worst_f32']:.2e} beyond {v['flipped_f32']:.1%} | bound {v['bound']:.2e}")
        assert v["flipped_f32"] <= bm.FWD_FLIP_SHARE_F32, f"{tag} {q}: the float32 model itself has {v['flipped_f32']:.1%} of its rows beyond the bound"
        assert v["p75"] <= v["bound"], f"{tag} {q}: 75th percentile {v['p75']:.3e} > {v['bound']:.3e}"
        assert v["flipped"] <= bm.FWD_FLIP_SHARE, f"{tag} {q}: {v['flipped']:.1%} of the rows beyond {v['bound']:.3e}"
    hold_plain(spec, flat, x, got, tag, plain)


def hold_plain(spec, flat, x, got, tag, quantities=bm.FWD_QUANTITIES):
    worst = {q: float(e.max()) for q, e in plain_errors(spec, flat, x, got).items()}
    print(f"{tag}: from the plain float32 oracle " + ", ".join(f"{q} {v:.2e}" for q, v in worst.items()))
    for q in quantities:
        assert worst[q] < bm.PLAIN_BOUND, f"{tag} {q}: {worst[q]:.3e} from the plain oracle"
    return worst


def prefix(d, n):
    return {k: v[:n] for k, v in d.items() if k != "tape"}


@pytest.mark.parametrize("D,T,H", list(FORWARD_SHAPES))
def test_forward_against_the_rounding_exact_model(D, T, H):
    spec = MAFSpec(D, T, hidden=H)
    flat = default_params(spec)
    f = bf16_flow(spec, flat)
    extra = FORWARD_SHAPES[(D, T, H)]
    counts = (33,) if extra is None else ROWS + extra
    x = rows_for(D, max(counts))
    ref = bm.BF16Model(spec, flat).forward(x)
    f32 = bm.BF16Model(spec, flat, np.float32).forward(x)
    xd = torch.from_numpy(x).cuda()
    for n in counts:
        tag = f"bf16 forward D={D} T={T} H={spec.hidden} n={n}"
        got = forward_call(f, xd, n)
        hold_forward(spec, flat, x[:n], got, prefix(ref, n), prefix(f32, n), tag,
                     plain=plain_held("d2-n16389" if (D, n) == (2, 16389) else None))
        for q in bm.FWD_QUANTITIES:                         # each output alone: the other two null
            alone = forward_call(f, xd, n, want=(q,))
            np.testing.assert_array_equal(alone[q], got[q], err_msg=f"{tag}: {q} requested alone")
    # the Flow's own entry points take the same path
    z, ladj = f.forward(torch.from_numpy(x[:33]))
    got = forward_call(f, xd, 33)
    np.testing.assert_array_equal(z.numpy(), got["z"])
    np.testing.assert_array_equal(ladj.numpy(), got["ladj"])
    np.testing.assert_array_equal(f.log_prob(torch.from_numpy(x[:33])).numpy(), got["log_prob"])


@pytest.mark.parametrize("D,T,H", [(33, 2, None), (64, 3, 256)])
def test_a_rows_outputs_do_not_depend_on_its_position(D, T, H):
    """Bit for bit: a permuted copy of the batch, and the same permutation through the ``idx`` gather argument."""
    spec = MAFSpec(D, T, hidden=H)
    f = bf16_flow(spec, default_params(spec))
    n = 53
    x = rows_for(D, n, seed=1)
    perm = np.random.default_rng(4).permutation(n)
    xd = torch.from_numpy(x).cuda()
    base = forward_call(f, xd, n)
    copy = forward_call(f, torch.from_numpy(np.ascontiguousarray(x[perm])).cuda(), n)
    gathered = forward_call(f, xd, n, idx=torch.from_numpy(perm.astype(np.int64)).cuda())
    short = forward_call(f, xd, 20, idx=torch.from_numpy(perm[:20].astype(np.int64)).cuda())
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(copy[q], base[q][perm], err_msg=f"{q}: permuted copy")
        np.testing.assert_array_equal(gathered[q], base[q][perm], err_msg=f"{q}: idx gather")
        np.testing.assert_array_equal(short[q], base[q][perm[:20]], err_msg=f"{q}: idx gather of 20 rows")


@pytest.mark.parametrize("D,T,H,n_big", [(7, 2, None, 4113), (2, 2, None, 16389)])
def test_a_rows_outputs_do_not_depend_on_the_row_sets(D, T, H, n_big):
    """The first 17 rows of a two-row-set call (eight waves at both sizes) against a call of 17 rows (eight waves, one row
    set): a tile's k order and the grouping of the log-determinant's per-wave partial sums depend on the wave count
    only, so z, ladj and log_prob are bit-equal."""
    spec = MAFSpec(D, T, hidden=H)
    f = bf16_flow(spec, default_params(spec))
    x = rows_for(D, n_big)
    xd = torch.from_numpy(x).cuda()
    big, small = forward_call(f, xd, n_big), forward_call(f, xd, 17)
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(big[q][:17], small[q], err_msg=q)
    # and the tail of the big launch: its last workgroup's rows against a launch that starts there
    tail0 = (n_big // 32) * 32
    tail = forward_call(f, xd[tail0:].contiguous(), n_big - tail0)
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(big[q][tail0:], tail[q], err_msg=f"{q}: tail")


def test_the_four_wave_launch():
    """``maf_forward_bf16_kernel<4, 1>``: n > 16384 on a flow whose two row sets do not fit 160 KB of LDS (H = 1024: 207 KB;
    one set 103 KB).  The criterion on the first 1024 and the last 517 rows (the float64 model of all 16389 takes 9 s), every
    row through the bit-for-bit checks: each output alone, a permuted copy, the ``idx`` gather; z of the first 17 rows
    against the sixteen-wave launch of 17 rows (the log-determinant's partial sums are grouped by wave there: it is held
    by the criterion)."""
    D, T, H, n = 4, 2, 1024, 16389
    spec = MAFSpec(D, T, hidden=H)
    nX2, nK2 = -(-spec.Dp // 32), -(-spec.Hp // 32)
    lds = lambda nw, rs: rs * (2 * spec.Dp * 16 * 4 + (2 * nX2 + 3 * nK2) * 1024) + 16 * nw * rs * 4      # fwd_bf16_lds
    assert lds(16, 2) > lds(8, 2) > 160 * 1024 >= lds(4, 1) and n > 16 * 1024        # (what sends this call to <4, 1>)
    flat = default_params(spec)
    f = bf16_flow(spec, flat)
    x = rows_for(D, n)
    xd = torch.from_numpy(x).cuda()
    got = forward_call(f, xd, n)
    sub = np.r_[0:1024, n - 517:n]
    ref = bm.BF16Model(spec, flat).forward(x[sub])
    f32 = bm.BF16Model(spec, flat, np.float32).forward(x[sub])
    hold_forward(spec, flat, x[sub], {q: got[q][sub] for q in bm.FWD_QUANTITIES}, prefix(ref, len(sub)), prefix(f32, len(sub)),
                 f"bf16 forward D={D} T={T} H={H} n={n} (four waves)")
    for q in bm.FWD_QUANTITIES:
        assert np.isfinite(got[q]).all()
        np.testing.assert_array_equal(forward_call(f, xd, n, want=(q,))[q], got[q], err_msg=f"{q} requested alone")
    perm = np.random.default_rng(8).permutation(n)
    copy = forward_call(f, torch.from_numpy(np.ascontiguousarray(x[perm])).cuda(), n)
    gathered = forward_call(f, xd, n, idx=torch.from_numpy(perm.astype(np.int64)).cuda())
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(copy[q], got[q][perm], err_msg=f"{q}: permuted copy")
        np.testing.assert_array_equal(gathered[q], got[q][perm], err_msg=f"{q}: idx gather")
    np.testing.assert_array_equal(got["z"][:17], forward_call(f, xd, 17)["z"])


# ---------------------------------------------------------------------------------------------------------- regimes
# (the edge rows of tests/flow_regimes.py -- knots, the box -- belong to the spline flows; the affine flows' edge rows are
# the non-finite ones)
REGIMES = {"maf3-d10-twin": None, "maf3-d10-g4": 4.0, "maf3-d10-g16": 16.0}      # tests/test_gpu_flow_regimes.py GAIN


@functools.lru_cache(maxsize=None)
def regime(name):
    """(spec, parameters, two-mode rows) of a trained / saturated flow (``tests/flow_regimes.py``)."""
    if REGIMES[name] is None:
        spec, flat = fr.twin_trained("maf3")
        return spec, flat, fr.two_modes(10, 1000, 9)
    spec = MAFSpec(10, 3)
    return spec, fr.gain_params(spec, REGIMES[name]), fr.two_modes(10, 1000, 9) * np.float32(1.3)


@pytest.mark.parametrize("name", list(REGIMES))
def test_forward_on_trained_and_saturated_flows(name):
    spec, flat, data = regime(name)
    f = bf16_flow(spec, flat)
    x = np.ascontiguousarray(data[:384])
    ref = bm.BF16Model(spec, flat).forward(x)
    f32 = bm.BF16Model(spec, flat, np.float32).forward(x)
    got = forward_call(f, torch.from_numpy(x).cuda(), len(x))
    hold_forward(spec, flat, x, got, prefix(ref, len(x)), prefix(f32, len(x)), f"bf16 forward {name}", plain=plain_held(name))


def open_case(case):
    """(spec, parameters, rows) of a case of PLAIN_OPEN."""
    if case == "d2-n16389":
        spec = MAFSpec(2, 2)
        return spec, default_params(spec), rows_for(2, 16389)
    spec, flat, data = regime(case)
    return spec, flat, np.ascontiguousarray(data[:384])


@pytest.mark.parametrize("case,q", [pytest.param(case, q, marks=pytest.mark.xfail(strict=True, reason=(
    f"open finding: the rounding-exact model itself is {fig:.2e} from the plain oracle in {q} here")))
    for case, open_q in PLAIN_OPEN.items() for q, fig in open_q.items()])
def test_open_finding_the_plain_oracle_bound(case, q):
    spec, flat, x = open_case(case)
    got = forward_call(bf16_flow(spec, flat), torch.from_numpy(x).cuda(), len(x))
    hold_plain(spec, flat, x, got, f"bf16 forward {case}", (q,))


def test_the_plain_oracle_bound_on_the_twins_log_prob():
    """Held where the float64 model on the twin's parameters AT HAND holds it (PLAIN_OPEN: they differ from machine to
    machine); where the model itself misses the 3e-2, the open finding, with both figures."""
    spec, flat, x = open_case("maf3-d10-twin")
    got = forward_call(bf16_flow(spec, flat), torch.from_numpy(x).cuda(), len(x))
    ref = bm.BF16Model(spec, flat).forward(x)
    model = plain_errors(spec, flat, x, {q: np.asarray(ref[q], np.float32) for q in bm.FWD_QUANTITIES})
    kernel = plain_errors(spec, flat, x, got)
    for q in PLAIN_BY_MODEL["maf3-d10-twin"]:
        print(f"bf16 forward maf3-d10-twin {q}: from the plain oracle kernel {kernel[q].max():.2e}, float64 model {model[q].max():.2e}")
        if model[q].max() >= bm.PLAIN_BOUND:
            pytest.xfail(f"open finding: the rounding-exact model itself is {model[q].max():.2e} from the plain oracle in {q} "
                         f"on these parameters (kernel {kernel[q].max():.2e})")
        assert kernel[q].max() < bm.PLAIN_BOUND, f"{q}: kernel {kernel[q].max():.3e}, model {model[q].max():.3e}"


@pytest.mark.parametrize("name", list(REGIMES))
@pytest.mark.parametrize("n", [64, 4096])
def test_non_finite_rows_stay_in_their_rows(name, n):
    """NaN / +inf / -inf in one coordinate of rows 0, 15, 16, 17 and n - 1: every other row is bit-identical to the same
    batch with those rows finite (one and two row sets per workgroup)."""
    spec, flat, data = regime(name)
    f = bf16_flow(spec, flat)
    good = np.ascontiguousarray(data[np.random.default_rng(n).choice(len(data), n, replace=n > len(data))])
    bad, rows = fr.with_nonfinite(good)
    keep = np.setdiff1d(np.arange(n), rows)
    a = forward_call(f, torch.from_numpy(good).cuda(), n)
    b = forward_call(f, torch.from_numpy(bad).cuda(), n)
    for q in bm.FWD_QUANTITIES:
        np.testing.assert_array_equal(b[q][keep], a[q][keep], err_msg=f"{name} n={n} {q}")
        assert np.isfinite(a[q]).all()
    assert not np.isfinite(b["z"][rows]).all(axis=1).any()           # (the bad rows do come out non-finite)


# ------------------------------------------------------------------------------------------------------------- pack
def test_pack_bf16_is_the_models_rne_bit_for_bit():
    from pocomc_amd import _lib
    lib = _lib.load()
    v, nan = bm.crafted_vector()
    n = len(v)
    idx = np.arange(n + 3, dtype=np.int32)
    idx[n], idx[n + 1], idx[n + 2] = -1, 0, -1                       # masked entries produce 0
    flat = torch.from_numpy(v).cuda()
    img = torch.full((n + 3,), 0x1234, dtype=torch.int16, device="cuda")
    with torch.cuda.device(flat.device):
        _lib.check(lib.pmc_maf_pack_bf16(_lib.ptr(flat), _lib.ptr(torch.from_numpy(idx).cuda()), _lib.ptr(img), n + 3,
                                         _lib.stream_handle()), "pmc_maf_pack_bf16")
    got = img.cpu().numpy().view(np.uint16)
    want = np.concatenate([bm.bf16_bits(v), np.array([0, bm.bf16_bits(v[:1])[0], 0], np.uint16)])
    np.testing.assert_array_equal(got, want)
    assert nan.sum() > 0 and ((got[:n][nan] & 0x7fc0) == 0x7fc0).all()


# ---------------------------------------------------------------------------------------------------------- trainer
TRAIN_CASES = [(5, 3, 32, 1, False), (5, 3, 32, 31, False), (5, 3, 32, 33, False), (16, 2, 64, 100, True),
               (33, 2, 128, 513, True),       # one row in the second 512-row chunk
               (50, 6, 256, 64, False), (128, 8, 512, 64, True)]


def kernel_loss_and_grad(f, x, w, idx=None):
    from pocomc_amd.train import loss_and_grad, _train_state
    loss = float(loss_and_grad(f, torch.from_numpy(x).cuda(), None if w is None else torch.from_numpy(w).cuda(),
                               idx=None if idx is None else torch.from_numpy(idx).cuda()))
    return loss, _train_state(f).grad.cpu().numpy().copy()


def hold_trainer(spec, flat, f, x, w, tag):
    R = bm.TrainReference(spec, flat, x, w)
    loss, g = kernel_loss_and_grad(f, x, w)
    v = R.verdict(loss, g)
    print(f"{tag}: kernel (float32 yardstick) {v['summary']}; largest kernel / yardstick {max(v['ratio'].values()):.2f}")
    assert np.all(g[spec.mask_flat() == 0] == 0.0), f"{tag}: a masked entry was written"
    assert v["ok"], f"{tag}: beyond {bm.TRAIN_C:g} x the yardstick: " + ", ".join(
        f"{k} {v['measures'][k]:.3e} > {v['limits'][k]:.3e}" for k in v["failing"])


@pytest.mark.parametrize("D,T,H,n,weighted", TRAIN_CASES)
def test_trainer_against_the_rounding_exact_model(D, T, H, n, weighted):
    spec = MAFSpec(D, T, hidden=H)
    flat = default_params(spec, 2)
    f = bf16_flow(spec, flat, engine="bf16")
    x = rows_for(D, n, seed=n)
    w = np.random.default_rng(n).uniform(0.1, 1.0, size=n).astype(np.float32) if weighted else None
    hold_trainer(spec, flat, f, x, w, f"bf16 trainer D={D} T={T} H={H} n={n} w={int(weighted)}")


@pytest.mark.parametrize("weighted", [False, True])
def test_trainer_on_the_trained_twin(weighted):
    spec, flat, data = regime("maf3-d10-twin")
    f = bf16_flow(spec, flat, engine="bf16")                 # (H = 32: the engine is forced)
    x = np.ascontiguousarray(data[:100])
    w = np.random.default_rng(7).uniform(0.1, 1.0, size=len(x)).astype(np.float32) if weighted else None
    hold_trainer(spec, flat, f, x, w, f"bf16 trainer maf3-d10-twin n={len(x)} w={int(weighted)}")


def test_indexed_batch_is_the_contiguous_batch_bit_for_bit_across_the_chunk_boundary():
    D, T, H, n = 33, 2, 128, 513
    spec = MAFSpec(D, T, hidden=H)
    f = bf16_flow(spec, default_params(spec, 2), engine="bf16")
    x = rows_for(D, n, seed=n)
    w = np.random.default_rng(n).uniform(0.1, 1.0, size=n).astype(np.float32)
    loss, g = kernel_loss_and_grad(f, x, w)
    perm = np.random.default_rng(6).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    loss2, g2 = kernel_loss_and_grad(f, np.ascontiguousarray(x[perm]), np.ascontiguousarray(w[perm]), idx=inv)
    assert loss2 == loss
    np.testing.assert_array_equal(g2, g)
    loss3, g3 = kernel_loss_and_grad(f, x, w)                # (and a second call reproduces the first)
    assert loss3 == loss
    np.testing.assert_array_equal(g3, g)
