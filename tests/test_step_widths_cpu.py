"""The references and bounds of ``tests/step_widths.py`` are sound: what ``test_gpu_step_widths.py`` holds the step's kernels
to is wider than float64, never vacuous, and able to tell the orders and decisions apart that the kernels could get wrong."""
import numpy as np
import pytest

import step_widths as sw


def test_the_extended_reference_is_wider_than_float64():
    assert sw.EXT_EPS < 2.0 ** -53
    one = sw.ext(np.float64(1.0))
    tiny = sw.ext(np.float64(2.0 ** -60))
    assert (one + tiny) - one == tiny                     # float64 would lose the term


@pytest.mark.parametrize("D", sw.PROPOSE_D)
def test_float64_proposal_stays_within_the_bound_in_both_orders(D):
    """A float64 restatement, summed first to last and last to first, against the extended reference: within the bound
    (SAFETY included), and every bound at most 1e-6 of what it bounds."""
    for cond in sw.CONDS:
        for nu in sw.NUS:
            case = sw.propose_case(D, 81, cond, nu, seed=7)
            z, g = sw.host_variates(case)
            for tpcn in (True, False):
                if not tpcn and nu != sw.NUS[0]:
                    continue                               # (RWM does not read nu)
                ref = sw.propose_reference(case, z, g, tpcn)
                for reverse in (False, True):
                    r = sw.propose_ratios(ref, sw.propose_float64(case, z, g, tpcn, reverse))
                    assert set(r) == ({"theta", "quad", "quad_prop"} if tpcn else {"theta"})
                    assert max(r.values()) <= 1.0, (D, cond, nu, tpcn, reverse, r)
                sizes = sw.propose_bound_sizes(ref)
                assert max(sizes.values()) <= 1e-6, (D, cond, nu, tpcn, sizes)
                assert min(float(np.min(ref[k])) for k in ref if k.endswith("_bound")) > 0.0


def test_the_proposal_bound_notices_a_swapped_pair_and_a_dropped_term():
    """What the bound is for: a z pair handed over the wrong way round, or one product missing from a row of L z, is
    far outside it."""
    case = sw.propose_case(17, 81, 1e4, 5.0, seed=7)
    z, g = sw.host_variates(case)
    ref = sw.propose_reference(case, z, g)
    swapped = z.copy()
    swapped[:, [4, 5]] = swapped[:, [5, 4]]
    assert sw.propose_ratios(ref, sw.propose_float64(case, swapped, g))["theta"] > 1e6
    dropped = dict(case, chol=case["chol"].copy())
    dropped["chol"][16, 12] = 0.0                          # a K step above the diagonal tile's start skipped
    assert sw.propose_ratios(ref, sw.propose_float64(dropped, z, g))["theta"] > 1e6


@pytest.mark.parametrize("D", sw.SCALER_D)
def test_the_sum_tree_rows_can_tell_the_orders_apart(D):
    """logdetj of the sum-tree case is numpy's pairwise sum (restated here, recursion included), and for D >= 16 a
    sequential sum differs on most rows: the bit-for-bit equality on the device proves the order."""
    c = sw.sum_tree_case(D, 130)
    tree = np.array([c["sum_log_sigma"] + sw.numpy_pairwise(c["t"][r]) for r in range(c["n"])])
    assert np.array_equal(tree.view(np.uint64), c["logdetj"].view(np.uint64))
    assert np.isfinite(c["x"]).all() and np.isfinite(c["logdetj"]).all()
    if D >= 16:
        seq = np.array([c["sum_log_sigma"] + sw.sequential_sum(c["t"][r]) for r in range(c["n"])])
        assert (seq != c["logdetj"]).mean() > 0.5
    if D > 128 and (D // 2) % 8:
        # the split point matters as well: halves that are not rounded down to a multiple of 8 give other bits
        n2 = D // 2
        other = np.array([c["sum_log_sigma"] + (sw.numpy_pairwise(c["t"][r][:n2]) + sw.numpy_pairwise(c["t"][r][n2:]))
                          for r in range(c["n"])])
        assert (other != c["logdetj"]).mean() > 0.25


def test_limits_are_the_lds_arithmetic():
    lds = 160 * 1024
    assert 2 * sw.PROPOSE_D_MAX * 65 * 8 <= lds < 2 * (sw.PROPOSE_D_MAX + 1) * 65 * 8
    assert 64 * sw.SCALER_D_MAX_PLAIN * 8 + 256 <= lds < 64 * (sw.SCALER_D_MAX_PLAIN + 1) * 8 + 256
    keep = lambda D: (64 + 65) * D * 8 + 256
    assert keep(sw.SCALER_D_MAX_KEEP_X) <= lds < keep(sw.SCALER_D_MAX_KEEP_X + 1)
    assert max(sw.PROPOSE_D) == sw.PROPOSE_D_MAX and max(sw.SCALER_D) == sw.SCALER_D_MAX_PLAIN


def test_accept_widths_are_the_fold_classes():
    S = {D: max(1, 256 // min(256, D + 4)) for D in sw.ACCEPT_D}
    assert {1, 2, 3, 4}.issubset(set(S.values())) and S[1] == 51
    assert [D for D in sw.ACCEPT_D if D + 4 > 256] == [253, 300]
    for a, b in ((28, 29), (60, 61), (124, 125), (252, 253)):          # S changes between them
        assert (256 // (a + 4)) != (256 // (b + 4)) or b + 4 > 256
    assert 817 > 16 * S[1] and 33 > 16 * S[124]                        # a second round of 16 blocks in flight


@pytest.mark.parametrize("D", [1, 33, 124, 300])
@pytest.mark.parametrize("pre,tpcn", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_accept_cases_decide_away_from_the_knife_edge(D, pre, tpcn):
    for n in sw.accept_rows(D):
        if n > 5000:
            continue
        c = sw.accept_case(D, n, pre, tpcn)
        assert sw.accept_knife_edges(c) == 0
        a = c["alpha"]
        assert (a[c["neg"]] == 0.0).all() and (a[c["nan"]] == 0.0).all() and ((a >= 0) & (a <= 1)).all()
        acc, post = sw.accept_post_state(c)
        assert not acc[c["neg"] | c["nan"]].any()
        if n >= 64:
            assert 0 < acc.sum() < n and ((a > 0) & (a < 1)).sum() >= n // 8      # both decisions, and ratios that are neither
        assert all(np.isfinite(v).all() for v in post.values())
        terms = sw.accept_sum_terms(c, a, post)
        assert set(terms) == {0, 1, 2} | {4 + j for j in range(D)}
        for t in terms.values():
            s, b = sw.fsum_and_bound(t)
            assert abs(float(np.sum(t)) - s) <= b
