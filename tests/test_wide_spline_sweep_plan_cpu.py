"""The plan of the workgroup inverse sweep of the spline flows (``PMC_INVERSE_TRIANGULAR_WG_NSF`` -> ``PMC_SWEEP_WG_NSF``,
``csrc/inverse_plan.hip``): an opt-in that covers every default-width 8-bin spline flow from n_dim 3 to 157 -- the
D = 97 - 108 that no other spline sweep fits among them -- and changes nothing about what AUTO, NAIVE and the affine
flows' workgroup sweep answer.  Host functions only: no GPU.

The sweep's LDS is restated here from its layout (``csrc/maf_inverse_wg_nsf.hip``): x and y by rank, the partial
pre-activations of hidden layer 1, the array of layer 2's partials / final h2 tiles, three tiles of the current hidden
tile's units, one output-partial tile per wavefront (eight), the rank's parameter panel [16][32] and knot tables [16][24],
the log-determinant words of eight wavefronts."""
import ctypes as C

import pytest

from pocomc_amd.maf_spec import MAFSpec
from test_wide_default_plan_cpu import descriptor, inverse_plan, lean_wg

CAP = 160 * 1024
AUTO, NAIVE, WG, WG_NSF = 0, 2, 10, 11
S_WG_NSF, S_DPASS_LEAN = 10, 8
DS = range(3, 158)

TRI = "pmc_maf_inverse: triangular sweep needs degree groups <= one tile"
BINS = "pmc_maf_inverse: the spline sweeps are built for 8 bins (PMC_INVERSE_NAIVE covers the others)"
TOO_WIDE = "pmc_maf_inverse: the workgroup spline sweep needs its arrays in 160 KiB of LDS"
SPLINE = "pmc_maf_inverse: spline flows know PMC_INVERSE_TRIANGULAR (_SOLO, _DUO) and PMC_INVERSE_NAIVE"
NO_FIELDS = dict(fused=0, epilogue=0, maxo=0, fm=0, subsets=0, waves=0, helper_fmt=0)


def nsf(D):
    return MAFSpec(D, 2, univariate="rqs")


def wg_nsf_bytes(s):
    return 4 * (2 * s.Dp * 16 + 2 * s.Hp * 16 + 3 * 256 + 8 * 256 + 16 * 32 + 16 * 24 + 16 * 8)


def nsf_solo_bytes(s):
    """The lone-wave spline sweep: three hidden-width arrays."""
    return 4 * (2 * s.Dp * 16 + 3 * s.Hp * 16 + 16 * 32 + 16 * 24)


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


def test_the_formula_at_the_sizes_the_design_quotes():
    assert {D: wg_nsf_bytes(nsf(D)) for D in (10, 86, 102, 157)} == {10: 23552, 86: 115712, 102: 134144, 157: 115712}


def test_the_sweep_covers_every_default_width_spline_flow(lib):
    sizes = {}
    for D in DS:
        s = nsf(D)
        sizes[D] = wg_nsf_bytes(s)
        assert sizes[D] <= CAP, D
        for n in (1, 17, 5000, 8193):
            assert inverse_plan(lib, s, WG_NSF, n=n) == dict(sweep=S_WG_NSF, lds_bytes=sizes[D], **NO_FIELDS), (D, n)
    widest = max(sizes.values())
    assert widest == 134144 and {D for D, v in sizes.items() if v == widest} == {102, 103, 104}


def test_why_the_sweep_exists():
    """The lone-wave spline sweep exceeds the LDS at exactly the D this sweep was built for."""
    assert {D for D in DS if nsf_solo_bytes(nsf(D)) > CAP} == set(range(97, 109))


def test_the_step_has_no_fused_instance_of_it(lib):
    from pocomc_amd import _lib
    for D in (10, 33, 102):
        d, p = descriptor(nsf(D)), _lib.pmc_inverse_plan_t()
        assert lib.pmc_maf_inverse_plan(C.byref(d), 21, WG_NSF, 1, C.byref(p)) == 0
        assert {k: getattr(p, k) for k, _ in p._fields_} == dict(sweep=0, lds_bytes=0, **NO_FIELDS), D


def test_refusals(lib):
    s = MAFSpec(2, 2, univariate="rqs")
    assert not s.tri_ok and inverse_plan(lib, s, WG_NSF) == TRI
    for bins in (4, 16):
        s = MAFSpec(10, 2, univariate="rqs", bins=bins)
        assert s.tri_ok and s.n_out == 3 * bins - 1 and inverse_plan(lib, s, WG_NSF) == BINS, bins
    # a hand-made width beyond the cap whose degree groups still fit a tile: 79 groups of 16 units
    s = MAFSpec(80, 3, 79 * 16, univariate="rqs")
    assert s.tri_ok and s.n_out == 23 and wg_nsf_bytes(s) == 187392 > CAP
    assert inverse_plan(lib, s, WG_NSF, n=17) == TOO_WIDE
    # the affine flows' opt-in stays the affine flows': the message spline flows always had
    for D in (10, 64, 102):
        assert inverse_plan(lib, nsf(D), WG) == SPLINE, D
        for algo in (8, 9):
            assert inverse_plan(lib, nsf(D), algo) == SPLINE, (D, algo)
    # ... and this one is unknown to the affine flows
    assert inverse_plan(lib, MAFSpec(102, 2), WG_NSF) == "pmc_maf_inverse: unknown algo"


def test_auto_and_naive_keep_their_plans(lib):
    s = nsf(102)
    want = dict(sweep=S_DPASS_LEAN, lds_bytes=lean_wg(s, 1), **NO_FIELDS)
    assert inverse_plan(lib, s, AUTO) == want and inverse_plan(lib, s, NAIVE) == want
