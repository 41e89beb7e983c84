"""The plan of the workgroup inverse sweep (``PMC_INVERSE_TRIANGULAR_WG`` -> ``PMC_SWEEP_WG``, ``csrc/inverse_plan.hip``):
an opt-in that covers every default-width affine flow from n_dim 3 to 157 -- the D = 92 - 114 that no other triangular
sweep fits among them -- and changes nothing about what AUTO and NAIVE choose.  Host functions only: no GPU.

The sweep's LDS is restated here from its layout (``csrc/maf_inverse_wg.hip``): x and y by rank, the partial
pre-activations of the two hidden layers, the partial output rows, three tiles of the current hidden tile's units and the
log-determinant words of eight wavefronts."""
import ctypes as C

import pytest

from pocomc_amd.maf_spec import MAFSpec
from test_wide_default_plan_cpu import descriptor, inverse_plan, lean_wg

CAP = 160 * 1024
AUTO, NAIVE, WG = 0, 2, 10
S_WG, S_DPASS_LEAN = 9, 8
DS = range(3, 158)

TRI = "pmc_maf_inverse: triangular sweep needs degree groups <= one tile"
TOO_WIDE = "pmc_maf_inverse: the workgroup sweep needs its arrays in 160 KiB of LDS"
SPLINE = "pmc_maf_inverse: spline flows know PMC_INVERSE_TRIANGULAR (_SOLO, _DUO) and PMC_INVERSE_NAIVE"


def wg_bytes(s):
    return 4 * (2 * s.Dp * 16 + 2 * s.Hp * 16 + s.nOT * 256 + 3 * 256 + 16 * 8)


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


def test_the_formula_at_the_sizes_the_design_quotes():
    assert {D: wg_bytes(MAFSpec(D, 2)) for D in (92, 102, 114, 157, 10)} == {92: 122368, 102: 136704, 114: 126464,
                                                                            157: 124416, 10: 13824}


def test_the_sweep_covers_every_default_width_affine_flow(lib):
    sizes = {}
    for D in DS:
        s = MAFSpec(D, 2)
        sizes[D] = wg_bytes(s)
        assert sizes[D] <= CAP, D
        for n in (1, 17, 5000, 8193):
            assert inverse_plan(lib, s, WG, n=n) == dict(sweep=S_WG, fused=0, epilogue=0, maxo=0, fm=0, subsets=0, waves=0,
                                                         helper_fmt=0, lds_bytes=sizes[D]), (D, n)
    widest = max(sizes.values())
    assert widest == 136704 and {D for D, v in sizes.items() if v == widest} == {102, 103, 104}


def test_the_step_has_no_fused_instance_of_it(lib):
    from pocomc_amd import _lib
    for D in (10, 33, 102):
        d, p = descriptor(MAFSpec(D, 2)), _lib.pmc_inverse_plan_t()
        assert lib.pmc_maf_inverse_plan(C.byref(d), 21, WG, 1, C.byref(p)) == 0
        assert {k: getattr(p, k) for k, _ in p._fields_} == dict(sweep=0, fused=0, epilogue=0, maxo=0, fm=0, subsets=0,
                                                                 waves=0, helper_fmt=0, lds_bytes=0), D


def test_refusals(lib):
    for D in (10, 64, 102):
        assert inverse_plan(lib, MAFSpec(D, 2, univariate="rqs"), WG) == SPLINE, D
    s = MAFSpec(2, 2)
    assert not s.tri_ok and inverse_plan(lib, s, WG) == TRI
    # a hand-made width beyond the cap.  (At D = 66 every width whose degree groups fit a tile -- at most 16 units in each
    # of 65 groups -- stays within it, and MAFSpec(66, 3, 1600) is refused for its groups; 79 groups of 16 units exceed it)
    s = MAFSpec(66, 3, 1600)
    assert not s.tri_ok and wg_bytes(s) > CAP and inverse_plan(lib, s, WG, n=17) == TRI
    s = MAFSpec(66, 3, 65 * 16)
    assert s.tri_ok and wg_bytes(s) <= CAP
    s = MAFSpec(80, 3, 79 * 16)
    assert s.tri_ok and s.n_out == 2 and wg_bytes(s) == 185856 > CAP
    assert inverse_plan(lib, s, WG, n=17) == TOO_WIDE
    # ... and the widest of that D within it
    s = MAFSpec(66, 3, 582)
    assert wg_bytes(s) <= CAP and inverse_plan(lib, s, WG, n=17)["sweep"] == S_WG


def test_auto_and_naive_keep_their_plans(lib):
    s = MAFSpec(102, 2)
    want = dict(sweep=S_DPASS_LEAN, fused=0, epilogue=0, maxo=0, fm=0, subsets=0, waves=0, helper_fmt=0, lds_bytes=lean_wg(s, 1))
    assert inverse_plan(lib, s, AUTO) == want and inverse_plan(lib, s, NAIVE) == want
    assert inverse_plan(lib, s, 11) == "pmc_maf_inverse: unknown algo"
