"""Which instance of the float32 flow kernels a default-width flow takes (``pmc_maf_lds_plan``, ``csrc/inverse_plan.hip``),
for every n_dim from 2 to 157 -- the widest MCMC step -- and both families.  The query reads layout fields only: no GPU.

The FULL instances keep three (the trainer: four) hidden-width activation arrays of 16 rows in LDS; their byte counts are
restated here from the launchers as they were before the lean instances existed.  The reference's width rule
(``flow.py:52``) gives H = 512 from D = 86 upwards and ``MAFSpec`` pads every degree group to whole quads (Hp up to 816
at D = 102 - 104), so those counts exceed the 160 KiB of a workgroup at the D listed in ``REFUSED`` below: there, and only
there, the query must report the LEAN instances (two hidden-width arrays), and nothing may be refused."""
import ctypes as C

import pytest

from pocomc_amd.maf_spec import MAFSpec

CAP = 160 * 1024
DS = range(2, 158)
AUTO, NAIVE = 0, 2
S_DPASS_LEAN = 8                 # PMC_SWEEP_DPASS_LEAN
LEAN_BIT = 8                     # PMC_MAF_VARIANT_LEAN_LDS
FAMILIES = ("affine", "rqs")


def span(*pairs):
    return {d for a, b in pairs for d in range(a, b + 1)}


# the D at which the full instances do not fit (the table of the issue this file came with)
REFUSED = {
    ("affine", "forward"): span((98, 107)),
    ("rqs", "forward"): span((86, 118), (154, 157)),
    ("affine", "train"): span((86, 127), (130, 157)),
    ("rqs", "train"): span((86, 157)),
    ("affine", "inverse"): span((96, 110)),      # lane sweep and lone-wave D-pass both too big
    ("rqs", "inverse"): span((97, 108)),         # lone-wave sweep too big
}


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


def spec(D, uni):
    return MAFSpec(D, 2, univariate=uni)


def descriptor(s, reserved=0):
    from pocomc_amd import _lib
    return _lib.pmc_maf_t(packed=None, meta=None, D=s.n_dim, H=s.hidden, T=s.n_transforms, Hp=s.Hp, Dp=s.Dp, nT=s.nT,
                          nXT=s.nXT, nOT=s.nOT, pk_per_transform=s.pk_per_transform, tri_ok=int(s.tri_ok), n_out=s.n_out,
                          lane16=None, lane16_fmt=0, reserved=reserved)


def lds_plan(lib, s, reserved=0):
    from pocomc_amd import _lib
    d, p = descriptor(s, reserved), _lib.pmc_flow_lds_plan_t()
    rc = lib.pmc_maf_lds_plan(C.byref(d), C.byref(p))
    return rc, {k: getattr(p, k) for k, _ in p._fields_}


def inverse_plan(lib, s, algo, n=5000, reserved=0):
    from pocomc_amd import _lib
    d, p = descriptor(s, reserved), _lib.pmc_inverse_plan_t()
    if lib.pmc_maf_inverse_plan(C.byref(d), n, algo, 0, C.byref(p)):
        return lib.pmc_last_error().decode()
    return {k: getattr(p, k) for k, _ in p._fields_}


# ---- the parent's formulas (bytes): maf_forward_wg.hip's launcher with eight wavefronts, maf_train.hip's train_lds_bytes
def panel(s):
    return 0 if s.n_out == 2 else s.n_out


def full_wg(s, inverse):
    return 4 * (2 * s.Dp * 16 + 3 * s.Hp * 16 + 16 * 8 + panel(s) * 256 + (s.Dp * 16 if inverse else 0))


def full_train(s):
    def size(ksplit):
        part = 16 * 256 if ksplit else 0
        if s.n_out != 2:
            return 4 * (4 * s.Hp * 16 + s.n_out * 256 + 2 * s.Dp * 16 + 16 + 16 * 16 + part)
        return 4 * (4 * s.Hp * 16 + 2 * s.Dp * 16 + s.Dp * 16 + 16 + 16 * 16 + part)
    return size(size(True) <= 64 * 1024)


def full_lane(s, ns):             # float32 helpers (tests/test_inverse_plan_cpu.py: lds_lane)
    return 4 * (ns * (2 * s.Dp * 16 + 3 * s.nT * 256) + 3 * 2 * ns * 16 * 20 + 2 * 2 * 16 * ns * 20) + 64


def full_dense(s):
    return 4 * (3 * s.Dp * 16 + 3 * s.Hp * 16)


def full_nsf_solo(s):
    return 4 * (2 * s.Dp * 16 + 3 * s.Hp * 16 + 16 * 32 + 16 * 24)


# ---- the lean instances: two hidden-width arrays; the affine trainer gets the x buffer the spline one has
def lean_wg(s, inverse):
    return full_wg(s, inverse) - 4 * s.Hp * 16


def lean_train(s):
    assert full_train(s) > 64 * 1024           # (no partial-tile staging at these sizes)
    return full_train(s) - 4 * 2 * s.Hp * 16 + (4 * s.Dp * 16 if s.n_out == 2 else 0)


@pytest.mark.parametrize("uni", FAMILIES)
def test_lean_exactly_where_the_full_instance_exceeds_the_lds(lib, uni):
    seen = {"forward": set(), "dpass": set(), "train": set()}
    for D in DS:
        s = spec(D, uni)
        rc, p = lds_plan(lib, s)
        assert rc == 0, (D, lib.pmc_last_error())                     # nothing is refused
        full = {"forward": full_wg(s, 0), "dpass": full_wg(s, 1), "train": full_train(s)}
        lean = {"forward": lean_wg(s, 0), "dpass": lean_wg(s, 1), "train": None}
        for call in seen:
            assert p[call + "_full_bytes"] == full[call], (D, call)
            assert p[call + "_lean"] == int(full[call] > CAP), (D, call)
            if p[call + "_lean"]:
                seen[call].add(D)
                want = lean[call] if lean[call] is not None else lean_train(s)
                assert p[call + "_lds_bytes"] == want <= CAP, (D, call)
            else:
                assert p[call + "_lds_bytes"] == full[call], (D, call)
    assert seen["forward"] == REFUSED[(uni, "forward")]
    assert seen["train"] == REFUSED[(uni, "train")]
    assert seen["dpass"] >= seen["forward"]                           # (the inverse's iterate makes the D-pass larger)


def test_the_widest_lean_plan():
    """The largest lean launch over both families and all D <= 157 is the spline D-pass at D = 102 - 104 (Hp = 816, Dp = 112)."""
    sizes = {(D, u): max(lean_wg(spec(D, u), 1), lean_train(spec(D, u)) if D >= 86 else 0) for D in DS for u in FAMILIES}
    assert max(sizes.values()) == 150016 and {k for k, v in sizes.items() if v == 150016} == {(D, "rqs") for D in (102, 103, 104)}
    assert max(spec(D, "affine").nT for D in DS) == 51 == spec(104, "affine").nT


@pytest.mark.parametrize("uni", FAMILIES)
def test_auto_inverse_falls_back_to_the_lean_dpass_only_where_nothing_else_fits(lib, uni):
    lean = set()
    for D in DS:
        s = spec(D, uni)
        p = inverse_plan(lib, s, AUTO)
        assert isinstance(p, dict), (D, p)
        if uni == "affine":
            nothing = min(full_lane(s, 1), full_dense(s)) > CAP and D > 64
        else:
            nothing = full_nsf_solo(s) > CAP and D > 64
        assert (p["sweep"] == S_DPASS_LEAN) == nothing, (D, p)
        if nothing:
            lean.add(D)
            assert p == dict(sweep=S_DPASS_LEAN, fused=0, epilogue=0, maxo=0, fm=0, subsets=0, waves=0, helper_fmt=0,
                             lds_bytes=lean_wg(s, 1)), D
            assert inverse_plan(lib, s, NAIVE) == p, D
        else:
            # every other D keeps the sweep it has: the affine flows the two-wave / lane-per-walker sweep, the spline flows
            # the two-wave (D <= 64) / lone-wave one
            if not s.tri_ok:                  # (D = 2, 3: one degree group wider than a tile -- the full D-pass kernels)
                assert D <= 3 and p["sweep"] == (1 if uni == "affine" else 2), (D, p)
            elif uni == "affine":
                if s.nT < 16 and D <= 64:
                    assert p["sweep"] == 4, (D, p)
                elif full_lane(s, 1) <= CAP:
                    assert p["sweep"] == 5 and p["lds_bytes"] == full_lane(s, p["subsets"]) <= CAP, (D, p)
                else:                          # (lane sweep beyond the LDS, the lone-wave D-pass kernel within: as before)
                    assert p["sweep"] == 1 and p["lds_bytes"] == full_dense(s) <= CAP, (D, p)
            else:
                assert p["sweep"] == (7 if D <= 64 else 6), (D, p)
                if p["sweep"] == 6:
                    assert p["lds_bytes"] == full_nsf_solo(s), D
    assert lean == REFUSED[(uni, "inverse")]


def test_the_fallback_is_bounded_to_default_width_layouts(lib):
    """Beyond 51 hidden tiles -- more than any default-width flow has for D <= 157 -- a layout keeps the refusal it had,
    although a two-array D-pass would fit it (``tests/test_inverse_plan_cpu.py`` pins the 64-tile flow at D = 66)."""
    s = MAFSpec(66, 3, 582)
    assert s.nT == 64 and lean_wg(s, 1) <= CAP < full_dense(s)
    assert inverse_plan(lib, s, AUTO, n=17) == "MAF too wide for one wave's LDS budget (160 KiB)"
    assert inverse_plan(lib, s, NAIVE, n=17) == "MAF too wide for one wave's LDS budget (160 KiB)"


@pytest.mark.parametrize("uni", FAMILIES)
@pytest.mark.parametrize("D", [10, 32])
def test_the_variant_bit_forces_the_lean_instances(lib, uni, D):
    s = MAFSpec(D, 3, univariate=uni)
    rc, p = lds_plan(lib, s)
    assert rc == 0 and (p["forward_lean"], p["dpass_lean"], p["train_lean"]) == (0, 0, 0)
    rc, q = lds_plan(lib, s, LEAN_BIT)
    assert rc == 0 and (q["forward_lean"], q["dpass_lean"], q["train_lean"]) == (1, 1, 1)
    assert q["forward_lds_bytes"] == p["forward_lds_bytes"] - 4 * s.Hp * 16
    assert q["dpass_lds_bytes"] == p["dpass_lds_bytes"] - 4 * s.Hp * 16
    assert q["train_lds_bytes"] == p["train_lds_bytes"] - 8 * s.Hp * 16 + (4 * s.Dp * 16 if uni == "affine" else 0)
    assert [q[k + "_full_bytes"] for k in ("forward", "dpass", "train")] == [p[k + "_lds_bytes"] for k in ("forward", "dpass", "train")]
    # the inverse: AUTO keeps its sweep, the D-pass algorithm goes through the lean workgroup kernel
    assert inverse_plan(lib, s, AUTO, reserved=LEAN_BIT) == inverse_plan(lib, s, AUTO)
    assert inverse_plan(lib, s, NAIVE)["sweep"] == (1 if uni == "affine" else 2)
    forced = inverse_plan(lib, s, NAIVE, reserved=LEAN_BIT)
    assert (forced["sweep"], forced["lds_bytes"]) == (S_DPASS_LEAN, q["dpass_lds_bytes"])


def test_a_flow_beyond_both_instances_is_refused_with_the_launchers_message(lib):
    from pocomc_amd import _lib
    import inverse_plan_cases as ic
    d, p = ic.descriptor("nsf_wide_hand", _lib.pmc_maf_t), _lib.pmc_flow_lds_plan_t()       # 160 hidden tiles
    assert lib.pmc_maf_lds_plan(C.byref(d), C.byref(p)) != 0
    assert lib.pmc_last_error().decode() == "pmc_maf_forward: flow too wide for 160 KB of LDS"
    assert (p.forward_lean, p.dpass_lean, p.train_lean) == (-1, -1, -1)
    assert lib.pmc_maf_lds_plan(None, C.byref(p)) != 0
