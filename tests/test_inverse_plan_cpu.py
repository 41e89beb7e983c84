"""The inverse plan (``csrc/inverse_plan.hip``: which flow-inverse kernel instance a call launches) on hand-filled
descriptors -- the plan reads layout fields only, so none of this needs a GPU.

(a) the three ``pmc_maf_inverse_auto_is_*`` queries against the answers of the parent commit's library
    (``tests/golden/inverse_queries_parent.json``), with the cases where the old query did not say what the launch path did;
(b) full plans written by hand from the rules of the launch path as it was before the plan existed, every algo constant,
    every error message of ``pmc_maf_inverse``, the fused question with and without the epilogue (the public query takes
    the scaler as eligible and as wide as the flow, so what decides here is whether the epilogue's scratch fits the
    activation arrays; a scaler or prior that does not qualify, another width and ``no_fuse & 2`` are ``pmc_step_pre``'s
    inputs: the ``no_fuse = 2`` runs of ``tests/test_gpu_epilogue_rows.py`` cover them);
(c) invariants over the whole grid of cases x rows x algos x (plain, fused)."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_plan_cases as ic  # noqa: E402

AUTO, TRI, NAIVE, SOLO, DUO, LANE, LANE16 = 0, 1, 2, 6, 7, 8, 9
ALGOS = (AUTO, TRI, NAIVE, SOLO, DUO, LANE, LANE16)
S_NONE, S_DPASS_AFFINE, S_DPASS_SPLINE, S_SOLO, S_DUO, S_LANE, S_NSF_SOLO, S_NSF_DUO = range(8)
FIELDS = ("sweep", "fused", "epilogue", "maxo", "fm", "subsets", "waves", "helper_fmt", "lds_bytes")
CAP = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


def plan(lib, name, n, algo, fused=0):
    """The plan as a dict, or the error message."""
    from pocomc_amd import _lib
    d, p = ic.descriptor(name, _lib.pmc_maf_t), _lib.pmc_inverse_plan_t()
    if lib.pmc_maf_inverse_plan(C.byref(d), n, algo, fused, C.byref(p)):
        return lib.pmc_last_error().decode()
    return {k: getattr(p, k) for k in FIELDS}


# ------------------------------------------------------------------------------------------------ (a) the parent's answers
# Where the old query and the launch path disagreed, the plan -- what is launched -- wins.  Each case by name:
IS_DUO_EXCEPTIONS = {
    # D <= 64 with >= 16 hidden tiles: AUTO launches the lane-per-walker sweep (pmc_tri6_preferred came first in
    # pmc_launch_inverse_tri4), while _is_duo only asked whether the two-wave tables fit
    "t16": "AUTO launches the lane sweep (16 hidden tiles); the old query looked at the two-wave LDS only",
    "t16_bf16": "the same flow with a bfloat16 helper image: the lane sweep",
    "t16_f16": "the same flow with a float16 helper image: the lane sweep",
}
IS_LANE_EXCEPTIONS = {
    # nOT > 8 answered 1 whatever pmc_launch_tri6 said; it refuses nT > 64 and a subset beyond the LDS, and AUTO then
    # runs (or fails in) the D-pass kernel
    "t46_d66": "46 hidden tiles: one float32 subset needs 164.9 KB of LDS, AUTO runs the D-pass kernel",
    "t64_d66": "64 hidden tiles in float32: beyond the LDS, AUTO ends in the D-pass kernel's error",
    "t65_d66": "65 hidden tiles: beyond the lane sweep's 64",
    "t65_d66_bf16": "65 hidden tiles: beyond the lane sweep's 64 whatever the helpers' format",
}


def test_queries_answer_what_the_parent_answered(lib):
    from pocomc_amd import _lib
    with open(os.path.join(os.path.dirname(ic.__file__), "golden", "inverse_queries_parent.json")) as f:
        parent = json.load(f)
    assert set(parent["answers"]) == set(ic.CASES) and tuple(parent["rows"]) == ic.ROWS
    for name, old in parent["answers"].items():
        d = ic.descriptor(name, _lib.pmc_maf_t)
        lane, nsf2 = lib.pmc_maf_inverse_auto_is_lane(C.byref(d)), lib.pmc_maf_inverse_auto_is_nsf2(C.byref(d))
        assert nsf2 == old["is_nsf2"], name
        if name in IS_LANE_EXCEPTIONS:
            assert (old["is_lane"], lane) == (1, 0), name
        else:
            assert lane == old["is_lane"], name
        for n in ic.ROWS:
            duo = lib.pmc_maf_inverse_auto_is_duo(C.byref(d), n)
            if name in IS_DUO_EXCEPTIONS:
                assert (old["is_duo"][str(n)], duo) == (1, 0), (name, n)
            else:
                assert duo == old["is_duo"][str(n)], (name, n)
        # the queries are the plan's answer for AUTO
        p = plan(lib, name, 17, AUTO)
        sweep = p["sweep"] if isinstance(p, dict) else S_NONE
        assert (lane, nsf2) == (int(sweep == S_LANE), int(sweep == S_NSF_DUO)), name
    assert lib.pmc_maf_inverse_auto_is_lane(None) == 0 and lib.pmc_maf_inverse_auto_is_nsf2(None) == 0
    assert lib.pmc_maf_inverse_auto_is_duo(None, 16) == 0


# ------------------------------------------------------------------------------------------------ (b) plans by hand
# The LDS formulas as the launchers of the parent commit wrote them (bytes), restated here on the layout fields.
def L(name):
    return ic.layout(name)


def lds_solo(name, maxo):
    m = L(name)
    return 4 * (2 * m["Dp"] * 16 + 2 * m["Hp"] * 16 + 3 * 256 + maxo * 256 + m["nT"] * 4 + 8)


def lds_duo(name, maxo):
    m = L(name)
    tt, yt = (m["nT"] + 2) * 16, m["T"] * ((m["nT"] + 2) * 4 + 1)
    table = ((tt + m["Dp"] + 2 * m["T"] + 3) & ~3) + m["Dp"] * 16 + ((yt + 3) & ~3)
    return 4 * (2 * m["Dp"] * 16 + 2 * m["Hp"] * 16 + 2 * 256 + 2 * (3 + maxo) * 256 + table)


def lds_lane(name, ns, hb=0):
    m = L(name)
    h = ((m["nT"] + 1) // 2) * 256 if hb else m["nT"] * 256
    x = m["Dp"] * 16 + ((m["nXT"] + 1) // 2) * 256 if hb else 2 * m["Dp"] * 16
    return 4 * (ns * (x + 3 * h) + 3 * 2 * ns * 16 * 20 + 2 * 2 * 16 * ns * 20) + (8 + 8) * 4


def lds_nsf_duo(name):
    m = L(name)
    words = (m["nT"] + 2) * 8 + m["Dp"] + m["T"] * ((m["nT"] + 2) * 4 + 1)
    base = 3 * m["Dp"] * 16 + 3 * m["Hp"] * 16 + 2 * 768 + 2 * 2048 + 16 * 32 + ((words + 3) & ~3)
    eager = 8 <= m["nT"] <= 11 and 4 * (base + 4096) <= 80 * 1024
    return 4 * (base + (4096 if eager else 0))


def lds_nsf_solo(name):
    m = L(name)
    return 4 * (2 * m["Dp"] * 16 + 3 * m["Hp"] * 16 + 16 * 32 + 16 * 24)


def lds_dense(name):
    m = L(name)
    return 4 * (3 * m["Dp"] * 16 + 3 * m["Hp"] * 16)


def lds_dpass_spline(name):
    m = L(name)
    return 4 * (3 * m["Dp"] * 16 + 3 * m["Hp"] * 16 + 16 * 8 + m["n_out"] * 256)


def P(sweep, lds, fused=0, epilogue=0, maxo=0, fm=0, subsets=0, waves=0, helper_fmt=0):
    return dict(sweep=sweep, fused=fused, epilogue=epilogue, maxo=maxo, fm=fm, subsets=subsets, waves=waves,
                helper_fmt=helper_fmt, lds_bytes=lds)


E_TRI = "pmc_maf_inverse: triangular sweep needs degree groups <= one tile"
E_BINS = "pmc_maf_inverse: the spline sweeps are built for 8 bins (PMC_INVERSE_NAIVE covers the others)"
E_NSF_DUO = "pmc_maf_inverse: the two-wave spline sweep needs D <= 64 and its tiles in 160 KiB of LDS"
E_NSF_ALGO = "pmc_maf_inverse: spline flows know PMC_INVERSE_TRIANGULAR (_SOLO, _DUO) and PMC_INVERSE_NAIVE"
E_NSF_WIDE = "pmc_maf_inverse: flow too wide for one wave's LDS budget (160 KiB)"
E_WG_WIDE = "pmc_maf_forward: flow too wide for 160 KB of LDS"
E_TILES = "pmc_maf_inverse: the triangular sweeps need their tiles in 160 KiB of LDS"
E_D64 = "pmc_maf_inverse: this sweep needs D <= 64 and its tiles in 160 KiB of LDS"
E_LANE16 = "pmc_maf_inverse: PMC_INVERSE_TRIANGULAR_LANE16 needs pmc_maf_t.lane16 (pmc_maf_pack_lane16)"
E_LANE = "pmc_maf_inverse: the lane-per-walker sweep needs an affine flow whose degree groups fit a tile"
E_DENSE = "MAF too wide for one wave's LDS budget (160 KiB)"
E_ALGO = "pmc_maf_inverse: unknown algo"
NOT_FUSED = P(S_NONE, 0)

# (case, rows, algo, fused) -> plan | message.  Order of precedence of AUTO / TRIANGULAR on an affine flow: lane if
# preferred (>= 16 hidden tiles; with a 16-bit image: the same bound) and covered; else duo if its LDS fits; else solo if
# nOT <= 8 and it fits; else lane if covered; else D-pass (AUTO) / error (TRIANGULAR).
EXPECT = [
    # ---- nOT <= 4, nT < 16: two waves, four output tiles in registers
    ("o4", 17, AUTO, 0, lambda: P(S_DUO, lds_duo("o4", 4), maxo=4)),
    ("o4", 8193, TRI, 0, lambda: P(S_DUO, lds_duo("o4", 4), maxo=4)),
    ("o4", 17, SOLO, 0, lambda: P(S_SOLO, lds_solo("o4", 4), maxo=4)),
    ("o4", 17, DUO, 0, lambda: P(S_DUO, lds_duo("o4", 4), maxo=4)),
    ("o4", 17, NAIVE, 0, lambda: P(S_DPASS_AFFINE, lds_dense("o4"))),
    ("o4", 17, LANE, 0, lambda: P(S_LANE, lds_lane("o4", 1), subsets=1, waves=4)),
    ("o4", 4097, LANE, 0, lambda: P(S_LANE, lds_lane("o4", 2), subsets=2, waves=4)),      # 4097 rows: 257 groups of 16
    ("o4", 8193, LANE, 0, lambda: P(S_LANE, lds_lane("o4", 4), subsets=4, waves=4)),      # 8193 rows: 257 groups of 32
    ("o4", 17, LANE16, 0, lambda: E_LANE16),
    ("o4", 17, 5, 0, lambda: E_ALGO),
    ("o4", 17, AUTO, 1, lambda: P(S_DUO, lds_duo("o4", 4), fused=1, epilogue=1, maxo=4, fm=4)),      # D = 10 <= 16
    ("o4", 17, TRI, 1, lambda: P(S_DUO, lds_duo("o4", 4), fused=1, epilogue=1, maxo=4, fm=4)),
    ("o4", 17, DUO, 1, lambda: NOT_FUSED),                # (the step fuses for AUTO / TRIANGULAR only)
    # ---- 4 < nOT <= 8, nT < 16
    ("o8_d33", 17, AUTO, 0, lambda: P(S_DUO, lds_duo("o8_d33", 8), maxo=8)),
    ("o8_d33", 17, AUTO, 1, lambda: P(S_DUO, lds_duo("o8_d33", 8), fused=1, epilogue=1, maxo=8, fm=16)),   # 32 < D
    ("o8_d33", 17, SOLO, 0, lambda: P(S_SOLO, lds_solo("o8_d33", 8), maxo=8)),
    ("o8_d60", 4097, AUTO, 0, lambda: P(S_DUO, lds_duo("o8_d60", 8), maxo=8)),
    ("o8_d64_hand", 17, AUTO, 0, lambda: P(S_DUO, lds_duo("o8_d64_hand", 8), maxo=8)),
    ("o8_d64_hand", 17, AUTO, 1, lambda: P(S_DUO, lds_duo("o8_d64_hand", 8), fused=1, epilogue=1, maxo=8, fm=16)),
    # ---- D <= 64 on both sides of 16 hidden tiles
    ("t15", 4097, AUTO, 0, lambda: P(S_DUO, lds_duo("t15", 8), maxo=8)),
    ("t15", 4097, AUTO, 1, lambda: P(S_DUO, lds_duo("t15", 8), fused=1, epilogue=1, maxo=8, fm=16)),
    ("t16", 17, AUTO, 0, lambda: P(S_LANE, lds_lane("t16", 1), subsets=1, waves=5)),
    ("t16", 4096, AUTO, 0, lambda: P(S_LANE, lds_lane("t16", 1), subsets=1, waves=5)),     # 256 workgroups: one round
    ("t16", 4097, TRI, 0, lambda: P(S_LANE, lds_lane("t16", 2), subsets=2, waves=5)),
    ("t16", 8193, AUTO, 0, lambda: P(S_LANE, lds_lane("t16", 2), subsets=2, waves=5)),     # five waves: two subsets at most
    ("t16", 17, AUTO, 1, lambda: NOT_FUSED),
    ("t16", 17, DUO, 0, lambda: P(S_DUO, lds_duo("t16", 8), maxo=8)),
    ("t16", 17, LANE16, 0, lambda: E_LANE16),
    # ---- D > 64
    ("d65_t15_hand", 17, AUTO, 0, lambda: P(S_LANE, lds_lane("d65_t15_hand", 1), subsets=1, waves=4)),
    ("d65_t15_hand", 8193, AUTO, 0, lambda: P(S_LANE, lds_lane("d65_t15_hand", 2), subsets=2, waves=4)),   # (four subsets: 276 KB)
    ("d65_t15_hand", 17, AUTO, 1, lambda: NOT_FUSED),
    ("d65_t16", 4097, AUTO, 0, lambda: P(S_LANE, lds_lane("d65_t16", 2), subsets=2, waves=5)),
    ("d65_t16", 17, SOLO, 0, lambda: E_D64),
    ("d65_t16", 17, DUO, 0, lambda: E_D64),
    ("d65_t16", 17, AUTO, 1, lambda: NOT_FUSED),
    # ---- the lane sweep's limits: LDS (float32: 45 tiles) and 64 tiles
    ("t45_d66", 8193, AUTO, 0, lambda: P(S_LANE, lds_lane("t45_d66", 1), subsets=1, waves=5)),
    ("t46_d66", 17, AUTO, 0, lambda: P(S_DPASS_AFFINE, lds_dense("t46_d66"))),
    ("t46_d66", 17, TRI, 0, lambda: E_TILES),
    ("t46_d66", 17, LANE, 0, lambda: E_LANE),
    ("t64_d66", 17, AUTO, 0, lambda: E_DENSE),
    ("t64_d66", 17, NAIVE, 0, lambda: E_DENSE),
    ("t65_d66", 17, LANE, 0, lambda: E_LANE),
    ("t65_d66", 17, TRI, 0, lambda: E_TILES),
    ("t64_d66_bf16", 8193, AUTO, 0, lambda: P(S_LANE, lds_lane("t64_d66_bf16", 1, 1), subsets=1, waves=4, helper_fmt=1)),
    ("t64_d66_bf16", 17, LANE, 0, lambda: E_LANE),        # (float32 helpers: beyond the LDS)
    ("t65_d66_bf16", 17, LANE16, 0, lambda: E_LANE),
    ("t65_d66_bf16", 17, AUTO, 0, lambda: E_DENSE),
    # ---- degree groups wider than a tile
    ("tri_no", 17, AUTO, 0, lambda: P(S_DPASS_AFFINE, lds_dense("tri_no"))),
    ("tri_no", 17, AUTO, 1, lambda: NOT_FUSED),
    ("tri_no", 17, TRI, 0, lambda: E_TRI),
    ("tri_no", 17, SOLO, 0, lambda: E_TRI),
    ("tri_no", 17, DUO, 0, lambda: E_TRI),
    ("tri_no", 17, LANE, 0, lambda: E_LANE),
    # ---- 16-bit helper images
    ("t15_bf16", 17, AUTO, 0, lambda: P(S_DUO, lds_duo("t15", 8), maxo=8)),
    ("t15_f16", 17, AUTO, 1, lambda: P(S_DUO, lds_duo("t15", 8), fused=1, epilogue=1, maxo=8, fm=16)),
    ("t15_f16", 17, LANE16, 0, lambda: P(S_LANE, lds_lane("t15", 1, 2), subsets=1, waves=4, helper_fmt=2)),
    ("t16_bf16", 17, AUTO, 0, lambda: P(S_LANE, lds_lane("t16", 1, 1), subsets=1, waves=4, helper_fmt=1)),
    ("t16_f16", 8193, AUTO, 0, lambda: P(S_LANE, lds_lane("t16", 2, 2), subsets=2, waves=4, helper_fmt=2)),   # (four subsets: 174 KB)
    ("t16_bf16", 4097, LANE16, 0, lambda: P(S_LANE, lds_lane("t16", 2, 1), subsets=2, waves=4, helper_fmt=1)),
    ("t16_bf16", 4097, LANE, 0, lambda: P(S_LANE, lds_lane("t16", 2), subsets=2, waves=5)),        # LANE strips the image
    ("t16_bf16", 17, AUTO, 1, lambda: NOT_FUSED),
    # ---- PMC_MAF_VARIANT_LANE_FOUR: no fifth wavefront, and with it no preference for the lane sweep
    ("t16_four", 17, AUTO, 0, lambda: P(S_DUO, lds_duo("t16", 8), maxo=8)),
    ("t16_four", 8193, LANE, 0, lambda: P(S_LANE, lds_lane("t16", 2), subsets=2, waves=4)),       # (four subsets: 280 KB)
    ("t16_four", 17, AUTO, 1, lambda: P(S_DUO, lds_duo("t16", 8), fused=1, epilogue=1, maxo=8, fm=16)),
    # ---- spline flows, 8 bins
    ("nsf_d1_hand", 17, AUTO, 0, lambda: P(S_NSF_SOLO, lds_nsf_solo("nsf_d1_hand"))),
    ("nsf_d1_hand", 17, AUTO, 1, lambda: NOT_FUSED),
    ("nsf_d2", 17, AUTO, 0, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_d2"))),
    # (the epilogue's scratch, (2 * 16 * 2 + 2 * 17) * 8 + 64 = 848 bytes, aliases 3 * Hp * 16 * 4 = 3072 bytes)
    ("nsf_d2", 17, AUTO, 1, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_d2"), fused=1, epilogue=1, fm=4)),
    ("nsf_d2", 17, SOLO, 0, lambda: P(S_NSF_SOLO, lds_nsf_solo("nsf_d2"))),
    ("nsf_d2", 17, DUO, 0, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_d2"))),
    ("nsf_d2", 17, NAIVE, 0, lambda: P(S_DPASS_SPLINE, lds_dpass_spline("nsf_d2"))),
    ("nsf_d2", 17, LANE, 0, lambda: E_NSF_ALGO),
    ("nsf_d2", 17, LANE16, 0, lambda: E_NSF_ALGO),
    ("nsf_d64", 8193, TRI, 0, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_d64"))),
    ("nsf_d64", 17, AUTO, 1, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_d64"), fused=1, epilogue=1, fm=16)),
    ("nsf_d65", 17, AUTO, 0, lambda: P(S_NSF_SOLO, lds_nsf_solo("nsf_d65"))),
    ("nsf_d65", 17, DUO, 0, lambda: E_NSF_DUO),
    ("nsf_d65", 17, AUTO, 1, lambda: NOT_FUSED),
    ("nsf_tri_no", 17, AUTO, 0, lambda: P(S_DPASS_SPLINE, lds_dpass_spline("nsf_tri_no"))),
    ("nsf_tri_no", 17, TRI, 0, lambda: E_TRI),
    ("nsf_wide_hand", 17, AUTO, 0, lambda: E_NSF_WIDE),
    ("nsf_wide_hand", 17, SOLO, 0, lambda: E_NSF_WIDE),
    ("nsf_wide_hand", 17, NAIVE, 0, lambda: E_WG_WIDE),
    # ---- spline flows, 4 and 16 bins: zuko's D-pass algorithm
    ("nsf_bins4", 17, AUTO, 0, lambda: P(S_DPASS_SPLINE, lds_dpass_spline("nsf_bins4"))),
    ("nsf_bins4", 17, TRI, 0, lambda: E_BINS),
    ("nsf_bins4", 17, AUTO, 1, lambda: NOT_FUSED),
    ("nsf_bins16", 17, AUTO, 0, lambda: P(S_DPASS_SPLINE, lds_dpass_spline("nsf_bins16"))),
    ("nsf_bins16", 17, SOLO, 0, lambda: E_BINS),
    # ---- two-wave tables beyond 160 KiB, lone-wave layout within (70 tiles: beyond the lane sweep's 64 as well)
    ("duo_big_hand", 17, AUTO, 0, lambda: P(S_SOLO, lds_solo("duo_big_hand", 4), maxo=4)),
    ("duo_big_hand", 17, DUO, 0, lambda: E_D64),
    ("duo_big_hand", 17, AUTO, 1, lambda: P(S_SOLO, lds_solo("duo_big_hand", 4), fused=1, epilogue=1, maxo=4, fm=4)),
    # ---- a fused instance without the epilogue: D = 10 on ONE hidden tile.  The scaler's scratch is
    #      (2 * 16 * 10 + 17 * 10) * 8 + 64 = 3984 bytes; the affine sweeps lend it two activation arrays of Hp * 16 floats
    #      = 2 * 16 * 16 * 4 = 2048 bytes, the spline sweep three = 3072 bytes: the scaler stays a launch of its own
    ("epi_no_hand", 17, AUTO, 0, lambda: P(S_DUO, lds_duo("epi_no_hand", 4), maxo=4)),
    ("epi_no_hand", 17, AUTO, 1, lambda: P(S_DUO, lds_duo("epi_no_hand", 4), fused=1, epilogue=0, maxo=4, fm=4)),
    ("epi_no_hand", 17, TRI, 1, lambda: P(S_DUO, lds_duo("epi_no_hand", 4), fused=1, epilogue=0, maxo=4, fm=4)),
    ("nsf_epi_no_hand", 17, AUTO, 0, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_epi_no_hand"))),
    ("nsf_epi_no_hand", 17, AUTO, 1, lambda: P(S_NSF_DUO, lds_nsf_duo("nsf_epi_no_hand"), fused=1, epilogue=0, fm=4)),
]


@pytest.mark.parametrize("case,n,algo,fused,expect", EXPECT, ids=[f"{c}-n{n}-algo{a}-{'fused' if f else 'plain'}" for c, n, a, f, _ in EXPECT])
def test_plan_is_the_one_written_by_hand(lib, case, n, algo, fused, expect):
    assert plan(lib, case, n, algo, fused) == expect()


def test_hand_table_covers_every_case_algo_and_sweep():
    assert {c for c, *_ in EXPECT} == set(ic.CASES)
    assert {a for _, _, a, _, _ in EXPECT} >= set(ALGOS)
    sweeps = {e()["sweep"] for *_, e in EXPECT if isinstance(e(), dict)}
    assert sweeps == set(range(8))
    assert lds_duo("duo_big_hand", 4) > CAP >= lds_solo("duo_big_hand", 4)
    assert lds_lane("t46_d66", 1) > CAP >= lds_lane("t45_d66", 1)


def test_fused_epilogue_needs_its_scratch_in_the_activation_arrays(lib):
    """The scaler's scratch ((2 * 16 * D + 17 * D) * 8 + 64 bytes) aliases the sweep's activation arrays: two of Hp * 16
    floats in the affine sweeps, three in the spline sweep.  Over every case with a fused instance the epilogue is there
    exactly when that fits (D = 10 on one tile: 3984 > 2048 / 3072 bytes, no epilogue; D = 64 on 15 / 17 tiles: 25152 <=
    30720 / 52224, an epilogue), and both answers occur for both kinds of flow."""
    seen = set()
    for name in ic.CASES:
        m, p = L(name), plan(lib, name, 17, AUTO, 1)
        if p["sweep"] == S_NONE:
            assert p["epilogue"] == 0, name
            continue
        arrays = 3 if p["sweep"] == S_NSF_DUO else 2
        fits = (2 * 16 * m["D"] + 17 * m["D"]) * 8 + 64 <= arrays * m["Hp"] * 16 * 4
        assert p["epilogue"] == int(fits), name
        seen.add((p["sweep"] == S_NSF_DUO, fits))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


# ------------------------------------------------------------------------------------------------ (c) the whole grid
def test_grid_invariants(lib):
    seen = set()
    for name in ic.CASES:
        D = L(name)["D"]
        for n in ic.ROWS:
            for algo in ALGOS:
                for fused in (0, 1):
                    p = plan(lib, name, n, algo, fused)
                    if fused:
                        assert isinstance(p, dict), (name, n, algo)       # "no fused instance" is not an error
                    if not isinstance(p, dict):
                        assert p.startswith(("pmc_maf_inverse: ", "pmc_maf_forward: ", "MAF too wide")), p
                        continue
                    key = (name, n, algo, fused)
                    seen.add(p["sweep"])
                    assert 0 <= p["lds_bytes"] <= CAP, key
                    assert p["fused"] == (1 if fused and p["sweep"] != S_NONE else 0), key
                    if not fused:
                        assert p["sweep"] != S_NONE and p["lds_bytes"] > 0, key
                    if p["waves"] == 5:
                        assert p["helper_fmt"] == 0 and not p["fused"] and p["subsets"] <= 2, key
                    if p["helper_fmt"]:
                        assert p["sweep"] == S_LANE and not p["fused"], key
                    if p["fused"]:
                        assert D <= 64 and p["fm"] == (4 if D <= 16 else 8 if D <= 32 else 16), key
                    else:
                        assert p["fm"] == 0 and p["epilogue"] == 0, key
                    assert (p["sweep"] == S_LANE) == (p["subsets"] in (1, 2, 4)) == (p["waves"] in (4, 5)), key
                    assert (p["sweep"] in (S_SOLO, S_DUO)) == (p["maxo"] in (4, 8)), key
    assert seen == set(range(8))
