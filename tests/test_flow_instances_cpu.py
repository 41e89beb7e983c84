"""The census of the float32 flow kernels' instances (``tests/flow_instances.py``): every instance the launchers can reach is
launched by a case of the suite, and the 4- and 16-bin default-width flows take -- or are refused -- exactly what the LDS
formulas say.  Layout fields and host code only: no GPU."""
import os
import re

import pytest

import flow_instances as fi
from flow_instances import CASES, FULL, LEAN, instances
from pocomc_amd.maf_spec import MAFSpec
from test_wide_default_plan_cpu import CAP, DS, full_train, full_wg, lean_train, lean_wg, span

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pocomc_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------- the census
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{c.group}-{'-'.join(map(str, c.spec))}-n{c.n}-{fi._kind(c.lean)}" for c in CASES])
def test_a_case_reaches_the_instances_it_claims(lib, i):
    c = CASES[i]
    got = instances(lib, c.spec, c.n, c.lean)
    assert c.reaches and {k: got[k] for k in c.reaches} == c.reaches


def test_every_case_names_a_test_that_exists():
    for c in CASES:
        path, name = (fi.NEW, c.test) if c.group != "suite" else c.test.split("::")
        assert (c.group == "suite") == ("::" in c.test)
        with open(os.path.join(ROOT, path)) as fh:
            assert re.search(rf"^def {name}\(", fh.read(), re.M), (path, name)


def test_the_cases_launch_every_instance():
    reached = {"forward": set(), "dpass": set(), "train": set()}
    for c in CASES:
        for k, v in c.reaches.items():
            if k in reached and not isinstance(v, str):
                reached[k].add(v[:3])                                   # (the trainer's ksplit is not a template argument)
    assert fi.ALL_FORWARD - reached["forward"] == set()
    assert fi.ALL_DPASS - reached["dpass"] == set()
    assert fi.ALL_TRAIN - reached["train"] == set()
    # ... and nothing that does not exist: the affine flows' full D-pass is the lone-wave kernel, no eight-wave affine trainer
    assert reached["forward"] == fi.ALL_FORWARD and reached["dpass"] == fi.ALL_DPASS and reached["train"] == fi.ALL_TRAIN
    assert len(fi.ALL_FORWARD) == 16 and len(fi.ALL_DPASS) == 7 and len(fi.ALL_TRAIN) == 14


def test_the_new_cases_alone_launch_every_forward_and_dpass_instance():
    """Only the sixteen-wave 8-bin trainer is left to a test the suite had before."""
    new = [c for c in CASES if c.group != "suite"]
    assert {c.reaches["forward"] for c in new if not isinstance(c.reaches.get("forward", ""), str)} == fi.ALL_FORWARD
    assert {c.reaches["dpass"] for c in new if not isinstance(c.reaches.get("dpass", ""), str)} == fi.ALL_DPASS
    assert fi.ALL_TRAIN - {c.reaches["train"][:3] for c in new if not isinstance(c.reaches.get("train", ""), str)} == {(16, 8, FULL), (16, 8, LEAN)}


def test_four_wavefronts_from_16385_rows(lib):
    for n, nw in ((1, 8), (16384, 8), (16385, 4), (fi.BIG, 4)):
        assert instances(lib, ("maf3", 10), n)["forward"] == (nw, 0, FULL)


def test_the_sixteen_wave_flows_of_section_b_are_sixteen_wave(lib):
    import ctypes as C
    for s, waves in zip(fi.B_FLOWS, (8, 8, 16, 16, 16, 8)):
        assert lib.pmc_maf_train_waves(C.byref(fi.descriptor(fi.make_spec(s)))) == waves


# ---------------------------------------------------------- 4 and 16 bins at default width: lean, full, refused
# recomputed from the launchers' byte counts (tests/test_wide_default_plan_cpu.py: full_wg, full_train, lean_wg,
# lean_train), T = 2, H = 512 from D = 86; nothing below 86 is lean but the 16-bin trainer at D = 52 (H = 256, Hp = 416)
TABLE = {
    (4, "forward"): dict(lean=span((92, 112)), refused=set()),
    (4, "dpass"): dict(lean=span((88, 116)), refused=set()),
    (4, "train"): dict(lean=span((86, 128), (130, 157)), refused=set()),
    (16, "forward"): dict(lean=span((86, 99), (107, 157)), refused=span((100, 106))),
    (16, "dpass"): dict(lean=span((86, 95), (112, 157)), refused=span((96, 111))),
    (16, "train"): dict(lean=span((52, 52), (86, 97), (108, 157)), refused=span((98, 107))),
}
MESSAGE = {"forward": fi.REFUSED_FORWARD, "dpass": fi.REFUSED_FORWARD, "train": fi.REFUSED_TRAIN}


@pytest.mark.parametrize("bins", [4, 16])
def test_lean_full_and_refused_ranges_at_4_and_16_bins(lib, bins):
    seen = {call: dict(lean=set(), refused=set()) for call in ("forward", "dpass", "train")}
    for D in DS:
        s = MAFSpec(D, 2, univariate="rqs", bins=bins)
        assert s.n_out == 3 * bins - 1 and (s.hidden == 512) == (D >= 86)
        full = {"forward": full_wg(s, 0), "dpass": full_wg(s, 1), "train": full_train(s)}
        want = {}
        for call in seen:
            if full[call] <= CAP:
                want[call] = (0, full[call])
                continue
            lean = lean_wg(s, call == "dpass") if call != "train" else lean_train(s)    # (a full plan beyond the LDS has no partial-tile staging)
            want[call] = (1, lean) if lean <= CAP else (-1, full[call])
            seen[call]["lean" if lean <= CAP else "refused"].add(D)
        err, p = fi.lds_plan(lib, s)
        for call in seen:
            assert p[call + "_full_bytes"] == full[call], (D, call)
            assert (p[call + "_lean"], p[call + "_lds_bytes"]) == want[call], (D, call)
        # the first refusal in the launchers' order is the message
        refused = [call for call in ("forward", "dpass", "train") if want[call][0] < 0]
        assert err == (MESSAGE[refused[0]] if refused else None), D
        # the inverse: the triangular sweeps are built for 8 bins, so AUTO is the D-pass algorithm -- the full instance,
        # the lean one (PMC_SWEEP_DPASS_LEAN), or the forward launcher's refusal
        sweep = {0: "dpass_spline", 1: "dpass_lean", -1: fi.REFUSED_FORWARD}[want["dpass"][0]]
        got = instances(lib, s, 33)
        assert got["auto"] == sweep, D
        assert got["dpass"] == ((bins, LEAN if want["dpass"][0] else FULL) if want["dpass"][0] >= 0 else fi.REFUSED_FORWARD), D
        assert got["forward"] == ((8, bins, LEAN if want["forward"][0] else FULL) if want["forward"][0] >= 0 else fi.REFUSED_FORWARD), D
        assert (got["train"] == fi.REFUSED_TRAIN) == (want["train"][0] < 0), D
        for algo in (fi.AUTO, fi.NAIVE):
            q = fi.inverse_plan(lib, s, algo, 33)
            if want["dpass"][0] < 0:
                assert q == fi.REFUSED_FORWARD, (D, algo)
            else:
                assert (q["sweep"], q["lds_bytes"]) == (8 if want["dpass"][0] else 2, want["dpass"][1]), (D, algo)
    for call in seen:
        assert seen[call] == TABLE[(bins, call)], call


def test_where_a_16_bin_flow_of_default_width_runs_nothing_but_lean_instances():
    """Every kernel lean and nothing refused: 4 bins at D = 92 - 112, 16 bins at D = 86 - 95 and 112 - 157 -- the ends are
    the GPU cases' widths (``flow_instances.D_FLOWS``); refused in some call: 16 bins at D = 96 - 111."""
    def all_lean(b):
        return set.intersection(*(TABLE[(b, c)]["lean"] for c in ("forward", "dpass", "train")))
    assert all_lean(4) == span((92, 112)) and all_lean(16) == span((86, 95), (112, 157))
    assert set.union(*(TABLE[(16, c)]["refused"] for c in ("forward", "dpass", "train"))) == span((96, 111))
    assert {s[0] for s in fi.D_FLOWS if s[4] == 4} == {92, 112} and {s[0] for s in fi.D_FLOWS if s[4] == 16} == {86, 95, 112}
    assert {s[0] for s in fi.D_REFUSED} <= set.intersection(*(TABLE[(16, c)]["refused"] for c in ("forward", "dpass", "train")))


@pytest.mark.parametrize("D", [96, 100, 104, 111])
def test_the_16_bin_refusals_carry_the_launchers_messages(lib, D):
    """Not a fall-through to another kernel, and not a plan with a size nobody can launch: the call's own message, and -1
    for the refused calls only."""
    s = MAFSpec(D, 2, univariate="rqs", bins=16)
    err, p = fi.lds_plan(lib, s)
    got = instances(lib, s, 33)
    assert got["dpass"] == got["auto"] == "pmc_maf_forward: flow too wide for 160 KB of LDS"
    assert (got["forward"] == "pmc_maf_forward: flow too wide for 160 KB of LDS") == (100 <= D <= 106) == (p["forward_lean"] == -1)
    assert (got["train"] == "pmc_maf_loss_grad: flow too wide for the 160 KB LDS of one workgroup") == (98 <= D <= 107) == (p["train_lean"] == -1)
    assert p["dpass_lean"] == -1 and err == "pmc_maf_forward: flow too wide for 160 KB of LDS"
    # forcing the lean instances changes no refusal: they are what was refused
    assert instances(lib, s, 33, lean_forced=True) == got
