"""Which instance of the float32 flow kernels a call takes, and the table of calls that launches every one of them
(``tests/test_flow_instances_cpu.py``, ``tests/test_gpu_flow_instances.py``).

The kernels are templates: ``maf_forward_wg_kernel<NW, UNI, MODE, LEAN>`` (``csrc/maf_forward_wg.hip``: wavefronts per row
set, univariate map -- 0 affine, else the spline's bins --, forward / D-pass inverse, two hidden-width arrays instead of
three) and ``maf_chain_kernel<NW, PF, PROF, UNI, LEAN>`` (``csrc/maf_train.hip``: the trainer).  Host code picks the
instance from the flow's layout and the row count; ``instances`` restates that choice from what the library reports on
the CPU (``pmc_maf_lds_plan``, ``pmc_maf_inverse_plan``, ``pmc_maf_train_waves``), and ``CASES`` lists, per instance, a call
of the suite that launches it: the new GPU cases of ``tests/test_gpu_flow_instances.py`` and, for the instances the suite
reached before, the test that does."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from pocomc_amd.maf_spec import MAFSpec, spec_by_name

CAP = 160 * 1024
AUTO, NAIVE = 0, 2                         # PMC_INVERSE_AUTO, PMC_INVERSE_NAIVE
LEAN_BIT = 8                               # PMC_MAF_VARIANT_LEAN_LDS
SWEEPS = {1: "dpass_affine", 2: "dpass_spline", 3: "solo", 4: "duo", 5: "lane", 6: "nsf_solo", 7: "nsf_duo", 8: "dpass_lean"}
FULL, LEAN = "full", "lean"
NW_ROWS = 16 * 1024                        # the largest call that takes eight wavefronts per row set


def make_spec(s):
    """``("maf3", D)`` / ``("nsf3", D)``: a named flow; ``(D, T, H, univariate, bins)``: a ``MAFSpec``."""
    if isinstance(s, MAFSpec):
        return s
    if isinstance(s[0], str):
        return spec_by_name(s[1], s[0])
    D, T, H, uni, bins = s
    return MAFSpec(D, T, H, univariate=uni, bins=bins)


def uni_of(spec):
    return 0 if spec.univariate == "affine" else spec.bins


def descriptor(s, reserved=0):             # as tests/test_wide_default_plan_cpu.py builds it: layout fields only, no GPU
    from pocomc_amd import _lib
    return _lib.pmc_maf_t(packed=None, meta=None, D=s.n_dim, H=s.hidden, T=s.n_transforms, Hp=s.Hp, Dp=s.Dp, nT=s.nT,
                          nXT=s.nXT, nOT=s.nOT, pk_per_transform=s.pk_per_transform, tri_ok=int(s.tri_ok), n_out=s.n_out,
                          lane16=None, lane16_fmt=0, reserved=reserved)


def lds_plan(lib, s, reserved=0):
    from pocomc_amd import _lib
    d, p = descriptor(s, reserved), _lib.pmc_flow_lds_plan_t()
    rc = lib.pmc_maf_lds_plan(C.byref(d), C.byref(p))
    return (lib.pmc_last_error().decode() if rc else None), {k: getattr(p, k) for k, _ in p._fields_}


def inverse_plan(lib, s, algo, n, reserved=0):
    from pocomc_amd import _lib
    d, p = descriptor(s, reserved), _lib.pmc_inverse_plan_t()
    if lib.pmc_maf_inverse_plan(C.byref(d), n, algo, 0, C.byref(p)):
        return lib.pmc_last_error().decode()
    return {k: getattr(p, k) for k, _ in p._fields_}


def train_ksplit(s):
    """The trainer's partial-tile staging is on where the FULL plan with it stays within 64 KiB (``pmc_train_instance``,
    ``csrc/maf_train.hip``; the ABI reports the bytes, not the switch).  ``test_wide_default_plan_cpu.full_train`` pins the
    reported bytes to the same formula."""
    own = s.n_out * 256 if s.n_out != 2 else s.Dp * 16
    return 4 * (4 * s.Hp * 16 + own + 2 * s.Dp * 16 + 16 + 16 * 16 + 16 * 256) <= 64 * 1024


def instances(lib, spec, n, lean_forced=False):
    """The instances a call of ``n`` rows on the flow ``spec`` takes:

    * ``forward``: ``(NW, UNI, "full" | "lean")`` of ``forward`` / ``log_prob``;
    * ``dpass``: ``(UNI, "full" | "lean")`` of the D-pass algorithm (``inverse_algo = 2``) where it runs the workgroup
      kernel, ``"dpass_affine"`` where the affine flows' lone-wave D-pass kernel runs;
    * ``auto``: the name of the sweep ``inverse_algo = 0`` takes (``SWEEPS``);
    * ``train``: ``(waves, UNI, "full" | "lean", ksplit)`` of ``loss_and_grad``.

    A call the library refuses has the refusal's message in place of the instance."""
    spec = make_spec(spec)
    reserved = LEAN_BIT if lean_forced else 0
    uni = uni_of(spec)
    err, p = lds_plan(lib, spec, reserved)
    # csrc/maf_forward_wg.hip, pmc_launch_forward_wg: "wide = n <= 16 * 1024" -> eight wavefronts, else four.  The ABI does
    # not report NW: this line is the one restatement of that rule.  (The plan's bytes are those of eight wavefronts; four
    # have 16 floats less per wavefront in the reduction array.)
    nw = 4 if n > NW_ROWS else 8
    out = {}
    full_bytes = p["forward_full_bytes"] - 4 * 16 * (8 - nw)
    fwd_lean = lean_forced or full_bytes > CAP
    fwd_bytes = full_bytes - (4 * spec.Hp * 16 if fwd_lean else 0)
    out["forward"] = (nw, uni, LEAN if fwd_lean else FULL) if fwd_bytes <= CAP else "pmc_maf_forward: flow too wide for 160 KB of LDS"
    if nw == 8:
        assert (p["forward_lean"] < 0) == isinstance(out["forward"], str) and (p["forward_lean"] < 0 or p["forward_lean"] == int(fwd_lean))
    q = inverse_plan(lib, spec, NAIVE, n, reserved)
    if isinstance(q, str):
        out["dpass"] = q
    elif q["sweep"] == 1:
        out["dpass"] = SWEEPS[1]
    else:
        assert q["sweep"] in (2, 8), q
        out["dpass"] = (uni, LEAN if q["sweep"] == 8 else FULL)
    q = inverse_plan(lib, spec, AUTO, n, reserved)
    out["auto"] = q if isinstance(q, str) else SWEEPS[q["sweep"]]
    if p["train_lean"] < 0:
        out["train"] = "pmc_maf_loss_grad: flow too wide for the 160 KB LDS of one workgroup"
    else:
        out["train"] = (int(lib.pmc_maf_train_waves(C.byref(descriptor(spec, reserved)))), uni, LEAN if p["train_lean"] else FULL,
                        train_ksplit(spec))
    return out


# ------------------------------------------------------------------------------------------------------- the cases
# group: the section of tests/test_gpu_flow_instances.py ("a" .. "e"), or "suite": a test the suite had before, named in
# ``test`` as "file::function" -- the census counts both kinds.  ``reaches``: the instances the call is meant to launch,
# in the words of ``instances``; what a row does not run (the wide forward cases train nothing) it does not claim.
Case = namedtuple("Case", "group spec n lean reaches test")
NEW = "tests/test_gpu_flow_instances.py"
BIG = NW_ROWS + 7                          # 16391 rows: four wavefronts, and a last row set of 7 rows

A_FLOWS = (("maf3", 10), ("nsf3", 10), (10, 2, None, "rqs", 4), (10, 2, None, "rqs", 16))
B_FLOWS = ((10, 2, 64, "rqs", 4), (10, 2, 64, "rqs", 16), (20, 2, 128, "rqs", 4), (20, 2, 128, "rqs", 16),
           (10, 1, None, "affine", 8), (10, 1, None, "rqs", 8))
C_FLOWS = (("maf3", 10), ("nsf3", 10))
C_ROWS = 64 * 16 * 2 + 37                  # tests/test_gpu_train.py::test_large_batch_loops_over_row_sets
D_FLOWS = ((92, 2, None, "rqs", 4), (112, 2, None, "rqs", 4), (86, 2, None, "rqs", 16), (95, 2, None, "rqs", 16),
           (112, 2, None, "rqs", 16))
D_REFUSED = ((100, 2, None, "rqs", 16), (104, 2, None, "rqs", 16))
E_FLOWS = ((102, 2, None, "affine", 8), (102, 2, None, "rqs", 8))
REFUSED_FORWARD = "pmc_maf_forward: flow too wide for 160 KB of LDS"
REFUSED_TRAIN = "pmc_maf_loss_grad: flow too wide for the 160 KB LDS of one workgroup"


def _kind(lean):
    return LEAN if lean else FULL


def _cases():
    rows = []
    # (a) one call of BIG rows: four wavefronts; the same rows as 16384 + 7: eight
    for s in A_FLOWS:
        u = uni_of(make_spec(s))
        for lean in (False, True):
            rows.append(Case("a", s, BIG, lean, {"forward": (4, u, _kind(lean))}, "test_four_waves_give_what_eight_give"))
            rows.append(Case("a", s, NW_ROWS, lean, {"forward": (8, u, _kind(lean))}, "test_four_waves_give_what_eight_give"))
    # (b) forced lean against full on small flows: eight- and sixteen-wave trainers at 4 and 16 bins, one transform
    waves = {B_FLOWS[0]: 8, B_FLOWS[1]: 8, B_FLOWS[2]: 16, B_FLOWS[3]: 16, B_FLOWS[4]: 16, B_FLOWS[5]: 8}
    ksplit = {B_FLOWS[0]: True, B_FLOWS[1]: False, B_FLOWS[2]: False, B_FLOWS[3]: False, B_FLOWS[4]: True, B_FLOWS[5]: True}
    for s in B_FLOWS:
        u = uni_of(make_spec(s))
        for lean in (False, True):
            dpass = SWEEPS[1] if (u == 0 and not lean) else (u, _kind(lean))
            rows.append(Case("b", s, 40, lean, {"forward": (8, u, _kind(lean)), "dpass": dpass,
                                                "train": (waves[s], u, _kind(lean), ksplit[s])},
                             "test_forced_lean_equals_full_bit_for_bit"))
    # (c) the lean trainer over several row-set chunks and through a row index
    rows.append(Case("c", C_FLOWS[0], C_ROWS, True, {"train": (16, 0, LEAN, True)}, "test_lean_trainer_in_chunks_and_through_an_index"))
    rows.append(Case("c", C_FLOWS[1], C_ROWS, True, {"train": (8, 8, LEAN, True)}, "test_lean_trainer_in_chunks_and_through_an_index"))
    # (d) default-width 4- and 16-bin flows: every kernel lean, the inverse the D-pass fallback
    for s in D_FLOWS:
        u = s[4]
        rows.append(Case("d", s, 33, False, {"forward": (8, u, LEAN), "dpass": (u, LEAN), "auto": "dpass_lean"},
                         "test_wide_forward_and_log_prob_match_the_oracle"))
        rows.append(Case("d", s, 40, False, {"train": (16, u, LEAN, False)}, "test_wide_loss_and_gradient_match_autograd"))
    rows.append(Case("d", D_REFUSED[0], 33, False, {"forward": REFUSED_FORWARD, "dpass": REFUSED_FORWARD, "auto": REFUSED_FORWARD,
                                                    "train": REFUSED_TRAIN}, "test_refused_widths_raise_the_launchers_errors"))
    rows.append(Case("d", D_REFUSED[1], 33, False, {"forward": REFUSED_FORWARD, "dpass": REFUSED_FORWARD, "auto": REFUSED_FORWARD,
                                                    "train": REFUSED_TRAIN}, "test_refused_widths_raise_the_launchers_errors"))
    # (e) the D-pass fallback at the edge rows
    for s in E_FLOWS:
        u = uni_of(make_spec(s))
        rows.append(Case("e", s, 33, False, {"forward": (8, u, LEAN), "auto": "dpass_lean"}, "test_non_finite_rows_stay_in_their_rows_at_102_dimensions"))
    # the sixteen-wave 8-bin trainer, full and lean: reached before this table existed
    for lean in (False, True):
        rows.append(Case("suite", ("nsf3", 32), 40, lean, {"train": (16, 8, _kind(lean), False)},
                         "tests/test_gpu_wide_default_flows.py::test_forced_lean_instances_equal_the_full_ones_bit_for_bit"))
    return tuple(rows)


CASES = _cases()

# every instance the launchers can reach
ALL_FORWARD = {(nw, u, k) for nw in (4, 8) for u in (0, 4, 8, 16) for k in (FULL, LEAN)}
ALL_DPASS = {(u, k) for u in (4, 8, 16) for k in (FULL, LEAN)} | {(0, LEAN)}     # (affine, full: the lone-wave kernel's)
ALL_TRAIN = {(16, u, k) for u in (0, 4, 8, 16) for k in (FULL, LEAN)} | {(8, u, k) for u in (4, 8, 16) for k in (FULL, LEAN)}
