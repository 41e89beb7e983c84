"""Flow layouts for the inverse-plan tests (``tests/test_inverse_plan_cpu.py``, ``tests/test_gpu_inverse_plan.py``): the
smallest flow in every class the plan of ``csrc/inverse_plan.hip`` tells apart, and the recorder of the parent commit's
answers (``python tests/inverse_plan_cases.py LIBRARY COMMIT`` writes ``tests/golden/inverse_queries_parent.json``).

A case is ``(spec arguments | hand-made layout, lane16_fmt, reserved bits)``.  ``MAFSpec`` pads every degree group to a
quad, so D features give at least ``ceil((D - 1) / 4)`` hidden tiles, and it keeps ``tri_ok`` only up to 16 units per
degree: the classes it cannot produce (D >= 64 with fewer than 16 tiles, a spline flow with D = 1, a D <= 64 flow of
more than 64 tiles) are layouts written by hand -- the plan reads the layout fields and follows no pointer."""
import ctypes as C
import json
import os
import sys

ROWS = (1, 16, 17, 4096, 4097, 8192, 8193)
LANE_FOUR = 2                                     # PMC_MAF_VARIANT_LANE_FOUR


def spec(D, hidden=None, uni="affine", bins=8, T=3):
    return dict(kind="spec", D=D, hidden=hidden, uni=uni, bins=bins, T=T)


def hand(D, nT, n_out=2, tri_ok=1, T=3):
    return dict(kind="hand", D=D, nT=nT, n_out=n_out, tri_ok=tri_ok, T=T)


#        name              layout                         lane16_fmt  reserved
CASES = {
    "o4":            (spec(10),                           0, 0),      # nOT = 2, nT = 3
    "o8_d33":        (spec(33),                           0, 0),      # nOT = 6, nT = 8
    "o8_d60":        (spec(60, 59),                       0, 0),      # nOT = 8, nT = 15
    "o8_d64_hand":   (hand(64, 15),                       0, 0),      # nOT = 8, nT = 15 (MAFSpec: D = 64 has >= 16 tiles)
    "t15":           (spec(50, 204),                      0, 0),      # D <= 64, nT = 15
    "t16":           (spec(50, 208),                      0, 0),      # D <= 64, nT = 16
    "d65_t15_hand":  (hand(65, 15),                       0, 0),      # nOT = 10, nT = 15
    "d65_t16":       (spec(65),                           0, 0),      # nOT = 10, nT = 16
    "t45_d66":       (spec(66, 544),                      0, 0),      # the widest flow whose float32 lane sweep fits 160 KiB
    "t46_d66":       (spec(66, 546),                      0, 0),      # ... and the first that does not
    "t64_d66":       (spec(66, 582),                      0, 0),
    "t65_d66":       (spec(66, 584),                      0, 0),
    "t64_d66_bf16":  (spec(66, 582),                      1, 0),
    "t65_d66_bf16":  (spec(66, 584),                      1, 0),
    "tri_no":        (spec(2, 32),                        0, 0),      # one degree group of 32 units
    "t15_bf16":      (spec(50, 204),                      1, 0),
    "t15_f16":       (spec(50, 204),                      2, 0),
    "t16_bf16":      (spec(50, 208),                      1, 0),
    "t16_f16":       (spec(50, 208),                      2, 0),
    "t16_four":      (spec(50, 208),                      0, LANE_FOUR),
    "nsf_d1_hand":   (hand(1, 1, n_out=23),               0, 0),
    "nsf_d2":        (spec(2, 16, "rqs"),                 0, 0),
    "nsf_d64":       (spec(64, None, "rqs"),              0, 0),
    "nsf_d65":       (spec(65, None, "rqs"),              0, 0),
    "nsf_tri_no":    (spec(2, 32, "rqs"),                 0, 0),
    "nsf_bins4":     (spec(10, None, "rqs", 4),           0, 0),
    "nsf_bins16":    (spec(10, None, "rqs", 16),          0, 0),
    "duo_big_hand":  (hand(10, 70),                       0, 0),      # two-wave tables beyond 160 KiB, lone-wave layout within
    "nsf_wide_hand": (hand(65, 160, n_out=23),            0, 0),      # no spline kernel's LDS fits
    "epi_no_hand":   (hand(10, 1),                        0, 0),      # one hidden tile: no room for the scaler epilogue's scratch
    "nsf_epi_no_hand": (hand(10, 1, n_out=23),            0, 0),      # the same, spline
}


class pmc_maf_t(C.Structure):                     # include/pocomc_amd.h (tests/test_abi.py holds its size)
    _fields_ = [("packed", C.c_void_p), ("meta", C.c_void_p), ("D", C.c_int32), ("H", C.c_int32), ("T", C.c_int32),
                ("Hp", C.c_int32), ("Dp", C.c_int32), ("nT", C.c_int32), ("nXT", C.c_int32), ("nOT", C.c_int32),
                ("pk_per_transform", C.c_int64), ("tri_ok", C.c_int32), ("n_out", C.c_int32), ("lane16", C.c_void_p),
                ("lane16_fmt", C.c_int32), ("reserved", C.c_int32)]


def layout(name):
    """The layout fields of a case as a dict (D, H, T, Hp, Dp, nT, nXT, nOT, pk_per_transform, tri_ok, n_out)."""
    lay = CASES[name][0]
    if lay["kind"] == "spec":
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        from pocomc_amd.maf_spec import MAFSpec
        s = MAFSpec(lay["D"], lay["T"], lay["hidden"], lay["uni"], lay["bins"])
        return dict(D=s.n_dim, H=s.hidden, T=s.n_transforms, Hp=s.Hp, Dp=s.Dp, nT=s.nT, nXT=s.nXT, nOT=s.nOT,
                    pk_per_transform=s.pk_per_transform, tri_ok=int(s.tri_ok), n_out=s.n_out)
    D, nT, n_out = lay["D"], lay["nT"], lay["n_out"]
    Dp = (D + 15) // 16 * 16
    nXT, nOT = Dp // 16, (n_out * Dp + 15) // 16
    pk = (nT * nXT * 2 + 2 * nT * nT + nOT * nT + 4 * nT) * 256 + Dp * nT * 16      # (about MAFSpec's; far below every offset limit)
    return dict(D=D, H=nT * 16, T=lay["T"], Hp=nT * 16, Dp=Dp, nT=nT, nXT=nXT, nOT=nOT, pk_per_transform=pk,
                tri_ok=lay["tri_ok"], n_out=n_out)


def descriptor(name, cls=pmc_maf_t):
    """A ``pmc_maf_t`` with the case's layout; ``lane16`` is a non-NULL word that nothing dereferences."""
    _, fmt, reserved = CASES[name]
    return cls(packed=None, meta=None, lane16=(8 if fmt else None), lane16_fmt=fmt, reserved=reserved, **layout(name))


def record(library, commit):
    lib = C.CDLL(library)
    lib.pmc_maf_inverse_auto_is_duo.argtypes = [C.POINTER(pmc_maf_t), C.c_int64]
    for q in ("pmc_maf_inverse_auto_is_lane", "pmc_maf_inverse_auto_is_nsf2"):
        getattr(lib, q).argtypes = [C.POINTER(pmc_maf_t)]
    table = {}
    for name in CASES:
        d = descriptor(name)
        table[name] = {"is_lane": lib.pmc_maf_inverse_auto_is_lane(C.byref(d)),
                       "is_nsf2": lib.pmc_maf_inverse_auto_is_nsf2(C.byref(d)),
                       "is_duo": {str(n): lib.pmc_maf_inverse_auto_is_duo(C.byref(d), n) for n in ROWS}}
    out = {"commit": commit, "what": "pmc_maf_inverse_auto_is_lane / _is_nsf2 / _is_duo(n) of the product library built "
           "from that commit, for every case of tests/inverse_plan_cases.py", "rows": list(ROWS), "answers": table}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inverse_queries_parent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return path


if __name__ == "__main__":
    print(record(sys.argv[1], sys.argv[2]))
