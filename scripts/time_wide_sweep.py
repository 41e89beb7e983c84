"""Time ``Flow.inverse`` of the default-width flows (H = 512) under AUTO and under the opt-in workgroup sweep of their family:
``--family affine``: ``Flow(inverse_sweep="workgroup")``, ``csrc/maf_inverse_wg.hip``;
``--family spline``: ``Flow(inverse_sweep="workgroup_spline")``, ``csrc/maf_inverse_wg_nsf.hip``.

    python scripts/time_wide_sweep.py [--family affine|spline] [--cell N] [--out FILE]

``--out`` defaults to nothing written; the kept results are ``profiles/wide_workgroup_sweep.txt`` (affine) and
``profiles/wide_workgroup_spline_sweep.txt`` (spline).

Cells, affine: maf6 and maf3 at D = 92, 102, 110, 114 -- where no other triangular sweep fits 160 KiB of LDS and AUTO takes
the D-pass algorithm -- and at D = 86 and 128, where AUTO takes the lane-per-walker sweep (twelve cells).  Spline: nsf6 and
nsf3 at D = 97, 102, 108 -- where the lone-wave spline sweep does not fit and AUTO takes the lean D-pass kernel -- and at
D = 65, 86, 128, 157, where AUTO takes the lone-wave spline sweep (fourteen cells).  ``--cell N``: one of them, appended to
``--out``; a caller gives every run its own time limit.  Per cell: us per call on 5000 and on 512 rows, AUTO next to the
workgroup sweep, each with the sweep the plan names, and AUTO's time over the workgroup sweep's.  Both flows of a cell hold
the same parameters, and the two results are compared before anything is timed.  Method: every call warmed up; then
``--rounds`` windows per call, a window being as many back-to-back calls between two device events as take about
``--window`` seconds (at least 3); the median of the windows' per-call times and their range."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pocomc_amd as pc                                    # noqa: E402
from pocomc_amd import _lib                                # noqa: E402

FAMILIES = {
    "affine": dict(cells=tuple((name, D) for D in (92, 102, 110, 114, 86, 128) for name in ("maf6", "maf3")),
                   inverse_sweep="workgroup", what="affine flows (H = 512)",
                   sweeps={1: "lone-wave D-pass", 5: "lane sweep", 8: "lean D-pass", 9: "workgroup sweep"}),
    "spline": dict(cells=tuple((name, D) for D in (97, 102, 108, 65, 86, 128, 157) for name in ("nsf6", "nsf3")),
                   inverse_sweep="workgroup_spline", what="spline flows (8 bins)",
                   sweeps={2: "D-pass", 6: "lone-wave sweep", 7: "two-wave sweep", 8: "lean D-pass", 10: "workgroup spline sweep"}),
}
ROWS = (5000, 512)


def timed(call, rounds, window):
    """us per call: (median, min, max) over ``rounds`` windows of back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(reps):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    run(2)                                                  # warm-up: code objects, the LDS attribute, allocations
    reps = int(max(3, min(2000, window * 1e6 / run(3))))
    t = [run(reps) for _ in range(rounds)]
    return float(np.median(t)), min(t), max(t)


def sweep_of(f, n, names):
    ip = _lib.pmc_inverse_plan_t()
    _lib.check(f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, f.inverse_algo, 0, C.byref(ip)))
    return names[ip.sweep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), default="affine")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    fam = FAMILIES[a.family]
    cells, opt_in = fam["cells"], fam["inverse_sweep"]
    if not torch.cuda.is_available():
        sys.exit("time_wide_sweep: no GPU; a timing is taken on the GPU or not at all")
    lines = []
    if a.cell in (None, 0):
        lines += [f"# python {' '.join([os.path.join('scripts', os.path.basename(sys.argv[0]))] + sys.argv[1:])}",
                  f"# Flow.inverse of the default-width {fam['what']}, float32, us per call: median of {a.rounds} windows of "
                  f"~{a.window} s of back-to-back calls [min .. max], and the sweep that ran; {torch.cuda.get_device_name(0)}",
                  f"# flow    D   nT  rows | AUTO | inverse_sweep=\"{opt_in}\" | AUTO / workgroup"]
    g = torch.Generator(device="cuda").manual_seed(3)
    for name, D in (cells if a.cell is None else cells[a.cell:a.cell + 1]):
        auto = pc.Flow(D, name, seed=0)
        wg = pc.Flow(D, name, seed=0, inverse_sweep=opt_in)
        wg.set_params(auto.params)
        for n in ROWS:
            z = torch.randn(n, D, device="cuda", generator=g)
            (xa, la), (xw, lw) = auto.inverse(z), wg.inverse(z)
            if not (torch.isfinite(xw).all() and torch.allclose(xa, xw, rtol=1e-4, atol=1e-4) and torch.allclose(la, lw, rtol=1e-4, atol=1e-3)):
                sys.exit(f"time_wide_sweep: the two sweeps disagree at {name} D = {D}")
            ta, tw = timed(lambda: auto.inverse(z), a.rounds, a.window), timed(lambda: wg.inverse(z), a.rounds, a.window)
            lines.append(f"{name:6s} {D:4d} {auto.spec.nT:4d} {n:5d} | {ta[0]:10.1f} [{ta[1]:.1f} .. {ta[2]:.1f}] {sweep_of(auto, n, fam['sweeps'])} | "
                         f"{tw[0]:9.1f} [{tw[1]:.1f} .. {tw[2]:.1f}] {sweep_of(wg, n, fam['sweeps'])} | {ta[0] / tw[0]:6.1f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.cell not in (None, 0) else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
