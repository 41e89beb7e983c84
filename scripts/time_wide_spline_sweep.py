"""Time ``Flow.inverse`` of the default-width spline flows (H = 512 from D = 86) under AUTO and under the opt-in workgroup
sweep of the spline flows (``Flow(inverse_sweep="workgroup_spline")``, ``csrc/maf_inverse_wg_nsf.hip``).  The sibling of
``scripts/time_wide_sweep.py``: the same method and the same ``--cell`` protocol.

    python scripts/time_wide_spline_sweep.py [--cell N] [--out profiles/wide_workgroup_spline_sweep.txt]

Cells: nsf6 and nsf3 at D = 97, 102, 108 -- where the lone-wave spline sweep does not fit 160 KiB of LDS and AUTO takes the
lean D-pass kernel -- and at D = 65, 86, 128, 157, where AUTO takes the lone-wave spline sweep (``--cell N``: one of the
fourteen, appended to ``--out``; a caller gives every run its own time limit).  Per cell: us per call on 5000 and on 512
rows, AUTO next to the workgroup sweep, each with the sweep the plan names, and AUTO's time over the workgroup sweep's.  Both flows of
a cell hold the same parameters, and the two results are compared before anything is timed.  Method: every call warmed up;
then ``--rounds`` windows per call, a window being as many back-to-back calls between two device events as take about
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

CELLS = tuple((name, D) for D in (97, 102, 108, 65, 86, 128, 157) for name in ("nsf6", "nsf3"))
ROWS = (5000, 512)
SWEEPS = {2: "D-pass", 6: "lone-wave sweep", 7: "two-wave sweep", 8: "lean D-pass", 10: "workgroup spline sweep"}


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


def sweep_of(f, n):
    ip = _lib.pmc_inverse_plan_t()
    _lib.check(f.lib.pmc_maf_inverse_plan(C.byref(f._desc), n, f.inverse_algo, 0, C.byref(ip)))
    return SWEEPS[ip.sweep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_wide_spline_sweep: no GPU; a timing is taken on the GPU or not at all")
    lines = []
    if a.cell in (None, 0):
        lines += [f"# python {' '.join([os.path.join('scripts', os.path.basename(sys.argv[0]))] + sys.argv[1:])}",
                  f"# Flow.inverse of the default-width spline flows (8 bins), float32, us per call: median of {a.rounds} windows of "
                  f"~{a.window} s of back-to-back calls [min .. max], and the sweep that ran; {torch.cuda.get_device_name(0)}",
                  "# flow    D   nT  rows | AUTO | inverse_sweep=\"workgroup_spline\" | AUTO / workgroup"]
    g = torch.Generator(device="cuda").manual_seed(3)
    for name, D in (CELLS if a.cell is None else CELLS[a.cell:a.cell + 1]):
        auto = pc.Flow(D, name, seed=0)
        wg = pc.Flow(D, name, seed=0, inverse_sweep="workgroup_spline")
        wg.set_params(auto.params)
        for n in ROWS:
            z = torch.randn(n, D, device="cuda", generator=g)
            (xa, la), (xw, lw) = auto.inverse(z), wg.inverse(z)
            if not (torch.isfinite(xw).all() and torch.allclose(xa, xw, rtol=1e-4, atol=1e-4) and torch.allclose(la, lw, rtol=1e-4, atol=1e-3)):
                sys.exit(f"time_wide_spline_sweep: the two sweeps disagree at {name} D = {D}")
            ta, tw = timed(lambda: auto.inverse(z), a.rounds, a.window), timed(lambda: wg.inverse(z), a.rounds, a.window)
            lines.append(f"{name:6s} {D:4d} {auto.spec.nT:4d} {n:5d} | {ta[0]:10.1f} [{ta[1]:.1f} .. {ta[2]:.1f}] {sweep_of(auto, n)} | "
                         f"{tw[0]:9.1f} [{tw[1]:.1f} .. {tw[2]:.1f}] {sweep_of(wg, n)} | {ta[0] / tw[0]:6.1f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.cell not in (None, 0) else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
