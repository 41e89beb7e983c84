"""Time the float32 flow calls of the default-width flows at n_dim >= 86 (H = 512 by the reference's width rule): the widths
whose full kernel instances exceed the 160 KiB LDS of a workgroup and take the lean ones (``pmc_maf_lds_plan``), or, for the
inverse, fall back to the lean D-pass kernel (``pmc_maf_inverse_plan``).

    python scripts/time_wide_default_flows.py [--cell N] [--out profiles/wide_default_flows.txt]

Cells: maf6 and nsf6 at D = 86, 102, 128, 157 (``--cell N``: one of the eight, appended to ``--out``; a caller gives every run
its own time limit).  Per cell: us per call of ``Flow.log_prob`` on 512 and on 5000 rows, of ``Flow.inverse`` (AUTO) on 5000
rows, and of one optimizer step on 512 rows (what ``AdamW.epoch`` enqueues per batch: loss and gradient, clip, AdamW, the
images' refresh), each with the instance that ran.  Method: every call warmed up; then ``--rounds`` windows per call, a window
being as many back-to-back calls between two device events as take about ``--window`` seconds (at least 3); the median of the
windows' per-call times and their range.  The parent of the commit that added the lean instances refuses these flows: there is
no earlier number to compare with, and none is a target."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pocomc_amd as pc                                    # noqa: E402
from pocomc_amd import _lib                                # noqa: E402
from pocomc_amd.train import AdamW, _train_state           # noqa: E402

CELLS = tuple((name, D) for D in (86, 102, 128, 157) for name in ("maf6", "nsf6"))
SWEEPS = {1: "lone-wave D-pass", 2: "D-pass (full)", 3: "lone-wave sweep", 4: "two-wave sweep", 5: "lane sweep", 6: "lone-wave spline sweep",
          7: "two-wave spline sweep", 8: "lean D-pass"}


def timed(call, rounds, window):
    """us per call: median [min .. max] over ``rounds`` windows of back-to-back calls."""
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
    return f"{np.median(t):9.1f} [{min(t):.1f} .. {max(t):.1f}]"


def step_call(f, x):
    start = f.params.clone()
    opt = AdamW(f, 1e-3)
    _train_state(f).repack(f)
    acc = torch.zeros(1, dtype=torch.float32, device="cuda")

    def call():
        opt.epoch(x, None, None, x.shape[0], 1.0, acc)     # one batch: one optimizer step

    return call, lambda: (f.set_params(start), float(acc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_wide_default_flows: no GPU; a timing is taken on the GPU or not at all")
    lines = []
    if a.cell in (None, 0):
        lines += [f"# float32 calls of the default-width flows (H = 512), us per call: median of {a.rounds} windows of ~{a.window} s of "
                  f"back-to-back calls [min .. max], and the instance that ran; {torch.cuda.get_device_name(0)}",
                  "# flow    D   Hp | log_prob 512 rows | log_prob 5000 rows | inverse (AUTO) 5000 rows | optimizer step 512 rows"]
    g = torch.Generator(device="cuda").manual_seed(3)
    for name, D in (CELLS if a.cell is None else CELLS[a.cell:a.cell + 1]):
        f = pc.Flow(D, name, seed=0)
        plan = f.lds_plan()
        ip = _lib.pmc_inverse_plan_t()
        _lib.check(f.lib.pmc_maf_inverse_plan(C.byref(f._desc), 5000, 0, 0, C.byref(ip)))
        x512 = torch.randn(512, D, device="cuda", generator=g) * 1.5
        x5000 = torch.randn(5000, D, device="cuda", generator=g) * 1.5
        z5000 = torch.randn(5000, D, device="cuda", generator=g)
        cols = [f"{timed(lambda: f.log_prob(x512), a.rounds, a.window)} {plan['forward'][0]}",
                f"{timed(lambda: f.log_prob(x5000), a.rounds, a.window)} {plan['forward'][0]}",
                f"{timed(lambda: f.inverse(z5000), a.rounds, a.window)} {SWEEPS[ip.sweep]}"]
        call, finish = step_call(f, x512)
        cols.append(f"{timed(call, a.rounds, a.window)} {plan['train'][0]}")
        _, loss = finish()
        if not np.isfinite(loss):
            sys.exit("time_wide_default_flows: non-finite loss")
        lines.append(f"{name:6s} {D:4d} {f.spec.Hp:4d} | " + " | ".join(cols))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.cell not in (None, 0) else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
