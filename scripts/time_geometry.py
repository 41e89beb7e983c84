"""Times ``Geometry.fit`` on float32 rows (theta) in both Student-t modes: ms per fit (device events around the call,
which ends in a download, after warm-up; median, minimum and maximum of ``--calls`` calls), and for ``student="em"`` the
EM iterations, the time per iteration over the reference mode's fit, and the host reads of a fit.

    python scripts/time_geometry.py [--calls 30] [--modes reference,em] [--root DIR]

``--root DIR`` imports ``pocomc_amd`` from another tree (a checkout of another commit, built) -- ``--modes reference``
there times the default path of that commit at the same shapes.  Rows: a correlated 5-degrees-of-freedom t, seeded.
Needs the GPU; prints one line per (shape, mode)."""
import argparse
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--modes", default="reference,em")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from pocomc_amd import geometry  # noqa: E402

SHAPES = [(1024, 10), (4096, 32), (4096, 128)]
LAST = {}                                        # the info of the latest pmc_student_em call (host_reads is not in student_info)
if hasattr(geometry, "student_em"):
    _student_em = geometry.student_em

    def _spy(*a, **k):
        out = _student_em(*a, **k)
        LAST.update(out[2])
        return out
    geometry.student_em = _spy


def rows(n, D):
    rng = np.random.default_rng(D)
    A = (np.eye(D) + 0.5 * rng.normal(size=(D, D)) / np.sqrt(D)) * np.linspace(0.5, 2.0, D)[:, None]
    z = rng.normal(size=(n, D)) @ A.T / np.sqrt(rng.chisquare(5.0, size=n) / 5.0)[:, None]
    return torch.from_numpy((rng.normal(size=D) * 3.0 + z).astype(np.float32)).cuda()


def time_fit(g, x, calls):
    for _ in range(5):
        g.fit(x)
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.fit(x)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.median(ms), min(ms), max(ms)


print(f"tree {os.path.abspath(args.root)}, {torch.cuda.get_device_name(0)}, {args.calls} calls per figure")
for n, D in SHAPES:
    x = rows(n, D)
    ref_ms = None
    for mode in args.modes.split(","):
        g = geometry.Geometry() if mode == "reference" else geometry.Geometry(student=mode)
        med, lo, hi = time_fit(g, x, args.calls)
        line = f"n {n:5d} D {D:4d} {mode:9s} {med:8.3f} ms per fit (min {lo:.3f}, max {hi:.3f})"
        if mode == "reference":
            ref_ms = med
            line += "; host reads 2 (moments, medians)"
        else:
            info = g.student_info
            line += f"; nu {info['nu']:.4f}, {info['iterations']} EM iterations ({info['status']})"
            if ref_ms is not None:
                line += f", {1e3 * (med - ref_ms) / info['iterations']:.1f} us per iteration over the reference mode"
            line += f"; host reads 2 + {LAST['host_reads']} (state, every 8 iterations) + 1 (result)"
        print(line, flush=True)
