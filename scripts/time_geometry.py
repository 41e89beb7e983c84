"""Times ``Geometry.fit`` on float32 rows (theta) in the Student-t modes: ms per fit (device events around the call,
which ends in a download, after warm-up; median, minimum and maximum of ``--calls`` calls), and for the EM modes the
EM iterations, the time per iteration over the reference mode's fit, and the host reads of a fit.

    python scripts/time_geometry.py [--calls 30] [--modes reference,em,em_weighted] [--weighted] [--root DIR]

``--weighted`` fits with seeded log-normal weights (sigma = 1), the way the Sampler calls ``fit``: ``"reference"`` and ``"em"``
then include their systematic resample, second moments pass and medians over the index gather.  ``"em_weighted"`` is also
timed at 4096 x 157, a width the other EM mode refuses.

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
ap.add_argument("--weighted", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from pocomc_amd import geometry  # noqa: E402

SHAPES = [(1024, 10), (4096, 32), (4096, 128), (4096, 157)]
WIDE_ONLY = ("em_weighted",)                     # the modes that run above D = 128
LAST = {}                                        # the info of the latest pmc_student_em* call (host_reads is not in student_info)


def _spy_on(name):
    if hasattr(geometry, name):
        inner = getattr(geometry, name)

        def spy(*a, **k):
            out = inner(*a, **k)
            LAST.update(out[2])
            return out
        setattr(geometry, name, spy)


_spy_on("student_em")
_spy_on("student_em_weighted")


def rows(n, D):
    rng = np.random.default_rng(D)
    A = (np.eye(D) + 0.5 * rng.normal(size=(D, D)) / np.sqrt(D)) * np.linspace(0.5, 2.0, D)[:, None]
    z = rng.normal(size=(n, D)) @ A.T / np.sqrt(rng.chisquare(5.0, size=n) / 5.0)[:, None]
    return torch.from_numpy((rng.normal(size=D) * 3.0 + z).astype(np.float32)).cuda()


def weights(n, D):
    return torch.from_numpy(np.exp(np.random.default_rng(1000 + D).normal(size=n))).cuda()


def time_fit(g, x, w, calls):
    for _ in range(5):
        g.fit(x, w)
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.fit(x, w)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.median(ms), min(ms), max(ms)


print(f"tree {os.path.abspath(args.root)}, {torch.cuda.get_device_name(0)}, {args.calls} calls per figure, "
      f"{'log-normal weights' if args.weighted else 'unweighted'}")
for n, D in SHAPES:
    x = rows(n, D)
    w = weights(n, D) if args.weighted else None
    ref_ms = None
    for mode in args.modes.split(","):
        if D > 128 and mode not in WIDE_ONLY:
            continue
        np.random.seed(0)                        # (the resample of the weighted "reference" / "em" fits: the same in every tree)
        g = geometry.Geometry() if mode == "reference" else geometry.Geometry(student=mode)
        med, lo, hi = time_fit(g, x, w, args.calls)
        line = f"n {n:5d} D {D:4d} {mode:11s} {med:8.3f} ms per fit (min {lo:.3f}, max {hi:.3f})"
        if mode == "reference":
            ref_ms = med
            if not args.weighted:
                line += "; host reads 2 (moments, medians)"
        elif mode == "em_weighted":
            info = g.student_info
            line += (f"; nu {info['nu']:.4f}, {info['iterations']} EM iterations ({info['status']}), "
                     f"{1e3 * med / info['iterations']:.1f} us per iteration of the whole fit, ESS {info['ess']:.0f}; host reads 1 (moments) + "
                     f"{LAST['host_reads']} (weight record, state every 8 iterations) + 1 (result)")
        else:
            info = g.student_info
            line += f"; nu {info['nu']:.4f}, {info['iterations']} EM iterations ({info['status']})"
            if ref_ms is not None:
                line += f", {1e3 * (med - ref_ms) / info['iterations']:.1f} us per iteration over the reference mode"
            line += (f"; host reads of the EM {LAST['host_reads']} (state, every 8 iterations)" if args.weighted else
                     f"; host reads 2 + {LAST['host_reads']} (state, every 8 iterations) + 1 (result)")
        print(line, flush=True)
