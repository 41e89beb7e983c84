"""Time ``Flow.log_prob`` of the neural spline flows: the float32 kernel (``csrc/maf_forward_wg.hip``, unchanged since before
the bf16 spline kernel existed) against the bf16 matrix-core kernel (``csrc/maf_forward_bf16.h``) on the same flow, the
same parameters and the same rows.

    python scripts/time_bf16_nsf_forward.py [--out profiles/bf16_nsf_forward.txt]

Flows: nsf6 at (D, H) = (128, 512) and (64, 256); rows 512 and 5000.  Method: both flows warmed up on every row count;
then ``--rounds`` rounds that ALTERNATE the two precisions, each window ``--calls`` back-to-back calls between two device
events (a window of 200 calls is 20 - 400 ms); per cell the median of the rounds' per-call times and their range.  The
calls include ``Flow.log_prob``'s own host work (two allocations, the launch): what a user of the flow pays.  Also printed:
how far the bf16 log-density is from the float32 one on these rows, so that the time is read next to what it buys."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pocomc_amd as pc                                    # noqa: E402
from pocomc_amd.maf_spec import MAFSpec                    # noqa: E402


def window(f, xs, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f.log_prob(xs)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3               # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_bf16_nsf_forward: no GPU; a timing is taken on the GPU or not at all")
    lines = [f"# Flow.log_prob of nsf6, float32 kernel vs bf16 matrix-core kernel; us per call: median of {a.rounds} alternating "
             f"rounds of {a.calls} calls [min .. max]; {torch.cuda.get_device_name(0)}",
             "# D    H    rows   float32 us              bf16 us                 float32 / bf16   max |dlog_prob| / max |log_prob|"]
    for D, H in ((128, 512), (64, 256)):
        spec = MAFSpec(D, 6, hidden=H, univariate="rqs")
        flows = {"f32": pc.Flow(D, spec, seed=0), "bf16": pc.Flow(D, spec, seed=0, precision="bf16")}
        flows["bf16"].set_params(flows["f32"].params)
        x = torch.randn(5000, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        for n in (512, 5000):
            xs = x[:n].contiguous()
            for f in flows.values():
                for _ in range(5):
                    f.log_prob(xs)
            torch.cuda.synchronize()
            t = {k: [] for k in flows}
            for _ in range(a.rounds):
                for k, f in flows.items():
                    t[k].append(window(f, xs, a.calls))
            lp32, lp16 = flows["f32"].log_prob(xs), flows["bf16"].log_prob(xs)
            err = float((lp16 - lp32).abs().max() / lp32.abs().max())
            m = {k: float(np.median(v)) for k, v in t.items()}
            cell = lambda k: f"{m[k]:8.1f} [{min(t[k]):.1f} .. {max(t[k]):.1f}]"
            lines.append(f"{D:4d} {H:4d} {n:6d}   {cell('f32'):<24s}{cell('bf16'):<24s}{m['f32'] / m['bf16']:6.2f}           {err:.1e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
