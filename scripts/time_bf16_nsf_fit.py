"""Time one optimizer step of ``Flow.fit`` on the neural spline flows: the float32 engine (``csrc/maf_train.hip``, whose source
is what it was before the bf16 spline trainer existed) against ``train_engine="bf16_spline"`` (``csrc/maf_train_bf16.hip``) on
the same flow, the same parameters and the same rows, in the same process.

    python scripts/time_bf16_nsf_fit.py [--cell N] [--out profiles/bf16_nsf_fit.txt]

Cells: nsf6 at (D, H) = (128, 512) and (64, 256), nsf3 at (32, 256); batches of 512 and 64 rows.  ``--cell N`` runs one of
the three flows (a caller gives every run its own time limit) and appends to ``--out``.  A step is what ``AdamW.epoch``
enqueues per batch: loss and gradient, clip, AdamW, the images' refresh.  Method: both engines warmed up on every batch size; then
``--rounds`` rounds that ALTERNATE the two engines, each window one ``epoch`` call of ``--steps`` batches between two device
events; per cell the median of the rounds' per-step times and their range.  Every window starts from the same parameters and
moments (a step's time does not depend on them; the losses stay finite).  An engine that refuses a flow is reported as such."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pocomc_amd as pc                                    # noqa: E402
from pocomc_amd._lib import PocomcAmdError                 # noqa: E402
from pocomc_amd.maf_spec import MAFSpec                    # noqa: E402
from pocomc_amd.train import AdamW, _train_state           # noqa: E402

CELLS = (("nsf6", 128, 6, 512), ("nsf6", 64, 6, 256), ("nsf3", 32, 3, 256))


def window(f, start, x, batch, steps):
    """us per optimizer step of one ``epoch`` call of ``steps`` batches, from the parameters ``start``."""
    f.set_params(start)
    opt = AdamW(f, 1e-3)
    _train_state(f).repack(f)
    acc = torch.zeros(1, dtype=torch.float32, device="cuda")
    xs = x[:batch * steps]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    opt.epoch(xs, None, None, batch, 1.0, acc)
    e1.record()
    torch.cuda.synchronize()
    if not np.isfinite(float(acc)):
        sys.exit("time_bf16_nsf_fit: non-finite loss")
    return e0.elapsed_time(e1) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_bf16_nsf_fit: no GPU; a timing is taken on the GPU or not at all")
    lines = []
    if a.cell in (None, 0):
        lines += [f"# one optimizer step of Flow.fit on spline flows, float32 engine vs train_engine='bf16_spline'; us per step: median of "
                  f"{a.rounds} alternating rounds of one {a.steps}-step epoch call [min .. max]; {torch.cuda.get_device_name(0)}",
                  "# flow   D    H   rows   float32 us              bf16_spline us          float32 / bf16_spline"]
    for name, D, T, H in (CELLS if a.cell is None else CELLS[a.cell:a.cell + 1]):
        spec = MAFSpec(D, T, hidden=H, univariate="rqs")
        flows = {"f32": pc.Flow(D, spec, seed=0), "bf16_spline": pc.Flow(D, spec, seed=0, precision="bf16", train_engine="bf16_spline")}
        start = flows["f32"].params.clone()
        x = torch.randn(512 * a.steps, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 1.5
        for batch in (512, 64):
            refused = {}
            for k, f in flows.items():
                try:
                    window(f, start, x, batch, 5)
                except PocomcAmdError as e:
                    refused[k] = str(e)
            t = {k: [] for k in flows if k not in refused}
            for _ in range(a.rounds):
                for k in t:
                    t[k].append(window(flows[k], start, x, batch, a.steps))
            m = {k: float(np.median(v)) for k, v in t.items()}
            cell = lambda k: f"{m[k]:8.1f} [{min(t[k]):.1f} .. {max(t[k]):.1f}]" if k in m else "refused"
            ratio = f"{m['f32'] / m['bf16_spline']:6.2f}" if len(m) == 2 else "     -"
            lines.append(f"{name:6s} {D:4d} {H:4d} {batch:5d}   {cell('f32'):<24s}{cell('bf16_spline'):<24s}{ratio}")
            for k, why in refused.items():
                lines.append(f"#   {k} refuses {name} at D = {D}, H = {H}: {why}")
            print("\n".join(lines[-1 - len(refused):]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.cell not in (None, 0) else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
