"""Steps per second of one MCMC kernel call with the likelihood on the device against the same call with bench.py's numpy
Rosenbrock on the host: 1e4 walkers x 32 dimensions, maf3 flow, prior U(-10, 10)^32, beta = 0.5, preconditioned tpCN.

    python scripts/time_device_likelihood.py [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3] [--out FILE]
                                             [--modes host_numpy,device_torch]

The device mode hands the likelihood an (n, D) float64 view of x' on the GPU (option_dict["device_likelihood"]); the
host mode is the pipelined host call (x_order='F': x' to pinned host memory, logl' read back by the accept kernel).
Both calls take the same Philox variates; each mode is timed over --repeats calls of --steps steps after one warm-up
call, and the best and median steps/s are printed as one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rosenbrock_torch(x):
    """README.md:53-55, -sum_i [10 (x_2i^2 - x_2i+1)^2 + (x_2i - 1)^2], as torch operations on the device."""
    a, b = x[:, 0::2], x[:, 1::2]
    t = a * a - b
    return -(10.0 * (t * t) + (a - 1.0) ** 2).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default="host_numpy,device_torch", help="comma-separated subset to time (e.g. one mode "
                    "under a memory-copy trace)")
    args = ap.parse_args()
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from bench import rosenbrock

    N, D = args.walkers, args.dim
    prior = pc.Prior([uniform(-10, 20)] * D)
    rng = np.random.default_rng(0)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    scaler.fit(prior.rvs(4 * N))
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    u = scaler.forward(x)
    flow = pc.Flow(D, "maf3", seed=0)
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    logl0 = rosenbrock(np.asfortranarray(x))

    def call(device):
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x),
                     beta=0.5, blobs=None)
        like = (lambda xt: (rosenbrock_torch(xt), None)) if device else (lambda xx: (rosenbrock(xx), None))
        funcs = dict(loglike=like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3)
        opts.update(dict(device_likelihood=True) if device else dict(x_order="F"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res

    out = dict(walkers=N, dim=D, flow="maf3", steps=args.steps, repeats=args.repeats, kind="preconditioned_pcn",
               gpu=torch.cuda.get_device_name(0))
    results = {}
    modes = args.modes.split(",")
    for mode, device in (("host_numpy", False), ("device_torch", True)):
        if mode not in modes:
            continue
        call(device)                                        # warm-up: code objects, pinned buffers, torch allocator
        rates = [call(device)[0] for _ in range(args.repeats)]
        out[mode] = dict(steps_per_s_best=max(rates), steps_per_s_median=float(np.median(rates)),
                         us_per_step_median=1e6 / float(np.median(rates)), all=rates)
        results[mode] = call(device)[1]
    # (the two Rosenbrocks sum a row in different orders: the trajectories agree to rounding, not bit for bit)
    for mode, res in results.items():
        out[mode]["accept"] = float(res["accept"])
    if len(results) == 2:
        out["speedup_median"] = out["device_torch"]["steps_per_s_median"] / out["host_numpy"]["steps_per_s_median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
