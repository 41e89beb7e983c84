"""Steps per second of one MCMC kernel call whose HOST likelihood returns blobs: bench.py's numpy Rosenbrock on 1e4 walkers
x 32 dimensions, maf3 flow, prior U(-10, 10)^32, beta = 0.5, preconditioned tpCN, 200-step calls.

    python scripts/time_host_blobs.py [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3] [--lanes 1]
                                      [--modes plain,pipelined:2,pipelined:8,whole_set:2,whole_set:8] [--root DIR] [--out FILE]

Modes (``name:B``, B float64 blob columns per row):
    plain          the pipelined call without blobs (x_order='F'), the headline mode;
    pipelined:B    the same call with ``state_dict["blobs"]`` a device tensor: the likelihood returns ``(logl, blobs)`` numpy,
                   the accepted walkers' rows move in a launch behind each accept (``pmc_blob_rows_move``);
    whole_set:B    the same blobs as a numpy array in ``state_dict``: one engine, no pipeline, sigma / mu from the host, the
                   accept mask downloaded every step for ``blobs[mask] = blobs_prime[mask]`` -- the route before this mode.
Every mode takes the same Philox variates and is timed over --repeats calls after one warm-up call; one JSON line.
``--root DIR``: import ``pocomc_amd`` and ``bench`` from another checkout (an A/B of ``plain`` against the parent commit)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--modes", default="plain,pipelined:2,pipelined:8,whole_set:2,whole_set:8")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from bench import rosenbrock

    N, D = args.walkers, args.dim
    prior = pc.Prior([uniform(-10, 20)] * D)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    scaler.fit(prior.rvs(4 * N))
    x = np.random.default_rng(0).uniform(-2.0, 2.0, size=(N, D))
    u = scaler.forward(x)
    flow = pc.Flow(D, "maf3", seed=0)
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    logl0 = rosenbrock(np.asfortranarray(x))

    def call(mode, B):
        def blobs_np(xx):
            """B derived columns of a row: x_j scaled (j < D), wrapped around beyond."""
            return np.stack([xx[:, j % D] * (j + 1.0) for j in range(B)], axis=1)
        blobs0 = None
        if mode == "pipelined":
            blobs0 = torch.zeros(N, B, dtype=torch.float64, device="cuda")
        elif mode == "whole_set":
            blobs0 = np.zeros((N, B))
        like = (lambda xx: (rosenbrock(xx), blobs_np(xx))) if B else (lambda xx: (rosenbrock(xx), None))
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x),
                     beta=0.5, blobs=blobs0)
        funcs = dict(loglike=like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                    x_order="F")
        if args.lanes > 1:
            opts["lanes"] = args.lanes
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res

    lib = pmcmc._lib.load()
    out = dict(walkers=N, dim=D, flow="maf3", steps=args.steps, repeats=args.repeats, lanes=args.lanes,
               kind="preconditioned_pcn", gpu=torch.cuda.get_device_name(torch.cuda.current_device()),
               root=os.path.abspath(args.root), build_id=lib.pmc_build_id().decode())
    for spec in args.modes.split(","):
        mode, _, b = spec.partition(":")
        B = int(b or 0)
        if mode not in ("plain", "pipelined", "whole_set") or (mode == "plain") != (B == 0):
            sys.exit(f"bad mode {spec}")
        call(mode, B)                                        # warm-up: code objects, pinned buffers, torch allocator
        rates, res = [], None
        for _ in range(args.repeats):
            r, res = call(mode, B)
            rates.append(r)
        out[spec] = dict(steps_per_s_best=max(rates), steps_per_s_median=float(np.median(rates)),
                         us_per_step_median=1e6 / float(np.median(rates)), all=rates, accept=float(res["accept"]))
        if B:
            blobs = res["blobs"]
            moved = (res["x"] != x).any(axis=1)
            want = np.stack([res["x"][:, j % D] * (j + 1.0) for j in range(B)], axis=1)
            out[spec]["blobs_follow_x"] = bool(np.array_equal(blobs[moved], want[moved]) and not blobs[~moved].any())
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
