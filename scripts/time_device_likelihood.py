"""Steps per second of one MCMC kernel call with the likelihood on the device against the same call with bench.py's numpy
Rosenbrock on the host: 1e4 walkers x 32 dimensions, maf3 flow, prior U(-10, 10)^32, beta = 0.5, preconditioned tpCN.

    python scripts/time_device_likelihood.py [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3] [--out FILE]
                                             [--modes host_numpy,device_torch] [--ranks N] [--blobs B]

The device mode hands the likelihood an (n, D) float64 view of x' on the GPU (option_dict["device_likelihood"]); the
host mode is the pipelined host call (x_order='F': x' to pinned host memory, logl' read back by the accept kernel).
``--blobs B`` (device mode only): the likelihood also returns B float64 columns per row as blobs, which stay on the device
and move with the accepted walkers in the accept launch (``state_dict["blobs"]`` a device tensor).
Both calls take the same Philox variates; each mode is timed over --repeats calls of --steps steps after one warm-up
call, and the best and median steps/s are printed as one JSON line.

``--ranks N`` (N > 1): the walker set row-sharded over N ranks, --walkers rows PER RANK, each rank a fresh child process of
this script on the visible GPUs round robin, talking over gloo; every rank prints its own JSON line (``rank`` in it) and
``--out FILE`` becomes ``FILE.rank<r>``.  The exchange tier is the environment's (``PMC_C_ALLREDUCE``, ``PMC_COMM_MAILBOX``).
Ranks that share one GPU share its compute units: their per-rank figure is what the exchange launch and the contention
cost together, not a scaling number."""
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


def launch_ranks(n_ranks):
    """This script once per rank, each a fresh child process; returns the worst exit status."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE=str(n_ranks))
        procs.append(subprocess.Popen([sys.executable] + sys.argv, env=env))
    return max(abs(p_.wait()) for p_ in procs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default="host_numpy,device_torch", help="comma-separated subset to time (e.g. one mode "
                    "under a memory-copy trace)")
    ap.add_argument("--ranks", type=int, default=1, help="shard the walkers over this many ranks (--walkers rows each)")
    ap.add_argument("--blobs", type=int, default=0, help="float64 blob columns the device likelihood returns per row")
    args = ap.parse_args()
    rank, world = 0, 1
    if args.ranks > 1:
        if "WORLD_SIZE" not in os.environ:
            sys.exit(launch_ranks(args.ranks))
        import torch.distributed as dist
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        assert world == args.ranks, f"--ranks {args.ranks} but WORLD_SIZE={world}"
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(rank % torch.cuda.device_count())
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from bench import rosenbrock

    N, D = args.walkers, args.dim
    prior = pc.Prior([uniform(-10, 20)] * D)
    rng = np.random.default_rng(rank)                      # (every rank its own rows)
    scaler = pc.Reparameterize(D, bounds=prior.bounds)
    scaler.fit(np.random.default_rng(0).uniform(-10.0, 10.0, size=(4 * N, D)) if world > 1 else prior.rvs(4 * N))
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    u = scaler.forward(x)
    flow = pc.Flow(D, "maf3", seed=0)
    geo = Geometry()
    u_geo = u if rank == 0 else scaler.forward(np.random.default_rng(0).uniform(-2.0, 2.0, size=(N, D)))   # (replicated: rank 0's rows)
    geo.fit(flow.forward(torch.from_numpy(u_geo).float())[0].numpy().astype(np.float64))
    logl0 = rosenbrock(np.asfortranarray(x))

    B = args.blobs
    if B and "host_numpy" in args.modes.split(","):
        sys.exit("--blobs times the device mode only: add --modes device_torch")

    def blobs_torch(xt):
        """B derived columns of a row: x_j scaled (j < D), wrapped around beyond."""
        return torch.stack([xt[:, j % D] * (j + 1.0) for j in range(B)], dim=1)

    def call(device):
        blobs0 = torch.zeros(N, B, dtype=torch.float64, device="cuda") if (B and device) else None
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x),
                     beta=0.5, blobs=blobs0)
        if device:
            like = (lambda xt: (rosenbrock_torch(xt), blobs_torch(xt))) if B else (lambda xt: (rosenbrock_torch(xt), None))
        else:
            like = lambda xx: (rosenbrock(xx), None)
        funcs = dict(loglike=like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3)
        opts.update(dict(device_likelihood=True) if device else dict(x_order="F"))
        if world > 1:
            opts.update(group=None, shard_offset=rank * N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res

    out = dict(walkers=N, dim=D, flow="maf3", steps=args.steps, repeats=args.repeats, kind="preconditioned_pcn",
               gpu=torch.cuda.get_device_name(torch.cuda.current_device()), rank=rank, ranks=world, blobs=B,
               c_allreduce=os.environ.get("PMC_C_ALLREDUCE", "1"), mailbox=os.environ.get("PMC_COMM_MAILBOX", ""))
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
    if world > 1:                                           # 0: device mailboxes, 1: host mailboxes, none: torch.distributed
        out["comm_kinds"] = sorted({int(pmcmc._lib.load().pmc_comm_kind(v[0])) for v in pmcmc._COMMS.values() if v[0]})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out if world == 1 else f"{args.out}.rank{rank}", "w") as f:
            f.write(line + "\n")
    if world > 1:
        pmcmc.drop_comms()
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
