"""Steps per second of one MCMC kernel call with Prior.logpdf on the host (scipy, one frozen-distribution call per
dimension) against the same call with the prior on the device (Prior(dists, device=True)): 1e4 walkers x 32 dimensions,
maf3 flow, beta = 0.5, preconditioned tpCN.  The prior's 32 factors cycle through the twelve families beyond uniform /
normal, placed so that the Rosenbrock likelihood's mass sits inside every support; a uniform(-10, 20)^32 prior (the
device's two-family path, bench.py's prior) is the reference row.

    python scripts/time_prior.py [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3] [--out FILE]

Modes: {host prior, device prior, uniform reference} x {bench.py's numpy Rosenbrock on the host (pipelined host call,
x_order='F'), the torch Rosenbrock on the device (device_likelihood=True)}.  Each mode takes one warm-up call, then the
modes are timed in turn, --repeats rounds; the best and median steps/s per mode and the host cost of one Prior.logpdf
call on the 1e4 x 32 block are printed as one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def families():
    """Twelve factors whose supports hold the Rosenbrock's mass (x_2i around [-2, 3], x_2i+1 around [-1, 9])."""
    from scipy import stats as ss
    return [ss.truncnorm(-3, 3, loc=1, scale=4), ss.loguniform(0.01, 30, loc=-10), ss.lognorm(0.8, loc=-10, scale=8),
            ss.halfnorm(loc=-10, scale=8), ss.expon(loc=-10, scale=8), ss.gamma(2.5, loc=-10, scale=4),
            ss.invgamma(3, loc=-10, scale=20), ss.beta(2, 2, loc=-10, scale=25), ss.cauchy(1, 3),
            ss.halfcauchy(loc=-10, scale=5), ss.laplace(1, 3), ss.t(4, loc=1, scale=3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from bench import rosenbrock
    from time_device_likelihood import rosenbrock_torch

    N, D = args.walkers, args.dim
    fam = families()
    dists = [fam[j % len(fam)] for j in range(D)]
    priors = dict(host=pc.Prior(dists, device=False), device=pc.Prior(dists, device=True),
                  uniform=pc.Prior([uniform(-10, 20)] * D))
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    logl0 = rosenbrock(np.asfortranarray(x))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))                # (the scaler's standardisation: the walkers' region)
    setups = {}
    for name in ("device", "uniform"):
        scaler = pc.Reparameterize(D, bounds=priors[name].bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(D, "maf3", seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        setups[name] = (priors[name], scaler, flow, geo, u)
    setups["host"] = (priors["host"],) + setups["device"][1:]   # the same scaler / flow / geometry as the device prior

    def call(pname, device_like):
        prior, scaler, flow, geo, u = setups[pname]
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x),
                     beta=0.5, blobs=None)
        like = (lambda xt: (rosenbrock_torch(xt), None)) if device_like else (lambda xx: (rosenbrock(xx), None))
        funcs = dict(loglike=like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3)
        opts.update(dict(device_likelihood=True) if device_like else dict(x_order="F"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res

    modes = [(f"{p}_prior__{lk}", p, lk == "device_torch") for lk in ("host_numpy", "device_torch")
             for p in ("host", "device", "uniform")]
    out = dict(walkers=N, dim=D, flow="maf3", steps=args.steps, repeats=args.repeats, kind="preconditioned_pcn",
               prior_factors=[f"{d.dist.name}{d.args}{d.kwds}" for d in fam], gpu=torch.cuda.get_device_name(0))
    last = {}
    for name, p, dev in modes:                                  # warm-up: code objects, pinned buffers, allocator
        last[name] = call(p, dev)[1]
    rates = {name: [] for name, _, _ in modes}
    for _ in range(args.repeats):                               # the modes alternate
        for name, p, dev in modes:
            r, res = call(p, dev)
            rates[name].append(r)
            last[name] = res
    for name, _, _ in modes:
        rs = rates[name]
        out[name] = dict(steps_per_s_best=max(rs), steps_per_s_median=float(np.median(rs)),
                         us_per_step_median=1e6 / float(np.median(rs)), all=rs, accept=float(last[name]["accept"]),
                         calls=int(last[name]["calls"]))
    for lk in ("host_numpy", "device_torch"):
        h, d = out[f"host_prior__{lk}"], out[f"device_prior__{lk}"]
        out[f"device_over_host_prior__{lk}"] = d["steps_per_s_median"] / h["steps_per_s_median"]
    # the host prior's own cost: one Prior.logpdf (32 scipy calls) on a block of N walkers
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        priors["host"].logpdf(x)
        t.append(time.perf_counter() - t0)
    out["host_prior_logpdf_ms_median"] = 1e3 * float(np.median(t))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
