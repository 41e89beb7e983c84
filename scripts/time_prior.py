"""Steps per second of one MCMC kernel call with Prior.logpdf on the host (scipy, one frozen-distribution call per
dimension) against the same call with the prior on the device (Prior(dists, device=True)): 1e4 walkers x 32 dimensions,
maf3 flow, beta = 0.5, preconditioned tpCN.  The prior's 32 factors cycle through the twelve families beyond uniform /
normal, placed so that the Rosenbrock likelihood's mass sits inside every support; a uniform(-10, 20)^32 prior (the
device's two-family path, bench.py's prior) is the reference row.

    python scripts/time_prior.py [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3] [--out FILE]

Modes: {host prior, device prior, uniform reference} x {bench.py's numpy Rosenbrock on the host (pipelined host call,
x_order='F'), the torch Rosenbrock on the device (device_likelihood=True)}.  Each mode takes one warm-up call, then the
modes are timed in turn, --repeats rounds; the best and median steps/s per mode and the host cost of one Prior.logpdf
call on the 1e4 x 32 block are printed as one JSON line.

    python scripts/time_prior.py --callable [--only MODE] [...]

The leg of a prior that no Prior(dists) states: uniform on the box (-10, 10)^32 cut by the joint constraint x0 < x1 + 5
(the Rosenbrock's mass lies inside), torch Rosenbrock on the device throughout, the same prior three ways --
``callable_host``: a numpy function the step calls on the host (x' and the finite mask cross PCIe, logp' comes back),
``callable_device``: the same function in torch through ``device_logprior`` (nothing crosses), ``uniform_table``: the
uniform(-10, 20)^32 ``Prior(dists)`` from the device's table, without the cut, as the baseline.  ``--only MODE`` runs one
mode (one warm-up call, then --repeats timed calls): the run to put under ``rocprofv3 --memory-copy-trace``, whose copies
per step are the difference of two runs with different --steps divided by the difference in steps."""
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
    ap.add_argument("--callable", action="store_true", help="time a joint prior as host function, GPU callable and table baseline")
    ap.add_argument("--only", default=None, help="with --callable: run this mode alone")
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

    if args.callable:
        return callable_leg(args, pmcmc, setups["uniform"], x, logl0, rosenbrock_torch)

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


CUT = 5.0


def joint_numpy(x):
    """log density (up to the constant both forms share) of the uniform box cut by x0 < x1 + CUT."""
    ok = np.ones(x.shape[0], dtype=bool)
    for j in range(x.shape[1]):
        ok = ok & (x[:, j] >= -10.0) & (x[:, j] <= 10.0)
    ok = ok & (x[:, 0] < x[:, 1] + CUT)
    return np.where(ok, 0.0, -np.inf)


def joint_torch(x):
    ok = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
    for j in range(x.shape[1]):
        ok = ok & (x[:, j] >= -10.0) & (x[:, j] <= 10.0)
    ok = ok & (x[:, 0] < x[:, 1] + CUT)
    zero = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device)
    return torch.where(ok, zero, torch.full_like(zero, float("-inf")))


def callable_leg(args, pmcmc, setup, x, logl0, rosenbrock_torch):
    table, scaler, flow, geo, u = setup
    D = x.shape[1]
    like = lambda xt: (rosenbrock_torch(xt), None)
    modes = dict(callable_host=(joint_numpy, {}), callable_device=(joint_torch, dict(device_logprior=True)),
                 uniform_table=(table.logpdf, {}))
    if args.only:
        modes = {args.only: modes[args.only]}

    def call(name):
        logprior, extra = modes[name]
        logp0 = table.logpdf(x) if name == "uniform_table" else joint_numpy(x)
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=logp0, beta=0.5, blobs=None)
        funcs = dict(loglike=like, logprior=logprior, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                    device_likelihood=True, **extra)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res
    out = dict(leg="callable", walkers=len(x), dim=D, flow="maf3", steps=args.steps, repeats=args.repeats,
               kind="preconditioned_pcn", gpu=torch.cuda.get_device_name(0))
    last = {name: call(name)[1] for name in modes}                  # warm-up
    rates = {name: [] for name in modes}
    for _ in range(args.repeats):                                   # the modes alternate
        for name in modes:
            r, last[name] = call(name)
            rates[name].append(r)
    for name, rs in rates.items():
        out[name] = dict(steps_per_s_best=max(rs), steps_per_s_median=float(np.median(rs)),
                         us_per_step_median=1e6 / float(np.median(rs)), all=rs, accept=float(last[name]["accept"]),
                         calls=int(last[name]["calls"]))
    if "callable_host" in last and "callable_device" in last:       # the two forms of the prior walk the same chain
        out["callable_device_equals_host"] = bool(all(np.array_equal(last["callable_host"][k], last["callable_device"][k])
                                                      for k in ("x", "logl", "logp")))
        out["device_over_host_callable"] = out["callable_device"]["steps_per_s_median"] / out["callable_host"]["steps_per_s_median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
