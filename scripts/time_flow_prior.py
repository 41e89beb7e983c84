"""What a flow prior (pocomc_amd.FlowPrior) costs: 1e4 walkers x 32 dimensions, maf3 and nsf6.

    python scripts/time_flow_prior.py [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3] [--calls 200] [--out FILE]
    python scripts/time_flow_prior.py --host [--walkers 10000] [--dim 32] [--steps 200] [--repeats 3]

Per flow:
  * microseconds per ``logpdf_device`` call (pre -> flow -> post) on the MCMC step's column-major view and on a C-contiguous
    block, next to the same flow's ``log_prob`` call alone on the float32 rows the prior hands it (``Flow.log_prob``: the
    forward kernel plus its two allocations): device events around --calls calls in a row, median of --repeats windows;
  * steps per second of one preconditioned tpCN kernel call of --steps steps with the torch Rosenbrock on the device
    (``device_likelihood=True``) and the flow prior inside the step (``device_logprior``), against the same call with the
    uniform(-10, 20)^32 ``Prior(dists)`` from the device's table: host clock around the call, the modes alternate, one
    warm-up call each, median of --repeats.
The flows carry their initial parameters: the kernels' time does not depend on the values.  One JSON line; --out writes a
readable table as well.

--host: the flow prior next to a HOST likelihood instead -- ``bench.py``'s numpy Rosenbrock on the pipelined step with the
lanes ``bench.py`` takes (two; the first 0.65 of the walkers for an affine flow, 0.82 for a spline flow), steps per second of
  * ``uniform_table``   the uniform(-10, 20)^32 ``Prior(dists)`` from the device's table,
  * ``host_route``      the flow prior through ``prior.logpdf`` on the host, once per lane and step,
  * ``step_prior``      the flow prior inside the step (kernel option ``step_prior``), every lane's stage behind the last
                        lane's pre-step,
  * ``step_prior_per_lane``  the same with every lane's stage right behind its own pre-step -- only with the measurement
                        library (``make DEBUG_HOOKS=1``, ``PMC_LIBRARY=.../libpocomc_amd_debug.so``), which has the switch;
one warm-up call each, then the modes alternate, --repeats calls each.  One JSON line per process: run it from several
processes in turn to see the spread between them (profiles/step_prior.txt)."""
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


def event_us(fn, calls, repeats):
    """Median over ``repeats`` windows of the device time of ``calls`` calls of ``fn`` in a row, per call, in microseconds."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / calls)
    return float(np.median(out)), out


def host_step_rates(name, priors, table, x, xs, args):
    """Steps per second of one pipelined kernel call with the numpy Rosenbrock for every mode of ``priors``
    (``mode -> (prior, extra kernel options, stage per lane)``) and for the uniform table: ``mode -> dict``."""
    import ctypes as C
    import pocomc_amd as pc
    from pocomc_amd import _lib, mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from bench import rosenbrock
    D = x.shape[1]
    scaler = pc.Reparameterize(D, bounds=table.bounds)
    scaler.fit(xs)
    u = scaler.forward(x)
    flow = pc.Flow(D, name, seed=0)
    geo = Geometry()
    geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
    like = lambda v: (rosenbrock(v), None)
    logl0 = rosenbrock(x)
    first = 0.82 if flow.spec.univariate == "rqs" else 0.65              # bench.py's --first-lane default for these flows
    lib = _lib.load()
    switch = getattr(lib, "pmc_debug_set_stage_per_lane", None)          # (the measurement library only)
    modes = dict(uniform_table=(table, {}, False), **priors)
    if switch is None:
        modes = {m: v for m, v in modes.items() if not v[2]}
    else:
        switch.restype, switch.argtypes = None, [C.c_int]

    def call(mode):
        prior, extra, per_lane = modes[mode]
        if switch is not None:
            switch(int(per_lane))
        state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x), beta=0.5,
                     blobs=None)
        funcs = dict(loglike=like, logprior=prior.logpdf, scaler=scaler, flow=flow, theta_geometry=geo)
        opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                    x_order="F", lanes=2, first_lane=first, host_prefetch=1, **extra)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pmcmc.preconditioned_pcn(state, funcs, opts)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert res["steps"] == args.steps
        return res["steps"] / dt, res
    old = np.setbufsize(1024)                                           # (as bench.py does for lanes below 8192 rows)
    try:
        last = {m: call(m)[1] for m in modes}                           # warm-up
        rates = {m: [] for m in modes}
        for _ in range(args.repeats):                                   # the modes alternate
            for m in modes:
                r, last[m] = call(m)
                rates[m].append(r)
    finally:
        np.setbufsize(old)
        if switch is not None:
            switch(0)
    stepped = [m for m in modes if m.startswith("step_prior")]
    for m in stepped:                                                   # the same trajectory, bit for bit
        for k in ("x", "logp", "logl"):
            assert np.array_equal(last[m][k], last["host_route"][k]), (m, k)
        assert last[m]["calls"] == last["host_route"]["calls"]
    return {m: dict(steps_per_s_median=float(np.median(rs)), all=[round(r, 1) for r in rs], accept=float(last[m]["accept"]),
                    calls=int(last[m]["calls"]), evaluations=int(last[m]["evaluations"])) for m, rs in rates.items()}


def host_main(args):
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import _lib
    N, D = args.walkers, args.dim
    table = pc.Prior([uniform(-10, 20)] * D)
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))
    out = dict(mode="host likelihood", walkers=N, dim=D, steps=args.steps, repeats=args.repeats, kind="preconditioned_pcn",
               library=os.path.basename(_lib.LIB_PATH), gpu=torch.cuda.get_device_name(0), flows={})
    for name in args.flows.split(","):
        scaler = pc.Reparameterize(D, bounds=table.bounds)
        scaler.fit(xs)
        prior = pc.FlowPrior(pc.Flow(D, name, seed=0), scaler)
        priors = dict(host_route=(prior, {}, False), step_prior=(prior, dict(step_prior=True), False),
                      step_prior_per_lane=(prior, dict(step_prior=True), True))
        out["flows"][name] = host_step_rates(name, priors, table, x, xs, args)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--flows", default="maf3,nsf6")
    ap.add_argument("--out", default=None)
    ap.add_argument("--host", action="store_true", help="the flow prior next to a host likelihood (see the module's text)")
    args = ap.parse_args()
    if args.host:
        return host_main(args)
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from time_device_likelihood import rosenbrock_torch

    N, D = args.walkers, args.dim
    table = pc.Prior([uniform(-10, 20)] * D)
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))                # (the scaler's standardisation: the walkers' region)
    xt = torch.from_numpy(x).cuda()
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    out = dict(walkers=N, dim=D, steps=args.steps, repeats=args.repeats, calls=args.calls, kind="preconditioned_pcn",
               gpu=torch.cuda.get_device_name(0), flows={})
    for name in args.flows.split(","):
        scaler = pc.Reparameterize(D, bounds=table.bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(D, name, seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        prior = pc.FlowPrior(flow, scaler)
        colmajor = xt.t().contiguous().t()
        u32 = torch.from_numpy(u).float().cuda()
        assert bool(torch.isfinite(prior.logpdf_device(xt)).all())
        assert torch.equal(prior.logpdf_device(xt), prior.logpdf_device(colmajor))
        row = {}
        for key, fn in (("logpdf_device_colmajor_us", lambda: prior.logpdf_device(colmajor)),
                        ("logpdf_device_contiguous_us", lambda: prior.logpdf_device(xt)),
                        ("flow_log_prob_us", lambda: prior.flow.log_prob(u32))):
            row[key], row[key + "_all"] = event_us(fn, args.calls, args.repeats)
        modes = dict(flow_prior=(prior.logpdf_device, dict(device_logprior=True), prior.logpdf(x)),
                     uniform_table=(table.logpdf, {}, table.logpdf(x)))

        def call(mode):
            logprior, extra, logp0 = modes[mode]
            state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=logp0.copy(), beta=0.5,
                         blobs=None)
            funcs = dict(loglike=like, logprior=logprior, scaler=scaler, flow=flow, theta_geometry=geo)
            opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                        device_likelihood=True, **extra)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pmcmc.preconditioned_pcn(state, funcs, opts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res["steps"] == args.steps
            return res["steps"] / dt, res
        last = {m: call(m)[1] for m in modes}                           # warm-up
        rates = {m: [] for m in modes}
        for _ in range(args.repeats):                                   # the modes alternate
            for m in modes:
                r, last[m] = call(m)
                rates[m].append(r)
        for m, rs in rates.items():
            row[m] = dict(steps_per_s_median=float(np.median(rs)), us_per_step_median=1e6 / float(np.median(rs)), all=rs,
                          accept=float(last[m]["accept"]), calls=int(last[m]["calls"]))
        assert np.isfinite(last["flow_prior"]["logp"]).all()
        row["flow_prior_over_uniform_table"] = row["flow_prior"]["steps_per_s_median"] / row["uniform_table"]["steps_per_s_median"]
        out["flows"][name] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_flow_prior.py --walkers {N} --dim {D} --steps {args.steps} --repeats {args.repeats} "
                    f"--calls {args.calls}   ({out['gpu']})\n")
            f.write("medians of the repeats; us per call from device events, steps/s from a host clock around a synchronised call\n\n")
            f.write(f"{'flow':6s} {'logpdf_device col-major':>24s} {'C-contiguous':>14s} {'Flow.log_prob alone':>20s}   "
                    f"{'step, flow prior':>18s} {'step, uniform table':>20s} {'ratio':>6s}\n")
            for name, r in out["flows"].items():
                f.write(f"{name:6s} {r['logpdf_device_colmajor_us']:21.1f} us {r['logpdf_device_contiguous_us']:11.1f} us "
                        f"{r['flow_log_prob_us']:17.1f} us   {r['flow_prior']['steps_per_s_median']:12.1f} st/s "
                        f"{r['uniform_table']['steps_per_s_median']:15.1f} st/s {r['flow_prior_over_uniform_table']:6.3f}\n")
            f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
