"""What a joint prior (pocomc_amd.JointPrior) costs next to the composition a user could write without it: 1e4 walkers x 32
dimensions, a flow prior on 24 of them and scipy factors on the other 8, maf3 and nsf6.

    python scripts/time_joint_prior.py [--walkers 10000] [--dim 32] [--flow-dim 24] [--steps 200] [--repeats 3] [--calls 200]
                                       [--out FILE]
    python scripts/time_joint_prior.py --host [--walkers 10000] [--dim 32] [--flow-dim 24] [--steps 200] [--repeats 3]
    python scripts/time_joint_prior.py --blocks [--host] [--walkers 10000] [--steps 200] [--repeats 3] [--calls 200] [--out FILE]

The two priors compute the same density:
  * ``joint``:     ``JointPrior.logpdf_device`` -- three launches, one pass over x;
  * ``composed``:  a ``DevicePrior`` whose function gathers the flow columns out of x with torch (a contiguous copy), calls
                   ``FlowPrior.logpdf_device`` on the copy and restates the factors (uniform, normal, gamma) in torch.
Per flow:
  * microseconds per ``logpdf_device`` call on the MCMC step's column-major view and on a C-contiguous block: device events
    around --calls calls in a row, median of --repeats windows; next to them the flow block's ``Flow.log_prob`` call alone on
    the float32 rows the prior hands it (the forward kernel plus its two allocations);
  * steps per second of one preconditioned tpCN kernel call of --steps steps with the torch Rosenbrock on the device
    (``device_likelihood=True``) and the prior inside the step (``device_logprior``): host clock around the call, the two
    priors alternate, one warm-up call each, median of --repeats.
The flows carry their initial parameters: the kernels' time does not depend on the values.  One JSON line; --out writes a
readable table as well.

--host: the joint prior next to a HOST likelihood -- the modes and the settings of ``scripts/time_flow_prior.py --host``
(``uniform_table``, ``host_route``, ``step_prior`` and, with the measurement library, ``step_prior_per_lane``), one JSON
line per process.

--blocks: the blocks form -- 32 columns as two flow blocks of 12 and 8 factors (``profiles/joint_prior_blocks.txt``).  Per flow
(maf3, nsf6; both blocks the same kind): one ``JointPrior.logpdf_device`` call in both layouts, the sum of the two blocks'
``Flow.log_prob`` calls alone, the same prior written as a ``DevicePrior`` in torch (two gathers, two
``FlowPrior.logpdf_device`` calls, the factors restated), and the 200-step device-likelihood call for both forms.  With --host:
the two-lane pipelined step with the numpy Rosenbrock, the prior inside the step (``step_prior``) and on the host route."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def rest_factors(Dr):
    """``Dr`` frozen scipy factors (uniform, normal, gamma, cycled) and the same factors as a torch function of the
    ``(n, Dr)`` block of their columns."""
    from scipy.stats import gamma, norm, uniform
    kinds = [("uniform", (-10.0, 20.0, 0.0)), ("norm", (0.0, 3.0, 0.0)), ("gamma", (-3.0, 1.5, 2.0))]
    spec = [kinds[m % len(kinds)] for m in range(Dr)]
    dists = [uniform(loc, scale) if k == "uniform" else norm(loc, scale) if k == "norm" else gamma(a, loc=loc, scale=scale)
             for k, (loc, scale, a) in spec]

    def torch_logpdf(xr):
        lp = torch.zeros(xr.shape[0], dtype=torch.float64, device=xr.device)
        for m, (k, (loc, scale, a)) in enumerate(spec):
            v = xr[:, m]
            if k == "uniform":
                lp = lp + torch.where((v >= loc) & (v <= loc + scale), torch.full_like(v, -math.log(scale)), -math.inf)
            elif k == "norm":
                z = (v - loc) / scale
                lp = lp + (-(z * z) / 2.0 - 0.5 * math.log(2.0 * math.pi)) - math.log(scale)
            else:
                z = (v - loc) / scale
                t = torch.xlogy(torch.full_like(z, a - 1.0), z) - z - math.lgamma(a) - math.log(scale)
                lp = lp + torch.where(z >= 0, t, -math.inf)
        return lp
    return dists, torch_logpdf


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


def host_main(args):
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import _lib
    from time_flow_prior import host_step_rates
    N, D, Df = args.walkers, args.dim, args.flow_dim
    columns = np.random.default_rng(0).permutation(D)[:Df]
    flow_cols, _ = pc.JointPrior.layout(columns, Df, D - Df)
    rest = pc.Prior(rest_factors(D - Df)[0], device=True)
    table = pc.Prior([uniform(-10, 20)] * D)
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))
    out = dict(mode="host likelihood", walkers=N, dim=D, flow_dim=Df, steps=args.steps, repeats=args.repeats,
               kind="preconditioned_pcn", library=os.path.basename(_lib.LIB_PATH), gpu=torch.cuda.get_device_name(0), flows={})
    for name in args.flows.split(","):
        block_scaler = pc.Reparameterize(Df, bounds=np.array([[-10.0, 10.0]] * Df))
        block_scaler.fit(xs[:, flow_cols])
        joint = pc.JointPrior(pc.FlowPrior(pc.Flow(Df, name, seed=0), block_scaler), flow_cols.tolist(), rest)
        priors = dict(host_route=(joint, {}, False), step_prior=(joint, dict(step_prior=True), False),
                      step_prior_per_lane=(joint, dict(step_prior=True), True))
        out["flows"][name] = host_step_rates(name, priors, table, x, xs, args)
    print(json.dumps(out))


BLOCKS = (12, 12)            # --blocks: two flow blocks of the 32 columns; the other 8 carry factors


def blocks_parts(name, D, xs):
    """The two flow blocks (``Flow(12, name)`` on interleaved columns, each under a scaler of its own), the table and its torch
    restatement, the blocks prior and the same density composed in torch."""
    import pocomc_amd as pc
    perm = np.random.default_rng(0).permutation(D)
    columns = [perm[:BLOCKS[0]].tolist(), perm[BLOCKS[0]:sum(BLOCKS)].tolist()]
    maps, rest_cols = pc.JointPrior.layout_blocks(columns, BLOCKS, D - sum(BLOCKS))
    dists, rest_torch = rest_factors(D - sum(BLOCKS))
    rest = pc.Prior(dists, device=True)
    blocks = []
    for b, m in enumerate(maps):
        sc = pc.Reparameterize(len(m), bounds=np.array([[-10.0, 10.0]] * len(m)))
        sc.fit(xs[:, m])
        blocks.append(pc.FlowPrior(pc.Flow(len(m), name, seed=b), sc))
    joint = pc.JointPrior(blocks, columns, rest)
    idx = [torch.from_numpy(m).long().cuda() for m in maps]
    rc = torch.from_numpy(rest_cols).long().cuda()

    def composed_device(t):
        return (blocks[0].logpdf_device(t[:, idx[0]].contiguous()) + blocks[1].logpdf_device(t[:, idx[1]].contiguous())) \
            + rest_torch(t[:, rc])
    composed = pc.DevicePrior(composed_device, joint.bounds, joint.rvs)
    return joint, composed, blocks, maps


def blocks_main(args):
    import pocomc_amd as pc
    from pocomc_amd import _lib, mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    N, D = args.walkers, 32
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))
    out = dict(mode="blocks" + (", host likelihood" if args.host else ""), walkers=N, dim=D, blocks=list(BLOCKS),
               rest_dim=D - sum(BLOCKS), steps=args.steps, repeats=args.repeats, calls=args.calls, kind="preconditioned_pcn",
               library=os.path.basename(_lib.LIB_PATH), gpu=torch.cuda.get_device_name(0), flows={})
    if args.host:
        from scipy.stats import uniform
        from time_flow_prior import host_step_rates
        table = pc.Prior([uniform(-10, 20)] * D)
        for name in args.flows.split(","):
            joint = blocks_parts(name, D, xs)[0]
            priors = dict(host_route=(joint, {}, False), step_prior=(joint, dict(step_prior=True), False))
            out["flows"][name] = host_step_rates(name, priors, table, x, xs, args)
        print(json.dumps(out))
        return
    from time_device_likelihood import rosenbrock_torch
    xt = torch.from_numpy(x).cuda()
    colmajor = xt.t().contiguous().t()
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    for name in args.flows.split(","):
        joint, composed, blocks, maps = blocks_parts(name, D, xs)
        a, b = joint.logpdf_device(xt), composed.logpdf_device(xt)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, joint.logpdf_device(colmajor))
        assert float((a - b).abs().max()) <= 1e-9 * float(a.abs().max())           # the same density
        row = {}
        for who, prior in (("blocks", joint), ("composed", composed)):
            for lay, t in (("colmajor", colmajor), ("contiguous", xt)):
                key = f"{who}_{lay}_us"
                row[key], row[key + "_all"] = event_us(lambda: prior.logpdf_device(t), args.calls, args.repeats)
        u32 = [torch.from_numpy(fp.scaler.forward(x[:, m])).float().cuda() for fp, m in zip(blocks, maps)]
        key = "flow_log_prob_sum_us"
        row[key], row[key + "_all"] = event_us(lambda: (blocks[0].flow.log_prob(u32[0]), blocks[1].flow.log_prob(u32[1])),
                                               args.calls, args.repeats)
        scaler = pc.Reparameterize(D, bounds=joint.bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(D, name, seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        modes = dict(blocks=joint, composed=composed)

        def call(mode):
            prior = modes[mode]
            state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x), beta=0.5,
                         blobs=None)
            funcs = dict(loglike=like, logprior=prior.logpdf_device, scaler=scaler, flow=flow, theta_geometry=geo)
            opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                        device_likelihood=True, device_logprior=True)
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
            assert np.isfinite(last[m]["logp"]).all()
        row["blocks_over_composed"] = row["blocks"]["steps_per_s_median"] / row["composed"]["steps_per_s_median"]
        out["flows"][name] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_joint_prior.py --blocks --walkers {N} --steps {args.steps} --repeats {args.repeats} "
                    f"--calls {args.calls}   ({out['gpu']})\n")
            f.write("32 columns: two flow blocks of 12 on interleaved columns, 8 factors (uniform, normal, gamma)\n")
            f.write("medians of the repeats; us per call from device events, steps/s from a host clock around a synchronised call\n")
            f.write("blocks: JointPrior([a, c], ...).logpdf_device, 4 launches; composed: a DevicePrior with two torch gathers, "
                    "two FlowPrior.logpdf_device calls and the factors restated in torch\n\n")
            f.write(f"{'flow':6s} {'blocks col-major':>17s} {'blocks C-contig.':>17s} {'composed col-major':>18s} "
                    f"{'composed C-contig.':>19s} {'2 x Flow.log_prob':>18s}   {'step, blocks':>14s} {'step, composed':>16s} {'ratio':>6s}\n")
            for name, r in out["flows"].items():
                f.write(f"{name:6s} {r['blocks_colmajor_us']:14.1f} us {r['blocks_contiguous_us']:14.1f} us "
                        f"{r['composed_colmajor_us']:15.1f} us {r['composed_contiguous_us']:16.1f} us "
                        f"{r['flow_log_prob_sum_us']:15.1f} us   "
                        f"{r['blocks']['steps_per_s_median']:9.1f} st/s {r['composed']['steps_per_s_median']:11.1f} st/s "
                        f"{r['blocks_over_composed']:6.3f}\n")
            f.write("\n" + line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--flow-dim", type=int, default=24)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--flows", default="maf3,nsf6")
    ap.add_argument("--out", default=None)
    ap.add_argument("--host", action="store_true", help="the joint prior next to a host likelihood (see the module's text)")
    ap.add_argument("--blocks", action="store_true", help="the blocks form: 12 + 12 + 8 columns (see the module's text)")
    args = ap.parse_args()
    if args.blocks:
        return blocks_main(args)
    if args.host:
        return host_main(args)
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from time_device_likelihood import rosenbrock_torch

    N, D, Df = args.walkers, args.dim, args.flow_dim
    Dr = D - Df
    columns = np.random.default_rng(0).permutation(D)[:Df]               # the flow block: interleaved, not sorted
    flow_cols, rest_cols = pc.JointPrior.layout(columns, Df, Dr)
    dists, rest_torch = rest_factors(Dr)
    rest = pc.Prior(dists, device=True)
    rng = np.random.default_rng(0)
    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))                # (the scalers' standardisation: the walkers' region)
    xt = torch.from_numpy(x).cuda()
    colmajor = xt.t().contiguous().t()
    fc, rc = torch.from_numpy(flow_cols).long().cuda(), torch.from_numpy(rest_cols).long().cuda()
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    out = dict(walkers=N, dim=D, flow_dim=Df, rest_dim=Dr, steps=args.steps, repeats=args.repeats, calls=args.calls,
               kind="preconditioned_pcn", gpu=torch.cuda.get_device_name(0), flows={})
    for name in args.flows.split(","):
        block_scaler = pc.Reparameterize(Df, bounds=np.array([[-10.0, 10.0]] * Df))
        block_scaler.fit(xs[:, flow_cols])
        block = pc.FlowPrior(pc.Flow(Df, name, seed=0), block_scaler)
        joint = pc.JointPrior(block, flow_cols.tolist(), rest)

        def composed_device(t):
            return block.logpdf_device(t[:, fc].contiguous()) + rest_torch(t[:, rc])
        composed = pc.DevicePrior(composed_device, joint.bounds, joint.rvs)
        a, b = joint.logpdf_device(xt), composed.logpdf_device(xt)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, joint.logpdf_device(colmajor))
        assert float((a - b).abs().max()) <= 1e-9 * float(a.abs().max())           # the same density
        row = {}
        for who, prior in (("joint", joint), ("composed", composed)):
            for lay, t in (("colmajor", colmajor), ("contiguous", xt)):
                key = f"{who}_{lay}_us"
                row[key], row[key + "_all"] = event_us(lambda: prior.logpdf_device(t), args.calls, args.repeats)
        u32 = torch.from_numpy(block_scaler.forward(x[:, flow_cols])).float().cuda()
        key = "flow_log_prob_us"
        row[key], row[key + "_all"] = event_us(lambda: block.flow.log_prob(u32), args.calls, args.repeats)
        # the step: all D dimensions under the Sampler's own scaler and flow
        scaler = pc.Reparameterize(D, bounds=joint.bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(D, name, seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        modes = dict(joint=joint, composed=composed)

        def call(mode):
            prior = modes[mode]
            state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=prior.logpdf(x), beta=0.5,
                         blobs=None)
            funcs = dict(loglike=like, logprior=prior.logpdf_device, scaler=scaler, flow=flow, theta_geometry=geo)
            opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                        device_likelihood=True, device_logprior=True)
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
            assert np.isfinite(last[m]["logp"]).all()
        row["joint_over_composed"] = row["joint"]["steps_per_s_median"] / row["composed"]["steps_per_s_median"]
        out["flows"][name] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_joint_prior.py --walkers {N} --dim {D} --flow-dim {Df} --steps {args.steps} "
                    f"--repeats {args.repeats} --calls {args.calls}   ({out['gpu']})\n")
            f.write("medians of the repeats; us per call from device events, steps/s from a host clock around a synchronised call\n")
            f.write("joint: JointPrior.logpdf_device; composed: a DevicePrior that gathers with torch, calls "
                    "FlowPrior.logpdf_device and restates the factors in torch\n\n")
            f.write(f"{'flow':6s} {'joint col-major':>16s} {'joint C-contig.':>16s} {'composed col-major':>18s} "
                    f"{'composed C-contig.':>19s} {'Flow.log_prob alone':>20s}   {'step, joint':>14s} {'step, composed':>16s} {'ratio':>6s}\n")
            for name, r in out["flows"].items():
                f.write(f"{name:6s} {r['joint_colmajor_us']:13.1f} us {r['joint_contiguous_us']:13.1f} us "
                        f"{r['composed_colmajor_us']:15.1f} us {r['composed_contiguous_us']:16.1f} us "
                        f"{r['flow_log_prob_us']:17.1f} us   "
                        f"{r['joint']['steps_per_s_median']:9.1f} st/s {r['composed']['steps_per_s_median']:11.1f} st/s "
                        f"{r['joint_over_composed']:6.3f}\n")
            f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
