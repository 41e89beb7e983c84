"""What the box of a truncated correlated normal prior (pocomc_amd.TruncatedGaussianPrior as a block of a pocomc_amd.JointPrior)
costs next to the untruncated prior of the same shape, and next to the same prior written as a ``DevicePrior`` in torch: 1e4
walkers x 32 dimensions, a 24-dimensional normal block on interleaved columns of which 4 columns are bounded (two below, two on
both sides), and uniform factors on the other 8.

    python scripts/time_gauss_box_prior.py [--walkers 10000] [--dim 32] [--gauss-dim 24] [--bounded 4] [--steps 200]
                                           [--repeats 5] [--calls 2000] [--flows maf3,nsf6] [--out profiles/gauss_box_prior.txt]

The priors, all in one process:
  * ``box``:    ``JointPrior([TruncatedGaussianPrior(mean, cov, bounds)], [columns], Prior(uniform factors)).logpdf_device`` -- one
                launch (``pmc_gauss_box_logpdf``), one pass over x;
  * ``gauss``:  the same with ``GaussianPrior(mean, cov)`` -- one launch (``pmc_gauss_blocks_logpdf``), the kernel's instance
                without the box test;
  * ``torch``:  ``box``'s density as a ``DevicePrior``: a gather, a subtraction, a matmul with the transposed inverse Cholesky
                factor, a square, a row sum, the box test, the uniform factors restated, the box's log mass subtracted;
  * ``box_alone`` / ``gauss_alone``: the 24-dimensional priors by themselves on the block's own (n, 24) array.
Measured:
  * microseconds per ``logpdf_device`` call on the MCMC step's column-major view and on a C-contiguous block: device events
    around --calls calls in a row after ten warm-up calls; the priors alternate, --repeats windows each, median and all;
  * per flow (the step's own flow over all 32 dimensions): steps per second of one preconditioned tpCN kernel call of --steps
    steps with the torch Rosenbrock on the device (``device_likelihood=True``), the prior inside the step
    (``device_logprior``): host clock around a synchronised call, the modes alternate, one warm-up call each, median of
    --repeats.
One JSON line; --out writes a readable table as well."""
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

from time_joint_prior import event_us                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--gauss-dim", type=int, default=24)
    ap.add_argument("--bounded", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--flows", default="maf3,nsf6")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scipy.stats import uniform
    import pocomc_amd as pc
    from pocomc_amd import mcmc as pmcmc
    from pocomc_amd.geometry import Geometry
    from time_device_likelihood import rosenbrock_torch

    N, D, K, nb = args.walkers, args.dim, args.gauss_dim, args.bounded
    Dr = D - K
    rng = np.random.default_rng(0)
    columns = rng.permutation(D)[:K]                                      # the block: interleaved, not sorted
    (cols,), rest_cols = pc.JointPrior.layout_blocks([columns], [K], Dr)
    # time_gauss_prior.py's covariance: a random orthogonal basis, eigenvalues log-spaced over a condition number of 100
    Q, _ = np.linalg.qr(rng.normal(size=(K, K)))
    cov = (Q * (4.0 * np.logspace(0.5, -1.5, K))) @ Q.T
    cov = 0.5 * (cov + cov.T)
    mean = rng.normal(size=K) * 0.5
    # the box: nb block columns spread over the block, alternately bounded below and on both sides; the walkers
    # (uniform(-2, 2)) lie inside it
    bounds = np.stack([np.full(K, -np.inf), np.full(K, np.inf)], axis=1)
    bounded = np.linspace(0, K - 1, nb).round().astype(int)
    for i, j in enumerate(bounded):
        bounds[j] = (-3.0, np.inf) if i % 2 == 0 else (-3.0, 3.5)
    t0 = time.perf_counter()
    boxed = pc.TruncatedGaussianPrior(mean, cov, bounds)
    construct_s = time.perf_counter() - t0
    plain = pc.GaussianPrior(mean, cov)
    own = pc.Prior([uniform(-10.0, 20.0)] * Dr)
    box = pc.JointPrior([boxed], [cols.tolist()], own)
    gauss = pc.JointPrior([plain], [cols.tolist()], own)

    blk = boxed.device_block()
    LinvT = torch.from_numpy(np.linalg.inv(np.linalg.cholesky(cov)).T.copy()).cuda()
    mean_t, lo_t, hi_t = (torch.from_numpy(blk[f]).cuda() for f in ("mean", "lo", "hi"))
    logc_box = float(blk["logc"])
    ci, ri = torch.from_numpy(cols).long().cuda(), torch.from_numpy(rest_cols).long().cuda()
    log_w = -Dr * math.log(20.0)

    def torch_device(t):
        xb = t[:, ci]
        y = (xb - mean_t) @ LinvT
        g = -0.5 * (y * y).sum(dim=1) - logc_box
        r = t[:, ri]
        inside = ((r >= -10.0) & (r <= 10.0)).all(dim=1) & ((xb >= lo_t) & (xb <= hi_t)).all(dim=1)
        return torch.where(inside, g + log_w, torch.full_like(g, -math.inf))
    composed = pc.DevicePrior(torch_device, box.bounds, box.rvs)

    x = rng.uniform(-2.0, 2.0, size=(N, D))
    xs = rng.uniform(-2.0, 2.0, size=(4 * N, D))                          # (the scaler's standardisation: the walkers' region)
    xt = torch.from_numpy(x).cuda()
    colmajor = xt.t().contiguous().t()
    xb = xt[:, ci].contiguous()
    xb_colmajor = xb.t().contiguous().t()
    a, b, c = box.logpdf_device(xt), composed.logpdf_device(xt), gauss.logpdf_device(xt)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, box.logpdf_device(colmajor))
    assert float((a - b).abs().max()) <= 1e-9 * float(a.abs().max())      # the same density
    assert float((a - (c - boxed.log_mass)).abs().max()) <= 1e-12 * float(a.abs().max())    # the untruncated one, shifted
    outside = np.array(x[:64])
    outside[:, cols[bounded[0]]] = -3.5
    assert bool(torch.isneginf(box.logpdf_device(torch.from_numpy(outside).cuda())).all())
    out = dict(walkers=N, dim=D, gauss_dim=K, bounded=int(nb), rest_dim=Dr, steps=args.steps, repeats=args.repeats,
               calls=args.calls, kind="preconditioned_pcn", gpu=torch.cuda.get_device_name(0), log_mass=boxed.log_mass,
               log_mass_spread=boxed.log_mass_spread, construct_s=construct_s, flows={})
    timed = {"box": (box, colmajor, xt), "gauss": (gauss, colmajor, xt), "torch": (composed, colmajor, xt),
             "box_alone": (boxed, xb_colmajor, xb), "gauss_alone": (plain, xb_colmajor, xb)}
    windows = {f"{who}_{lay}_us": [] for who in timed for lay in ("colmajor", "contiguous")}
    for _ in range(args.repeats):                                         # the priors alternate
        for who, (prior, cm, cc) in timed.items():
            for lay, t in (("colmajor", cm), ("contiguous", cc)):
                windows[f"{who}_{lay}_us"].append(event_us(lambda: prior.logpdf_device(t), args.calls, 1)[0])
    for key, w in windows.items():
        out[key], out[key + "_all"] = float(np.median(w)), w
    logl0 = rosenbrock_torch(xt).cpu().numpy()
    like = lambda t: (rosenbrock_torch(t), None)
    for name in args.flows.split(","):
        # the step: all D dimensions under the Sampler's own scaler and flow (the box's bounds for every mode)
        scaler = pc.Reparameterize(D, bounds=box.bounds)
        scaler.fit(xs)
        u = scaler.forward(x)
        flow = pc.Flow(D, name, seed=0)
        geo = Geometry()
        geo.fit(flow.forward(torch.from_numpy(u).float())[0].numpy().astype(np.float64))
        modes = dict(box=(box.logpdf_device, box.logpdf(x)), gauss=(gauss.logpdf_device, gauss.logpdf(x)),
                     torch=(composed.logpdf_device, composed.logpdf(x)))

        def call(mode):
            logprior, logp0 = modes[mode]
            state = dict(u=u.copy(), x=x.copy(), logdetj=scaler.inverse(u)[1], logl=logl0.copy(), logp=logp0.copy(), beta=0.5,
                         blobs=None)
            funcs = dict(loglike=like, logprior=logprior, scaler=scaler, flow=flow, theta_geometry=geo)
            opts = dict(n_max=args.steps, n_steps=10 ** 9, progress_bar=None, proposal_scale=2.38 / D ** 0.5, seed=3,
                        device_likelihood=True, device_logprior=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pmcmc.preconditioned_pcn(state, funcs, opts)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert res["steps"] == args.steps
            return res["steps"] / dt, res
        last = {m: call(m)[1] for m in modes}                             # warm-up
        rates = {m: [] for m in modes}
        for _ in range(args.repeats):                                     # the modes alternate
            for m in modes:
                r, last[m] = call(m)
                rates[m].append(r)
        row = {}
        for m, rs in rates.items():
            row[m] = dict(steps_per_s_median=float(np.median(rs)), us_per_step_median=1e6 / float(np.median(rs)), all=rs,
                          accept=float(last[m]["accept"]), calls=int(last[m]["calls"]))
            assert np.isfinite(last[m]["logp"]).all()
        row["box_over_gauss"] = row["box"]["steps_per_s_median"] / row["gauss"]["steps_per_s_median"]
        row["box_over_torch"] = row["box"]["steps_per_s_median"] / row["torch"]["steps_per_s_median"]
        out["flows"][name] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(f"scripts/time_gauss_box_prior.py --walkers {N} --dim {D} --gauss-dim {K} --bounded {nb} --steps {args.steps} "
                    f"--repeats {args.repeats} --calls {args.calls}   ({out['gpu']})\n")
            f.write(f"{D} columns: a {K}-dimensional normal block on interleaved columns (condition number 100), {nb} of its columns "
                    f"bounded, {Dr} uniform factors\n")
            f.write(f"the box's log mass {boxed.log_mass:.9f}, spread {boxed.log_mass_spread:.2e}; the constructor took "
                    f"{construct_s:.2f} s on the host\n")
            f.write("medians of the repeats (all windows in the JSON line); us per call from device events around --calls calls, "
                    "the priors alternating; steps/s from a host clock around a synchronised call\n")
            f.write("box: JointPrior([TruncatedGaussianPrior], ...), one launch; gauss: JointPrior([GaussianPrior], ...), one launch; "
                    "torch: box's density as a DevicePrior; *_alone: the 24-column priors by themselves\n\n")
            f.write(f"{'one logpdf_device call':24s} {'col-major':>12s} {'min .. max':>18s} {'C-contig.':>12s} {'min .. max':>18s}\n")
            for who in timed:
                cm, cc = out[who + "_colmajor_us_all"], out[who + "_contiguous_us_all"]
                f.write(f"{who:24s} {out[who + '_colmajor_us']:9.2f} us {min(cm):8.2f} .. {max(cm):6.2f} "
                        f"{out[who + '_contiguous_us']:9.2f} us {min(cc):8.2f} .. {max(cc):6.2f}\n")
            f.write(f"\n{'flow':6s} {'step, box':>16s} {'step, gauss':>16s} {'step, torch':>16s} {'box / gauss':>12s} {'box / torch':>12s}"
                    f"   (min .. max of box; of gauss)\n")
            for name, r in out["flows"].items():
                f.write(f"{name:6s} {r['box']['steps_per_s_median']:11.1f} st/s {r['gauss']['steps_per_s_median']:11.1f} st/s "
                        f"{r['torch']['steps_per_s_median']:11.1f} st/s {r['box_over_gauss']:12.3f} {r['box_over_torch']:12.3f}"
                        f"   ({min(r['box']['all']):.0f} .. {max(r['box']['all']):.0f}; {min(r['gauss']['all']):.0f} .. "
                        f"{max(r['gauss']['all']):.0f})\n")
            f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
