"""Every mode of the flow fit driver (pocomc_amd/train.py, fit_flow) on small seeded fits, one .npz per fit: loss and
validation-loss history, final parameters, inverse guard.  Two trees with the same library build give the same bytes, which
is how a change to the driver is checked against the commit before it.
    python scripts/fit_modes_dump.py OUTDIR            python scripts/fit_modes_dump.py --compare DIR_A DIR_B

D = 6, 96 rows, batches of 32 (three per training pass at validation_split=0.5, a partial last one at 0.7), 12 epochs;
weights, shuffle, validation_split=0.5, patience=10**6 unless the case says otherwise."""
import json
import os
import socket
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

D, ROWS = 6, 96
BASE = dict(epochs=12, batch_size=32, validation_split=0.5, patience=10 ** 6, annealing=False)
A, B = ("maf3", {}), ("nsf3", {})
CASES = {
    "a_maf3": A, "b_nsf3_side": B,
    "c_nsf3_annealing": ("nsf3", dict(annealing=True)),
    "d_unfused": ("maf3", dict(shuffle=False)), "d_unfused_unweighted": ("maf3", dict(shuffle=False, weights=None)),
    "e_no_validation": ("maf3", dict(validation_split=0.0)),
    "f_partial_batch": ("maf3", dict(validation_split=0.7)),
    "g_early_stop_maf3": ("maf3", dict(patience=2, epochs=40)), "g_early_stop_nsf3": ("nsf3", dict(patience=2, epochs=40)),
    "h_laplace": ("maf3", dict(laplace_scale=0.1)),
    "h_gaussian_no_validation": ("maf3", dict(gaussian_scale=0.1, validation_split=0.0)),
    "i_noise_maf3": ("maf3", dict(noise=0.1)), "i_noise_nsf3": ("nsf3", dict(noise=0.1)),
    "j_bf16": ("bf16", {}),
    # (a) on the narrowest flow family whose inverse takes the 16-bit lane sweep (D = 128, 8 transforms, as in
    # tests/test_gpu_config.py): the one case whose inverse_guard is not null
    "l_inverse_guard": ("lane16", {}),
}
SHARDED = ["a_maf3", "h_laplace", "h_gaussian_no_validation", "i_noise_maf3"]


def data(n_dim):
    rng = np.random.default_rng(11)
    x = (rng.normal(size=(ROWS, n_dim)) * np.linspace(0.5, 2.0, n_dim) + 0.3).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(rng.uniform(0.2, 1.0, size=ROWS).astype(np.float32))


def show_plan(f, n_rows, kw):
    """Print the plan the driver makes for these settings, where it has one to show (the one use of a private name here:
    the fits themselves go through ``Flow.fit`` alone, and the plan is built again, after the fit, only to be printed).
    The printed plan is NOT the object the fit used: it is derived a second time from the same settings, and would drift
    from the fit's if ``fit_flow`` came to prepare ``_FitPlan``'s arguments differently."""
    from pocomc_amd import train
    if hasattr(train, "_FitPlan"):
        split = kw["validation_split"]
        x_valid = torch.empty(n_rows - int(split * n_rows), 0) if split > 0.0 else None
        penalised = kw.get("laplace_scale") is not None or kw.get("gaussian_scale") is not None
        plan = train._FitPlan(f, x_valid, kw["batch_size"], kw.get("shuffle", True), penalised, kw["annealing"], None, None)
        print("    plan:", json.dumps(vars(plan), sort_keys=True), flush=True)


def run(name, out, rows=slice(None), **extra):
    from pocomc_amd import Flow
    from pocomc_amd.maf_spec import MAFSpec
    flow_name, kw = CASES[name]
    kw = {**BASE, **kw, **extra}
    torch.manual_seed(1234)
    if flow_name == "bf16":             # the smallest flow of tests/test_gpu_train_bf16.py on its bf16 engine
        f = Flow(5, MAFSpec(5, 3, hidden=32), seed=3, precision="bf16")
        f.train_engine = "bf16"
    elif flow_name == "lane16":
        f = Flow(128, MAFSpec(128, 8), seed=3, inverse_precision="bf16")
    else:
        f = Flow(D, flow_name, seed=3)
    x, w = data(f.n_dim)
    print(name, flush=True)
    h = f.fit(x[rows], weights=kw.pop("weights", w[rows]), **kw)
    show_plan(f, x[rows].shape[0], kw)
    np.savez(out, loss=np.array(h["loss"]), val_loss=np.array(h["val_loss"]), params=f.params.cpu().numpy(),
             inverse_guard=np.array(json.dumps(h.get("inverse_guard"), sort_keys=True, default=float)))


def worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for name in SHARDED:
        run(name, os.path.join(outdir, "k_sharded_%s_rank%d.npz" % (name, rank)), rows=slice(rank, None, world))
    dist.barrier()
    dist.destroy_process_group()


def compare(dir_a, dir_b):
    names = sorted(os.listdir(dir_a))
    assert names == sorted(os.listdir(dir_b)) and names, "the two directories hold different files"
    n_arrays, differ = 0, []
    for name in names:
        a, b = np.load(os.path.join(dir_a, name)), np.load(os.path.join(dir_b, name))
        assert sorted(a.files) == sorted(b.files)
        for key in a.files:
            n_arrays += 1
            if a[key].shape != b[key].shape or a[key].tobytes() != b[key].tobytes():
                worst = float(np.max(np.abs(a[key] - b[key]))) if a[key].shape == b[key].shape and a[key].dtype.kind == "f" else None
                differ.append((name, key, worst))
    print(json.dumps({"files": len(names), "arrays": n_arrays, "identical": n_arrays - len(differ), "differ": differ}))
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    for case in CASES:
        run(case, os.path.join(outdir, case + ".npz"))
    # k: two ranks that share the one GPU over gloo, each writing its own files; the spawn has its own time limit
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.spawn(worker, args=(2, port, outdir), nprocs=2, join=False)
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            sys.exit("the two ranks did not finish in time")
