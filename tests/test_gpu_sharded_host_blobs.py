"""Blobs of a vectorised host likelihood on sharded walkers, one process per GPU: each rank's likelihood sees its own rows,
each rank's move launches follow its accepts, and the Sampler's ranks all-gather the walkers' blobs (and the warm-up
block's) so that every rank holds the same pool.  The invariant of ``tests/test_gpu_host_blobs.py``: every row carries g(x),
bit for bit.

Two ranks on one GPU over ``gloo``, started like the ranks of ``tests/test_gpu_sharded_device_blobs.py``: two processes
next to the test's own; every rank's process ends itself after ``LIMIT`` seconds (SIGALRM)."""
import signal

import numpy as np
import pytest

from .test_gpu_host_blobs import DS, g, gauss
from .test_gpu_sharded_device_blobs import LIMIT, _spawn
from .test_gpu_sharded_device_likelihood import WAIT, _done, _init, skip_unless_gpus_for


def _sampler_worker(rank, world, port, out):
    signal.alarm(LIMIT)
    dist = _init(rank, world, port)
    from scipy.stats import uniform
    import pocomc_amd as pc
    prior = pc.Prior([uniform(-5, 10)] * DS)
    rows = []

    def like(x):
        rows.append(len(x))
        return gauss(x), g(x)
    mk = lambda blobs: pc.Sampler(prior=prior, likelihood=like if blobs else gauss, vectorize=True,
                                  blobs_dtype=float if blobs else None, flow="maf3", n_active=64, n_effective=128,
                                  random_state=3, train_config=dict(epochs=30),
                                  mcmc_options=dict(x_order="F", lanes=2, wait_timeout=WAIT))
    s = mk(True)
    assert s.world == world and s.rank == rank
    s.run(n_total=256, n_evidence=256, progress=False)
    assert max(rows[:4]) == 64 // world                     # the warm-up blocks: this rank's share of the rows only
    x, w, logl, logp, b = s.posterior(return_blobs=True, trim_importance_weights=False)
    assert s.particles.blob_rows().is_cuda and s.walkers["blobs"].is_cuda
    res = s.results
    plain = mk(False)
    plain.run(n_total=256, n_evidence=256, progress=False)
    xp, wp, _, _ = plain.posterior(trim_importance_weights=False)
    np.savez(out % rank, x=x, w=w, b=b, calls=s.calls, logz=s.evidence()[0], rx=res["x"], rb=res["blobs"],
             wx=s.walkers["x"].cpu().numpy(), wb=s.walkers["blobs"].cpu().numpy(), xp=xp, wp=wp, callsp=plain.calls,
             logzp=plain.evidence()[0])
    _done(dist)


@pytest.mark.gpu
def test_two_rank_sampler_with_blobs_of_a_vectorised_host_likelihood(tmp_path):
    """Both ranks hold the same results and the same blobs, g of the rows they belong to -- pool and walkers; the run without
    blobs is the same run."""
    skip_unless_gpus_for(2)
    out = str(tmp_path / "rank%d.npz")
    _spawn(_sampler_worker, 2, out)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    for k in ("x", "w", "b", "rx", "rb", "wx", "wb", "calls", "logz"):
        assert np.array_equal(r0[k], r1[k]), k
    assert r0["b"].shape == (len(r0["x"]), 3) and r0["b"].dtype == np.float64
    assert np.array_equal(r0["b"], g(r0["x"]))
    assert np.array_equal(r0["rb"].reshape(-1, 3), g(r0["rx"].reshape(-1, DS)))
    assert np.array_equal(r0["wb"], g(r0["wx"]))
    assert np.array_equal(r0["x"], r0["xp"]) and np.array_equal(r0["w"], r0["wp"])
    assert int(r0["calls"]) == int(r0["callsp"]) and float(r0["logz"]) == float(r0["logzp"])
