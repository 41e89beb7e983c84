"""What runs downstream of the gradient in ``pmc_maf_train_epoch`` -- the sums of squares ``maf_dw_kernel`` leaves in
``sq_partial``, the clip coefficient, ``adamw_kernel``, the refresh of both kernel images, the snapshot -- against the float64 model of ``tests/optimizer_model.py``, by direct library calls with explicit batches.

``bound`` is derived there from the kernel's operation count and fixed on the CPU (``tests/test_optimizer_model_cpu.py``:
the float32 twin stays within half of it); nothing here widens it.  The largest deviation-to-bound ratio of every family
is printed (``-s``) and recorded in ``profiles/optimizer_epoch.txt``.

The gate of ``pmc_maf_train_epoch_gated`` has no test here: a validation pass long enough to outlast the first batch's
launches fills the device, the epoch's launches wait behind it, and the pass's loss comes out the same with
``gate_event = NULL`` (measured at 50000 .. 800000 rows, same file) -- a test that cannot fail."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cases
import flow_instances as fi
import optimizer_model as om
from pocomc_amd.maf_spec import MAFSpec

pytestmark = pytest.mark.gpu

FLOWS = {
    "maf3-d10": (("maf3", 10), False),
    "nsf3-d10": (("nsf3", 10), False),                      # 8 bins, one padding job
    "rqs4-d10": ((10, 2, 64, "rqs", 4), False),
    "rqs16-d10": ((10, 2, 64, "rqs", 16), False),
    "maf3-d32": (MAFSpec(32, 3), False),                    # 136512 parameters: a second trip through the stride loop
    "rqs16-d20": ((20, 2, 128, "rqs", 16), False),          # 313944 parameters, 862 jobs
    "maf3-d10-lean": (("maf3", 10), True),
    "nsf3-d10-lean": (("nsf3", 10), True),
}
BATCH = 40
PARTIAL_RTOL = 16 * 2.0 ** -24          # a partial is at most about 12 float32 roundings of positive terms
RATIO = {}                              # family -> largest deviation / bound seen in this session


def note(family, r):
    RATIO[family] = max(RATIO.get(family, 0.0), float(r))
    return r


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIO):
        print(f"\noptimizer epoch, largest deviation / bound, {k}: {RATIO[k]:.3f}", end="")


def data(D, n, weighted, seed=0):
    rng = np.random.default_rng([seed, D, n])
    x = torch.from_numpy((rng.normal(size=(n, D)) * 1.5).astype(np.float32)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32)).cuda() if weighted else None
    return x, w


class Rig:
    """One flow with its training state and an optimizer descriptor of its own: ``pmc_maf_train_epoch`` through ctypes."""

    def __init__(self, key, set_cap=None):
        from pocomc_amd import Flow, _lib
        from pocomc_amd.train import _train_state
        s, lean = FLOWS[key]
        self.spec = spec = fi.make_spec(s)
        self.flat = torch.from_numpy(cases.flow_params(spec, 3))
        self.f = f = Flow(spec.n_dim, spec, seed=0)
        if lean:
            f.lean_lds = True
        self.ts = ts = _train_state(f)
        if set_cap is not None:
            assert ts.n_sets == 0
            ts.set_cap = set_cap
        ts.ensure_sets(100)
        self.lib, self._lib = f.lib, _lib
        self.m, self.v = torch.zeros_like(f.params), torch.zeros_like(f.params)
        self.acc = torch.zeros(1, dtype=torch.float32, device="cuda")
        self.sc_ptr, self.sc_dst = ts.scatter_maps(f)
        self.padding = ts.jobs.cpu().numpy().reshape(-1, 8)[:, 0] < 0
        self.desc = _lib.pmc_adamw_t(
            params=f.params.data_ptr(), grad=ts.grad.data_ptr(), exp_avg=self.m.data_ptr(), exp_avg_sq=self.v.data_ptr(),
            n_params=f.params.numel(), pack_idx=f._pack_idx.data_ptr(), packed=f._packed.data_ptr(),
            n_packed=f._packed.numel(), packT_idx=ts.packT_idx.data_ptr(), packedT=ts.packedT.data_ptr(),
            n_packedT=ts.packedT.numel(), beta1=0.9, beta2=0.999, eps=1e-8)
        self.reset()

    def reset(self, step=0, scatter=True):
        self.f.set_params(self.flat, check=False)
        self.ts.repack(self.f)
        self.m.zero_(), self.v.zero_(), self.acc.zero_()
        self.desc.step = step
        self.desc.scatter_ptr = self.sc_ptr.data_ptr() if scatter else None
        self.desc.scatter_dst = self.sc_dst.data_ptr() if scatter else None
        return self

    def epoch(self, x, w, perm, n, bs, lr=1e-3, wd=0.0, max_norm=1.0, snapshot=None):
        d, p = self.desc, self._lib.ptr
        d.lr, d.weight_decay, d.max_norm = lr, wd, max_norm
        d.snapshot = snapshot.data_ptr() if snapshot is not None else None
        self._lib.check(self.lib.pmc_maf_train_epoch(C.byref(self.f._desc), C.byref(self.ts.desc), C.byref(d), p(x), p(w), p(perm), n, bs,
                                                     p(self.acc), self._lib.stream_handle()), "pmc_maf_train_epoch")

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.f.params, self.m, self.v))

    def images(self):
        return self.f._packed.cpu().numpy().copy(), self.ts.packedT.cpu().numpy().copy()

    def everything(self):
        return self.state() + self.images() + (self.acc.cpu().numpy().copy(),)

    def gradient(self):
        return self.ts.grad.cpu().numpy().copy(), self.ts.sq_partial[:self.ts.n_jobs].cpu().numpy().copy()

    def fresh_images(self):
        """Both images from ``pmc_maf_pack`` of the parameters into new buffers (NaN first: every position is written)."""
        out = []
        for idx in (self.f._pack_idx, self.ts.packT_idx):
            img = torch.full((idx.numel(),), float("nan"), dtype=torch.float32, device="cuda")
            self._lib.check(self.lib.pmc_maf_pack(self._lib.ptr(self.f.params), self._lib.ptr(idx), self._lib.ptr(img), img.numel(),
                                                  self._lib.stream_handle()), "pmc_maf_pack")
            out.append(img.cpu().numpy())
        return out


@functools.lru_cache(maxsize=None)
def rig(key, set_cap=None):
    return Rig(key, set_cap)


def same(a, b, what=""):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and np.array_equal(u.view(np.uint32), v.view(np.uint32)), f"{what}: item {i} differs in its bits"


def check_partials(r, g, part, tag):
    """Every unmasked entry of the final gradient is squared into exactly one partial; padding jobs write 0."""
    assert part.shape == r.padding.shape and not part[r.padding].any(), f"{tag}: a padding job's partial is not 0"
    S, G = part.astype(np.float64).sum(), (g.astype(np.float64) ** 2).sum()
    assert not g[r.spec.mask_flat() == 0].any()
    assert G > 0 and abs(S - G) <= PARTIAL_RTOL * G, f"{tag}: sum of partials {S!r} against |grad|^2 {G!r}: {abs(S - G) / G:.3e}"
    return abs(S - G) / G / PARTIAL_RTOL


def check_step(r, before, g, part, step, lr, wd, max_norm, tag, family):
    sc = om.scalars(step, lr, wd, max_norm)
    want, bnd = om.step64(*before[:1], g, *before[1:], sc, part), om.bound(before[0], g, before[1], before[2], sc, part)
    ratio = note(family, om.worst_ratio(r.state(), want, bnd))
    assert ratio <= 1.0, f"{tag}: p, m, v leave the bound of the float64 step: {ratio:.3f}"
    return ratio


def check_images(r, tag):
    same(r.images(), r.fresh_images(), f"{tag}: kernel images against pmc_maf_pack of the parameters")


def teacher_forced(r, x, w, n, combos, tag, family, step0=0, lrs=(1e-3, 1e-3, 1e-3), scatter=True):
    """One batch per call over the rows of ``x``; after every call the partials, the step and both images are checked.
    Returns, per combination, the state after every call and the accumulated loss."""
    out = {}
    for wd, max_norm in combos:
        r.reset(step0, scatter)
        trail = []
        for k, b0 in enumerate(range(0, n, BATCH)):
            nb = min(BATCH, n - b0)
            before = r.state()
            r.epoch(x[b0:b0 + nb], None if w is None else w[b0:b0 + nb], None, nb, nb, lrs[k], wd, max_norm)
            g, part = r.gradient()
            t = f"{tag} wd={wd} max_norm={max_norm} batch {k}"
            note("partials", check_partials(r, g, part, t))
            assert r.desc.step == step0 + k + 1
            check_step(r, before, g, part, step0 + k + 1, lrs[k], wd, max_norm, t, family)
            check_images(r, t)
            trail.append(r.state() + r.images())
        out[(wd, max_norm)] = (trail, r.acc.cpu().numpy().copy())
    return out


COMBOS = [(wd, mn) for wd in (0.0, 0.01) for mn in (1.0, 0.0, 1e9)]


# ------------------------------------------------------------------------------------- (a), (c), (d): teacher-forced steps
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [100, 81])
@pytest.mark.parametrize("key", list(FLOWS))
def test_teacher_forced_steps_partials_images_and_the_single_call(key, n, weighted):
    """(a) three one-batch calls (40, 40, 20 rows; n = 81: 40, 40, 1), state carried forward: the partials add up to the device gradient's
    squared norm, ``p, m, v`` are within ``bound`` of ``step64`` on the device gradient and partials, (c) both images are
    ``pmc_maf_pack`` of the parameters bit for bit -- by the scatter map and by ``pack2_kernel``, which also give the same
    ``p, m, v`` --, ``max_norm = 1e9`` (a norm below it) gives the bits of ``max_norm = 0``, and (d) ONE call over all rows
    gives the bits of the three calls, loss included."""
    r = rig(key)
    x, w = data(r.spec.n_dim, n, weighted)
    tag = f"{key} n={n} w={int(weighted)}"
    by_scatter = teacher_forced(r, x, w, n, COMBOS, tag, "a: epoch step")
    for wd in (0.0, 0.01):
        for (ta, la), (tb, lb) in [(by_scatter[(wd, 0.0)], by_scatter[(wd, 1e9)])]:
            for a, b in zip(ta, tb):
                same(a, b, f"{tag} wd={wd}: max_norm 1e9 against 0")
            same([la], [lb], f"{tag}: loss")
    by_pack2 = teacher_forced(r, x, w, n, [(0.01, 1.0)], tag + " pack2", "c: pack2 path", scatter=False)
    for a, b in zip(by_scatter[(0.01, 1.0)][0], by_pack2[(0.01, 1.0)][0]):
        same(a, b, f"{tag}: scatter map against pack2_kernel")
    for wd, max_norm in ((0.01, 1.0), (0.0, 0.0)):
        trail, loss = by_scatter[(wd, max_norm)]
        r.reset()
        r.epoch(x, w, None, n, BATCH, 1e-3, wd, max_norm)
        assert r.desc.step == 3
        same(r.state() + r.images() + (r.acc.cpu().numpy(),), trail[-1] + (loss,), f"{tag}: one call against its batches")


def test_step_offsets_and_a_learning_rate_that_drops():
    """Bias corrections at steps 1.. and 10000.., and ``lr`` 1e-3 -> 2e-4 between calls (what the scheduler does)."""
    r = rig("maf3-d10")
    x, w = data(10, 100, True)
    for step0 in (0, 9999):
        teacher_forced(r, x, w, 100, [(0.01, 1.0), (0.0, 0.0)], f"maf3-d10 from step {step0 + 1}", "a: epoch step", step0=step0,
                       lrs=(1e-3, 2e-4, 2e-4))


# ------------------------------------------------------------------------------------- (b): a batch in chunks
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("key", ["maf3-d10", "nsf3-d10"])
def test_a_chunked_batch_leaves_the_final_gradients_squares(key, weighted):
    """``set_cap = 2``: a 40-row batch is two chunks (2 + 1 row sets), the second adding to the gradient in place.  The
    partials are those of the FINAL gradient, and the step agrees with the unchunked call."""
    r, c = rig(key), rig(key, 2)
    assert c.ts.desc.max_sets == 2 and r.ts.desc.max_sets >= 3
    x, w = data(r.spec.n_dim, BATCH, weighted, seed=1)
    for wd, max_norm in COMBOS[:2] + COMBOS[3:4]:
        tag = f"{key} chunked w={int(weighted)} wd={wd} max_norm={max_norm}"
        ends = []
        for q in (r, c):
            q.reset()
            before = q.state()
            q.epoch(x, w, None, BATCH, BATCH, 1e-3, wd, max_norm)
            g, part = q.gradient()
            note("partials", check_partials(q, g, part, tag))
            check_step(q, before, g, part, 1, 1e-3, wd, max_norm, tag, "b: chunked")
            check_images(q, tag)
            ends.append((q.state(), g, part))
        (su, gu, pu), (sc_, _, _) = ends
        sc = om.scalars(1, 1e-3, wd, max_norm)
        bnd = om.bound(before[0], gu, before[1], before[2], sc, pu)
        ratio = note("b: chunked against unchunked", om.worst_ratio(sc_, [a.astype(np.float64) for a in su], bnd))
        assert ratio <= 1.0, f"{tag}: chunked against unchunked {ratio:.3f}"


# ------------------------------------------------------------------------------------- (d): permutation, batch size
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [100, 81])
@pytest.mark.parametrize("key", ["maf3-d10", "nsf3-d10", "maf3-d32", "nsf3-d10-lean"])
def test_no_permutation_is_the_identity_permutation(key, n, weighted):
    """``perm = NULL`` (``x + b0 D``, ``w + b0``) gives the bits of ``perm = arange(n)``; n = 81: a last batch of one row.
    ``batch_size > n`` is one batch."""
    r = rig(key)
    x, w = data(r.spec.n_dim, n, weighted, seed=2)
    ident = torch.arange(n, dtype=torch.int64, device="cuda")
    got = []
    for perm in (None, ident):
        r.reset()
        r.epoch(x, w, perm, n, BATCH, 1e-3, 0.01, 1.0)
        assert r.desc.step == 3
        got.append(r.everything())
        check_images(r, f"{key} n={n}")
    same(*got, f"{key} n={n} w={int(weighted)}: perm NULL against arange")
    one = []
    for bs in (n, n + 7, 4096):
        r.reset()
        r.epoch(x, w, None, n, bs, 1e-3, 0.01, 1.0)
        assert r.desc.step == 1
        one.append(r.everything())
    same(one[0], one[1], "batch_size n + 7")
    same(one[0], one[2], "batch_size 4096")


# ------------------------------------------------------------------------------------- (e): the snapshot
@pytest.mark.parametrize("n", [100, 81, 80, 40])
@pytest.mark.parametrize("key", ["maf3-d10", "nsf3-d10", "maf3-d32"])
def test_the_snapshot_is_the_parameters_behind_the_last_step(key, n):
    """Poisoned with NaN before the call; n = 81: the last batch is one row, n = 80: it is a whole one, n = 40: the only one."""
    r = rig(key)
    x, w = data(r.spec.n_dim, n, True, seed=3)
    r.reset()
    r.epoch(x, w, None, n, BATCH, 1e-3, 0.01, 1.0)
    plain = r.everything()
    snap = torch.full_like(r.f.params, float("nan"))
    r.reset()
    r.epoch(x, w, None, n, BATCH, 1e-3, 0.01, 1.0, snapshot=snap)
    assert r.desc.step == -(-n // BATCH)
    same([snap.cpu().numpy()], [r.f.params.cpu().numpy()], f"{key} n={n}: snapshot against params")
    same(r.everything(), plain, f"{key} n={n}: with a snapshot against without")


# ------------------------------------------------------------------------------------- (f): pmc_adamw_step
@pytest.mark.parametrize("kind", om.STATES)
@pytest.mark.parametrize("n", [9372, 313944])
def test_adamw_step_on_the_table(n, kind):
    """The per-batch path (penalised and sharded fits): ``sqnorm_partial_kernel`` + ``adamw_kernel`` on every input of the
    model's table; the model squares the gradient itself, so the partials' own roundings (``sq_depth``) enter the bound."""
    from pocomc_amd import _lib
    lib = _lib.load()
    host = om.state(kind, n)
    p0, g, m0, v0 = (torch.from_numpy(a).cuda() for a in host)
    sq = torch.zeros(256, dtype=torch.float32, device="cuda")
    zero = {}
    for step, lr, wd, max_norm in om.HYPER:
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        _lib.check(lib.pmc_adamw_step(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n, lr, 0.9, 0.999, 1e-8, wd, max_norm, step,
                                      _lib.ptr(sq), _lib.stream_handle()), "pmc_adamw_step")
        got = tuple(t.cpu().numpy() for t in (p, m, v))
        sc = om.scalars(step, lr, wd, max_norm)
        ratio = note("f: pmc_adamw_step", om.worst_ratio(got, om.step64(*host, sc), om.bound(*host, sc, sq_roundings=om.sq_depth(n))))
        assert ratio <= 1.0, f"pmc_adamw_step n={n} {kind} step={step} lr={lr} wd={wd} max_norm={max_norm}: {ratio:.3f}"
        if max_norm == 0.0:
            zero[(step, lr, wd)] = got
        elif max_norm == 1e9:
            same(got, zero[(step, lr, wd)], "max_norm 1e9 against 0")


# ------------------------------------------------------------------------------------- (g): the bf16 engines
def _bf16_flow(engine):
    from pocomc_amd import Flow
    if engine == "bf16":
        spec = MAFSpec(16, 2, hidden=64)
        f = Flow(16, spec, precision="bf16")
        f.train_engine = "bf16"
    else:                                   # as tests/test_gpu_train_bf16_spline.py builds its smallest
        spec = MAFSpec(16, 2, hidden=64, univariate="rqs", bins=8)
        f = Flow(16, spec, seed=0)
        f.precision = "bf16"
        f.train_engine = engine
    f.set_params(cases.flow_params(spec, 2, gain=1.0))
    return f, spec


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("engine", ["bf16", "bf16_spline"])
def test_bf16_engines_take_the_same_step(engine, weighted):
    """``AdamW.epoch`` of the bf16 engines, one batch per call: the step on the device gradient (the clip reads the whole
    gradient there: ``partials=None``), and the float32 image after the call."""
    from pocomc_amd import _lib
    from pocomc_amd.train import AdamW, _train_state
    f, spec = _bf16_flow(engine)
    x, w = data(16, 100, weighted, seed=4)
    n_par = f.params.numel()
    for wd, max_norm in ((0.01, 1.0), (0.0, 0.0), (0.01, 1e9)):
        f.set_params(cases.flow_params(spec, 2, gain=1.0), check=False)
        opt = AdamW(f, 1e-3, weight_decay=wd)
        acc = torch.zeros(1, dtype=torch.float32, device="cuda")
        for k, b0 in enumerate(range(0, 100, BATCH)):
            before = tuple(t.cpu().numpy().copy() for t in (f.params, opt.m, opt.v))
            xb, wb = x[b0:b0 + BATCH].contiguous(), None if w is None else w[b0:b0 + BATCH].contiguous()
            opt.epoch(xb, wb, None, BATCH, max_norm, acc)
            assert opt.t == k + 1
            g = _train_state(f).grad.cpu().numpy()
            assert np.abs(g).max() > 0 and not g[spec.mask_flat() == 0].any()
            sc = om.scalars(k + 1, 1e-3, wd, max_norm)
            got = tuple(t.cpu().numpy() for t in (f.params, opt.m, opt.v))
            want = om.step64(before[0], g, before[1], before[2], sc)
            bnd = om.bound(before[0], g, before[1], before[2], sc, sq_roundings=om.sq_depth(n_par))
            ratio = note("g: bf16 engines", om.worst_ratio(got, want, bnd))
            assert ratio <= 1.0, f"{engine} w={int(weighted)} wd={wd} max_norm={max_norm} batch {k}: {ratio:.3f}"
            img = torch.full_like(f._packed, float("nan"))
            _lib.check(f.lib.pmc_maf_pack(_lib.ptr(f.params), _lib.ptr(f._pack_idx), _lib.ptr(img), img.numel(), _lib.stream_handle()),
                       "pmc_maf_pack")
            same([f._packed.cpu().numpy()], [img.cpu().numpy()], f"{engine}: float32 image after AdamW.epoch")

