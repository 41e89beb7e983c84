"""Flow training -- host-side mirror of ``Flow.fit`` (``pocomc/flow.py:165-384``).

The loop structure, the split quirk (``validation_split`` is the TRAIN fraction,
``flow.py:248-249``), the weighted loss (``:311-312``), global-norm clipping (``:318``),
AdamW (``:268``), the per-dataset loss normalisation (``:323``, ``:348``),
ReduceLROnPlateau (``:275-283``, ``:352-355``), the best-state snapshot (``:364-367``) and the
early stop at ``int(1.5 * patience)`` stale epochs (``:369-374``) follow the reference.
The arithmetic -- forward, backward, clip, optimizer -- runs in the gfx950 kernels
(``pmc_maf_loss_grad``, ``pmc_adamw_step``, ``pmc_maf_forward``, ``pmc_neg_weighted_sum``).
"""
from __future__ import annotations

import ctypes as C
import time
from functools import partial

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .maf_spec import WIDE_MIN_HIDDEN       # precision="bf16" affine flows at least this wide train on the bf16 matrix cores
from .mcmc import _pinned_give, _pinned_take


MAX_SETS = 256              # row sets of 16 per loss/gradient launch (one workgroup each; larger batches come in chunks)
SCRATCH_BUDGET = 1 << 29    # bytes of activation / delta scratch a flow may hold (wide flows keep fewer sets, >= 32)


class TrainState:
    """Training-side device buffers of one Flow (built on first ``fit``)."""

    def __init__(self, flow, light=False):
        """``light``: only what every engine needs (gradient, scalars); the bf16 engine keeps its own images
        (:class:`WideState`) and never touches the float32 training image."""
        spec, dev = flow.spec, flow.device
        n = spec.n_params
        # masked entries stay 0 for ever; one extra element carries the batch loss through the
        # gradient all-reduce of sharded training
        self.grad_ext = torch.zeros(n + 1, dtype=torch.float32, device=dev)
        self.grad = self.grad_ext[:n]
        self.wsum = torch.zeros(1, dtype=torch.float32, device=dev)
        self.scal = torch.zeros(4, dtype=torch.float32, device=dev)      # [loss, spare...]
        self.light = bool(light)
        self.n_sets = 0
        if light:
            self.sq_partial = torch.zeros(256, dtype=torch.float32, device=dev)       # PMC_ADAMW_SCRATCH
            self.desc = None
            return
        L = spec.train_layout()
        pT_idx, gmap = spec.train_index()
        jobs = spec.train_jobs()
        self.packT_idx = torch.from_numpy(pT_idx).to(dev)
        self.gmap = torch.from_numpy(gmap).to(dev)
        self.jobs = torch.from_numpy(jobs.reshape(-1).copy()).to(dev)
        self.n_waves = int(flow.lib.pmc_maf_train_waves(C.byref(flow._desc)))   # waves per chain workgroup
        self.tables = torch.from_numpy(spec.train_tables(self.n_waves)).to(dev)
        self.n_jobs = int(jobs.shape[0])
        self.packedT = torch.zeros(pT_idx.size, dtype=torch.float32, device=dev)
        self.sq_partial = torch.zeros(max(self.n_jobs, 256), dtype=torch.float32, device=dev)   # >= PMC_ADAMW_SCRATCH
        self.par_pt = spec.par_per_transform()
        self.desc = _lib.pmc_maf_train_t(packedT=self.packedT.data_ptr(), gmap=self.gmap.data_ptr(),
                                         pkT_per_transform=L["pkT_per_transform"],
                                         gmap_per_transform=L["gmap_per_transform"],
                                         jobs=self.jobs.data_ptr(), n_jobs=self.n_jobs,
                                         tables=self.tables.data_ptr(), table_waves=self.n_waves,
                                         n_sq_partial=self.sq_partial.numel(), par_per_transform=self.par_pt,
                                         sq_partial=self.sq_partial.data_ptr())
        self.xt_floats = (spec.n_transforms + 1) * spec.Dp * 16
        self.act_floats = spec.n_transforms * 3 * spec.Hp * 16
        self.par_floats = spec.n_transforms * self.par_pt
        per_set = 4 * (self.xt_floats + 2 * self.act_floats + self.par_floats)
        self.set_cap = int(max(32, min(MAX_SETS, SCRATCH_BUDGET // per_set)))
        self.scatter_maps(flow)             # (host-built once per Flow, like the maps above: not a per-fit cost)
        # the stream the validation passes of a fit run on (fit_flow): created and used once here -- a new HIP stream's first
        # launch sets up its hardware queue, tens of milliseconds that do not belong to an epoch
        self.side_stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(self.side_stream):
            self.scal.zero_()
        self.side_stream.synchronize()

    def ensure_sets(self, n_rows):
        """Scratch for the row sets of one launch: transform inputs, activations, deltas, output gradients."""
        need = max(1, min(self.set_cap, (int(n_rows) + 15) // 16))
        if need <= self.n_sets:
            return
        dev = self.grad.device
        self.xt_scratch = torch.empty(need * self.xt_floats, dtype=torch.float32, device=dev)
        self.act_scratch = torch.empty(need * self.act_floats, dtype=torch.float32, device=dev)
        self.delta_scratch = torch.empty(need * self.act_floats, dtype=torch.float32, device=dev)
        self.par_scratch = torch.empty(need * self.par_floats, dtype=torch.float32, device=dev)
        self.loss_partial = torch.zeros(need, dtype=torch.float32, device=dev)
        self.n_sets = need
        self.desc.xt_scratch = self.xt_scratch.data_ptr()
        self.desc.act_scratch = self.act_scratch.data_ptr()
        self.desc.delta_scratch = self.delta_scratch.data_ptr()
        self.desc.par_scratch = self.par_scratch.data_ptr()
        self.desc.loss_partial = self.loss_partial.data_ptr()
        self.desc.max_sets = need

    def scatter_maps(self, flow):
        """CSR inverse of the two pack maps (``pmc_adamw_t.scatter_*``): where every parameter sits in the forward /
        inverse image (``Flow._packed``) and in the transposed training image (``packedT``)."""
        if getattr(self, "_scatter", None) is None:
            a = flow._pack_idx.cpu().numpy().astype(np.int64)
            b = self.packT_idx.cpu().numpy().astype(np.int64)
            src = np.concatenate([a, b])                       # parameter index of every image position, -1 = padding
            pos = np.nonzero(src >= 0)[0]
            order = np.argsort(src[pos], kind="stable")
            dst = pos[order].astype(np.int32)
            counts = np.bincount(src[pos], minlength=flow.params.numel())
            ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            dev = flow.params.device
            self._scatter = (torch.from_numpy(ptr).to(dev), torch.from_numpy(dst).to(dev))
        return self._scatter

    def repack(self, flow):
        if self.light:
            return
        with torch.cuda.device(flow.device):
            _lib.check(flow.lib.pmc_maf_pack(_lib.ptr(flow.params), _lib.ptr(self.packT_idx), _lib.ptr(self.packedT),
                                             self.packedT.numel(), _lib.stream_handle()), "pmc_maf_pack(T)")


def _train_state(flow):
    want_light = _wide_state(flow) is not None
    ts = getattr(flow, "_train", None)
    if ts is None or (ts.light and not want_light):
        flow._train = TrainState(flow, light=want_light)
    return flow._train


class WideState:
    """Device side of ``csrc/maf_train_bf16.hip`` (``pmc_maf_wide_t``): the row-major bf16 weight image with its index
    map, the float32 bias image and the activation scratch -- for an affine flow or a spline flow (``OK = n_out DK``
    output rows; the scratch of a spline flow also holds its raw spline parameters in float32)."""

    def __init__(self, flow):
        spec, dev, lib = flow.spec, flow.device, flow.lib
        L = spec.wide_layout()
        img_idx, bias_idx = spec.wide_index()
        self.image_idx = torch.from_numpy(img_idx).to(dev)
        self.bias_idx = torch.from_numpy(bias_idx).to(dev)
        self.image = torch.zeros(img_idx.size, dtype=torch.int16, device=dev)
        self.bias = torch.zeros(bias_idx.size, dtype=torch.float32, device=dev)
        nbytes = int(lib.pmc_maf_wide_scratch_bytes(C.byref(flow._desc)))
        self.scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.sq = torch.zeros(256, dtype=torch.float32, device=dev)      # PMC_ADAMW_SCRATCH
        self.desc = _lib.pmc_maf_wide_t(image=self.image.data_ptr(), image_idx=self.image_idx.data_ptr(),
                                        image_per_transform=L["per_transform"], bias=self.bias.data_ptr(),
                                        bias_idx=self.bias_idx.data_ptr(), bias_per_transform=L["bias_per_transform"],
                                        scratch=self.scratch.data_ptr(), scratch_bytes=nbytes, wsum=None)

    def refresh(self, flow):
        with torch.cuda.device(flow.device):
            _lib.check(flow.lib.pmc_maf_wide_refresh(C.byref(flow._desc), C.byref(self.desc), _lib.ptr(flow.params),
                                                     _lib.stream_handle()), "pmc_maf_wide_refresh")


def _wide_state(flow):
    """The bf16 training engine of this flow, or None (float32 kernels): ``precision="bf16"`` affine flows of hidden
    width >= WIDE_MIN_HIDDEN; ``flow.train_engine = "f32" | "bf16"`` overrides the width rule.  A spline flow takes the
    engine only when asked: ``flow.train_engine = "bf16_spline"`` with ``precision="bf16"``, at any width."""
    engine = getattr(flow, "train_engine", None)
    bf16 = getattr(flow, "precision", "f32") == "bf16"
    if engine == "bf16_spline":
        if not bf16 or flow.spec.univariate != "rqs":
            raise ValueError("train_engine='bf16_spline' needs a spline flow with precision='bf16' "
                             "(affine flows: train_engine='bf16')")
    elif engine == "f32" or not bf16 or flow.spec.univariate != "affine":
        if engine == "bf16":
            raise ValueError("train_engine='bf16' needs an affine flow with precision='bf16' "
                             "(spline flows: train_engine='bf16_spline')")
        return None
    elif engine != "bf16" and flow.spec.hidden < WIDE_MIN_HIDDEN:
        return None
    if getattr(flow, "_wide", None) is None:
        flow._wide = WideState(flow)
    return flow._wide


def _loss_grad_call(flow, ts, ws, xb, wb, idx, loss_ptr, n, stream):
    """The loss / gradient launch of the flow's engine (``ws``: its bf16 state, None = float32) inside the caller's device context."""
    what = "pmc_maf_loss_grad" if ws is None else "pmc_maf_loss_grad_bf16"
    _lib.check(getattr(flow.lib, what)(C.byref(flow._desc), C.byref((ws or ts).desc), _lib.ptr(xb), _lib.ptr(wb), _lib.ptr(idx),
                                       1000.0, _lib.ptr(ts.grad), loss_ptr, n, stream), what)


def loss_and_grad(flow, xb, wb=None, idx=None, refresh=True):
    """Loss of one batch (device scalar tensor) and its gradient (in ``flow._train.grad``).
    ``idx`` (int64, device) selects the batch rows out of ``xb`` / ``wb``.  (``refresh=False``: the caller keeps the
    bf16 training image in step with the parameters itself.)"""
    ts = _train_state(flow)
    n = xb.shape[0] if idx is None else idx.numel()
    ts.scal.zero_()
    ws = _wide_state(flow)
    if ws is None:
        ts.ensure_sets(n)
    elif refresh:
        ws.refresh(flow)
    with torch.cuda.device(flow.device):
        _loss_grad_call(flow, ts, ws, xb, wb, idx, _lib.ptr(ts.scal), n, _lib.stream_handle())
    return ts.scal[0]


def batch_loss(flow, xb, wb=None, group=None, sharded=False):
    """Loss of one batch without gradient (validation, ``flow.py:327-346``).  ``sharded``: ``xb`` is
    this rank's part of the batch, the weight normalisation uses the all-reduced weight sum."""
    ts = _train_state(flow)
    lib = flow.lib
    st = _lib.stream_handle()
    n = xb.shape[0]
    z = torch.empty_like(xb)
    lp = torch.empty(n, dtype=torch.float32, device=flow.device)
    ts.scal.zero_()
    with torch.cuda.device(flow.device):
        _lib.check(lib.pmc_maf_forward(C.byref(flow._desc), _lib.ptr(xb), _lib.ptr(z), None, _lib.ptr(lp), n, st),
                   "pmc_maf_forward")
        if wb is not None:
            _lib.check(lib.pmc_sum_f32(_lib.ptr(wb), C.c_void_p(ts.scal.data_ptr() + 4), n, st), "pmc_sum_f32")
            if sharded:
                dist.all_reduce(ts.scal[1:2], group=group)
        _lib.check(lib.pmc_neg_weighted_sum(_lib.ptr(lp), _lib.ptr(wb) if wb is not None else None,
                                            C.c_void_p(ts.scal.data_ptr() + 4) if wb is not None else None,
                                            1000.0, _lib.ptr(ts.scal), n, st), "pmc_neg_weighted_sum")
    return ts.scal[0]


class AdamW:
    """``torch.optim.AdamW`` on the flat parameter vector (``flow.py:268``)."""

    def __init__(self, flow, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
        self.flow, self.lr, self.wd, self.betas, self.eps = flow, float(lr), float(weight_decay), betas, eps
        self.m = torch.zeros_like(flow.params)
        self.v = torch.zeros_like(flow.params)
        self.t = 0
        ws = _wide_state(flow)
        if ws is not None:
            ws.refresh(flow)

    def step(self, max_norm):
        """One clipped step on the gradient in ``flow._train.grad``, then refresh both kernel images."""
        f = self.flow
        ts = _train_state(f)
        self.t += 1
        with torch.cuda.device(f.device):
            _lib.check(f.lib.pmc_adamw_step(_lib.ptr(f.params), _lib.ptr(ts.grad), _lib.ptr(self.m), _lib.ptr(self.v),
                                            f.params.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                                            float(max_norm) if max_norm is not None else 0.0, self.t,
                                            _lib.ptr(ts.sq_partial), _lib.stream_handle()),
                       "pmc_adamw_step")
        f.repack()
        ws = _wide_state(f)
        if ws is not None:
            ws.refresh(f)
        else:
            ts.repack(f)

    def epoch(self, x, w, perm, batch_size, max_norm, loss_acc, gate=None, stream=None, snapshot=None):
        """``flow.py:297-323`` for one epoch in a single library call: every batch's loss/gradient,
        clip, AdamW step and image refresh is enqueued back to back; ``loss_acc`` (f32 [1], device)
        accumulates the batch losses.  ``gate`` (a recorded ``torch.cuda.Event``): the epoch's first optimizer step waits
        for it (``pmc_maf_train_epoch_gated``: the previous epoch's validation pass on another stream)."""
        f = self.flow
        ts = _train_state(f)
        ws = _wide_state(f)
        if ws is not None:
            c = _lib.pmc_adamw_t(params=f.params.data_ptr(), grad=ts.grad.data_ptr(), exp_avg=self.m.data_ptr(),
                                 exp_avg_sq=self.v.data_ptr(), n_params=f.params.numel(), lr=self.lr,
                                 beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.wd,
                                 max_norm=float(max_norm) if max_norm is not None else 0.0, step=self.t)
            with torch.cuda.device(f.device):
                _lib.check(f.lib.pmc_maf_train_epoch_bf16(C.byref(f._desc), C.byref(ws.desc), C.byref(c), _lib.ptr(x),
                                                          _lib.ptr(w), _lib.ptr(perm), x.shape[0], int(batch_size), _lib.ptr(loss_acc),
                                                          _lib.ptr(ws.sq), _lib.stream_handle()),
                           "pmc_maf_train_epoch_bf16")
            self.t = int(c.step)
            f.repack()                      # the float32 / fragment images follow once per epoch (validation, inference)
            return
        ts.ensure_sets(batch_size)
        # (the descriptor is built once per optimizer: an epoch of the Sampler's fits is ~100 us and this method runs once
        #  per epoch on the driver thread -- only what changes between epochs is written)
        c = getattr(self, "_desc", None)
        if c is None:
            sc_ptr, sc_dst = ts.scatter_maps(f)
            c = self._desc = _lib.pmc_adamw_t(
                params=f.params.data_ptr(), grad=ts.grad.data_ptr(), exp_avg=self.m.data_ptr(),
                exp_avg_sq=self.v.data_ptr(), n_params=f.params.numel(),
                pack_idx=f._pack_idx.data_ptr(), packed=f._packed.data_ptr(), n_packed=f._packed.numel(),
                packT_idx=ts.packT_idx.data_ptr(), packedT=ts.packedT.data_ptr(), n_packedT=ts.packedT.numel(),
                beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.wd,
                scatter_ptr=sc_ptr.data_ptr(), scatter_dst=sc_dst.data_ptr())
            self._desc_refs = (C.byref(f._desc), C.byref(ts.desc), C.byref(c))
        c.lr, c.step, c.max_norm = self.lr, self.t, float(max_norm) if max_norm is not None else 0.0
        c.snapshot = snapshot.data_ptr() if snapshot is not None else None     # (the parameters behind the epoch's last step)
        d_maf, d_tr, d_opt = self._desc_refs

        def call():
            return f.lib.pmc_maf_train_epoch_gated(d_maf, d_tr, d_opt, x.data_ptr(), w.data_ptr() if w is not None else None,
                                                   perm.data_ptr() if perm is not None else None, x.shape[0], int(batch_size),
                                                   loss_acc.data_ptr(), gate.cuda_event if gate is not None else None,
                                                   stream if stream is not None else torch.cuda.current_stream(f.device).cuda_stream)
        if torch.cuda.current_device() == f.device.index:           # (the usual case: no device switch to pay for)
            rc = call()
        else:
            with torch.cuda.device(f.device):
                rc = call()
        if rc:
            _lib.check(rc, "pmc_maf_train_epoch")
        self.t = int(c.step)


class ReduceLROnPlateau:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor=0.2, threshold=1e-4,
    threshold_mode='abs', min_lr=1e-6)`` as configured at ``flow.py:275-283``."""

    def __init__(self, opt, patience, factor=0.2, threshold=1e-4, min_lr=1e-6):
        self.opt, self.patience, self.factor, self.threshold, self.min_lr = opt, patience, factor, threshold, min_lr
        self.best, self.bad = float("inf"), 0

    def step(self, metric):
        if metric < self.best - self.threshold:
            self.best, self.bad = metric, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            new = max(self.opt.lr * self.factor, self.min_lr)
            if self.opt.lr - new > 1e-8:
                self.opt.lr = new
            self.bad = 0


def _weight_flags(flow):
    """uint8 [n_params]: 1 for the entries of the hyper-networks' weight matrices (what ``parameter_name.endswith('weight')``
    selects at ``flow.py:409-411`` -- masked-out entries included), 0 for biases."""
    ts = _train_state(flow)
    if getattr(ts, "weight_flags", None) is None:
        spec = flow.spec
        f = np.zeros(spec.n_params, dtype=np.uint8)
        for t in range(spec.n_transforms):
            for name in ("W0", "W1", "W2", "W3"):
                off, sz = spec.offsets[name]
                f[t * spec.params_per_transform + off: t * spec.params_per_transform + off + sz] = 1
        ts.weight_flags = torch.from_numpy(f).to(flow.device)
    return ts.weight_flags


def _batch_at(x, w, perm, b0, nb):
    """``(idx, xb, wb)`` of a pass's batch at ``b0``: entries of the permutation (the kernels gather), or slices."""
    if perm is not None:
        return perm[b0:b0 + nb], x, w
    return None, x[b0:b0 + nb], None if w is None else w[b0:b0 + nb]


def _add_penalty(flow, penalty, grad, loss, mult=1.0):
    """flow.py:304-307, :314-315: ``mult`` times the weight penalty onto ``loss``, its gradient onto ``grad`` (or None)."""
    b, g, flags = penalty
    with torch.cuda.device(flow.device):
        _lib.check(flow.lib.pmc_weight_penalty(_lib.ptr(flow.params), _lib.ptr(flags), _lib.ptr(grad), flow.params.numel(),
                                               b, g, float(mult), _lib.ptr(loss), _lib.ptr(flow._train.sq_partial),
                                               _lib.stream_handle()), "pmc_weight_penalty")


def _train_penalised(flow, opt, x, w, perm, batch_size, max_norm, loss_acc, penalty):
    """Batch by batch (flow.py:301-321) with the penalty's gradient added before the clip (flow.py:314-318)."""
    n, bs = x.shape[0], int(batch_size)
    for b0 in range(0, n, bs):
        idx, xb, wb = _batch_at(x, w, perm, b0, min(bs, n - b0))
        loss_acc += loss_and_grad(flow, xb, wb, idx, refresh=False)
        penalty(flow._train.grad, loss_acc)
        opt.step(max_norm)


def _train_sharded(flow, opt, x, w, perm, batch_size, max_norm, loss_acc, group, penalty=None):
    """One epoch of data-parallel training: every rank holds a shard of the training rows; a global
    batch of ``batch_size`` rows is ``batch_size / world`` local rows per rank.  Per batch: [all-reduce of the weight sum] ->
    local loss/gradient -> ONE all-reduce of (gradient, loss) -> the same clip + AdamW step on every rank (the clip needs the
    norm of the reduced gradient, flow.py:318)."""
    ts = _train_state(flow)
    lb = max(1, int(batch_size) // dist.get_world_size(group))
    n = x.shape[0]
    wide = _wide_state(flow)
    if wide is None:
        ts.ensure_sets(lb)
    st = _lib.stream_handle()
    loss_ptr = C.c_void_p(ts.grad_ext.data_ptr() + 4 * ts.grad.numel())     # (the element behind the gradient)
    for b0 in range(0, n, lb):
        nb = min(lb, n - b0)
        idx, xb, wb = _batch_at(x, w, perm, b0, nb)
        with torch.cuda.device(flow.device):
            if w is not None:
                ts.wsum.zero_()
                wsel = w[idx] if idx is not None else wb
                _lib.check(flow.lib.pmc_sum_f32(_lib.ptr(wsel), _lib.ptr(ts.wsum), nb, st), "pmc_sum_f32")
                dist.all_reduce(ts.wsum, group=group)
                (wide or ts).desc.wsum = ts.wsum.data_ptr()
            ts.grad_ext[-1:].zero_()
            _loss_grad_call(flow, ts, wide, xb, wb, idx, loss_ptr, nb, st)
            (wide or ts).desc.wsum = None
        dist.all_reduce(ts.grad_ext, group=group)
        loss_acc += ts.grad_ext[-1:]
        if penalty is not None:                   # the same penalty on every rank, once per global batch
            penalty(ts.grad, loss_acc)
        opt.step(max_norm)


sharded_epoch = _train_sharded


def _valid_epoch_call(flow, slots, w, batch_size, stream, sl, x):
    """The whole pass in one library call on ``stream`` (batches of the reference's DataLoader, flow.py:327-348)."""
    perm = None
    if slots.shuffle:                               # (fused staging: uploaded with the training pass's permutation)
        perm = slots.upload(1, sl) if not slots.fused else slots.d_perm[1][sl] if slots.n_valid else None
    with torch.cuda.device(flow.device):
        _lib.check(flow.lib.pmc_maf_valid_epoch(C.byref(flow._desc), _lib.ptr(x), _lib.ptr(w), _lib.ptr(perm), slots.n_valid,
                                                int(batch_size), _lib.ptr(flow._train.logp_scratch),
                                                _lib.ptr(slots.acc_valid[sl]), stream), "pmc_maf_valid_epoch")


def _valid_sharded(flow, slots, w, local_batch, shuffle, group, sl, x):
    """Batch by batch on this rank's shard of the validation rows, as ``DataLoader(TensorDataset(...), batch_size, shuffle)``
    hands them out: a fresh permutation per epoch, last partial batch kept (the ranks' sum follows in ``_enqueue``)."""
    order = torch.randperm(slots.n_valid) if shuffle else torch.arange(slots.n_valid)
    for b0 in range(0, slots.n_valid, local_batch):
        idx = order[b0:b0 + local_batch].to(flow.device)
        slots.acc_valid[sl] += batch_loss(flow, x[idx].contiguous(), None if w is None else w[idx].contiguous(), group, True)


class _FitPlan:
    """Every decision of one fit, taken once: the functions its epochs call follow from these fields alone.
    ``train_mode``: "epoch_call" (``AdamW.epoch``), "penalised" (``_train_penalised``), "sharded" (``_train_sharded``);
    ``valid_mode``: None, "call" / "call_side" (``_valid_epoch_call`` on the main / side stream), "sharded" (``_valid_sharded``)."""

    def __init__(self, flow, x_valid, batch_size, shuffle, penalised, annealing, group, sharded):
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.sharded = bool(self.world > 1 if sharded is None else sharded)
        self.validation, self.n_valid = validation, n_valid = x_valid is not None, 0 if x_valid is None else x_valid.shape[0]
        self.engine = "bf16" if _wide_state(flow) is not None else "f32"
        self.train_mode = "sharded" if self.sharded else "penalised" if penalised else "epoch_call"
        # Float32 engine, one process, no penalty term (the other paths enqueue batch by batch from Python):
        plain = self.engine == "f32" and not self.sharded and not penalised
        # Plain shuffled fits: ONE host-to-device copy per epoch carries both
        # permutations AND the zeros of the two loss accumulators (two int64 words in front of the permutations in one staging
        # buffer), and the parameters behind the epoch's last step are written by that step itself (pmc_adamw_t.snapshot) --
        # three ~5 us launches fewer per epoch, of the ~75-120 us an epoch of the Sampler's fits takes.
        self.fused_staging = plain and bool(shuffle)
        # The validation pass of epoch e only READS the parameters, and so do the loss / gradient launches of epoch e + 1's
        # first batch; a batch's chain kernel occupies 32 of 256 compute units.  So the pass runs on a second stream, next to
        # that batch, and only the first optimizer step of epoch e + 1 waits for it (pmc_maf_train_epoch_gated): plain fits.
        # It pays where the pass (two cross-stream hand-overs of ~16 us, the forward launch, the reduction, the copies: ~65 us
        # at the Sampler's sizes) is SHORTER than the first batch's chain + weight-gradient launches it hides behind, and costs
        # the host ~15 us per epoch: deep or spline flows (chain >= ~80 us) with a validation set of at most two batches' worth
        # of rows -- the Sampler's regime (README example, nsf6: 152 -> 123 us per epoch).  Measured otherwise: maf3 at D = 10
        # 76 -> 91 us (the epoch is bound by its ~120 us of enqueue, not by the device), the bench's fit (maf3 at D = 32, ten
        # batches, 5000 validation rows whose 313 workgroups crowd the chain's 32) 0.95 -> 1.05 ms.
        long_chain = flow.spec.n_transforms * (2 if flow.spec.univariate == "rqs" else 1) >= 6
        side = plain and long_chain and n_valid <= 2 * int(batch_size)
        self.valid_mode = None if not validation else "sharded" if self.sharded else "call_side" if side else "call"
        # One epoch may be IN FLIGHT while the host looks at the previous epoch's losses (no scheduler, one GPU): the
        # early-stop test needs every epoch's loss on the host, and waiting for it before enqueuing the next epoch
        # leaves the GPU idle for the whole host turn-around (most of an epoch when the training set is one or two
        # batches, the Sampler's usual case).  The speculative epoch changes nothing observable: on an early stop the
        # best parameters are restored (flow.py:369-374), and no epoch is enqueued past `epochs`.
        self.pipelined = not annealing and not self.sharded
        self.slots = 2 if self.pipelined else 1


def _prepare_data(flow, x, weights, validation_split, shuffle):
    """Cast, initial shuffle and split (flow.py:234-259): ``x, (x_train, w_train, x_valid, w_valid)`` -- all rows on the
    device, then the two parts (the validation part None without a split)."""
    from .flow import torch_double_to_float
    x = torch_double_to_float(torch.as_tensor(x))
    n_samples, n_dim = x.shape
    if n_dim != flow.n_dim:
        raise ValueError("x has the wrong number of columns")
    x = x.to(flow.device)
    w = None if weights is None else torch.as_tensor(weights).to(torch.float32).to(flow.device)
    if shuffle:                                                     # flow.py:234-238 (the permutation still comes
        rand_indx = torch.randperm(n_samples).to(flow.device)       # from torch's CPU generator; rows move on the device)
        x = x[rand_indx]
        if w is not None:
            w = w[rand_indx]
    x = x.contiguous()
    w = None if w is None else w.contiguous()
    if validation_split > 0.0:                                      # flow.py:247-259
        cut = int(validation_split * n_samples)
        return x, (x[:cut], None if w is None else w[:cut], x[cut:], None if w is None else w[cut:])
    return x, (x, w, None, None)


def _noise_setup(flow, x, noise, plan, group):
    """``(scale, seed)`` of the noise a fit adds to its rows (flow.py:240-245; pmc_add_noise_f32 in the header), or None."""
    if noise is None:
        return None
    # flow.py:241-245: `mean_min_dist = torch.mean(min_dist)` -- the mean of the LAST row's distances to all rows
    # (the nearest-neighbour distances `min_dists` computed in the loop above it are never used); its loop raises
    # for a row without a positive distance, like torch.min of an empty tensor
    n_samples, n_dim = x.shape
    if n_samples < 2:
        raise RuntimeError("min(): Expected reduction dim to be specified for input.numel() == 0.")
    dev, world, xc = flow.device, plan.world, x
    md = torch.zeros(1, dtype=torch.float32, device=dev)
    if plan.sharded:
        # one scale for all ranks, the single-process value: the mean distance of the LAST row of the whole set (the
        # last rank's last row) to every row of every shard
        last = x[-1:].clone()
        dist.broadcast(last, src=dist.get_global_rank(group, world - 1) if group is not None else world - 1, group=group)
        xc = torch.cat([x, last]).contiguous()
    with torch.cuda.device(dev):
        _lib.check(flow.lib.pmc_mean_distance_f32(_lib.ptr(xc), xc.shape[0], n_dim, xc.shape[0] - 1, _lib.ptr(md),
                                                  _lib.stream_handle()), "pmc_mean_distance_f32")
    if plan.sharded:
        tot = md.double() * (n_samples + 1)            # (the appended row adds a zero distance)
        dist.all_reduce(tot, group=group)
        md = (tot / (n_samples * world)).float()
    scale = float(noise) * float(md.item())
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) * 2 ** 31 + int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    if plan.sharded:
        sd = torch.tensor([seed], dtype=torch.int64, device=dev)
        dist.broadcast(sd, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        seed = int(sd.item())
    return scale, seed


class _FitSlots:
    """The buffers of the epochs a fit has enqueued, one slot each (``_FitPlan.slots``), and ``gate``: the event the NEXT
    epoch's first update waits for (the validation pass on the side stream)."""

    def __init__(self, flow, plan, x_train, x_valid, shuffle, noise, rank):
        dev, k = flow.device, range(plan.slots)
        self.flow, self.fused, self.shuffle, self.gate = flow, plan.fused_staging, bool(shuffle), None
        self.noise, self.rank, self.n_train, self.n_valid = noise, rank, x_train.shape[0], plan.n_valid
        n_train, n_valid = self.n_train, self.n_valid
        # per slot ONE staging buffer, pinned and on the device: [the two losses in the first word, zeros on the host | training
        # | validation permutation]  (pinned staging from the process-wide free list: page-locking a buffer costs ~1 ms)
        self.h_stage = [_pinned_take((2 + n_train + n_valid,), torch.int64).zero_() for _ in k]
        self.d_stage = [torch.zeros(2 + n_train + n_valid, dtype=torch.int64, device=dev) for _ in k]
        self.h_perm = [[h[2:2 + n_train] for h in self.h_stage], [h[2 + n_train:] for h in self.h_stage]]   # [0 train | 1 valid][sl]
        self.d_perm = [[d[2:2 + n_train] for d in self.d_stage], [d[2 + n_train:] for d in self.d_stage]]
        self.acc_d = [d[:1].view(torch.float32) for d in self.d_stage]            # [train loss, val loss]
        self.acc_train, self.acc_valid = [a[0:1] for a in self.acc_d], [a[1:2] for a in self.acc_d]
        self.acc_h = [_pinned_take((2,), torch.float32).zero_() for _ in k]      # the losses on the host, complete at `done`
        self.done = [torch.cuda.Event() for _ in k]
        self.after = [torch.empty_like(flow.params) for _ in k]                  # parameters after the epoch
        self.noisy = None if noise is None else [[torch.empty_like(x_train) for _ in k],
                                                 [torch.empty_like(x_valid) if plan.validation else None for _ in k]]
        self.main = torch.cuda.current_stream(dev)                    # (looked up once: the fit stays on this stream)
        self.side = flow._train.side_stream if plan.valid_mode == "call_side" else None
        self.train_done = [torch.cuda.Event() for _ in k] if self.side is not None else None

    def upload(self, which, sl):
        # DataLoader(shuffle=...), flow.py:251-265: a fresh permutation per pass (pinned staging, no host sync)
        torch.randperm(self.h_perm[which][sl].numel(), out=self.h_perm[which][sl])
        self.d_perm[which][sl].copy_(self.h_perm[which][sl], non_blocking=True)
        return self.d_perm[which][sl]

    def upload_perms(self, sl):
        # zeroes the slot's losses, returns its training permutation (or None); fused: ONE copy with the zeros and both passes'
        if not self.fused:
            self.acc_d[sl].zero_()
            return self.upload(0, sl) if self.shuffle else None
        torch.randperm(self.n_train, out=self.h_perm[0][sl])          # (the same draws in the same order as unfused)
        if self.n_valid:
            torch.randperm(self.n_valid, out=self.h_perm[1][sl])
        self.d_stage[sl].copy_(self.h_stage[sl], non_blocking=True)
        return self.d_perm[0][sl]

    def with_noise(self, which, sl, epoch, src):
        """Fresh noise on every row of a pass (the reference draws it per batch of every epoch, flow.py:305 / :334)."""
        if self.noisy is None:
            return src
        dst, (scale, seed) = self.noisy[which][sl], self.noise
        with torch.cuda.device(self.flow.device):
            # (a rank's shard draws the noise of ITS rows of the whole set: keyed by the global row)
            _lib.check(self.flow.lib.pmc_add_noise_rows_f32(_lib.ptr(src), src.shape[0], src.shape[1], scale, seed,
                                                            2 * epoch + which, self.rank * src.shape[0], _lib.ptr(dst),
                                                            _lib.stream_handle()), "pmc_add_noise_rows_f32")
        return dst

    def release(self):
        # a speculative epoch may still be copying its permutations / losses: wait before the staging goes back
        if self.side is not None:
            torch.cuda.current_stream(self.flow.device).wait_stream(self.side)
            self.side.synchronize()
        torch.cuda.current_stream().synchronize()
        for t in self.acc_h + self.h_stage:
            _pinned_give(t)


def _enqueue(slots, n_slots, train, validate, sum_ranks, valid_penalty, x_train, x_valid, epoch):
    """One epoch on the device: staging, training pass, validation pass, the slot's tail -- on the main stream, or from the
    validation pass on behind ``train_done`` on the side stream, whose ``done`` then gates the next epoch's first update."""
    sl = epoch % n_slots
    perm = slots.upload_perms(sl)
    xs = slots.with_noise(0, sl, epoch, x_train)
    keep = None if slots.fused else slots.after[sl]                  # (fused: the epoch's last step writes them itself)
    if slots.side is None:
        train[sl](xs, perm=perm)
        if validate is not None:
            validate(sl, slots.with_noise(1, sl, epoch, x_valid))
        if sum_ranks is not None:            # a sum over the ranks' shards (the training loss rode along with the gradients)
            sum_ranks(slots.acc_valid[sl])
        if valid_penalty is not None:
            valid_penalty(slots.acc_valid[sl])
        if keep is not None:
            keep.copy_(slots.flow.params)
        slots.acc_h[sl].copy_(slots.acc_d[sl], non_blocking=True)
        slots.done[sl].record()
    else:                                                             # (a plain fit: one process, no penalty)
        train[sl](xs, perm=perm, gate=slots.gate)
        if keep is not None:
            keep.copy_(slots.flow.params)
        slots.train_done[sl].record(slots.main)
        with torch.cuda.stream(slots.side):
            slots.side.wait_event(slots.train_done[sl])
            validate(sl, slots.with_noise(1, sl, epoch, x_valid))
            slots.acc_h[sl].copy_(slots.acc_d[sl], non_blocking=True)
            slots.done[sl].record(slots.side)
        slots.gate = slots.done[sl]


def _host_loop(flow, plan, slots, enqueue, sched, epochs, patience, verbose):
    """The host's side of the epochs (flow.py:323-374): losses, scheduler, best-state snapshot, early stop."""
    history = dict(loss=[], val_loss=[])
    validation, pipelined, monitor = plan.validation, plan.pipelined, "val_loss" if plan.validation else "loss"
    best_epoch, best_loss, best_model = 0, np.inf, flow.params.clone()
    n_tr, n_va = (max(n * (plan.world if plan.sharded else 1), 1) for n in (slots.n_train, slots.n_valid))
    start = time.time()
    if epochs > 0:
        enqueue(0)
    for epoch in range(epochs):
        sl = epoch % plan.slots
        if pipelined and epoch + 1 < epochs:
            enqueue(epoch + 1)                                        # speculative: runs while we read this epoch's losses
        slots.done[sl].synchronize()                                  # the one wait of the epoch
        both = slots.acc_h[sl].numpy()
        train_loss = float(both[0]) / n_tr                            # flow.py:323
        history["loss"].append(train_loss)
        if validation:
            val_loss = float(both[1]) / n_va                          # flow.py:348
            history["val_loss"].append(val_loss)
        if sched is not None:
            sched.step(val_loss if validation else train_loss)
        if verbose > 1:
            print("Epoch %3d/%3d, train loss: %5.2f" % (epoch + 1, epochs, train_loss)
                  + (", val loss: %5.2f" % val_loss if validation else ""))
        if history[monitor][-1] < best_loss:                          # flow.py:364-367
            best_loss, best_epoch = history[monitor][-1], epoch
            best_model.copy_(slots.after[sl])
        if epoch - best_epoch >= int(1.5 * patience):                 # flow.py:369-374
            if slots.side is not None:                                # (a speculative validation pass still reads the images)
                torch.cuda.current_stream(flow.device).wait_stream(slots.side)
            flow.params.copy_(best_model)
            flow.repack()
            if verbose > 0:
                print("Finished early after %3d epochs" % best_epoch)
                print("Best loss achieved %5.2f" % best_loss)
            break
        if not pipelined and epoch + 1 < epochs:
            enqueue(epoch + 1)
    if verbose > 0:
        total = time.time() - start
        print("\nTime total:     %5.2f sec" % total)
        print("Time per epoch: %5.2f sec" % (total / epochs))
    return history


def _post_fit(flow, plan, x, history, group):
    """The 16-bit images follow the trained float32 parameters, and the 16-bit inverse sweep is checked on them."""
    if getattr(flow, "_bf16", None) is not None or getattr(flow, "_lane16", None) is not None:
        flow.repack()
    if getattr(flow, "_lane16", None) is not None:
        # the 16-bit sweep's safety net: compared with the float32 sweep on the latent image of the training rows
        # (what mcmc.py:88 inverts), float32 from here on if it is not an inverse within the bounds
        guard = flow.check_inverse_precision(theta=flow.forward(x[:4096])[0], rows=4096)
        if guard is not None:
            if plan.sharded:
                # every rank takes the same sweep: one rank's fallback is everybody's
                flag = torch.tensor([0.0 if guard["passed"] else 1.0], device=flow.device)
                dist.all_reduce(flag, group=group)
                if float(flag.item()) > 0 and guard["passed"]:
                    flow._desc.lane16 = None
                    guard["passed"] = False
            history["inverse_guard"] = guard


def fit_flow(flow, x, weights=None, validation_split=0.0, epochs=1000, batch_size=1000, patience=20,
             learning_rate=1e-3, weight_decay=0, laplace_scale=None, gaussian_scale=None, annealing=True,
             noise=None, shuffle=True, clip_grad_norm=1.0, verbose=0, group=None, sharded=None):
    """``sharded`` (default: a ``torch.distributed`` group with more than one rank exists): ``x`` / ``weights`` are THIS rank's
    shard of the training rows (equal shard sizes), ``batch_size`` is the global batch; gradients and losses are all-reduced
    (RCCL on the GPUs) so that every rank takes the same optimizer steps and the same early-stopping decisions."""
    x, (x_train, w_train, x_valid, w_valid) = _prepare_data(flow, x, weights, validation_split, shuffle)
    penalty = None                                  # flow.py:304-307, :314-315: see pmc_weight_penalty in the header
    if laplace_scale is not None or gaussian_scale is not None:
        penalty = partial(_add_penalty, flow, (float(laplace_scale or 0.0), float(gaussian_scale or 0.0), _weight_flags(flow)))
    plan = _FitPlan(flow, x_valid, batch_size, shuffle, penalty is not None, annealing, group, sharded)
    noise = _noise_setup(flow, x, noise, plan, group)
    opt = AdamW(flow, learning_rate, weight_decay)
    sched = ReduceLROnPlateau(opt, patience) if annealing else None
    _train_state(flow).repack(flow)
    slots = _FitSlots(flow, plan, x_train, x_valid, shuffle, noise, dist.get_rank(group) if plan.sharded else 0)

    # the mode's functions, bound once: an epoch of the Sampler's fits is 75-120 us and bound by the host's enqueue
    if plan.train_mode == "sharded":
        train = partial(_train_sharded, flow, opt, group=group, penalty=penalty)
    elif plan.train_mode == "penalised":
        train = partial(_train_penalised, flow, opt, penalty=penalty)
    else:
        train = partial(opt.epoch, stream=slots.main.cuda_stream)
    train = [partial(train, w=w_train, batch_size=batch_size, max_norm=clip_grad_norm, loss_acc=a) for a in slots.acc_train]
    if plan.fused_staging:                          # (the epoch's last step writes the parameters behind it itself)
        train = [partial(t, snapshot=p) for t, p in zip(train, slots.after)]
    validate = None
    local_batch = max(1, int(batch_size) // plan.world) if plan.sharded else int(batch_size)
    if plan.valid_mode == "sharded":
        validate = partial(_valid_sharded, flow, slots, w_valid, local_batch, shuffle, group)
    elif plan.valid_mode is not None:
        if getattr(flow._train, "logp_scratch", None) is None or flow._train.logp_scratch.numel() < plan.n_valid:
            flow._train.logp_scratch = torch.empty(plan.n_valid, dtype=torch.float32, device=flow.device)
        stream = slots.side if plan.valid_mode == "call_side" else slots.main
        validate = partial(_valid_epoch_call, flow, slots, w_valid, batch_size, C.c_void_p(stream.cuda_stream))
    valid_penalty = None
    if plan.validation and penalty is not None:     # flow.py:342-343: every validation batch's loss carries the penalty
        valid_penalty = partial(penalty, None, mult=-(-plan.n_valid // local_batch))
    enqueue = partial(_enqueue, slots, plan.slots, train, validate,
                      partial(dist.all_reduce, group=group) if plan.sharded else None, valid_penalty, x_train, x_valid)

    history = _host_loop(flow, plan, slots, enqueue, sched, epochs, patience, verbose)
    slots.release()
    _post_fit(flow, plan, x, history, group)
    return history
