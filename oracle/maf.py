"""ORACLE (test infrastructure, never shipped, never measured as the product).

CPU restatement of the masked autoregressive flow behind ``pocomc.flow.Flow``.

PARITY UNPINNED: the flow arithmetic is not in ``/root/reference``; it lives in
the third-party package ``zuko`` (``requirements.txt:3``: ``zuko>=1.1.0``, no
lockfile, not installed, not installable here).  The reference call sites are
``pocomc/flow.py:55-68`` (constructor), ``:114`` (``transform.call_and_ladj``),
``:131`` (``transform.inv.call_and_ladj``), ``:147`` (``log_prob``), ``:162``
(``rsample_and_log_prob``).  The reference's tests hold no numeric expected
values for it (``tests/test_flow.py`` is property-only), so this file restates
zuko's *published* algorithm (see ``pocomc_amd/maf_spec.py`` for the exact
architecture) and is pinned only by those properties:
round trip <= 1e-5 (``tests/test_flow.py:88``), ``ladj_fwd == -ladj_inv``
(``:164``, ``:205``), shapes / dtypes / finiteness.

Everything here is float32 like the reference (``pocomc/tools.py:279-292``).
The inverse is the reference's algorithm: ``D`` fixed-point passes of the full
masked MLP per transform (zuko ``AutoregressiveTransform._inverse``) plus one
pass for the log-determinant.
"""
from __future__ import annotations

import math

import numpy as np

from pocomc_amd.maf_spec import MAFSpec      # the canonical PARAMETER LAYOUT only (offsets / shapes of the flat vector)

F32 = np.float32
LOG_SLOPE = math.log(1e-3)                   # zuko MonotonicAffineTransform / MonotonicRQSTransform: slope = 1e-3


# --------------------------------------------------------------------------
# Masks of zuko's MaskedMLP, built here from zuko's published recipe -- NOT taken from the product
# (``tests/test_oracle_golden.py::test_oracle_masks_equal_the_product_masks`` asserts that the two constructions
# agree).  zuko ``MaskedAutoregressiveTransform``: ``adjacency[o, i] = order[feature(o)] > order[i]`` with
# ``feature(o) = o // total`` (``total`` hyper-network outputs per feature: 2 for the affine map, 3 bins - 1 for the
# spline); zuko ``MaskedMLP(adjacency, hidden_features, residual=True)``:
#     adjacency, inverse = unique(adjacency, dim=0)                 (rows sorted lexicographically)
#     precedence[i, j]   = adjacency[j] is a subset of adjacency[i] (A A^T == row sums)
#     layer 0:      mask = adjacency;              later layers: mask = precedence[:, indices]
#     hidden layer: reachable = rows of mask with any entry; indices = reachable[arange(H) % len(reachable)];
#                   mask = mask[indices]
#     output layer: mask = mask[inverse]
# --------------------------------------------------------------------------
def zuko_masks(order, total, hidden, n_hidden=3):
    """Boolean masks ``[M0 (H, D), M1 (H, H), ..., M_out (total * D, H)]`` for the feature ``order`` (rank per feature)."""
    order = np.asarray(order)
    D = len(order)
    out_order = np.repeat(order, total)
    adjacency = out_order[:, None] > order[None, :]
    adjacency, inverse = np.unique(adjacency, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    a = adjacency.astype(np.int64)
    precedence = (a @ a.T) == a.sum(axis=-1)[None, :]
    masks, indices = [], None
    for i in range(n_hidden + 1):
        mask = adjacency if i == 0 else precedence[:, indices]
        if not mask.any():
            raise ValueError("The adjacency matrix leads to a null Jacobian.")
        if i < n_hidden:
            reachable = np.flatnonzero(mask.sum(axis=-1))
            indices = reachable[np.arange(hidden) % len(reachable)]
            mask = mask[indices]
        else:
            mask = mask[inverse]
        masks.append(mask)
    return masks


def soft_log_scale(raw):
    """zuko ``MonotonicAffineTransform``: ``scale / (1 + |scale / log(slope)|)`` (in the dtype of ``raw``)."""
    F = raw.dtype.type
    return (raw / (F(1.0) + np.abs(raw / F(LOG_SLOPE)))).astype(F)


# --------------------------------------------------------------------------
# NSF univariate: zuko ``MonotonicRQSTransform(widths, heights, derivatives, bound=5, slope=1e-3)``
# (pocomc/flow.py:69-86 builds ``zuko.flows.NSF(bins=8)``).  PARITY UNPINNED like the rest of the
# flow: restated from zuko's published definition --
#   widths, heights: ``v / (1 + |2 v / log(slope)|)`` -> softmax -> knots ``bound * (2 cumsum - 1)``
#   derivatives:     ``v / (1 + |v / log(slope)|)`` -> exp, end knots have derivative 1
#   bin ``k = searchsorted(knots, x) - 1``; outside ``[0, K)`` the map is the identity
#   (Durkan et al. 2019 rational-quadratic spline inside).
# --------------------------------------------------------------------------
RQS_BOUND = 5.0


def _rqs_knots(phi, K, xp):
    """phi (..., 3K-1) -> knots x (..., K+1), y (..., K+1), derivatives (..., K+1)."""
    ls = LOG_SLOPE
    w, h, d = phi[..., :K], phi[..., K:2 * K], phi[..., 2 * K:]
    w = w / (1 + abs(2 * w / ls))
    h = h / (1 + abs(2 * h / ls))
    d = d / (1 + abs(d / ls))
    if xp is np:
        F = phi.dtype.type                          # float32 like the reference; float64 for the yardstick evaluation

        def softmax(v):
            e = np.exp(v - v.max(axis=-1, keepdims=True))
            return (e / e.sum(axis=-1, keepdims=True, dtype=F)).astype(F)
        zero = np.zeros(phi.shape[:-1] + (1,), dtype=F)
        xk = (F(RQS_BOUND) * (2 * np.cumsum(np.concatenate([zero, softmax(w)], -1), axis=-1, dtype=F) - 1)).astype(F)
        yk = (F(RQS_BOUND) * (2 * np.cumsum(np.concatenate([zero, softmax(h)], -1), axis=-1, dtype=F) - 1)).astype(F)
        dk = np.exp(np.concatenate([zero, d, zero], -1)).astype(F)
        return xk, yk, dk
    import torch
    zero = torch.zeros(phi.shape[:-1] + (1,), dtype=phi.dtype)
    xk = RQS_BOUND * (2 * torch.cumsum(torch.cat([zero, torch.softmax(w, -1)], -1), -1) - 1)
    yk = RQS_BOUND * (2 * torch.cumsum(torch.cat([zero, torch.softmax(h, -1)], -1), -1) - 1)
    dk = torch.exp(torch.cat([zero, d, zero], -1))
    return xk, yk, dk


def _take(a, k, xp):
    if xp is np:
        return np.take_along_axis(a, k[..., None], axis=-1)[..., 0]
    return a.gather(-1, k[..., None])[..., 0]


def rqs_forward(x, phi, K=8, xp=np, tables=None):
    """``y, ladj`` of the spline at ``x`` (..., ) with parameters ``phi`` (..., 3K-1).  ``tables``: a function applied to the
    knots ``(xk, yk, dk)`` before use (the sensitivity envelope of tests/flow_regimes.py perturbs them)."""
    xk, yk, dk = _rqs_knots(phi, K, xp)
    if tables is not None:
        xk, yk, dk = tables(xk, yk, dk)
    k = (xk < x[..., None]).sum(-1) - 1                  # searchsorted(knots, x) - 1
    mask = (k >= 0) & (k < K)
    kc = k.clip(0, K - 1) if xp is np else k.clamp(0, K - 1)
    x0, x1 = _take(xk, kc, xp), _take(xk, kc + 1, xp)
    y0, y1 = _take(yk, kc, xp), _take(yk, kc + 1, xp)
    d0, d1 = _take(dk, kc, xp), _take(dk, kc + 1, xp)
    s = (y1 - y0) / (x1 - x0)
    z = (x - x0) / (x1 - x0)
    z = xp.where(mask, z, xp.zeros_like(z))
    den = s + (d0 + d1 - 2 * s) * z * (1 - z)
    y = y0 + (y1 - y0) * (s * z * z + d0 * z * (1 - z)) / den
    jac = s * s * (2 * s * z * (1 - z) + d0 * (1 - z) ** 2 + d1 * z * z) / (den * den)
    ladj = xp.log(jac)
    return xp.where(mask, y, x), xp.where(mask, ladj, xp.zeros_like(ladj))


def rqs_inverse(y, phi, K=8, xp=np, tables=None):
    """``x, ladj_forward(x)`` with ``rqs_forward(x) = y``."""
    xk, yk, dk = _rqs_knots(phi, K, xp)
    if tables is not None:
        xk, yk, dk = tables(xk, yk, dk)
    k = (yk < y[..., None]).sum(-1) - 1
    mask = (k >= 0) & (k < K)
    kc = k.clip(0, K - 1) if xp is np else k.clamp(0, K - 1)
    x0, x1 = _take(xk, kc, xp), _take(xk, kc + 1, xp)
    y0, y1 = _take(yk, kc, xp), _take(yk, kc + 1, xp)
    d0, d1 = _take(dk, kc, xp), _take(dk, kc + 1, xp)
    s = (y1 - y0) / (x1 - x0)
    y_ = xp.where(mask, y - y0, xp.zeros_like(y))
    a = (y1 - y0) * (s - d0) + y_ * (d0 + d1 - 2 * s)
    b = (y1 - y0) * d0 - y_ * (d0 + d1 - 2 * s)
    c = -s * y_
    z = 2 * c / (-b - xp.sqrt(b * b - 4 * a * c))
    x = x0 + z * (x1 - x0)
    den = s + (d0 + d1 - 2 * s) * z * (1 - z)
    jac = s * s * (2 * s * z * (1 - z) + d0 * (1 - z) ** 2 + d1 * z * z) / (den * den)
    ladj = xp.log(jac)
    return xp.where(mask, x, y), xp.where(mask, ladj, xp.zeros_like(ladj))


class OracleMAF:
    """float32 numpy MAF / NSF with the canonical parameter vector of ``MAFSpec``."""

    def __init__(self, spec: MAFSpec, flat: np.ndarray, dtype=F32):
        """``dtype=np.float64``: the SAME float32 parameters, every operation of the flow in float64 -- the yardstick
        for two float32 evaluations (this file's, a kernel's) of an ill-conditioned map such as the spline."""
        self.spec = spec
        self.F = F = np.dtype(dtype).type
        self.tables = None                   # optional hook on the spline's knots (rqs_forward / rqs_inverse)
        self.flat = np.asarray(flat, dtype=F32)
        assert self.flat.shape == (spec.n_params,)
        self._mats = []
        D = spec.n_dim
        for t in range(spec.n_transforms):
            # zuko MAF / NSF: the feature order alternates identity / reversed per transform
            order = np.arange(D) if t % 2 == 0 else np.arange(D)[::-1]
            M0, M1, M2, M3 = zuko_masks(order, spec.n_out, spec.hidden)
            v = lambda n: spec.view(self.flat, t, n)
            self._mats.append(dict(
                W0=(v("W0") * M0).astype(F), b0=v("b0").astype(F),
                W1=(v("W1") * M1).astype(F), b1=v("b1").astype(F),
                W2=(v("W2") * M2).astype(F), b2=v("b2").astype(F),
                W3=(v("W3") * M3).astype(F), b3=v("b3").astype(F)))

    # hyper-network of one transform: x (N,D) -> phi (N, D, n_out)
    def _phi(self, t: int, x: np.ndarray):
        m = self._mats[t]
        h = np.maximum(x @ m["W0"].T + m["b0"], self.F(0))
        h = np.maximum(h + (h @ m["W1"].T + m["b1"]), self.F(0))
        h = np.maximum(h + (h @ m["W2"].T + m["b2"]), self.F(0))
        phi = (h @ m["W3"].T + m["b3"]).astype(self.F)
        return phi.reshape(len(x), self.spec.n_dim, self.spec.n_out)

    def _hyper(self, t: int, x: np.ndarray):
        """affine flows: ``(shift, soft-clipped log-scale)`` of transform t."""
        phi = self._phi(t, x)
        return phi[..., 0], soft_log_scale(phi[..., 1])

    def _fwd(self, t, x):
        """univariate maps of transform t at x: ``(y, per-feature ladj)``."""
        phi = self._phi(t, x)
        if self.spec.univariate == "affine":
            ls = soft_log_scale(phi[..., 1])
            return (x * np.exp(ls) + phi[..., 0]).astype(self.F), ls
        y, l = rqs_forward(x, phi, self.spec.bins, tables=self.tables)
        return y.astype(self.F), l.astype(self.F)

    def _inv(self, t, xcur, y):
        """one fixed-point pass: parameters from ``xcur``, inverse univariate applied to ``y``."""
        phi = self._phi(t, xcur)
        if self.spec.univariate == "affine":
            ls = soft_log_scale(phi[..., 1])
            return ((y - phi[..., 0]) / np.exp(ls)).astype(self.F), ls
        x, l = rqs_inverse(y, phi, self.spec.bins, tables=self.tables)
        return x.astype(self.F), l.astype(self.F)

    def forward(self, x):
        """data -> latent, ``(z, ladj)``; ``pocomc/flow.py:99-114``."""
        x = np.asarray(x, dtype=self.F)
        ladj = np.zeros(len(x), dtype=self.F)
        for t in range(self.spec.n_transforms):
            x, l = self._fwd(t, x)
            ladj = (ladj + l.sum(axis=1, dtype=self.F)).astype(self.F)
        return x, ladj

    def ladj_abs_terms(self, x):
        """``sum_j |ladj term_j|`` of ``forward(x)`` per row, in float64 (test infrastructure): the size of the terms
        the log-determinant sums.  The terms have either sign, so two valid float32 evaluations of the sum (zuko's, this
        file's, a kernel's) agree to ``eps * sum|terms|``, not to ``eps * |sum|``: parity tests measure a
        log-determinant's error against this figure (the condition of the sum), never against a global maximum."""
        x = np.asarray(x, dtype=self.F)
        acc = np.zeros(len(x), dtype=np.float64)
        for t in range(self.spec.n_transforms):
            x, l = self._fwd(t, x)
            acc += np.abs(l.astype(np.float64)).sum(axis=1)
        return acc

    def inverse(self, z):
        """latent -> data, ``(x, ladj)``; ``pocomc/flow.py:116-132``.  ``ladj`` is
        the log-determinant of the inverse map (= ``-ladj_forward(x)``)."""
        y = np.asarray(z, dtype=self.F)
        D = self.spec.n_dim
        ladj = np.zeros(len(y), dtype=self.F)
        for t in reversed(range(self.spec.n_transforms)):
            x = np.zeros_like(y)
            for _ in range(D):                      # zuko: passes = features
                x, _l = self._inv(t, x, y)
            _x, l = self._inv(t, x, y)              # extra pass for the ladj
            ladj = (ladj - l.sum(axis=1, dtype=self.F)).astype(self.F)
            y = x
        return y, ladj

    def log_prob(self, x):
        """``pocomc/flow.py:134-147``: base ``N(0,I)`` log-density + ladj."""
        z, ladj = self.forward(x)
        D = self.spec.n_dim
        base = (-0.5 * (z.astype(self.F) ** 2).sum(axis=1, dtype=self.F)
                - self.F(0.5 * D * math.log(2 * math.pi))).astype(self.F)
        return (base + ladj).astype(self.F)

    def sample_from(self, z):
        """``pocomc/flow.py:149-163`` with the base draw ``z`` given (replay)."""
        x, ladj_inv = self.inverse(z)
        D = self.spec.n_dim
        base = (-0.5 * (np.asarray(z, self.F) ** 2).sum(axis=1, dtype=self.F)
                - self.F(0.5 * D * math.log(2 * math.pi))).astype(self.F)
        # log q(x) = log N(z) + ladj_forward(x) = log N(z) - ladj_inverse(z)
        return x, (base - ladj_inv).astype(self.F)


class TorchFlowAdapter:
    """Duck-typed ``pocomc.flow.Flow`` contract (``pocomc/tools.py:336-349``):
    ``forward/inverse`` on float32 torch tensors, backed by ``OracleMAF``.
    Lets the reference's own ``pocomc.mcmc`` kernels run on this flow when
    golden vectors are generated."""

    def __init__(self, maf: OracleMAF):
        self.maf = maf
        self.n_dim = maf.spec.n_dim

    def forward(self, x):
        import torch
        z, l = self.maf.forward(x.detach().numpy())
        return torch.from_numpy(z), torch.from_numpy(l)

    def inverse(self, u):
        import torch
        x, l = self.maf.inverse(u.detach().numpy())
        return torch.from_numpy(x), torch.from_numpy(l)


# --------------------------------------------------------------------------
# torch-autograd twin: the fp32 reference for the training kernels
# --------------------------------------------------------------------------
def torch_log_prob(spec: MAFSpec, flat_t, x_t):
    """Differentiable ``log_prob`` on a flat torch parameter vector."""
    import torch
    D = spec.n_dim
    x = x_t
    ladj = torch.zeros(x.shape[0], dtype=x.dtype)
    for t in range(spec.n_transforms):
        M = [torch.from_numpy(m.astype(np.float32)) for m in spec.masks(t)]
        def v(name):
            off, sz = spec.offsets[name]
            b = t * spec.params_per_transform + off
            return flat_t[b:b + sz].reshape(spec.shapes()[name])
        h = torch.relu(x @ (v("W0") * M[0]).T + v("b0"))
        h = torch.relu(h + h @ (v("W1") * M[1]).T + v("b1"))
        h = torch.relu(h + h @ (v("W2") * M[2]).T + v("b2"))
        phi = (h @ (v("W3") * M[3]).T + v("b3")).reshape(x.shape[0], D, spec.n_out)
        if spec.univariate == "affine":
            shift, raw = phi[..., 0], phi[..., 1]
            ls = raw / (1 + torch.abs(raw / LOG_SLOPE))
            x = x * torch.exp(ls) + shift
        else:
            x, ls = rqs_forward(x, phi, spec.bins, xp=torch)
        ladj = ladj + ls.sum(dim=1)
    base = -0.5 * (x ** 2).sum(dim=1) - 0.5 * D * math.log(2 * math.pi)
    return base + ladj


def torch_loss(spec, flat_t, x_t, w_t=None):
    """``pocomc/flow.py:308-312``: ``-sum(log_prob)`` or the weighted form
    ``-(log_prob * w * 1000).sum() / w.sum()``."""
    lp = torch_log_prob(spec, flat_t, x_t)
    if w_t is None:
        return -lp.sum()
    return (-(lp * w_t * 1000.0)).sum() / w_t.sum()
