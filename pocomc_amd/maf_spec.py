"""Architecture of the masked autoregressive flow (MAF) used on the hot path.

This is host logic only (numpy): mask construction, the canonical parameter
layout and the index maps that pack canonical parameters into the layouts the
gfx950 kernels consume.  No arithmetic of the flow itself lives here.

What it restates
----------------
``pocomc/flow.py:46-68`` builds ``zuko.flows.MAF(n_dim, transforms=T,
hidden_features=[H]*3, residual=True)`` with ``H = max(next_pow2(3*n_dim), 32)``
(``pocomc/flow.py:49-52``).  ``zuko`` is a third-party package that is NOT under
``/root/reference`` (pinned only as ``zuko>=1.1.0`` in ``requirements.txt:3``),
so the architecture below is a restatement of zuko's published MAF, not of a
file in the reference (*parity unpinned*):

* ``T`` masked-autoregressive transforms; variable order alternates identity /
  reversed per transform; base distribution is a diagonal ``N(0, I)``.
* each transform: a masked MLP ``D -> H -> H -> H -> 2D`` with ReLU; the two
  ``H -> H`` layers carry a skip connection (``h' = relu(h + W h + b)``);
  outputs are ``(shift_j, raw_j)`` per feature ``j`` (row ``2j`` / ``2j+1``).
* univariate map ``y = x * exp(ls) + shift`` with the soft-clipped log-scale
  ``ls = raw / (1 + |raw / log(1e-3)|)``; ``ladj = sum_j ls_j``.
* masks (zuko ``MaskedMLP``): hidden unit ``k`` has degree
  ``deg(k) = 1 + k mod (D-1)``; it reads inputs of rank ``< deg(k)`` and hidden
  units of degree ``<= deg(k)``; the outputs of the feature of rank ``r`` read
  hidden units of degree ``<= r`` (rank 0 reads nothing: bias only).

Canonical parameter layout (one flat fp32 vector, transform after transform):
``W0[H,D] b0[H] W1[H,H] b1[H] W2[H,H] b2[H] W3[2D,H] b3[2D]`` with torch
``nn.Linear`` convention ``weight[out, in]``.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

LOG_SLOPE = math.log(1e-3)  # zuko MonotonicAffineTransform slope=1e-3


def next_power_of_2(n: int) -> int:
    """``pocomc/flow.py:49-50``."""
    return 1 if n == 0 else 2 ** (int(n) - 1).bit_length()


def default_hidden(n_dim: int) -> int:
    """``pocomc/flow.py:52``: ``np.maximum(next_power_of_2(3*n_dim), 32)``."""
    return max(next_power_of_2(3 * n_dim), 32)


def _ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------- images and their parts
# A device image is a gather map into the canonical parameter vector.  Every image is cut from the connection matrices of
# MAFSpec.connections (canonical index, or -1: masked, padding slot, rank beyond D) by the helpers below and by nothing else.
_Layout = namedtuple("_Layout", "shapes sizes offsets total")


def _layout(parts):
    """Ordered ``(name, shape)`` list of one transform's parts -> their shapes, sizes, offsets and the total, in elements."""
    shapes = {name: tuple(int(d) for d in shape) for name, shape in parts}
    sizes = {name: math.prod(shape) for name, shape in shapes.items()}
    offsets, total = {}, 0
    for name, sz in sizes.items():
        offsets[name] = total
        total += sz
    return _Layout(shapes, sizes, offsets, total)


def _fill(image, base, layout, parts):
    """Write the arrays ``parts`` (name -> array of the part's shape) into ``image`` from element ``base`` on."""
    for name, a in parts.items():
        o = base + layout.offsets[name]
        image[o:o + layout.sizes[name]].reshape(layout.shapes[name])[...] = a


def _pad(a, shape):
    """``a`` in the leading corner of an array of ``shape``, -1 elsewhere."""
    out = np.full(shape, -1, dtype=a.dtype)
    out[tuple(slice(n) for n in a.shape)] = a
    return out


def _frag_a4(w):
    """A operands of ``mfma_f32_16x16x4f32`` of ``w [rows][k]``: ``[row tile][k tile][lane = 16 k + i][c]`` holds
    ``w[16 row tile + i][16 k tile + 4 c + k]``."""
    R, K = w.shape[0] // 16, w.shape[1] // 16
    return w.reshape(R, 16, K, 4, 4).transpose(0, 2, 4, 1, 3).reshape(R, K, 64, 4)


def _frag_a32(w):
    """A operands of ``v_mfma_f32_16x16x32_bf16`` of ``w [rows][k]``, k padded to 32-wide tiles:
    ``[row tile][k tile][lane = 16 g + i][e]`` holds ``w[16 row tile + i][32 k tile + 8 g + e]``."""
    R, K = w.shape[0] // 16, -(-w.shape[1] // 32)
    return _pad(w, (16 * R, 32 * K)).reshape(R, 16, K, 4, 8).transpose(0, 2, 3, 1, 4).reshape(R, K, 64, 8)


def _frag_c(w):
    """MFMA C layout of the 16 x 16 tiles of ``w [rows][cols]``: ``[row tile][col tile][lane = 16 q + j][r]`` holds
    ``w[16 row tile + 4 q + r][16 col tile + j]``."""
    R, K = w.shape[0] // 16, w.shape[1] // 16
    return w.reshape(R, 4, 4, K, 16).transpose(0, 3, 1, 4, 2).reshape(R, K, 64, 4)


def _frag_chain(blocks):
    """A operands of ``v_mfma_f32_4x4x1_16b_f32`` of the per-tile ``blocks [tile][4 n rows][16 k slots]``:
    ``[tile][lane = 4 k + i][a]`` holds ``blocks[tile][4 a + i][k]`` (one VGPR = a 4 x 16 block)."""
    nT, n = blocks.shape[0], blocks.shape[1] // 4
    return blocks.reshape(nT, n, 4, 16).transpose(0, 3, 2, 1).reshape(nT, 64, n)


@dataclass
class MAFSpec:
    """Static description of one MAF: shapes, masks, packing maps."""

    n_dim: int
    n_transforms: int = 3
    hidden: int | None = None
    univariate: str = "affine"      # "affine" (MAF) | "rqs" (NSF: monotonic rational-quadratic spline)
    bins: int = 8                   # spline bins (pocomc/flow.py:71), ignored for "affine"

    # filled by __post_init__
    orders: list = field(default_factory=list, repr=False)
    # test switch (pmc_maf_t.reserved & PMC_MAF_VARIANT_LEAN_LDS): the float32 kernels' two-array instances also where the
    # full ones fit; the wide default flows take them by themselves
    lean_lds: bool = field(default=False, repr=False, compare=False)

    def __post_init__(self):
        D = int(self.n_dim)
        if D < 2:
            # zuko raises "The adjacency matrix leads to a null Jacobian." for D=1
            raise ValueError("MAF needs n_dim >= 2 (the adjacency matrix of a 1-D "
                             "autoregressive transform leads to a null Jacobian)")
        self.n_dim = D
        self.n_transforms = int(self.n_transforms)
        if self.hidden is None:
            self.hidden = default_hidden(D)
        self.hidden = int(self.hidden)
        H = self.hidden
        if H < D - 1:
            raise NotImplementedError("hidden width must be >= n_dim - 1")
        if self.univariate not in ("affine", "rqs"):
            raise ValueError("univariate must be 'affine' or 'rqs'")
        self.bins = int(self.bins)
        if self.univariate == "rqs" and self.bins not in (4, 8, 16):
            # (the reference builds 8 bins, pocomc/flow.py:71,77,83, and accepts any zuko flow object, :87-88; the element
            #  code is instantiated for these three counts -- csrc/rqs.h -- and only the default 8 has the triangular
            #  inverse sweeps: the others invert with zuko's own D-pass algorithm)
            raise NotImplementedError("spline flows are built for bins in (4, 8, 16)")
        # hyper-network outputs per feature: (shift, raw log-scale) or (K widths, K heights, K-1 derivatives)
        self.n_out = 2 if self.univariate == "affine" else 3 * int(self.bins) - 1
        # rank of every input feature, per transform (zuko MAF: orders[i % 2])
        ident = np.arange(D)
        self.orders = [ident.copy() if t % 2 == 0 else ident[::-1].copy()
                       for t in range(self.n_transforms)]
        # degree of every hidden unit (same for the three hidden layers)
        self.degree = 1 + (np.arange(H) % (D - 1))
        # canonical offsets inside one transform
        _, sizes, off, self.params_per_transform = _layout(self.shapes().items())
        self.offsets = {name: (off[name], sizes[name]) for name in sizes}
        self.n_params = self.params_per_transform * self.n_transforms
        self._build_device_layout()

    # ------------------------------------------------------------------ masks
    def masks(self, t: int):
        """Boolean masks ``(M0[H,D], M1[H,H], M2[H,H], M3[2D,H])`` of transform t."""
        D, H = self.n_dim, self.hidden
        rank = self.orders[t]                      # rank[j] of feature j
        deg = self.degree
        M0 = rank[None, :] < deg[:, None]
        M1 = deg[None, :] <= deg[:, None]
        M3 = deg[None, :] <= np.repeat(rank, self.n_out)[:, None]
        return M0, M1, M1.copy(), M3

    def shapes(self):
        D, H = self.n_dim, self.hidden
        return {"W0": (H, D), "b0": (H,), "W1": (H, H), "b1": (H,),
                "W2": (H, H), "b2": (H,), "W3": (self.n_out * D, H), "b3": (self.n_out * D,)}

    def view(self, flat: np.ndarray, t: int, name: str) -> np.ndarray:
        """View of one canonical tensor inside the flat parameter vector."""
        off, sz = self.offsets[name]
        base = t * self.params_per_transform + off
        return flat[base:base + sz].reshape(self.shapes()[name])

    def mask_flat(self) -> np.ndarray:
        """0/1 float mask over the flat parameter vector (1 for biases)."""
        m = np.ones(self.n_params, dtype=np.float32)
        for t in range(self.n_transforms):
            M0, M1, M2, M3 = self.masks(t)
            for name, M in (("W0", M0), ("W1", M1), ("W2", M2), ("W3", M3)):
                self.view(m, t, name)[...] = M.astype(np.float32)
        return m

    def init_params(self, seed: int | None = None) -> np.ndarray:
        """``nn.Linear`` default init: ``U(-1/sqrt(fan_in), 1/sqrt(fan_in))`` for
        weights and biases (fan_in = unmasked ``in_features``)."""
        rng = np.random.default_rng(seed)
        flat = np.empty(self.n_params, dtype=np.float32)
        fan = {"W0": self.n_dim, "b0": self.n_dim, "W1": self.hidden, "b1": self.hidden,
               "W2": self.hidden, "b2": self.hidden, "W3": self.hidden, "b3": self.hidden}
        for t in range(self.n_transforms):
            for name in self.offsets:
                v = self.view(flat, t, name)
                b = 1.0 / math.sqrt(fan[name])
                v[...] = rng.uniform(-b, b, size=v.shape).astype(np.float32)
        return flat

    # ---------------------------------------------------------- device layout
    def _build_device_layout(self):
        """Slot layout of the gfx950 kernels.

        Hidden units are sorted by degree; every degree group is padded to a
        multiple of 4 slots (one *quad* = the K of one ``mfma_f32_16x16x4f32``)
        and the total to a multiple of 16 (one *tile* = 4 quads = the M of the
        same MFMA).  Features are addressed by rank, padded to ``Dp`` (multiple
        of 16).  Output rows are ``2*rank`` (shift) and ``2*rank+1`` (raw),
        padded to ``Op = 2*Dp``.
        """
        D, H = self.n_dim, self.hidden
        deg = self.degree
        slots = []          # canonical unit index per slot, -1 = padding
        sdeg = []           # degree per slot (D = padding, never reached)
        tri_ok = True
        for g in range(1, D):
            units = np.nonzero(deg == g)[0]
            nq = _ceil_to(len(units), 4) // 4
            if nq <= 4:
                # a degree group never straddles a tile boundary: its units all
                # read each other's previous-layer values, so the sweep of the
                # triangular inverse finishes a group inside one tile
                in_tile = (len(slots) // 4) % 4
                if in_tile + nq > 4:
                    fill = (4 - in_tile) * 4
                    slots += [-1] * fill
                    sdeg += [D] * fill
            else:
                tri_ok = False
            pad = nq * 4 - len(units)
            slots += list(units) + [-1] * pad
            sdeg += [g] * (len(units) + pad)
        self.tri_ok = tri_ok
        Hp = _ceil_to(len(slots), 16)
        slots += [-1] * (Hp - len(slots))
        sdeg += [D] * (Hp - len(sdeg))          # trailing pad: never reached
        self.Hp = Hp
        self.nT = Hp // 16                       # hidden tiles
        self.nQ = Hp // 4                        # hidden quads
        self.Dp = _ceil_to(D, 16)
        self.nXT = self.Dp // 16                 # input (rank) tiles
        self.Op = _ceil_to(self.n_out * self.Dp, 16)   # output rows n_out*rank + j
        self.nOT = self.Op // 16                 # output tiles (8 ranks each for the affine map)
        self.slot_unit = np.asarray(slots, dtype=np.int64)
        self.slot_deg = np.asarray(sdeg, dtype=np.int32)
        qdeg = self.slot_deg.reshape(-1, 4)
        assert (qdeg == qdeg[:, :1]).all()
        qdeg = qdeg[:, 0].copy()
        # a quad is "last" of its degree if the next quad has a different degree
        qlast = np.ones(self.nQ, dtype=np.int32)
        qlast[:-1] = (qdeg[1:] != qdeg[:-1]).astype(np.int32)
        qlast[qdeg >= D] = 0                     # padding quads trigger nothing
        self.quad_deg = qdeg
        self.quad_last = qlast
        # quad meta word: degree | last << 16
        self.quad_meta = (qdeg.astype(np.int32) | (qlast << 16)).astype(np.int32)

        # ---- the parts of the packed image (floats), per transform
        D, Hp, Dp, nT, nXT, nOT = self.n_dim, self.Hp, self.Dp, self.nT, self.nXT, self.nOT
        parts = [("f0", (nT, nXT, 64, 4)),       # W0 fragments  [tile][xtile][lane][4]
                 ("f1", (nT, nT, 64, 4)),        # W1/W2 fragments [tile][ktile][lane][4]
                 ("f2", (nT, nT, 64, 4)),
                 ("f3", (nOT, nT, 64, 4)),       # W3 fragments  [otile][ktile][lane][4]
                 ("w0n", (Dp, Hp)),              # W0 natural    [rank][slot]
                 ("b0", (Hp,)), ("b1", (Hp,)), ("b2", (Hp,)),    # b0,b1,b2 [slot]
                 ("b3", (self.Op,))]             # b3            [n_out*rank + s]
        if self.univariate == "rqs" and self.bins == 8:
            # inverse sweep: the 23 output rows of every rank padded to two 16-row tiles of their own
            parts += [("f3i", (D, 2, nT, 64, 4)),     # [rank][half][ktile][lane][4]
                      ("b3i", (D, 32))]               # [rank][32]
            # the two-wave spline sweep (csrc/maf_inverse_nsf2.hip) shares the affine two-wave sweep's hidden part: the
            # layer-0 window columns (cw0), the masked layer-0 fragments (f0c), the transposed biases -- see below
            parts += [("cw0", (nT, 64, 4)), ("f0c", (nT, nXT, 64, 4)), ("b0t", (Hp,)), ("b1t", (Hp,)), ("b2t", (Hp,))]
        elif self.univariate == "affine":
            # chain image of the lane-per-walker inverse sweep (csrc/maf_inverse_tri6.hip): A operands of
            # v_mfma_f32_4x4x1_16b_f32 -- lane l holds W[out quad row l & 3][k slot l >> 2], one VGPR = a 4 x 16 block --
            # for the diagonal tile of the hidden layers (cw1, cw2: [tile][lane][out quad]), the layer-0 columns of the
            # ranks the previous and the own tile produce (cw0: k slots 0-3 / 4-7) and the output rows of the own
            # tile's ranks (cw3: [tile][lane][pair of groups]); f0c = f0 with the columns of those ranks zeroed (what
            # the helper wavefront multiplies while the chain adds the newest ranks from registers)
            parts += [("cw1", (nT, 64, 4)), ("cw2", (nT, 64, 4)), ("cw0", (nT, 64, 4)), ("cw3", (nT, 64, 2)),
                      ("f0c", (nT, nXT, 64, 4))]
            # the hidden layers' biases with the rows of every tile transposed (slot 16 T + 4 q + r holds the bias of unit
            # 16 T + 4 r + q): what a lane of the two-wave sweep's transposed accumulators (csrc/maf_chain_rot.h) starts
            # from, one 16-byte load per tile
            parts += [("b0t", (Hp,)), ("b1t", (Hp,)), ("b2t", (Hp,))]
        self.pk_shapes, sizes, self.pk_offsets, self.pk_per_transform = _layout(parts)
        self.pk_size = self.pk_per_transform * self.n_transforms
        for attr, name in (("f0", "f0"), ("f12", "f1"), ("f3", "f3"), ("w0n", "w0n"), ("b", "b0"), ("b3", "b3"),
                           ("f3i", "f3i"), ("b3i", "b3i")):
            if name in sizes:
                setattr(self, "sz_" + attr, sizes[name])

    def packed_view(self, image: np.ndarray, t: int, name: str) -> np.ndarray:
        """View of one part of transform t inside a packed image (or its gather map), in the part's shape
        (``pk_shapes``): the sibling of :meth:`view` for the canonical vector."""
        base = t * self.pk_per_transform + self.pk_offsets[name]
        shape = self.pk_shapes[name]
        return image[base:base + math.prod(shape)].reshape(shape)

    # ------------------------------------------------------------- connections
    def connections(self, by_rank: bool = True, tile: int = 16):
        """Per transform, in turn, its index matrices in device coordinates: name -> canonical flat index of every entry of
        ``W0 [Hp][Dp]  W1, W2 [Hp][Hp]  W3 [Op][Hp]  b0, b1, b2 [Hp]  b3 [Op]``, or -1 where the connection is masked, the
        slot is padding or the rank is beyond ``D``.  Hidden units are addressed by slot, features by rank and output
        rows are ``n_out * rank + s``; with ``by_rank=False`` features and output rows are in canonical order (the
        row-major training image).  ``tile``: slots and features are padded to a multiple of it (16: ``Hp`` and ``Dp``).

        Every device image is a re-tiling of these matrices: this is the one place that reads a mask or meets a padding
        slot or a rank beyond ``D``; the canonical index of an entry is its position in :meth:`view`."""
        D, NO = self.n_dim, self.n_out
        su = _pad(self.slot_unit, (_ceil_to(self.Hp, tile),))            # canonical unit of every slot, -1 = padding
        canonical, absent = np.arange(self.n_params, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        for t in range(self.n_transforms):
            feat = _pad(np.argsort(self.orders[t]) if by_rank else np.arange(D), (_ceil_to(D, tile),))     # -1 beyond D
            orow = np.where(feat[:, None] >= 0, NO * feat[:, None] + np.arange(NO), -1).reshape(-1)
            M0, M1, M2, M3 = self.masks(t)
            out = {}
            for name, mask, rows, cols in (("W0", M0, su, feat), ("W1", M1, su, su), ("W2", M2, su, su), ("W3", M3, orow, su)):
                # the canonical tensor's own indices where unmasked, behind them one more row and column of -1: what an
                # index of -1 reads
                v = self.view(canonical, t, name)
                c = np.full((v.shape[0] + 1, v.shape[1] + 1), -1, dtype=np.int32)
                np.copyto(c[:-1, :-1], v, where=mask)
                out[name] = c.take(rows, axis=0).take(cols, axis=1)
                # its bias: one per row
                b = self.view(canonical, t, "b" + name[1])
                out["b" + name[1]] = np.concatenate((b, absent)).take(rows)
            yield out

    def pack_index(self) -> np.ndarray:
        """int32 gather map: ``packed[i] = flat[idx[i]] if idx[i] >= 0 else 0``.

        Masked-out weights map to -1 (exact zeros in the packed image), so the
        kernels never need the masks.
        """
        D, NO, Hp, Dp, nT = self.n_dim, self.n_out, self.Hp, self.Dp, self.nT
        idx = np.full(self.pk_size, -1, dtype=np.int32)
        sweeps = "cw0" in self.pk_shapes                 # the sweeps' images (cw1 / cw2 / cw3: the affine one only)
        if sweeps:
            # per tile: the rank of every k slot of the layer-0 window (-1: none), the ranks its own groups produce and
            # the first rank the chain adds itself
            tg = self.tile_groups()                      # per tile: degrees of its groups (in order)
            win = np.full((nT, 16), -1, dtype=np.int64)
            own = np.full((nT, 4), -1, dtype=np.int64)
            cut = np.zeros(nT, dtype=np.int64)
            for T in range(nT):
                prev = [0] if T == 0 else tg[T - 1]      # ranks produced before this tile's chain starts its own
                win[T, :len(prev)] = prev
                own[T, :len(tg[T])] = tg[T]
                cut[T] = 0 if T == 0 else (prev[0] if prev else D)
            win[:, 4:8] = own
            before_cut = np.arange(Dp) < np.repeat(cut, 16)[:, None]     # [slot][rank]
            tiles = np.arange(nT)
            diagonal = lambda w: w.reshape(nT, 16, nT, 16)[tiles, :, tiles, :]      # [tile][out slot][in slot] of the tiles (T, T)
        for t, c in enumerate(self.connections()):
            W0, W1, W2, W3 = c["W0"], c["W1"], c["W2"], c["W3"]
            # --- fragments: A[i][k] = W[out slot (row of (rank, s)) 16*T+i][in rank (slot) 16*K + 4c + k]
            img = {"f0": _frag_a4(W0), "f1": _frag_a4(W1), "f2": _frag_a4(W2), "f3": _frag_a4(W3), "w0n": W0.T,
                   "b0": c["b0"], "b1": c["b1"], "b2": c["b2"], "b3": c["b3"]}
            if sweeps:
                # layer 0: the window's columns as the chain's operand (column Dp: a k slot without a rank), and the
                # fragments without the columns at and above the tile's cut
                W0w = _pad(W0, (Hp, Dp + 1)).reshape(nT, 16, Dp + 1)
                img["cw0"] = _frag_chain(np.take_along_axis(W0w, win[:, None, :], axis=2))
                img["f0c"] = _frag_a4(np.where(before_cut, W0, -1))
                for b in ("b0", "b1", "b2"):
                    img[b + "t"] = c[b].reshape(nT, 4, 4).transpose(0, 2, 1).reshape(Hp)
            if "cw1" in self.pk_shapes:
                # the chain's diagonal tiles of the hidden layers, and the rows (rank, s) of the own tile's ranks against
                # the own tile's slots (rank Dp: a group the tile does not have)
                W3r = _pad(W3.reshape(Dp, NO, nT, 16), (Dp + 1, NO, nT, 16))
                img["cw1"], img["cw2"] = _frag_chain(diagonal(W1)), _frag_chain(diagonal(W2))
                img["cw3"] = _frag_chain(W3r[own, :, tiles[:, None], :].reshape(nT, 4 * NO, 16))
            if "f3i" in self.pk_shapes:
                # the NO output rows of every rank at the head of 32 rows of their own
                W3i = _pad(W3[:NO * D].reshape(D, NO, Hp), (D, 32, Hp))
                img["f3i"] = _frag_a4(W3i.reshape(32 * D, Hp)).reshape(D, 2, nT, 64, 4)
                img["b3i"] = _pad(c["b3"][:NO * D].reshape(D, NO), (D, 32))
            assert img.keys() == self.pk_shapes.keys()
            for name, a in img.items():
                self.packed_view(idx, t, name)[...] = a
        return idx

    def tile_groups(self):
        """Per hidden tile: the degrees (= the ranks they produce) of its degree groups, in slot order."""
        out = []
        for T in range(self.nT):
            dq = self.quad_deg[4 * T:4 * T + 4]
            g = []
            for d in dq:
                if d < self.n_dim and (not g or g[-1] != d):
                    g.append(int(d))
            out.append(g)
        return out

    @property
    def has_sweep_tables(self) -> bool:
        """The flows the two-wave affine sweep (``csrc/maf_inverse_tri4.hip``: ``maf_inverse_tri5_kernel``) covers: their
        metadata carries the sweep's table image (:meth:`sweep_tables`)."""
        return bool(self.n_out == 2 and self.tri_ok and self.nOT <= 8 and self.n_dim <= 64)

    def sweep_tables(self) -> np.ndarray:
        """The constant tables of the two-wave affine sweep in the layout of its LDS, so that a workgroup copies them instead
        of deriving them (``pmc_maf_t.reserved & PMC_MAF_TABLES``; the kernel's own construction -- ``fill_table`` and the
        ``YT`` loop, the same integer arithmetic -- stays for an image without them):

        ``DGT [(nT+2)][16]``  per hidden tile (two rows of "no groups" behind the last): the ranks its four degree groups
                              produce (word 0 also: the quad pattern << 16), the byte offsets of each rank's x / y word, of
                              its (shift, raw) pair in a staged output tile and of its two rows in an output fragment record
        ``PRM [Dp]``          feature of every rank of transform 0
        ``YT  [T][nT+2][4]``  byte offset of the y word of the rank a group produces, in the x array of transform t + 1
        ``Y0T [T]``           the same for rank 0; zeros up to a multiple of 4 words
        """
        D, T, nT, Dp = self.n_dim, self.n_transforms, self.nT, self.Dp
        oob = 0x40000000
        f_o_r = [np.argsort(o) for o in self.orders]
        r_o_f = self.orders
        deg = (self.quad_meta & 0xffff).astype(np.int64)
        dgt = np.zeros((nT + 2, 16), dtype=np.int64)
        for tile in range(nT + 2):
            g4, pat = [D] * 4, 1
            if tile < nT:
                x, y, z, w = (int(v) for v in deg[4 * tile:4 * tile + 4])
                ny, nz, nw = y != x, z != y, w != z
                pat = 1 | (ny << 1) | (nz << 2) | (nw << 3)
                g1 = y if ny else (z if nz else (w if nw else D))
                g2 = (z if nz else (w if nw else D)) if ny else (w if (nz and nw) else D)
                g3 = w if (ny and nz and nw) else D
                g4 = [x, g1, g2, g3]
            for k in range(16):
                i = k & 3
                g = g4[i]
                live = g < D
                gg = g if live else 0
                if k < 4:
                    v = g | ((pat << 16) if i == 0 else 0)
                elif k < 8:
                    v = 4 * (((gg >> 4) << 8) + ((gg & 3) << 6) + ((gg >> 2) & 3))
                elif k < 12:
                    v = 4 * ((gg >> 3) * 256 + 2 * (gg & 7))
                else:
                    v = (((((gg >> 3) * nT) << 6) + 2 * (gg & 7)) << 4) if live else oob
                dgt[tile, k] = v
        woff = lambda r: 4 * (((r >> 4) << 8) + ((r & 3) << 6) + ((r >> 2) & 3))

        def src_rank(tt, g):                              # where rank g of transform tt sits in its input array
            if g >= D:
                return 0
            return g if tt == T - 1 else int(r_o_f[tt + 1][f_o_r[tt][g]])
        yt = np.zeros((T, nT + 2, 4), dtype=np.int64)
        for tt in range(T):
            for tile in range(nT + 2):
                for i in range(4):
                    yt[tt, tile, i] = woff(src_rank(tt, int(dgt[tile, i]) & 0xffff))
        y0t = np.array([woff(src_rank(tt, 0)) for tt in range(T)], dtype=np.int64)
        prm = np.zeros(Dp, dtype=np.int64)
        prm[:D] = f_o_r[0]
        tail = np.concatenate([yt.reshape(-1), y0t])
        tail = np.concatenate([tail, np.zeros(-len(tail) % 4, dtype=np.int64)])
        return np.concatenate([dgt.reshape(-1), prm, tail]).astype(np.int32)

    def device_meta(self) -> np.ndarray:
        """int32 metadata consumed by the kernels.

        ``[0:8]``  header: D, H, T, Hp, Dp, nT, pk_per_transform, live hidden tiles
        ``[8:8+T*D]``        feature index of every rank, per transform
        ``[8+T*D:8+2*T*D]``  rank of every feature, per transform
        ``[8+2*T*D: +nQ]``   quad meta words (degree | last<<16), shared by all transforms
        behind them, from the next multiple of 4 words: :meth:`sweep_tables` (``has_sweep_tables``)
        """
        D, T = self.n_dim, self.n_transforms
        live = int(np.sum((self.quad_deg.reshape(-1, 4) < D).any(axis=1)))      # hidden tiles with a degree group (the padding tiles trail)
        hdr = np.array([D, self.hidden, T, self.Hp, self.Dp, self.nT,
                        self.pk_per_transform, live], dtype=np.int32)
        f_o_r = np.concatenate([np.argsort(o) for o in self.orders]).astype(np.int32)
        r_o_f = np.concatenate(self.orders).astype(np.int32)
        meta = np.concatenate([hdr, f_o_r, r_o_f, self.quad_meta]).astype(np.int32)
        if self.has_sweep_tables:
            meta = np.concatenate([meta, np.zeros(-len(meta) % 4, dtype=np.int32), self.sweep_tables()])
        return meta

    # ------------------------------------------------------- bf16 forward image
    def bf16_layout(self):
        """Sizes / offsets (in bf16 elements, per transform) of the weight fragments of the bf16 forward kernel
        (``csrc/maf_forward_bf16.hip``): A operands of ``v_mfma_f32_16x16x32_bf16`` -- lane l holds row ``l & 15`` of the
        16-row out tile and the 8 consecutive k ``8 (l >> 4) .. + 7`` of a 32-wide k tile --
        ``g0 [nT][nX2]``, ``g1 / g2 [nT][nK2]``, ``g3 [nOT][nK2]``, each ``[64 lanes][8]``; biases stay float32 (they are
        read from the float32 image)."""
        nX2, nK2, (_, sz, off, total) = self._bf16_parts()
        return dict(nX2=nX2, nK2=nK2, sz=sz, off=off, per_transform=total)

    def _bf16_parts(self):
        nX2, nK2 = -(-self.Dp // 32), -(-self.Hp // 32)
        return nX2, nK2, _layout([("g0", (self.nT, nX2, 64, 8)), ("g1", (self.nT, nK2, 64, 8)),
                                  ("g2", (self.nT, nK2, 64, 8)), ("g3", (self.nOT, nK2, 64, 8))])

    def pack_index_bf16(self) -> np.ndarray:
        """int32 gather map of the bf16 fragment image: ``image[i] = bf16(flat[idx[i]]) if idx[i] >= 0 else 0``."""
        *_, layout = self._bf16_parts()
        idx = np.full(layout.total * self.n_transforms, -1, dtype=np.int32)
        for t, c in enumerate(self.connections()):
            _fill(idx, t * layout.total, layout, {"g" + k: _frag_a32(c["W" + k]) for k in "0123"})
        return idx

    # ------------------------------------------- bf16 training image (wide flows)
    def wide_layout(self):
        """Sizes of the row-major bf16 weight image of ``csrc/maf_train_bf16.hip`` (elements per transform):
        ``W0f [HK][DK]  W0b = W0f^T  W1f [HK][HK]  W1b  W2f  W2b  W3f [OK][HK]  W3b`` and of its float32 bias image
        ``b0 b1 b2 [HK]  b3 [OK]``; hidden units in slot order, features in canonical order, ``OK = n_out DK`` and W3 rows
        ``n_out feature + s`` (the canonical order: shift, raw for the affine map; widths, heights, derivatives for a spline)."""
        DK, HK, OK, weights, biases = self._wide_parts()
        return dict(DK=DK, HK=HK, OK=OK, per_transform=weights.total, bias_per_transform=biases.total)

    def _wide_parts(self):
        DK, HK = _ceil_to(self.n_dim, 32), _ceil_to(self.Hp, 32)
        OK = self.n_out * DK
        shapes = {"W0": (HK, DK), "W1": (HK, HK), "W2": (HK, HK), "W3": (OK, HK)}
        weights = _layout([(k + d, s if d == "f" else s[::-1]) for k, s in shapes.items() for d in "fb"])
        return DK, HK, OK, weights, _layout([("b0", (HK,)), ("b1", (HK,)), ("b2", (HK,)), ("b3", (OK,))])

    def wide_index(self):
        """``(image_idx, bias_idx)`` int32: canonical index of every element of the two images, -1 where masked or
        padded.  ``image[i] = bf16(flat[idx[i]])``; the ``W?f`` parts double as the scatter map of the weight gradients."""
        *_, weights, biases = self._wide_parts()
        img = np.full(self.n_transforms * weights.total, -1, dtype=np.int32)
        bias = np.full(self.n_transforms * biases.total, -1, dtype=np.int32)
        for t, c in enumerate(self.connections(by_rank=False, tile=32)):     # (slots and features padded to the 32-wide k tiles)
            _fill(img, t * weights.total, weights, {k + d: c[k] if d == "f" else c[k].T
                                                 for k in ("W0", "W1", "W2", "W3") for d in "fb"})
            _fill(bias, t * biases.total, biases, {k: c[k] for k in biases.shapes})
        return img, bias

    # ------------------------------------------------------------- training
    def train_layout(self):
        """Sizes of the training-side device arrays, per transform.

        ``packedT`` (float): transposed weight fragments for the data-gradient products
        ``dh = W^T da``:  f0T [nXT][nT], f1T/f2T [nT][nT], f3T [nT][nOT], each ``[..][..][lane][4]``
        with ``A[i][k] = W[out 16*To + 4c + k][in 16*Ti + i]``.
        ``gmap`` (int32): canonical index of every element of a weight-gradient tile in MFMA C
        layout (lane (q, j) reg r <-> W[out 16*To + 4q + r][in 16*Ti + j]), -1 = masked / padding:
        g0 [nT][nXT], g1/g2 [nT][nT], g3 [nOT][nT], then the bias maps b0,b1,b2 [Hp], b3 [Op].
        """
        (_, szT, offT, pkT), (_, szG, offG, gmap) = self._train_parts()
        return dict(szT=szT, offT=offT, pkT_per_transform=pkT, szG=szG, offG=offG, gmap_per_transform=gmap)

    def _train_parts(self):
        nT, nXT, nOT = self.nT, self.nXT, self.nOT
        return (_layout([("f0T", (nXT, nT, 64, 4)), ("f1T", (nT, nT, 64, 4)), ("f2T", (nT, nT, 64, 4)),
                         ("f3T", (nT, nOT, 64, 4))]),
                _layout([("g0", (nT, nXT, 64, 4)), ("g1", (nT, nT, 64, 4)), ("g2", (nT, nT, 64, 4)), ("g3", (nOT, nT, 64, 4)),
                         ("gb0", (self.Hp,)), ("gb1", (self.Hp,)), ("gb2", (self.Hp,)), ("gb3", (self.Op,))]))

    def par_per_transform(self) -> int:
        """Floats of the hyper-network's outputs kept per row set and transform (``pmc_maf_train_t.par_scratch``):
        ``nOT`` tiles for the affine flows, ``nXT`` panels of ``n_out`` (= 3 bins - 1) tiles for the spline flows."""
        return 256 * (self.nXT * self.n_out if self.univariate == "rqs" else self.nOT)

    def train_tables(self, n_waves: int = 16) -> np.ndarray:
        """``int32`` tables of the chain kernel (``pmc_maf_train_t.tables``):

        ``[16][8]`` ownership of the hidden tiles of the triangular layers: row ``w`` lists the COST RANKS (0 = the
        tile with the longest contraction: ``nT - r`` K tiles when the degree groups fit a tile) wave ``w`` of the
        ``n_waves`` takes, most expensive first, -1 ends the row.  The four SIMDs of a compute unit each run
        ``n_waves / 4`` of the waves (wave ``w`` on SIMD ``w % 4``) and a layer is bound by its busiest f32 matrix pipe,
        so tiles go to the least-loaded SIMD first and to its least-loaded wave (longest processing time first).
        ``[T][D]`` the rank in transform ``t + 1`` of the feature at rank ``r`` of transform ``t`` (last row unused);
        ``[T][D]`` likewise for ``t - 1`` (first row unused)."""
        nT, D, T = self.nT, self.n_dim, self.n_transforms
        own = np.full((16, 8), -1, dtype=np.int64)
        if nT <= 8 * n_waves:
            simd_load = np.zeros(4)
            wave_load = np.zeros(n_waves)
            wave_cnt = np.zeros(n_waves, dtype=np.int64)
            for r in range(nT):
                cost = (nT - r) if self.tri_ok else nT
                live = [sd for sd in range(min(4, n_waves)) if any(wave_cnt[w] < 8 for w in range(sd, n_waves, 4))]
                sd = min(live, key=lambda k: (simd_load[k], k))
                w = min((w for w in range(sd, n_waves, 4) if wave_cnt[w] < 8), key=lambda k: (wave_load[k], k))
                own[w, wave_cnt[w]] = r
                wave_cnt[w] += 1
                wave_load[w] += cost
                simd_load[sd] += cost
        else:
            raise NotImplementedError("more than 8 hidden tiles per wave of the training workgroup")
        f_o_r = [np.argsort(o) for o in self.orders]
        nxt = np.zeros((T, D), dtype=np.int64)
        prv = np.zeros((T, D), dtype=np.int64)
        for t in range(T):
            if t + 1 < T:
                nxt[t] = np.asarray(self.orders[t + 1])[f_o_r[t]]
            if t > 0:
                prv[t] = np.asarray(self.orders[t - 1])[f_o_r[t]]
        return np.concatenate([own.reshape(-1), nxt.reshape(-1), prv.reshape(-1)]).astype(np.int32)

    def train_jobs(self) -> np.ndarray:
        """``int32 [n_jobs][8]``: the weight-gradient tiles of one minibatch, one workgroup of ``maf_dw_kernel`` each.

        ``{kind_a, off_a, kind_b, off_b, g_w, g_b, 0, 0}``: the tile ``dW[out tile][in tile] = sum over the batch's rows
        of delta[out] x activation[in]`` takes its A operand (delta, 16 x rows) from scratch array ``kind_a`` at float
        offset ``off_a`` inside a row set's block and its B operand (activation) likewise; ``g_w`` is the offset of
        the tile's 256 entries in ``gmap`` (or -1: bias only), ``g_b`` the offset of the 16 bias entries of the out
        tile (carried by ONE job per out tile, -1 elsewhere).  Kinds: 0 ``xt_scratch`` (transform inputs), 1
        ``act_scratch`` (h0, h1, h2), 2 ``delta_scratch`` (da0, da1, da2), 3 ``par_scratch`` (output gradients).
        Only tiles with at least one unmasked entry get a job.

        Order: workgroup ``b`` of a launch runs on XCD ``b % 8`` (observed on MI355X, used for speed only), and the eight
        L2s are not shared.  Jobs that read the same operand tiles -- the tiles of one layer of one transform -- are
        therefore placed in the same residue class mod 8 (pieces of a layer's job list, longest first onto the least
        loaded class), so that an operand crosses the fabric into ONE L2 instead of eight; classes are padded to equal
        length with no-op jobs (``kind_a = -1``)."""
        L = self.train_layout()
        _, gm = self.train_index()
        nT, nXT, nOT, Hp, Dp = self.nT, self.nXT, self.nOT, self.Hp, self.Dp
        G = L["gmap_per_transform"]
        ppt = self.par_per_transform()
        jobs, groups, g_start = [], [], 0
        for t in range(self.n_transforms):
            gt = t * G
            layers = (
                # (gmap weights, [out tiles][in tiles], gmap bias, A kind / base, B kind / base)
                ("g0", nT, nXT, "gb0", 2, (t * 3 + 0) * Hp * 16, 0, t * Dp * 16),
                ("g1", nT, nT, "gb1", 2, (t * 3 + 1) * Hp * 16, 1, (t * 3 + 0) * Hp * 16),
                ("g2", nT, nT, "gb2", 2, (t * 3 + 2) * Hp * 16, 1, (t * 3 + 1) * Hp * 16),
                ("g3", nOT, nT, "gb3", 3, t * ppt, 1, (t * 3 + 2) * Hp * 16),
            )
            for gname, n_out_t, n_in_t, bname, ka, base_a, kb, base_b in layers:
                gw0, gb0 = gt + L["offG"][gname], gt + L["offG"][bname]
                n_bias = L["szG"][bname]
                for To in range(n_out_t):
                    bias_live = 16 * To < n_bias and (gm[gb0 + 16 * To: gb0 + min(16 * To + 16, n_bias)] >= 0).any()
                    first = True
                    for Ti in range(n_in_t):
                        off = gw0 + (To * n_in_t + Ti) * 256
                        if not (gm[off: off + 256] >= 0).any():
                            continue
                        jobs.append((ka, base_a + To * 256, kb, base_b + Ti * 256, off,
                                     gb0 + 16 * To if (first and bias_live) else -1, 0, 0))
                        first = False
                    if first and bias_live:                  # an out tile whose weights are all masked still has biases
                        jobs.append((ka, base_a + To * 256, -1, 0, -1, gb0 + 16 * To, 0, 0))
                groups.append(jobs[g_start:])
                g_start = len(jobs)
        # ---- placement by XCD (docstring): pieces of <= piece jobs, longest processing time first
        piece = max(4, -(-len(jobs) // 32))
        pieces = [g[i:i + piece] for g in groups for i in range(0, len(g), piece)]
        buckets = [[] for _ in range(8)]
        for pc in sorted(pieces, key=len, reverse=True):
            min(buckets, key=len).extend(pc)
        buckets.sort(key=len, reverse=True)                  # (block 0, which also adds up the loss, gets a real job)
        depth = len(buckets[0])
        noop = (-1, 0, -1, 0, -1, -1, 0, 0)
        out = [buckets[b][k] if k < len(buckets[b]) else noop for k in range(depth) for b in range(8)]
        while out and out[-1] == noop:
            out.pop()
        return np.asarray(out, dtype=np.int32).reshape(-1, 8)

    def train_index(self):
        """``(packT_idx, gmap)``: gather map for ``packedT`` (like ``pack_index``) and the
        gradient scatter map, both int32, all transforms concatenated.  (Built once per spec: ``train_jobs`` reads it too.)"""
        if getattr(self, "_train_index", None) is None:
            self._train_index = self._build_train_index()
        return self._train_index

    def _build_train_index(self):
        packT, gmap = self._train_parts()
        pT = np.full(packT.total * self.n_transforms, -1, dtype=np.int32)
        gm = np.full(gmap.total * self.n_transforms, -1, dtype=np.int32)
        for t, c in enumerate(self.connections()):
            # transposed fragments: A operands of W^T; gradient scatter: the tiles of W in C layout
            _fill(pT, t * packT.total, packT, {f"f{k}T": _frag_a4(c["W" + k].T) for k in "0123"})
            _fill(gm, t * gmap.total, gmap, {**{"g" + k: _frag_c(c["W" + k]) for k in "0123"},
                                          **{"gb" + k: c["b" + k] for k in "0123"}})
        return pT, gm

    # ------------------------------------------------------------ accounting
    def flops_forward_dense(self) -> int:
        """``F_fwd = T*2*(3*D*H + 2*H*H)`` per particle for the affine flows;
        in general the output layer has ``n_out*D`` rows: ``T*2*((1 + n_out)*D*H + 2*H*H)``."""
        D, H = self.n_dim, self.hidden
        return self.n_transforms * 2 * ((1 + self.n_out) * D * H + 2 * H * H)

    def flops_inverse_naive(self) -> int:
        """``F_inv = (D+1) * F_fwd`` per particle."""
        return (self.n_dim + 1) * self.flops_forward_dense()

    def macs_masked(self) -> int:
        """Unmasked multiply-accumulates per particle (the work that is left
        once the masks are exploited)."""
        n = 0
        for t in range(self.n_transforms):
            n += sum(int(M.sum()) for M in self.masks(t))
        return n


WIDE_MIN_HIDDEN = 256       # hidden width from which the bf16 matrix cores pay: the bf16 trainer (train.py) and the spline flows' bf16 forward


def bf16_forward_refusal(spec: "MAFSpec"):
    """Why ``Flow(..., precision="bf16")`` refuses ``spec``, or None where it accepts it -- the one rule of that switch.
    Affine flows: every width (``csrc/maf_forward_bf16.hip``).  Spline flows: ``hidden >= WIDE_MIN_HIDDEN`` only -- a
    narrower hyper-network has one to four 32-wide k tiles per layer, its call is a chain of barrier-separated layers
    that the matrix cores do not shorten, so such a flow would pay bf16's rounding for nothing."""
    if spec.univariate == "affine" or spec.hidden >= WIDE_MIN_HIDDEN:
        return None
    return (f"precision='bf16' takes spline flows of hidden width >= {WIDE_MIN_HIDDEN} (this one: {spec.hidden}): "
            f"narrower flows gain nothing on the bf16 matrix cores and keep the float32 kernels")


SPEC_BY_NAME = {"maf3": 3, "maf6": 6, "maf12": 12}
NSF_BY_NAME = {"nsf3": 3, "nsf6": 6, "nsf12": 12}          # pocomc/flow.py:69-86


def spec_by_name(n_dim: int, name: str) -> "MAFSpec":
    """The six predefined flows of ``pocomc/flow.py:54-86``."""
    if name in SPEC_BY_NAME:
        return MAFSpec(n_dim, SPEC_BY_NAME[name])
    if name in NSF_BY_NAME:
        return MAFSpec(n_dim, NSF_BY_NAME[name], univariate="rqs", bins=8)
    raise KeyError(name)
