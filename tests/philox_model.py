"""A host model of ``csrc/philox.h`` and of the kernels that draw from it, in plain numpy.

The suite pins the generator's *laws* (``tests/test_gpu_rng.py``) and the equality of the inline draws with
``pmc_rng_fill`` (``test_proposal_in_every_width_class``, ``test_fused_proposal_and_inverse_equal_the_two_launches``,
``test_variates_drawn_ahead_equal_inline_draws``).  This module says which *values* a (seed, step, particle, stream,
draw) has to produce, so that one comparison of ``pmc_rng_fill`` with it pins every kernel that draws:

* the cipher is Philox4x32-10 of Salmon et al. (2011), checked against Random123's known answers;
* the counter layout is the table in :func:`counter`;
* integer words, the uniform conversion, the bootstrap indices and the float32 noise arithmetic are exact here and are
  compared bit for bit; the normals and the gamma value go through ``log``, ``sqrt``, ``sincospi`` and ``pow`` and are
  compared with an ``np.longdouble`` yardstick within a bound that comes from the float64 twin's own error
  (:func:`bound_ulps`), never from the device.

``tests/test_philox_model_cpu.py`` judges the model; ``tests/test_gpu_philox_model.py`` holds the kernels to it.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
MUL0, MUL1 = U64(0xD2511F53), U64(0xCD9E8D57)          # multiplies ctr[0] / ctr[2]
WEYL0, WEYL1 = U64(0x9E3779B9), U64(0xBB67AE85)        # key bumps: golden ratio, sqrt(3) - 1
STEP_FOLD = U64(0x9E3779B9)
STREAMS = {"gamma": 0, "normal": 1, "accept": 2, "bootstrap": 3, "fit_noise": 4}


def u64(x):
    """Anything integral (Python ints up to 2^64 - 1 included) as a uint64 array."""
    return np.asarray(x, dtype=U64)


# ------------------------------------------------------------------------------------------------------------ cipher
def philox4x32_10(ctr, key):
    """Philox4x32-10.  ``ctr``: (..., 4), ``key``: (..., 2), 32-bit words held in uint64; returns (..., 4) likewise.

    One round: the two 32x32 -> 64 bit products ``MUL0 * c0`` and ``MUL1 * c2`` are split into high and low words;
    the new counter is ``(hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)``; the key then moves on by the Weyl constants."""
    ctr, key = u64(ctr), u64(key)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = np.broadcast_to(ctr & M32, shape + (4,))
    k = np.broadcast_to(key & M32, shape + (2,))
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = MUL0 * c0, MUL1 * c2                   # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + WEYL0) & M32, (k1 + WEYL1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def key_split(seed):
    """``key[0]`` = low word of the 64-bit seed, ``key[1]`` = high word."""
    seed = u64(seed)
    return np.stack([seed & M32, seed >> U64(32)], axis=-1)


def counter(seed, step, particle, stream, draw):
    """Key and counter of one Philox call: ``(ctr (..., 4), key (..., 2))``; the arguments broadcast.

    ====== ==================================================================================================
    word   holds
    ====== ==================================================================================================
    key[0] ``seed & 0xffffffff``
    key[1] ``seed >> 32``
    ctr[0] ``draw``: the n-th Philox call of this (step, particle, stream); every call yields four words, i.e.
           two uniforms or one Box-Muller pair
    ctr[1] ``particle & 0xffffffff`` (the GLOBAL walker / row index; bootstrap: the pair of draws ``e >> 1``)
    ctr[2] ``(particle >> 32) ^ (stream << 24)``
    ctr[3] ``(step & 0xffffffff) ^ ((step >> 32) * 0x9E3779B9 mod 2^32)`` (the step of the run; bootstrap: the
           replicate; fit noise: the pass over the data)
    ====== ==================================================================================================

    Streams: 0 the gamma scale of the proposal, 1 its normal noise (draw = coordinate pair), 2 the accept uniform,
    3 the bootstrap of the evidence error, 4 the noise augmentation of ``Flow.fit`` (draw = coordinate pair).

    The map is injective on ``step < 2^32``, ``particle < 2^56``, ``stream < 256``, ``draw < 2^32``
    (:func:`unpack_counter` inverts it there).  Outside that box it collides: from ``particle = 2^56`` on the bits of
    ``particle >> 32`` meet the stream number, and the step fold maps 64 bits to 32."""
    seed, step, particle, stream, draw = np.broadcast_arrays(u64(seed), u64(step), u64(particle), u64(stream), u64(draw))
    sh = U64(32)
    c2 = ((particle >> sh) ^ (stream << U64(24))) & M32
    c3 = (step & M32) ^ (((step >> sh) * STEP_FOLD) & M32)
    return np.stack([draw & M32, particle & M32, c2, c3], axis=-1), key_split(seed)


def unpack_counter(ctr):
    """``(step, particle, stream, draw)`` of a counter built inside the injectivity box of :func:`counter`."""
    ctr = u64(ctr)
    return (ctr[..., 3], ctr[..., 1] | ((ctr[..., 2] & U64(0xFFFFFF)) << U64(32)), ctr[..., 2] >> U64(24), ctr[..., 0])


def words(seed, step, particle, stream, draw):
    return philox4x32_10(*counter(seed, step, particle, stream, draw))


# ---------------------------------------------------------------------------------------------------------- uniforms
def uniform_from_word(x):
    """The header's conversion of one 64-bit word, in its operation order: ``((x >> 11) + 0.5) * 2^-53`` in float64.

    ``k = x >> 11`` has 53 bits and converts exactly.  ``k + 0.5`` is representable only below 2^52; from there on the
    sum rounds to even, so ``k`` and ``k + 1`` (k odd) give the same value and the largest word gives ``2^53``, i.e.
    exactly 1.0.  The result therefore lies in **[2^-54, 1]**, not in (0, 1): below 1/2 it is an odd multiple of 2^-54
    (every ``k`` its own value), from 1/2 on a multiple of 2^-52 reached by two values of ``k``, and 1.0 has probability
    2^-53.  Every consumer tolerates 1.0: ``log(1.0) = 0`` is finite -- it makes a Box-Muller pair (0, 0) and a gamma
    candidate's ``log(uu)`` an ordinary number to compare -- and ``pow(1, .) = 1``; the bootstrap clamps
    ``floor(u n) = n`` to ``n - 1`` (``i >= n``); the accept test ``u < alpha`` with ``alpha <= 1`` merely rejects."""
    k = (u64(x) >> U64(11)).astype(np.float64)
    return (k + 0.5) * 2.0 ** -53


def uniform2(w):
    """Two uniforms from the four words of one call: ``(w0 << 32 | w1, w2 << 32 | w3)``."""
    w = u64(w)
    sh = U64(32)
    return uniform_from_word((w[..., 0] << sh) | w[..., 1]), uniform_from_word((w[..., 2] << sh) | w[..., 3])


# ----------------------------------------------------------------------------------------------------------- normals
# pi to a 64-bit mantissa as the sum of two doubles (the second is pi - float64(pi) to its own precision)
PI_LD = np.longdouble(3.141592653589793) + np.longdouble(1.2246467991473532e-16)


def _cospi_sinpi(t, pi):
    """``cos(pi t), sin(pi t)`` for ``0 <= t <= 2`` in the precision of ``t``: ``t = k/2 + s`` with ``|s| <= 1/4``
    (subtracting a multiple of 1/2 from a binary floating-point number of this size is exact), the functions at
    ``pi s`` and the quadrant's swap and signs.  Without the reduction the error of ``pi t`` next to a zero of sin or
    cos, relative to the value, is unbounded -- in extended precision too."""
    k = np.rint(2 * t)
    s = t - k / 2
    a = pi * s
    ca, sa = np.cos(a), np.sin(a)
    q = k.astype(np.int64) & 3
    return np.choose(q, [ca, -sa, -ca, sa]), np.choose(q, [sa, ca, -sa, -ca])


def normal2(u1, u2, dtype=np.float64):
    """Box-Muller as the header has it: ``r = sqrt(-2 log u1)``, ``(a, b) = r (cos, sin)(2 pi u2)``.

    ``dtype=np.float64``: the twin (numpy's ``log``, ``sqrt``, ``sin``, ``cos``).  ``dtype=np.longdouble``: the
    yardstick (64-bit mantissa)."""
    pi = PI_LD if dtype is np.longdouble else np.float64(np.pi)
    u1, u2 = np.asarray(u1, dtype=dtype), np.asarray(u2, dtype=dtype)
    r = np.sqrt(-2 * np.log(u1))
    c, s = _cospi_sinpi(2 * u2, pi)
    return r * c, r * s


def ulps(got, yard):
    """``|got - yard|`` in units of the float64 spacing at ``yard`` (element-wise; ``yard``: longdouble)."""
    yard = np.asarray(yard, np.longdouble)
    sp = np.spacing(np.abs(yard.astype(np.float64)))
    return (np.abs(np.asarray(got, np.longdouble) - yard) / sp).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------- gamma
MARGIN_MIN = 2.0 ** -40     # a row whose accept decision is closer than this (relative to its terms) is left out
GAMMA_ROUNDINGS = 2.0       # see std_gamma: in units of the bound


def std_gamma(shape, seed, step, particle, stream=STREAMS["gamma"]):
    """Marsaglia & Tsang's standard gamma in the header's draw order, one row per ``particle``.

    Draws of a row's (seed, step, particle, stream): with ``shape < 1`` draw 0 is the boost uniform (first of the
    pair; ``boost = u^(1/shape)``, then ``shape + 1``); after it every round trip takes two draws, one ``normal2`` and
    one ``uniform2``, and looks at two candidates: ``(x_a, u_a)`` then ``(x_b, u_b)``.  A candidate with
    ``t = 1 + c x > 0`` is accepted when ``log u < x^2/2 + d - d v + d log v`` (``v = t^3``), value ``boost d v``.

    Returns a namespace of per-row arrays:

    * ``value``: the float64 twin; ``yard``: the same candidate's value in longdouble arithmetic on the yardstick normal;
    * ``candidate``: number of the accepting candidate, ``2 * round trip + (0 | 1)``;
    * ``margin``: the smallest ``|log u - rhs| / (|x^2/2| + d + |d v| + |d log v| + |log u|)`` over the candidates
      the row looked at (and ``|t| / (1 + |c x|)`` for the sign test of ``t``): how far, relative to its terms, the
      closest decision was from going the other way.  The device's terms differ from the twin's by a few 2^-53 each,
      so a row above ``MARGIN_MIN`` takes the same candidate on any conforming device;
    * ``factor``: the row's value bound in units of :func:`bound_ulps`.  The value is ``boost d (1 + c x)^3``: an
      error ``e`` (relative) of the normal ``x`` becomes ``3 |c x / t| e``; ``pow`` is one more library call and
      the eight rounded operations around it (``1/shape``, ``9 d``, ``sqrt``, ``1/.``, ``c x``, ``1 + .``, two for the
      cube, ``d v``, ``boost .``) add half an ulp each: together at most ``GAMMA_ROUNDINGS`` = 2 bounds, as the bound
      is at least 4 ulps.  ``factor = 3 |c x / t| + 2``.
    """
    particle = np.atleast_1d(u64(particle))
    n = particle.shape[0]
    shape = float(shape)
    draw0 = 0
    boost = np.ones(n)
    boost_ld = np.ones(n, np.longdouble)
    if shape < 1.0:
        u, _ = uniform2(words(seed, step, particle, stream, 0))
        boost = np.power(u, 1.0 / shape)
        boost_ld = np.power(u.astype(np.longdouble), np.longdouble(1.0) / np.longdouble(shape))
        shape += 1.0
        draw0 = 1
    d = shape - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    d_ld = np.longdouble(shape) - np.longdouble(1) / np.longdouble(3)
    c_ld = 1 / np.sqrt(9 * d_ld)
    out = SimpleNamespace(value=np.full(n, np.nan), yard=np.full(n, np.nan, np.longdouble), candidate=np.full(n, -1),
                          margin=np.full(n, np.inf), factor=np.full(n, np.nan))
    open_ = np.arange(n)
    for it in range(256):
        if open_.size == 0:
            break
        p = particle[open_]
        wn, wu = words(seed, step, p, stream, draw0 + 2 * it), words(seed, step, p, stream, draw0 + 2 * it + 1)
        x = normal2(*uniform2(wn))
        x_ld = normal2(*uniform2(wn), dtype=np.longdouble)
        uu = uniform2(wu)
        for k in range(2):
            rows = open_
            xx, lu = x[k], np.log(uu[k])
            t = 1.0 + c * xx
            v = t * t * t
            with np.errstate(invalid="ignore", divide="ignore"):
                terms = [0.5 * xx * xx, d, d * v, d * np.log(v)]
                rhs = terms[0] + terms[1] - terms[2] + terms[3]
                m = np.abs(lu - rhs) / (np.abs(terms[0]) + d + np.abs(terms[2]) + np.abs(terms[3]) + np.abs(lu))
            m = np.where(t > 0.0, m, np.inf)
            out.margin[rows] = np.minimum(out.margin[rows], np.minimum(m, np.abs(t) / (1.0 + np.abs(c * xx))))
            with np.errstate(invalid="ignore"):
                acc = (t > 0.0) & (lu < rhs)
            a = rows[acc]
            out.value[a] = boost[a] * d * v[acc]
            t_ld = 1 + c_ld * x_ld[k][acc]
            out.yard[a] = boost_ld[a] * d_ld * t_ld * t_ld * t_ld
            out.candidate[a] = 2 * it + k
            out.factor[a] = 3.0 * np.abs(c * xx[acc] / t[acc]) + GAMMA_ROUNDINGS
            keep = ~acc
            open_, x, x_ld, uu = rows[keep], (x[0][keep], x[1][keep]), (x_ld[0][keep], x_ld[1][keep]), (uu[0][keep], uu[1][keep])
    assert open_.size == 0, "a row found no candidate in 256 round trips"
    return out


def first_rows(g, n):
    """The first ``n`` rows of a :func:`std_gamma` namespace."""
    return SimpleNamespace(**{k: v[:n] for k, v in vars(g).items()})


# --------------------------------------------------------------------------------------------------- composed models
def normal_rows(seed, step, particle, D, stream):
    """The (n, D) normals of rows ``particle``: pair ``j`` (coordinates ``2j, 2j + 1``) is draw ``j``; an odd ``D``
    drops the last pair's second normal.  Returns ``(twin, yardstick, u1 (n, pairs))``."""
    particle = np.atleast_1d(u64(particle))
    pairs = (D + 1) // 2
    w = words(seed, step, particle[:, None], stream, np.arange(pairs)[None, :])
    u1, u2 = uniform2(w)
    tw = np.stack(normal2(u1, u2), axis=-1).reshape(len(particle), 2 * pairs)[:, :D]
    yd = np.stack(normal2(u1, u2, dtype=np.longdouble), axis=-1).reshape(len(particle), 2 * pairs)[:, :D]
    return tw, yd, u1


def rng_fill(seed, step, offset, n, D, gamma_shape=0.0):
    """What ``pmc_rng_fill`` writes for rows ``offset .. offset + n - 1``: ``normal`` / ``normal_yard`` (n, D), ``u1``
    (n, pairs), ``uniform`` (n), and ``gamma`` (:func:`std_gamma`'s namespace, or None)."""
    particle = (u64(offset) + u64(np.arange(n))).astype(U64)         # wraps like the device's uint64 sum
    tw, yd, u1 = normal_rows(seed, step, particle, D, STREAMS["normal"])
    uni, _ = uniform2(words(seed, step, particle, STREAMS["accept"], 0))
    g = std_gamma(gamma_shape, seed, step, particle) if gamma_shape > 0 else None
    return SimpleNamespace(normal=tw, normal_yard=yd, u1=u1, uniform=uni, gamma=g)


def bootstrap_indices(seed, B, n):
    """The (B, n) indices ``bootstrap_lse_kernel`` draws: replicate ``b`` is the step word, the pair of elements
    ``e, e + 1`` (``e`` even) is particle ``e >> 1``, draw 0 of stream 3 gives the two indices
    ``min(floor(u n), n - 1)``; an odd ``n`` uses only the first of its last pair."""
    pairs = (n + 1) // 2
    u0, u1 = uniform2(words(seed, np.arange(B)[:, None], np.arange(pairs)[None, :], STREAMS["bootstrap"], 0))
    idx = np.stack([u0, u1], axis=-1).reshape(B, 2 * pairs)[:, :n] * float(n)
    return np.minimum(np.floor(idx).astype(np.int64), n - 1)


def fit_noise(seed, pass_, row0, n, D):
    """The noise ``add_noise_kernel`` adds to rows ``row0 .. row0 + n - 1`` before its cast to float32:
    ``(twin, yardstick)``, each (n, D); the pass over the data is the step word."""
    tw, yd, _ = normal_rows(seed, pass_, u64(row0) + u64(np.arange(n)), D, STREAMS["fit_noise"])
    return tw, yd


def float32_of(yard, bound):
    """``(float32(yard), decided)``: the float32 a value rounds to, and whether every number within ``bound`` float64
    ulps of ``yard`` rounds to the same one."""
    yard = np.asarray(yard, np.longdouble)
    h = np.longdouble(bound) * np.spacing(np.abs(yard.astype(np.float64))).astype(np.longdouble)
    lo, hi = (yard - h).astype(np.float32), (yard + h).astype(np.float32)
    return yard.astype(np.float32), lo == hi


# ------------------------------------------------------------------------------- the cases both test files work on
SEED, STEP = 20240928, 3                                     # tests/test_gpu_rng.py's gamma case
FILL_N = (1, 257, 1000)
FILL_D = (1, 2, 5, 32, 157)
FILL_SHAPE = 18.5                                            # the gamma that rides along in the shape cases (bench: D=32, nu=5)
GAMMA_SHAPES = (0.5, 1.05, 1.5, 18.5, 5005.0, 500016.0)
GAMMA_N = 4096               # rows of the gamma cases: enough for a few rows that accept in the second round trip
EDGE_SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 0x9E3779B97F4A7C15, 2 ** 62 - 1, 2 ** 64 - 1)
EDGE_STEPS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3)
EDGE_OFFSETS = (0, 2 ** 32 - 8, 2 ** 40)
EDGE_N, EDGE_D = 64, 4
EDGE_SHAPES = (0.5, 18.5)                                    # with and without the boost draw
NOISE_SEED, NOISE_PASS = 77, 3                               # test_fit_with_noise_augmentation's
NOISE_N = (1, 300, 5000)
NOISE_D = (1, 3, 6, 33)
NOISE_LARGE = (70000, 33)                                    # n * ceil(D/2) > 4096 * 256 (from n = 61681 on at D = 33): 9 MB
BOUND_FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def fill_case(seed, step, offset, n, D, gamma_shape=0.0):
    """:func:`rng_fill`, computed once per case and shared (read-only) by the tests."""
    return rng_fill(seed, step, offset, n, D, gamma_shape)


@functools.lru_cache(maxsize=None)
def gamma_case(shape, seed=SEED, step=STEP, offset=0, n=GAMMA_N):
    return std_gamma(shape, seed, step, (u64(offset) + u64(np.arange(n))).astype(U64))


@functools.lru_cache(maxsize=None)
def noise_case(n, D, seed=NOISE_SEED, pass_=NOISE_PASS):
    return fit_noise(seed, pass_, 0, n, D)


@functools.lru_cache(maxsize=None)
def twin_error():
    """Largest error of the float64 twin against the yardstick, in ulps of the value, over the normals of the largest
    fill case (1000 x 157: every smaller case at the same seed is a subset of its draws) and, for ``pow``, over the
    boost draws of the shapes below one."""
    f = fill_case(SEED, STEP, 0, max(FILL_N), max(FILL_D))
    e_normal = float(ulps(f.normal, f.normal_yard).max())
    u, _ = uniform2(words(SEED, STEP, np.arange(max(FILL_N)), STREAMS["gamma"], 0))
    e_pow = max(float(ulps(np.power(u, 1.0 / s), np.power(u.astype(np.longdouble), 1 / np.longdouble(s))).max())
                for s in GAMMA_SHAPES if s < 1)
    return SimpleNamespace(normal=e_normal, pow=e_pow)


def bound_ulps():
    """The bound a device normal is held to, in ulps of the yardstick's value: ``BOUND_FACTOR`` = 4 times the twin's
    own largest error (normals and ``pow``), and at least 4 ulps.  The host functions are good to about an ulp; a
    conforming device library is allowed a few (OpenCL's double table: 3 for ``log``, 4 for ``sinpi`` / ``cospi``);
    the defects worth catching -- a float32 intermediate, ``sincos(2 pi u)`` for ``sincospi``, a wrong constant --
    are 10^3 times or more outside it.  A gamma value's bound is its row's ``factor`` times this."""
    e = twin_error()
    return BOUND_FACTOR * max(e.normal, e.pow, 1.0)
