"""The host model of the Philox generator (``tests/philox_model.py``) is judged here, before any kernel is held to it
(``tests/test_gpu_philox_model.py``): the cipher against Random123's known answers, the counter layout by unpacking
it, the uniform conversion at the extreme words, the float64 twin of the normals against the longdouble yardstick
(this is where the GPU bound comes from), the gamma rows' decision margins on every case the GPU test uses, and the
laws of the model's own variates.  ``-s`` prints the measured figures."""
import numpy as np
import pytest
from scipy import stats

import philox_model as pm

P_MIN = 1e-3          # tests/test_gpu_rng.py


def test_longdouble_has_a_64_bit_mantissa():
    """The yardstick needs three decades below float64 (x87 extended precision); its pi is pi to that precision."""
    assert np.finfo(np.longdouble).eps < 2e-19
    assert abs(pm.PI_LD - 4 * np.arctan(np.longdouble(1))) <= 2 * np.spacing(pm.PI_LD)
    assert float(pm.PI_LD) == np.pi


# ------------------------------------------------------------------------------------------------------------ cipher
@pytest.mark.parametrize("ctr, key, out", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_known_answers_of_philox4x32_10(ctr, key, out):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    w = lambda s: [int(x, 16) for x in s.split()]
    assert [int(x) for x in pm.philox4x32_10(w(ctr), w(key))] == w(out)


def test_the_cipher_is_vectorised_over_counters_and_keys():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(5, 3, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(3, 2), dtype=np.uint64)
    out = pm.philox4x32_10(ctr, key)
    assert out.shape == (5, 3, 4) and out.max() < 2 ** 32
    for i in range(5):
        for j in range(3):
            assert np.array_equal(out[i, j], pm.philox4x32_10(ctr[i, j], key[j]))
    # a bijection of the counter for a fixed key: neighbouring counters differ in about half of the 128 bits
    a, b = pm.philox4x32_10([7, 0, 0, 0], [1, 2]), pm.philox4x32_10([8, 0, 0, 0], [1, 2])
    assert 32 < sum(bin(int(x ^ y)).count("1") for x, y in zip(a, b)) < 96


# ----------------------------------------------------------------------------------------------------------- counter
def test_key_split_uses_both_words_of_the_seed():
    assert pm.key_split(2 ** 64 - 1).tolist() == [2 ** 32 - 1, 2 ** 32 - 1]
    assert pm.key_split(2 ** 32).tolist() == [0, 1]
    assert pm.key_split(0x9E3779B97F4A7C15).tolist() == [0x7F4A7C15, 0x9E3779B9]
    assert pm.key_split(2 ** 62 - 1).tolist() == [2 ** 32 - 1, 2 ** 30 - 1]        # the largest seed mcmc.py draws


def test_counter_layout_word_by_word():
    ctr, key = pm.counter(seed=5, step=9, particle=(3 << 32) | 11, stream=4, draw=6)
    assert ctr.tolist() == [6, 11, 3 ^ (4 << 24), 9] and key.tolist() == [5, 0]
    # the step fold: low word xor (high word * 0x9E3779B9 mod 2^32) -- the product first, then the xor
    ctr, _ = pm.counter(0, (5 << 32) | 0x1234, 0, 0, 0)
    assert int(ctr[3]) == 0x1234 ^ ((5 * 0x9E3779B9) & 0xFFFFFFFF)
    assert int(pm.counter(0, 2 ** 40 + 3, 0, 0, 0)[0][3]) == 3 ^ ((256 * 0x9E3779B9) & 0xFFFFFFFF)


def test_counter_map_is_injective_inside_its_box():
    """``step < 2^32``, ``particle < 2^56``, stream 0..4, ``draw < 2^32``: unpacking the four words returns the
    arguments, at the box's corners and at random points of it."""
    rng = np.random.default_rng(1)
    edge = lambda hi: np.concatenate([pm.u64([0, 1, hi - 1]), rng.integers(0, hi, size=37, dtype=np.uint64)])
    step, particle, draw = edge(2 ** 32), edge(2 ** 56), edge(2 ** 32)
    particle[3:6] = [2 ** 32 - 1, 2 ** 32, 2 ** 40]
    assert int(particle[2]) == 2 ** 56 - 1
    for stream in pm.STREAMS.values():
        s, p, d = np.meshgrid(step, particle, draw, indexing="ij")
        ctr, _ = pm.counter(0, s, p, stream, d)
        assert ctr.max() < 2 ** 32
        us, up, ust, ud = pm.unpack_counter(ctr)
        assert np.array_equal(us, s) and np.array_equal(up, p) and np.array_equal(ud, d) and (ust == stream).all()
    # the seed lives in the key alone, the other four in the counter alone
    assert np.array_equal(pm.counter(1, 2, 3, 4, 5)[0], pm.counter(99, 2, 3, 4, 5)[0])
    assert np.array_equal(pm.counter(1, 2, 3, 4, 5)[1], pm.counter(1, 7, 8, 0, 9)[1])


def test_what_collides_outside_the_box():
    """Documentation of the layout's limits, not a defect: a population has far fewer than 2^56 walkers and a run far
    fewer than 2^32 steps."""
    # the stream number sits in bits 24.. of ctr[2], where particle >> 32 reaches from 2^56 on
    a, _ = pm.counter(0, 0, 1 << 56, pm.STREAMS["gamma"], 0)
    b, _ = pm.counter(0, 0, 0, pm.STREAMS["normal"], 0)
    assert np.array_equal(a, b)
    # the step fold maps 64 bits to 32: (2^32) folds to 0x9E3779B9, which is also a step below 2^32
    a, _ = pm.counter(0, 1 << 32, 0, 0, 0)
    b, _ = pm.counter(0, 0x9E3779B9, 0, 0, 0)
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------- uniforms
def test_uniform_conversion_at_the_extreme_words():
    top = 2 ** 64 - 1
    assert pm.uniform_from_word(0) == 2.0 ** -54                      # the smallest value; the word's low 11 bits are dropped
    assert pm.uniform_from_word(2 ** 11 - 1) == 2.0 ** -54
    assert pm.uniform_from_word(2 ** 11) == 3 * 2.0 ** -54
    assert pm.uniform_from_word(top) == 1.0                           # 2^53 - 1 + 0.5 rounds to even: exactly one
    assert pm.uniform_from_word(top - 2 ** 11) == 1.0 - 2.0 ** -52    # k = 2^53 - 2 is even and keeps its value
    assert pm.uniform_from_word((2 ** 52 + 1) << 11) == (2 ** 52 + 2) * 2.0 ** -53   # first tie: odd k moves up
    assert pm.uniform_from_word((2 ** 52 - 1) << 11) == (2 ** 52 - 0.5) * 2.0 ** -53  # last representable k + 0.5
    x = np.sort(np.concatenate([np.random.default_rng(2).integers(0, 2 ** 64, size=20000, dtype=np.uint64),
                                np.array([0, top, 2 ** 63, 2 ** 63 - 1, 2 ** 63 + 2 ** 11], dtype=np.uint64)]))
    u = pm.uniform_from_word(x)
    assert (np.diff(u) >= 0).all() and u.min() >= 2.0 ** -54 and u.max() <= 1.0       # monotone, inside [2^-54, 1]
    # the word order of a call: (w0 << 32 | w1, w2 << 32 | w3)
    a, b = pm.uniform2([0x80000000, 0, 0, 1 << 11])
    assert a == 0.5 and b == 3 * 2.0 ** -54


# ----------------------------------------------------------------------------------------------------------- normals
def test_quadrant_reduction_is_exact_at_the_axes():
    t = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 0.25, 0.75, 2.0 ** -53, 2.0 - 2.0 ** -52])
    c, s = pm._cospi_sinpi(t, np.float64(np.pi))
    assert c[:5].tolist() == [1, 0, -1, 0, 1] and s[:5].tolist() == [0, 1, 0, -1, 0]
    np.testing.assert_allclose(c[5:7], [0.5 ** 0.5, -0.5 ** 0.5], rtol=2e-16)
    np.testing.assert_allclose(s[7:], [np.pi * 2.0 ** -53, -np.pi * 2.0 ** -52], rtol=2e-16)   # relative, next to a zero


def test_float64_twin_against_the_yardstick():
    """The twin's largest error on the draws the GPU test uses, in ulps of the value: the GPU bound is 4 times it.
    A sound pair of host libraries keeps Box-Muller (log, sqrt, one multiple of pi, sin / cos, one product) within a
    few ulps; a yardstick that lost digits next to the zeros of sin and cos would show here as thousands."""
    e = pm.twin_error()
    print(f"\ntwin vs yardstick, ulps of the value: normals {e.normal:.3f}, pow {e.pow:.3f}; GPU bound {pm.bound_ulps():.3f}")
    assert 0.4 < e.normal < 8.0 and e.pow < 4.0
    assert pm.bound_ulps() == 4.0 * max(e.normal, e.pow, 1.0)
    # the edge seeds' draws and the fit noise do not stretch it: the same functions on other arguments
    worst = 0.0
    for seed in pm.EDGE_SEEDS:
        f = pm.fill_case(seed, pm.EDGE_STEPS[-1], pm.EDGE_OFFSETS[1], pm.EDGE_N, pm.EDGE_D)
        worst = max(worst, float(pm.ulps(f.normal, f.normal_yard).max()))
    tw, yd = pm.noise_case(max(pm.NOISE_N), max(pm.NOISE_D))
    worst = max(worst, float(pm.ulps(tw, yd).max()))
    print(f"twin on the edge seeds and the fit noise: {worst:.3f}")
    assert worst <= pm.bound_ulps() / 2
    # every pair returns its first uniform: exp(-(a^2 + b^2) / 2) = u1
    f = pm.fill_case(pm.SEED, pm.STEP, 0, max(pm.FILL_N), 32)
    r2 = f.normal[:, 0::2] ** 2 + f.normal[:, 1::2] ** 2
    np.testing.assert_allclose(np.exp(-0.5 * r2), f.u1, rtol=1e-12)


def test_fit_noise_rounds_to_float32_unambiguously():
    """No element of the GPU test's fit-noise cases lies within the normal bound of a float32 rounding boundary: the
    float32 comparison there leaves out nothing."""
    for n, D in [(max(pm.NOISE_N), D) for D in pm.NOISE_D] + [pm.NOISE_LARGE]:
        _, yd = pm.noise_case(n, D)
        _, decided = pm.float32_of(yd, pm.bound_ulps())
        assert decided.all(), (n, D, int((~decided).sum()))
    for D in (3, 33):                  # test_fit_noise_arithmetic_shards_and_passes: other passes, seed and rows
        for p in (pm.NOISE_PASS + 1, 2 ** 32 + 1):
            assert pm.float32_of(pm.noise_case(300, D, pass_=p)[1], pm.bound_ulps())[1].all()
        assert pm.float32_of(pm.noise_case(300, D, seed=2 ** 62 - 1)[1], pm.bound_ulps())[1].all()
        _, yd = pm.fit_noise(pm.NOISE_SEED, pm.NOISE_PASS, 2 ** 32 - 8, 64, D)
        assert pm.float32_of(yd, pm.bound_ulps())[1].all()


# ------------------------------------------------------------------------------------------------------------- gamma
def test_gamma_margins_of_every_case_the_gpu_test_uses():
    """No row is left out: every accept decision the model takes is farther than 2^-40 (relative to its terms) from
    going the other way -- three decades above what a few ulps in ``log`` can move."""
    print()
    for shape in pm.GAMMA_SHAPES:
        g = pm.gamma_case(shape, n=pm.GAMMA_N)
        print(f"shape {shape:g}: smallest margin {g.margin.min():.2e}, candidates {np.bincount(g.candidate).tolist()}, "
              f"largest value factor {g.factor.max():.1f}")
        assert (g.margin >= pm.MARGIN_MIN).all(), shape
        assert (g.candidate >= 0).all() and np.isfinite(g.value).all() and (g.value > 0).all()
        # the twin's value against the yardstick's, inside its own row bound
        assert (pm.ulps(g.value, g.yard) <= g.factor * pm.bound_ulps()).all()
    for shape in (0.5, 1.05):
        # the draw bookkeeping past the first round trip (draws 2.. / 3.. with the boost) is exercised
        c = pm.gamma_case(shape, n=pm.GAMMA_N).candidate
        assert (c == 1).any() and (c >= 2).any(), (shape, np.bincount(c))
    worst = np.inf
    for seed in pm.EDGE_SEEDS:
        for step in pm.EDGE_STEPS:
            for offset in pm.EDGE_OFFSETS:
                for shape in pm.EDGE_SHAPES:
                    worst = min(worst, pm.gamma_case(shape, seed, step, offset, pm.EDGE_N).margin.min())
    print(f"edge seeds / steps / offsets: smallest margin {worst:.2e}")
    assert worst >= pm.MARGIN_MIN
    g = pm.fill_case(pm.SEED, pm.STEP, 0, max(pm.FILL_N), 2, pm.FILL_SHAPE).gamma
    assert (g.margin >= pm.MARGIN_MIN).all()


def test_gamma_margins_at_the_size_of_the_law_test():
    """``test_gamma_draws_follow_the_gamma_law``'s 200 000 walkers: the large shape is the tight one (the cancellation
    in ``d - d v + d log v``), and still three times above 2^-40."""
    g = pm.gamma_case(500016.0, n=200_000)
    print(f"\nshape 500016, 200 000 walkers: smallest margin {g.margin.min():.2e}")
    assert 2.5e-12 < g.margin.min() < 3.5e-12
    assert (g.candidate == 0).all()


def test_gamma_draw_order():
    """The candidates of a row, spelled out from single draws: with the boost, draw 0 is its uniform and round trip
    ``i`` takes draws ``1 + 2 i`` (normals) and ``2 + 2 i`` (uniforms)."""
    for shape, boost in ((0.5, 1), (1.05, 0)):
        g = pm.gamma_case(shape, n=pm.GAMMA_N)
        row = int(np.nonzero(g.candidate >= 2)[0][0])
        it, k = divmod(int(g.candidate[row]), 2)
        x = pm.normal2(*pm.uniform2(pm.words(pm.SEED, pm.STEP, row, 0, boost + 2 * it)))[k]
        d = shape + boost - 1.0 / 3.0
        v = (1.0 + x / np.sqrt(9.0 * d)) ** 3
        b = pm.uniform2(pm.words(pm.SEED, pm.STEP, row, 0, 0))[0] ** (1.0 / shape) if boost else 1.0
        np.testing.assert_allclose(g.value[row], b * d * v, rtol=1e-13)


# -------------------------------------------------------------------------------------------------- composed models
def test_composed_models_are_keyed_by_the_global_index():
    a = pm.fill_case(pm.SEED, pm.STEP, 0, 257, 5, 18.5)
    b = pm.rng_fill(pm.SEED, pm.STEP, 100, 50, 5, 18.5)
    assert np.array_equal(b.normal, a.normal[100:150]) and np.array_equal(b.uniform, a.uniform[100:150])
    assert np.array_equal(b.gamma.value, a.gamma.value[100:150])
    assert a.normal.shape == (257, 5) and a.u1.shape == (257, 3)
    # an odd D drops the last pair's second normal and nothing else
    assert np.array_equal(a.normal[:, :4], pm.fill_case(pm.SEED, pm.STEP, 0, 257, 32, 0.0).normal[:, :4])
    tw, _ = pm.fit_noise(pm.NOISE_SEED, pm.NOISE_PASS, 40, 10, 3)
    assert np.array_equal(tw, pm.noise_case(300, 3)[0][40:50])
    assert not np.array_equal(tw, pm.fit_noise(pm.NOISE_SEED, pm.NOISE_PASS + 1, 40, 10, 3)[0])


def test_bootstrap_indices_layout():
    idx = pm.bootstrap_indices(12345, 4, 7)
    assert idx.shape == (4, 7) and idx.min() >= 0 and idx.max() <= 6
    u0, u1 = pm.uniform2(pm.words(12345, 2, 1, 3, 0))               # replicate 2, elements 2 and 3
    assert idx[2, 2] == int(u0 * 7) and idx[2, 3] == int(u1 * 7)
    u0, _ = pm.uniform2(pm.words(12345, 3, 3, 3, 0))                # the odd tail: element 6 alone
    assert idx[3, 6] == int(u0 * 7)
    assert np.array_equal(pm.bootstrap_indices(12345, 4, 1), np.zeros((4, 1), np.int64))
    big = pm.bootstrap_indices(2 ** 40 + 5, 8, 1025)
    assert abs(big.mean() - 512) < 5 * 1025 / np.sqrt(12 * big.size) and len(np.unique(big)) > 1000


# ------------------------------------------------------------------------------------------- the model's own law
def test_the_models_variates_follow_their_laws():
    """A model that matched a wrong kernel would show here: KS of its uniforms, normals and gammas at 2e4 draws."""
    n = 20_000
    f = pm.rng_fill(seed=99, step=0, offset=0, n=n, D=2)
    assert stats.kstest(f.uniform, "uniform").pvalue > P_MIN
    assert stats.kstest(f.normal.ravel(), "norm").pvalue > P_MIN
    assert stats.kstest(f.normal[:, 0], "norm").pvalue > P_MIN and stats.kstest(f.normal[:, 1], "norm").pvalue > P_MIN
    assert abs(np.corrcoef(f.normal.T)[0, 1]) < 5 / np.sqrt(n)
    for shape in pm.GAMMA_SHAPES:
        g = pm.gamma_case(shape, seed=7, step=11, offset=12345, n=n)
        assert stats.kstest(g.value, stats.gamma(a=shape).cdf).pvalue > P_MIN, shape
    idx = pm.bootstrap_indices(5, 40, 500)
    assert stats.chisquare(np.bincount(idx.ravel(), minlength=500)).pvalue > P_MIN
