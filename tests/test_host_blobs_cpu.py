"""``mcmc.host_blobs`` / ``mcmc.host_blobs_dtype``: what a vectorised host likelihood that returns ``(logl, blobs)`` may hand
back, checked and cast on the host (pure numpy, no GPU) -- accepted dtypes and shapes, and the messages of what is refused."""
import numpy as np
import pytest


def test_accepted_dtypes():
    from pocomc_amd.mcmc import HOST_BLOB_DTYPES, host_blobs_dtype
    assert host_blobs_dtype(float) == np.float64 and host_blobs_dtype(int) == np.int64
    assert host_blobs_dtype("float32") == np.float32 and host_blobs_dtype(np.int32) == np.int32
    assert set(HOST_BLOB_DTYPES) == {np.dtype(t) for t in (np.float64, np.float32, np.int64, np.int32)}
    for dt in (object, bool, np.float16, np.int16, np.uint32, np.complex128, "U4", np.dtype([("a", "f8"), ("b", "i4")])):
        with pytest.raises(ValueError, match="float64, float32, int64 or int32.*vectorize=False"):
            host_blobs_dtype(dt)
    with pytest.raises(ValueError, match="no numpy dtype"):
        host_blobs_dtype("not a dtype")


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int64, np.int32])
@pytest.mark.parametrize("shape", [(), (1,), (3,), (2, 3)])
def test_blobs_are_cast_and_contiguous(dtype, shape):
    from pocomc_amd.mcmc import host_blobs
    n = 5
    raw = np.arange(n * int(np.prod(shape, dtype=int)), dtype=np.float64).reshape((n,) + shape)
    logl, b = host_blobs((np.zeros(n, dtype=np.float32), raw), n, dtype)
    assert logl.dtype == np.float64 and logl.shape == (n,)
    assert b.dtype == dtype and b.shape == (n,) + shape and b.flags.c_contiguous and np.array_equal(b, raw.astype(dtype))
    logl, b2 = host_blobs((np.zeros(n), raw), n, dtype, blob_shape=shape)
    assert np.array_equal(b, b2)
    # lists and Fortran-ordered arrays are array-likes too; a right array comes back without a copy
    assert np.array_equal(host_blobs((np.zeros(n), raw.tolist()), n, dtype)[1], b)
    assert host_blobs((np.zeros(n), np.asfortranarray(raw)), n, dtype)[1].flags.c_contiguous
    assert host_blobs((np.zeros(n), b), n, dtype)[1] is b


def test_what_is_refused():
    from pocomc_amd.mcmc import PMC_BLOB_ROW_BYTES_MAX, host_blobs
    n = 4
    ll, ok = np.zeros(n), np.zeros((n, 3))
    assert PMC_BLOB_ROW_BYTES_MAX == 1 << 20
    for out, kw, word in ((ll, {}, r"tuple \(logl, blobs\), got ndarray"), ((ll, ok, ok), {}, "a tuple of 3"),
                          ([ll, ok], {}, r"tuple \(logl, blobs\), got list"), ((ll, None), {}, "got None"),
                          ((np.zeros(n - 1), ok), {}, r"logl of shape \(4,\), got \(3,\)"),
                          ((np.zeros((n, 1)), ok), {}, r"logl of shape \(4,\), got \(4, 1\)"),
                          ((ll, ok[:-1]), {}, r"shape \(4, ...\), got \(3, 3\)"),
                          ((ll, 1.0), {}, r"shape \(4, ...\), got \(\)"),
                          ((ll, np.zeros((n, 0))), {}, "at least one element"),
                          ((ll, [[1.0], [1.0, 2.0], [1.0], [1.0]]), {}, "do not form"),
                          ((ll, np.array([["a"]] * n)), {}, "do not form"),
                          ((ll, np.zeros((n, 2))), dict(blob_shape=(3,)), r"blob_shape \(3,\) as in the first call, got \(2,\)"),
                          ((ll, np.zeros(n)), dict(blob_shape=(1,)), r"blob_shape \(1,\) as in the first call, got \(\)"),
                          ((ll, np.zeros((n, PMC_BLOB_ROW_BYTES_MAX // 8 + 1))), {}, "1048584 bytes is more than PMC_BLOB_ROW_BYTES_MAX")):
        with pytest.raises(ValueError, match=word):
            host_blobs(out, n, np.float64, **kw)
    with pytest.raises(ValueError, match="float64, float32, int64 or int32"):
        host_blobs((ll, ok), n, np.float16)
    # exactly the limit is a row the device takes
    assert host_blobs((ll, np.zeros((n, PMC_BLOB_ROW_BYTES_MAX // 4), dtype=np.int32)), n, np.int32)[1].shape[1] == 1 << 18
