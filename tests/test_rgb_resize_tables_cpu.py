"""CPU: the coefficient tables of csrc/rgb_preprocess.hip (svr_rgb_resize_table, host code in double) applied in numpy with
the kernel's integer arithmetic reproduce ``PIL.Image.resize(..., Image.BILINEAR)`` on 8-bit images byte for byte."""
import numpy as np
import pytest
from PIL import Image

PAIRS = [(5, 8), (7, 8), (8, 3), (33, 256), (320, 256), (640, 256), (300, 7), (256, 256)]


def _table(n_in, n_out):
    import __graft_entry__ as ge
    ge.build()
    import svr_amd  # noqa: F401
    from svr_amd import ops
    return ops.rgb_resize_table(n_in, n_out)


def apply_table(a, table, axis):
    """One pass of the 8-bit resampler along `axis` of an (H, W, C) uint8 array: int32 accumulator, 2^21 rounding term,
    arithmetic shift by 22, clamp."""
    a = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((table.shape[0],) + a.shape[1:], dtype=np.int32)
    for xx, row in enumerate(table):
        first, count = int(row[0]), int(row[1])
        acc = np.full(a.shape[1:], 1 << 21, dtype=np.int32)
        for t in range(count):
            acc = acc + a[first + t] * np.int32(row[2 + t])
        out[xx] = acc >> 22
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_table_shape_bounds_and_sum(n_in, n_out):
    t = _table(n_in, n_out)
    K = t.shape[1] - 2
    scale = max(n_in / n_out, 1.0)
    assert t.dtype == np.int32 and t.shape[0] == n_out and K == int(np.ceil(scale)) * 2 + 1
    first, count, taps = t[:, 0], t[:, 1], t[:, 2:]
    assert (first >= 0).all() and (count >= 1).all() and (count <= K).all() and (first + count <= n_in).all()
    assert (taps >= 0).all() and all((taps[i, count[i]:] == 0).all() for i in range(n_out))
    # every row is a partition of 2^22 up to the rounding of its taps (half a unit each)
    assert (np.abs(taps.sum(axis=1).astype(np.int64) - (1 << 22)) <= count).all()
    if n_in == n_out:                                   # the identity: Pillow skips such a pass, the table agrees with that
        assert (first == np.arange(n_out)).all() and (taps[:, 0] == 1 << 22).all() and (taps[:, 1:] == 0).all()


@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("n_in,n_out", PAIRS)
def test_tables_reproduce_pillow_bilinear(n_in, n_out, bands):
    """Square n_in -> n_out (both passes) and a non-square one (n_in columns x 9 rows -> n_out x 9: the horizontal pass
    alone, and transposed: the vertical pass alone)."""
    t = _table(n_in, n_out)
    rng = np.random.default_rng(n_in * 1000 + n_out + bands)

    def pil(a, size):
        img = Image.fromarray(a[:, :, 0] if bands == 1 else a)          # 2-D: mode "L", (H, W, 3): "RGB"
        return np.asarray(img.resize(size, Image.BILINEAR), dtype=np.uint8).reshape(size[1], size[0], bands)

    a = rng.integers(0, 256, (n_in, n_in, bands), dtype=np.uint8)
    got = apply_table(apply_table(a, t, 1), t, 0) if n_in != n_out else a
    assert np.array_equal(got, pil(a, (n_out, n_out)))
    a = rng.integers(0, 256, (9, n_in, bands), dtype=np.uint8)
    assert np.array_equal(apply_table(a, t, 1), pil(a, (n_out, 9)))
    a = np.ascontiguousarray(a.transpose(1, 0, 2))
    assert np.array_equal(apply_table(a, t, 0), pil(a, (9, n_out)))


def test_extremes_survive_the_fixed_point_sum():
    """All-255 and all-0 images: the int32 accumulator neither overflows nor loses the top value at the widest table."""
    t = _table(300, 7)
    for v in (0, 255):
        a = np.full((300, 300, 3), v, dtype=np.uint8)
        assert (apply_table(apply_table(a, t, 1), t, 0) == v).all()


def test_table_function_refuses_bad_arguments():
    import ctypes
    import svr_amd  # noqa: F401
    from svr_amd import _lib
    l = _lib.lib()
    assert l.svr_rgb_resize_taps(0, 8) == -2 and l.svr_rgb_resize_taps(8, 0) == -2 and l.svr_rgb_resize_taps(640, 256) == 7
    buf = np.zeros(8 * 5, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert l.svr_rgb_resize_table(5, 8, 2, p) == -1 and l.svr_rgb_resize_table(5, 8, 3, None) == -1
    assert l.svr_rgb_resize_table(5, 8, 3, p) == 0
