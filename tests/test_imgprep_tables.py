"""CPU suite: the pure host entries of the image-preparation stage (rcn_img_reshape_size, rcn_img_resize_tables,
rcn_img_prepare_plan) equal tests/img_ref.py exactly.  No device is needed: the tables are built on the host, in resize.cpp's own
float / double operations, and are all the floating point the stage has."""
import ctypes as C

import numpy as np
import pytest

import img_ref


@pytest.fixture(scope="module")
def imgprep():
    from reconstructor_amd import _build, imgprep
    _build.build()
    return imgprep


def test_reshape_size_equals_reference(imgprep):
    from reconstructor_amd import _lib
    rng = np.random.default_rng(0)
    cases = [(2048, 3072, 512), (3072, 2048, 512), (700, 700, 512), (300, 480, 512), (37, 50, 24), (50, 37, 24), (513, 512, 512), (512, 513, 512)]
    cases += [tuple(int(v) for v in rng.integers(1, 5000, 3)) for _ in range(3000)]
    errors = 0
    for rows, cols, mx in cases:
        try:
            want = img_ref.reshape_size(rows, cols, mx)
        except ValueError:
            errors += 1
            with pytest.raises(_lib.RcnError) as e:
                imgprep.reshape_size(rows, cols, mx)
            assert e.value.code == -1
            continue
        assert imgprep.reshape_size(rows, cols, mx) == want, (rows, cols, mx)
    assert errors > 0                                       # the sweep reaches the empty-side error
    assert imgprep.reshape_size(2048, 3072, 512) == (336, 512, 1.0 / 6.0)
    lib = _lib.load()
    r, c = C.c_int32(), C.c_int32()
    assert lib.rcn_img_reshape_size(0, 5, 5, C.byref(r), C.byref(c), None) == -1
    assert lib.rcn_img_reshape_size(5, 5, 5, None, C.byref(c), None) == -1
    assert lib.rcn_img_reshape_size(90, 50, 45, C.byref(r), C.byref(c), None) == 0 and (r.value, c.value) == (45, 24)     # factor_out may be NULL


def test_resize_tables_equal_reference_over_the_sweep(imgprep):
    """Source 9..700 against destination 1..130, both axes: equal sizes, the factor-2 pairs and enlargements are all inside."""
    srcs = range(9, 701)
    seen_equal = seen_half = seen_larger = 0
    for src in srcs:
        for dst in range(1, 131):
            seen_equal += src == dst
            seen_half += src == 2 * dst
            seen_larger += dst > src
            for horizontal in (True, False):
                s, w, xmax = imgprep.resize_tables(src, dst, horizontal)
                s0, w0, xmax0 = img_ref.resize_tables(src, dst, horizontal)
                assert np.array_equal(s, s0) and np.array_equal(w, w0) and xmax == xmax0, (src, dst, horizontal)
    assert seen_equal and seen_half and seen_larger


def test_resize_tables_of_the_large_cases(imgprep):
    for src, dst in ((3072, 512), (2048, 336), (2100, 30), (30000, 16), (10, 33), (12, 40)):
        for horizontal in (True, False):
            s, w, xmax = imgprep.resize_tables(src, dst, horizontal)
            s0, w0, xmax0 = img_ref.resize_tables(src, dst, horizontal)
            assert np.array_equal(s, s0) and np.array_equal(w, w0) and xmax == xmax0


def test_resize_tables_reject_bad_arguments(imgprep):
    from reconstructor_amd import _lib
    lib = _lib.load()
    idx, w = np.zeros(4, np.int32), np.zeros((4, 2), np.int16)
    assert lib.rcn_img_resize_tables(0, 4, 1, idx.ctypes.data, w.ctypes.data, None) == -1
    assert lib.rcn_img_resize_tables(4, 0, 1, idx.ctypes.data, w.ctypes.data, None) == -1
    assert lib.rcn_img_resize_tables(4, 4, 1, None, w.ctypes.data, None) == -1
    assert lib.rcn_img_resize_tables(8, 4, 1, idx.ctypes.data, w.ctypes.data, None) == 0          # xmax_out may be NULL


def test_plan_follows_the_horizontal_scale(imgprep):
    """The tile height shrinks as the staged spans grow; any scale up to 64 still stages its rows, and a span that cannot fit even
    once falls to the one-row tile that reads memory directly."""
    p = imgprep.plan(3072, 512, 3)
    assert p["tile_cols"] == 64 and p["tile_rows"] == 8 and 0 < p["lds_bytes"] <= 64 * 1024
    rows = [imgprep.plan(64 * s, 64, 3)["tile_rows"] for s in (1, 2, 6, 16, 32, 64)]
    assert all(r >= 1 for r in rows) and rows == sorted(rows, reverse=True) and rows[0] == 8 and rows[-1] < 8
    direct = imgprep.plan(30000, 16, 3)
    assert direct["tile_rows"] == 0 and direct["lds_bytes"] < p["lds_bytes"]
    assert imgprep.plan(33, 16, 3)["tile_rows"] == 8 and imgprep.plan(10, 33, 1)["tile_rows"] == 8
    default = imgprep.options()
    assert (default.order, default.gray_bits) == (1, 14)
