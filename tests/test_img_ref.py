"""CPU suite: tests/img_ref.py, the contract of the image-preparation stage, checked against itself -- OpenCV is not available
here, so what can be checked is the restatement's own structure: the sizes reshapeImg asks for, weights that sum to one, constants
that stay constant, the branch that is taken, and the distance of the fixed-point arithmetic from float64 bilinear
interpolation, within the bound derived in img_ref's docstring."""
import numpy as np
import pytest

import img_ref

# (source rows, source cols, rows, cols) of every resize the GPU suite runs, plus the reference's own case
SHAPES = [(37, 50, 16, 24), (50, 37, 24, 16), (40, 64, 16, 32), (48, 64, 24, 32), (12, 10, 40, 33), (2048, 3072, 336, 512), (2100, 33, 30, 16),
          (4, 30000, 4, 16), (31, 29, 31, 29), (43, 239, 19, 141), (11, 1500, 11, 70), (5, 4000, 5, 70), (45, 77, 19, 35), (150, 200, 72, 96)]


def test_reshape_size():
    assert img_ref.reshape_size(2048, 3072, 512) == (336, 512, 1.0 / 6.0)
    assert img_ref.reshape_size(3072, 2048, 512) == (512, 336, 1.0 / 6.0)
    assert img_ref.reshape_size(700, 700, 512) == (512, 512, 512.0 / 700.0)          # rows == cols takes the second branch
    assert img_ref.reshape_size(300, 480, 512) == (300, 480, 1.0)
    assert img_ref.reshape_size(480, 300, 512) == (480, 300, 1.0)
    assert img_ref.reshape_size(37, 50, 24) == (16, 24, 24.0 / 50.0)
    with pytest.raises(ValueError):
        img_ref.reshape_size(1000, 15, 100)          # 1.5 columns, cut down to a multiple of 8: none
    with pytest.raises(ValueError):
        img_ref.reshape_size(0, 5, 100)


@pytest.mark.parametrize("shape", SHAPES)
def test_weights_sum_to_one(shape):
    H, W, rows, cols = shape
    for src, dst, horizontal in ((W, cols, True), (H, rows, False)):
        s, w, xmax = img_ref.resize_tables(src, dst, horizontal)
        assert (w.astype(np.int32).sum(1) == img_ref.ONE).all() and (w >= 0).all()
        if horizontal:
            assert s.min() >= 0 and s.max() <= src - 1 and (np.diff(s) >= 0).all()
            assert (w[xmax:, 0] == img_ref.ONE).all() and (s[xmax:] == src - 1).all() and (s[:xmax] + 1 < src).all()
        else:
            assert s.min() >= -1 and s.max() <= src - 1 and xmax == dst


def test_enlargement_reaches_both_border_branches():
    s, w, xmax = img_ref.resize_tables(10, 33, True)
    assert xmax < 33 and (w[0] == (img_ref.ONE, 0)).all()        # s < 0 on the left: f zeroed; xmax on the right
    sv, wv, _ = img_ref.resize_tables(12, 40, False)
    assert sv[0] == -1 and wv[0, 1] != 0                          # vertically f is NOT zeroed: both clipped rows are row 0


def test_constant_images_stay_constant():
    for H, W, rows, cols in [s for s in SHAPES if s[0] * s[1] < 10000]:
        vals = np.arange(256, dtype=np.uint8)
        img = np.broadcast_to(vals[:, None, None, None], (256, H, W, 3))
        for v in (0, 1, 127, 128, 254, 255):
            assert (img_ref.resize_linear_u8(np.ascontiguousarray(img[v]), rows, cols) == v).all()
    # every value through one fractional resize and both grey tables
    for v in range(256):
        out = img_ref.resize_linear_u8(np.full((37, 50, 3), v, np.uint8), 16, 24)
        assert (out == v).all()
        assert (img_ref.rgb_to_gray_u8(out, 14) == v).all() and (img_ref.rgb_to_gray_u8(out, 15) == v).all()
        assert (img_ref.resize_linear_u8(np.full((48, 64), v, np.uint8), 24, 32) == v).all()
        assert (img_ref.resize_linear_u8(np.full((12, 10), v, np.uint8), 40, 33) == v).all()


@pytest.mark.parametrize("shape", [s for s in SHAPES if max(s[0], s[1]) <= 4096 and not img_ref.is_area_fast(*s)])
def test_fixed_point_within_derived_bound_of_float64(shape):
    H, W, rows, cols = shape
    rng = np.random.default_rng(H * 7 + W)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img[::3, ::2] = 255
    img[1::3, 1::2] = 0                                            # full-swing neighbours: the worst case of every weight error
    got = img_ref.resize_linear_u8(img, rows, cols).astype(np.float64)
    want = img_ref.resize_bilinear_f64(img, rows, cols)
    err = np.abs(got - want).max()
    print("%s: max |fixed point - float64| = %.4f grey levels (bound %.2f)" % (shape, err, img_ref.RESIZE_BOUND))
    assert err <= img_ref.RESIZE_BOUND


def test_area_branch_is_taken_only_when_both_axes_halve():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    assert img_ref.is_area_fast(48, 64, 24, 32)
    blocks = a.astype(np.int32).reshape(24, 2, 32, 2, 3)
    assert np.array_equal(img_ref.resize_linear_u8(a, 24, 32), ((blocks.sum((1, 3)) + 2) >> 2).astype(np.uint8))
    b = rng.integers(0, 256, (40, 64, 3), dtype=np.uint8)
    assert not img_ref.is_area_fast(40, 64, 16, 32)
    out = img_ref.resize_linear_u8(b, 16, 32)
    xs, xw, _ = img_ref.resize_tables(64, 32, True)
    assert (xw == 1024).all() and np.array_equal(xs, 2 * np.arange(32))                # x halves exactly ...
    ys, yw, _ = img_ref.resize_tables(40, 16, False)
    assert not (yw[:, 0] == 1024).all()                                                 # ... y does not: the linear path
    y, x = 5, 7
    h0 = b[ys[y], 2 * x].astype(np.int32) * 1024 + b[ys[y], 2 * x + 1].astype(np.int32) * 1024
    h1 = b[ys[y] + 1, 2 * x].astype(np.int32) * 1024 + b[ys[y] + 1, 2 * x + 1].astype(np.int32) * 1024
    v = ((int(yw[y, 0]) * (h0 >> 4)) >> 16) + ((int(yw[y, 1]) * (h1 >> 4)) >> 16)
    assert np.array_equal(out[y, x], ((v + 2) >> 2).astype(np.uint8))


def test_equal_sizes_copy_and_linear_formula_agrees():
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (31, 29, 3), dtype=np.uint8)
    assert np.array_equal(img_ref.resize_linear_u8(a, 31, 29), a)
    s, w, _ = img_ref.resize_tables(29, 29, True)
    assert np.array_equal(s, np.arange(29)) and (w == (img_ref.ONE, 0)).all()          # the tables of a copy are the identity


def test_prepare_order_and_grey_of_the_resized_image():
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (37, 50, 3), dtype=np.uint8)
    rgb, gray, factor = img_ref.prepare(bgr, "bgr", 24)
    rgb2, gray2, _ = img_ref.prepare(np.ascontiguousarray(bgr[:, :, ::-1]), "rgb", 24)
    assert np.array_equal(rgb, rgb2) and np.array_equal(gray, gray2) and factor == 24.0 / 50.0
    assert np.array_equal(gray, img_ref.rgb_to_gray_u8(rgb)) and rgb.shape == (16, 24, 3)
    assert not np.array_equal(gray, img_ref.resize_linear_u8(img_ref.rgb_to_gray_u8(bgr[:, :, ::-1]), 16, 24))     # not readGrayImg's order
    lattice = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij"), -1).astype(np.uint8)
    g14, g15 = img_ref.rgb_to_gray_u8(lattice, 14).astype(int), img_ref.rgb_to_gray_u8(lattice, 15).astype(int)
    assert 0 < np.abs(g14 - g15).max() <= 1          # the two tables are different roundings of the same weights: rarely, and by one
    none, plane, _ = img_ref.prepare(bgr[:, :, 0], "bgr", 24)
    assert none is None and np.array_equal(plane, img_ref.resize_linear_u8(np.ascontiguousarray(bgr[:, :, 0]), 16, 24))


def test_colours_and_cloud():
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    xy = np.array([[0, 0], [23, 15], [24, 0], [5, -1], [3, 4]], np.int32)
    c = img_ref.feat_colors(rgb, xy, 4)
    assert np.array_equal(c[0, :3], rgb[0, 0]) and np.array_equal(c[1, :3], rgb[15, 23]) and not c[2:].any() and not c[:, 3].any()
    lm = img_ref.landmark_colors(c[None], [0, 0, 1, 0], [1, 7, 0, -1])
    assert np.array_equal(lm[0], c[1]) and not lm[1:].any()
    xyz = rng.normal(size=(5, 3))
    P = np.concatenate([np.eye(3), [[1.0], [2.0], [3.0]]], 1).reshape(1, 12)
    v = img_ref.cloud_vertices(xyz, rng.integers(1, 250, (5, 4), dtype=np.uint8), [1, 0, 1, 1, 0], P)
    assert len(v) == 11 and v.dtype.itemsize == 16 and (v["alpha"] == 255).all()
    assert [tuple(r)[3:6] == img_ref.OUTLIER_RGB for r in v[:5].tolist()] == [False, True, False, False, True]
    assert np.array_equal(v["x"][:5], v["x"][5:10]) and tuple(v[10].tolist())[:6] == (-1.0, -2.0, -3.0) + img_ref.CAMERA_RGB
    assert len(img_ref.cloud_vertices(xyz, np.zeros((5, 3), np.uint8), None, P)) == 6
