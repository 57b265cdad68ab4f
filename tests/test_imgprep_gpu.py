"""GPU suite: the image-preparation stage (rcn_img_prepare_device, rcn_feat_colors_device, rcn_landmark_colors_device,
rcn_cloud_vertices_device, rcn_cloud_write_ply; csrc/imgprep.hip) against tests/img_ref.py, byte for byte: the kernels do integer
arithmetic on tables the host built, so there is no tolerance anywhere in this file."""
import ctypes as C
import os

import numpy as np
import pytest

import img_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(H, W, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, ch), dtype=np.uint8)


def _gradient(H, W, ch):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(5 * x + y) % 256, (255 - 3 * y - x) % 256, (2 * x + 4 * y) % 256][:ch], -1).astype(np.uint8)


def _pair(H, W, ch=3, seed=0):
    """A seeded noise image and a smooth gradient: a wrong index shows on the first, a wrong weight on the second."""
    return np.stack([_noise(H, W, ch, seed), _gradient(H, W, ch)])


def _ref(src, rows, cols, order="bgr", bits=14):
    """img_ref's chain to an explicit size: (rgb, gray) of one image [H][W][3], or (None, plane) of [H][W]."""
    if src.ndim == 2:
        return None, img_ref.resize_linear_u8(src, rows, cols)
    rgb = img_ref.resize_linear_u8(np.ascontiguousarray(src[:, :, ::-1] if order == "bgr" else src), rows, cols)
    return rgb, img_ref.rgb_to_gray_u8(rgb, bits)


def _run(ctx, srcs, rows, cols, **kw):
    import torch
    from reconstructor_amd import imgprep
    rgb, gray = imgprep.prepare_to(ctx, torch.from_numpy(np.ascontiguousarray(srcs)).cuda(), rows, cols, **kw)
    return (None if rgb is None else rgb.cpu().numpy()), (None if gray is None else gray.cpu().numpy())


def _check(ctx, srcs, rows, cols, **kw):
    rgb, gray = _run(ctx, srcs, rows, cols, **kw)
    assert rgb.shape == (len(srcs), rows, cols, 3) and gray.shape == (len(srcs), rows, cols)
    for i, s in enumerate(srcs):
        r0, g0 = _ref(s, rows, cols, kw.get("order", "bgr"), kw.get("gray_bits", 14))
        assert np.array_equal(rgb[i], r0), "colour of image %d differs at %s" % (i, np.argwhere(rgb[i] != r0)[:4].tolist())
        assert np.array_equal(gray[i], g0), "grey of image %d differs" % i


def _tiled_case():
    """A destination that crosses two tile boundaries on each axis and ends in a partial tile, at a non-integer scale, from the
    kernel's own tile."""
    from reconstructor_amd import imgprep
    cols = 2 * imgprep.plan(240, 141)["tile_cols"] + 13
    src_cols = int(cols * 1.7)
    p = imgprep.plan(src_cols, cols)
    rows = 2 * p["tile_rows"] + 3
    assert p["tile_rows"] >= 1 and cols > 2 * p["tile_cols"] and cols % p["tile_cols"] and rows % p["tile_rows"]
    return int(rows * 2.3), src_cols, rows, cols


CASES = {
    "fractional 2.31 x 2.08": lambda: (37, 50) + img_ref.reshape_size(37, 50, 24)[:2],
    "portrait": lambda: (50, 37) + img_ref.reshape_size(50, 37, 24)[:2],
    "x exactly 2, y 2.5: linear": lambda: (40, 64, 16, 32),
    "2 x 2 area": lambda: (48, 64, 24, 32),
    "copy": lambda: (31, 29, 31, 29),
    "enlargement": lambda: (12, 10, 40, 33),
    "tile boundaries": _tiled_case,
    "vertical scale 70": lambda: (2100, 33, 30, 16),
    "tile of 4 rows": lambda: (11, 1500, 11, 70),
    "tile of 2 rows": lambda: (5, 4000, 5, 70),
    "scale 64, staged": lambda: (3, 4096, 3, 64),
    "tile of 1 row": lambda: (3, 9000, 3, 64),
    "one-row tile without staging": lambda: (4, 30000, 4, 16),
}


@pytest.mark.parametrize("name", list(CASES))
def test_prepare_equals_reference(gpu_ctx, name):
    from reconstructor_amd import imgprep
    H, W, rows, cols = CASES[name]()
    if name == "fractional 2.31 x 2.08":
        assert (rows, cols) == (16, 24)
    tr = imgprep.plan(W, cols)["tile_rows"]
    want = {"tile of 4 rows": 4, "tile of 2 rows": 2, "scale 64, staged": 2, "tile of 1 row": 1, "one-row tile without staging": 0}.get(name, 8)
    assert tr == want, "the case no longer reaches the path it was written for"
    if name == "tile of 1 row":
        assert imgprep.plan(W, cols)["lds_bytes"] > 48 * 1024          # the largest staging the suite runs
    assert img_ref.is_area_fast(H, W, rows, cols) == (name == "2 x 2 area")
    _check(gpu_ctx, _pair(H, W, 3, seed=len(name)), rows, cols)


def test_the_reference_s_own_case(gpu_ctx):
    """One 2048 x 3072 photograph to 336 x 512."""
    rows, cols, factor = img_ref.reshape_size(2048, 3072, 512)
    assert (rows, cols) == (336, 512)
    _check(gpu_ctx, _noise(2048, 3072, 3, 99)[None], rows, cols)


def test_strides_order_bits_channels_and_single_outputs(gpu_ctx):
    import torch
    from reconstructor_amd import imgprep
    H, W, rows, cols = 37, 50, 16, 24
    srcs = _pair(H, W, 3, seed=21)
    want = [_ref(s, rows, cols) for s in srcs]
    # a row stride with 5 bytes of padding, an image stride with a gap of two rows and three bytes
    buf = torch.full((2 * ((H + 2) * (W * 3 + 5) + 3),), 0xAB, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((2, H, W, 3), ((H + 2) * (W * 3 + 5) + 3, W * 3 + 5, 3, 1), 1)           # and an odd first address
    view.copy_(torch.from_numpy(srcs).cuda())
    rgb, gray = imgprep.prepare_to(gpu_ctx, view, rows, cols)
    for i in range(2):
        assert np.array_equal(rgb[i].cpu().numpy(), want[i][0]) and np.array_equal(gray[i].cpu().numpy(), want[i][1])
    # BGR against RGB: the same bytes after swapping the input
    rgb2, gray2 = _run(gpu_ctx, srcs[..., ::-1], rows, cols, order="rgb")
    assert np.array_equal(rgb2, rgb.cpu().numpy()) and np.array_equal(gray2, gray.cpu().numpy())
    rgb3, _ = _run(gpu_ctx, srcs, rows, cols, order="rgb")
    assert np.array_equal(rgb3, rgb2[..., ::-1])
    # both grey tables, on colours where they differ (a copy keeps the lattice) and through a resize
    lat = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij"), -1).astype(np.uint8).reshape(1, 52 * 4, 13 * 52, 3)
    g = {b: _run(gpu_ctx, lat, 52 * 4, 13 * 52, order="rgb", gray_bits=b)[1] for b in (14, 15)}
    assert not np.array_equal(g[14], g[15])
    for b in (14, 15):
        assert np.array_equal(g[b][0], img_ref.rgb_to_gray_u8(lat[0], b))
        _check(gpu_ctx, srcs, rows, cols, gray_bits=b)
    # one channel: readGrayImg + reshapeImg
    planes = np.ascontiguousarray(srcs[..., 1])
    none, plane = _run(gpu_ctx, planes, rows, cols)
    assert none is None and all(np.array_equal(plane[i], img_ref.resize_linear_u8(planes[i], rows, cols)) for i in range(2))
    _, plane_big = _run(gpu_ctx, planes, 40, 33)
    assert np.array_equal(plane_big[0], img_ref.resize_linear_u8(planes[0], 40, 33))
    # either output alone
    only_rgb, no_gray = _run(gpu_ctx, srcs, rows, cols, want_gray=False)
    no_rgb, only_gray = _run(gpu_ctx, srcs, rows, cols, want_rgb=False)
    assert no_gray is None and no_rgb is None and np.array_equal(only_rgb, rgb.cpu().numpy()) and np.array_equal(only_gray, gray.cpu().numpy())
    # the public chain: sizes from reshape_size, the factor with them
    rgb4, gray4, factor = imgprep.prepare(gpu_ctx, torch.from_numpy(srcs).cuda(), max_size=24)
    assert factor == 24.0 / 50.0 and np.array_equal(rgb4.cpu().numpy(), rgb.cpu().numpy())
    # n == 0 launches nothing and returns empty results
    e_rgb, e_gray = imgprep.prepare_to(gpu_ctx, torch.zeros((0, H, W, 3), dtype=torch.uint8, device="cuda"), rows, cols)
    assert tuple(e_rgb.shape) == (0, rows, cols, 3) and tuple(e_gray.shape) == (0, rows, cols)


def test_an_image_does_not_depend_on_its_batch(gpu_ctx):
    H, W, rows, cols = 45, 77, 19, 35
    srcs = np.stack([_noise(H, W, 3, 40 + i) for i in range(5)])
    rgb, gray = _run(gpu_ctx, srcs, rows, cols)
    again = _run(gpu_ctx, srcs, rows, cols)
    assert np.array_equal(rgb, again[0]) and np.array_equal(gray, again[1])
    perm = [3, 0, 4, 2, 1]
    rgb_p, gray_p = _run(gpu_ctx, srcs[perm], rows, cols)
    for i in range(5):
        alone = _run(gpu_ctx, srcs[i:i + 1], rows, cols)
        assert np.array_equal(alone[0][0], rgb[i]) and np.array_equal(alone[1][0], gray[i])
        assert np.array_equal(rgb_p[i], rgb[perm[i]]) and np.array_equal(gray_p[i], gray[perm[i]])


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "imgprep_small.npz")))


def test_golden_file(gpu_ctx, golden):
    import torch
    from reconstructor_amd import imgprep
    g = golden
    rgb, gray, factor = imgprep.prepare(gpu_ctx, torch.from_numpy(g["images"]).cuda(), max_size=24)
    assert np.array_equal(rgb.cpu().numpy(), g["rgb"]) and np.array_equal(gray.cpu().numpy(), g["gray"]) and factor == float(g["factor"])
    feat = imgprep.feat_colors(gpu_ctx, rgb, torch.from_numpy(g["xy_int"]).cuda(), torch.from_numpy(g["counts"]).cuda())
    assert np.array_equal(feat.cpu().numpy(), g["feat_rgba"])
    lm = imgprep.landmark_colors(gpu_ctx, feat, g["first_img"], g["first_feat"])
    assert np.array_equal(lm.cpu().numpy(), g["lm_rgba"])
    v = imgprep.cloud_vertices(gpu_ctx, g["xyz"], lm, g["inlier"], g["poses34"])
    assert v.tobytes() == g["vertices"].tobytes()
    assert imgprep.cloud_vertices(gpu_ctx, g["xyz"], lm, None, g["poses34"]).tobytes() == g["vertices_plain"].tobytes()


def test_feat_and_landmark_colors(gpu_ctx):
    import torch
    from reconstructor_amd import imgprep
    rows, cols, n, K = 16, 24, 3, 10
    rng = np.random.default_rng(8)
    rgb = rng.integers(1, 256, (n, rows, cols, 3), dtype=np.uint8)
    xy = np.stack([rng.integers(0, cols, (n, K)), rng.integers(0, rows, (n, K))], -1).astype(np.int32)
    xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3] = (0, 5), (cols - 1, 5), (7, 0), (7, rows - 1)        # a coordinate on every edge
    xy[:, 4] = (cols, 0)                                                                           # one outside
    xy[1, 5], xy[2, 5] = (3, rows), (-1, 2)
    counts = np.array([7, 10, 14], np.int32)                                                       # below, at and above K
    got = imgprep.feat_colors(gpu_ctx, torch.from_numpy(rgb).cuda(), torch.from_numpy(xy).cuda(), torch.from_numpy(counts).cuda())
    want = np.stack([img_ref.feat_colors(rgb[i], xy[i], counts[i]) for i in range(n)])
    assert np.array_equal(got.cpu().numpy(), want)
    assert not want[0, 7:].any() and not want[:, 4].any() and want[:, :4, :3].all() and not want[..., 3].any()
    first_img = np.array([0, 2, 1, 3, -1, 1, 2], np.int32)
    first_feat = np.array([0, 9, 3, 0, 0, K, -1], np.int32)
    lm = imgprep.landmark_colors(gpu_ctx, got, first_img, first_feat)
    want_lm = img_ref.landmark_colors(want, first_img, first_feat)
    assert np.array_equal(lm.cpu().numpy(), want_lm) and want_lm[:3].any(1).all() and not want_lm[3:].any()
    assert tuple(imgprep.landmark_colors(gpu_ctx, got, [], []).shape) == (0, 4)


def _rotation(w):
    t = np.linalg.norm(w)
    k = w / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


@pytest.mark.parametrize("L", [0, 1, 300])
@pytest.mark.parametrize("Cn", [1, 7])
def test_cloud_vertices_and_ply(gpu_ctx, tmp_path, L, Cn):
    from reconstructor_amd import imgprep
    rng = np.random.default_rng(100 * L + Cn)
    xyz = rng.normal(size=(L, 3)) * 1e3 ** rng.uniform(-1, 1, (L, 1))
    col = rng.integers(0, 256, (L, 4), dtype=np.uint8)
    inl = (np.arange(L) % 3 != 0).astype(np.uint8)                                    # a third outliers
    poses = np.stack([np.concatenate([_rotation(rng.normal(size=3)), rng.normal(size=(3, 1)) * 10], 1).reshape(12) for _ in range(Cn)])
    for flags in (inl, None):
        v = imgprep.cloud_vertices(gpu_ctx, xyz, col, flags, poses)
        want = img_ref.cloud_vertices(xyz, col, flags, poses)
        assert len(v) == (2 if flags is not None else 1) * L + Cn
        assert v.tobytes() == want.tobytes()                                          # colours and floats alike, bit for bit
        for binary in (False, True):
            path = tmp_path / ("cloud_%d.ply" % binary)
            imgprep.write_ply(path, v, binary)
            assert img_ref.read_ply(path).tobytes() == v.tobytes()
    lib = gpu_ctx.lib
    assert lib.rcn_cloud_write_ply(str(tmp_path / "missing" / "cloud.ply").encode(), None, 0, 0) == -8
    assert lib.rcn_cloud_write_ply(None, None, 0, 0) == -1 and lib.rcn_cloud_write_ply(b"x.ply", None, 3, 0) == -1


def test_producer_chain_into_sift(gpu_ctx):
    """prepare, then sift.detect_and_compute on its grey image, equals the same call on img_ref.prepare's; the colours under
    the keypoints equal the reference's."""
    import torch
    from reconstructor_amd import imgprep, sift
    from reconstructor_amd.synth import blob_image
    H, W = 150, 200
    rng = np.random.default_rng(17)
    ims = []
    for s in range(2):
        chans = []
        for c in range(3):
            blobs = [(rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(3, 9), rng.uniform(3, 9), rng.uniform(0, 3.1),
                      rng.uniform(40, 110) * rng.choice([-1, 1])) for _ in range(16)]
            chans.append(np.rint(blob_image(H, W, blobs, texture=3.0, seed=10 * s + c)).astype(np.uint8))
        ims.append(np.stack(chans, -1))
    ims = np.stack(ims)
    ref = [img_ref.prepare(im, "bgr", 96) for im in ims]
    rgb, gray, factor = imgprep.prepare(gpu_ctx, torch.from_numpy(ims).cuda(), max_size=96)
    assert tuple(gray.shape) == (2, 72, 96) and factor == ref[0][2]
    K = 128
    got = sift.detect_and_compute(gpu_ctx, gray, K)
    want = sift.detect_and_compute(gpu_ctx, torch.from_numpy(np.stack([r[1] for r in ref])).cuda(), K)
    assert (got["counts"] > 0).all()
    for k in got:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    col = imgprep.feat_colors(gpu_ctx, rgb, got["xy_int"], got["counts"]).cpu().numpy()
    xy, counts = got["xy_int"].cpu().numpy(), got["counts"].cpu().numpy()
    for i in range(2):
        assert np.array_equal(col[i], img_ref.feat_colors(ref[i][0], xy[i], counts[i]))
        assert col[i, :min(counts[i], K), :3].any()


def test_session_chain_to_a_coloured_ply(gpu_ctx, tmp_path):
    """A small synthetic scene through a BA session: save_cloud after validity has 2 L + C vertices, red ones exactly where
    the flags are 0."""
    from reconstructor_amd import ba, imgprep, synth_ba
    nc, L = 6, 150
    c = synth_ba.make_validity_case(nc, L, obs_per_point=4, seed=9, defect_rate=0.2)
    ses = ba.BaSession(gpu_ctx)
    try:
        for l in range(nc):
            ses.add_camera(np.zeros(6), c["intrinsics"][l])
        ses.add_points(c["points"])
        ses.add_observations(np.repeat(np.arange(L), np.diff(c["pt_off"])).astype(np.int32), c["obs_cam"], c["obs_xy"])
        inl, _ = ses.validity(c["poses34"], 4.0, 1.0)
        assert 0 < inl.sum() < L
        col = np.random.default_rng(1).integers(0, 250, (L, 4), dtype=np.uint8)          # never the outliers' 253
        for binary in (False, True):
            path = tmp_path / ("session_%d.ply" % binary)
            v = imgprep.save_cloud(ses, path, inl, binary=binary, lm_rgba=col, poses34=c["poses34"])
            back = img_ref.read_ply(path)
            assert back.tobytes() == v.tobytes() and len(back) == 2 * L + nc
            red = (back["red"] == 253) & (back["green"] == 0) & (back["blue"] == 0)
            assert np.array_equal(red[:L], ~inl) and not red[L:].any()
            assert back.tobytes() == img_ref.cloud_vertices(ses.points(), col, inl, c["poses34"]).tobytes()
        plain = imgprep.save_cloud(ses, tmp_path / "plain.ply", lm_rgba=col, poses34=c["poses34"])
        assert len(plain) == L + nc and len(imgprep.save_cloud(ses, tmp_path / "own_poses.ply", inl)) == 2 * L + nc
    finally:
        ses.close()


def test_bad_arguments_are_refused_before_anything_is_launched(gpu_ctx):
    import torch
    from reconstructor_amd import _lib
    lib, h = gpu_ctx.lib, gpu_ctx.h
    H, W, rows, cols = 20, 30, 10, 15
    src = torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda")
    rgb = torch.full((1, rows, cols, 3), 7, dtype=torch.uint8, device="cuda")
    gray = torch.full((1, rows, cols), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s, r, g = src.data_ptr(), rgb.data_ptr(), gray.data_ptr()

    def opt(order=1, bits=14):
        o = _lib.ImgOptions()
        o.order, o.gray_bits = order, bits
        return C.byref(o)

    def call(src_p=s, si=H * W * 3, sr=W * 3, ch=3, n=1, sh=H, sw=W, dr=rows, dc=cols, o=None, rgb_p=r, gray_p=g):
        return lib.rcn_img_prepare_device(h, src_p, si, sr, ch, n, sh, sw, dr, dc, o, rgb_p, gray_p)

    bad = {
        "null source": dict(src_p=None), "both outputs null": dict(rgb_p=None, gray_p=None), "two channels": dict(ch=2), "four channels": dict(ch=4),
        "no source rows": dict(sh=0), "no source columns": dict(sw=0), "no rows": dict(dr=0), "negative columns": dict(dc=-3), "negative n": dict(n=-1),
        "short row stride": dict(sr=W * 3 - 1), "output too large": dict(dr=30000, dc=30000), "unknown order": dict(o=opt(order=2)),
        "unknown grey table": dict(o=opt(bits=16)), "colour output of a plane": dict(ch=1, sr=W),
        "more tiles than a launch holds": dict(dr=150_000_000, dc=1),
    }
    for name, kw in bad.items():
        assert call() == 0                                                # clears nothing, but the next text must be this call's own
        assert call(**kw) == -1, name
        text = lib.rcn_last_error(h).decode()
        assert text.startswith("rcn_img_prepare_device: bad argument ("), (name, text)
    assert lib.rcn_img_prepare_device(None, s, H * W * 3, W * 3, 3, 1, H, W, rows, cols, None, r, g) == -1
    rgb.fill_(7)
    gray.fill_(7)
    torch.cuda.synchronize()
    for kw in bad.values():
        call(**kw)
    assert call(n=0, src_p=None) == 0                                     # an empty batch needs no buffer
    gpu_ctx.check(lib.rcn_synchronize(h))
    assert (rgb == 7).all() and (gray == 7).all()                         # nothing was launched
    xy = torch.zeros((1, 4, 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    out = torch.zeros((1, 4, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.rcn_feat_colors_device(h, r, 1, rows, cols, xy.data_ptr(), cnt.data_ptr(), 0, out.data_ptr()) == -1
    assert lib.rcn_last_error(h).decode().startswith("rcn_feat_colors_device: bad argument (")
    assert lib.rcn_feat_colors_device(h, None, 1, rows, cols, xy.data_ptr(), cnt.data_ptr(), 4, out.data_ptr()) == -1
    assert lib.rcn_feat_colors_device(h, None, 0, rows, cols, None, None, 4, None) == 0
    assert lib.rcn_feat_colors_device(h, r, 1 << 22, rows, cols, xy.data_ptr(), cnt.data_ptr(), 2048, out.data_ptr()) == -1      # 2^33 slots: no launch holds them
    assert "more than one launch holds" in lib.rcn_last_error(h).decode()
    assert lib.rcn_landmark_colors_device(h, out.data_ptr(), 1, 4, 2, None, None, None) == -1
    assert lib.rcn_last_error(h).decode().startswith("rcn_landmark_colors_device: bad argument (")
    nv = C.c_int64(-5)
    assert lib.rcn_cloud_vertices_device(h, None, None, None, 2, None, 0, None, C.byref(nv)) == -1 and nv.value == -5
    assert lib.rcn_last_error(h).decode().startswith("rcn_cloud_vertices_device: bad argument (")
    assert lib.rcn_cloud_vertices_device(h, out.data_ptr(), out.data_ptr(), out.data_ptr(), 2 ** 31 - 1, None, 0, out.data_ptr(), C.byref(nv)) == -1 and nv.value == -5
    assert "more vertices than one launch holds" in lib.rcn_last_error(h).decode()
    assert lib.rcn_cloud_vertices_device(h, None, None, None, 0, None, 0, None, None) == -1
    assert lib.rcn_cloud_vertices_device(h, None, None, None, 0, None, 0, None, C.byref(nv)) == 0 and nv.value == 0
