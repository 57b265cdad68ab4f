"""GPU suite of the keypoint stage (csrc/keypoints.hip) against tests/kp_ref.py: the heat map within
its derived tolerance, every stage behind it bit for bit, the whole detector against its own heat map and the golden file,
and the producer chain detect -> descriptor rows in the landing slot -> exchange -> match against the oracle."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kp_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "keypoints_small.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def random_heat():
    """3 x 120 x 160: the reference's own heat maps of the golden logits (different content per image)."""
    return np.stack([kp_ref.heat_as_written(l) for l in golden()["logits"]])


def sparse_heat(H, W, seed, rate=0.02):
    rng = np.random.default_rng(seed)
    h = rng.random((H, W), dtype=np.float32)
    return np.where(h > 1 - rate, h, np.float32(0.001)).astype(np.float32)


def run_nms(ctx, heat, K, thresh=0.015, radius=4, border=4):
    import torch
    from reconstructor_amd import keypoints
    heat = np.ascontiguousarray(heat, np.float32)
    r = keypoints.nms(ctx, torch.from_numpy(heat if heat.ndim == 3 else heat[None]).cuda(), K, thresh, radius, border)
    return {k: v.cpu().numpy() for k, v in r.items() if v is not None}


def check_exact(ctx, heat, K, thresh=0.015, radius=4, border=4, rounds=False):
    heat = np.ascontiguousarray(heat, np.float32)
    heat = heat if heat.ndim == 3 else heat[None]
    got = run_nms(ctx, heat, K, thresh, radius, border)
    counts = []
    for i, h in enumerate(heat):
        xy, conf, count = kp_ref.nms_greedy(h, thresh, radius, border, K)
        assert got["counts"][i] == count, (i, got["counts"][i], count)
        assert np.array_equal(got["xy"][i], xy), i
        assert got["conf"][i].tobytes() == conf.tobytes(), i
        if rounds:
            assert got["rounds"][i] == kp_ref.nms_fixed_point(h, thresh, radius)[1]
        counts.append(count)
    return counts, got


# ---- 1. heat tolerance ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["reference", "softmax"])
@pytest.mark.parametrize("H,W", [(40, 56), (120, 160)])
def test_heat_map_within_the_derived_tolerance(gpu_ctx, mode, H, W):
    """|got - want| <= 2^-21 want + 2^-126 against the float64 restatement: 1 ulp for expf (its documented accuracy on the
    device), <= 1 for S_r, which inherits it (the fp64 sums add nothing visible), 1/2 for rounding S_r to fp32, 1/2 for the
    division; 4 ulp with the margin."""
    import torch
    from reconstructor_amd import keypoints
    rng = np.random.default_rng(H)
    lg = (1.2 * rng.standard_normal((2, 65, H // 8, W // 8))).astype(np.float32)
    lg[0, 7, 1, 2] = 8.0
    lg[1, 64, 2, 3] = 6.0
    lg[1, 20, :, 1] = -8.0
    r = keypoints.detect(gpu_ctx, torch.from_numpy(lg).cuda(), H, W, 64, mode=keypoints.HEAT_REFERENCE if mode == "reference" else keypoints.HEAT_SOFTMAX,
                         want_heat=True)
    got = r["heat"].cpu().numpy().astype(np.float64)
    f = kp_ref.heat_reference_f64 if mode == "reference" else kp_ref.heat_softmax_f64
    want = np.stack([f(l) for l in lg])
    err = np.abs(got - want)
    print("heat %s %dx%d: max error %.2f ulp of fp32" % (mode, H, W, np.max(err / want) * 2.0 ** 23))
    assert (err <= 2.0 ** -21 * want + 2.0 ** -126).all()


# ---- 2. exact stages -----------------------------------------------------------------------------------------------------

def test_random_maps_three_images(gpu_ctx):
    counts, _ = check_exact(gpu_ctx, random_heat(), 512, rounds=True)
    assert counts == golden()["counts"].tolist()


def test_image_without_a_candidate(gpu_ctx):
    heat = random_heat().copy()
    heat[1] = np.float32(0.001)
    counts, got = check_exact(gpu_ctx, heat, 400, rounds=True)
    assert counts[1] == 0 and (got["xy"][1] == -1).all() and got["rounds"][1] == 0 and counts[0] > 0 and counts[2] > 0


@pytest.mark.parametrize("name", ["dense", "ties", "ramp"])
def test_dense_tie_heavy_and_ramp_maps(gpu_ctx, name):
    heat, thresh = kp_ref.named_maps()[name]
    counts, got = check_exact(gpu_ctx, heat, 512, thresh=thresh, border=0, rounds=True)
    assert counts[0] > 100
    if name == "ramp":
        assert got["rounds"][0] == 64


def test_corners_and_border_line(gpu_ctx):
    """Windows clipped by the image edge; a peak inside the border strip suppresses its neighbour and is then dropped; a peak
    on the border line itself (x == border) stays."""
    H, W = 64, 96
    heat = np.full((H, W), 0.001, np.float32)
    for (y, x), v in {(0, 0): 0.9, (0, W - 1): 0.8, (H - 1, 0): 0.7, (H - 1, W - 1): 0.6,       # corners
                      (1, 1): 0.5, (2, W - 3): 0.85,                                             # beside a corner: one loses, one wins
                      (20, 3): 0.9, (21, 6): 0.5,                                                # strip peak kills an inside point
                      (40, 4): 0.4, (H - 5, 50): 0.3, (H - 4, 70): 0.3, (10, W - 5): 0.2, (33, W - 4): 0.9}.items():
        heat[y, x] = v
    for border in (4, 0):
        counts, got = check_exact(gpu_ctx, heat, 32, border=border, rounds=True)
        kept = {tuple(p) for p in got["xy"][0, :counts[0]].tolist()}
        if border == 4:
            assert kept == {(4, 40), (50, H - 5), (W - 5, 10)}
        else:
            assert {(0, 0), (W - 3, 2), (0, H - 1), (W - 1, H - 1), (3, 20), (W - 4, 33)} <= kept and (6, 21) not in kept and (1, 1) not in kept


@pytest.mark.parametrize("radius", [0, 8])
def test_nms_radius_extremes(gpu_ctx, radius):
    counts, _ = check_exact(gpu_ctx, random_heat()[:2], 4096, radius=radius, rounds=True)
    if radius == 0:       # nothing suppresses anything: every candidate inside the border survives
        assert counts[0] == int((random_heat()[0][4:-4, 4:-4].astype(np.float64) >= 0.015).sum())


def test_border_zero_and_odd_sizes(gpu_ctx):
    check_exact(gpu_ctx, random_heat()[:1], 512, border=0)
    check_exact(gpu_ctx, sparse_heat(37, 53, 3, rate=0.2), 256, radius=2, border=1, rounds=True)
    check_exact(gpu_ctx, sparse_heat(1, 16, 4, rate=0.5), 16, radius=1, border=0, rounds=True)
    check_exact(gpu_ctx, random_heat()[:1], 512, border=60)          # the border swallows the image: nothing left
    check_exact(gpu_ctx, random_heat()[:1], 512, thresh=-1.0, radius=3)       # every pixel a candidate


def test_nan_pixels(gpu_ctx):
    heat = random_heat()[0].copy()
    cand = np.argwhere(heat >= 0.05)
    for y, x in cand[::7]:
        heat[y, x] = np.nan                 # strong peaks become holes: their neighbours are no longer suppressed by them
    heat[60, 80] = np.nan
    heat[0, 0] = -np.nan
    counts, got = check_exact(gpu_ctx, heat, 512, rounds=True)
    assert not np.isnan(got["conf"]).any() and counts[0] > 0


def test_cap_smaller_than_the_survivor_count(gpu_ctx):
    for K in (50, 1, 323):
        counts, got = check_exact(gpu_ctx, random_heat(), K)
        assert min(counts) > K or K == 323
    heat, thresh = kp_ref.named_maps()["ties"]          # the K-th key is decided by the raster index
    counts, _ = check_exact(gpu_ctx, heat, 40, thresh=thresh, border=0)
    assert counts[0] > 40


@pytest.mark.parametrize("side", ["lds", "global"])
def test_both_sides_of_the_status_switch(gpu_ctx, side):
    """The status map (2 bits per pixel) lives in LDS up to RCN_KP_LDS_STATUS_BYTES, in HBM beyond: the largest image of the
    one kind and one a little over it, plus the shapes the issue names."""
    from reconstructor_amd import keypoints
    limit = 4 * keypoints.LDS_STATUS_BYTES                 # pixels
    assert limit == 512 * 1024
    shapes = [(480, 640), (512, 1024)] if side == "lds" else [(520, 1016), (1088, 1920)]
    for H, W in shapes:
        assert (H * W <= limit) == (side == "lds")
        heat = sparse_heat(H, W, H, rate=0.004 if H > 600 else 0.02)
        heat[H - 1, W - 1] = 2.0            # the last pixel of the map is in play
        heat[H - 3, W - 2] = 1.5
        counts, _ = check_exact(gpu_ctx, heat, 8192, border=0)
        assert counts[0] > 1000
    heat = np.stack([sparse_heat(*shapes[1], s, rate=0.004) for s in (1, 2)])      # two images: per-image offsets of the status / list
    check_exact(gpu_ctx, heat, 2000)


# ---- 3. detect end to end ------------------------------------------------------------------------------------------------

def _detect(ctx, logits_t, H, W, K, **kw):
    from reconstructor_amd import keypoints
    r = keypoints.detect(ctx, logits_t, H, W, K, want_heat=True, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("mode", [0, 1])
def test_detect_equals_the_exact_stages_on_its_own_heat_map(gpu_ctx, mode):
    import torch
    rng = np.random.default_rng(5 + mode)
    H, W, K = 72, 104, 300
    lg = ((1.2 if mode == 0 else 3.0) * rng.standard_normal((3, 65, H // 8, W // 8))).astype(np.float32)
    got = _detect(gpu_ctx, torch.from_numpy(lg).cuda(), H, W, K, mode=mode)
    for i in range(3):
        xy, conf, count = kp_ref.nms_greedy(got["heat"][i], 0.015, 4, 4, K)
        assert count == got["counts"][i] > 20 and np.array_equal(xy, got["xy"][i]) and conf.tobytes() == got["conf"][i].tobytes()
        assert got["rounds"][i] == kp_ref.nms_fixed_point(got["heat"][i], 0.015, 4)[1]


def test_detect_reproduces_the_golden_keypoints(gpu_ctx):
    import torch
    g = golden()
    K = g["xy"].shape[1] + 7
    got = _detect(gpu_ctx, torch.from_numpy(g["logits"]).cuda(), 120, 160, K, conf_thresh=float(g["conf_thresh"]),
                  nms_radius=int(g["nms_radius"]), border=int(g["border"]))
    assert np.array_equal(got["counts"], g["counts"])
    for i, n in enumerate(g["counts"]):
        assert np.array_equal(got["xy"][i, :n], g["xy"][i, :n]) and (got["xy"][i, n:] == -1).all() and (got["conf"][i, n:] == 0).all()
        # the coordinates are exact (guard band of the golden input); the confidences carry the tolerance of the heat stage
        # (2^-21 to the float64 restatement) plus the distance of the stored fp32 heat map from it (2^-19, test_keypoints_ref.py)
        assert np.allclose(got["conf"][i, :n], g["conf"][i, :n], rtol=2.0 ** -21 + 2.0 ** -19, atol=0)


def test_layouts_and_repeated_runs_give_identical_bytes(gpu_ctx):
    import torch
    lg = torch.from_numpy(golden()["logits"]).cuda()
    nhwc = lg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # same values, channel-last memory
    assert nhwc.stride()[1] == 1 and torch.equal(nhwc, lg)
    for mode in (0, 1):
        a = _detect(gpu_ctx, lg, 120, 160, 400, mode=mode)
        b = _detect(gpu_ctx, nhwc, 120, 160, 400, mode=mode)
        c = _detect(gpu_ctx, lg, 120, 160, 400, mode=mode)
        for k in ("xy", "conf", "counts", "heat", "rounds"):
            assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), (mode, k)
        assert a["counts"].min() > 0


# ---- 4. producer chain ---------------------------------------------------------------------------------------------------

def test_detector_feeds_the_matcher_without_a_host_copy(gpu_ctx):
    import torch
    from oracle import orc
    from reconstructor_amd import keypoints, pairgrid
    from reconstructor_amd.matcher import all_pairs
    n, H, W, K, D = 4, 120, 160, 448, 256
    Hc, Wc = H // 8, W // 8
    rng = np.random.default_rng(21)
    lg = (1.2 * rng.standard_normal((n, 65, Hc, Wc))).astype(np.float32)
    lg[1:] = (0.7 * lg[0] + 0.3 * lg[1:]).astype(np.float32) * np.float32(1.3)          # the images share most of their keypoints' cells
    maps = rng.standard_normal((n, 256, Hc, Wc)).astype(np.float32)
    maps[1:] = (0.9 * maps[0] + 0.1 * maps[1:]).astype(np.float32)
    dl, dm = torch.from_numpy(lg).cuda(), torch.from_numpy(maps).cuda()
    sh = pairgrid.Shard(gpu_ctx, 0, 1, pairgrid.unique_id())
    try:
        gpu_ctx.check(gpu_ctx.lib.rcn_desc_clear(gpu_ctx.h))
        assert gpu_ctx.lib.rcn_desc_sample_errors(gpu_ctx.h, None) == 0
        slot = sh.reserve(n, K, D)
        r = keypoints.detect(gpu_ctx, dl, H, W, K)
        keypoints.sample_batch(gpu_ctx, dm, r["xy"], r["counts"], D, out=slot)
        counts = r["counts"].cpu().numpy()
        xy = r["xy"].cpu().numpy()
        assert (counts > 100).all() and (counts < K).all() and len(set(counts.tolist())) > 1
        # the batch rows: bit-equal to the single-image entry, image by image; tails zero; nothing counted as out of the map
        rows_dev = torch.empty((n, K, D), dtype=torch.float32, device="cuda")
        assert keypoints.sample_batch(gpu_ctx, dm, r["xy"], r["counts"], D, out=rows_dev.data_ptr()) is None
        batch = rows_dev.cpu().numpy()
        for i in range(n):
            m = int(counts[i])
            one = torch.full((m, D), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.check(gpu_ctx.lib.rcn_desc_sample_device(gpu_ctx.h, dm[i].data_ptr(), Hc * Wc, Wc, 1, Hc, Wc, r["xy"][i].data_ptr(), m, D, one.data_ptr()))
            gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
            assert batch[i, :m].tobytes() == one.cpu().numpy().tobytes()
            assert (batch[i, m:] == 0).all() and (xy[i, m:] == -1).all()
        n_bad = C.c_int32(-1)
        assert gpu_ctx.lib.rcn_desc_sample_errors(gpu_ctx.h, C.byref(n_bad)) == 0 and n_bad.value == 0
        rows = [orc.desc_sample(maps[i], xy[i, :counts[i]]) for i in range(n)]
        assert all(batch[i, :counts[i]].tobytes() == rows[i].tobytes() for i in range(n))
        exp, ec = orc.match_grid(rows, all_pairs(n), threads=4)
        sh.exchange(None, counts)
        P = n * (n - 1) // 2
        out = torch.empty((P, K), dtype=torch.int32, device="cuda")
        cnt = torch.empty((P,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sh.match(0.7, out.data_ptr(), K, cnt.data_ptr())
        gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
        got = out.cpu().numpy()
        assert np.array_equal(cnt.cpu().numpy(), ec) and ec.sum() > 0
        for p, (i, j) in enumerate(all_pairs(n)):
            assert np.array_equal(got[p, :counts[i]], exp[p, :counts[i]]), p
    finally:
        sh.close()


# ---- 5. argument errors --------------------------------------------------------------------------------------------------

def test_argument_errors(gpu_ctx):
    import torch
    lib, h = gpu_ctx.lib, gpu_ctx.h
    K = 16
    lg = torch.zeros((1, 65, 2, 2), dtype=torch.float32, device="cuda")
    heat = torch.zeros((1, 16, 16), dtype=torch.float32, device="cuda")
    xy = torch.full((K, 2), 5, dtype=torch.int32, device="cuda")
    counts = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def detect(logits=lg, n=1, H=16, W=16, mode=0, r=4, b=4, k=K, xy_=xy, cnt=counts):
        return lib.rcn_kp_detect_device(h, P(logits), 65 * 4, 4, 2, 1, n, H, W, mode, 0.015, r, b, k, P(xy_), None, P(cnt), None, None)

    def nms(heat_=heat, n=1, H=16, W=16, r=4, b=4, k=K, xy_=xy, cnt=counts):
        return lib.rcn_kp_nms_device(h, P(heat_), n, H, W, 0.015, r, b, k, P(xy_), None, P(cnt), None)

    def refused(rc, word):
        text = lib.rcn_last_error(h).decode()
        assert rc == -1 and word in text, (rc, text)

    refused(detect(H=12), "multiples of 8")
    refused(detect(W=20), "multiples of 8")
    refused(detect(H=0), "positive")
    refused(detect(n=-1), "n < 0")
    refused(detect(k=0), "K < 1")
    refused(detect(r=-1), "nms_radius")
    refused(detect(r=9), "nms_radius")
    refused(detect(b=-1), "border")
    refused(detect(mode=2), "mode")
    refused(detect(mode=-1), "mode")
    refused(detect(logits=None), "null")
    refused(detect(xy_=None), "null")
    refused(detect(cnt=None), "null")
    refused(detect(H=65536, W=32768), "2^31")
    refused(nms(H=65536, W=32768), "2^31")
    refused(nms(n=-1), "n < 0")
    refused(nms(k=0), "K < 1")
    refused(nms(r=9), "nms_radius")
    refused(nms(b=-1), "border")
    refused(nms(heat_=None), "null")
    refused(nms(cnt=None), "null")
    refused(nms(W=0), "positive")
    rows = torch.zeros((K, 256), dtype=torch.float32, device="cuda")
    dmap = torch.zeros((256, 2, 2), dtype=torch.float32, device="cuda")
    batch = lambda n=1, k=K, D=256, kp=xy, c=counts: lib.rcn_desc_sample_batch_device(h, P(dmap), 0, 4, 2, 1, 2, 2, P(kp), P(c), n, k, D, P(rows))
    refused(batch(n=-1), "rcn_desc_sample_batch_device")
    refused(batch(D=257), "rcn_desc_sample_batch_device")
    refused(batch(c=None), "rcn_desc_sample_batch_device")
    # nothing ran: the outputs are untouched
    gpu_ctx.check(lib.rcn_synchronize(h))
    assert (xy.cpu().numpy() == 5).all() and (counts.cpu().numpy() == 5).all()
    # n == 0 is fine and launches nothing
    assert detect(n=0) == 0 and nms(n=0) == 0 and batch(n=0) == 0
    gpu_ctx.check(lib.rcn_synchronize(h))
    assert (xy.cpu().numpy() == 5).all() and (counts.cpu().numpy() == 5).all()
    # and the smallest valid call works afterwards
    assert nms() == 0 and detect() == 0
    gpu_ctx.check(lib.rcn_synchronize(h))
