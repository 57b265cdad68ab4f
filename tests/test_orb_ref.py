"""CPU suite of the ORB stage's contract (tests/orb_ref.py): the host entry rcn_orb_layout against the
restatement, the FAST score against a brute-force sweep over t, planted corners, the strict maximum, ties kept, the quarter turn
(exact), the built-in pattern against its generator and the golden file against its generator.  No device is needed."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import orb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orb():
    from reconstructor_amd import _build, orb
    _build.build()
    return orb


def generator():
    spec = importlib.util.spec_from_file_location("make_orb_golden", os.path.join(ROOT, "tests", "golden", "make_orb_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def half_shape():
    """the smallest H with H / scale_l within 1e-6 of a half at some level l >= 1 of the default pyramid"""
    for H in range(8, 4000):
        for l in range(1, 8):
            q = np.float64(H) / np.float64(np.float32(1.2 ** l))
            if abs(q - np.floor(q) - 0.5) < 1e-6:
                return H, l
    raise AssertionError("no such shape")


def same_layout(got, want):
    for k in ("n_levels", "level_h", "level_w", "quota", "active", "level_offset", "bytes_per_image"):
        assert got[k] == want[k], k
    assert np.array_equal(np.array(got["scale"], np.float32), np.array(want["scale"], np.float32))


@pytest.mark.parametrize("shape", [(96, 128), (97, 131), (129, 129), (200, 264), (62, 62)])
def test_layout_equals_reference(orb, shape):
    want = orb_ref.layout(*shape)
    same_layout(orb.layout(*shape), want)
    assert sum(want["quota"]) == 500
    assert want["active"] == [int(min(h, w) > 62) for h, w in zip(want["level_h"], want["level_w"])]


def test_layout_at_a_half_and_with_options(orb):
    H, l = half_shape()
    print("H = %d: H / scale_%d = %.9f" % (H, l, H / np.float64(np.float32(1.2 ** l))))
    want = orb_ref.layout(H, H + 3, dict(nlevels=l + 1))
    same_layout(orb.layout(H, H + 3, orb.options(nlevels=l + 1)), want)
    assert want["level_h"][l] == 7                          # 7.4999997: float32(1.2) lies above 1.2, so this is no tie
    for nf, sf, nl in ((24, 1.2, 8), (1000, 1.1, 12), (7, 1.5, 3), (500, 1.9, 4), (500, 1.2, 1)):
        want = orb_ref.layout(300, 413, dict(nfeatures=nf, scale_factor=sf, nlevels=nl))
        same_layout(orb.layout(300, 413, orb.options(nfeatures=nf, scale_factor=sf, nlevels=nl)), want)
        assert sum(want["quota"]) == nf


def test_layout_errors(orb):
    from reconstructor_amd import _lib
    bad = [dict(nlevels=0), dict(nlevels=17), dict(nfeatures=0), dict(edge_threshold=21), dict(fast_threshold=0), dict(fast_threshold=255),
           dict(scale_factor=1.0), dict(scale_factor=4.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            orb_ref.layout(96, 128, kw)
        with pytest.raises(_lib.RcnError) as e:
            orb.layout(96, 128, orb.options(**kw))
        assert e.value.code == -1
    for shape in ((0, 5), (1, 1), (2, 2), (70000, 5)):        # empty, an empty level, a level that halves its predecessor, too long
        with pytest.raises(ValueError):
            orb_ref.layout(*shape)
        with pytest.raises(_lib.RcnError):
            orb.layout(*shape)
    with pytest.raises(ValueError):                          # a factor of 2 halves a level: cv::resize takes its area branch there
        orb_ref.layout(300, 412, dict(scale_factor=2.0))
    with pytest.raises(_lib.RcnError):
        orb.layout(300, 412, orb.options(scale_factor=2.0))
    pat = orb_ref.default_pattern()
    pat[517] = 16
    with pytest.raises(ValueError):
        orb_ref.check_pattern(pat)
    with pytest.raises(_lib.RcnError):
        orb.layout(96, 128, orb.options(pattern=pat))
    assert _lib.load().rcn_orb_layout(96, 128, None, None) == -1


def brute_force_score(img, y, x, thr):
    p = int(img[y, x])
    c = [int(img[y + dy, x + dx]) for dx, dy in orb_ref.CIRCLE]
    best = 0
    for t in range(thr, 256):
        ok = any(all(c[(s + k) % 16] > p + t for k in range(9)) or all(c[(s + k) % 16] < p - t for k in range(9)) for s in range(16))
        if not ok:
            break
        best = t
    return best


def test_fast_score_equals_a_sweep_over_t():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (24, 31), dtype=np.uint8)
    img[8:16, 10:20] = (img[8:16, 10:20] // 8) + 200           # a bright patch: corners with long arcs
    img[2:9, 20:29] = img[2:9, 20:29] // 16
    for thr in (1, 20, 90):
        s = orb_ref.fast_scores(img, thr)
        want = np.zeros_like(s)
        for y in range(3, 21):
            for x in range(3, 28):
                want[y, x] = brute_force_score(img, y, x, thr)
        assert np.array_equal(s, want), thr
        assert (s > 0).sum() > (3 if thr == 90 else 10)
    assert (orb_ref.fast_scores(img, 20)[:3] == 0).all() and (orb_ref.fast_scores(img, 20)[:, -3:] == 0).all()


def arc_image(length, bright):
    img = np.full((80, 80), 100, np.uint8)
    for k in range(length):
        dx, dy = orb_ref.CIRCLE[(5 + k) % 16]
        img[40 + dy, 37 + dx] = 160 if bright else 40
    return img


@pytest.mark.parametrize("bright", [True, False])
def test_planted_corner_and_arc_lengths(bright):
    img = arc_image(9, bright)
    s = orb_ref.fast_scores(img, 20)
    assert s[40, 37] == 59                                    # |160 - 100| - 1 = |40 - 100| - 1
    ys, xs = orb_ref.nms(s, 31)
    assert (40, 37) in set(zip(ys.tolist(), xs.tolist()))
    assert orb_ref.fast_scores(arc_image(8, bright), 20)[40, 37] == 0
    assert orb_ref.fast_scores(arc_image(16, bright), 20)[40, 37] == 59


def test_nms_is_strict():
    s = np.zeros((80, 80), np.uint8)
    s[40, 40] = s[40, 41] = 50                               # two equal neighbours: neither
    s[45, 45], s[46, 46] = 50, 51                            # the larger of two
    s[50, 50] = 30                                           # beyond the edge border of an 80-pixel level: [31, 49)
    s[10, 40] = 99                                           # inside FAST's border, outside the edge border
    s[31, 31] = s[48, 48] = 7                                # the first pixel inside the edge border; the last
    s[48, 49] = 0
    ys, xs = orb_ref.nms(s, 31)
    assert sorted(zip(ys.tolist(), xs.tolist())) == [(31, 31), (46, 46), (48, 48)]
    assert len(orb_ref.nms(np.full((62, 90), 9, np.uint8), 31)[0]) == 0


def tie_image(H=160, W=160):
    """a periodic image: every period holds the same corners, so FAST scores and responses tie across the level"""
    cell = np.random.default_rng(21).integers(0, 256, (16, 16), dtype=np.uint8)
    return np.tile(cell, (H // 16, W // 16))


def test_retain_best_keeps_ties():
    img = tie_image()
    r = orb_ref.detect_and_compute(img, 4096, dict(nfeatures=40, nlevels=1))
    # one level, quota 40: the interior holds far more than 40 corners and they tie in classes of equal score and response
    assert r["count"] > 40
    resp = np.sort(r["response64"])[::-1]
    assert resp[39] == resp[-1]                              # everything past the quota ties with the quota-th
    lo = orb_ref.detect_and_compute(img, 4096, dict(nfeatures=r["count"], nlevels=1))
    assert lo["count"] >= r["count"]


def test_quarter_turn_is_exact():
    img = orb_ref.corner_image(128, 128, seed=9, n_rect=50)
    rot = np.rot90(img).copy()                               # pixel (x, y) of img is pixel (y, 127 - x) of rot
    ys = np.array([40, 64, 90]); xs = np.array([50, 64, 33])
    m10, m01 = orb_ref.moments(img, ys, xs)
    r10, r01 = orb_ref.moments(rot, 127 - xs, ys)
    assert np.array_equal(r10, m01) and np.array_equal(r01, -m10)
    a = orb_ref.detect_and_compute(img, 2048)
    b = orb_ref.detect_and_compute(rot, 2048)
    ka = {(int(x), int(y)): a["packed"][k] for k, (l, y, x) in enumerate(zip(a["level"], a["y"], a["x"])) if l == 0}
    kb = {(int(x), int(y)): b["packed"][k] for k, (l, y, x) in enumerate(zip(b["level"], b["y"], b["x"])) if l == 0}
    assert len(ka) > 20 and len(ka) == len(kb)
    for (x, y), row in ka.items():
        assert np.array_equal(kb[(y, 127 - x)], row)


def test_default_pattern_table(orb):
    want = orb_ref.default_pattern()
    got = orb.default_pattern()
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert np.abs(want.astype(np.int32)).max() <= 13
    t = want.reshape(256, 4)
    assert not ((t[:, 0] == t[:, 2]) & (t[:, 1] == t[:, 3])).any()
    assert 4.5 < t.astype(np.float64).std() < 7.0            # sigma 31 / 5, a little less after the clip


def test_blur_weights_and_umax():
    assert orb_ref.BLUR_W == [18, 34, 49, 54, 49, 34, 18] and sum(orb_ref.BLUR_W) == 256
    assert orb_ref.UMAX == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    flat = np.full((70, 70), 137, np.uint8)
    assert (orb_ref.blur(flat) == 137).all()                 # weights sum to 256 on both axes: a constant is kept


def test_golden_file_equals_its_generator():
    gen = generator()
    path = os.path.join(ROOT, "tests", "golden", "orb_small.npz")
    g = np.load(path)
    want = gen.make()
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
    assert [g["image%d" % i].shape for i in range(3)] == [(96, 128), (96, 128), (97, 131)]
    assert (g["counts"] < g["candidates"]).all() and g["counts"].min() > 0          # the quota binds
    assert os.path.getsize(path) < 1 << 20
