"""GPU suite: the two-view classification (rcn_twoview_geometry*, k_tv_classify in csrc/homography.hip) -- the E outputs
against rcn_twoview_init and the H outputs against rcn_homography_ransac on the same input, bit for bit; ratio, median angle
and label against tests/homography_ref.py exactly; the classification families; the device entry against the host entry;
argument errors; and the geometry-checked choice of the initial pair with the sessions started from both choices."""
import numpy as np
import pytest

import homography_ref as hr
import nextview_ref as nr
import tri_ref
import twoview_ref as tv
from reconstructor_amd import _lib, ba, homography, nextview, twoview

pytestmark = pytest.mark.gpu
ERR_ARG = -1
E_KEYS = ("E", "pose34", "mask", "cheir_mask", "count", "iterations")
H_KEYS = ("H", "mask", "count", "iterations")
FAR = 1e9           # distance_threshold of the E search for the classification families (see test_homography_ref.py)


def _batch(pairs):
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(p["xy1"]) for p in pairs])
    return (off, np.concatenate([p["xy1"] for p in pairs]), np.concatenate([p["xy2"] for p in pairs]),
            np.stack([p["K1"] for p in pairs]), np.stack([p["K2"] for p in pairs]))


def _far(ctx):
    o = twoview.default_options(ctx)
    o.distance_threshold = FAR
    return o


def _assert_parts(ctx, got, off, xy1, xy2, K1, K2, tv_opt=None, what=""):
    e = twoview.two_view_init(ctx, off, xy1, xy2, K1, K2, tv_opt)
    h = homography.find(ctx, off, xy1, xy2)
    for k in E_KEYS:
        assert np.asarray(got[k]).tobytes() == np.asarray(e[k]).tobytes(), (what, k)
    for k in H_KEYS:
        assert np.asarray(got["H" if k == "H" else "h_" + k]).tobytes() == np.asarray(h[k]).tobytes(), (what, "h_" + k)
    return e, h


def _assert_classified(got, e, h, off, xy1, xy2, K1, K2, what=""):
    """ratio, median_angle and label against the restatement on the kernel's own E and H outputs, exactly."""
    for p in range(len(off) - 1):
        a, b = int(off[p]), int(off[p + 1])
        ratio, angle, label = hr.classify(xy1[a:b], xy2[a:b], K1[p], K2[p], int(e["count"][p, 0]), e["cheir_mask"][a:b], e["pose34"][p],
                                          int(h["count"][p]))
        assert (got["ratio"][p], got["median_angle"][p], got["label"][p]) == (ratio, angle, label), (what, p)


def test_geometry_equals_its_parts_and_the_restatement(gpu_ctx):
    """Scenes of every kind and size in one ragged call: general, planar, pure rotation, too few entries, empty, past the
    counts kept in LDS (2048 entries of the searches, 4096 keys of the classification)."""
    pairs = [tv.scene_pair(1, 0.3), tv.scene_pair(2, 0.0, n=200, planar=True), tv.scene_pair(3, 0.2, n=150, baseline=0.0),
             tv.scene_pair(4, 0.0, n=4), tv.scene_pair(5, 0.0, n=0), tv.scene_pair(6, 0.1, n=4100), tv.scene_pair(7, 0.5, n=2049, baseline=0.1),
             tv.scene_pair(8, 0.1, n=65, distortion=True)]
    off, xy1, xy2, K1, K2 = _batch(pairs)
    for opt in (None, _far(gpu_ctx)):
        got = twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2, tv_options=opt)
        e, h = _assert_parts(gpu_ctx, got, off, xy1, xy2, K1, K2, opt)
        _assert_classified(got, e, h, off, xy1, xy2, K1, K2)
        assert got["label"][3] == got["label"][4] == twoview.NO_MODEL and got["ratio"][4] == 0.0 and got["median_angle"][4] == 0.0
        assert got["label"][0] == got["label"][5] == twoview.GENERAL and got["label"][1] == twoview.PLANAR
    assert got["label"][2] == twoview.PANORAMIC


@pytest.mark.parametrize("family", range(6))
def test_classification_families(gpu_ctx, family):
    """The families of tests/test_homography_ref.py (same seeds, same E-search options) get their labels on the GPU, and the outputs equal the restatement."""
    name, kw, label = hr.classification_families()[family]
    pairs = [tv.scene_pair(seed, share, n=200, **kw) for seed in hr.family_seeds(name) for share in (0.0, 0.3)]
    off, xy1, xy2, K1, K2 = _batch(pairs)
    got = twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2, tv_options=_far(gpu_ctx))
    assert got["label"].tolist() == [label] * len(pairs), (name, got["ratio"], got["median_angle"])
    e = dict(count=got["count"], cheir_mask=got["cheir_mask"], pose34=got["pose34"])
    _assert_classified(got, e, dict(count=got["h_count"]), off, xy1, xy2, K1, K2, name)
    want = [hr.geometry(p["xy1"], p["xy2"], p["K1"], p["K2"], tv_opt=dict(distance_threshold=FAR)) for p in pairs[:2]]
    assert [w[4] for w in want] == [label] * 2 and [w[2] for w in want] == got["ratio"][:2].tolist()
    assert [w[3] for w in want] == got["median_angle"][:2].tolist()


def test_options_and_argument_errors(gpu_ctx):
    s = tv.scene_pair(3, 0.0, n=120)
    off, xy1, xy2, K1, K2 = _batch([s])
    o = twoview.geometry_default_options(gpu_ctx)
    assert (o.max_h_ratio, o.min_angle, o.min_inliers, o.top_m) == (0.8, 1.0, 15, 10)
    base = twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2)
    assert base["label"][0] == twoview.GENERAL
    for field, val, label in (("min_inliers", 121, twoview.NO_MODEL), ("min_angle", 90.0, twoview.SMALL_BASELINE), ("max_h_ratio", 1e-3, twoview.PLANAR)):
        o = twoview.geometry_default_options(gpu_ctx)
        setattr(o, field, val)
        assert twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2, o)["label"][0] == label, field
    o.min_angle = 90.0
    assert twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2, o)["label"][0] == twoview.PANORAMIC
    h = homography.default_options(gpu_ctx)
    h.threshold = 0.5
    assert twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2, h_options=h)["h_count"][0] == homography.find(gpu_ctx, off, xy1, xy2, h)["count"][0] != base["h_count"][0]
    bad = []
    for field, val in (("max_h_ratio", 0.0), ("max_h_ratio", -1.0), ("top_m", 0)):
        o = twoview.geometry_default_options(gpu_ctx)
        setattr(o, field, val)
        bad.append(dict(options=o))
    for field, val in (("threshold", 0.0), ("confidence", 1.0), ("max_iterations", 0)):
        h = homography.default_options(gpu_ctx)
        setattr(h, field, val)
        bad.append(dict(h_options=h))
    for field, val in (("threshold", -1.0), ("confidence", 0.0), ("distance_threshold", 0.0), ("max_iterations", 0)):
        t = twoview.default_options(gpu_ctx)
        setattr(t, field, val)
        bad.append(dict(tv_options=t))
    for kw in bad:
        with pytest.raises(_lib.RcnError) as e:
            twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2, **kw)
        assert e.value.code == ERR_ARG and gpu_ctx.lib.rcn_last_error(gpu_ctx.h)
    with pytest.raises(_lib.RcnError) as e:
        twoview.geometry(gpu_ctx, np.array([0, 50, 20], np.int64), xy1, xy2, np.stack([K1[0]] * 2), np.stack([K2[0]] * 2))
    assert e.value.code == ERR_ARG
    lib, hh = gpu_ctx.lib, gpu_ctx.h
    n = len(xy1)
    outs = [np.zeros(9), np.zeros(12), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(9),
            np.zeros(n, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1), np.zeros(1), np.zeros(1, np.int32)]
    ins = [off, xy1, xy2, K1, K2]
    ok = [a.ctypes.data for a in ins] + [None, None, None] + [a.ctypes.data for a in outs]
    assert lib.rcn_twoview_geometry(hh, 1, *ok) == _lib.RCN_OK and outs[12][0] == twoview.GENERAL
    for k in (0, 1, 2, 3, 4, 9, 10, 12, 14, 15, 16, 18, 19, 20):      # inputs; pose, mask, count; H, h_mask, h_count, ratio, angle, label
        a = list(ok)
        a[k] = None
        assert lib.rcn_twoview_geometry(hh, 1, *a) == ERR_ARG, k
    assert lib.rcn_twoview_geometry(hh, -1, *ok) == ERR_ARG and lib.rcn_twoview_geometry(None, 1, *ok) == ERR_ARG
    assert twoview.geometry(gpu_ctx, off, xy1, xy2, K1, K2)["label"][0] == twoview.GENERAL       # the ctx is still usable


NOT_RESIDENT = (7, 9)


def test_device_entry_equals_host_entry(gpu_ctx):
    """rcn_twoview_geometry_device behind the resident lists and coordinates against the host entry: a stored orientation, a
    mirrored pair, a pair without a list, a pair beyond `capacity`; guard words behind every output; one synchronisation."""
    import torch
    ctx = gpu_ctx
    dev = torch.device("cuda", ctx.device)
    L = tri_ref.loop_containers(25, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    for i, xy in L["coords"].items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))
    nextview.upload_feature_matches(ctx, {k: v for k, v in nr.canonical_lists(L["feature_matches"]).items() if k != NOT_RESIDENT}, mirror=True)
    try:
        def entries(i, j):
            qt = sorted(L["feature_matches"][(i, j)].items())
            return (np.array(qt, np.int32).reshape(-1, 2), np.array([L["coords"][i][f] for f, _ in qt], np.int32).reshape(-1, 2),
                    np.array([L["coords"][j][g] for _, g in qt], np.int32).reshape(-1, 2))
        pairs = [(20, 22), (22, 20), NOT_RESIDENT[::-1], (0, 1)]
        ents = [entries(i, j) if (i, j) != NOT_RESIDENT[::-1] else (np.zeros((0, 2), np.int32),) * 3 for i, j in pairs]
        K1 = np.stack([L["intrinsics"][i] for i, _ in pairs]).astype(np.float64)
        K2 = np.stack([L["intrinsics"][j] for _, j in pairs]).astype(np.float64)
        off = np.concatenate([[0], np.cumsum([len(e[0]) for e in ents])]).astype(np.int64)
        want = twoview.geometry(ctx, off, np.concatenate([e[1] for e in ents]), np.concatenate([e[2] for e in ents]), K1, K2)
        assert (want["count"][[0, 1, 3], 0] > 50).all() and want["label"][2] == twoview.NO_MODEL
        K1d, K2d = (torch.as_tensor(a).to(dev) for a in (K1, K2))
        total, n = int(off[-1]), len(pairs)
        pr = np.ascontiguousarray(pairs, np.int32)
        shapes = dict(E=(9 * n, torch.float64), pose34=(12 * n, torch.float64), mask=(None, torch.uint8), cheir_mask=(None, torch.uint8),
                      count=(2 * n, torch.int32), iterations=(n, torch.int32), H=(9 * n, torch.float64), h_mask=(None, torch.uint8),
                      h_count=(n, torch.int32), h_iterations=(n, torch.int32), ratio=(n, torch.float64), median_angle=(n, torch.float64),
                      label=(n, torch.int32))

        def run(cap):
            size = {k: (cap if s is None else s) for k, (s, _) in shapes.items()}
            bufs = {k: torch.full((size[k] + 8,), 77, dtype=dt, device=dev) for k, (_, dt) in shapes.items()}
            offd = torch.full((n + 1 + 4,), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            ctx.check(ctx.lib.rcn_twoview_geometry_device(ctx.h, n, pr.ctypes.data, K1d.data_ptr(), K2d.data_ptr(), None, None, None, cap,
                                                          offd.data_ptr(), None, *[bufs[k].data_ptr() for k in shapes]))
            ctx.check(ctx.lib.rcn_synchronize(ctx.h))
            out = {k: v.cpu().numpy() for k, v in bufs.items()}
            for k in shapes:
                assert (out[k][size[k]:] == 77).all(), (cap, k)
            o = offd.cpu().numpy()
            assert (o[n + 1:] == -7).all()
            return o[:n + 1], out

        for cap in (total, total + 50):
            o, got = run(cap)
            assert o.tolist() == off.tolist()
            for k, (s, _) in shapes.items():
                m = total if s is None else s
                assert got[k][:m].tobytes() == np.asarray(want[k]).tobytes(), (cap, k)
        o, got = run(total - 1)                                       # no room for the last pair
        assert o.tolist() == off[:-1].tolist() + [int(off[-2])]
        assert got["count"][2 * (n - 1):2 * n].tolist() == [-2, 0] and got["h_count"][n - 1] == -2 and got["label"][n - 1] == twoview.NO_MODEL
        assert got["label"][:n - 1].tolist() == want["label"][:n - 1].tolist() and got["median_angle"][:n - 1].tobytes() == want["median_angle"][:n - 1].tobytes()
        r = twoview.geometry_device(ctx, pairs, K1d, K2d, total)
        ctx.check(ctx.lib.rcn_synchronize(ctx.h))
        assert r["label"].cpu().numpy().tolist() == want["label"].tolist() and r["qt"].cpu().numpy()[:total].tobytes() == np.concatenate([e[0] for e in ents]).tobytes()
    finally:
        ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))


def test_the_pair_choice(gpu_ctx):
    """A match graph of six images: the pair with the most matches is a pure rotation, the second a tiny baseline, the third
    general.  The canonical choice takes the first; the geometry-checked one the third; a session started from the third
    triangulates the pair's correct matches, one started from the first next to nothing."""
    ctx = gpu_ctx
    scenes = {(0, 1): tv.scene_pair(31, 0.1, n=300, baseline=0.0), (2, 3): tv.scene_pair(32, 0.1, n=280, baseline=0.02),
              (4, 5): tv.scene_pair(33, 0.1, n=260), (0, 2): tv.scene_pair(34, 0.1, n=90), (1, 5): tv.scene_pair(35, 0.1, n=40),
              (3, 4): tv.scene_pair(36, 0.0, n=12)}
    keys = sorted(scenes, key=lambda k: (k[1], k[0]))                # not in the order of the sizes
    off, xy1, xy2, K1, K2 = _batch([scenes[k] for k in keys])
    pairs = np.array(keys, np.int32)
    i, j, k = twoview.choose_initial_pair(pairs, off)
    assert (i, j) == (0, 1) == tuple(tv.choose_initial_pair(pairs, off)[:2])          # unchanged
    got = twoview.choose_initial_pair_by_geometry(ctx, pairs, off, xy1, xy2, K1, K2)
    assert got["pair"] == (4, 5) and got["position"] == 2 and not got["fallback"]
    assert [tuple(pairs[c]) for c in got["candidates"][:3]] == [(0, 1), (2, 3), (4, 5)] and len(got["candidates"]) == 6
    assert got["table"]["label"][2] == twoview.GENERAL and all(v in (twoview.NO_MODEL, twoview.PANORAMIC) for v in got["table"]["label"][:2])
    labels = [hr.geometry(scenes[tuple(pairs[c])]["xy1"], scenes[tuple(pairs[c])]["xy2"], K1[c], K2[c])[4] for c in got["candidates"]]
    assert got["table"]["label"].tolist() == labels
    assert hr.choose_initial_pair_by_geometry(pairs, off, labels)[1:] == (2, False)
    o = twoview.geometry_default_options(ctx)
    o.top_m = 2
    fb = twoview.choose_initial_pair_by_geometry(ctx, pairs, off, xy1, xy2, K1, K2, o)
    assert fb["pair"] == (0, 1) and fb["fallback"] and fb["position"] == 0 and len(fb["candidates"]) == 2
    assert hr.choose_initial_pair_by_geometry(pairs, off, labels[:2], top_m=2)[1:] == (0, True)
    added = {}
    for name, pick in (("geometry", got["pair"]), ("canonical", (i, j))):
        s = scenes[pick]
        ses = ba.BaSession(ctx)
        try:
            r = ses.init_pair(s["xy1"], s["xy2"], s["K1"], s["K2"])
            added[name] = (int(r["added"]), int((~s["wrong"]).sum()))
        finally:
            ses.close()
    assert added["geometry"][0] >= 0.8 * added["geometry"][1], added
    assert added["canonical"][0] < o.min_inliers, added
    e = twoview.two_view_init(ctx, [0, 260], scenes[(4, 5)]["xy1"], scenes[(4, 5)]["xy2"], scenes[(4, 5)]["K1"], scenes[(4, 5)]["K2"])
    assert got["pose34"].tobytes() == e["pose34"][0].tobytes() and got["count"].tolist() == e["count"][0].tolist()
