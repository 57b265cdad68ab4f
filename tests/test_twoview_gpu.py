"""GPU suite: two-view initialisation (rcn_twoview_init*, rcn_ba_session_init_pair; csrc/twoview.hip) against
tests/twoview_ref.py bit for bit -- E, pose, both masks, counts, iterations; a batch against its pairs one at a time; the
device entry against the host entry; the session entry against its parts; argument errors and malformed device data; and
the reference's incremental loop started from nothing but match lists, pixel coordinates and intrinsics."""
import os

import numpy as np
import pytest

import nextview_ref as nr
import pnp_ref
import tri_ref
import twoview_ref as tv
from reconstructor_amd import _lib, ba, nextview, pnp, twoview
from reconstructor_amd import triangulate as tri

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twoview_small.npz")
ERR_ARG = -1
KEYS = ("E", "pose34", "mask", "cheir_mask", "count", "iterations")


def _batch(pairs):
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in pairs])
    xy1 = np.concatenate([np.asarray(p[0], np.int32).reshape(-1, 2) for p in pairs])
    xy2 = np.concatenate([np.asarray(p[1], np.int32).reshape(-1, 2) for p in pairs])
    return off, xy1, xy2, np.stack([p[2] for p in pairs]).astype(np.float64), np.stack([p[3] for p in pairs]).astype(np.float64)


def _assert_same(got, want, what):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("count", "iterations"):
            assert g.tolist() == w.tolist(), (what, k, g, w)
        else:
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, k)


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("share", (0.0, 0.3, 0.6))
def test_scenes_equal_the_restatement_bit_for_bit(gpu_ctx, seed, share):
    """B1 on the scenes of A2 / A3."""
    s = tv.scene_pair(seed, share)
    off, xy1, xy2, K1, K2 = _batch([(s["xy1"], s["xy2"], s["K1"], s["K2"])])
    got = twoview.two_view_init(gpu_ctx, off, xy1, xy2, K1, K2)
    _assert_same(got, tv.two_view_init_batch(off, xy1, xy2, K1, K2), (seed, share))
    assert got["count"][0, 0] >= 0.7 * int((~s["wrong"]).sum())


def test_edge_cases_equal_the_restatement_bit_for_bit(gpu_ctx):
    """B1 on the edge cases of A4, all of them in one call."""
    cases = tv.edge_cases()
    off, xy1, xy2, K1, K2 = _batch([c[1:] for c in cases])
    got = twoview.two_view_init(gpu_ctx, off, xy1, xy2, K1, K2)
    _assert_same(got, tv.two_view_init_batch(off, xy1, xy2, K1, K2), [c[0] for c in cases])
    assert not np.isnan(got["pose34"]).any() and not np.isnan(got["E"]).any()


def test_golden(gpu_ctx):
    with np.load(GOLD) as g:
        got = twoview.two_view_init(gpu_ctx, g["off"], g["xy1"], g["xy2"], g["intr6_1"], g["intr6_2"])
        _assert_same(got, {k: g[k] for k in KEYS}, "golden")


def _ragged(seed=7):
    """24 pairs, n from 0 to 5000: both the LDS and the workspace path, some empty, some < 5."""
    rng = np.random.default_rng(seed)
    sizes = [0, 4, 5000, 2048, 2049, 5, 0, 3, 6] + [int(s) for s in rng.integers(10, 900, 15)]
    return [(lambda s: (s["xy1"], s["xy2"], s["K1"], s["K2"]))(tv.scene_pair(100 + k, 0.1 * (k % 6), n=n, distortion=k % 4 == 3))
            for k, n in enumerate(sizes)]


def test_batch_equals_single_calls(gpu_ctx):
    """B2."""
    pairs = _ragged()
    off, xy1, xy2, K1, K2 = _batch(pairs)
    got = twoview.two_view_init(gpu_ctx, off, xy1, xy2, K1, K2)
    assert (got["count"][:, 0] == -2).sum() == 4 and (got["count"][:, 0] > 0).sum() >= 18
    for p, (a, b, k1, k2) in enumerate(pairs):
        one = twoview.two_view_init(gpu_ctx, [0, len(a)], a, b, k1, k2)
        lo, hi = int(off[p]), int(off[p + 1])
        assert got["mask"][lo:hi].tobytes() == one["mask"].tobytes() and got["cheir_mask"][lo:hi].tobytes() == one["cheir_mask"].tobytes()
        for key in ("E", "pose34", "count", "iterations"):
            assert got[key][p].tobytes() == one[key][0].tobytes(), (p, key)
    # the workspace path against the restatement as well (n > 2048)
    for p in (2, 4):
        a, b, k1, k2 = pairs[p]
        r = tv.two_view_init(a, b, k1, k2)
        assert r["count"] == got["count"][p, 0] and r["cheir_count"] == got["count"][p, 1] and r["iterations"] == got["iterations"][p]
        assert r["pose34"].tobytes() == got["pose34"][p].tobytes() and r["E"].tobytes() == got["E"][p].tobytes()
        assert np.array_equal(r["mask"], got["mask"][off[p]:off[p + 1]]) and np.array_equal(r["cheir_mask"], got["cheir_mask"][off[p]:off[p + 1]])


def test_options_reach_the_kernel(gpu_ctx):
    s = tv.scene_pair(3, 0.4, n=250)
    off, xy1, xy2, K1, K2 = _batch([(s["xy1"], s["xy2"], s["K1"], s["K2"])])
    o = twoview.default_options(gpu_ctx)
    assert (o.threshold, o.confidence, o.distance_threshold, o.max_iterations) == (1.0, 0.999, 50.0, 1000)
    o.threshold, o.confidence, o.distance_threshold, o.max_iterations = 2.5, 0.95, 6.0, 40
    got = twoview.two_view_init(gpu_ctx, off, xy1, xy2, K1, K2, o)
    want = tv.two_view_init_batch(off, xy1, xy2, K1, K2, dict(threshold=2.5, confidence=0.95, distance_threshold=6.0, max_iterations=40))
    _assert_same(got, want, "options")
    assert 0 < got["count"][0, 1] < got["count"][0, 0]          # the distance threshold cuts the far points


def test_argument_errors(gpu_ctx):
    """B4: the conventions of tests/test_api_errors_gpu.py -- RCN_ERR_ARG, a message, and a ctx that still works."""
    s = tv.scene_pair(3, 0.0, n=120)
    xy1, xy2, K1, K2 = s["xy1"], s["xy2"], s["K1"], s["K2"]
    off = np.array([0, len(xy1)], np.int64)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    E, pose, mask, cm, cnt, it = np.zeros(9), np.zeros(12), np.zeros(len(xy1), np.uint8), np.zeros(len(xy1), np.uint8), np.zeros(2, np.int32), np.zeros(1, np.int32)

    def call(off=off, xy1=xy1, xy2=xy2, K1=K1, K2=K2, opt=None, E=E, pose=pose, mask=mask, cm=cm, cnt=cnt, it=it, npairs=1):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.rcn_twoview_init(h, npairs, p(off), p(xy1), p(xy2), p(K1), p(K2), opt, p(E), p(pose), p(mask), p(cm), p(cnt), p(it))

    assert call() == _lib.RCN_OK and cnt[0] > 60
    assert call(E=None, cm=None, it=None) == _lib.RCN_OK            # the optional outputs
    for kw in (dict(off=None), dict(xy1=None), dict(xy2=None), dict(K1=None), dict(K2=None), dict(pose=None), dict(mask=None), dict(cnt=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(npairs=-1) == ERR_ARG
    assert call(off=np.array([0, 10, 5], np.int64), K1=np.stack([K1, K1]), K2=np.stack([K2, K2]), npairs=2) == ERR_ARG
    assert call(off=np.array([1, len(xy1)], np.int64)) == ERR_ARG
    for field, val in (("confidence", 0.0), ("confidence", 1.0), ("threshold", 0.0), ("threshold", -1.0), ("distance_threshold", 0.0),
                       ("max_iterations", 0)):
        o = twoview.default_options(gpu_ctx)
        setattr(o, field, val)
        assert call(opt=o) == ERR_ARG, field
        assert lib.rcn_last_error(h)
    assert lib.rcn_twoview_init(None, 1, off.ctypes.data, None, None, None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert call() == _lib.RCN_OK                                    # the ctx is still usable
    ses = ba.BaSession(gpu_ctx)
    try:
        p = lambda a: a.ctypes.data
        ci = cnt.ctypes.data
        args = (None, 4.0, 1.0, None, None, None, None, ci, None, None, None)
        assert lib.rcn_ba_session_init_pair(ses.h, len(xy1), None, p(xy2), p(K1), p(K2), *args) == ERR_ARG
        assert lib.rcn_ba_session_init_pair(ses.h, len(xy1), p(xy1), p(xy2), None, p(K2), *args) == ERR_ARG
        assert lib.rcn_ba_session_init_pair(ses.h, -1, p(xy1), p(xy2), p(K1), p(K2), *args) == ERR_ARG
        assert lib.rcn_ba_session_init_pair(ses.h, len(xy1), p(xy1), p(xy2), p(K1), p(K2), None, 4.0, 1.0, None, None, None, None, None, None, None, None) == ERR_ARG
        assert ses.counts() == (0, 0, 0)
        r = ses.init_pair(xy1[:4], xy2[:4], K1, K2)                 # too few entries: no pose, the session stays empty
        assert r["count"].tolist() == [-2, 0] and ses.counts() == (0, 0, 0)
        r = ses.init_pair(xy1, xy2, K1, K2)
        assert r["count"][0] > 60 and ses.counts()[0] == 2 and ses.counts()[1] == r["added"] > 60
        with pytest.raises(_lib.RcnError):                          # not empty any more
            ses.init_pair(xy1, xy2, K1, K2)
    finally:
        ses.close()


def _upload_coords(ctx, coords):
    for i, xy in coords.items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))


NOT_RESIDENT = (7, 9)         # a pair of the scene whose list is left out of the upload (in both directions)


def _resident(ctx, L):
    """The loop scene's coordinates and canonical i < j lists resident in the ctx (mirror on), one pair left out."""
    _upload_coords(ctx, L["coords"])
    lists = {k: v for k, v in nr.canonical_lists(L["feature_matches"]).items() if k != NOT_RESIDENT}
    nextview.upload_feature_matches(ctx, lists, mirror=True)


def _host_entries(L, i, j):
    qt = sorted(L["feature_matches"][(i, j)].items())
    return (np.array(qt, np.int32).reshape(-1, 2), np.array([L["coords"][i][f] for f, _ in qt], np.int32).reshape(-1, 2),
            np.array([L["coords"][j][g] for _, g in qt], np.int32).reshape(-1, 2))


def test_device_entry_equals_host_entry(gpu_ctx):
    """B3a: rcn_twoview_init_device behind rcn_match_lists_upload and rcn_coords_upload against the host entry on the same
    pairs -- a stored orientation (i < j), mirrored ones (j, i), a pair without a list -- enqueued, one rcn_synchronize."""
    import torch
    ctx = gpu_ctx
    dev = torch.device("cuda", ctx.device)
    L = tri_ref.loop_containers(25, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    fm = L["feature_matches"]
    _resident(ctx, L)
    try:
        assert NOT_RESIDENT in fm
        pairs = [(20, 22), (22, 20), (0, 1), (5, 3), NOT_RESIDENT[::-1], (1, 0)]
        ents = [_host_entries(L, i, j) if (i, j) != NOT_RESIDENT[::-1] else (np.zeros((0, 2), np.int32),) * 3 for i, j in pairs]
        K1 = np.stack([L["intrinsics"][i] for i, _ in pairs]).astype(np.float64)
        K2 = np.stack([L["intrinsics"][j] for _, j in pairs]).astype(np.float64)
        off = np.concatenate([[0], np.cumsum([len(e[0]) for e in ents])]).astype(np.int64)
        want = twoview.two_view_init(ctx, off, np.concatenate([e[1] for e in ents]), np.concatenate([e[2] for e in ents]), K1, K2)
        assert (want["count"][:, 0] > 50).sum() == 5 and want["count"][4, 0] == -2
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(dev)
        K1d, K2d = t(K1), t(K2)
        torch.cuda.synchronize(dev)
        total = int(off[-1])
        for cap in (total, total + 100):
            got = twoview.two_view_init_device(ctx, pairs, K1d, K2d, cap)
            ctx.check(ctx.lib.rcn_synchronize(ctx.h))
            assert got["off"].cpu().numpy().tolist() == off.tolist()
            assert got["qt"].cpu().numpy()[:total].tobytes() == np.concatenate([e[0] for e in ents]).tobytes()
            for k in KEYS:
                g = got[k].cpu().numpy()
                g = g[:total] if k in ("mask", "cheir_mask") else g
                assert g.tobytes() == want[k].tobytes(), (cap, k)
        # no room for the last pair: it gets no entries and count -2, the others are untouched
        got = twoview.two_view_init_device(ctx, pairs, K1d, K2d, total - 1, want_qt=False)
        ctx.check(ctx.lib.rcn_synchronize(ctx.h))
        o = got["off"].cpu().numpy()
        assert o.tolist() == off[:-1].tolist() + [int(off[-2])] and got["count"].cpu().numpy()[5].tolist() == [-2, 0]
        assert got["pose34"].cpu().numpy()[:5].tobytes() == want["pose34"][:5].tobytes() and not got["pose34"].cpu().numpy()[5].any()
    finally:
        ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))


def test_device_entry_errors_and_malformed_data(gpu_ctx):
    """B4, device entry: an unknown image id, no resident lists, a pair (a, a), null pointers return codes; a pair that is not
    resident gives count -2; features outside the coordinates (the coordinates replaced by a shorter array after the lists
    went up) are ignored.  Nothing faults, and the ctx still works."""
    import torch
    ctx = gpu_ctx
    dev = torch.device("cuda", ctx.device)
    L = tri_ref.loop_containers(25, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    K = torch.as_tensor(np.stack([L["intrinsics"][20], L["intrinsics"][22]]).astype(np.float64)).to(dev)
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))
    with pytest.raises(_lib.RcnError) as e:                      # no lists
        twoview.two_view_init_device(ctx, [(20, 22)], K[:1], K[1:], 500)
    assert e.value.code == ERR_ARG
    _resident(ctx, L)
    try:
        for pairs, code in (([(20, 99)], -5), ([(-3, 22)], -5), ([(20, 20)], ERR_ARG)):
            with pytest.raises(_lib.RcnError) as e:
                twoview.two_view_init_device(ctx, pairs, K[:1], K[1:], 500)
            assert e.value.code == code, pairs
        lib, h = ctx.lib, ctx.h
        pr = np.array([[20, 22]], np.int32)
        off = torch.zeros(2, dtype=torch.int64, device=dev)
        pose, cnt = torch.zeros(12, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        mask = torch.zeros(500, dtype=torch.uint8, device=dev)
        ok = (h, 1, pr.ctypes.data, K[:1].data_ptr(), K[1:].data_ptr(), None, 500, off.data_ptr(), None, None, pose.data_ptr(), mask.data_ptr(), None,
              cnt.data_ptr(), None)
        for k in (2, 3, 4, 7, 10, 11, 13):                         # pairs, intrinsics, off, pose, mask, count
            bad = list(ok)
            bad[k] = None
            assert lib.rcn_twoview_init_device(*bad) == ERR_ARG, k
        assert lib.rcn_twoview_init_device(*(list(ok[:6]) + [-1] + list(ok[7:]))) == ERR_ARG
        assert lib.rcn_twoview_init_device(*ok) == _lib.RCN_OK       # optional outputs left out
        ctx.check(lib.rcn_synchronize(h))
        _, xy1, xy2 = _host_entries(L, 20, 22)
        want = twoview.two_view_init(ctx, [0, len(xy1)], xy1, xy2, L["intrinsics"][20], L["intrinsics"][22])
        assert cnt.cpu().numpy().tolist() == want["count"][0].tolist() and pose.cpu().numpy().tobytes() == want["pose34"].tobytes()
        # malformed: image 22's coordinates replaced by their first 40 rows; list entries that name later features are ignored
        short = {22: np.asarray(L["coords"][22], np.int32).reshape(-1, 2)[:40]}
        _upload_coords(ctx, short)
        Ka, Kb = K[[0, 1]].contiguous(), K[[1, 0]].contiguous()
        torch.cuda.synchronize(dev)
        got = twoview.two_view_init_device(ctx, [(20, 22), (22, 20)], Ka, Kb, 600)
        ctx.check(lib.rcn_synchronize(h))
        qt, xy1, xy2 = _host_entries(L, 20, 22)
        keep = qt[:, 1] < 40
        o = got["off"].cpu().numpy()
        assert o.tolist() == [0, int(keep.sum()), 2 * int(keep.sum())] and got["qt"].cpu().numpy()[:o[1]].tobytes() == qt[keep].tobytes()
        w = twoview.two_view_init(ctx, [0, int(keep.sum())], xy1[keep], xy2[keep], L["intrinsics"][20], L["intrinsics"][22])
        assert got["count"].cpu().numpy()[0].tolist() == w["count"][0].tolist() and got["mask"].cpu().numpy()[:o[1]].tobytes() == w["mask"].tobytes()
        assert lib.rcn_twoview_init_device(*ok) == _lib.RCN_OK       # the ctx is still usable
        ctx.check(lib.rcn_synchronize(h))
    finally:
        ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))


def _pair_tracks(n):
    off = 2 * np.arange(n + 1, dtype=np.int32)
    cam = np.tile(np.array([0, 1], np.int32), n)
    return off, cam


def test_session_init_pair_equals_its_parts(gpu_ctx):
    """B3: BaSession.init_pair against two_view_init + add_camera twice + triangulate on the same tracks, bit for bit."""
    for seed, share in ((1, 0.3), (4, 0.0)):
        s = tv.scene_pair(seed, share, n=400)
        xy1, xy2, K1, K2 = s["xy1"], s["xy2"], s["K1"], s["K2"]
        a, b = ba.BaSession(gpu_ctx), ba.BaSession(gpu_ctx)
        try:
            got = a.init_pair(xy1, xy2, K1, K2)
            r = twoview.two_view_init(gpu_ctx, [0, len(xy1)], xy1, xy2, K1, K2)
            for k in KEYS:
                assert np.asarray(got[k]).tobytes() == np.asarray(r[k]).reshape(np.asarray(got[k]).shape).tobytes(), k
            b.add_camera(np.zeros(6), K1)
            b.add_camera(twoview.pose6_from_pose34(gpu_ctx, r["pose34"][0]), K2)
            off, cam = _pair_tracks(len(xy1))
            P = np.stack([np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), r["pose34"][0]])
            st, first, added = b.triangulate(off, cam, np.stack([xy1, xy2], 1).reshape(-1, 2), poses34=P)
            assert first == 0 and added == got["added"] > 0.5 * r["count"][0, 0] and st.tobytes() == got["status"].tobytes()
            assert a.counts() == b.counts() and a.points().tobytes() == b.points().tobytes()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.graph(), b.graph()))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.cameras(), b.cameras()))
            # every match is triangulated, not the inliers only: outliers are rejected by the triangulation's own tests
            assert len(st) == len(xy1) and (not s["wrong"].any() or (st[s["wrong"]] != 0).mean() > 0.9)
            # the stored camera is the recovered pose (angle-axis round trip)
            back = ba.poses34_from_angle_axis(a.cameras()[0])
            assert np.abs(back[1] - r["pose34"][0]).max() <= 1e-5 and not back[0][[3, 7, 11]].any()
        finally:
            a.close()
            b.close()


class _Loop:
    """_Loop of tests/test_pnp_gpu.py (use_pnp=True: every later view's pose is BaSession.pnp's on the candidate's own 2D-3D
    list), restated here; from_nothing=True replaces start(): choose_initial_pair over the match lists, init_pair on the
    pair's entries, and no scene pose anywhere."""

    def __init__(self, ctx, from_nothing):
        self.ctx, self.from_nothing, self.n = ctx, from_nothing, 25
        self.L = tri_ref.loop_containers(self.n, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
        L = self.L
        self.co, self.ids, self.fm, self.im = L["coords"], L["landmark_ids"], L["feature_matches"], L["img_matches"]
        self.shape = {i: nr.SHAPE for i in range(self.n)}
        _upload_coords(ctx, self.co)
        nextview.upload_feature_matches(ctx, nr.canonical_lists(self.fm), mirror=True)
        self.ses = ba.BaSession(ctx)
        self.lms, self.cam_of, self.chosen, self.log = [], {}, [], []

    def poses34(self):
        return ba.poses34_from_angle_axis(self.ses.cameras()[0])

    def add_tracks(self, tracks):
        off, cam, xy = tri.tracks_to_arrays(tracks, self.cam_of, self.co)
        st, first, added = self.ses.triangulate(off, cam, xy, poses34=self.poses34())
        self._adopt(tracks, st, first)

    def _adopt(self, tracks, st, first):
        for k, j in enumerate(np.flatnonzero(st == 0)):
            for i, f in tracks[j]:
                self.ids[i][f] = first + k
            self.lms.append({"track": list(tracks[j])})

    def sync_mirror(self, strict=False):
        pt, cam, xy = self.ses.graph()
        for j, lm in enumerate(self.lms):
            mine = [(c, x, y) for c, (x, y) in zip(cam[pt == j], xy[pt == j])]
            kept, q = [], 0
            for i, f in lm["track"]:
                if q < len(mine) and mine[q] == (self.cam_of[i], *self.co[i][f]):
                    kept.append((i, f)); q += 1
            assert q == len(mine) and (not strict or len(kept) == len(lm["track"]))
            lm["track"] = kept

    def start(self):
        L = self.L
        if not self.from_nothing:
            for v in (0, 1):
                self.cam_of[v] = self.ses.add_camera(L["poses6"][v], L["intrinsics"][v])
            self.add_tracks(tri.initial_pair_tracks(self.fm[(0, 1)], 0, 1))
            self.registered = [(1, True), (0, True)]
            self.first = (0, 1)
            return
        keys = sorted(self.fm)
        off = np.concatenate([[0], np.cumsum([len(self.fm[k]) for k in keys])])
        i, j, _ = twoview.choose_initial_pair(keys, off)
        assert (i, j) == tv.choose_initial_pair(keys, off)[:2] == (20, 22)
        qt = sorted(self.fm[(i, j)].items())                     # ascending query feature
        xy1 = np.array([self.co[i][f] for f, _ in qt], np.int32)
        xy2 = np.array([self.co[j][g] for _, g in qt], np.int32)
        K1, K2 = L["intrinsics"][i], L["intrinsics"][j]
        r = self.ses.init_pair(xy1, xy2, K1, K2)
        want = tv.two_view_init(xy1, xy2, K1, K2)                # the host run
        assert r["count"].tolist() == [want["count"], want["cheir_count"]] and r["iterations"][0] == want["iterations"]
        for k in ("E", "pose34", "mask", "cheir_mask"):
            assert r[k].tobytes() == want[k].tobytes(), k
        assert r["count"][0] >= 0, "no pose for the initial pair"
        self.cam_of[i], self.cam_of[j] = 0, 1
        tracks = [[(i, f), (j, g)] for f, g in qt]
        P = np.stack([np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), want["pose34"]])
        Ks = np.stack([K1, K2]).astype(np.float64)
        toff, tcam = _pair_tracks(len(qt))
        ref = tri_ref.canonical_tracks(P, Ks, toff, tcam, np.stack([xy1, xy2], 1).reshape(-1, 2))      # the host run
        assert r["status"].tolist() == list(ref[1]) and self.ses.points().tobytes() == np.asarray(ref[0])[np.asarray(ref[1]) == 0].tobytes()
        self._adopt(tracks, r["status"], 0)
        self.registered = [(j, True), (i, True)]
        self.first = (i, j)
        self.log.append(("pair", i, j, len(qt), int(r["count"][0]), int(r["count"][1]), int(r["iterations"][0]), r["added"]))

    def candidates(self):
        cand = [i for i in range(self.n) if i not in self.cam_of]
        return cand, [lm["track"] for lm in self.lms]

    def step(self):
        """One view; False when no candidate qualifies."""
        L, co, ids, fm, im, ses = self.L, self.co, self.ids, self.fm, self.im, self.ses
        cand, tracks = self.candidates()
        coff, lmk, ftr, cells, _ = nextview.corr_2d3d(self.ctx, *nextview.graph_arrays(tracks), cand, [self.shape[c] for c in cand])
        order = nextview.rank_next_images(cand, np.diff(coff), cells, nextview.MATCH_DENSITY, 30)
        lids, fids = nr.literal_calc_2d3d_matches(cand, im, fm, ids, tracks)                      # the host run
        sc = [nr.literal_density(fids[c], co[c], self.shape[c]) for c in cand]
        assert sc == cells.tolist()
        assert order == nextview.rank_next_images(cand, [len(lids[c]) for c in cand], sc)
        if not order:
            return False
        v = order[0]
        k = cand.index(v)
        assert lmk[coff[k]:coff[k + 1]].tolist() == lids[v] and ftr[coff[k]:coff[k + 1]].tolist() == fids[v]
        xy = [co[v][g] for g in fids[v]]
        lm_v, ft_v = list(lids[v]), list(fids[v])
        X = ses.points()
        pose, mask, cnt = ses.pnp(lm_v, xy, L["intrinsics"][v])
        want = pnp_ref.pnp_ransac(lm_v, xy, X, L["intrinsics"][v])                                # the host run
        assert cnt == want["count"] and mask.tobytes() == want["mask"].tobytes(), (len(self.chosen), v)
        assert pose.tobytes() == want["pose34"].tobytes(), (len(self.chosen), v)
        self.log.append((v, len(lm_v), cnt, want["iterations"]))
        assert cnt >= 0, "view %d (step %d): no pose from %d entries" % (v, len(self.chosen), len(lm_v))
        P34 = pose.reshape(3, 4)
        self.cam_of[v] = ses.add_camera(np.concatenate([ba._rot_to_angle_axis(P34[:, :3]), P34[:, 3]]), L["intrinsics"][v])
        keep = np.flatnonzero(mask)
        lm_v, ft_v, xy = [lm_v[e] for e in keep], [ft_v[e] for e in keep], [xy[e] for e in keep]
        self.chosen.append(v)
        P = self.poses34()
        X = ses.points()
        st, added = ses.attach(self.cam_of[v], lm_v, ft_v, xy, poses34=P)
        want = nr.literal_attach(P[self.cam_of[v]], L["intrinsics"][v], X, list(zip(lm_v, ft_v, xy)))
        assert st.tolist() == want and added == want.count(0)
        for e in np.flatnonzero(st == 0):
            self.lms[lm_v[e]]["track"].append((v, ft_v[e]))
            ids[v][ft_v[e]] = lm_v[e]
        self.sync_mirror(strict=True)
        self.add_tracks(tri.new_view_tracks(v, ids, self.registered, im, fm))
        self.registered.append((v, True))
        ses.validity()
        ses.solve()
        ses.validity()
        self.sync_mirror()
        new_idx, _ = ses.remove_outliers()
        self.lms[:] = [lm for j, lm in enumerate(self.lms) if new_idx[j] >= 0]
        for i in ids:
            ids[i] = [int(new_idx[l]) if l >= 0 else -1 for l in ids[i]]
        return True

    def centre_errors(self):
        """Every registered camera's centre against the scene's, after a similarity transform over the centres
        (Umeyama), in units of the scene's own camera spread."""
        P = self.poses34().reshape(-1, 3, 4)
        G = ba.poses34_from_angle_axis(self.L["poses6"]).reshape(-1, 3, 4)
        imgs = sorted(self.cam_of)
        A = np.stack([-P[self.cam_of[i]][:, :3].T @ P[self.cam_of[i]][:, 3] for i in imgs])
        B = np.stack([-G[i][:, :3].T @ G[i][:, 3] for i in imgs])
        ma, mb = A.mean(0), B.mean(0)
        U, S, Vt = np.linalg.svd((B - mb).T @ (A - ma) / len(A))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = U @ D @ Vt
        s = (S * np.diag(D)).sum() / ((A - ma) ** 2).sum(1).mean()
        err = np.linalg.norm((s * (A - ma) @ R.T + mb) - B, axis=1)
        return err / np.sqrt(((B - mb) ** 2).sum(1).mean()), imgs


def test_incremental_loop_from_nothing(gpu_ctx):
    """B5: the loop from match lists, pixel coordinates and intrinsics alone, the host run (twoview_ref, tri_ref, pnp_ref,
    nextview_ref) alongside at every step.  End conditions of the existing loop test; every registered camera's centre error
    after a similarity alignment is bounded by 3 x the same figure of the scene-pose-seeded loop, run here too.
    The two figures are printed; DESIGN.md section 18 says whether they have been recorded."""
    worst = {}
    for from_nothing in (False, True):
        lp = _Loop(gpu_ctx, from_nothing)
        try:
            lp.start()
            while len(lp.cam_of) < lp.n and lp.step():
                pass
            err, imgs = lp.centre_errors()
            print("from nothing:" if from_nothing else "seeded by the scene's poses:", "pair", lp.first, "views chosen:", lp.chosen)
            print("  log:", lp.log)
            print("  landmarks:", lp.ses.counts()[1], " centre errors (relative to the cameras' spread): max %.3e mean %.3e" % (err.max(), err.mean()))
            assert len(lp.chosen) >= 15 and len(set(lp.chosen)) == len(lp.chosen) and not set(lp.chosen) & set(lp.first)
            assert lp.ses.counts()[1] > 500
            worst[from_nothing] = float(err.max())
        finally:
            lp.ses.close()
            gpu_ctx.check(gpu_ctx.lib.rcn_coords_clear(gpu_ctx.h))
    assert worst[True] <= 3.0 * worst[False], worst
