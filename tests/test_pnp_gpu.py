"""GPU suite: P3P-RANSAC view registration (rcn_pnp_ransac*, rcn_ba_session_pnp; csrc/pnp.hip) against tests/pnp_ref.py bit
for bit -- mask, count, iterations, both poses; a batch against its views one at a time; the device entry behind
rcn_corr_2d3d_device without a host wait in between; the session entry; argument errors and malformed device data; and the
reference's incremental loop running on its own poses."""
import os

import numpy as np
import pytest

import nextview_ref as nr
import pnp_ref
import tri_ref
from reconstructor_amd import _lib, ba, nextview, pnp
from reconstructor_amd import triangulate as tri

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_small.npz")
ERR_ARG = -1
KEYS = ("mask", "pose34", "ransac_pose34", "count", "iterations")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _batch(views):
    off = np.zeros(len(views) + 1, np.int64)
    off[1:] = np.cumsum([len(v[0]) for v in views])
    lm = np.concatenate([np.asarray(v[0], np.int32) for v in views]) if views else np.zeros(0, np.int32)
    xy = np.concatenate([np.asarray(v[1], np.int32).reshape(-1, 2) for v in views]) if views else np.zeros((0, 2), np.int32)
    return off, lm, xy, np.stack([v[2] for v in views])


def _assert_same(got, want, what):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype or k in ("count", "iterations"), (what, k)
        if k in ("count", "iterations"):
            assert g.tolist() == w.tolist(), (what, k, g, w)
        else:
            assert np.array_equal(_bits(g), _bits(w)), (what, k)


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("w", (0.0, 0.3, 0.6))
def test_scenes_equal_the_restatement_bit_for_bit(gpu_ctx, seed, w):
    """B1 on the scenes of A3: all 12 views in one call."""
    pts, views = pnp_ref.scene_views(seed, w)
    off, lm, xy, K = _batch([(v["landmark"], v["xy"], v["intr6"]) for v in views])
    got = pnp.pnp_ransac(gpu_ctx, off, lm, xy, pts, K)
    _assert_same(got, pnp_ref.pnp_ransac_batch(off, lm, xy, pts, K), (seed, w))


def test_edge_cases_equal_the_restatement_bit_for_bit(gpu_ctx):
    """B1 on the edge cases of A5, one call per case (each has its own points)."""
    for name, lm, xy, pts, K in pnp_ref.edge_cases():
        off = np.array([0, len(lm)], np.int64)
        got = pnp.pnp_ransac(gpu_ctx, off, lm, xy, pts, K)
        _assert_same(got, pnp_ref.pnp_ransac_batch(off, lm, xy, pts, K[None]), name)
        assert not np.isnan(got["pose34"]).any()


def test_golden(gpu_ctx):
    with np.load(GOLD) as g:
        got = pnp.pnp_ransac(gpu_ctx, g["off"], g["landmark"], g["xy"], g["points"], g["intr6"])
        _assert_same(got, {k: g[k] for k in KEYS}, "golden")


def _ragged(seed=7):
    """40 views, n from 0 to 6000: both the LDS and the index path, some empty, some < 4."""
    rng = np.random.default_rng(seed)
    pts, views = pnp_ref.scene_views(5, 0.0, n_cams=8, n_pts=1200)
    sizes = [0, 3, 6000, 4096, 4097, 5, 0, 2, 4500, 4] + [int(s) for s in rng.integers(10, 1500, 30)]
    out = []
    for k, n in enumerate(sizes):
        v = views[k % len(views)]
        P, K = v["pose34_gt"].reshape(3, 4), v["intr6"]
        lm = rng.integers(0, len(pts), n).astype(np.int32)
        l = pts[lm] @ P[:, :3].T + P[:, 3]
        xy = np.trunc(np.stack([K[0] * l[:, 0] / l[:, 2] + K[2], K[1] * l[:, 1] / l[:, 2] + K[3]], 1) + rng.normal(0, 0.5, (n, 2))).astype(np.int32)
        bad = rng.random(n) < (0.1 * (k % 6))
        lm[bad] = rng.integers(0, len(pts), int(bad.sum()))
        out.append((lm, xy, K))
    return pts, out


def test_batch_equals_single_calls(gpu_ctx):
    """B2."""
    pts, views = _ragged()
    off, lm, xy, K = _batch(views)
    got = pnp.pnp_ransac(gpu_ctx, off, lm, xy, pts, K)
    assert (got["count"] == -2).sum() == 4 and (got["count"] > 0).sum() >= 30
    for v, (l, x, k) in enumerate(views):
        one = pnp.pnp_ransac(gpu_ctx, [0, len(l)], l, x, pts, k)
        a, b = int(off[v]), int(off[v + 1])
        assert got["mask"][a:b].tobytes() == one["mask"].tobytes()
        for key in ("pose34", "ransac_pose34", "count", "iterations"):
            assert got[key][v].tobytes() == one[key][0].tobytes(), (v, key)
    # the index path against the restatement as well (n > 4096)
    for v in (2, 4):
        l, x, k = views[v]
        r = pnp_ref.pnp_ransac(l, x, pts, k)
        assert r["count"] == got["count"][v] and r["iterations"] == got["iterations"][v]
        assert np.array_equal(_bits(r["pose34"]), _bits(got["pose34"][v])) and np.array_equal(r["mask"], got["mask"][off[v]:off[v + 1]])


def test_argument_errors(gpu_ctx):
    """B5, host entries."""
    pts, views = pnp_ref.scene_views(3, 0.0, n_cams=4, n_pts=400)
    v = views[0]
    lm, xy, K = v["landmark"], v["xy"], v["intr6"]
    off = np.array([0, len(lm)], np.int64)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    pose, mask, cnt = np.zeros(12), np.zeros(len(lm), np.uint8), np.zeros(1, np.int32)
    X = np.ascontiguousarray(pts)

    def call(off=off, lm=lm, xy=xy, X=X, K=K, opt=None, pose=pose, mask=mask, cnt=cnt, n_points=len(pts), nv=1):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.rcn_pnp_ransac(h, nv, p(off), p(lm), p(xy), n_points, p(X), p(K), opt, p(pose), None, p(mask), p(cnt), None)

    assert call() == _lib.RCN_OK and cnt[0] > 100
    for kw in (dict(off=None), dict(lm=None), dict(xy=None), dict(X=None), dict(K=None), dict(pose=None), dict(mask=None), dict(cnt=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(off=np.array([0, 10, 5], np.int64), K=np.stack([K, K]), nv=2) == ERR_ARG
    bad = lm.copy()
    bad[17] = len(pts)
    assert call(lm=bad) == ERR_ARG
    bad[17] = -1
    assert call(lm=bad) == ERR_ARG
    for field, val in (("confidence", 0.0), ("confidence", 1.0), ("confidence", 1.5), ("max_projection_error", 0.0),
                       ("max_projection_error", -1.0), ("max_iterations", 0)):
        o = pnp.default_options(gpu_ctx)
        setattr(o, field, val)
        assert call(opt=o) == ERR_ARG, field
        assert gpu_ctx.lib.rcn_last_error(h)
    o = pnp.default_options(gpu_ctx)
    assert (o.max_projection_error, o.confidence, o.max_iterations, o.refine_iterations) == (4.0, 0.99, 10000, 20)
    assert call() == _lib.RCN_OK                                        # the ctx is still usable
    ses = ba.BaSession(gpu_ctx)
    try:
        ses.add_points(pts)
        p = lambda a: a.ctypes.data
        assert lib.rcn_ba_session_pnp(ses.h, len(lm), p(bad), p(xy), p(K), None, p(pose), p(mask), cnt.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))) == ERR_ARG
        assert lib.rcn_ba_session_pnp(ses.h, len(lm), None, p(xy), p(K), None, p(pose), p(mask), cnt.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))) == ERR_ARG
        got = ses.pnp(lm, xy, K)                                        # B4 in small
        want = pnp.pnp_ransac(gpu_ctx, off, lm, xy, ses.points(), K)
        assert got[0].tobytes() == want["pose34"].tobytes() and got[1].tobytes() == want["mask"].tobytes() and got[2] == want["count"][0]
    finally:
        ses.close()


def _upload_coords(ctx, coords):
    for i, xy in coords.items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))


def test_malformed_device_data(gpu_ctx):
    """B5, device entry: a landmark = n_points, a feature = K, an image never uploaded -- malformed data, handled."""
    import torch
    dev = torch.device("cuda", gpu_ctx.device)
    pts, views = pnp_ref.scene_views(3, 0.0, n_cams=4, n_pts=400)
    ctx = gpu_ctx
    ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
    lm_all, ft_all, imgs, Ks, off = [], [], [], [], [0]
    for i, v in enumerate(views[:3]):
        img = 100 + 2 * i
        if i < 2:
            _upload_coords(ctx, {img: v["xy"]})
        lm_all.append(v["landmark"].copy()); ft_all.append(np.arange(len(v["landmark"]), dtype=np.int32))
        imgs.append(img); Ks.append(v["intr6"]); off.append(off[-1] + len(v["landmark"]))
    imgs[2] = 101                                     # inside the span of ids, never uploaded
    lm_all[0][[3, 50]] = [len(pts), -4]
    ft_all[0][[9, 60]] = [len(views[0]["landmark"]), -1]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
    X = t(pts, np.float64)
    out = pnp.pnp_ransac_device(ctx, t(off, np.int64), t(np.concatenate(lm_all), np.int32), t(np.concatenate(ft_all), np.int32),
                                t(imgs, np.int32), len(pts), X, t(np.stack(Ks), np.float64))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    cnt, mask = out["count"].cpu().numpy(), out["mask"].cpu().numpy()
    assert cnt[2] == -2 and not mask[off[2]:off[3]].any()
    assert cnt[0] > 0.8 * (off[1] - 4) and not mask[[3, 50, 9, 60]].any()
    want = pnp.pnp_ransac(ctx, [0, off[2] - off[1]], views[1]["landmark"], views[1]["xy"], pts, views[1]["intr6"])
    assert cnt[1] == want["count"][0] and out["pose34"][1].cpu().numpy().tobytes() == want["pose34"].tobytes()
    ctx.check(ctx.lib.rcn_coords_clear(ctx.h))


class _Loop:
    """test_incremental_loop_with_gpu_ranking's loop (tests/test_nextview_gpu.py), with the pose of a new view either the
    scene's (use_pnp=False) or BaSession.pnp's on the candidate's own 2D-3D list (use_pnp=True)."""

    def __init__(self, ctx, use_pnp):
        self.ctx, self.use_pnp, self.n = ctx, use_pnp, 25
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
        for v in (0, 1):
            self.cam_of[v] = self.ses.add_camera(L["poses6"][v], L["intrinsics"][v])
        self.add_tracks(tri.initial_pair_tracks(self.fm[(0, 1)], 0, 1))
        self.registered = [(1, True), (0, True)]

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
        if self.use_pnp:
            X = ses.points()
            pose, mask, cnt = ses.pnp(lm_v, xy, L["intrinsics"][v])
            want = pnp_ref.pnp_ransac(lm_v, xy, X, L["intrinsics"][v])                            # the host run
            assert cnt == want["count"] and mask.tobytes() == want["mask"].tobytes(), (len(self.chosen), v)
            assert pose.tobytes() == want["pose34"].tobytes(), (len(self.chosen), v)
            self.log.append((v, len(lm_v), cnt, want["iterations"]))
            assert cnt >= 0, "view %d (step %d): no pose from %d entries" % (v, len(self.chosen), len(lm_v))
            P34 = pose.reshape(3, 4)
            self.cam_of[v] = ses.add_camera(np.concatenate([ba._rot_to_angle_axis(P34[:, :3]), P34[:, 3]]), L["intrinsics"][v])
            keep = np.flatnonzero(mask)
            lm_v, ft_v, xy = [lm_v[e] for e in keep], [ft_v[e] for e in keep], [xy[e] for e in keep]
        else:
            self.cam_of[v] = ses.add_camera(L["poses6"][v], L["intrinsics"][v])
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


def test_device_entry_behind_corr_2d3d_device(gpu_ctx):
    """B3: all 13 candidates after 12 views; both device calls enqueued, one rcn_synchronize, then the outputs."""
    import torch
    ctx = gpu_ctx
    dev = torch.device("cuda", ctx.device)
    lp = _Loop(ctx, use_pnp=False)
    try:
        lp.start()
        while len(lp.cam_of) < 12:
            assert lp.step()
        cand, tracks = lp.candidates()
        assert len(cand) == 13
        g = nextview.graph_arrays(tracks)
        shapes = np.asarray([lp.shape[c] for c in cand], np.int32)
        K = np.stack([lp.L["intrinsics"][c] for c in cand]).astype(np.float64)
        coff_h, lm_h, ft_h, _, _ = nextview.corr_2d3d(ctx, *g, cand, shapes)
        total = int(coff_h[-1])
        t = lambda a, dt=np.int32: torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
        off, img, feat, cand_d, shp = t(g[0]), t(g[1]), t(g[2]), t(cand), t(shapes)
        coff = torch.zeros(len(cand) + 1, dtype=torch.int64, device=dev)
        lm = torch.zeros(total + 8, dtype=torch.int32, device=dev)
        ft = torch.zeros(total + 8, dtype=torch.int32, device=dev)
        tot = torch.zeros(1, dtype=torch.int64, device=dev)
        cells = torch.zeros(len(cand), dtype=torch.int32, device=dev)
        outside = torch.zeros(len(cand), dtype=torch.int32, device=dev)
        K_d = t(K, np.float64)
        npts = lp.ses.counts()[1]
        pts_ptr = ctx.lib.rcn_ba_session_points_device(lp.ses.h)
        torch.cuda.synchronize(dev)
        ctx.check(ctx.lib.rcn_corr_2d3d_device(ctx.h, len(g[0]) - 1, len(g[1]), off.data_ptr(), img.data_ptr(), feat.data_ptr(), len(cand),
                                               cand_d.data_ptr(), shp.data_ptr(), coff.data_ptr(), lm.data_ptr(), ft.data_ptr(),
                                               total + 8, tot.data_ptr(), cells.data_ptr(), outside.data_ptr()))
        out = pnp.pnp_ransac_device(ctx, coff, lm, ft, cand_d, npts, pts_ptr, K_d)         # nothing synchronised in between
        ctx.check(ctx.lib.rcn_synchronize(ctx.h))
        assert np.array_equal(coff.cpu().numpy(), coff_h) and lm[:total].cpu().numpy().tobytes() == lm_h.tobytes()
        xy_h = np.concatenate([np.asarray(lp.co[c], np.int32).reshape(-1, 2)[ft_h[coff_h[k]:coff_h[k + 1]]] for k, c in enumerate(cand)])
        want = pnp.pnp_ransac(ctx, coff_h, lm_h, xy_h, lp.ses.points(), K)
        assert (want["count"] > 30).sum() >= 5
        for k in KEYS:
            gk = out[k].cpu().numpy()
            gk = gk[:total] if k == "mask" else gk
            assert gk.tobytes() == want[k].tobytes(), k
    finally:
        lp.ses.close()


def test_session_pnp_equals_host_entry(gpu_ctx):
    """B4."""
    pts, views = pnp_ref.scene_views(2, 0.3)
    ses = ba.BaSession(gpu_ctx)
    try:
        ses.add_points(pts)
        for v in views[:4]:
            got = ses.pnp(v["landmark"], v["xy"], v["intr6"])
            want = pnp.pnp_ransac(gpu_ctx, [0, len(v["landmark"])], v["landmark"], v["xy"], ses.points(), v["intr6"])
            assert got[0].tobytes() == want["pose34"].tobytes() and got[1].tobytes() == want["mask"].tobytes() and got[2] == want["count"][0] > 0
    finally:
        ses.close()


def test_incremental_loop_on_its_own_poses(gpu_ctx):
    """B6: test_incremental_loop_with_gpu_ranking with BaSession.pnp in the scene pose's place; the host run uses pnp_ref
    on the same lists and points.  End conditions unchanged: >= 15 views registered by the loop, > 500 landmarks."""
    lp = _Loop(gpu_ctx, use_pnp=True)
    try:
        lp.start()
        while len(lp.cam_of) < lp.n and lp.step():
            pass
        print("views chosen:", lp.chosen)
        print("(view, entries, inliers, iterations):", lp.log)
        print("landmarks:", lp.ses.counts()[1])
        assert len(lp.chosen) >= 15 and len(set(lp.chosen)) == len(lp.chosen)
        assert lp.ses.counts()[1] > 500
    finally:
        lp.ses.close()
