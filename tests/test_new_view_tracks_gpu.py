"""GPU suite: step 3 of triangulateMatchedLandmarks on the device (rcn_landmark_ids_*, rcn_new_view_tracks_device,
rcn_new_view_triangulate_device, rcn_ba_session_grow_view; csrc/corr2d3d.hip) against the literal host walk
(triangulate.new_view_tracks + tracks_to_arrays): the candidates and their CSR arrays exactly, under mirror and without, in
two orders of the registered images, across several workgroup-wide chunks, under a capacity too small; the fused call
against the triangulation of the host's candidates bit for bit, table included; a session grown view by view next to one
fed by the host walk; the argument errors."""
import copy

import numpy as np
import pytest

import nextview_ref as nr
import nvt_ref
import tri_ref
from reconstructor_amd import _lib, ba, newview, nextview
from reconstructor_amd import triangulate as tri

pytestmark = pytest.mark.gpu


def _upload(ctx, L, mirror, ids=None):
    for i, xy in L["coords"].items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))
    fm = L["feature_matches"]
    nextview.upload_feature_matches(ctx, nr.canonical_lists(fm) if mirror else fm, mirror=mirror)
    table = newview.LandmarkIds(ctx)
    table.reset()
    table.set_all(L["landmark_ids"] if ids is None else ids)
    return table


def _host(L, registered=None):
    """The literal walk and its flattening: (tracks, trk_off, obs_cam, obs_xy, trk_src)."""
    tracks = tri.new_view_tracks(L["v"], L["landmark_ids"], registered if registered is not None else L["registered"],
                                 L["img_matches"], L["feature_matches"])
    off, cam, xy = tri.tracks_to_arrays(tracks, L["cam_index"], L["coords"])
    src = np.asarray([(r, g, f) for (r, g), (_, f) in tracks], np.int32).reshape(-1, 3)
    return tracks, off, cam, xy.reshape(-1, 2), src


def _assert_equal(got, want, cap):
    n_tracks, off, cam, xy, src = (a.cpu().numpy() for a in got)
    tracks, w_off, w_cam, w_xy, w_src = want
    n = len(tracks)
    assert int(n_tracks[0]) == n
    m = min(n, cap)
    assert np.array_equal(off, 2 * np.minimum(np.arange(cap + 1), n))
    assert np.array_equal(off[:m + 1], w_off[:m + 1])
    assert np.array_equal(cam[:2 * m], w_cam[:2 * m]) and np.array_equal(xy[:2 * m], w_xy[:2 * m])
    assert np.array_equal(src[:m], w_src[:m])


@pytest.mark.parametrize("mirror", [True, False])
def test_small_scene_equals_the_host_walk(gpu_ctx, mirror):
    L = nvt_ref.scene(5, 70, 3, 1)
    v, ids = L["v"], L["landmark_ids"]
    orders = [L["registered"], L["registered"][::-1]]
    partners = []
    for reg in orders:                                                     # from the host reference alone
        kinds = nvt_ref.classify(v, ids, reg, L["img_matches"], L["feature_matches"])
        for kind in (nvt_ref.TAKEN, nvt_ref.FIRST, nvt_ref.FALL_THROUGH, nvt_ref.NO_TRACK):
            assert kinds.count(kind) >= 1, kind
        want = _host(L, reg)
        assert len(want[0]) == kinds.count(nvt_ref.FIRST) + kinds.count(nvt_ref.FALL_THROUGH)
        partners.append(want[4][:, 0].tolist())
    assert partners[0] != partners[1]                                      # the order of registered decides
    _upload(gpu_ctx, L, mirror)
    K = len(L["coords"][v])
    for reg in orders:
        got = newview.new_view_tracks_device(gpu_ctx, v, reg, L["img_matches"], L["cam_index"], K)
        _assert_equal(got, _host(L, reg), K)


def test_compaction_across_chunks_and_twice_the_same_bytes(gpu_ctx):
    L = nvt_ref.scene(8, 2000, 5, 2)
    v = L["v"]
    K = len(L["coords"][v])
    assert K > 1024                                                        # several workgroup-wide chunks of the ordered compaction
    want = _host(L)
    kinds = nvt_ref.classify(v, L["landmark_ids"], L["registered"], L["img_matches"], L["feature_matches"])
    assert kinds.count(nvt_ref.FALL_THROUGH) >= 1 and max(f for _, _, f in want[4].tolist()) > 1024
    _upload(gpu_ctx, L, True)
    runs = [newview.new_view_tracks_device(gpu_ctx, v, L["registered"], L["img_matches"], L["cam_index"], K) for _ in range(2)]
    _assert_equal(runs[0], want, K)
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_capacity_drops_the_tail_and_writes_nothing_behind(gpu_ctx):
    L = nvt_ref.scene(8, 2000, 5, 2)
    v = L["v"]
    want = _host(L)
    n = len(want[0])
    cap, pad = n // 2, 64
    assert cap >= 1
    _upload(gpu_ctx, L, False)
    n_tracks, off, cam, xy, src = newview.new_view_tracks_device(gpu_ctx, v, L["registered"], L["img_matches"], L["cam_index"], cap, pad=pad)
    for a, size in ((n_tracks, 1), (off, cap + 1), (cam, 2 * cap), (xy, 4 * cap), (src, 3 * cap)):
        assert a.numel() == size + pad and bool((a[size:] == -7).all())
    assert int(n_tracks[0].item()) == n                                    # the full count
    _assert_equal((n_tracks[:1], off[:cap + 1], cam[:2 * cap], xy[:4 * cap].reshape(-1, 2), src[:3 * cap].reshape(-1, 3)), want, cap)


def test_fused_call_equals_the_triangulation_of_the_host_walk(gpu_ctx):
    L = nvt_ref.scene(8, 2000, 5, 3)
    v, ids = L["v"], L["landmark_ids"]
    n_img = len(L["coords"])
    P = np.stack([L["poses34"][i] for i in range(n_img)])
    Kc = np.stack([L["intrinsics"][i] for i in range(n_img)])
    tracks, off, cam, xy, src = _host(L)
    n, first, K = len(tracks), 1000, len(L["coords"][v])
    table = _upload(gpu_ctx, L, True)
    w_xyz, w_st, w_compact, w_cnt = tri.triangulate_tracks_device(gpu_ctx, P, Kc, off, cam, xy, compact_first=first)
    w_st = w_st.cpu().numpy()
    assert (w_st == 0).sum() >= 10 and (w_st != 0).sum() >= 1              # accepted and rejected tracks
    out = newview.new_view_triangulate_device(gpu_ctx, v, L["registered"], L["img_matches"], L["cam_index"], P, Kc, first, K, compact_first=first)
    _assert_equal((out["n_tracks"], out["trk_off"], out["obs_cam"], out["obs_xy"], out["trk_src"]), (tracks, off, cam, xy, src), K)
    assert int(out["n_accepted"][0].item()) == int(w_cnt[0].item()) == (w_st == 0).sum()
    assert out["xyz"][:n].cpu().numpy().tobytes() == w_xyz.cpu().numpy().tobytes()
    st = out["status"].cpu().numpy()
    assert np.array_equal(st[:n], w_st) and (st[n:] == 1).all()            # rows past the count: empty tracks
    assert out["compact"][:first + n].cpu().numpy().tobytes() == w_compact[:first + n].cpu().numpy().tobytes()
    want_ids = copy.deepcopy(ids)
    for rank, j in enumerate(np.flatnonzero(w_st == 0)):
        for i, f in tracks[j]:
            want_ids[i][f] = first + rank
    assert want_ids != ids
    for i in range(n_img):
        assert table.read(i, len(ids[i])).tolist() == want_ids[i]


def _grow_loop(ctx, L, n, use_grow_view):
    """The loop of test_nextview_gpu.py::test_incremental_loop_with_gpu_ranking; step 3 either by the host walk and
    BaSession.triangulate or by BaSession.grow_view.  Returns what every view left behind."""
    L = copy.deepcopy(L)
    co, ids, fm, im = L["coords"], L["landmark_ids"], L["feature_matches"], L["img_matches"]
    shape = {i: nr.SHAPE for i in range(n)}
    table = newview.LandmarkIds(ctx)
    table.reset()
    ses = ba.BaSession(ctx)
    lms, cam_of, snaps, fell = [], {}, [], 0

    def poses34():
        return ba.poses34_from_angle_axis(ses.cameras()[0])

    def accept(tracks, st, first):
        for k, j in enumerate(np.flatnonzero(st == 0)):
            for i, f in tracks[j]:
                ids[i][f] = first + k
            lms.append({"track": list(tracks[j])})

    def sync_mirror():
        pt, cam, xy = ses.graph()
        for j, lm in enumerate(lms):
            mine = [(c, x, y) for c, (x, y) in zip(cam[pt == j], xy[pt == j])]
            kept, q = [], 0
            for i, f in lm["track"]:
                if q < len(mine) and mine[q] == (cam_of[i], *co[i][f]):
                    kept.append((i, f)); q += 1
            assert q == len(mine)
            lm["track"] = kept

    try:
        for v in (0, 1):
            cam_of[v] = ses.add_camera(L["poses6"][v], L["intrinsics"][v])
        tracks = tri.initial_pair_tracks(fm[(0, 1)], 0, 1)
        st, first, _ = ses.triangulate(*tri.tracks_to_arrays(tracks, cam_of, co), poses34=poses34())
        accept(tracks, st, first)
        if use_grow_view:
            table.set_all(ids)
        registered = [(1, True), (0, True)]
        while len(cam_of) < n:
            cand = [i for i in range(n) if i not in cam_of]
            coff, lmk, ftr, cells, _ = nextview.corr_2d3d(ctx, *nextview.graph_arrays([lm["track"] for lm in lms]), cand, [shape[c] for c in cand])
            order = nextview.rank_next_images(cand, np.diff(coff), cells, nextview.MATCH_DENSITY, 30)
            if not order:
                break
            v = order[0]
            k = cand.index(v)
            lids, fids = lmk[coff[k]:coff[k + 1]].tolist(), ftr[coff[k]:coff[k + 1]].tolist()
            cam_of[v] = ses.add_camera(L["poses6"][v], L["intrinsics"][v])          # PnP's place: the scene pose
            P = poses34()
            st, _ = ses.attach(cam_of[v], lids, fids, [co[v][g] for g in fids], poses34=P)
            hit = np.flatnonzero(st == 0)
            for e in hit:
                lms[lids[e]]["track"].append((v, fids[e]))
                ids[v][fids[e]] = lids[e]
            if use_grow_view:
                table.set(v, [fids[e] for e in hit], [lids[e] for e in hit])
                src, st, first, _ = ses.grow_view(v, len(co[v]), registered, im, cam_of, poses34=P)
                tracks = [[(int(r), int(g)), (v, int(f))] for r, g, f in src]
            else:
                fell += nvt_ref.classify(v, ids, registered, im, fm).count(nvt_ref.FALL_THROUGH)
                tracks = tri.new_view_tracks(v, ids, registered, im, fm)
                st, first, _ = ses.triangulate(*tri.tracks_to_arrays(tracks, cam_of, co), poses34=P)
            accept(tracks, st, first)
            registered.append((v, True))
            ses.validity()
            ses.solve()
            ses.validity()
            sync_mirror()
            new_idx, _ = ses.remove_outliers()
            lms[:] = [lm for j, lm in enumerate(lms) if new_idx[j] >= 0]
            before = copy.deepcopy(ids) if use_grow_view else None
            for i in ids:
                ids[i] = [int(new_idx[l]) if l >= 0 else -1 for l in ids[i]]
            if use_grow_view:                                              # the wrapper keeps the table current
                ch = [(i, f, ids[i][f]) for i in ids for f in range(len(ids[i])) if ids[i][f] != before[i][f]]
                if ch:
                    table.set(*zip(*ch))
                for i in ids:
                    assert table.read(i, len(ids[i])).tolist() == ids[i]
            snaps.append((v, ses.graph(), ses.points().view(np.uint64).copy(), copy.deepcopy(ids)))
    finally:
        ses.close()
    return snaps, fell


def test_session_grown_by_grow_view_equals_the_host_walk(gpu_ctx):
    n = 10
    L = tri_ref.loop_containers(n, 600, obs_per_point=6, seed=33)
    for i, xy in L["coords"].items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        gpu_ctx.check(gpu_ctx.lib.rcn_coords_upload(gpu_ctx.h, int(i), a.ctypes.data, len(a)))
    nextview.upload_feature_matches(gpu_ctx, nr.canonical_lists(L["feature_matches"]), mirror=True)
    host, fell = _grow_loop(gpu_ctx, L, n, False)
    assert len(host) >= 5 and fell >= 1                                    # views registered; a track that fell through a taken partner
    grown, _ = _grow_loop(gpu_ctx, L, n, True)
    assert len(grown) == len(host)
    for (v0, g0, x0, i0), (v1, g1, x1, i1) in zip(host, grown):
        assert v0 == v1
        assert all(np.array_equal(a, b) for a, b in zip(g0, g1))
        assert np.array_equal(x0, x1)
        assert i0 == i1


def test_argument_errors_leave_the_ctx_usable(gpu_ctx):
    L = nvt_ref.scene(5, 70, 3, 1)
    v, im, cams = L["v"], L["img_matches"], L["cam_index"]
    K = len(L["coords"][v])
    table = newview.LandmarkIds(gpu_ctx)

    def err(code, text, fn, *a):
        with pytest.raises(_lib.RcnError) as e:
            fn(*a)
        assert e.value.code == code and text in str(e.value)

    call = lambda reg, img=v: newview.new_view_tracks_device(gpu_ctx, img, reg, im, cams, K)
    _upload(gpu_ctx, L, True)
    nextview.clear_lists(gpu_ctx)
    err(-1, "no match lists", call, L["registered"])
    err(-1, "no match lists", table.reset)                                 # ... and the table is gone with the failed reset
    nextview.upload_feature_matches(gpu_ctx, L["feature_matches"])
    err(-1, "no landmark-id table", call, L["registered"])
    err(-1, "no landmark-id table", table.read, v, K)
    table.reset()
    nextview.upload_feature_matches(gpu_ctx, L["feature_matches"])       # a new upload invalidates the table
    err(-1, "invalidated", call, L["registered"])
    err(-1, "invalidated", table.set, v, [0], [5])
    table.reset()
    table.set_all(L["landmark_ids"])
    err(-1, "listed twice", call, [(0, True), (1, True), (0, True)])
    im2 = dict(im)
    im2[v] = list(im[v]) + [v]
    err(-1, "among the registered", lambda: newview.new_view_tracks_device(gpu_ctx, v, [(0, True), (v, True)], im2, cams, K))
    im2[v] = list(im[v]) + [999]
    cams2 = dict(cams)
    cams2[999] = 0
    err(-5, "999", lambda: newview.new_view_tracks_device(gpu_ctx, v, [(0, True), (999, True)], im2, cams2, K))
    cams2[777] = 0
    im2[777] = [0]
    err(-5, "777", lambda: newview.new_view_tracks_device(gpu_ctx, 777, [(0, True)], im2, cams2, K))
    err(-1, "out of range", table.set, v, [K], [5])
    err(-5, "no row", table.set, 123456, [0], [5])
    _assert_equal(call(L["registered"]), _host(L), K)                      # the ctx still works
