"""GPU suite: the next-view search (rcn_corr_2d3d*, rcn_landmark_attach, rcn_ba_session_attach; csrc/corr2d3d.hip) against
the transcriptions of tests/nextview_ref.py -- lists, counts, cells and out-of-frame counts exactly; the device entry and
every workspace budget give the same bytes; the argument errors; attach statuses and the session graph; and the reference's
incremental loop with every view chosen by the GPU ranking."""
import numpy as np
import pytest

import nextview_ref as nr
import tri_ref
from reconstructor_amd import _lib, ba, nextview
from reconstructor_amd import triangulate as tri

pytestmark = pytest.mark.gpu


def _upload_coords(ctx, coords):
    for i, xy in coords.items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))


def _inputs(L, mirror):
    lists = nr.canonical_lists(L["feature_matches"]) if mirror else L["feature_matches"]
    off, img, feat = nextview.graph_arrays(L["tracks"])
    cand = L["candidates"]
    return lists, (off, img, feat), cand, np.asarray([L["shapes"][c] for c in cand], np.int32)


def _edge_case(n_images, n_points, seed):
    """make_case plus a candidate with no lists at all, and the matched features of one candidate moved onto the frame
    edge: x = -1 (cell 0), x = cols - 1 (cell 31), x = cols and x = -cols / 32 (outside)."""
    L = nr.make_case(n_images, n_points, seed=seed)
    rows, cols = nr.SHAPE
    lone = n_images
    L["coords"][lone] = [(5, 5), (100, 200)]
    L["img_matches"][lone] = []
    L["landmark_ids"][lone] = [-1, -1]
    L["shapes"][lone] = nr.SHAPE
    L["candidates"].append(lone)
    c = L["candidates"][0]
    co = list(L["coords"][c])
    for k, g in enumerate(sorted({g for (i, cc), m in L["feature_matches"].items() if cc == c for g in m.values()})[:40]):
        co[g] = [(-1, 3), (cols - 1, rows - 1), (cols, 10), (-cols // 32, 7), (3, -1), (10, rows)][k % 6]
    L["coords"][c] = co
    return L


@pytest.mark.parametrize("n_images,n_points,seed,mirror", [(25, 1500, 41, True), (60, 3000, 42, False), (200, 6000, 43, True)])
def test_corr_equals_the_transcription(gpu_ctx, n_images, n_points, seed, mirror):
    L = _edge_case(n_images, n_points, seed)
    _upload_coords(gpu_ctx, L["coords"])
    lists, g, cand, shapes = _inputs(L, mirror)
    nextview.upload_feature_matches(gpu_ctx, lists, mirror=mirror)
    got = nextview.corr_2d3d(gpu_ctx, *g, cand, shapes)
    want = nr.vector_corr(*g, *nextview.lists_from_dict(lists), mirror, cand, shapes, L["coords"])
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    lids, fids = nr.literal_calc_2d3d_matches(cand, L["img_matches"], L["feature_matches"], L["landmark_ids"], L["tracks"])
    coff, lm, ft, cells, outside = got
    for k, c in enumerate(cand):
        assert lm[coff[k]:coff[k + 1]].tolist() == lids[c] and ft[coff[k]:coff[k + 1]].tolist() == fids[c]
    assert coff[-1] - coff[-2] == 0 and cells[-1] == 0                 # the candidate without lists
    assert outside[0] > 0 and outside.sum() > outside[0]                # the edge features, and synth_ba's own
    assert (cells > 30).sum() >= 1


def test_device_entry_and_budgets_give_the_same_bytes(gpu_ctx):
    import torch
    L = _edge_case(40, 2500, 44)
    _upload_coords(gpu_ctx, L["coords"])
    lists, g, cand, shapes = _inputs(L, True)
    nextview.upload_feature_matches(gpu_ctx, lists, mirror=True)
    ref = nextview.corr_2d3d(gpu_ctx, *g, cand, shapes)
    total = int(ref[0][-1])
    n_obs = len(g[1])
    try:
        for budget in (1 << 30, 4 * n_obs + 1, 3 * 4 * 4096 * ((n_obs + 4095) // 4096)):
            nextview.set_workspace_bytes(gpu_ctx, budget)
            assert all(np.array_equal(a, b) for a, b in zip(nextview.corr_2d3d(gpu_ctx, *g, cand, shapes), ref))
            coff, lm, ft, tot, cells, outside = nextview.corr_2d3d_device(gpu_ctx, *g, cand, shapes, total + 5)
            assert int(tot.item()) == total
            assert np.array_equal(coff.cpu().numpy(), ref[0])
            assert lm[:total].cpu().numpy().tobytes() == ref[1].tobytes() and ft[:total].cpu().numpy().tobytes() == ref[2].tobytes()
            assert (lm[total:] == -7).all() and (ft[total:] == -7).all()
            assert np.array_equal(cells.cpu().numpy(), ref[3]) and np.array_equal(outside.cpu().numpy(), ref[4])
        # too small a capacity on the device: the entries past it are dropped, the total still counts them
        coff, lm, ft, tot, _, _ = nextview.corr_2d3d_device(gpu_ctx, *g, cand, shapes, total // 2)
        assert int(tot.item()) == total and lm[:total // 2].cpu().numpy().tobytes() == ref[1][:total // 2].tobytes()
    finally:
        nextview.set_workspace_bytes(gpu_ctx, 1 << 30)
    torch.cuda.synchronize()


def test_argument_errors(gpu_ctx):
    L = nr.make_case(10, 400, seed=45)
    _upload_coords(gpu_ctx, L["coords"])
    lists, g, cand, shapes = _inputs(L, False)
    nextview.upload_feature_matches(gpu_ctx, lists)
    off, img, feat = g

    def err(fn, *a, text=""):
        with pytest.raises(_lib.RcnError) as e:
            fn(*a)
        assert e.value.code == -1 and text in str(e.value)

    dup = np.concatenate([img, img[:1]]), np.concatenate([feat, feat[:1]])
    off2 = np.concatenate([off, [off[-1] + 1]]).astype(np.int32)
    err(nextview.corr_2d3d, gpu_ctx, off2, *dup, cand, shapes, text="observed twice")
    err(nextview.corr_2d3d, gpu_ctx, *g, cand + cand[:1], np.concatenate([shapes, shapes[:1]]), text="listed twice")
    err(nextview.corr_2d3d, gpu_ctx, *g, [999], [[10, 10]], text="coordinates")
    err(nextview.corr_2d3d, gpu_ctx, *g, cand[:1], [[0, 10]], text="shape")
    with pytest.raises(_lib.RcnError) as e:
        nextview.corr_2d3d(gpu_ctx, *g, cand, shapes, capacity=1)
    assert e.value.code == -1 and "capacity" in str(e.value)
    pairs, offsets, qt = nextview.lists_from_dict(lists)
    err(nextview.upload_lists, gpu_ctx, np.concatenate([pairs, pairs[:1]]), np.concatenate([offsets, offsets[-1:] + 1]),
        np.concatenate([qt, qt[:1]]), text="given twice")
    p = int(np.flatnonzero(np.diff(offsets) >= 2)[0])
    bad = qt.copy()
    bad[offsets[p] + 1, 1] = bad[offsets[p], 1]
    err(nextview.upload_lists, gpu_ctx, pairs, offsets, bad, text="injective")
    bad = qt.copy()
    bad[0, 0] = 10 ** 6
    err(nextview.upload_lists, gpu_ctx, pairs, offsets, bad, text="out of range")
    p2 = pairs.copy()
    p2[0, 0] = 777
    err(nextview.upload_lists, gpu_ctx, p2, offsets, qt, text="no coordinates")
    nextview.clear_lists(gpu_ctx)
    err(nextview.corr_2d3d, gpu_ctx, *g, cand, shapes, text="no match lists")


def _attach_scene(seed):
    rng = np.random.default_rng(seed)
    c, s = np.cos(0.1), np.sin(0.1)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    P = np.concatenate([R, np.array([[0.2], [-0.1], [0.3]])], 1).reshape(-1)
    K = np.array([600.0, 600.0, 256.0, 168.0, 1e-3, -2e-4])
    pts = np.column_stack([rng.uniform(-1.5, 1.5, 400), rng.uniform(-1, 1, 400), rng.uniform(2, 8, 400)])
    pts[:20, 2] = -pts[:20, 2] - 1.0                                      # behind the camera
    ents = []
    for e in range(4000):
        l = int(rng.integers(0, 400))
        u, v = _project(P, K, pts[l])
        ents.append((l, int(rng.integers(0, 500)), (int(np.clip(np.trunc(u + rng.normal(0, 3)), -1e6, 1e6)),
                                                    int(np.clip(np.trunc(v + rng.normal(0, 3)), -1e6, 1e6)))))
    return P, K, pts, ents


def _project(P, K, X):
    l = np.asarray(P).reshape(3, 4) @ np.append(X, 1.0)
    x, y = l[0] / l[2], l[1] / l[2]
    r = x * x + y * y
    d = K[4] * r + K[5] * r * r
    return K[0] * (x + d) + K[2], K[1] * (y + d) + K[3]


def test_attach_statuses(gpu_ctx):
    P, K, pts, ents = _attach_scene(46)
    # a residual of exactly 4.0: K without distortion, P = [I | 0], a point on the ray of pixel (256, 168) (the principal
    # point: projects to it exactly), observed at (258, 166) -> |2| + |2| = 4.0, rejected (strict <)
    Pi = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(-1)
    K0 = np.array([600.0, 600.0, 256.0, 168.0, 0.0, 0.0])
    pts0 = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0], [0.0, 0.0, 3.0]])
    e0 = [(0, 7, (258, 166)), (1, 8, (256, 168)), (0, 9, (259, 168)), (0, 9, (256, 168)), (2, 9, (256, 168)), (2, 7, (257, 168))]
    st = nextview.attach(gpu_ctx, Pi, K0, pts0, *zip(*[(l, f, xy) for l, f, xy in e0]))
    assert st.tolist() == [2, 1, 0, 3, 3, 0] == nr.literal_attach(Pi, K0, pts0, e0)
    e1 = [(0, 5, (270, 168)), (0, 5, (256, 169)), (2, 5, (256, 168))]     # the first entry of a feature rejected, the second attached
    assert nextview.attach(gpu_ctx, Pi, K0, pts0, *zip(*e1)).tolist() == [2, 0, 3] == nr.literal_attach(Pi, K0, pts0, e1)
    lm, ft, xy = zip(*ents)
    st = nextview.attach(gpu_ctx, P, K, pts, lm, ft, xy)
    assert st.tolist() == nr.literal_attach(P, K, pts, ents)
    assert {0, 1, 2, 3} <= set(st.tolist())
    with pytest.raises(_lib.RcnError):
        nextview.attach(gpu_ctx, P, K, pts, [400], [0], [(0, 0)])


def test_session_attach_equals_add_observations(gpu_ctx):
    P, K, pts, ents = _attach_scene(47)
    lm, ft, xy = (np.asarray(a) for a in zip(*ents))
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    sessions = [ba.BaSession(gpu_ctx), ba.BaSession(gpu_ctx)]
    try:
        for s in sessions:
            s.add_camera(np.zeros(6), K)
            s.add_camera(np.zeros(6), K)
            s.add_points(pts)
            s.add_observations(np.arange(400), np.zeros(400, np.int32), np.zeros((400, 2), np.int32))
        poses34 = np.stack([np.eye(3, 4).reshape(-1), P])
        st, added = sessions[0].attach(1, lm, ft, xy, poses34=poses34)
        want = np.asarray(nr.literal_attach(P, K, pts, ents))
        assert np.array_equal(st, want) and added == (want == 0).sum()
        ok = np.flatnonzero(want == 0)
        sessions[1].add_observations(lm[ok], np.ones(len(ok), np.int32), xy[ok])
        for a, b in zip(sessions[0].graph(), sessions[1].graph()):
            assert np.array_equal(a, b)
        assert sessions[0].counts() == sessions[1].counts()
    finally:
        for s in sessions:
            s.close()


def test_incremental_loop_with_gpu_ranking(gpu_ctx):
    """The reference's loop on a 25-view scene with every view chosen on the GPU: corr_2d3d over the session's graph ->
    rank (MatchDensity, 30) -> scene pose in PnP's place -> BaSession.attach (step 1) -> BaSession.triangulate (step 3) ->
    validity -> solve -> validity -> remove_outliers.  A host run of the same loop over the transcriptions chooses the same
    view and builds the same graph at every step; the loop stops cleanly when no candidate qualifies."""
    n = 25
    L = tri_ref.loop_containers(n, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    co, ids, fm, im = L["coords"], L["landmark_ids"], L["feature_matches"], L["img_matches"]
    shape = {i: nr.SHAPE for i in range(n)}
    _upload_coords(gpu_ctx, co)
    nextview.upload_feature_matches(gpu_ctx, nr.canonical_lists(fm), mirror=True)
    ses = ba.BaSession(gpu_ctx)
    lms = []
    cam_of = {}

    def poses34():
        return ba.poses34_from_angle_axis(ses.cameras()[0])

    def register(v):
        cam_of[v] = ses.add_camera(L["poses6"][v], L["intrinsics"][v])

    def add_tracks(tracks):
        off, cam, xy = tri.tracks_to_arrays(tracks, cam_of, co)
        st, first, added = ses.triangulate(off, cam, xy, poses34=poses34())
        acc = np.flatnonzero(st == 0)
        for k, j in enumerate(acc):
            for i, f in tracks[j]:
                ids[i][f] = first + k
            lms.append({"track": list(tracks[j])})

    def sync_mirror(strict=False):
        pt, cam, xy = ses.graph()
        for j, lm in enumerate(lms):
            mine = [(c, x, y) for c, (x, y) in zip(cam[pt == j], xy[pt == j])]
            kept, q = [], 0
            for i, f in lm["track"]:
                if q < len(mine) and mine[q] == (cam_of[i], *co[i][f]):
                    kept.append((i, f)); q += 1
            assert q == len(mine) and (not strict or len(kept) == len(lm["track"]))
            lm["track"] = kept

    chosen = []
    try:
        register(0)
        register(1)
        add_tracks(tri.initial_pair_tracks(fm[(0, 1)], 0, 1))
        registered = [(1, True), (0, True)]
        while len(cam_of) < n:
            cand = [i for i in range(n) if i not in cam_of]
            tracks = [lm["track"] for lm in lms]
            coff, lmk, ftr, cells, _ = nextview.corr_2d3d(gpu_ctx, *nextview.graph_arrays(tracks), cand, [shape[c] for c in cand])
            order = nextview.rank_next_images(cand, np.diff(coff), cells, nextview.MATCH_DENSITY, 30)
            lids, fids = nr.literal_calc_2d3d_matches(cand, im, fm, ids, tracks)                  # the host run
            sc = [nr.literal_density(fids[c], co[c], shape[c]) for c in cand]
            assert sc == cells.tolist()
            assert order == nextview.rank_next_images(cand, [len(lids[c]) for c in cand], sc)
            ref = nr.literal_rank(lids, fids, "density", co, shape, 30)
            if not order:
                assert not ref
                break
            v = order[0]
            if sc.count(max(sc)) == 1:
                assert v == ref[0]
            k = cand.index(v)
            assert lmk[coff[k]:coff[k + 1]].tolist() == lids[v] and ftr[coff[k]:coff[k + 1]].tolist() == fids[v]
            chosen.append(v)
            register(v)                                                    # PnP's place: the scene pose
            P = poses34()
            X = ses.points()
            xy = [co[v][g] for g in fids[v]]
            st, added = ses.attach(cam_of[v], lids[v], fids[v], xy, poses34=P)
            want = nr.literal_attach(P[cam_of[v]], L["intrinsics"][v], X, list(zip(lids[v], fids[v], xy)))
            assert st.tolist() == want and added == want.count(0)
            for e in np.flatnonzero(st == 0):
                lms[lids[v][e]]["track"].append((v, fids[v][e]))
                ids[v][fids[v][e]] = lids[v][e]
            sync_mirror(strict=True)                                       # the session graph is the mirror's, in order
            add_tracks(tri.new_view_tracks(v, ids, registered, im, fm))
            registered.append((v, True))
            ses.validity()
            ses.solve()
            ses.validity()
            sync_mirror()
            new_idx, _ = ses.remove_outliers()
            lms[:] = [lm for j, lm in enumerate(lms) if new_idx[j] >= 0]
            for i in ids:
                ids[i] = [int(new_idx[l]) if l >= 0 else -1 for l in ids[i]]
        assert len(chosen) >= 15 and len(set(chosen)) == len(chosen)
        assert ses.counts()[1] > 500
    finally:
        ses.close()
