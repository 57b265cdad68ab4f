"""GPU suite: batched multi-view triangulation (rcn_triangulate*, csrc/triangulate.hip) against the canonical restatement
of its arithmetic (bit for bit) and numpy's SVD (to rounding), each acceptance rule on its own, the argument checks, the
device and session entries, and the reference's incremental loop with every landmark created by the kernel."""
import os

import numpy as np
import pytest

import tri_ref
from oracle import orc_ba
from reconstructor_amd import _lib, ba
from reconstructor_amd import triangulate as tri

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "triangulate_small.npz")
K0 = [600.0, 600.0, 256.0, 168.0, 0.0, 0.0]
FLAT = ("poses34", "intrinsics", "trk_off", "obs_cam", "obs_xy")


def _flat(c):
    return {k: c[k] for k in FLAT}


def _same_as_canonical(ctx, c):
    xyz, st = tri.triangulate_tracks(ctx, **_flat(c))
    x0, s0 = tri_ref.canonical_tracks(**_flat(c))
    assert np.array_equal(st, s0)
    assert xyz.tobytes() == x0.tobytes()
    return xyz, st


def test_golden_fixture(gpu_ctx):
    g = np.load(GOLD)
    xyz, st = tri.triangulate_tracks(gpu_ctx, **{k: g[k] for k in FLAT})
    assert np.array_equal(st, g["status"])
    assert xyz.tobytes() == g["xyz"].tobytes()


@pytest.mark.parametrize("n_cams,n_tracks,lo,hi,seed", [(25, 4096, 2, 2, 11), (40, 20000, 2, 16, 12), (64, 1, 64, 64, 13)])
def test_seeded_sets_bit_exact(gpu_ctx, n_cams, n_tracks, lo, hi, seed):
    c = tri_ref.make_tracks(n_cams, n_tracks, lo, hi, seed=seed, defect_rate=0.1 if n_tracks > 1 else 0.0, distortion=n_tracks > 1)
    xyz, st = _same_as_canonical(gpu_ctx, c)
    x1, s1 = tri_ref.numpy_tracks(**_flat(c))
    ok = (st == 0) & (s1 == 0)
    assert ok.sum() >= max(1, 0.3 * n_tracks)
    assert np.all(np.abs(xyz[ok] - x1[ok]) <= 1e-9 * np.abs(x1[ok]).max(1, keepdims=True))
    if n_tracks > 1:
        assert (st != s1).mean() < 1e-3


def _look_at_x(theta, Z=5.0):
    """[R | t] of a camera on the circle of radius Z around X = (0, 0, Z) through the origin, at angle theta, looking at X
    (X then projects to the principal point, (256, 168) with K0)."""
    s, c = np.sin(theta), np.cos(theta)
    R = np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])
    C = np.array([Z * s, 0.0, Z - Z * c])
    return np.concatenate([R, (-R @ C)[:, None]], 1).reshape(-1)


def _case(poses, xy, cams=None):
    poses = np.array(poses, np.float64).reshape(-1, 12)
    cams = np.arange(len(xy)) if cams is None else np.asarray(cams)
    return {"poses34": poses, "intrinsics": np.tile(K0, (len(poses), 1)), "trk_off": np.array([0, len(xy)], np.int32),
            "obs_cam": cams.astype(np.int32), "obs_xy": np.array(xy, np.int32)}


def test_rule_world_z(gpu_ctx):
    # two cameras looking down -z: X = (0, 0, -5) is in front of both (depth 5) but its WORLD z is negative -> status 1
    Q0 = [-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, -1.0, 0]
    Q1 = [-1.0, 0, 0, 1.0, 0, 1.0, 0, 0, 0, 0, -1.0, 0]
    xyz, st = _same_as_canonical(gpu_ctx, _case([Q0, Q1], [(256, 168), (376, 168)]))
    assert st[0] == 1 and np.allclose(xyz[0], [0, 0, -5], rtol=1e-12)


def test_rule_reprojection_is_l1(gpu_ctx):
    poses = [_look_at_x(a) for a in np.radians([0, 10, 20, 30, 40, 50, 60, 70])] + [_look_at_x(np.radians(80))]
    xy = [(256, 168)] * 8 + [(259, 171)]                 # the last one 3 px off in u and in v: |du|, |dv| < 4 < |du| + |dv|
    c = _case(poses, xy)
    xyz, st = _same_as_canonical(gpu_ctx, c)
    assert st[0] == 2
    P = [float(v) for v in c["poses34"][8]]
    e, _ = tri_ref.reproj_l1(P, K0, list(xyz[0]), 259, 171)
    assert 4.0 < e < 8.0
    l = np.array(P).reshape(3, 4) @ np.append(xyz[0], 1.0)
    du, dv = 600 * l[0] / l[2] + 256 - 259, 600 * l[1] / l[2] + 168 - 171
    assert abs(du) < 4 and abs(dv) < 4


def test_rule_angle_pins_the_constant(gpu_ctx):
    # X = (0, 5 / 600, 5) is seen one pixel below the principal point by both cameras (pixels whose system is not exactly
    # of rank 3); an angle in [3.1415 / 180, pi / 180) rad: at least 1 "degree" with the reference's 3.1415, under 1 with pi -> accepted
    theta = 0.5 * (3.1415 / 180 + np.pi / 180)
    assert 180 * theta / 3.1415 >= 1.0 > 180 * theta / np.pi
    xyz, st = _same_as_canonical(gpu_ctx, _case([_look_at_x(0.0), _look_at_x(theta)], [(256, 169), (256, 169)]))
    assert st[0] == 0 and np.allclose(xyz[0], [0, 5 / 600, 5], atol=1e-9)
    # the same pair at 0.999 "degrees" is rejected
    xyz, st = _same_as_canonical(gpu_ctx, _case([_look_at_x(0.0), _look_at_x(0.999 * 3.1415 / 180)], [(256, 169), (256, 169)]))
    assert st[0] == 3


def test_rule_angle_every_pair(gpu_ctx):
    # pairs (0, 2), (1, 2) are 20 degrees wide, (0, 1) only 0.5: the reference rejects on ANY narrow pair
    poses = [_look_at_x(0.0), _look_at_x(np.radians(0.5)), _look_at_x(np.radians(20))]
    xyz, st = _same_as_canonical(gpu_ctx, _case(poses, [(256, 169)] * 3))
    assert st[0] == 3
    xyz, st = _same_as_canonical(gpu_ctx, _case([poses[0], poses[2]], [(256, 169)] * 2))
    assert st[0] == 0


def test_same_camera_same_pixel(gpu_ctx):
    c = _case([_look_at_x(0.0)], [(300, 200), (300, 200)], cams=[0, 0])
    xyz, st = tri.triangulate_tracks(gpu_ctx, **_flat(c))
    x0, s0 = tri_ref.canonical_tracks(**_flat(c))
    assert np.array_equal(st, s0) and st[0] != 0
    assert np.array_equal(xyz, x0, equal_nan=True)


def test_argument_errors_and_empty_batch(gpu_ctx):
    c = tri_ref.make_tracks(6, 10, 2, 3, seed=3)
    bad = dict(_flat(c)); bad["trk_off"] = c["trk_off"].copy(); bad["trk_off"][1] = bad["trk_off"][0] + 1      # 1-observation track
    with pytest.raises(_lib.RcnError) as e:
        tri.triangulate_tracks(gpu_ctx, **bad)
    assert e.value.code == -1
    bad = dict(_flat(c)); bad["obs_cam"] = c["obs_cam"].copy(); bad["obs_cam"][3] = 6                        # camera out of range
    with pytest.raises(_lib.RcnError):
        tri.triangulate_tracks(gpu_ctx, **bad)
    bad = dict(_flat(c)); bad["trk_off"] = c["trk_off"].copy(); bad["trk_off"][2] = bad["trk_off"][1] - 1    # decreasing offsets
    with pytest.raises(_lib.RcnError):
        tri.triangulate_tracks(gpu_ctx, **bad)
    xyz, st = tri.triangulate_tracks(gpu_ctx, c["poses34"], c["intrinsics"], [0], np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    assert xyz.shape == (0, 3) and st.shape == (0,)
    tri.triangulate_tracks(gpu_ctx, **_flat(c))                                                             # the ctx is still usable


def test_device_entry_and_compaction(gpu_ctx):
    import torch
    c = tri_ref.make_tracks(30, 5000, 2, 8, seed=14, defect_rate=0.2)
    xyz, st = tri.triangulate_tracks(gpu_ctx, **_flat(c))
    dx, ds, comp, cnt = tri.triangulate_tracks_device(gpu_ctx, **_flat(c), compact_first=7)
    torch.cuda.synchronize()
    dx, ds, comp, cnt = dx.cpu().numpy(), ds.cpu().numpy(), comp.cpu().numpy(), int(cnt.cpu()[0])
    assert dx.tobytes() == xyz.tobytes() and np.array_equal(ds, st)
    acc = st == 0
    assert cnt == acc.sum() and 0 < cnt < len(st)
    assert comp[7:7 + cnt].tobytes() == xyz[acc].tobytes()
    assert not comp[:7].any() and not comp[7 + cnt:].any()


def _session_with_cameras(ctx, c):
    ses = ba.BaSession(ctx)
    for p, k in zip(c["poses34"], c["intrinsics"]):
        R = p.reshape(3, 4)[:, :3]
        ses.add_camera(np.concatenate([ba._rot_to_angle_axis(R), p.reshape(3, 4)[:, 3]]), k)
    return ses


def test_session_entry_equals_host_entry_plus_adds(gpu_ctx):
    c = tri_ref.make_tracks(20, 3000, 2, 6, seed=15, defect_rate=0.2)
    s1, s2 = _session_with_cameras(gpu_ctx, c), _session_with_cameras(gpu_ctx, c)
    try:
        seed_pts = np.arange(30, dtype=np.float64).reshape(10, 3)
        for s in (s1, s2):
            s.add_points(seed_pts)
            s.add_observations(np.arange(10), np.zeros(10, np.int32), np.tile([[5, 6]], (10, 1)))
        st, first, added = s1.triangulate(c["trk_off"], c["obs_cam"], c["obs_xy"], poses34=c["poses34"])
        xyz, st2 = tri.triangulate_tracks(gpu_ctx, **_flat(c))
        acc = np.flatnonzero(st2 == 0)
        assert np.array_equal(st, st2) and first == 10 and added == len(acc)
        f2 = s2.add_points(xyz[acc])
        pt, cam, xy = [], [], []
        for k, j in enumerate(acc):
            o = np.arange(c["trk_off"][j], c["trk_off"][j + 1])
            pt += [f2 + k] * len(o); cam += list(c["obs_cam"][o]); xy += list(map(tuple, c["obs_xy"][o]))
        s2.add_observations(pt, cam, xy)
        assert s1.counts() == s2.counts()
        assert s1.points().tobytes() == s2.points().tobytes()
        for a, b in zip(s1.graph(), s2.graph()):
            assert np.array_equal(a, b)
        st0, first0, added0 = s1.triangulate([0], np.zeros(0, np.int32), np.zeros((0, 2), np.int32), poses34=c["poses34"])
        assert len(st0) == 0 and first0 == s1.counts()[1] and added0 == 0
    finally:
        s1.close(); s2.close()


def test_incremental_loop_with_kernel_landmarks(gpu_ctx):
    """The reference's loop (SequentialReconstructor.cpp:1000-1094) on a 25-view scene: the initial pair's landmarks from the
    pair's matches, every later view's from new_view_tracks after step 1, all through rcn_ba_session_triangulate; scene
    poses stand in for PnP.  Then validity -> solve -> validity -> remove_outliers; every solve equals rcn_ba_solve on the
    re-packed problem bit for bit and the CPU oracle to 1e-5 px."""
    L = tri_ref.loop_containers(25, 1500, obs_per_point=6, seed=31, wrong_rate=0.0)
    co, ids, fm, im = L["coords"], L["landmark_ids"], L["feature_matches"], L["img_matches"]
    ses = ba.BaSession(gpu_ctx)
    lms = []                                                  # mirror: {"xyz", "track": [(img, feat)]}, session order
    ident = {i: i for i in range(25)}                         # session camera index = image index (registration order)

    def poses34():
        return ba.poses34_from_angle_axis(ses.cameras()[0])

    def add_tracks(tracks):
        off, cam, xy = tri.tracks_to_arrays(tracks, ident, co)
        st, first, added = ses.triangulate(off, cam, xy, poses34=poses34())
        acc = np.flatnonzero(st == 0)
        assert added == len(acc) and first == len(lms)
        for k, j in enumerate(acc):
            for i, f in tracks[j]:
                ids[i][f] = first + k
            lms.append({"xyz": None, "track": list(tracks[j])})
        return len(acc)

    def sync_mirror():
        pt, cam, xy = ses.graph()
        X = ses.points()
        for j, lm in enumerate(lms):
            mine = [(c, x, y) for c, (x, y) in zip(cam[pt == j], xy[pt == j])]
            kept, q = [], 0
            for i, f in lm["track"]:
                if q < len(mine) and mine[q] == (i, *co[i][f]):
                    kept.append((i, f)); q += 1
            assert q == len(mine)
            lm["track"], lm["xyz"] = kept, list(X[j])

    try:
        ses.add_camera(L["poses6"][0], L["intrinsics"][0])
        ses.add_camera(L["poses6"][1], L["intrinsics"][1])
        assert add_tracks(tri.initial_pair_tracks(fm[(0, 1)], 0, 1)) > 50
        registered = [(1, True), (0, True)]
        for v in range(2, 25):
            ses.add_camera(L["poses6"][v], L["intrinsics"][v])          # PnP's place: the scene pose
            sync_mirror()
            P = dict(enumerate(poses34()))
            K = {i: L["intrinsics"][i] for i in range(v + 1)}
            fids, lids = tri_ref.calc_2d3d_matches(v, im, fm, ids, lms)
            before = [len(lm["track"]) for lm in lms]
            tri_ref.sequential_matched_landmarks(v, fids, lids, [], im, fm, co, ids, lms, P, K)     # step 1, on the host
            new = [(j, f) for j, lm in enumerate(lms) for (i, f) in lm["track"][before[j]:]]
            if new:
                ses.add_observations([j for j, _ in new], [v] * len(new), [co[v][f] for _, f in new])
            add_tracks(tri.new_view_tracks(v, ids, registered, im, fm))                             # step 3, one launch
            registered.append((v, True))
            n = v + 1
            ses.validity()
            poses, intr = ses.cameras()
            pt, cam, xy = ses.graph()
            X = ses.points()
            flat = {"poses": poses, "intrinsics": intr, "points": X, "obs_uv": xy.astype(np.float64), "obs_cam": cam, "obs_pt": pt}
            P1, I1, X1, s1 = ba.solve_scene(gpu_ctx, flat)
            P0, I0, X0, s0 = orc_ba.solve(flat, threads=4)
            s2 = ses.solve()
            P2, I2 = ses.cameras()
            X2 = ses.points()
            assert P2.tobytes() == P1.tobytes() and I2.tobytes() == I1.tobytes() and X2.tobytes() == X1.tobytes()
            assert s2["iterations"] == s1["iterations"] and np.array_equal(s2["cost_trace"], s1["cost_trace"])
            assert s2["iterations"] == s0["iterations"] and s2["termination"] == s0["termination"]
            assert abs(s2["final_rms_px"] - s0["final_rms_px"]) <= 1e-5
            assert ses.counts()[0] == n
            ses.validity()
            sync_mirror()
            new_idx, _ = ses.remove_outliers()
            lms[:] = [lm for j, lm in enumerate(lms) if new_idx[j] >= 0]
            for i in ids:
                ids[i] = [int(new_idx[l]) if l >= 0 else -1 for l in ids[i]]
        assert ses.counts()[1] > 500
    finally:
        ses.close()
