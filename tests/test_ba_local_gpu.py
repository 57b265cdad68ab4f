"""GPU suite: local bundle adjustment on a session (rcn_ba_session_solve_local, rcn_ba_session_covisible; csrc/ba_local.hip).

Held against: the session's own global solve (every camera free: the extraction is the identity), rcn_ba_solve_constant on the
sub-problem packed on the host by the numpy restatement of tests/ba_local_ref.py (bit for bit: pins the order and the indices of the
device extraction), the judge's record (tests/golden/ba_local_judge.npz), and the all-global incremental loop."""
import ctypes as C

import numpy as np
import pytest

import ba_graphs
import ba_local_ref as L
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu

COUNTERS = ("iterations", "successful_steps", "unsuccessful_steps", "invalid_steps", "termination", "line_search_backtracks",
            "bound_projections", "reduced_dim", "initial_cost", "final_cost")


def _session(ctx, sc, poses=None, intr=None, points=None):
    from reconstructor_amd import ba
    ses = ba.BaSession(ctx)
    for p, k in zip(sc["poses"] if poses is None else poses, sc["intrinsics"] if intr is None else intr):
        ses.add_camera(p, k)
    ses.add_points(sc["points"] if points is None else points)
    ses.add_observations(sc["obs_pt"], sc["obs_cam"], np.asarray(sc["obs_uv"]).astype(np.int32))
    return ses


def _state(ses):
    P, I = ses.cameras()
    pt, cam, xy = ses.graph()
    return dict(poses=P, intrinsics=I, points=ses.points(), obs_pt=pt, obs_cam=cam, obs_uv=xy.astype(np.float64))


def _options(ctx, n, **kw):
    from reconstructor_amd import ba
    o = ba.default_options(ctx, n)
    o.fix_cam0_pose = o.fix_cam1_translation = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _same_summary(a, b):
    return all(a[k] == b[k] for k in COUNTERS) and np.array_equal(a["cost_trace"], b["cost_trace"])


def _local_against_host_packing(ctx, ses, free, o):
    """solve_local, and rcn_ba_solve_constant on the sub-problem the restatement packs from the state before: equal bits; everything
    outside the sub-problem untouched.  Returns (state before, state after, extraction, summary)."""
    from reconstructor_amd import ba
    before = _state(ses)
    nc = len(before["poses"])
    fm = L.mask(nc, free)
    sub, e = L.sub_scene(before["poses"], before["intrinsics"], before["points"], before["obs_uv"], before["obs_pt"], before["obs_cam"], fm)
    counts = ses.counts()
    s, info = ses.solve_local(free, o)
    assert info == dict(n_cams=len(e["cam_map"]), n_constant=int(e["constant"].sum()), n_points=len(e["pt_map"]), n_obs=len(e["obs"]))
    P1, I1, X1, s1 = ba.solve_scene(ctx, sub, o, constant=e["constant"])
    after = _state(ses)
    assert _same_summary(s, s1)
    fl = ~e["constant"]
    assert after["poses"][e["cam_map"][fl]].tobytes() == P1[fl].tobytes() and after["intrinsics"][e["cam_map"][fl]].tobytes() == I1[fl].tobytes()
    assert after["points"][e["pt_map"]].tobytes() == X1.tobytes()
    moved = np.zeros(nc, bool)
    moved[e["cam_map"][fl]] = True
    assert after["poses"][~moved].tobytes() == before["poses"][~moved].tobytes() and after["intrinsics"][~moved].tobytes() == before["intrinsics"][~moved].tobytes()
    assert after["points"][~e["sel"]].tobytes() == before["points"][~e["sel"]].tobytes()
    assert ses.counts() == counts
    for k in ("obs_pt", "obs_cam", "obs_uv"):
        assert np.array_equal(after[k], before[k])
    return before, after, e, s


@pytest.mark.parametrize("nc,npts", [(6, 150), (12, 2500)])
def test_all_cameras_free_is_the_global_session_solve(gpu_ctx, nc, npts):
    """Every landmark has an observation and every camera is free: the extraction is the identity.  12 x 2500: more than 1024 landmarks
    and more than 4096 observations, so every run of the one-workgroup scans crosses thread and wave boundaries inside tracks."""
    sc = ba_graphs.graph_scene(nc, npts, 40 + nc, lengths=[2, 3, 4, nc])
    assert np.diff(sc["pt_off"]).min() >= 2 and (npts < 1024 or len(sc["obs_pt"]) > 4096)
    a, b = _session(gpu_ctx, sc), _session(gpu_ctx, sc)
    try:
        sa = a.solve()
        sb, info = b.solve_local(np.arange(nc)[::-1].copy())       # any order
        assert info == dict(n_cams=nc, n_constant=0, n_points=npts, n_obs=len(sc["obs_pt"]))
        assert _same_summary(sa, sb) and sa["final_cost"] < sa["initial_cost"]
        for x, y in zip(a.cameras() + (a.points(),), b.cameras() + (b.points(),)):
            assert x.tobytes() == y.tobytes()
    finally:
        a.close(); b.close()


def test_extraction_on_a_ragged_session(gpu_ctx):
    """Empty tracks (from the scene, and from a validity sweep that erases), landmarks seen only by cameras that are not free, a free
    camera without observations (12), a camera that sees no selected landmark (13), landmarks that see one camera twice."""
    from reconstructor_amd import ba
    sc = ba_graphs.graph_scene(12, 400, 21, lengths=[0, 1, 2, 3, 4], repeat=0.3)
    ses = _session(gpu_ctx, sc)
    try:
        ses.add_camera(sc["poses"][3] + 0.01, sc["intrinsics"][3])          # 12: no observation
        ses.add_camera(sc["poses"][0] + 0.01, sc["intrinsics"][0])          # 13: sees only the six landmarks below, with camera 0
        first = ses.add_points(sc["points"][:6] + 0.5)
        lm = np.repeat(np.arange(first, first + 6), 2)
        ses.add_observations(lm, np.tile([13, 0], 6), np.tile([[100, 90], [120, 80]], (6, 1)))
        _, erased = ses.validity(max_err=3.0)
        st = _state(ses)
        k = np.bincount(st["obs_pt"], minlength=406)
        print("validity sweep: %d observations erased, %d empty tracks (%d before it)" % (erased, (k == 0).sum(), (np.diff(sc["pt_off"]) == 0).sum()))
        assert erased > 0 and (k == 0).any()
        free = [9, 12, 4]
        e = L.extract(L.mask(14, free), 406, st["obs_pt"], st["obs_cam"])
        assert 13 not in e["cam_map"] and 12 not in e["cam_map"] and 0 in e["cam_map"] and e["constant"].sum() >= 2
        assert (~e["sel"] & (k > 0)).any() and (~e["sel"] & (k == 0)).any()
        key = st["obs_pt"][e["obs"]].astype(np.int64) * 14 + st["obs_cam"][e["obs"]]
        assert len(np.unique(key)) < len(key)                               # a selected landmark sees a camera twice
        _local_against_host_packing(gpu_ctx, ses, free, _options(gpu_ctx, 3))
        _local_against_host_packing(gpu_ctx, ses, [0, 13], _options(gpu_ctx, 2))          # again on what the first left, another window
        s, info = ses.solve_local(free)                                     # options NULL: rcn_ba_default_options(3)
        assert s["reduced_dim"] == 12 and info["n_constant"] >= 2
    finally:
        ses.close()


def test_a_window_of_three_in_twelve(gpu_ctx):
    from reconstructor_amd import ba
    nc, npts, seed, const = L.MANY_CONSTANT[2]                              # cameras 3 .. 11 constant: 0, 1, 2 free
    sc = L.scene(nc, npts, seed)
    Pj, Xj, rj, (s_rms, s_pose, s_pts) = L.recorded(nc, npts, seed, const)
    ses = _session(gpu_ctx, sc)
    try:
        # two global solves of no iteration first (the state stays the scene's start, which is the judge's start): the ctx then holds this
        # session's pair lists under its token, as the second one shows
        none = _options(gpu_ctx, nc, intrinsics_mode=0, max_iterations=0)
        g0, g00 = ses.solve(none), ses.solve(none)
        assert g0["iterations"] == 0 and (g0["pair_lists_reused"], g00["pair_lists_reused"]) == (0, 1)
        assert ses.cameras()[0].tobytes() == sc["poses"].tobytes() and ses.points().tobytes() == sc["points"].tobytes()
        o = _options(gpu_ctx, 3, max_iterations=150, **L.TO_THE_END)
        before, after, e, s = _local_against_host_packing(gpu_ctx, ses, [2, 0, 1], o)
        assert e["constant"].tolist() == [False] * 3 + [True] * 9 and s["reduced_dim"] == 18
        # the judge frees the same three cameras over ALL observed points; the points the window does not see decouple from it
        sub = {"poses": Pj, "intrinsics": sc["intrinsics"], "points": Xj, "obs_uv": sc["obs_uv"][e["obs"]], "obs_cam": sc["obs_cam"][e["obs"]], "obs_pt": sc["obs_pt"][e["obs"]]}
        d_rms = abs(s["final_rms_px"] - L.rms(sub))
        d_pose, d_pts = np.abs(after["poses"] - Pj).max(), np.abs(after["points"] - Xj)[e["sel"]].max()
        print("window (0, 1, 2) of 12: %d iterations, termination %d; against the judge: rms %.2e px, poses %.2e (margin %.2e), points %.2e (margin %.2e)" %
              (s["iterations"], s["termination"], d_rms, d_pose, max(100 * s_pose, 1e-9), d_pts, max(100 * s_pts, 1e-9)))
        assert d_rms <= 1e-5 and d_pose <= max(100 * s_pose, 1e-9) and d_pts <= max(100 * s_pts, 1e-9)
        # the global solve behind it rebuilds its pair lists (the local solve left the ctx without a token) and is a fresh session's
        g1 = ses.solve()
        fresh = _session(gpu_ctx, sc, after["poses"], after["intrinsics"], after["points"])
        try:
            g2 = fresh.solve()
            assert g1["pair_lists_reused"] == 0 and _same_summary(g1, g2)
            for x, y in zip(ses.cameras() + (ses.points(),), fresh.cameras() + (fresh.points(),)):
                assert x.tobytes() == y.tobytes()
        finally:
            fresh.close()
    finally:
        ses.close()


def test_covisible(gpu_ctx):
    from reconstructor_amd import ba
    sc = ba_graphs.graph_scene(12, 400, 21, lengths=[0, 1, 2, 3, 4], repeat=0.3)
    assert ba_graphs.repeated_second(sc).any()
    ses = _session(gpu_ctx, sc)
    try:
        for cam in (0, 7, 11):
            want = L.covisible_counts(12, 400, sc["obs_pt"], sc["obs_cam"], cam)
            for k in (0, 3, 50):
                got, counts = ses.covisible(cam, k)
                assert np.array_equal(counts, want) and np.array_equal(got, L.covisible_pick(want, cam, k))
            assert want[cam] == len(np.unique(sc["obs_pt"][sc["obs_cam"] == cam]))
    finally:
        ses.close()
    # ties to the lower index, fewer sharing cameras than k, a camera without a landmark: the hand-made graph of tests/test_ba_local_ref.py
    tracks = [(2, 0), (), (3, 4), (4, 2, 4), (1,), (0, 3), (2, 3, 2), (2, 4)]
    ses = ba.BaSession(gpu_ctx)
    try:
        for c in range(6):
            ses.add_camera(sc["poses"][c], sc["intrinsics"][c])
        ses.add_points(sc["points"][:8])
        pt = np.repeat(np.arange(8), [len(t) for t in tracks])
        cam = np.concatenate([np.array(t, np.int32) for t in tracks])
        ses.add_observations(pt, cam, np.arange(2 * len(pt)).reshape(-1, 2))
        got, counts = ses.covisible(2, 5)
        assert counts.tolist() == [1, 0, 4, 1, 2, 0] and got.tolist() == [4, 0, 3]
        assert ses.covisible(2, 1)[0].tolist() == [4] and ses.covisible(2, 0)[0].tolist() == []
        got, counts = ses.covisible(5, 3)
        assert counts.tolist() == [0] * 6 and got.tolist() == []
    finally:
        ses.close()


def test_argument_errors_leave_the_session_usable(gpu_ctx):
    from reconstructor_amd import _lib, ba
    sc = L.scene(6, 120, 1)
    ses = _session(gpu_ctx, sc)
    try:
        ses.add_camera(sc["poses"][0], sc["intrinsics"][0])                 # 6: no observation
        before = _state(ses)
        bad = [lambda: ses.solve_local([]), lambda: ses.solve_local([1, 7]), lambda: ses.solve_local([-1]), lambda: ses.solve_local([2, 3, 2]),
               lambda: ses.solve_local([6]), lambda: ses.covisible(7, 2), lambda: ses.covisible(-1, 2), lambda: ses.covisible(1, -1)]
        for f in bad:
            with pytest.raises(_lib.RcnError) as e:
                f()
            assert e.value.code == -1 and len(str(e.value)) > 25, str(e.value)
        s = _lib.BaSummary()
        assert gpu_ctx.lib.rcn_ba_session_solve_local(ses.h, None, 2, None, C.byref(s), None) == -1      # a null list
        after = _state(ses)
        assert all(after[k].tobytes() == before[k].tobytes() for k in before)
        s, info = ses.solve_local([1, 2], _options(gpu_ctx, 2))
        assert s["final_cost"] < s["initial_cost"] and info["n_cams"] == 6 and info["n_constant"] == 4
    finally:
        ses.close()


def _grow(ses, sc, n, live, sid):
    """Camera n - 1 with what registering it adds (tests/test_ba_session_gpu.py's loop, no sweeps)."""
    xy_all = sc["obs_uv"].astype(np.int32)
    ses.add_camera(sc["poses"][n - 1], sc["intrinsics"][n - 1])
    cnt = np.bincount(sc["obs_pt"][sc["obs_cam"] < n], minlength=len(sc["points"]))
    live_now = cnt >= 2
    new_pts = np.flatnonzero(live_now & ~live)
    o_new = np.flatnonzero((sc["obs_cam"] == n - 1) & live[sc["obs_pt"]])
    ses.add_observations([sid[j] for j in sc["obs_pt"][o_new]], sc["obs_cam"][o_new], xy_all[o_new])
    if len(new_pts):
        first = ses.add_points(sc["points"][new_pts])
        for k, j in enumerate(new_pts):
            sid[j] = first + k
        o_tr = np.flatnonzero(np.isin(sc["obs_pt"], new_pts) & (sc["obs_cam"] < n))
        ses.add_observations([sid[j] for j in sc["obs_pt"][o_tr]], sc["obs_cam"][o_tr], xy_all[o_tr])
    return live_now


def test_reference_loop_with_local_adjustments(gpu_ctx):
    """3 -> 25 cameras (tests/test_cfg1_plumbing.py's scene): a local adjustment (the new view + its 5 most covisible) after every view
    against a global one after every view; both loops end in a tight global solve of the same graph.  No validity sweeps, so the
    graphs are the same.  As IncrementalBundleAdjuster::adjustLocal does, cameras 0 and 1 are never freed with a window: every global
    solve holds camera 0's pose and camera 1's translation AT THEIR CURRENT VALUES, so a local solve that moved them would change the
    constants of the final solve, and the two loops would minimise different functions (measured that way: 0.696263 px against
    0.696191 px, the cost falling monotonically along the segment between the two end points)."""
    from reconstructor_amd import ba
    sc = synth_ba.make_scene(25, 1500, obs_per_point=6, seed=31)
    final = {}
    for how in ("global", "local"):
        ses = ba.BaSession(gpu_ctx)
        try:
            live, sid, n_local = np.zeros(len(sc["points"]), bool), {}, 0
            for n in range(1, 26):
                live = _grow(ses, sc, n, live, sid)
                if n < 3:
                    continue
                near = ses.covisible(n - 1, 5)[0] if how == "local" else []
                if how == "global" or len(near) + 1 == n:
                    ses.solve()
                else:
                    free = np.concatenate([[n - 1], near[near >= 2]])      # cameras 0 and 1 hold the frame of every global solve: never freed
                    s, info = ses.solve_local(free, _options(gpu_ctx, len(free)))
                    assert info["n_cams"] - info["n_constant"] == len(free) >= 4 and s["final_cost"] <= s["initial_cost"]
                    n_local += 1
            o = ba.default_options(gpu_ctx, 25)
            o.max_iterations = 150
            for k, v in L.TIGHT.items():
                setattr(o, k, v)
            final[how] = (ses.solve(o), ses.graph(), n_local)
            again = ses.solve(o)
            print("%s loop: tight global solve %d iterations, termination %d, rms %.9f -> %.9f px; the same solve again: %d iterations, termination %d, rms %.9f px" %
                  (how, final[how][0]["iterations"], final[how][0]["termination"], final[how][0]["initial_rms_px"], final[how][0]["final_rms_px"],
                   again["iterations"], again["termination"], again["final_rms_px"]))
        finally:
            ses.close()
    (sg, gg, _), (sl, gl, n_local) = final["global"], final["local"]
    assert n_local >= 15 and all(np.array_equal(a, b) for a, b in zip(gg, gl))
    print("final rms: all-global loop %.9f px, local loop %.9f px (difference %.2e; %d local solves)" %
          (sg["final_rms_px"], sl["final_rms_px"], abs(sg["final_rms_px"] - sl["final_rms_px"]), n_local))
    assert abs(sg["final_rms_px"] - sl["final_rms_px"]) <= 1e-5
