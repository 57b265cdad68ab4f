"""GPU suite: shared intrinsics of the bundle adjuster -- cameras tied in groups (rcn_ba_solve_tied, rcn_ba_session_set_groups;
csrc/ba_tied.h, csrc/ba_tied.hip).

Held against: rcn_ba_solve_constant (no live group: bit for bit), itself (a second run, a session, the members of a group: bit for
bit), and the judge of tests/ba_tied_ref.py, whose results on the cases below are read from tests/golden/ba_tied_judge.npz
(tests/test_ba_tied_ref.py holds the record against a fresh run of the judge):
  the first step   x_out - x_in of a solve with max_iterations = 1 against one LM step in long double with one parameter block per
                   group: |D - d_ref| <= 16 max(|d_f64 - d_ref|, u |d_ref|) + 2 u |x|, cameras and landmarks apart (2-norms;
                   tests/test_ba_step_gpu.py's rule plus the rounding of the subtraction);
  the minimum      RMS, poses, shared intrinsics and points against scipy's minimum, with the margins tests/test_ba_constant_gpu.py
                   uses: 1e-5 px, and 100 x what the judge's two minimisers differ by (floor 1e-9).
Every check prints its figures before it asserts (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import ba_graphs
import ba_local_ref as L
import ba_tied_ref as T
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
COUNTERS = ("iterations", "successful_steps", "unsuccessful_steps", "invalid_steps", "termination", "line_search_backtracks",
            "bound_projections", "reduced_dim", "initial_cost", "final_cost")


def _options(ctx, nc, mode=1, fix=(1, 1), max_iterations=None, **tol):
    from reconstructor_amd import ba
    o = ba.default_options(ctx, nc)
    o.intrinsics_mode, o.fix_cam0_pose, o.fix_cam1_translation = mode, fix[0], fix[1]
    if max_iterations:
        o.max_iterations = max_iterations
    for k, v in tol.items():
        setattr(o, k, v)
    return o


def _entry(ctx, sc, o, mask, groups, tied=True):
    """rcn_ba_solve_tied (or rcn_ba_solve_constant) called directly: None is a NULL pointer.  Returns (P, I, X, summary, status)."""
    from reconstructor_amd import _lib, ba
    P, I, X = (np.array(sc[k], np.float64, order="C") for k in ("poses", "intrinsics", "points"))
    uv, cam, pt = np.ascontiguousarray(sc["obs_uv"], np.float64), np.ascontiguousarray(sc["obs_cam"], np.int32), np.ascontiguousarray(sc["obs_pt"], np.int32)
    pb = _lib.BaProblem(len(P), len(X), len(cam), 0, P.ctypes.data, I.ctypes.data, X.ctypes.data, uv.ctypes.data, cam.ctypes.data, pt.ctypes.data)
    s = _lib.BaSummary()
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    g = None if groups is None else np.ascontiguousarray(groups, np.int32)
    mp, gp = (m.ctypes.data if m is not None else None), (g.ctypes.data if g is not None else None)
    if tied:
        rc = ctx.lib.rcn_ba_solve_tied(ctx.h, C.byref(pb), C.byref(o), None, mp, gp, C.byref(s), None, None)
    else:
        rc = ctx.lib.rcn_ba_solve_constant(ctx.h, C.byref(pb), C.byref(o), None, mp, C.byref(s), None, None)
    return P, I, X, ba.summary_dict(s), rc


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and all(a[3][k] == b[3][k] for k in COUNTERS) and \
        np.array_equal(a[3]["cost_trace"], b[3]["cost_trace"])


def _members_identical(I, groups):
    g = np.asarray(groups)
    return all(I[g == k].tobytes() == np.tile(I[g == k][0], ((g == k).sum(), 1)).tobytes() for k in np.unique(g[g >= 0]))


# ---------------------------------------------------------------------------------------------------------------- 1. equivalences
@pytest.mark.parametrize("how", ["null", "all_minus_one", "singletons", "groups_in_mode_0"])
def test_no_live_group_is_rcn_ba_solve_constant_bit_for_bit(gpu_ctx, how):
    sc, kw = T.case("mixed_12")
    mask = np.zeros(12, np.uint8)
    mask[7] = 1
    o = _options(gpu_ctx, 12, mode=0 if how == "groups_in_mode_0" else 1)
    groups = {"null": None, "all_minus_one": np.full(12, -1), "singletons": np.arange(12)[::-1].copy() + 3, "groups_in_mode_0": kw["groups"]}[how]
    ref = _entry(gpu_ctx, sc, o, mask, None, tied=False)
    got = _entry(gpu_ctx, sc, o, mask, groups)
    assert ref[4] == 0 and got[4] == 0 and ref[3]["final_cost"] < ref[3]["initial_cost"]
    assert _same_bits(ref, got)


def test_a_tied_solve_twice_and_its_members(gpu_ctx):
    sc, kw = T.case("mixed_12")
    o = _options(gpu_ctx, 12)
    a = _entry(gpu_ctx, sc, o, None, kw["groups"])
    b = _entry(gpu_ctx, sc, o, None, kw["groups"])
    u = _entry(gpu_ctx, sc, o, None, None)
    assert a[4] == 0 and _same_bits(a, b)
    assert _members_identical(a[1], kw["groups"]) and not _members_identical(u[1], kw["groups"])
    assert a[3]["reduced_dim"] == 6 * 12 - 9 + 4 * 4 + 8 and u[3]["reduced_dim"] == 6 * 12 - 9 + 4 * 12
    assert a[3]["final_cost"] < 0.1 * a[3]["initial_cost"]
    free = np.asarray(kw["groups"]) < 0
    assert not np.array_equal(a[1][~free][:, [0, 1, 4, 5]], sc["intrinsics"][~free][:, [0, 1, 4, 5]])      # the shared intrinsics moved
    assert a[1][:, 2:4].tobytes() == sc["intrinsics"][:, 2:4].tobytes()                                       # cx, cy: constant


def _session(ctx, sc):
    from reconstructor_amd import ba
    ses = ba.BaSession(ctx)
    for p, k in zip(sc["poses"], sc["intrinsics"]):
        ses.add_camera(p, k)
    ses.add_points(sc["points"])
    ses.add_observations(sc["obs_pt"], sc["obs_cam"], np.asarray(sc["obs_uv"]).astype(np.int32))
    return ses


def test_a_session_with_groups_is_the_flat_tied_solve(gpu_ctx):
    from reconstructor_amd import ba
    sc, kw = T.case("mixed_12")
    o = _options(gpu_ctx, 12)
    ref = ba.solve_scene(gpu_ctx, sc, o, groups=kw["groups"])
    ses = _session(gpu_ctx, sc)
    try:
        ses.set_groups(kw["groups"])
        s = ses.solve(o)
        P, I = ses.cameras()
        X = ses.points()
    finally:
        ses.close()
    assert _same_bits(ref, (P, I, X, s))


# ---------------------------------------------------------------------------------------------------------------- 2. the first step
def _norm(v):
    return float(np.sqrt((np.asarray(v, np.float64) ** 2).sum()))


@pytest.mark.parametrize("name", list(T.CASES))
def test_the_first_step_against_long_double(gpu_ctx, name):
    from reconstructor_amd import ba
    c = T.CASES[name]
    sc, kw = T.case(name)
    rec = T.recorded(name)
    o = _options(gpu_ctx, c["nc"], fix=kw["fix"], max_iterations=1, focal_upper_bound=c.get("ub", 1000.0))
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, o, constant=kw["constant"], groups=kw["groups"], loss=c.get("loss"))
    assert s["successful_steps"] == 1 and s["line_search_backtracks"] == 0, "the case must take its first step whole: %r" % (s,)
    seen = np.zeros(len(X), bool)
    seen[sc["obs_pt"]] = True
    cams = (np.concatenate([P - sc["poses"], I - rec["I0"]], 1), np.concatenate([rec["dP"], rec["dI"]], 1), np.concatenate([rec["eP"], rec["eI"]], 1),
            np.concatenate([sc["poses"], rec["I0"]], 1))
    pts = ((X - sc["points"])[seen], rec["dX"][seen], rec["eX"][seen], sc["points"][seen])
    for tag, (d, ref, e64, x) in (("cameras", cams), ("landmarks", pts)):
        err, bound = _norm(d - ref), 16 * max(_norm(e64), U * _norm(ref)) + 2 * U * _norm(x)
        print("%s %s: |step| %.3e, error %.3e, bound %.3e, ratio %.3g" % (name, tag, _norm(ref), err, bound, err / bound))
        assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- 3. to the minimum
@pytest.mark.parametrize("name", list(T.CASES))
def test_to_the_minimum_against_the_judge(gpu_ctx, name):
    from reconstructor_amd import ba
    c = T.CASES[name]
    nc = c["nc"]
    sc, kw = T.case(name)
    rec = T.recorded(name)
    s_rms, s_pose, s_intr, s_pts = (float(v) for v in rec["spread"])
    o = _options(gpu_ctx, nc, fix=kw["fix"], max_iterations=150, focal_upper_bound=c.get("ub", 1000.0), **L.TO_THE_END)
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, o, constant=kw["constant"], groups=kw["groups"], loss=c.get("loss"), report=True)
    seen = np.zeros(len(X), bool)
    seen[sc["obs_pt"]] = True
    st = T.structure(nc, kw["groups"], kw["constant"], 1, kw["fix"])
    rms = s["loss_report"]["plain_rms_px"]
    d_rms, d_pose, d_intr, d_pts = abs(rms - float(rec["rms"])), np.abs(P - rec["P"]).max(), np.abs(I - rec["I"]).max(), np.abs(X - rec["X"])[seen].max()
    print("%s: n' = %d, %d iterations, termination %d, rms %.6f px; against the judge: rms %.2e px, poses %.2e (margin %.2e), intrinsics %.2e (margin %.2e), "
          "points %.2e (margin %.2e)" % (name, s["reduced_dim"], s["iterations"], s["termination"], rms, d_rms, d_pose, max(100 * s_pose, 1e-9), d_intr,
                                         max(100 * s_intr, 1e-9), d_pts, max(100 * s_pts, 1e-9)))
    assert s["reduced_dim"] == st["n_tied"] == {"one_group_12": 67, "one_group_20": 115, "exactly_128": 128, "n_138": 138, "two_groups_66": 395}.get(name, st["n_tied"])
    assert _members_identical(I, kw["groups"])
    m = kw["constant"]
    assert P[m].tobytes() == sc["poses"][m].tobytes() and I[m].tobytes() == sc["intrinsics"][m].tobytes()
    assert I[:, 2:4].tobytes() == sc["intrinsics"][:, 2:4].tobytes()
    if name == "held_12":      # a constant member: the intrinsics of all members come back as they went in, the poses move
        assert I.tobytes() == sc["intrinsics"].tobytes() and not np.array_equal(P[~m][1:], sc["poses"][~m][1:])
    if name == "bound_12":     # the start above the bound: projected at entry, once per tied fx, fy
        assert s["bound_projections"] == 2 and (I[:, :2] <= c["ub"]).all()
    else:
        assert s["bound_projections"] == 0
    assert d_rms <= 1e-5
    assert d_pose <= max(100 * s_pose, 1e-9) and d_intr <= max(100 * s_intr, 1e-9) and d_pts <= max(100 * s_pts, 1e-9)


# ---------------------------------------------------------------------------------------------------------------- 4. errors
def test_argument_errors_write_nothing(gpu_ctx):
    from reconstructor_amd import ba
    sc, kw = T.case("one_group_12")
    o = _options(gpu_ctx, 12)
    bad_intr = ba_graphs.copy_scene(sc)
    bad_intr["intrinsics"][5, 4] = np.nextafter(bad_intr["intrinsics"][5, 4], 1.0)      # one bit of k1 of camera 5
    below = np.array(kw["groups"])
    below[3] = -2
    for scene, groups, word in ((bad_intr, kw["groups"], "camera 5"), (sc, below, "camera 3")):
        P, I, X, s, rc = _entry(gpu_ctx, scene, o, None, groups)
        msg = gpu_ctx.lib.rcn_last_error(gpu_ctx.h).decode()
        assert rc == -1 and word in msg, (rc, msg)
        assert P.tobytes() == scene["poses"].tobytes() and I.tobytes() == scene["intrinsics"].tobytes() and X.tobytes() == scene["points"].tobytes()
    with pytest.raises(ValueError):
        ba.solve_scene(gpu_ctx, sc, o, groups=kw["groups"][:11])
    ses = _session(gpu_ctx, sc)
    try:
        for g in (kw["groups"][:11], np.append(kw["groups"], 0), below):
            with pytest.raises(Exception) as e:
                ses.set_groups(g)
            assert "rcn_ba_session_set_groups" in str(e.value)
        ses.set_groups(kw["groups"])
        assert ses.solve(o)["reduced_dim"] == 67      # the session is usable, and no refused call has changed its groups
    finally:
        ses.close()
    assert ba.solve_scene(gpu_ctx, sc, o, groups=kw["groups"])[3]["final_rms_px"] < 1.0      # the ctx is usable afterwards


# ---------------------------------------------------------------------------------------------------------------- 5. session and window
def _grow(ses, sc, n, live, sid, intr):
    """Camera n - 1 with what registering it adds (tests/test_ba_local_gpu.py's loop, no sweeps)."""
    xy_all = sc["obs_uv"].astype(np.int32)
    ses.add_camera(sc["poses"][n - 1], intr)
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


def test_the_incremental_loop_with_one_shared_camera(gpu_ctx):
    """3 -> 25 cameras (tests/test_cfg1_plumbing.py's scene), every camera in one group from the tenth view on (where the reference's
    options free the intrinsics): every session solve equals rcn_ba_solve_tied on the repacked problem, bit for bit.  A new view enters
    with the group's current intrinsics.  Then one local solve on a window whose constant cameras share the group: it is held."""
    from reconstructor_amd import ba
    sc = synth_ba.make_scene(25, 1500, obs_per_point=6, seed=31)
    ses = ba.BaSession(gpu_ctx)
    try:
        live, sid = np.zeros(len(sc["points"]), bool), {}
        for n in range(1, 26):
            intr = sc["intrinsics"][n - 1] if n == 1 else ses.cameras()[1][0]
            live = _grow(ses, sc, n, live, sid, intr)
            if n < 3:
                continue
            groups = np.zeros(n, np.int32) if n >= 10 else None
            if groups is not None:
                ses.set_groups(groups)
            P0, I0 = ses.cameras()
            X0, (pt, cam, xy) = ses.points(), ses.graph()
            ref = ba.solve_flat(gpu_ctx, P0, I0, X0, xy.astype(np.float64), cam, pt, groups=groups)
            s = ses.solve()
            P1, I1 = ses.cameras()
            assert _same_bits(ref, (P1, I1, ses.points(), s)), n
            assert s["reduced_dim"] == (6 * (n - 1) - 3 + (4 if n >= 10 else 0)) and _members_identical(I1, np.zeros(n, np.int32))
        assert not np.array_equal(I1[0], sc["intrinsics"][0])
        near = ses.covisible(24, 5)[0]
        free = np.concatenate([[24], near[near >= 2]])
        o = _options(gpu_ctx, len(free), mode=1, fix=(0, 0))
        Pa, Ia = ses.cameras()
        Pa[free, 3:] += 0.01                                  # (the global solve has just converged: give the window something to do)
        ses.cameras(poses=Pa)
        s, info = ses.solve_local(free, o)
        Pb, Ib = ses.cameras()
        assert info["n_constant"] > 0 and s["final_cost"] < s["initial_cost"] and s["reduced_dim"] == 6 * len(free)
        assert Ib.tobytes() == Ia.tobytes() and not np.array_equal(Pb[free], Pa[free])
        held = np.setdiff1d(np.arange(25), free)
        assert Pb[held].tobytes() == Pa[held].tobytes()
    finally:
        ses.close()
