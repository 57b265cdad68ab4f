"""Local bundle adjustment: the judge (test helper, CPU only).

Three things the GPU suites (tests/test_ba_constant_gpu.py, tests/test_ba_local_gpu.py) are held against, none of which shares
code with the library:

  extract / sub_scene    a numpy restatement of the sub-problem a local solve works on (csrc/ba_local.hip): the landmarks with an
                         observation in a free camera, the cameras that see one of them (ascending session index = local index),
                         the observations in the original landmark-major, track order;
  covisible_counts/pick  landmarks shared with one camera, per camera, and the k that share the most;
  judge                  scipy.optimize.least_squares on synth_ba.project residuals over the free poses and the observed points --
                         another minimiser (trust-region reflective or dogleg on a finite-difference Jacobian) than the library's
                         Levenberg-Marquardt on analytic derivatives and than the oracle's.

With ONE constant camera the scale of the scene is free (position and orientation are held, nothing holds a length): two correct
minimisers end at different points of that valley, so only the RMS is comparable.  With two or more the gauge is fixed and the
parameters are comparable too.  tests/test_ba_local_ref.py checks the judge itself: against the oracle, and trf against dogbox.
"""
import functools
import os

import numpy as np

from reconstructor_amd import synth_ba

import ba_graphs

LENGTHS = lambda nc: [2, 3, 4, nc]
# (cameras, landmarks, seed, constant cameras) of graph_scene(nc, npts, seed, lengths=[2, 3, 4, nc])
ONE_CONSTANT = ((6, 120, 1, (3,)), (8, 200, 2, (7,)), (12, 300, 3, (0,)))
MANY_CONSTANT = ((8, 200, 2, (2, 5)), (12, 300, 3, (0, 4, 11)), (12, 300, 3, tuple(range(3, 12))))
TIGHT = dict(function_tolerance=1e-14, parameter_tolerance=1e-12, gradient_tolerance=1e-14)
# Where PARAMETERS are compared with the judge's, the solve must not end on the function tolerance: near the minimum the cost is quadratic
# in the distance to it, so a step that changes the cost by 1e-14 of itself can still be 1e-7 sqrt(2 cost / lambda) long in a direction of
# curvature lambda -- 1e-8 .. 1e-7 for a landmark seen by two views, which is what the library was measured to be off by when it stopped
# there (poses 1.8e-9, points 9.7e-8 on the first case of MANY_CONSTANT, the RMS equal to 2e-15 px).  Without it the loop runs until a step
# no longer lowers the cost at all or is shorter than 1e-12 (|x| + 1e-12).
TO_THE_END = dict(function_tolerance=0.0, parameter_tolerance=1e-12, gradient_tolerance=1e-14)


@functools.lru_cache(maxsize=None)
def _scene(nc, npts, seed, repeat):
    sc = ba_graphs.graph_scene(nc, npts, seed, lengths=LENGTHS(nc), repeat=repeat)
    for v in sc.values():
        v.setflags(write=False)
    return sc


def scene(nc, npts, seed, repeat=0.0):
    return dict(_scene(nc, npts, seed, repeat))


def mask(nc, cams):
    m = np.zeros(nc, bool)
    m[list(cams)] = True
    return m


# ---------------------------------------------------------------- extraction
def extract(free, n_points, obs_pt, obs_cam):
    """free: bool per session camera.  Returns dict(sel, pt_map, cam_map, obs, ocam, opt, constant): selected flag per landmark,
    local -> session landmark and camera, the kept observations (indices into the flat arrays, order kept), their local camera
    and landmark, constant flag per local camera."""
    free = np.asarray(free, bool)
    obs_pt, obs_cam = np.asarray(obs_pt), np.asarray(obs_cam)
    sel = np.zeros(n_points, bool)
    sel[obs_pt[free[obs_cam]]] = True
    obs = np.flatnonzero(sel[obs_pt])
    takes_part = np.zeros(len(free), bool)
    takes_part[obs_cam[obs]] = True
    cam_map, pt_map = np.flatnonzero(takes_part), np.flatnonzero(sel)
    cam_loc, pt_loc = np.cumsum(takes_part) - 1, np.cumsum(sel) - 1
    return dict(sel=sel, pt_map=pt_map.astype(np.int32), cam_map=cam_map.astype(np.int32), obs=obs,
                ocam=cam_loc[obs_cam[obs]].astype(np.int32), opt=pt_loc[obs_pt[obs]].astype(np.int32), constant=~free[cam_map])


def sub_scene(poses, intr, points, obs_uv, obs_pt, obs_cam, free):
    """The sub-problem as a scene dict (what solve_scene takes), packed on the host, and the extraction."""
    e = extract(free, len(points), obs_pt, obs_cam)
    sc = {"poses": np.ascontiguousarray(np.asarray(poses)[e["cam_map"]]), "intrinsics": np.ascontiguousarray(np.asarray(intr)[e["cam_map"]]),
          "points": np.ascontiguousarray(np.asarray(points)[e["pt_map"]]), "obs_uv": np.ascontiguousarray(np.asarray(obs_uv, np.float64)[e["obs"]]),
          "obs_cam": e["ocam"], "obs_pt": e["opt"]}
    return sc, e


# ---------------------------------------------------------------- covisibility
def covisible_counts(n_cams, n_points, obs_pt, obs_cam, cam):
    """Landmarks shared with `cam` per camera; a landmark that sees a camera twice counts once.  [cam]: its own landmarks."""
    sees = np.zeros((n_points, n_cams), bool)
    sees[np.asarray(obs_pt), np.asarray(obs_cam)] = True
    return sees[sees[:, cam]].sum(axis=0).astype(np.int32)


def covisible_pick(counts, cam, k):
    order = [c for c in sorted(range(len(counts)), key=lambda c: (-int(counts[c]), c)) if c != cam and counts[c] > 0]
    return np.array(order[:k], np.int32)


# ---------------------------------------------------------------- the judge
def rms(sc, poses=None, points=None):
    P = sc["poses"] if poses is None else poses
    X = sc["points"] if points is None else points
    uv, _ = synth_ba.project(P[sc["obs_cam"]], sc["intrinsics"][sc["obs_cam"]], X[sc["obs_pt"]])
    return float(np.sqrt(((uv - sc["obs_uv"]) ** 2).sum() / max(len(sc["obs_pt"]), 1)))


def judge(sc, constant, method="trf"):
    """Minimise the reprojection error over the poses of the cameras that are not constant and the points that are observed;
    intrinsics are held.  Returns (poses, points, rms in pixels)."""
    from scipy.optimize import least_squares
    constant = np.asarray(constant, bool)
    fc = np.flatnonzero(~constant)
    seen = np.zeros(len(sc["points"]), bool)
    seen[sc["obs_pt"]] = True
    fp = np.flatnonzero(seen)
    P0, X0 = np.array(sc["poses"], np.float64), np.array(sc["points"], np.float64)
    cam, pt, K, uv0 = sc["obs_cam"], sc["obs_pt"], sc["intrinsics"][sc["obs_cam"]], sc["obs_uv"]

    def unpack(x):
        P, X = P0.copy(), X0.copy()
        P[fc] = x[:6 * len(fc)].reshape(-1, 6)
        X[fp] = x[6 * len(fc):].reshape(-1, 3)
        return P, X

    def fun(x):
        P, X = unpack(x)
        uv, _ = synth_ba.project(P[cam], K, X[pt])
        return (uv - uv0).reshape(-1)

    x0 = np.concatenate([P0[fc].reshape(-1), X0[fp].reshape(-1)])
    r = least_squares(fun, x0, jac="3-point", method=method, x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400)
    P, X = unpack(r.x)
    return P, X, float(np.sqrt((r.fun ** 2).sum() / max(len(pt), 1)))


@functools.lru_cache(maxsize=None)
def judged(nc, npts, seed, constant, method="trf"):
    """judge() of a named case, once per process (the GPU suites share it)."""
    P, X, r = judge(scene(nc, npts, seed), mask(nc, constant), method)
    P.setflags(write=False); X.setflags(write=False)
    return P, X, r


def spread(nc, npts, seed, constant):
    """What two correct minimisers differ by on this case: |trf - dogbox| in (RMS, poses, points)."""
    Pa, Xa, ra = judged(nc, npts, seed, constant, "trf")
    Pb, Xb, rb = judged(nc, npts, seed, constant, "dogbox")
    seen = np.zeros(npts, bool)
    seen[scene(nc, npts, seed)["obs_pt"]] = True
    return abs(ra - rb), float(np.abs(Pa - Pb).max()), float(np.abs(Xa - Xb)[seen].max())


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_local_judge.npz")


def _key(nc, npts, seed, constant):
    return "c%d_p%d_s%d_k%s" % (nc, npts, seed, "-".join(str(c) for c in constant))


def write_golden(path=GOLDEN):
    """The judge's results on MANY_CONSTANT (trf; the trf / dogbox spread beside them), recorded: a run of the judge is tens of
    seconds on a CPU, which the GPU suites do not spend.  tests/test_ba_local_ref.py runs the judge afresh and holds the record
    against it.   PYTHONPATH=. python tests/ba_local_ref.py   rewrites the file."""
    out = {}
    for nc, npts, seed, const in MANY_CONSTANT:
        P, X, r = judged(nc, npts, seed, const)
        k = _key(nc, npts, seed, const)
        out[k + "_P"], out[k + "_X"], out[k + "_rms"], out[k + "_spread"] = P, X, np.float64(r), np.array(spread(nc, npts, seed, const))
    np.savez(path, **out)


@functools.lru_cache(maxsize=None)
def recorded(nc, npts, seed, constant):
    """(poses, points, rms, (spread in rms, poses, points)) of the judge on a case of MANY_CONSTANT, from tests/golden/"""
    with np.load(GOLDEN) as z:
        k = _key(nc, npts, seed, constant)
        return z[k + "_P"], z[k + "_X"], float(z[k + "_rms"]), tuple(float(v) for v in z[k + "_spread"])


def permuted_to_front(sc, c):
    """The scene with camera c moved to index 0 (the others keep their order): the oracle's fix_cam0_pose then holds it."""
    nc = len(sc["poses"])
    order = np.array([c] + [i for i in range(nc) if i != c])
    new_of = np.empty(nc, np.int32)
    new_of[order] = np.arange(nc, dtype=np.int32)
    out = ba_graphs.copy_scene(sc)
    for key in ("poses", "intrinsics", "poses_gt"):
        out[key] = np.ascontiguousarray(sc[key][order])
    out["obs_cam"] = np.ascontiguousarray(new_of[sc["obs_cam"]])
    return out, order


if __name__ == "__main__":
    write_golden()
    print("wrote", GOLDEN)
