"""Bundle-adjustment scenes whose observation GRAPH is not the one synth_ba.make_scene fixes (test helper, CPU only).

make_scene gives every landmark the same number of sorted, distinct cameras (at most 10), k1 = k2 = 0, fx = fy, and a ring of
cameras none of which has a small rotation.  The two builders here leave all of that behind:

  graph_scene   ragged tracks (0, 1, ... n_cams observations, in any order inside a track), a camera seen twice by one landmark,
                fx != fy, an off-centre principal point and non-zero radial distortion -- on make_scene's cameras and points;
  rig_scene     cameras side by side looking down +z whose rotation vectors have the magnitudes at which the rotation and its
                derivative change form: exactly 0, either side of sqrt(DBL_EPSILON) = 1.49e-8 (first-order branch of
                ceres::AngleAxisRotatePoint) and either side of 1e-2 (series / closed form of the right Jacobian).

Both return the dict ba.solve_scene and orc_ba.solve take (poses, intrinsics, points, obs_uv, obs_cam, obs_pt; landmark-major)
plus poses_gt, points_gt and pt_off.  SCENES names the cases of the two suites (tests/test_ba_graphs_ref.py, _gpu.py) and
`conditions` states, from the scene itself, what each case is there to reach.
"""
import functools

import numpy as np

from reconstructor_amd import synth_ba

INTRINSICS_RIG = (614.4, 650.0, 259.5, 165.75, -0.08, 0.02)
K1, K2 = -0.08, 0.02
ROT_MAG = (0.0, 0.0, 0.0, 1e-9, 1.2e-8, 1.6e-8, 1e-5, 5e-3, 9.9e-3, 1.01e-2, 5e-2)
SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


def _finish(sc, poses_gt, intr, pts_gt, tracks, rng, noise_px=0.5):
    """Observations of `tracks` (a list of camera arrays, one per landmark) = trunc(projection of the truth + noise)."""
    lens = np.array([len(t) for t in tracks], np.int64)
    obs_pt = np.repeat(np.arange(len(tracks), dtype=np.int32), lens)
    obs_cam = (np.concatenate(tracks) if lens.sum() else np.zeros(0)).astype(np.int32)
    uv, depth = synth_ba.project(poses_gt[obs_cam], intr[obs_cam], pts_gt[obs_pt])
    assert (depth > 0.1).all()
    uv = np.trunc(uv + noise_px * rng.standard_normal(uv.shape))
    sc.update(obs_uv=np.ascontiguousarray(uv), obs_cam=np.ascontiguousarray(obs_cam), obs_pt=np.ascontiguousarray(obs_pt),
              pt_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    return sc


def graph_scene(nc, npts, seed, lengths, repeat=0.0, shuffle=True, cycle=False):
    """make_scene's poses and points (truth and perturbed start) under another graph: per landmark a length drawn from `lengths`
    (taken in turn when `cycle`), that many distinct cameras in random order (sorted unless `shuffle`), and with probability
    `repeat`, for a track of two or more, a second observation of one of its own cameras at a random position (its own noise,
    so another pixel).  Intrinsics -- the same for the observations and for the start: fy = 1.07 fx, the principal point
    moved by (3.5, -2.25), k1 = -0.08, k2 = 0.02."""
    base = synth_ba.make_scene(nc, npts, obs_per_point=nc, seed=seed)
    rng = np.random.default_rng(seed + 7919)
    lengths = np.asarray(lengths, np.int64)
    assert lengths.min() >= 0 and lengths.max() <= nc
    tracks = []
    for j in range(npts):
        k = int(lengths[j % len(lengths)] if cycle else rng.choice(lengths))
        cams = rng.permutation(nc)[:k]
        if not shuffle:
            cams = np.sort(cams)
        if k >= 2 and rng.random() < repeat:
            cams = np.insert(cams, rng.integers(0, k + 1), cams[rng.integers(0, k)])
        tracks.append(cams)
    intr = base["intr_gt"].copy()
    intr[:, 1] *= 1.07
    intr[:, 2] += 3.5
    intr[:, 3] -= 2.25
    intr[:, 4], intr[:, 5] = K1, K2
    sc = {"poses_gt": base["poses_gt"], "points_gt": base["points_gt"], "poses": base["poses"], "points": base["points"],
          "intrinsics": intr}
    return _finish(sc, base["poses_gt"], intr, base["points_gt"], tracks, rng)


def rig_scene(nc, npts, seed, k=4, mag=ROT_MAG):
    """Cameras at C_i = (0.5 (i - (nc-1)/2), 0.1 sin i, 0) looking down +z, camera i turned by mag[i % len(mag)] about a random
    axis (with fewer cameras than magnitudes: the first three, which are the exact zeros of ROT_MAG, then the rest of the list
    spread evenly over the remaining cameras, first and last included -- so that eight cameras still meet every regime);
    points in the box [-1.5, 1.5] x [-1, 1] x [4, 8], each seen by k sorted distinct cameras.  The start differs from the
    truth in the translations of cameras >= 2 (sigma 0.02) and in the points (sigma 0.05) ONLY: every rotation starts at exactly
    its listed magnitude, so the first Jacobian is taken in that regime."""
    rng = np.random.default_rng(seed)
    i = np.arange(nc)
    C = np.stack([0.5 * (i - (nc - 1) / 2), 0.1 * np.sin(i), np.zeros(nc)], 1)
    axis = rng.standard_normal((nc, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    poses = np.zeros((nc, 6))
    which = i % len(mag)
    if 3 < nc < len(mag):
        which[3:] = 3 + np.rint(np.linspace(0, len(mag) - 4, nc - 3)).astype(np.int64)
    poses[:, :3] = axis * np.asarray(mag, np.float64)[which][:, None]
    for c in range(nc):
        poses[c, 3:] = -synth_ba.rodrigues(poses[c, :3]) @ C[c]
    pts = np.stack([rng.uniform(-1.5, 1.5, npts), rng.uniform(-1, 1, npts), rng.uniform(4, 8, npts)], 1)
    tracks = [np.sort(rng.permutation(nc)[:k]) for _ in range(npts)]
    intr = np.tile(np.array(INTRINSICS_RIG), (nc, 1))
    p0, x0 = poses.copy(), pts.copy()
    p0[2:, 3:] += 0.02 * rng.standard_normal((nc - 2, 3))
    x0 += 0.05 * rng.standard_normal(x0.shape)
    sc = {"poses_gt": poses, "points_gt": pts, "poses": p0, "points": x0, "intrinsics": intr}
    return _finish(sc, poses, intr, pts, tracks, rng)


def copy_scene(sc):
    return {key: np.array(v, copy=True) for key, v in sc.items()}


def select(sc, keep):
    """The scene with the observations keep[] (a mask over the observations) only."""
    out = copy_scene(sc)
    for key in ("obs_cam", "obs_pt", "obs_uv"):
        out[key] = np.ascontiguousarray(sc[key][keep])
    out["pt_off"] = np.concatenate([[0], np.cumsum(np.bincount(out["obs_pt"], minlength=len(sc["points"])))]).astype(np.int64)
    return out


def reorder_tracks(sc, how, seed=0):
    """The same problem with the observations permuted INSIDE every track (pt_off unchanged): how = "shuffle" or "sort"
    (by camera, stable)."""
    rng = np.random.default_rng(seed)
    off = sc["pt_off"]
    perm = np.arange(len(sc["obs_pt"]))
    for j in range(len(off) - 1):
        a, b = off[j], off[j + 1]
        perm[a:b] = a + (rng.permutation(b - a) if how == "shuffle" else np.argsort(sc["obs_cam"][a:b], kind="stable"))
    out = copy_scene(sc)
    for key in ("obs_cam", "obs_pt", "obs_uv"):
        out[key] = np.ascontiguousarray(sc[key][perm])
    return out


def repeated_second(sc):
    """Mask over the observations: True at every observation whose (landmark, camera) already occurred earlier in its track."""
    key = sc["obs_pt"].astype(np.int64) * len(sc["poses"]) + sc["obs_cam"]
    first = np.zeros(len(key), bool)
    first[np.unique(key, return_index=True)[1]] = True
    return ~first


def track_lengths(sc):
    return np.diff(sc["pt_off"])


def segment_lengths(sc):
    """Entries of every camera-pair list of the Schur build: ordered pairs (o, o2), o != o2, of one landmark with
    cam(o2) <= cam(o) and both cameras free (camera 0 is fixed and has no free parameter below 10 cameras)."""
    nc = len(sc["poses"])
    seg = np.zeros((nc, nc), np.int64)
    off, cam = sc["pt_off"], sc["obs_cam"]
    free = np.ones(nc, bool)
    free[0] = nc >= 10
    for j in range(len(off) - 1):
        c = cam[off[j]:off[j + 1]]
        if len(c) < 2:
            continue
        a, b = np.meshgrid(c, c, indexing="ij")
        m = (b <= a) & ~np.eye(len(c), dtype=bool) & free[a] & free[b]
        np.add.at(seg, (a[m], b[m]), 1)
    return seg


def distortion_shift_px(sc):
    """|project(truth) - project(truth with k1 = k2 = 0)| per observation, in pixels."""
    i0 = sc["intrinsics"].copy()
    i0[:, 4:] = 0.0
    a, _ = synth_ba.project(sc["poses_gt"][sc["obs_cam"]], sc["intrinsics"][sc["obs_cam"]], sc["points_gt"][sc["obs_pt"]])
    b, _ = synth_ba.project(sc["poses_gt"][sc["obs_cam"]], i0[sc["obs_cam"]], sc["points_gt"][sc["obs_pt"]])
    return np.abs(a - b).max(axis=1)


LONG = (0, 1, 2, 2, 3, 3, 4, 5, 7, 11, 16, 17, 25)


def _one_obs_camera():
    sc = scene("long_general")
    idx = np.flatnonzero(sc["obs_cam"] == 24)
    keep = np.ones(len(sc["obs_cam"]), bool)
    keep[idx[1:]] = False
    return select(sc, keep)


SCENES = {
    "long_small": lambda: graph_scene(25, 100, 101, LONG, repeat=0.1),
    "long_general": lambda: graph_scene(25, 400, 102, LONG, repeat=0.1),
    "few_cams": lambda: graph_scene(6, 300, 103, (0, 1, 2, 3, 6), repeat=0.15),
    "edge_256": lambda: graph_scene(17, 200, 104, (16, 17), cycle=True),
    "sees_all": lambda: graph_scene(40, 300, 105, (2, 3, 40), repeat=0.1),
    "one_obs_camera": _one_obs_camera,
    "rig8": lambda: rig_scene(8, 200, 108),
    "rig11": lambda: rig_scene(11, 300, 111),
    "rig22": lambda: rig_scene(22, 500, 122),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc = SCENES[name]()
    for v in sc.values():
        v.setflags(write=False)
    return sc


def scene(name):
    """The named scene, built once per process; the arrays are read-only (copy_scene gives a writable copy)."""
    return dict(_scene(name))


def conditions(name, sc):
    """What the case is in the suite for, asserted on the scene itself: a change of a builder cannot quietly empty a case."""
    nc = len(sc["poses"])
    k = track_lengths(sc)
    sumsq = int((k * k).sum())
    assert len(sc["obs_pt"]) <= 5000 and nc <= 40 and (np.diff(sc["obs_pt"]) >= 0).all()
    if name == "long_small":
        assert nc * nc <= 1024 and sumsq <= 16384, sumsq               # the one-workgroup list builder
        assert k.max() >= 25 and (k == 0).any() and (k == 1).any()
        assert repeated_second(sc).any()
    elif name == "long_general":
        assert sumsq > 16384, sumsq                                     # count / scan / fill
        assert k.max() >= 25 and (k == 0).any() and (k == 1).any() and repeated_second(sc).any()
        assert (segment_lengths(sc) > 32).any()                         # k_pair_sort_long
        assert segment_lengths(sc).diagonal().sum() > 0                 # diagonal lists
    elif name == "few_cams":
        assert nc < 10 and repeated_second(sc).any() and (k == 0).any() and (k == 1).any()
        assert distortion_shift_px(sc).max() >= 4.0
    elif name == "edge_256":
        assert (k == 16).any() and (k == 17).any() and set(k.tolist()) == {16, 17}
    elif name == "sees_all":
        assert nc * nc > 1024 and k.max() >= 40
    elif name == "one_obs_camera":
        assert np.bincount(sc["obs_cam"], minlength=nc).min() == 1
    else:
        w = np.linalg.norm(sc["poses"][2:, :3], axis=1)                 # free cameras with a free rotation AND translation
        assert (w == 0).any() and ((w > 0) & (w < SQRT_EPS)).any() and ((w > SQRT_EPS) & (w < 1e-2)).any() and (w > 1e-2).any()
        assert (nc >= 10) == (name != "rig8")
    # tracks are unsorted where the case says so
    if name in ("long_small", "long_general", "few_cams", "sees_all"):
        assert any((np.diff(sc["obs_cam"][sc["pt_off"][j]:sc["pt_off"][j + 1]]) < 0).any() for j in range(len(k)))
