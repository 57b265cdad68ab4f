"""CPU suite: the two restatements of batched triangulation (tests/tri_ref.py) against each other, the candidate builders
(reconstructor_amd/triangulate.py) against the reference's loops run one triangulateMultiView at a time, and the golden
fixture against its generator."""
import importlib.util
import os

import numpy as np
import pytest

import tri_ref
from reconstructor_amd import triangulate as tri

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "triangulate_small.npz")


def _flat(c):
    return {k: c[k] for k in ("poses34", "intrinsics", "trk_off", "obs_cam", "obs_xy")}


def _margins(c, xyz):
    """Per track: largest L1 reprojection error and smallest pairwise angle of X (numpy, for the distance to the thresholds)."""
    P = c["poses34"].reshape(-1, 3, 4)
    K = c["intrinsics"]
    cen = -np.einsum("cji,cj->ci", P[:, :, :3], P[:, :, 3])
    off = c["trk_off"]
    res, ang = np.zeros(len(off) - 1), np.full(len(off) - 1, np.inf)
    with np.errstate(all="ignore"):
        for j in range(len(off) - 1):
            o = np.arange(off[j], off[j + 1])
            cam = c["obs_cam"][o]
            loc = np.einsum("lij,j->li", P[cam, :, :3], xyz[j]) + P[cam, :, 3]
            x, y = loc[:, 0] / loc[:, 2], loc[:, 1] / loc[:, 2]
            d = K[cam, 4] * (x * x + y * y) + K[cam, 5] * (x * x + y * y) ** 2
            res[j] = np.max(np.abs(K[cam, 0] * (x + d) + K[cam, 2] - c["obs_xy"][o, 0]) + np.abs(K[cam, 1] * (y + d) + K[cam, 3] - c["obs_xy"][o, 1]))
            r = xyz[j] - cen[cam]
            r /= np.linalg.norm(r, axis=1, keepdims=True)
            cs = np.clip(r @ r.T, -1, 1)
            a = 180 * np.arccos(cs) / 3.1415
            ang[j] = np.min(a[~np.eye(len(o), dtype=bool)])
    return res, ang


@pytest.mark.parametrize("n_cams,n_tracks,lo,hi,seed,defects", [(25, 600, 2, 2, 1, 0.0), (16, 500, 2, 8, 2, 0.0),
                                                                  (12, 500, 2, 6, 3, 0.3), (40, 200, 10, 16, 4, 0.2)])
def test_canonical_against_numpy_svd(n_cams, n_tracks, lo, hi, seed, defects):
    c = tri_ref.make_tracks(n_cams, n_tracks, lo, hi, seed=seed, defect_rate=defects, distortion=defects > 0)
    x0, s0 = tri_ref.canonical_tracks(**_flat(c))
    x1, s1 = tri_ref.numpy_tracks(**_flat(c))
    res, ang = _margins(c, x1)
    away = (np.abs(res - 4.0) > 1e-6) & (np.abs(ang - 1.0) > 1e-6) & (np.abs(x1[:, 2]) > 1e-9)
    assert away.mean() > 0.99
    assert np.array_equal(s0[away], s1[away])
    wc = s1 == 0                                  # accepted: at least 1 degree between every pair of rays
    assert wc.mean() > 0.3
    assert np.all(np.abs(x0[wc] - x1[wc]) <= 1e-9 * np.abs(x1[wc]).max(1, keepdims=True))
    if defects:
        assert set(np.unique(s0)) >= {0, 1, 2}


def test_canonical_rules_on_hand_made_tracks():
    K = [600.0, 600.0, 256.0, 168.0, 0.0, 0.0]
    P0 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    P1 = [1.0, 0, 0, -1.0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]                  # centre (1, 0, 0)
    C = [tri_ref.cam_centre(P0), tri_ref.cam_centre(P1)]
    # X = (0.5, 0.2, 5): pixels (316, 192) and (196, 192) exactly
    X, st = tri_ref.canonical_track([P0, P1], [K, K], [(316, 192), (196, 192)], C)
    assert st == 0 and np.allclose(X, [0.5, 0.2, 5.0], rtol=1e-12)
    # two cameras looking down -z (R = diag(-1, 1, -1)): X = (0, 0, -5) is in front of both, world z < 0 -> status 1
    Q0 = [-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, -1.0, 0]
    Q1 = [-1.0, 0, 0, 1.0, 0, 1.0, 0, 0, 0, 0, -1.0, 0]                # centre (1, 0, 0)
    X, st = tri_ref.canonical_track([Q0, Q1], [K, K], [(256, 168), (376, 168)], [tri_ref.cam_centre(Q0), tri_ref.cam_centre(Q1)])
    assert st == 1 and np.allclose(X, [0.0, 0.0, -5.0], rtol=1e-12)
    # a 1-observation track cannot be triangulated
    assert tri_ref.canonical_track([P0], [K], [(316, 192)], C[:1])[1] == 1


def _builder_case(seed):
    L = tri_ref.loop_containers(8, 700, obs_per_point=5, seed=seed)
    return L


def _run_loop(L, batched, views):
    """initial pair (0, 1), then triangulateMatchedLandmarks for `views`; batched: step 3 through the builders and one
    canonical batch, else the reference's loop one call at a time."""
    c, ids, fm, im = L["coords"], L["landmark_ids"], L["feature_matches"], L["img_matches"]
    P, K = L["poses34"], L["intrinsics"]
    lms = []
    if batched:
        tracks = tri.initial_pair_tracks(fm[(0, 1)], 0, 1)
        _batch(tracks, L, lms)
    else:
        tri_ref.sequential_initial_pair(0, 1, fm, c, ids, lms, P, K)
    registered = [(1, True), (0, True)]
    for v in views:
        fids, lids = tri_ref.calc_2d3d_matches(v, im, fm, ids, lms)
        if batched:
            tri_ref.sequential_matched_landmarks(v, fids, lids, [], im, fm, c, ids, lms, P, K)     # step 1 alone (no registered image: no step 3)
            _batch(tri.new_view_tracks(v, ids, registered, im, fm), L, lms)
        else:
            tri_ref.sequential_matched_landmarks(v, fids, lids, registered, im, fm, c, ids, lms, P, K)
        registered = [(v, v % 3 != 2)] + registered          # an unregistered entry now and then (regStatus false)
    return lms, ids


def _batch(tracks, L, lms):
    imgs = sorted(L["poses34"])
    off, cam, xy = tri.tracks_to_arrays(tracks, {i: i for i in imgs}, L["coords"])
    xyz, st = tri_ref.canonical_tracks(np.stack([L["poses34"][i] for i in imgs]), np.stack([L["intrinsics"][i] for i in imgs]),
                                       off, cam, xy)
    for j, t in enumerate(tracks):
        if st[j] == 0:
            for i, f in t:
                L["landmark_ids"][i][f] = len(lms)
            lms.append({"xyz": list(xyz[j]), "track": list(t)})
    return st


@pytest.mark.parametrize("seed", [1, 2])
def test_builders_equal_the_reference_loops(seed):
    import copy
    L = _builder_case(seed)
    La, Lb = copy.deepcopy(L), copy.deepcopy(L)
    views = [2, 3, 4, 5, 6, 7]
    lm_a, ids_a = _run_loop(La, False, views)
    lm_b, ids_b = _run_loop(Lb, True, views)
    assert len(lm_a) == len(lm_b) > 0
    for a, b in zip(lm_a, lm_b):
        assert a["track"] == b["track"]
        assert np.array(a["xyz"]).tobytes() == np.array(b["xyz"]).tobytes()
    assert ids_a == ids_b


def test_new_view_tracks_break_and_partner_rules():
    # image 2 is new; registered order (1, 0); feature 0 of image 2 matches feature 5 of image 1 and 7 of image 0
    ids = {0: [-1] * 10, 1: [-1] * 10, 2: [-1] * 4}
    fm = {(2, 1): {0: 5, 1: 6, 3: 2}, (2, 0): {0: 7, 1: 8, 2: 9, 3: 1}}
    im = {2: [0, 1]}
    ids[1][6] = 4                                  # partner of feature 1 in image 1 is already a landmark: image 0 is tried next
    ids[2][3] = 0                                  # feature 3 of the new image is a landmark already (step 1): skipped
    got = tri.new_view_tracks(2, ids, [(1, True), (0, True)], im, fm)
    assert got == [[(1, 5), (2, 0)], [(0, 8), (2, 1)], [(0, 9), (2, 2)]]
    # registered order decides which image the (only) track is built with; an unregistered image is skipped
    assert tri.new_view_tracks(2, ids, [(0, True), (1, True)], im, fm)[0] == [(0, 7), (2, 0)]
    assert tri.new_view_tracks(2, ids, [(0, False), (1, True)], im, fm)[0] == [(1, 5), (2, 0)]
    # an image that is registered but not in imgMatches[img] is skipped
    assert tri.new_view_tracks(2, ids, [(1, True), (0, True)], {2: [0]}, fm)[0] == [(0, 7), (2, 0)]
    # initial pair: the iteration order given
    assert tri.initial_pair_tracks({3: 1, 0: 2}, 4, 9) == [[(4, 3), (9, 1)], [(4, 0), (9, 2)]]


def test_golden_regenerates_identically():
    spec = importlib.util.spec_from_file_location("make_triangulate_golden", os.path.join(HERE, "golden", "make_triangulate_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    g = m.make()
    f = np.load(GOLD)
    assert sorted(g) == sorted(f.files)
    for k in f.files:
        assert g[k].tobytes() == f[k].tobytes() and g[k].dtype == f[k].dtype, k
    assert set(np.unique(f["status"])) == {0, 1, 2, 3}
