"""CPU suite: the contract of track building (tests/tracks_ref.py) against an independent breadth-first search over an adjacency dict,
its invariances, the golden file, and the property every scene of tests/test_tracks_gpu.py is named for.  No GPU."""
import os
from collections import deque

import numpy as np
import pytest

import tracks_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tracks_small.npz")


def bfs_tracks(fm, K, min_length=2, max_length=0, conflict=T.DROP_TRACK, select=None):
    """Tracks as sorted lists of (image, feature), by a search that shares nothing with the contract: adjacency dict, deque, sets."""
    imgs = sorted({i for p in fm for i in p})
    adj = {(i, f): set() for i in imgs for f in range(K[i])}
    for (a, b), m in fm.items():
        for f, g in m:
            adj[(a, f)].add((b, g))
            adj[(b, g)].add((a, f))
    seen, out = set(), []
    sel = None if select is None else set(int(i) for i in select[0])
    for start in sorted(adj):
        if start in seen:
            continue
        comp, todo = [], deque([start])
        seen.add(start)
        while todo:
            x = todo.popleft()
            comp.append(x)
            for y in adj[x]:
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        if len(comp) < 2:
            continue
        per_img = {}
        for i, f in comp:
            per_img.setdefault(i, []).append(f)
        bad = {i for i, fs in per_img.items() if len(fs) >= 2}
        if bad and conflict == T.DROP_TRACK:
            continue
        keep = sorted((i, f) for i, f in comp if i not in bad and (sel is None or i in sel))
        if len(keep) >= min_length and (max_length == 0 or len(keep) <= max_length):
            out.append(keep)
    return sorted(out)


def random_scene(rng):
    n = int(rng.integers(2, 13))
    ids = sorted(rng.choice(40, n, replace=False).tolist())
    K = {i: int(rng.integers(0, 41)) for i in ids}
    fm = {}
    for a in ids:
        for b in ids:
            if a >= b:
                continue
            mode = rng.integers(0, 4)                 # neither, a -> b, b -> a, both
            for x, y in ([(a, b)] if mode in (1, 3) else []) + ([(b, a)] if mode in (2, 3) else []):
                m = int(rng.integers(0, min(K[x], K[y]) + 1))
                fm[(x, y)] = list(zip(rng.permutation(K[x])[:m].tolist(), rng.permutation(K[y])[:m].tolist()))
    if not fm:
        fm[(ids[0], ids[1])] = []
    used = {i for p in fm for i in p}
    return fm, {i: K[i] for i in used}


@pytest.mark.parametrize("seed", range(12))
def test_contract_equals_bfs_on_random_graphs(seed):
    rng = np.random.default_rng(seed)
    fm, K = random_scene(rng)
    imgs = sorted(K)
    sel_n = int(rng.integers(1, len(imgs) + 1))
    sel_img = rng.permutation(imgs)[:sel_n]
    select = (sel_img, rng.integers(0, 50, sel_n))
    for conflict in (T.DROP_TRACK, T.DROP_IMAGE):
        for sel in (None, select):
            for mn, mx in ((2, 0), (3, 0), (2, 4), (3, 3)):
                r = T.build(*T.lists_of(fm), K, min_length=mn, max_length=mx, conflict=conflict, select=sel)
                assert r["tracks"] == bfs_tracks(fm, K, mn, mx, conflict, sel), (seed, conflict, mn, mx)
                # canonical order and the arrays' mutual consistency
                assert all(t == sorted(t) for t in r["tracks"]) and r["tracks"] == sorted(r["tracks"], key=lambda t: t[0])
                assert r["counts"].tolist() == [len(r["tracks"]), sum(len(t) for t in r["tracks"])]
                ft = r["feat_track"]
                for j, t in enumerate(r["tracks"]):
                    for i, f in t:
                        assert ft[r["node_off"][list(r["img_ids"]).index(i)] + f] == j
                assert (ft >= 0).sum() == r["counts"][1]
                if sel is not None:
                    cam = dict(zip(sel[0].tolist(), sel[1].tolist()))
                    assert r["obs_cam"].tolist() == [cam[i] for t in r["tracks"] for i, f in t]


@pytest.mark.parametrize("seed", range(4))
def test_invariant_under_order_and_mirror(seed):
    fm, K = random_scene(np.random.default_rng(100 + seed))
    base = T.build(*T.lists_of(fm), K, conflict=T.DROP_IMAGE)
    for s in range(3):
        other = T.build(*T.lists_of(T.shuffled(fm, s)), K, conflict=T.DROP_IMAGE, mirror=bool(s & 1))
        for k in ("counts", "trk_off", "obs_img", "obs_feat", "feat_track", "stats"):
            assert np.array_equal(base[k], other[k]), k


def test_statistics_of_a_known_scene():
    fm, K = T.scene_conflict()
    r = T.build(*T.lists_of(fm), K)
    assert r["tracks"] == [[(10, 1), (11, 1), (12, 1), (14, 1)]]
    assert r["stats"].tolist() == [2, 1, 5, 0, 5, 4, 7, 0]
    r = T.build(*T.lists_of(fm), K, conflict=T.DROP_IMAGE)
    assert r["tracks"] == [[(10, 0), (12, 0), (14, 0)], [(10, 1), (11, 1), (12, 1), (14, 1)]]
    assert r["stats"].tolist() == [2, 1, 2, 0, 5, 4, 7, 0]
    r = T.build(*T.lists_of(fm), K, conflict=T.DROP_IMAGE, min_length=4)
    assert r["stats"].tolist() == [2, 1, 2, 1, 5, 4, 7, 0]
    with pytest.raises(ValueError):
        T.build(*T.lists_of(fm), K, min_length=1)


def test_truncate():
    fm, K = T.scene_chain(5, K=3)
    r = T.build(*T.lists_of(fm), K)
    assert r["counts"].tolist() == [3, 15]
    t = T.truncate(r, 3, 15)
    assert t["written"] == 3 and np.array_equal(t["trk_off"], [0, 5, 10, 15])
    t = T.truncate(r, 2, 15)
    assert t["written"] == 2 and np.array_equal(t["trk_off"], [0, 5, 10]) and (t["feat_track"] >= 0).sum() == 10
    t = T.truncate(r, 5, 14)
    assert t["written"] == 2 and np.array_equal(t["trk_off"], [0, 5, 10, 10, 10, 10]) and len(t["obs_img"]) == 10
    t = T.truncate(r, 0, 0)
    assert t["written"] == 0 and np.array_equal(t["trk_off"], [0]) and (t["feat_track"] == -1).all()


def test_golden():
    g = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in g.files})
    assert len(names) >= 3
    for n in names:
        K = dict(zip(g[n + ".K_img"].tolist(), g[n + ".K"].tolist()))
        opt = g[n + ".options"].tolist()
        sel = (g[n + ".sel_img"], g[n + ".sel_cam"]) if len(g[n + ".sel_img"]) else None
        r = T.build(g[n + ".pairs"], g[n + ".offsets"], g[n + ".qt"], K, min_length=opt[0], max_length=opt[1], conflict=opt[2], select=sel)
        for k in ("counts", "trk_off", "obs_img", "obs_feat", "feat_track", "stats"):
            assert np.array_equal(r[k], g[n + "." + k]), (n, k)


# ---- the scenes of the GPU tests have the property they are named for ---------------------------------------------------------------

@pytest.mark.parametrize("L", [2, 63, 64, 65, 1024, 1025])
def test_chain_scene_has_tracks_of_exactly_L(L):
    fm, K = T.scene_chain(L)
    r = T.build(*T.lists_of(fm), K)
    assert r["counts"].tolist() == [2, 2 * L] and np.array_equal(np.diff(r["trk_off"]), [L, L]) and r["stats"][5] == L


def test_star_scene_is_one_track_of_65():
    fm, K = T.scene_star()
    r = T.build(*T.lists_of(fm), K)
    assert r["counts"].tolist() == [1, 65] and r["stats"][1] == 0 and r["tracks"][0][0] == (0, 0)


def test_grid_scene_is_600_cliques():
    fm, K = T.scene_grid()
    assert len(fm) == 66
    r = T.build(*T.lists_of(fm), K)
    assert r["counts"].tolist() == [600, 7200] and r["stats"].tolist() == [600, 0, 0, 0, 12, 12, 66 * 600, 0]


def test_giant_scene_has_a_component_above_the_image_count():
    fm, K = T.scene_giant()
    r = T.build(*T.lists_of(fm), K)
    assert r["stats"][4] > 12 and r["stats"][4] == 7200 and r["counts"].tolist() == [0, 0] and r["stats"][2] == 7200
    r = T.build(*T.lists_of(fm), K, conflict=T.DROP_IMAGE)
    assert r["counts"].tolist() == [0, 0] and r["stats"][1] == 1


def test_conflict_scene_has_a_two_feature_conflict_in_a_component_of_5():
    fm, K = T.scene_conflict()
    r = T.build(*T.lists_of(fm), K)
    assert r["stats"][1] == 1 and r["stats"][2] == 5 and r["stats"][4] == 5


def test_six_scene_exercises_selection_and_both_length_limits():
    fm, K = T.scene_six()
    full = T.build(*T.lists_of(fm), K, conflict=T.DROP_IMAGE)
    lens = np.diff(full["trk_off"])
    assert full["stats"][1] > 0 and (lens == 2).any() and (lens >= 5).any() and (full["feat_track"] < 0).any()
    sel = ([7, 3, 5], [2, 0, 1])
    r = T.build(*T.lists_of(fm), K, select=sel)
    assert 0 < r["counts"][0] < T.build(*T.lists_of(fm), K)["counts"][0] and set(r["obs_cam"].tolist()) == {0, 1, 2}
    assert T.build(*T.lists_of(fm), K, min_length=3)["stats"][3] > 0
    assert T.build(*T.lists_of(fm), K, max_length=4)["stats"][3] > 0


def test_degenerate_scene():
    fm, K = T.scene_degenerate()
    r = T.build(*T.lists_of(fm), K)
    assert r["tracks"] == [[(1, 0), (2, 1)]] and r["node_off"].tolist() == [0, 0, 2, 6, 6, 7] and r["feat_track"][2 + 3] == -1
    fm0, K0 = {(0, 1): []}, {0: 3, 1: 0}
    assert T.build(*T.lists_of(fm0), K0)["counts"].tolist() == [0, 0]
