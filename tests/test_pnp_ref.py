"""CPU suite: the restatement of P3P-RANSAC view registration (tests/pnp_ref.py) against itself
(literal loop = round-structured form, bit for bit), against planted poses, against an independent minimiser, on the edge
cases, and the golden fixture against its generator."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import pnp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "pnp_small.npz")
SHARES = (0.0, 0.3, 0.6)
SEEDS = (1, 2)


def same_bits(a, b):
    for k in ("count", "iterations"):
        if int(a[k]) != int(b[k]):
            return False
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in ("mask", "pose34", "ransac_pose34"))


@functools.lru_cache(maxsize=None)
def scene(seed, w):
    pts, views = pnp_ref.scene_views(seed, w)
    return pts, views, [pnp_ref.pnp_ransac(v["landmark"], v["xy"], pts, v["intr6"]) for v in views]


def rot_err(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("w", SHARES)
def test_literal_loop_equals_rounds_on_scenes(w):
    """A1: two views per outlier share; the round form also for another B."""
    pts, views, res = scene(1, w)
    for i in range(2):
        v = views[i]
        lit = pnp_ref.pnp_ransac(v["landmark"], v["xy"], pts, v["intr6"], literal=True)
        assert same_bits(lit, res[i])
        assert same_bits(pnp_ref.pnp_ransac(v["landmark"], v["xy"], pts, v["intr6"], B=7), res[i])


def test_p3p_finds_planted_pose():
    """A2: 2000 seeded noiseless triples; planted pose among the solutions for >= 99.5 %, all depths positive."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(1)
    ok, N = 0, 2000
    for _ in range(N):
        R = Rotation.from_rotvec(rng.normal(0, 0.5, 3)).as_matrix()
        t = rng.normal(0, 1, 3) + [0, 0, 6]
        P = rng.normal(0, 1, (3, 3))
        Y = P @ R.T + t
        f = Y / np.linalg.norm(Y, axis=1)[:, None]
        sols = [np.array(s).reshape(3, 4) for s in pnp_ref.p3p(f.tolist(), P.tolist())]
        assert len(sols) <= 4
        for s in sols:
            assert np.all((P @ s[:, :3].T + s[:, 3])[:, 2] > 0)
        ok += any(rot_err(s[:, :3], R) < 1e-6 and np.linalg.norm(s[:, 3] - t) < 1e-6 for s in sols)
    print("planted pose found: %d / %d" % (ok, N))
    assert ok >= 0.995 * N


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("w", SHARES)
def test_scenes_recover_planted_pose(seed, w):
    """A3."""
    pts, views, res = scene(seed, w)
    for v, r in zip(views, res):
        n = len(v["landmark"])
        assert 972 <= n <= 1032
        planted = int(pnp_ref.within(v["pose34_gt"], v["intr6"], pts, v["landmark"], v["xy"]).sum())
        after = int(pnp_ref.within(r["pose34"], v["intr6"], pts, v["landmark"], v["xy"]).sum())
        P, G = r["pose34"].reshape(3, 4), v["pose34_gt"].reshape(3, 4)
        c, cg = -P[:, :3].T @ P[:, 3], -G[:, :3].T @ G[:, 3]
        scale = np.linalg.norm(pts[v["landmark"][~v["wrong"]]].mean(0) - cg)
        print(seed, w, n, planted, r["count"], after, r["iterations"], rot_err(P[:, :3], G[:, :3]), np.linalg.norm(c - cg) / scale)
        assert r["count"] == int(r["mask"].sum())
        assert r["count"] >= 0.9 * planted
        assert after >= 0.99 * planted
        assert rot_err(P[:, :3], G[:, :3]) <= 5e-3
        assert np.linalg.norm(c - cg) <= 5e-3 * scale
        assert r["iterations"] <= 1000


REFIT_EXCESS = 8.42e-14     # 10 x the largest excess measured over the 72 views (8.42e-15)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("w", SHARES)
def test_refit_against_scipy(seed, w):
    """A4: the cost at pose34 against scipy.optimize.least_squares over an angle-axis pose on the same inliers from the
    same start (tolerances 1e-15).  Largest relative excess measured with pnp_ref over the 72 views: 8.42e-15; the bound
    is ten times that.  R R' = I to 1e-12 and det R > 0 for every pose returned."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    pts, views, res = scene(seed, w)
    for v, r in zip(views, res):
        m = r["mask"].astype(bool)
        X, xy, K = pts[v["landmark"]][m], v["xy"][m].astype(float), v["intr6"]

        def resid(p):
            l = X @ Rotation.from_rotvec(p[:3]).as_matrix().T + p[3:]
            x, y = l[:, 0] / l[:, 2], l[:, 1] / l[:, 2]
            rr = x * x + y * y
            d = K[4] * rr + K[5] * rr * rr
            return np.stack([K[0] * (x + d) + K[2] - xy[:, 0], K[1] * (y + d) + K[3] - xy[:, 1]], 1).ravel()

        P0, P = r["ransac_pose34"].reshape(3, 4), r["pose34"].reshape(3, 4)
        ls = least_squares(resid, np.concatenate([Rotation.from_matrix(P0[:, :3]).as_rotvec(), P0[:, 3]]), xtol=1e-15, ftol=1e-15, gtol=1e-15)
        cs = float((ls.fun ** 2).sum())
        # the cost at pose34 itself, without the detour over a rotation vector
        l = X @ P[:, :3].T + P[:, 3]
        c = float(((K[0] * l[:, 0] / l[:, 2] + K[2] - xy[:, 0]) ** 2 + (K[1] * l[:, 1] / l[:, 2] + K[3] - xy[:, 1]) ** 2).sum())
        print(seed, w, "excess", (c - cs) / cs)
        assert (c - cs) / cs <= REFIT_EXCESS
        for Q in (P0, P):
            assert np.abs(Q[:, :3] @ Q[:, :3].T - np.eye(3)).max() <= 1e-12
            assert np.linalg.det(Q[:, :3]) > 0


@functools.lru_cache(maxsize=None)
def edge():
    return {c[0]: c[1:] for c in pnp_ref.edge_cases()}


EXPECT = {"n0": -2, "n3": -2, "same_landmark": -1}


@pytest.mark.parametrize("name", ["n0", "n3", "n4", "n4_coplanar", "same_landmark", "repeated50", "nan_points", "distortion", "w09"])
def test_edge_cases(name):
    """A5: literal loop = round form on every edge case; the fixed outcomes."""
    lm, xy, pts, K = edge()[name]
    r = pnp_ref.pnp_ransac(lm, xy, pts, K)
    lit = pnp_ref.pnp_ransac(lm, xy, pts, K, literal=True)
    assert same_bits(lit, r)
    assert same_bits(pnp_ref.pnp_ransac(lm, xy, pts, K, B=5), r)
    assert not np.isnan(r["pose34"]).any() and not np.isnan(r["ransac_pose34"]).any()
    if name in EXPECT:
        assert r["count"] == EXPECT[name] and not r["mask"].any() and not r["pose34"].any() and not r["ransac_pose34"].any()
    else:
        assert r["count"] == int(r["mask"].sum()) >= 4
    if name == "same_landmark":
        assert r["iterations"] == 10000
    if name == "nan_points":
        assert not r["mask"][np.isnan(pts[lm]).any(1)].any()
    if name == "repeated50":
        assert r["count"] >= 90
    if name == "w09":       # the cap, or the update rule's stop: whatever the literal loop does (same_bits above)
        assert r["iterations"] <= 10000
    if name == "distortion":
        assert K[4] != 0 and K[5] != 0 and r["count"] >= 0.6 * len(lm)


def test_golden_matches_generator():
    spec = importlib.util.spec_from_file_location("make_pnp_golden", os.path.join(HERE, "golden", "make_pnp_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = gen.make()
    with np.load(GOLD) as g:
        assert sorted(g.files) == sorted(fresh)
        for k in g.files:
            assert np.array_equal(g[k].view(np.uint8), np.ascontiguousarray(fresh[k]).view(np.uint8)), k
