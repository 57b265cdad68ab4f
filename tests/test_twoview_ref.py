"""CPU suite: the canonical two-view initialisation (tests/twoview_ref.py) -- the five-point solver
against an independent numpy transcription, the loop forms against each other, the pose recovery against planted poses,
the edge cases, the choice of the initial pair and the golden file."""
import itertools
import os

import numpy as np
import pytest

import tri_ref
import twoview_ref as tv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twoview_small.npz")
N_SOLVER_SAMPLES = 300
SOLVER_SEED = 2024
COND_MAX = 1e9            # condition bound on the 10 x 10 elimination block: beyond it the transcription itself is unreliable
ROOT_GAP_MIN = 1e-5       # relative gap between neighbouring real roots of the transcription's polynomial
RESIDUAL_MAX = 1e-9       # a transcription solution counts when its own constraint residual is below this
ILL_SHARE_MAX = 0.02


# ---- the independent transcription: SVD null space, dict polynomials, numpy.linalg.solve, numpy.roots, SVD pose ---------

def _pmul(a, b):
    out = {}
    for (ea, ca), (eb, cb) in itertools.product(a.items(), b.items()):
        e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
        out[e] = out.get(e, 0.0) + ca * cb
    return out


def _padd(a, b, s=1.0):
    out = dict(a)
    for e, c in b.items():
        out[e] = out.get(e, 0.0) + s * c
    return out


# Nister's order: what the elimination keeps on the left, then x (z^2, z, 1), y (z^2, z, 1), z^3, z^2, z, 1
_ORDER = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
          (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _residual(E, q1, q2):
    E = E / np.linalg.norm(E)
    c = 2 * E @ E.T @ E - np.trace(E @ E.T) * E
    ep = max(abs(np.array([*b, 1.0]) @ E @ np.array([*a, 1.0])) for a, b in zip(q1, q2))
    return max(np.abs(c).max(), abs(np.linalg.det(E)), ep)


def transcription_five_point(q1, q2):
    """q1, q2: 5 x 2 normalised points.  Returns (list of (3 x 3 E, its own constraint residual), ill-conditioned flag)."""
    Q = np.array([[b[0] * a[0], b[0] * a[1], b[0], b[1] * a[0], b[1] * a[1], b[1], a[0], a[1], 1.0] for a, b in zip(q1, q2)])
    N = np.linalg.svd(Q)[2][5:]
    var = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
    E = [[{var[b]: N[b][3 * i + j] for b in range(4)} for j in range(3)] for i in range(3)]
    EEt = [[_padd(_padd(_pmul(E[i][0], E[j][0]), _pmul(E[i][1], E[j][1])), _pmul(E[i][2], E[j][2])) for j in range(3)] for i in range(3)]
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    eqs = []
    for i in range(3):
        for j in range(3):
            p = {}
            for k in range(3):
                lam = _padd(EEt[i][k], tr, -0.5) if i == k else EEt[i][k]
                p = _padd(p, _pmul(lam, E[k][j]))
            eqs.append(p)
    det = _padd(_padd(_pmul(_padd(_pmul(E[1][1], E[2][2]), _pmul(E[1][2], E[2][1]), -1.0), E[0][0]),
                      _pmul(_padd(_pmul(E[1][0], E[2][2]), _pmul(E[1][2], E[2][0]), -1.0), E[0][1]), -1.0),
                _pmul(_padd(_pmul(E[1][0], E[2][1]), _pmul(E[1][1], E[2][0]), -1.0), E[0][2]))
    eqs.append(det)
    A = np.array([[p.get(e, 0.0) for e in _ORDER] for p in eqs])
    cond = np.linalg.cond(A[:, :10])
    if not np.isfinite(cond) or cond > COND_MAX:
        return [], True
    G = np.linalg.solve(A[:, :10], A[:, 10:])
    B = []
    for e, f in ((4, 5), (6, 7), (8, 9)):           # descending powers for numpy.poly*
        re, rf = G[e], G[f]
        B.append((np.array([-rf[0], re[0] - rf[1], re[1] - rf[2], re[2]]), np.array([-rf[3], re[3] - rf[4], re[4] - rf[5], re[5]]),
                  np.array([-rf[6], re[6] - rf[7], re[7] - rf[8], re[8] - rf[9], re[9]])))
    p1 = np.polysub(np.polymul(B[0][1], B[1][2]), np.polymul(B[0][2], B[1][1]))
    p2 = np.polysub(np.polymul(B[0][2], B[1][0]), np.polymul(B[0][0], B[1][2]))
    p3 = np.polysub(np.polymul(B[0][0], B[1][1]), np.polymul(B[0][1], B[1][0]))
    c = np.polyadd(np.polyadd(np.polymul(p1, B[2][0]), np.polymul(p2, B[2][1])), np.polymul(p3, B[2][2]))
    roots = np.roots(c)
    real = np.sort(roots[np.abs(roots.imag) <= 1e-9 * (1 + np.abs(roots.real))].real)
    ill = len(real) > 1 and bool((np.diff(real) <= ROOT_GAP_MIN * (1 + np.abs(real[:-1]))).any())
    # a complex pair about to merge on the real axis is the same kind of near-coincidence
    near = roots[(np.abs(roots.imag) > 1e-9 * (1 + np.abs(roots.real))) & (np.abs(roots.imag) <= ROOT_GAP_MIN * (1 + np.abs(roots.real)))]
    ill = ill or len(near) > 0
    out = []
    for z in real:
        w = np.polyval(p3, z)
        x, y = np.polyval(p1, z) / w, np.polyval(p2, z) / w
        Em = (x * N[0] + y * N[1] + z * N[2] + N[3]).reshape(3, 3)
        if np.isfinite(Em).all():
            out.append((Em / np.linalg.norm(Em), _residual(Em, q1, q2)))
    return out, ill


def _dist(E, F):
    E, F = np.asarray(E, np.float64).reshape(3, 3), np.asarray(F, np.float64).reshape(3, 3)
    E, F = E / np.linalg.norm(E), F / np.linalg.norm(F)
    return min(np.linalg.norm(E - F), np.linalg.norm(E + F))


def _solver_samples():
    rng = np.random.default_rng(SOLVER_SEED)
    for _ in range(N_SOLVER_SAMPLES):
        R = tv.rot(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 1, 3)
        t /= np.linalg.norm(t)
        X = np.stack([rng.uniform(-2, 2, 5), rng.uniform(-2, 2, 5), rng.uniform(3, 8, 5)], 1)
        Y = X @ R.T + t
        yield X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:], tv.essential(R, t)


def test_solver_against_the_independent_transcription():
    """A1.  Measured (SOLVER_SEED, 300 samples): see the printed figures; DESIGN.md section 18 records them."""
    kept, ill_n, own_worst = [], 0, 0.0
    for q1, q2, Et in _solver_samples():
        sols, ill = transcription_five_point(q1, q2)
        if ill:
            ill_n += 1
            continue
        own = min([_dist(E, Et) for E, _ in sols], default=np.inf)
        assert np.isfinite(own), "the transcription has no real solution on a sample it calls well-conditioned"
        own_worst = max(own_worst, own)
        kept.append((q1, q2, Et, [E for E, res in sols if res <= RESIDUAL_MAX]))
    assert ill_n <= ILL_SHARE_MAX * N_SOLVER_SAMPLES, ill_n
    bound = 10.0 * own_worst
    worst_true, worst_pair = 0.0, 0.0
    for q1, q2, Et, sols in kept:
        mine = tv.five_point(*[[float(v) for v in col] for col in (q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1])])
        assert 1 <= len(mine) <= 10
        worst_true = max(worst_true, min(_dist(E, Et) for E in mine))
        for S in sols:
            worst_pair = max(worst_pair, min(_dist(E, S) for E in mine))
    print("five-point: %d of %d samples ill-conditioned; transcription's worst deviation from the planted E %.3e, bound %.3e; "
          "restatement's worst deviation from the planted E %.3e, from a transcription solution %.3e"
          % (ill_n, N_SOLVER_SAMPLES, own_worst, bound, worst_true, worst_pair))
    assert worst_true <= bound and worst_pair <= bound


def test_roots_are_ascending_and_real():
    c = np.poly([-3.0, -1.5, 0.25, 2.0, 7.0, 1 + 2j, 1 - 2j, -2 + 0.5j, -2 - 0.5j, 4.5])[::-1]
    r = tv.real_roots([float(v.real) for v in c])
    assert np.allclose(r, [-3.0, -1.5, 0.25, 2.0, 4.5, 7.0], rtol=0, atol=1e-9) and r == sorted(r)
    assert tv.real_roots([1.0] + [0.0] * 9 + [0.0]) == [] and tv.real_roots([float("nan")] * 11) == []
    assert tv.real_roots([1.0] + [0.0] * 9 + [1.0]) == []           # z^10 + 1


SCENES = [(1, 0.0), (1, 0.3), (1, 0.6), (2, 0.3)]


def _same(a, b, what):
    for k in ("count", "iterations", "cheir_count", "candidate"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("mask", "cheir_mask", "E", "pose34"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


@pytest.mark.parametrize("seed,share", SCENES)
def test_round_form_equals_the_sequential_loop(seed, share):
    """A2: B = 32, 7 and 5 against the literal loop, bit for bit."""
    s = tv.scene_pair(seed, share, n=160)
    lit = tv.two_view_init(s["xy1"], s["xy2"], s["K1"], s["K2"], literal=True)
    assert lit["count"] >= 0.7 * int((~s["wrong"]).sum())
    for B in (32, 7, 5):
        _same(tv.two_view_init(s["xy1"], s["xy2"], s["K1"], s["K2"], B=B), lit, (seed, share, B))


# ---- pose recovery ---------------------------------------------------------------------------------------------------

def transcription_recover_pose(E, P, mask, dist=50.0):
    """cv::recoverPose as OpenCV writes it: SVD decomposition, DLT triangulation by SVD, the four masks, the cascade."""
    U, _, Vt = np.linalg.svd(np.asarray(E).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    good = []
    for R, tt in cands:
        P1 = np.hstack([R, tt[:, None]])
        m = np.zeros(len(P), bool)
        for e, (x1, y1, x2, y2) in enumerate(P):
            A = np.stack([x1 * P0[2] - P0[0], y1 * P0[2] - P0[1], x2 * P1[2] - P1[0], y2 * P1[2] - P1[1]])
            Q = np.linalg.svd(A)[2][3]
            ok = Q[2] * Q[3] > 0
            Q = Q / Q[3]
            ok = ok and Q[2] < dist
            z2 = (P1 @ Q)[2]
            m[e] = ok and z2 > 0 and z2 < dist
        good.append(m & mask.astype(bool))
    g = [int(m.sum()) for m in good]
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]:
        w = 0
    elif g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]:
        w = 1
    elif g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]:
        w = 2
    else:
        w = 3
    return cands[w][0], cands[w][1], good[w], g


def _angles(R, t, Rg, tg):
    rot = float(np.arccos(np.clip((np.trace(R @ Rg.T) - 1) / 2, -1, 1)))
    td = float(np.arccos(np.clip(t @ tg / (np.linalg.norm(t) * np.linalg.norm(tg)), -1, 1)))
    return rot, td


def test_pose_recovery_against_planted_poses():
    """A3.  Rotation and translation-direction errors against the planted pose, bounded by 10 x what the transcription
    reaches from the same E on the same inliers; the cascade picks the transcription's candidate on every scene."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for seed, share in [(s, w) for s in (1, 2, 3, 4) for w in (0.0, 0.3, 0.6)]:
        s = tv.scene_pair(seed, share, n=200)
        r = tv.two_view_init(s["xy1"], s["xy2"], s["K1"], s["K2"])
        assert r["count"] > 0 and r["cheir_count"] >= 0.9 * r["count"]
        P, _ = tv.normalised_entries(s["xy1"], s["xy2"], [float(v) for v in s["K1"]], [float(v) for v in s["K2"]])
        Rt, tt, gm, g = transcription_recover_pose(r["E"], P, r["mask"])
        pose = r["pose34"].reshape(3, 4)
        # the same candidate of the four (they differ by a half turn or by the sign of t): the SVD projects E onto the
        # essential matrices first, the closed form does not, hence 1e-6 and not rounding
        assert np.abs(pose[:, :3] - Rt).max() <= 1e-6 and np.abs(pose[:, 3] - tt).max() <= 1e-6, (seed, share)
        assert sorted(g) == sorted(int(x) for x in _all_counts(r, P)), (seed, share)
        assert np.array_equal(gm, r["cheir_mask"].astype(bool)), (seed, share)
        mine, theirs = _angles(pose[:, :3], pose[:, 3], s["R"], s["t"]), _angles(Rt, tt, s["R"], s["t"])
        assert mine[0] <= 10 * theirs[0] and mine[1] <= 10 * theirs[1], (seed, share, mine, theirs)
        assert abs(np.linalg.norm(pose[:, 3]) - 1) <= 1e-12 and np.abs(pose[:, :3] @ pose[:, :3].T - np.eye(3)).max() <= 1e-6
        worst = [max(worst[0], mine[0]), max(worst[1], mine[1]), max(worst[2], theirs[0]), max(worst[3], theirs[1])]
    print("pose recovery: worst rotation error %.3e rad (transcription %.3e), worst translation direction error %.3e rad "
          "(transcription %.3e)" % (worst[0], worst[2], worst[1], worst[3]))


def _all_counts(r, P):
    return [int((tv._good(R, t, P, 50.0, False) & r["mask"].astype(bool)).sum()) for R, t in tv.candidates([float(v) for v in r["E"]])]


def test_decomposition_gives_the_four_candidates():
    rng = np.random.default_rng(8)
    for _ in range(50):
        R, t = tv.rot(rng.normal(0, 0.8, 3)), rng.normal(0, 1, 3)
        t /= np.linalg.norm(t)
        E = tv.essential(R, t) * rng.uniform(0.1, 10) * rng.choice([-1, 1])
        R1, R2, tt = [np.array(v) for v in tv.decompose([float(v) for v in E.ravel()])]
        R1, R2 = R1.reshape(3, 3), R2.reshape(3, 3)
        assert min(np.abs(R1 - R).max(), np.abs(R2 - R).max()) <= 1e-12 and min(np.abs(tt - t).max(), np.abs(tt + t).max()) <= 1e-12
        for Q in (R1, R2):
            assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Q) - 1) <= 1e-12


# ---- edge cases ------------------------------------------------------------------------------------------------------

def test_edge_cases():
    """A4: what the canonical loop gives on each of them, in both loop forms."""
    seen = {}
    for name, a, b, K1, K2 in tv.edge_cases():
        r = tv.two_view_init(a, b, K1, K2)
        if len(a) <= 60 or name in ("identical", "nan_coordinates"):
            _same(tv.two_view_init(a, b, K1, K2, literal=True), r, name)
        _same(tv.two_view_init(a, b, K1, K2, B=7), r, name)
        assert not np.isnan(r["pose34"]).any() and not np.isnan(r["E"]).any(), name
        if r["count"] >= 0:
            assert r["count"] == int(r["mask"].sum()) > 4 and r["cheir_count"] == int(r["cheir_mask"].sum()), name
            assert not (r["cheir_mask"] & ~r["mask"]).any(), name
        else:
            assert not r["mask"].any() and not r["cheir_mask"].any() and not r["E"].any() and not r["pose34"].any(), name
        seen[name] = (r["count"], r["cheir_count"], r["iterations"])
    print("edge cases (count, cheirality count, iterations):", seen)
    assert seen["n0"] == (-2, 0, 0) and seen["n4"] == (-2, 0, 0)
    assert seen["n5"] == (5, 4, 1) and seen["n6"] == (5, 3, 13)       # a model always fits its own five entries
    assert seen["random12"] == (7, 4, 99)                             # twelve random matches: a sample's five and two by chance
    assert seen["identical"] == (-1, 0, 1000)               # every design matrix has rank 1: no sample gives a model
    assert seen["nan_coordinates"] == (-1, 0, 1000)         # the best count never exceeds 4
    assert seen["planar"][0] >= 100 and seen["distortion"][0] >= 120
    assert seen["pure_rotation"][0] >= 100                  # E fits (any t does); the pose's t is meaningless


# ---- the initial pair ------------------------------------------------------------------------------------------------

def test_choose_initial_pair():
    """A5."""
    from reconstructor_amd import twoview
    for choose in (tv.choose_initial_pair, twoview.choose_initial_pair):
        pairs = [(3, 4), (1, 2), (2, 1), (0, 5), (5, 0)]
        off = np.concatenate([[0], np.cumsum([7, 9, 9, 9, 9])])
        assert choose(pairs, off) == (0, 5, 3)
        assert choose(pairs[::-1], np.concatenate([[0], np.cumsum([9, 9, 9, 9, 7])])) == (0, 5, 1)
        assert choose([(4, 2)], [0, 0]) == (4, 2, 0)
        assert choose([(4, 2), (2, 4), (1, 9)], [0, 3, 6, 8]) == (2, 4, 1)
    L = tri_ref.loop_containers(25, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    keys = sorted(L["feature_matches"])
    off = np.concatenate([[0], np.cumsum([len(L["feature_matches"][k]) for k in keys])])
    for choose in (tv.choose_initial_pair, twoview.choose_initial_pair):
        i, j, k = choose(keys, off)
        assert (i, j) == (20, 22) and off[k + 1] - off[k] == 269 == len(L["feature_matches"][(22, 20)])


# ---- golden ----------------------------------------------------------------------------------------------------------

def test_golden():
    """A6: the restatement against tests/golden/twoview_small.npz (written by tests/golden/make_twoview_golden.py)."""
    with np.load(GOLD) as g:
        got = tv.two_view_init_batch(g["off"], g["xy1"], g["xy2"], g["intr6_1"], g["intr6_2"])
        for k in ("E", "pose34", "mask", "cheir_mask", "count", "iterations"):
            assert np.asarray(got[k]).tobytes() == g[k].astype(np.asarray(got[k]).dtype).tobytes(), k
        assert (g["count"][:, 0] > 0).sum() >= 3
