"""CPU suite (no GPU): the judge of csrc/homography.hip is judged.  tests/homography_ref.py's sequential loop and its round
form agree bit for bit; an independent transcription written here (SVD DLT with Hartley normalisation, numpy.linalg.lstsq
for the refinement, its own sampler and loop) bounds the restatement's error and pins its inlier counts and labels; the
classification families get the labels of the issue's table; the edge cases end as stated.

The classification families run the E search with distance_threshold = 1e9 (FAR).  With cv::recoverPose's default of 50
baselines the cheirality mask of a pure rotation or a tiny baseline holds 0 - 14 of 200 entries (the recovered |t| = 1 puts
every point beyond 50), so that rule 1 (cheir < min_inliers) labels them NO_MODEL before the parallax is looked at, and
the mask of a small baseline keeps only the near points, whose parallax is above the scene's median.  Without the cut the
measured medians are the planted ones.  Both variants are asserted: with the default cut a degenerate family is never
GENERAL or PLANAR.
"""
import math

import numpy as np
import pytest

import homography_ref as hr
import twoview_ref as tv

FAR = 1e9
SCENES = [(seed, share) for seed in (1, 2) for share in (0.0, 0.3, 0.6)]


def _same(a, b):
    return (a["count"] == b["count"] and a["iterations"] == b["iterations"] and a["mask"].tobytes() == b["mask"].tobytes() and
            np.asarray(a["H"]).tobytes() == np.asarray(b["H"]).tobytes())


@pytest.mark.parametrize("seed,share", SCENES)
def test_forms_agree_on_scenes(seed, share):
    s = hr.scene(seed, share)
    lit = hr.find(s["xy1"], s["xy2"], literal=True)
    for B in (32, 7, 5):
        assert _same(lit, hr.find(s["xy1"], s["xy2"], B=B)), B
    assert lit["count"] >= 0.8 * int((~s["wrong"]).sum())
    Ht = (s["H"] / s["H"][2, 2]).ravel()
    assert np.abs(lit["H"] - Ht).max() < 1.0                         # pixels truncated to integers: the translation is off by ~1/2


def test_forms_agree_on_edge_cases():
    count = {}
    for name, a, b in hr.edge_cases():
        lit = hr.find(a, b, literal=True)
        for B in (32, 7, 5):
            assert _same(lit, hr.find(a, b, B=B)), (name, B)
        count[name] = (lit["count"], lit["iterations"])
        assert not np.isnan(lit["H"]).any() and lit["count"] == (int(lit["mask"].sum()) if lit["count"] >= 0 else lit["count"])
    assert count["n0"] == (-2, 0) and count["n3"] == (-2, 0) and count["n4"] == (4, 0)
    assert count["identical"] == (-1, 0) and count["line"] == (-1, 0)        # no subset ever passes: the attempt cap at iteration 0
    assert count["flip4"] == (-1, 0) and count["n4_collinear"] == (-1, 0)
    assert count["n5"][0] >= 4 and count["n8"][0] >= 4 and count["flip"][0] >= 4
    assert count["random12"][0] in (-1, 4, 5) and count["random12"][1] > 100  # no model worth the name among 12 random pairs


# ---- the independent transcription -------------------------------------------------------------------------------------

def _t_norm(p):
    c = p.mean(0)
    s = len(p) / np.abs(p - c).sum(0)
    return np.array([[s[0], 0, -s[0] * c[0]], [0, s[1], -s[1] * c[1]], [0, 0, 1.0]])


def t_dlt(src, dst):
    """Hartley-normalised DLT through the SVD; H with h33 = 1, or None."""
    with np.errstate(all="ignore"):
        Ts, Td = _t_norm(src), _t_norm(dst)
        if not (np.isfinite(Ts).all() and np.isfinite(Td).all()):
            return None
        a = np.c_[src, np.ones(len(src))] @ Ts.T
        b = np.c_[dst, np.ones(len(dst))] @ Td.T
        rows = []
        for (X, Y, _), (x, y, _) in zip(a, b):
            rows += [[X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x], [0, 0, 0, X, Y, 1, -y * X, -y * Y, -y]]
        _, sv, Vt = np.linalg.svd(np.array(rows))
        if len(src) == 4 and not sv[7] > 1e-12 * sv[0]:
            return None
        H = np.linalg.inv(Td) @ Vt[-1].reshape(3, 3) @ Ts
        if not np.isfinite(H).all() or H[2, 2] == 0:
            return None
        return H / H[2, 2]


def _t_residual(h8, src, dst):
    H = np.append(h8, 1.0).reshape(3, 3)
    q = np.c_[src, np.ones(len(src))] @ H.T
    return (q[:, :2] / q[:, 2:] - dst).ravel(), q


def t_refine(H, src, dst):
    """At most 10 Gauss-Newton steps through numpy.linalg.lstsq, a step kept only if it lowers the cost."""
    h = (H / H[2, 2]).ravel()[:8]
    r, q = _t_residual(h, src, dst)
    for _ in range(10):
        J = np.zeros((2 * len(src), 8))
        w = q[:, 2]
        J[0::2, 0], J[0::2, 1], J[0::2, 2] = src[:, 0] / w, src[:, 1] / w, 1 / w
        J[1::2, 3], J[1::2, 4], J[1::2, 5] = src[:, 0] / w, src[:, 1] / w, 1 / w
        J[0::2, 6], J[0::2, 7] = -q[:, 0] / w * src[:, 0] / w, -q[:, 0] / w * src[:, 1] / w
        J[1::2, 6], J[1::2, 7] = -q[:, 1] / w * src[:, 0] / w, -q[:, 1] / w * src[:, 1] / w
        hn = h - np.linalg.lstsq(J, r, rcond=None)[0]
        rn, qn = _t_residual(hn, src, dst)
        if not rn @ rn < r @ r:
            break
        h, r, q = hn, rn, qn
    return np.append(h, 1.0).reshape(3, 3)


def _t_subset_ok(src, dst):
    def tri(p, a, b, c):
        return np.linalg.det(np.array([[p[a, 0], p[a, 1], 1.0], [p[b, 0], p[b, 1], 1.0], [p[c, 0], p[c, 1], 1.0]]))
    for p in (src, dst):
        for i in (2, 3):
            for j in range(i):
                for k in range(j):
                    d1, d2 = p[j] - p[i], p[k] - p[i]
                    if abs(d2[0] * d1[1] - d2[1] * d1[0]) <= 2.0 ** -23 * (abs(d1).sum() + abs(d2).sum()):
                        return False
    neg = sum(tri(src, *t) * tri(dst, *t) < 0 for t in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)))
    return neg in (0, 4)


def t_find(xy1, xy2, thr=3.0, conf=0.995, max_iters=2000):
    """cv::findHomography's RANSAC written once more: returns (count, H) of the refitted model, count -1 / -2 as the kernel."""
    src, dst = np.asarray(xy1, np.float64).reshape(-1, 2), np.asarray(xy2, np.float64).reshape(-1, 2)
    n = len(src)
    if n < 4:
        return -2, None
    state = 2 ** 64 - 1

    def inl(H):
        with np.errstate(all="ignore"):
            q = np.c_[src, np.ones(n)] @ H.T
            e = ((q[:, :2] / q[:, 2:] - dst) ** 2).sum(1)
            return e.astype(np.float32) <= np.float32(thr * thr)
    best, bestH, niters, it = 0, None, max_iters, 0
    while it < niters:
        found = False
        for _ in range(10000):
            idx = []
            while len(idx) < 4:
                state = (state & 0xFFFFFFFF) * 4164903690 + (state >> 32)
                k = (state & 0xFFFFFFFF) % n
                if k not in idx:
                    idx.append(k)
            if _t_subset_ok(src[idx], dst[idx]):
                found = True
                break
        if not found:
            break
        H = t_dlt(src[idx], dst[idx])
        if H is not None:
            good = int(inl(H).sum())
            if good > max(best, 3):
                best, bestH = good, H
                ep = (n - good) / n
                den = 1.0 - (1.0 - ep) ** 4
                if den < 2.2250738585072014e-308:
                    niters = 0
                else:
                    num, den = math.log(1.0 - conf), math.log(den)
                    niters = niters if den >= 0 or -num >= niters * -den else int(np.rint(num / den))
        it += 1
    if bestH is None:
        return -1, None
    m = inl(bestH)
    H = t_dlt(src[m], dst[m])
    H = t_refine(H if H is not None else bestH, src[m], dst[m])
    return int(inl(H).sum()), H


def test_deviation_from_a_planted_homography_is_rounding_level():
    """300 seeded four-point samples of exact correspondences (subpixel coordinates, no truncation): worst deviation of
    H / |H| from the planted homography.  Measured: transcription (SVD) 1.325e-11, restatement (Gauss-Jordan, complete
    pivoting) 6.659e-12 -- the restatement must stay within 10 x the transcription's figure, the margin of section 18: both
    are rounding-level, and a wrong formula misses by orders of magnitude."""
    rng = np.random.default_rng(5)
    worst_t = worst_r = 0.0
    done = 0
    while done < 300:
        s = hr.scene(int(rng.integers(1 << 30)), 0.0, n=4)
        src = rng.uniform([0, 0], [1280, 960], (4, 2))
        q = np.c_[src, np.ones(4)] @ s["H"].T
        dst = q[:, :2] / q[:, 2:]
        if not _t_subset_ok(src, dst) or not hr.subset_ok(np.c_[src, dst]):
            continue
        done += 1
        Ht = s["H"] / np.linalg.norm(s["H"])
        A = t_dlt(src, dst)
        B = np.array(hr.homography4(np.c_[src, dst])).reshape(3, 3)
        worst_t = max(worst_t, np.abs(A / np.linalg.norm(A) - Ht).max())
        worst_r = max(worst_r, np.abs(B / np.linalg.norm(B) - Ht).max())
    print("worst deviation: transcription %.3e, restatement %.3e" % (worst_t, worst_r))
    assert worst_t < 1e-6                                               # the transcription itself is sane
    assert worst_r <= 10 * worst_t


# ---- the classification families -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def families():
    """Every family's scenes with the restatement's geometry, computed once."""
    out = {}
    for name, kw, label in hr.classification_families():
        rows = []
        for seed in hr.family_seeds(name):
            for share in (0.0, 0.3):
                s = tv.scene_pair(seed, share, n=200, **kw)
                rows.append((seed, share, s, hr.geometry(s["xy1"], s["xy2"], s["K1"], s["K2"], tv_opt=dict(distance_threshold=FAR))))
        out[name] = (label, rows)
    return out


def test_classification_families_get_their_labels(families):
    for name, (label, rows) in families.items():
        for seed, share, s, (e, h, ratio, angle, got) in rows:
            assert got == label, (name, seed, share, ratio, angle, hr.LABEL_NAMES[got])
            assert abs(ratio - 0.8) > 0.08 and abs(angle - 1.0) > 0.1, (name, seed, share, ratio, angle)      # far from both thresholds


def test_degenerate_families_are_never_chosen_with_the_default_depth_cut():
    """distance_threshold 50 (the default of the E search): the pure rotation and the tiny baseline end as NO_MODEL or
    PANORAMIC -- never as a label the pair choice accepts."""
    for name, kw, _ in hr.classification_families()[3:5]:
        for seed in (21, 22):
            s = tv.scene_pair(seed, 0.3, n=200, **kw)
            label = hr.geometry(s["xy1"], s["xy2"], s["K1"], s["K2"])[4]
            assert label in (hr.NO_MODEL, hr.PANORAMIC), (name, seed, hr.LABEL_NAMES[label])


def test_pinned_parity_with_the_transcription(families):
    """The restatement's homography inlier count and the label built on it equal those of the transcription's H, found by
    its own loop on the same sample stream."""
    for name, (label, rows) in families.items():
        for seed, share, s, (e, h, ratio, angle, got) in rows[:4]:
            count, _ = t_find(s["xy1"], s["xy2"])
            assert count == h["count"], (name, seed, share, count, h["count"])
            assert hr.classify(s["xy1"], s["xy2"], s["K1"], s["K2"], e["count"], e["cheir_mask"], e["pose34"], count)[2] == got


def test_choice_walks_down_the_candidates():
    pairs = [(0, 1), (0, 2), (1, 2), (2, 3)]
    off = [0, 50, 150, 250, 260]
    order, pos, fb = hr.choose_initial_pair_by_geometry(pairs, off, [hr.PANORAMIC, hr.PLANAR, hr.GENERAL, hr.GENERAL])
    assert (order, pos, fb) == ([1, 2, 0, 3], 2, False)                 # size descending, then (i, j)
    assert hr.choose_initial_pair_by_geometry(pairs, off, [hr.PANORAMIC, hr.PLANAR, hr.NO_MODEL, hr.SMALL_BASELINE])[1:] == (1, False)
    assert hr.choose_initial_pair_by_geometry(pairs, off, [hr.PANORAMIC, hr.NO_MODEL], top_m=2) == ([1, 2], 0, True)
    assert tv.choose_initial_pair(pairs, off)[2] == order[0]


def test_acos_from_basic_operations():
    """Within 8 ulp of pi of libm's: the series is good to an ulp or two of its sum, and the branch above 120 degrees
    multiplies it by four."""
    for c in list(np.linspace(-1, 1, 401)) + [1 - 1e-12, 1 - 1e-9, -1 + 1e-9, 0.5, -0.5, 0.9999, 1.0, -1.0]:
        assert abs(hr.acos_basic(float(c)) - math.acos(float(c))) <= 8 * 4.45e-16, c
