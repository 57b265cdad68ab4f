"""The contract of guided matching (tests/guided_ref.py) against an independent double loop, its identities, and its golden file.  No GPU."""
import os

import numpy as np
import pytest

import guided_ref
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "guided_small.npz")


def _loop_match(q, xy1, t, xy2, F, ratio=0.7, err=3.0, max_distance=0.0):
    """One query row and one train row at a time: Python floats for the band, orc.l2sq per candidate, a sort for the order.
    Returns (raw [K1], idx [K1][4], d2 [K1][2], candidates)."""
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    thr2 = float(np.float32(err)) * float(np.float32(err))
    big = float(np.finfo(np.float64).max)
    K1, K2 = len(q), len(t)
    raw = np.full(K1, -1, np.int32)
    idx = np.full((K1, 4), -1, np.int32)
    idx[:, 2:] = 0
    d2 = np.full((K1, 2), np.inf)
    total = 0
    with np.errstate(all="ignore"):
        for i in range(K1):
            x1, y1 = np.float64(xy1[i][0]), np.float64(xy1[i][1])
            found = []
            for j in range(K2):
                x2, y2 = np.float64(xy2[j][0]), np.float64(xy2[j][1])
                a = F[0] * x1 + F[1] * y1 + F[2]; b = F[3] * x1 + F[4] * y1 + F[5]; c = F[6] * x1 + F[7] * y1 + F[8]
                q2 = a * a + b * b; e2 = x2 * a + y2 * b + c; t2 = e2 * e2
                a = F[0] * x2 + F[3] * y2 + F[6]; b = F[1] * x2 + F[4] * y2 + F[7]; c = F[2] * x2 + F[5] * y2 + F[8]
                q1 = a * a + b * b; e1 = x1 * a + y1 * b + c; t1 = e1 * e1
                if q1 > 0 and q2 > 0 and q1 < big and q2 < big and t1 <= thr2 * q1 and t2 <= thr2 * q2:
                    found.append((orc.l2sq(q[i], t[j]), j))
            found.sort()
            total += len(found)
            idx[i, 2] = len(found)
            for k, (d, j) in enumerate(found[:2]):
                idx[i, k], d2[i, k] = j, d
            if found:
                dist0 = np.sqrt(np.float32(found[0][0]))
                dist1 = np.sqrt(np.float32(found[1][0])) if len(found) > 1 else np.float32(np.inf)
                if dist0 < np.float32(ratio) * dist1 and (not max_distance > 0 or dist0 <= np.float32(max_distance)):
                    raw[i] = found[0][1]
    return raw, idx, d2, total


CASES = {
    "two_view_40_33": lambda: guided_ref.shape_case(40, 33, 40, seed=41),
    "two_view_3_2": lambda: guided_ref.shape_case(3, 2, 32, seed=42),
    "planted_counts": lambda: guided_ref.planted_counts_case(32),
    "all_in_band": lambda: guided_ref.all_in_band_case(4, 30, 32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_double_loop(name):
    q, xy1, t, xy2, F = CASES[name]()
    for err, md in ((3.0, 0.0), (1.0, 0.0), (3.0, 5.0)):
        raw, idx, d2, total = _loop_match(q, xy1, t, xy2, F, err=err, max_distance=md)
        m = guided_ref.band(F, xy1, xy2, err)
        gi, gd = guided_ref.knn2(q, t, m)
        assert int(m.sum()) == total
        assert np.array_equal(gi, idx) and np.array_equal(gd, d2)
        assert np.array_equal(guided_ref.raw(gi, gd, 0.7, md), raw)
        # one-way table: the lowest query row keeps a contested train row
        out, cand = guided_ref.match_pair(q, xy1, t, xy2, F, max_error_px=err, max_distance=md)
        want, taken = np.full(len(q), -1, np.int32), set()
        for i, j in enumerate(raw):
            if j >= 0 and j not in taken:
                taken.add(int(j))
                want[i] = j
        assert np.array_equal(out, want) and cand == total
        # cross-check: the reversed pair under F^T through the loop as well
        rt = _loop_match(t, xy2, q, xy1, np.asarray(F).reshape(3, 3).T, err=err, max_distance=md)[0]
        cross = np.array([j if j >= 0 and rt[j] == i else -1 for i, j in enumerate(raw)], np.int32).reshape(len(q))
        got = guided_ref.match_pair(q, xy1, t, xy2, F, max_error_px=err, max_distance=md, cross_check=1)[0]
        assert np.array_equal(got, cross)
        kept = got[got >= 0]
        assert len(set(kept.tolist())) == len(kept)


def test_planted_counts_are_what_the_case_says():
    q, xy1, t, xy2, F = guided_ref.planted_counts_case(32)
    assert list(guided_ref.band(F, xy1, xy2).sum(axis=1)) == guided_ref.PLANT_COUNTS
    q, xy1, t, xy2, F = guided_ref.all_in_band_case(4, 30, 32)
    assert guided_ref.band(F, xy1, xy2).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_transposition_identity(seed):
    rng = np.random.default_rng(seed)
    xy1, xy2, F, _ = guided_ref.two_view(rng, 90, 70)
    for err in (0.5, 3.0, 1e4, np.inf):
        a = guided_ref.band(F, xy1, xy2, err)
        b = guided_ref.band(F.reshape(3, 3).T, xy2, xy1, err)
        assert np.array_equal(a, b.T)
    Fr = rng.standard_normal(9)                   # not a fundamental matrix: the identity is about the arithmetic
    assert np.array_equal(guided_ref.band(Fr, xy1, xy2, 40.0), guided_ref.band(Fr.reshape(3, 3).T, xy2, xy1, 40.0).T)


def test_rectified_band_is_the_row_distance():
    rng = np.random.default_rng(4)
    xy1 = np.c_[rng.integers(0, 2000, 50), rng.integers(0, 2000, 50)]
    xy2 = np.c_[rng.integers(0, 2000, 400), rng.integers(0, 2000, 400)]
    xy2[7, 1], xy2[8, 1] = xy1[0, 1] + 3, xy1[0, 1] + 4          # planted on and just past the edge
    xy2[9, 1], xy2[10, 1] = xy1[1, 1] - 3, xy1[1, 1] - 4
    m = guided_ref.band(guided_ref.RECT_F, xy1, xy2, 3.0)
    assert np.array_equal(m, np.abs(xy1[:, 1][:, None] - xy2[:, 1][None, :]) <= 3)
    assert m[0, 7] and not m[0, 8] and m[1, 9] and not m[1, 10]


def test_zero_and_degenerate_F_give_nothing():
    q, xy1, t, xy2, F = guided_ref.shape_case(20, 30, 32, seed=43)
    for bad in (np.zeros(9), np.full(9, np.nan), F * 1e200, np.array([0, 0, 0, 0, 0, 0, 0, 0, 1.0])):
        assert not guided_ref.band(bad, xy1, xy2).any()
        out, cand = guided_ref.match_pair(q, xy1, t, xy2, bad, stride=25)
        assert cand == 0 and (out == -1).all() and len(out) == 25


def test_golden_file():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_guided_golden
    g = np.load(GOLDEN)
    want = make_guided_golden.arrays()
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
