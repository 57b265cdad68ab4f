"""CPU suite: the reference's calc2d3dMatches / rankNextImages / step 1 of triangulateMatchedLandmarks, transcribed literally
(tests/nextview_ref.py), against the restatement the next-view kernels implement (obs_of + list walk + order by observation,
first passing entry per feature wins): on seeded containers, with mirror on and off, pairs given both ways with different
lists, empty lists, repeated landmarks and features."""
import numpy as np
import pytest

import nextview_ref as nr
from reconstructor_amd import nextview


def _both(L, lists, mirror):
    off, img, feat = nextview.graph_arrays(L["tracks"])
    pairs, offsets, qt = nextview.lists_from_dict(lists)
    cand = L["candidates"]
    shapes = [L["shapes"][c] for c in cand]
    got = nr.vector_corr(off, img, feat, pairs, offsets, qt, mirror, cand, shapes, L["coords"])
    lids, fids = nr.literal_calc_2d3d_matches(cand, L["img_matches"], L["feature_matches"], L["landmark_ids"], L["tracks"])
    return got, lids, fids


def _check(L, got, lids, fids):
    coff, lm, ft, cells, _ = got
    for k, c in enumerate(L["candidates"]):
        assert lm[coff[k]:coff[k + 1]].tolist() == lids[c]
        assert ft[coff[k]:coff[k + 1]].tolist() == fids[c]
        assert cells[k] == nr.literal_density(fids[c], L["coords"][c], L["shapes"][c])


@pytest.mark.parametrize("seed,mirror", [(1, False), (1, True), (2, True), (3, False)])
def test_walk_equals_the_reference_loop(seed, mirror):
    L = nr.make_case(14, 700, seed=seed)
    lists = nr.canonical_lists(L["feature_matches"]) if mirror else L["feature_matches"]
    got, lids, fids = _both(L, lists, mirror)
    _check(L, got, lids, fids)
    coff, lm, ft, _, outside = got
    assert coff[-1] > 500
    assert any(len(set(v)) < len(v) for v in lids.values())          # a landmark twice for one candidate
    assert any(len(set(v)) < len(v) for v in fids.values())          # a feature twice ("a feature possibly twice")
    assert outside.sum() > 0                                           # out-of-frame keypoints of synth_ba


def test_pairs_given_both_ways_with_different_lists_and_empty_lists():
    L = nr.make_case(12, 600, seed=7)
    fm = L["feature_matches"]
    rng = np.random.default_rng(0)
    keys = sorted(k for k in fm if k[0] < k[1])
    for (i, j) in keys[::3]:                                  # (j, i) no longer the inverse of (i, j)
        back = fm[(j, i)]
        drop = [g for g in back if rng.random() < 0.4]
        for g in drop:
            del back[g]
    for k in keys[1::7]:                                      # empty lists, both directions
        fm[k] = {}
        fm[(k[1], k[0])] = {}
    for mirror in (False, True):
        got, lids, fids = _both(L, fm, mirror)
        _check(L, got, lids, fids)
    # mirror with only one direction of an edited pair: the reverse is read backwards, which differs from the edited list
    half = nr.canonical_lists(fm)
    got = nr.vector_corr(*nextview.graph_arrays(L["tracks"]), *nextview.lists_from_dict(half), True, L["candidates"],
                         [L["shapes"][c] for c in L["candidates"]], L["coords"])
    assert got[0][-1] >= 0


def test_rank_modes():
    L = nr.make_case(16, 900, seed=5)
    got, lids, fids = _both(L, L["feature_matches"], False)
    cand = L["candidates"]
    coff, _, _, cells, _ = got
    counts = np.diff(coff)
    order = nextview.rank_next_images(cand, counts, cells, nextview.MATCH_DENSITY, 30)
    ref = nr.literal_rank(lids, fids, "density", L["coords"], L["shapes"], 30)
    assert order and ref
    assert sorted(order) == sorted(c for c, s in zip(cand, cells) if s > 30)
    top = max(cells)
    if list(cells).count(top) == 1:
        assert order[0] == ref[0]
    assert set(ref) <= set(order)
    assert nextview.rank_next_images(cand, counts, cells, nextview.MATCH_TOTAL) == nr.literal_rank(lids, fids, "total", L["coords"], L["shapes"])
    # the reference's map keeps one image per score: the last in iteration order
    s2 = {c: 40 for c in cand[:3]}
    f2 = {c: fids[c] for c in cand[:3]}
    for rev in (False, True):
        o = list(reversed(cand[:3])) if rev else cand[:3]
        r = nr.literal_rank({c: lids[c] for c in cand[:3]}, f2, "density", L["coords"], L["shapes"], 0, order=o)
        assert r[0] in cand[:3]
    assert nextview.rank_next_images(cand[:3], [1, 1, 1], [s2[c] for c in cand[:3]]) == sorted(cand[:3])


def test_cells_at_the_frame_edge():
    rows, cols = nr.SHAPE
    assert nr.cell_of(0, 0, rows, cols) == (0, 0)
    assert nr.cell_of(-1, -1, rows, cols) == (0, 0)                       # truncation toward zero
    assert nr.cell_of(-cols // 32, 5, rows, cols) is None                 # exactly -1
    assert nr.cell_of(cols - 1, rows - 1, rows, cols) == (31, 31)
    assert nr.cell_of(cols, 0, rows, cols) is None
    assert nr.cell_of(0, rows, rows, cols) is None


def test_attach_rule_equals_the_sequential_loop():
    rng = np.random.default_rng(3)
    P = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    K = [600.0, 600.0, 256.0, 168.0, 0.0, 0.0]
    pts = np.column_stack([rng.uniform(-1, 1, 200), rng.uniform(-1, 1, 200), rng.uniform(-1, 6, 200)])
    ents = []
    for e in range(3000):
        l = int(rng.integers(0, 200))
        X = pts[l]
        u = 600 * X[0] / X[2] + 256 if X[2] != 0 else 0
        v = 600 * X[1] / X[2] + 168 if X[2] != 0 else 0
        ents.append((l, int(rng.integers(0, 300)), (int(np.clip(np.round(u + rng.normal(0, 3)), -1e6, 1e6)),
                                                    int(np.clip(np.round(v + rng.normal(0, 3)), -1e6, 1e6)))))
    a = nr.literal_attach(P, K, pts, ents)
    b = nr.vector_attach(P, K, pts, ents)
    assert a == b
    assert {0, 1, 2, 3} <= set(a)
