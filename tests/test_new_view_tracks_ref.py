"""CPU suite: the turned-round restatement of step 3 of triangulateMatchedLandmarks (tests/nvt_ref.py: per list the minimum
of (position, partner), read out in feature order -- what csrc/corr2d3d.hip computes) against the literal loop
(reconstructor_amd.triangulate.new_view_tracks) on seeded scenes with 35 % of all ids taken."""
import copy

import numpy as np
import pytest

import nvt_ref
from reconstructor_amd import triangulate as tri


def _both(L, registered=None, img_matches=None, feature_matches=None):
    a = (L["v"], L["landmark_ids"], registered if registered is not None else L["registered"],
         img_matches if img_matches is not None else L["img_matches"],
         feature_matches if feature_matches is not None else L["feature_matches"])
    lit, turned = tri.new_view_tracks(*a), nvt_ref.turned_round(*a)
    assert lit == turned
    assert [t[1][1] for t in lit] == sorted(t[1][1] for t in lit)          # ascending feature of the new image
    return lit, nvt_ref.classify(*a)


@pytest.mark.parametrize("n_images,n_points,opp,seed", [(5, 70, 3, 1), (8, 400, 5, 2), (12, 900, 6, 3)])
def test_turned_round_equals_the_literal_loop(n_images, n_points, opp, seed):
    L = nvt_ref.scene(n_images, n_points, opp, seed)
    lit, kinds = _both(L)
    assert len(lit) == kinds.count(nvt_ref.FIRST) + kinds.count(nvt_ref.FALL_THROUGH)
    assert {nvt_ref.TAKEN, nvt_ref.FIRST, nvt_ref.FALL_THROUGH, nvt_ref.NO_TRACK} <= set(kinds)


def test_the_order_of_registered_decides():
    L = nvt_ref.scene(8, 400, 5, 4)
    rng = np.random.default_rng(9)
    seen = set()
    for _ in range(4):
        reg = [L["registered"][i] for i in rng.permutation(len(L["registered"]))]
        lit, _ = _both(L, registered=reg)
        seen.add(tuple(t[0] for t in lit))
    assert len(seen) > 1                                                   # another order, other partners


def test_status_false_and_unmatched_images_are_not_visited():
    L = nvt_ref.scene(8, 400, 5, 5)
    v = L["v"]
    off = [r for r, s in L["registered"] if not s]
    assert len(off) == 1
    lit, _ = _both(L)
    assert all(t[0][0] != off[0] for t in lit)
    everyone = [(r, True) for r, _ in L["registered"]]
    assert any(t[0][0] == off[0] for t in _both(L, registered=everyone)[0])
    im = copy.deepcopy(L["img_matches"])
    gone = everyone[0][0]
    im[v] = [i for i in im[v] if i != gone]
    lit, _ = _both(L, registered=everyone, img_matches=im)
    assert all(t[0][0] != gone for t in lit)
    assert any(t[0][0] == gone for t in _both(L, registered=everyone)[0])


def test_both_directions_with_different_maps_and_empty_maps():
    L = nvt_ref.scene(8, 400, 5, 6)
    v = L["v"]
    fm = copy.deepcopy(L["feature_matches"])
    r0, r1 = L["registered"][0][0], L["registered"][1][0]
    # (v, r0) and (r0, v) no longer inverse to each other: only (v, r0) is step 3's
    m = fm[(r0, v)]
    keys = list(m)
    fm[(r0, v)] = {keys[i]: m[keys[(i + 1) % len(keys)]] for i in range(len(keys))}
    assert {g: f for f, g in fm[(r0, v)].items()} != fm[(v, r0)]
    base, _ = _both(L)
    assert _both(L, feature_matches=fm)[0] == base
    fm[(v, r1)] = {}                                                       # an empty map: nothing from r1
    lit, _ = _both(L, feature_matches=fm)
    assert all(t[0][0] != r1 for t in lit) and any(t[0][0] == r1 for t in base)
    del fm[(v, r1)]                                                        # no map at all: the same
    assert _both(L, feature_matches=fm)[0] == lit
