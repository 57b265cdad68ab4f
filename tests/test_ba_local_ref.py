"""CPU suite: the judge of the local bundle adjustment (tests/ba_local_ref.py) checked on its own -- the numpy restatement of the
extraction and of the covisibility counts on hand-made graphs, and the independent minimiser against the oracle (one constant camera:
the oracle with that camera moved to index 0) and against itself (trf / dogbox, two or more constant cameras).  No GPU."""
import numpy as np
import pytest

import ba_local_ref as L
from oracle import orc_ba


def test_extraction_on_a_hand_made_graph():
    # landmark: cameras of its track     0: (2, 0)   1: ()   2: (3, 4)   3: (4, 2, 4)   4: (1,)   5: (0, 3)
    tracks = [(2, 0), (), (3, 4), (4, 2, 4), (1,), (0, 3)]
    pt = np.repeat(np.arange(6), [len(t) for t in tracks]).astype(np.int32)
    cam = np.concatenate([np.array(t, np.int32) for t in tracks])
    e = L.extract(L.mask(6, (2, 5)), 6, pt, cam)                 # camera 5 is free and sees nothing
    assert e["sel"].tolist() == [True, False, False, True, False, False]
    assert e["pt_map"].tolist() == [0, 3] and e["cam_map"].tolist() == [0, 2, 4]            # cameras 1 and 3 see no selected landmark
    assert e["obs"].tolist() == [0, 1, 4, 5, 6]
    assert e["ocam"].tolist() == [1, 0, 2, 1, 2] and e["opt"].tolist() == [0, 0, 1, 1, 1]   # track order kept, the repeat too
    assert e["constant"].tolist() == [True, False, True]
    every = L.extract(np.ones(6, bool), 6, pt, cam)              # all free: the identity on what has observations
    assert every["pt_map"].tolist() == [0, 2, 3, 4, 5] and every["cam_map"].tolist() == [0, 1, 2, 3, 4] and not every["constant"].any()
    none = L.extract(L.mask(6, (5,)), 6, pt, cam)
    assert len(none["pt_map"]) == 0 and len(none["cam_map"]) == 0 and len(none["obs"]) == 0


def test_covisibility_counts_and_choice():
    tracks = [(2, 0), (), (3, 4), (4, 2, 4), (1,), (0, 3), (2, 3, 2), (2, 4)]
    pt = np.repeat(np.arange(8), [len(t) for t in tracks]).astype(np.int32)
    cam = np.concatenate([np.array(t, np.int32) for t in tracks])
    c = L.covisible_counts(6, 8, pt, cam, 2)
    assert c.tolist() == [1, 0, 4, 1, 2, 0]                       # landmark 6 sees camera 2 twice: once; landmark 3 sees 4 twice: once
    assert L.covisible_pick(c, 2, 5).tolist() == [4, 0, 3]        # the tie of 0 and 3 to the lower index; fewer than k share any
    assert L.covisible_pick(c, 2, 1).tolist() == [4] and L.covisible_pick(c, 2, 0).tolist() == []
    assert L.covisible_counts(6, 8, pt, cam, 5).tolist() == [0] * 6


@pytest.mark.parametrize("nc,npts,seed,const", L.ONE_CONSTANT)
def test_judge_agrees_with_the_oracle_for_one_constant_camera(nc, npts, seed, const):
    """One constant camera = the oracle's fix_cam0_pose with that camera at index 0, camera 1's translation free, mode 0.  Only the RMS
    is compared: the scale is free and two minimisers drift along it differently."""
    sc = L.scene(nc, npts, seed)
    _, _, r = L.judged(nc, npts, seed, const)
    perm, _ = L.permuted_to_front(sc, const[0])
    o = orc_ba.default_options(nc)
    o.intrinsics_mode, o.fix_cam0_pose, o.fix_cam1_translation = 0, 1, 0
    _, _, _, s = orc_ba.solve(perm, o, threads=2)
    print("one constant camera %s of %d: judge %.12f px, oracle %.12f px, difference %.3e" % (const, nc, r, s["final_rms_px"], abs(r - s["final_rms_px"])))
    assert abs(r - s["final_rms_px"]) <= 1e-5
    assert r < L.rms(sc)


@pytest.mark.parametrize("nc,npts,seed,const", L.MANY_CONSTANT)
def test_two_minimisers_of_the_judge_agree_when_the_gauge_is_fixed(nc, npts, seed, const):
    d_rms, d_pose, d_pts = L.spread(nc, npts, seed, const)
    print("constant %s of %d: trf / dogbox differ by %.3e px in RMS, %.3e in the poses, %.3e in the points" % (const, nc, d_rms, d_pose, d_pts))
    P, X, r = L.judged(nc, npts, seed, const)
    sc = L.scene(nc, npts, seed)
    m = L.mask(nc, const)
    assert P[m].tobytes() == sc["poses"][m].tobytes()            # the constant cameras did not move
    assert d_rms <= 1e-9 and d_pose <= 1e-6 and d_pts <= 1e-4     # (measured: 9e-16, 1.4e-9, 1e-6)
    assert r < L.rms(sc)
    # the record the GPU suites read (tests/golden/ba_local_judge.npz) is this judge's: within the margin they grant the library
    Pg, Xg, rg, sg = L.recorded(nc, npts, seed, const)
    seen = np.zeros(npts, bool)
    seen[sc["obs_pt"]] = True
    assert abs(rg - r) <= 1e-9 and np.abs(Pg - P).max() <= max(100 * d_pose, 1e-9) and np.abs(Xg - X)[seen].max() <= max(100 * d_pts, 1e-9)
    assert sg[0] <= 1e-9 and sg[1] <= 1e-6 and sg[2] <= 1e-4
