"""GPU suite: the C++ triangulation adapter (reconstructor_amd/host/HipTriangulator.h) run by tests/cpp/triangulate_adapter_test
on the reference's containers -- triangulateInitialPair, then triangulateMatchedLandmarks for every further view -- against
the reference's loops restated one triangulateMultiView call at a time (tests/tri_ref.py), in the iteration orders of the
driver's own std::unordered_maps."""
import os
import subprocess

import pytest

import tri_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "triangulate_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def _write(path, L, init, views):
    imgs = sorted(L["coords"])
    with open(path, "w") as f:
        f.write("images %d\n" % len(imgs))
        for i in imgs:
            f.write("%d %d\n" % (i, len(L["coords"][i])))
            f.write(" ".join(repr(float(v)) for v in L["poses34"][i]) + "\n")
            f.write(" ".join(repr(float(v)) for v in L["intrinsics"][i]) + "\n")
            f.write(" ".join("%d %d" % xy for xy in L["coords"][i]) + "\n")
        f.write("pairs %d\n" % len(L["feature_matches"]))
        for (i, j), m in L["feature_matches"].items():
            f.write("%d %d %d " % (i, j, len(m)) + " ".join("%d %d" % kv for kv in m.items()) + "\n")
        for i in imgs:
            f.write("%d " % len(L["img_matches"][i]) + " ".join(map(str, L["img_matches"][i])) + "\n")
        f.write("init %d %d\nviews %d %s\n" % (init[0], init[1], len(views), " ".join(map(str, views))))


def _read(path):
    pair_order, reg_orders, lms, ids = None, {}, [], {}
    for line in open(path):
        w = line.split()
        if w[0] == "pairorder":
            pair_order = [int(x) for x in w[1:]]
        elif w[0] == "regorder":
            v = int(w[1])
            reg_orders[v] = [(int(w[k]), w[k + 1] == "1") for k in range(2, len(w), 2)]
        elif w[0] == "lm":
            n = int(w[4])
            lms.append({"xyz": [float.fromhex(x) for x in w[1:4]], "track": [(int(w[5 + 2 * k]), int(w[6 + 2 * k])) for k in range(n)]})
        elif w[0] == "ids":
            ids[int(w[1])] = [int(x) for x in w[2:]]
    return pair_order, reg_orders, lms, ids


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 4])
def test_adapter_equals_the_sequential_loop(tmp_path, seed):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    L = tri_ref.loop_containers(9, 800, obs_per_point=5, seed=seed, wrong_rate=0.03)
    init, views = (0, 1), [2, 3, 4, 5, 6, 7, 8]
    _write(tmp_path / "in.txt", L, init, views)
    subprocess.run([BIN, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], check=True, timeout=300)
    pair_order, reg_orders, got, got_ids = _read(tmp_path / "out.txt")
    # the reference's loops in the driver's iteration orders, one triangulateMultiView at a time
    fm = dict(L["feature_matches"])
    fm[init] = {q: fm[init][q] for q in pair_order}
    assert sorted(pair_order) == sorted(L["feature_matches"][init])
    co, ids, im, P, K = L["coords"], L["landmark_ids"], L["img_matches"], L["poses34"], L["intrinsics"]
    lms = []
    tri_ref.sequential_initial_pair(init[0], init[1], fm, co, ids, lms, P, K)
    for v in views:
        fids, lids = tri_ref.calc_2d3d_matches(v, im, fm, ids, lms)
        tri_ref.sequential_matched_landmarks(v, fids, lids, reg_orders[v], im, fm, co, ids, lms, P, K)
    assert len(got) == len(lms) > 200
    for a, b in zip(got, lms):
        assert a["track"] == b["track"]
        assert [x.hex() for x in a["xyz"]] == [float(x).hex() for x in b["xyz"]]
    assert got_ids == ids
    assert any(len(lm["track"]) > 2 for lm in lms)             # step 1 attached observations to existing landmarks
