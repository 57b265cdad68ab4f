"""GPU suite: NextViewSearch::chooseInitialPairByGeometry (reconstructor_amd/host/HipNextView.h) and
GeometricFilter::estimateHomography (HipGeometricFilter.h) run by tests/cpp/twoview_geometry_adapter_test on the reference's
containers: the driver compares them with the C calls bit for bit; here its report is compared with the Python entries, and
chooseInitialPair with what it gave before."""
import os
import struct
import subprocess

import numpy as np
import pytest

import twoview_ref as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "twoview_geometry_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter headers and their driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def _graph():
    """Six images; the pair with the most matches a pure rotation, the second a tiny baseline, the third general."""
    scenes = {(0, 1): tv.scene_pair(31, 0.1, n=300, baseline=0.0), (2, 3): tv.scene_pair(32, 0.1, n=280, baseline=0.02),
              (4, 5): tv.scene_pair(33, 0.1, n=260), (1, 2): tv.scene_pair(34, 0.1, n=90)}
    coords = {i: [] for i in range(6)}
    intr, fm = {}, {}
    for (i, j), s in scenes.items():
        intr.setdefault(i, s["K1"])
        intr.setdefault(j, s["K2"])
        m = {}
        for a, b in zip(s["xy1"], s["xy2"]):
            m[len(coords[i])] = len(coords[j])
            coords[i].append(tuple(int(v) for v in a))
            coords[j].append(tuple(int(v) for v in b))
        fm[(i, j)] = m
    return coords, intr, fm


@pytest.mark.gpu
@pytest.mark.parametrize("top_m", (10, 2))
def test_adapter_reproduces_the_python_entry(tmp_path, gpu_ctx, top_m):
    from reconstructor_amd import homography, twoview
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    co, K, fm = _graph()
    keys = sorted(fm)
    with open(tmp_path / "in.txt", "w") as f:
        f.write("images %d\n" % len(co))
        for i in sorted(co):
            f.write("%d " % i + " ".join(repr(float(k)) for k in K[i]) + " %d\n" % len(co[i]))
            f.write(" ".join("%d %d" % tuple(p) for p in co[i]) + "\n")
        f.write("pairs %d\n" % len(keys))
        for i, j in keys[::-1]:                       # written backwards: the choice must not depend on the order
            f.write("%d %d %d\n" % (i, j, len(fm[(i, j)])))
            f.write(" ".join("%d %d" % (a, b) for a, b in list(fm[(i, j)].items())[::-1]) + "\n")
    r = subprocess.run([BIN, str(tmp_path / "in.txt"), str(top_m)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "end"
    ents = {k: sorted(fm[k].items()) for k in keys}
    off = np.concatenate([[0], np.cumsum([len(ents[k]) for k in keys])])
    xy1 = np.array([co[i][a] for (i, j) in keys for a, _ in ents[(i, j)]], np.int32)
    xy2 = np.array([co[j][b] for (i, j) in keys for _, b in ents[(i, j)]], np.int32)
    K1, K2 = np.stack([K[i] for i, _ in keys]), np.stack([K[j] for _, j in keys])
    unhex = lambda line: b"".join(struct.pack("<Q", int(w, 16)) for w in line.split() if len(w) == 16)
    # chooseInitialPair: what it gave before
    i, j, k = twoview.choose_initial_pair(keys, off)
    e = twoview.two_view_init(gpu_ctx, [0, len(ents[(i, j)])], xy1[off[k]:off[k + 1]], xy2[off[k]:off[k + 1]], K[i], K[j])
    assert lines[0].split() == ["canonical", str(i), str(j)] and (i, j) == (0, 1)
    assert unhex(lines[1]) == e["pose34"].tobytes()
    o = twoview.geometry_default_options(gpu_ctx)
    o.top_m = top_m
    want = twoview.choose_initial_pair_by_geometry(gpu_ctx, keys, off, xy1, xy2, K1, K2, o)
    assert lines[2].split() == ["chosen", str(want["pair"][0]), str(want["pair"][1]), str(want["position"]), str(int(want["fallback"]))]
    assert (want["pair"], want["fallback"]) == (((4, 5), False) if top_m == 10 else ((0, 1), True))
    t, nc = want["table"], len(want["candidates"])
    for c in range(nc):
        a, b = keys[want["candidates"][c]]
        w = lines[3 + c].split()
        assert w[:8] == ["cand", str(a), str(b), str(len(ents[(a, b)])), str(t["count"][c, 0]), str(t["count"][c, 1]), str(t["h_count"][c]), str(t["label"][c])]
        assert unhex(lines[3 + c]) == t["ratio"][c].tobytes() and unhex(lines[3 + nc + c]) == t["median_angle"][c].tobytes()
    rest = lines[3 + 2 * nc:]
    assert rest[0].startswith("pose") and unhex(rest[0]) == want["pose34"].tobytes()
    kk = want["index"]
    h = homography.find(gpu_ctx, [0, off[kk + 1] - off[kk]], xy1[off[kk]:off[kk + 1]], xy2[off[kk]:off[kk + 1]])
    assert rest[1].startswith("H") and unhex(rest[1]) == h["H"].tobytes() and rest[2].split() == ["hcount", str(h["count"][0])]
