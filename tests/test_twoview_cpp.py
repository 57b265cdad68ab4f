"""GPU suite: NextViewSearch::chooseInitialPair (reconstructor_amd/host/HipNextView.h) and GeometricFilter::estimateEssential
(HipGeometricFilter.h) run by tests/cpp/twoview_adapter_test on the reference's containers: the canonical pair, the pose and E
of the Python entry bit for bit, the mask filled."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tri_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "twoview_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter headers and their driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_adapter_reproduces_the_python_entry(tmp_path, gpu_ctx):
    from reconstructor_amd import twoview
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    L = tri_ref.loop_containers(25, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    co, fm, K = L["coords"], L["feature_matches"], L["intrinsics"]
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
    r = subprocess.run([BIN, str(tmp_path / "in.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "end"
    off = np.concatenate([[0], np.cumsum([len(fm[k]) for k in keys])])
    i, j, _ = twoview.choose_initial_pair(keys, off)
    qt = sorted(fm[(i, j)].items())
    xy1 = np.array([co[i][a] for a, _ in qt], np.int32)
    xy2 = np.array([co[j][b] for _, b in qt], np.int32)
    want = twoview.two_view_init(gpu_ctx, [0, len(qt)], xy1, xy2, K[i], K[j])
    assert lines[0].split() == ["pair", str(i), str(j), str(len(qt)), str(want["count"][0, 0]), str(want["count"][0, 1])]
    assert (i, j) == (20, 22) and want["count"][0, 0] > 100
    unhex = lambda line: b"".join(struct.pack("<Q", int(w, 16)) for w in line.split()[1:])
    assert lines[1].startswith("pose") and unhex(lines[1]) == want["pose34"].tobytes()
    assert lines[2].startswith("E") and unhex(lines[2]) == want["E"].tobytes()
