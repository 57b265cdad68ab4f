"""GPU suite: the C++ next-view adapter (reconstructor_amd/host/HipNextView.h) run by tests/cpp/next_view_adapter_test on the
reference's containers: at every step calc2d3dMatches and rankNextImages (MatchTotal and MatchDensity, ties included) equal
a plain restatement of the reference's loops written in the driver, on the same maps, and so does step 1."""
import os
import subprocess

import pytest

import tri_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "next_view_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def _write(path, L, init, shape):
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
        f.write("init %d %d\nshape %d %d\n" % (init[0], init[1], shape[0], shape[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [5, 6])
def test_adapter_equals_the_reference_loops(tmp_path, seed):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    L = tri_ref.loop_containers(12, 900, obs_per_point=5, seed=seed, wrong_rate=0.03)
    _write(tmp_path / "in.txt", L, (0, 1), (336, 512))
    r = subprocess.run([BIN, str(tmp_path / "in.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    steps = [w.split() for w in r.stdout.splitlines() if w.startswith("step")]
    assert len(steps) >= 6
    assert [int(s[1]) for s in steps] == list(range(10, 10 - len(steps), -1))      # MatchTotal: every candidate each step
    assert sum(int(s[5]) for s in steps) > 0                                         # step 1 attached observations
    assert r.stdout.splitlines()[-1].startswith("end")
