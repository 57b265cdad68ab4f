"""GPU suite: Triangulator::triangulateMatchedLandmarksDevice (reconstructor_amd/host/HipTriangulator.h) run by
tests/cpp/new_view_tracks_adapter_test next to the host method on equal containers: the same landmarks bit for bit, the same
tracks in the same order, the same landmarkId on every feature, and the device's table equal to the containers."""
import os
import subprocess

import pytest

import tri_ref
from test_triangulate_cpp import _write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "new_view_tracks_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


def test_host_loop_timer_counts_the_tracks_of_the_walk(tmp_path):
    """CPU tier: the driver's timing mode walks the reference's containers (no GPU) and finds the tracks of the host walk."""
    import nvt_ref
    from reconstructor_amd import triangulate as tri
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    L = nvt_ref.scene(8, 400, 5, 2)
    v, ids = L["v"], L["landmark_ids"]
    reg = [(r, True) for r, s in L["registered"] if s]
    with open(tmp_path / "t.txt", "w") as f:
        f.write("view %d %d %d\n%s\n" % (v, len(ids[v]), len(reg), " ".join(map(str, ids[v]))))
        for r, _ in reg:
            m = L["feature_matches"].get((v, r), {})
            f.write("%d %d %d\n%s\n%s\n" % (r, len(ids[r]), len(m), " ".join(map(str, ids[r])), " ".join("%d %d" % kv for kv in m.items())))
    out = subprocess.run([BIN, "--time-host-loop", str(tmp_path / "t.txt"), "3"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert out[0] == "host_loop" and int(out[2]) == len(tri.new_view_tracks(v, ids, reg, L["img_matches"], L["feature_matches"])) > 0


def _read(path):
    runs = {"host": {"lms": [], "ids": {}}, "dev": {"lms": [], "ids": {}, "table": {}}}
    last = None
    for line in open(path):
        w = line.split()
        last = w[0]
        if len(w) < 2:
            continue
        r = runs[w[0]]
        if w[1] == "lm":
            n = int(w[5])
            r["lms"].append(([x for x in w[2:5]], [(int(w[6 + 2 * k]), int(w[7 + 2 * k])) for k in range(n)]))
        else:
            r[w[1]][int(w[2])] = [int(x) for x in w[3:]]
    assert last == "end"
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 4])
def test_device_method_equals_the_host_method(tmp_path, seed):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    L = tri_ref.loop_containers(9, 800, obs_per_point=5, seed=seed, wrong_rate=0.03)
    _write(tmp_path / "in.txt", L, (0, 1), [2, 3, 4, 5, 6, 7, 8])
    r = subprocess.run([BIN, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    runs = _read(tmp_path / "out.txt")
    host, dev = runs["host"], runs["dev"]
    assert len(host["lms"]) > 200
    assert sum(t[1][0] >= 2 for _, t in host["lms"]) > 50                   # landmarks of step 3: (registered, new view), behind the initial pair's
    assert dev["lms"] == host["lms"]                                        # hex floats and tracks, in order
    assert dev["ids"] == host["ids"] and len(host["ids"]) == 9
    assert dev["table"] == dev["ids"]
    assert any(len(t) > 2 for _, t in host["lms"])                          # step 1 attached observations to existing landmarks
