"""GPU suite: NextViewSearch::registerImagePnP (reconstructor_amd/host/HipNextView.h) run by tests/cpp/pnp_adapter_test on the
reference's containers: the pose of rcn_pnp_ransac, both lists trimmed to the inliers in order, a throw on a view without a
model."""
import os
import subprocess

import numpy as np
import pytest

import pnp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pnp_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_adapter_returns_the_abi_pose_and_trims_the_lists(tmp_path):
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    pts, views = pnp_ref.scene_views(6, 0.3, n_cams=5, n_pts=500)
    views = [(10 + i, v["landmark"], v["xy"], v["intr6"]) for i, v in enumerate(views)]
    views.append((30, np.full(40, 3, np.int32), views[0][2][:40], views[0][3]))          # one landmark only: no model
    views.append((31, views[1][1][:3], views[1][2][:3], views[1][3]))                    # fewer than 4 entries
    with open(tmp_path / "in.txt", "w") as f:
        f.write("points %d\n" % len(pts))
        for p in pts:
            f.write(" ".join(repr(float(x)) for x in p) + "\n")
        f.write("views %d\n" % len(views))
        for img, lm, xy, K in views:
            f.write("%d " % img + " ".join(repr(float(k)) for k in K) + " %d\n" % len(lm))
            f.write(" ".join("%d %d %d" % (l, x, y) for l, (x, y) in zip(lm, xy)) + "\n")
    r = subprocess.run([BIN, str(tmp_path / "in.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "end"
    rows = [l.split() for l in lines if l.startswith("view")]
    assert len(rows) == len(views)
    for row, (img, lm, xy, K) in zip(rows, views):
        want = pnp_ref.pnp_ransac(lm, xy, pts, K)
        assert int(row[1]) == img and int(row[2]) == want["count"]
        assert row[3] == ("threw" if want["count"] < 0 else str(want["count"]))
    assert [row[3] for row in rows[-2:]] == ["threw", "threw"] and [int(row[2]) for row in rows[-2:]] == [-1, -2]
