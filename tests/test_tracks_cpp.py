"""TrackBuilder (reconstructor_amd/host/HipTrackBuilder.h) run by tests/cpp/tracks_adapter_test: build() on the reference's containers
and buildDevice()'s CSR equal a sequential union-find written in the driver itself, under both conflict policies, a selection and
min_length 3."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "tracks_adapter_test")


def test_driver_builds_without_gpu():
    """CPU tier: the adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_adapter_equals_the_drivers_union_find():
    assert os.path.exists(BIN), "run __graft_entry__.build() first"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    w = r.stdout.split()
    assert w[0] == "tracks" and w[5] == "observations"
    a, b, c, d, obs = (int(w[k]) for k in (1, 2, 3, 4, 6))
    assert a > 50 and b > a and 0 < c < a and d == c and obs >= 2 * a      # DROP_IMAGE keeps more; the selection and min_length 3 fewer
