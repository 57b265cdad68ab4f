"""csrc/guided_band.h is the one text of the epipolar band for the GPU kernels and for host C++.  No GPU here: tests/cpp/guided_band_test.cpp
includes that header alone, built with g++, -ffp-contract=off and the address and undefined-behaviour sanitizers, evaluates it on the golden
coordinates (and on knife-edge and degenerate cases) and prints the masks; they must equal tests/guided_ref.py's numpy band bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import guided_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "guided_small.npz")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("guided_band") / "guided_band_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "guided_band_test.cpp")])
    return out


def _cases():
    g = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in g.files})
    out = [(n, g[n + ".xy1"], g[n + ".xy2"], g[n + ".F"], 3.0) for n in names]
    n0 = names[0]
    rng = np.random.default_rng(3)
    out.append(("zero_F", g[n0 + ".xy1"], g[n0 + ".xy2"], np.zeros(9), 3.0))
    out.append(("nan_F", g[n0 + ".xy1"], g[n0 + ".xy2"], np.full(9, np.nan), 3.0))
    out.append(("huge_F", g[n0 + ".xy1"], g[n0 + ".xy2"], g[n0 + ".F"] * 1e200, 3.0))          # q overflows: no candidates
    out.append(("inf_thr", g[n0 + ".xy1"], g[n0 + ".xy2"], g[n0 + ".F"], np.inf))
    out.append(("wide", g[n0 + ".xy1"], g[n0 + ".xy2"], g[n0 + ".F"], 1e4))
    ys = np.arange(-6, 7)                                # rectified: rows at every offset around the 3 px edge
    out.append(("rect_edges", np.c_[rng.integers(0, 50, 13), np.full(13, 40)], np.c_[rng.integers(0, 50, 13), 40 + ys], guided_ref.RECT_F, 3.0))
    out.append(("empty", np.zeros((0, 2), np.int32), g[n0 + ".xy2"], g[n0 + ".F"], 3.0))
    return out


def test_header_equals_numpy_bit_for_bit(exe, tmp_path):
    cases = _cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for _, xy1, xy2, F, err in cases:
            f.write("%d %d\n" % (len(xy1), len(xy2)))
            f.write(" ".join(float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else "inf")
                             for v in [guided_ref.thr2_of(err)] + list(np.asarray(F, np.float64))) + "\n")
            for x, y in list(np.asarray(xy1).reshape(-1, 2)) + list(np.asarray(xy2).reshape(-1, 2)):
                f.write("%d %d\n" % (x, y))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.split("\n")
    assert "%d cases done" % len(cases) in r.stdout
    at = 0
    for name, xy1, xy2, F, err in cases:
        K1, K2 = len(xy1), len(xy2)
        assert lines[at] == "case %d %d" % (K1, K2), name
        got = np.array([[c == "1" for c in lines[at + 1 + q]] for q in range(K1)], bool).reshape(K1, K2)
        at += 1 + K1
        want = guided_ref.band(F, xy1, xy2, err)
        assert np.array_equal(got, want), name
        if name in ("zero_F", "nan_F", "huge_F"):
            assert not got.any()
        if name == "inf_thr":
            assert got.all()
        if name == "rect_edges":
            assert np.array_equal(got[0], np.abs(np.arange(-6, 7)) <= 3)
