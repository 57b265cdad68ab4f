"""csrc/mvs_geom.h is the one text of the plane sweep's arithmetic for the GPU kernels, for the host entries rcn_mvs_inv_depths and
rcn_mvs_homographies (whose bodies it holds) and for host C++.  No GPU here: tests/cpp/mvs_host_test.cpp, a stand-alone program that
includes the header alone, is built with g++, -ffp-contract=off and the address and undefined-behaviour sanitizers, evaluates every
function of the header on random cameras and edge cases and prints hexadecimal doubles; they must equal tests/mvs_ref.py bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import mvs_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mvs_host") / "mvs_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, os.path.join(ROOT, "tests", "cpp", "mvs_host_test.cpp")])
    return out


def _hex(v):
    v = float(v)
    return v.hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run(exe, tmp_path, lines, n_cases):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    out = r.stdout.strip().split("\n")
    assert out[-1] == "%d cases done" % n_cases
    return out[:-1]


def _bits(words):
    return np.array([float.fromhex(w) if w not in ("nan", "-nan", "inf", "-inf") else float(w) for w in words], np.float64).view(np.uint64)


def random_cameras(rng, n):
    """Rows of [R | t] with R an exact-enough rotation (QR of a random matrix) and intrinsics with distortion."""
    P, K = np.zeros((n, 12)), np.zeros((n, 6))
    for i in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        R = np.eye(3) + 0.1 * (Q - np.eye(3)) if i else np.eye(3)          # not orthonormal for i > 0: the formula does not care
        P[i] = np.c_[R, rng.uniform(-1, 1, 3)].reshape(12)
        K[i] = [rng.uniform(50, 900), rng.uniform(50, 900), rng.uniform(10, 400), rng.uniform(10, 300), rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05)]
    return P, K


def test_inv_depths_and_homographies_equal_numpy_bit_for_bit(exe, tmp_path):
    rng = np.random.default_rng(32)
    lines, want = [], []
    for near, far, D in ((3.0, 8.0, 32), (0.7, 0.7, 4), (1.0, 1e6, 1), (2.5, 40.0, 2), (1e-3, 3.0, 1024)):
        lines.append("inv %s %s %d" % (_hex(near), _hex(far), D))
        want.append(M.inv_depths(near, far, D))
    for near, far, D in ((0.0, 1.0, 4), (2.0, 1.0, 4), (1.0, np.inf, 4), (1.0, 2.0, 0), (1.0, 2.0, 1025), (np.nan, 2.0, 3)):
        lines.append("inv %s %s %d" % (_hex(near), _hex(far), D))
        want.append(None)
    plane_lists = [M.inv_depths(3.0, 8.0, 7), M.inv_depths(3.0, 8.0, 5)[::-1].copy(), np.array([0.2]), np.array([0.1, 0.1, 0.3, 0.3]), np.array([0.0, -0.5, 1e3])]
    for trial in range(12):
        nc = int(rng.integers(2, 6))
        P, K = random_cameras(rng, nc)
        ref = int(rng.integers(0, nc))
        S = int(rng.integers(1, 5))
        srcs = [int(rng.choice([c for c in range(-1, nc) if c != ref])) for _ in range(S)]
        inv = plane_lists[trial % len(plane_lists)]
        lines.append("hom %d %d %d %d %s %s %s %s" % (nc, ref, S, len(inv), " ".join(_hex(v) for v in P.ravel()), " ".join(_hex(v) for v in K.ravel()),
                                                      " ".join(str(s) for s in srcs), " ".join(_hex(v) for v in inv)))
        want.append(M.homographies(P, K, ref, srcs, inv).ravel())
    P, K = random_cameras(rng, 3)
    lines.append("hom 3 1 2 1 %s %s 0 1 %s" % (" ".join(_hex(v) for v in P.ravel()), " ".join(_hex(v) for v in K.ravel()), _hex(0.2)))       # its own source
    want.append(None)
    got = _run(exe, tmp_path, lines, len(lines))
    for line, w, g in zip(lines, want, got):
        if w is None:
            assert g == "bad", line[:60]
        else:
            assert np.array_equal(_bits(g.split()), np.asarray(w, np.float64).view(np.uint64)), line[:60]


def test_sample_positions_costs_and_geometry_equal_numpy_bit_for_bit(exe, tmp_path):
    rng = np.random.default_rng(33)
    lines, checks = [], []
    rows, cols = 13, 17
    P, K = random_cameras(rng, 2)
    P[1, 3] += 0.4
    Hs = [M.homography(P[0], K[0], P[1], K[1], v) for v in (0.2, 0.01)]
    Hs.append(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1]))                      # the identity: every pixel on itself
    Hs.append(np.array([1.0, 0, 0.5 / 32, 0, 1, -0.5 / 32, 0, 0, 1]))       # halves of a 1/32 step: floor(x + 0.5) rounds them up, and just below 0 is outside
    Hs.append(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, -1]))                     # w < 0: behind
    Hs.append(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 0]))                      # w = 0
    Hs.append(np.array([np.nan, 0, 0, 0, 1, 0, 0, 0, 1]))
    Hs.append(np.array([1.0, 0, 1e300, 0, 1, 0, 0, 0, 1e-300]))             # u overflows
    for H in Hs:
        lines.append("warp %d %d %s" % (rows, cols, " ".join(_hex(v) for v in H)))
        qu, qv, ok = M.warp(np.asarray(H, np.float64), rows, cols)
        checks.append(("warp", " ".join("%d %d" % (a, b) if o else "- -" for a, b, o in zip(qu.ravel(), qv.ravel(), ok.ravel()))))
    img = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    for qu, qv in ((0, 0), (32 * (cols - 1), 32 * (rows - 1)), (32 * (cols - 1), 5), (7, 32 * (rows - 1)), (100, 77), (31, 31), (33, 64)):
        lines.append("sample %d %d %d %d %s" % (rows, cols, qu, qv, " ".join(str(v) for v in img.ravel())))
        checks.append(("int", str(int(M.sample(img, np.array([qu]), np.array([qv]))[0]))))
    for n in (9, 49, 121):
        for _ in range(6):
            a, b = rng.integers(0, 256, n), rng.integers(0, 255 * 1024 + 1, n)
            Sa, Saa, Sb, Sbb, Sab = int(a.sum()), int((a * a).sum()), int(b.sum()), int((b * b).sum()), int((a * b).sum())
            Va = n * Saa - Sa * Sa
            lines.append("cost %d %d %d %d %d %d" % (n, Sa, Va, Sb, Sbb, Sab))
            c = 1.0 - np.float64(n * Sab - Sa * Sb) / np.sqrt(np.float64(Va) * np.float64(n * Sbb - Sb * Sb))
            checks.append(("f", [c]))
    lines.append("cost 9 900 90 9 9 900")                                   # a constant source patch: Vb = 0
    checks.append(("raw", "-"))
    big = 121 * 255 * 1024
    lines.append("cost 121 %d %d %d %d %d" % (121 * 255, 121 * 121 * 255 * 255 - (121 * 254) ** 2, big - 1024, (big - 1024) * 255 * 1024, 255 * (big - 1024)))
    checks.append(("any", None))                                            # the largest sums: no overflow under the sanitizer
    for cm, c0, cp, hm, hp in ((0.5, 0.2, 0.4, 1, 1), (0.2, 0.2, 0.2, 1, 1), (0.9, 0.2, 0.21, 1, 1), (0.21, 0.2, 0.9, 1, 1), (0.5, 0.2, 0.4, 0, 1), (0.5, 0.2, 0.4, 1, 0),
                           (0.1, 0.2, 0.1, 1, 1), (0.3, 0.2, 0.3, 1, 1)):
        for im, i0, ip in ((0.1, 0.15, 0.2), (0.3, 0.2, 0.15), (0.2, 0.2, 0.2)):
            lines.append("refine %s %s %s %d %d %s %s %s" % (_hex(cm), _hex(c0), _hex(cp), hm, hp, _hex(im), _hex(i0), _hex(ip)))
            vol = np.array([cm if hm else np.inf, c0, cp if hp else np.inf]).reshape(3, 1, 1)
            checks.append(("f", [M.refine(vol, np.array([[1]]), [im, i0, ip])[0, 0]]))
    for _ in range(8):
        x, y, z = int(rng.integers(0, 500)), int(rng.integers(0, 400)), float(np.float32(rng.uniform(0.5, 30)))
        lines.append("lift %s %s %d %d %s" % (" ".join(_hex(v) for v in P[1]), " ".join(_hex(v) for v in K[1, :4]), x, y, _hex(z)))
        depth = np.zeros((y + 1, x + 1), np.float32)
        depth[y, x] = z
        X = M.lift(P[1], K[1], depth)[y, x]
        checks.append(("f", X))
        lines.append("proj %s %s %s" % (" ".join(_hex(v) for v in P[0]), " ".join(_hex(v) for v in K[0, :4]), " ".join(_hex(v) for v in X)))
        checks.append(("f", [float(v[0]) for v in M.project(P[0], K[0], X[None])]))
        lines.append("dist %s %d %d" % (" ".join(_hex(v) for v in K[1]), x, y))
        ys, xs = np.float64(y), np.float64(x)
        xn, yn = (xs - K[1, 2]) / K[1, 0], (ys - K[1, 3]) / K[1, 1]
        rho = xn * xn + yn * yn
        d = K[1, 4] * rho + (K[1, 5] * rho) * rho
        checks.append(("f", [K[1, 0] * (xn + d) + K[1, 2], K[1, 1] * (yn + d) + K[1, 3]]))
    got = _run(exe, tmp_path, lines, len(lines))
    for line, (kind, w), g in zip(lines, checks, got):
        if kind == "f":
            assert np.array_equal(_bits(g.split()), np.asarray(w, np.float64).view(np.uint64)), line[:50]
        elif kind != "any":
            assert g.strip() == w, line[:50]
