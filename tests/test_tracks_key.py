"""csrc/tracks_key.h is the one text of the conflict table's key packing, hash and sizing for the GPU kernels, the host sizing and host
C++.  No GPU here: tests/cpp/tracks_key_test.cpp includes that header alone, built with g++ and the address and undefined-behaviour
sanitizers, inserts the items of a file sequentially and prints key, hash, cell and count of each; they must equal the restatement
below, number for number."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tracks_key") / "tracks_key_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(ROOT, "tests", "cpp", "tracks_key_test.cpp")])
    return out


def key_of(root, slot):
    return (root << 14) | slot


def hash_of(k):
    k ^= k >> 30
    k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 27
    k = (k * 0x94d049bb133111eb) & M64
    return k ^ (k >> 31)


def cells_for(n):
    c = 64
    while c < 2 * n:
        c <<= 1
    return c


def restated(items):
    cells = cells_for(len(items))
    keys, cnt, out = {}, {}, []
    for r, s in items:
        k = key_of(r, s)
        c = hash_of(k) & (cells - 1)
        while c in keys and keys[c] != k:
            c = (c + 1) & (cells - 1)
        keys[c] = k
        cnt[c] = cnt.get(c, 0) + 1
        out.append((k, hash_of(k), c, cnt[c]))
    return out, cells


def _cases():
    rng = np.random.default_rng(11)
    big = 2 ** 31 - 2
    yield "empty", []
    yield "extremes", [(0, 0), (big, 16383), (big, 0), (0, 16383), (big, 16383), (1, 1)]
    yield "consecutive_roots", [(r, s) for r in range(0, 3000, 7) for s in range(3)]
    yield "one_component", [(12345, int(s)) for s in rng.integers(0, 12, 5000)]          # a giant component: 12 keys, large counts
    yield "random", [(int(r), int(s)) for r, s in zip(rng.integers(0, big, 4000), rng.integers(0, 16384, 4000))]
    yield "size_edges_32", [(i, 0) for i in range(32)]                                   # 2 n == the minimum table exactly
    yield "size_edges_33", [(i, 0) for i in range(33)]


@pytest.mark.parametrize("name,items", list(_cases()), ids=[n for n, _ in _cases()])
def test_header_equals_restatement(exe, tmp_path, name, items):
    path = str(tmp_path / "items.txt")
    with open(path, "w") as f:
        f.writelines("%d %d\n" % it for it in items)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.split("\n")
    want, cells = restated(items)
    assert lines[len(items)] == "cells %d" % cells
    got = [tuple(int(v) for v in ln.split()) for ln in lines[:len(items)]]
    assert got == want
    if name == "one_component":
        assert len({c for _, _, c, _ in got}) == 12 and max(n for _, _, _, n in got) > 300
    if name.startswith("size_edges"):
        assert cells == (64 if name.endswith("32") else 128)
