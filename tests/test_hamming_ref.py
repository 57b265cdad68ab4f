"""tests/hamming_ref.py is the contract of the Hamming matcher.  Here it is checked against a literal double loop with Python's
int.bit_count, its set rule against the reference's sequential loop, and its answers on the planted cases against what they were planted
to give: the fp32 edges of the ratio test, the tie rules, rows < 2, the clamping of counts.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import hamming_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loop_knn2(q, t):
    """Every distance by int.bit_count, the two smallest (d, j) by sorting tuples."""
    out = np.full((len(q), 4), -1, np.int32)
    for i in range(len(q)):
        a = int.from_bytes(q[i].tobytes(), "little")
        ds = sorted(((a ^ int.from_bytes(t[j].tobytes(), "little")).bit_count(), j) for j in range(len(t)))
        for k, (d, j) in enumerate(ds[:2]):
            out[i, 2 * k], out[i, 2 * k + 1] = j, d
    return out


SMALL = {k: v for k, v in hr.shape_cases().items() if len(v[0]) * len(v[1]) <= 129 * 257}


@pytest.mark.parametrize("name", list(SMALL) + list(hr.planted_cases()))
def test_knn2_equals_the_bit_count_loop(name):
    q, t = {**SMALL, **hr.planted_cases()}[name]
    assert np.array_equal(hr.knn2(q, t), loop_knn2(q, t))


@pytest.mark.parametrize("name", list(hr.shape_cases()) + list(hr.planted_cases()))
def test_set_rule_equals_the_sequential_loop(name):
    q, t = {**hr.shape_cases(), **hr.planted_cases()}[name]
    a, na = hr.match_pair(q, t)
    b, nb = hr.match_pair_loop(q, t)
    assert np.array_equal(a, b) and na == nb == (a >= 0).sum()
    got = a[a >= 0]
    assert len(set(got.tolist())) == len(got)


def test_a_good_fraction_passes_and_queries_contest_train_rows():
    q, t = hr.shape_cases()["shape_300_515"]
    k = hr.knn2(q, t)
    ok = hr.ratio_pass(k[:, 1], k[:, 3])
    out, n = hr.match_pair(q, t)
    assert ok.sum() > 60 and n > 50
    # contested train rows exist somewhere in the cases (the uniqueness rule is exercised)
    t, q = hr.planted_pair(np.random.default_rng(3), 40, 200, share=1.0, max_flips=4)       # 200 queries, each planted near one of 40 train rows
    k = hr.knn2(q, t)
    ok = hr.ratio_pass(k[:, 1], k[:, 3])
    out, n = hr.match_pair(q, t)
    assert n < ok.sum()
    for j in set(k[ok, 0].tolist()):
        assert out[np.nonzero(ok & (k[:, 0] == j))[0][0]] == j


def test_fp32_edges():
    for d0, d1 in hr.EDGES:
        assert not hr.ratio_pass(d0, d1)
        assert np.float32(0.7) * np.float32(d1) == np.float32(d0)         # 0.7f d1 lies below d0 and rounds up to it: in fp32 the product IS d0
        q, t = hr.planted_cases()["edge_%d_%d" % (d0, d1)]
        assert hr.knn2(q, t).tolist() == [[4, d0, 1, d1]] and hr.match_pair(q, t)[1] == 0
    q, t = hr.planted_cases()["edge_6_10"]
    assert hr.ratio_pass(6, 10) and hr.match_pair(q, t)[0].tolist() == [4]
    assert not hr.ratio_pass(0, 0) and not hr.ratio_pass(5, 5) and hr.ratio_pass(0, 1)


def test_tie_rules_and_planted_answers():
    c = hr.planted_cases()
    q, t = c["twins"]
    k = hr.knn2(q, t)
    assert k[2].tolist() == [9, 3, 31, 3] and hr.match_pair(q, t)[0][2] == -1
    q, t = c["exact"]
    k = hr.knn2(q, t)
    assert k[1, :2].tolist() == [5, 0] and k[1, 3] > 0 and k[2].tolist() == [11, 0, 12, 0]
    out, _ = hr.match_pair(q, t)
    assert out[1] == 5 and out[2] == -1
    q, t = c["extremes"]
    assert hr.knn2(q, t).tolist() == [[1, 0, 0, 256], [0, 0, 2, 0]]
    assert hr.match_pair(q, t)[0].tolist() == [1, -1]
    q, t = c["extremes_only"]
    assert hr.knn2(q, t).tolist() == [[0, 256, 1, 256]] * 2
    q, t = hr.far_rows_case()
    k = hr.knn2(q, t)
    assert k[0].tolist() == [3, 5, 4099, 5] and k[1, :2].tolist() == [4099, 3]


def test_fewer_than_two_train_rows_and_empty_queries():
    rng = np.random.default_rng(1)
    q = hr.random_rows(rng, 3)
    assert hr.match_pair(q, q[:1])[0].tolist() == [-1, -1, -1] and hr.knn2(q, q[:1]).tolist() == [[0, 0, -1, -1], [0, hr.distances(q[1:2], q[:1])[0, 0], -1, -1],
                                                                                                   [0, hr.distances(q[2:3], q[:1])[0, 0], -1, -1]]
    assert hr.match_pair(q, q[:0])[0].tolist() == [-1, -1, -1] and (hr.knn2(q, q[:0]) == -1).all()
    assert hr.match_pair(q[:0], q)[0].shape == (0,) and hr.match_pair_loop(q[:0], q)[1] == 0


def test_counts_are_clamped_and_rows_past_them_never_take_part():
    K = 40
    assert [hr.rows_of(c, K) for c in (-1, 0, 1, K - 1, K, K + 7)] == [0, 0, 1, K - 1, K, K]
    by, counts = hr.counts_case(K)
    images = {i: (by[i], counts[i]) for i in range(6)}
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    table, n = hr.match_grid(images, pairs, stride=K)
    assert n.sum() > 40
    for p, (a, b) in enumerate(pairs):
        ra, rb = hr.rows_of(counts[a], K), hr.rows_of(counts[b], K)
        assert (table[p, ra:] == -1).all() and table[p].max() < max(rb, 1)
        if rb < 2 or ra == 0:
            assert n[p] == 0
    # with the garbage taking part the answer would differ: the check has power
    other, _ = hr.match_grid({i: (by[i], None) for i in range(6)}, pairs, stride=K)
    assert not np.array_equal(other, table)


def test_golden_file_is_what_the_reference_gives():
    spec = importlib.util.spec_from_file_location("make_hamming_golden", os.path.join(ROOT, "tests", "golden", "make_hamming_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = mod.arrays()
    with np.load(mod.PATH) as got:
        assert sorted(got.files) == sorted(want)
        for k, v in want.items():
            assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
