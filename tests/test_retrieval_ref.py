"""CPU suite of the retrieval ImageMatcher: tests/retr_ref.py (the contract of csrc/retrieval.hip) against independent code where
every sum is exact, the golden file, the structure of the pair lists, and the quality conditions on ring scenes."""
import importlib.util
import os

import numpy as np
import pytest

import retr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "retrieval_small.npz")


def _maker():
    spec = importlib.util.spec_from_file_location("make_retrieval_golden", os.path.join(ROOT, "tests", "golden", "make_retrieval_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _int_scene(n, K, D, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, K, D)).astype(np.float32)


def test_restatement_against_independent_code_on_integer_rows():
    """Integer descriptors 0..255 at D = 32: squared distances, segment sums and the sums over images are integers below 2^53, so
    any summation order gives the same bits.  The independent code uses matrix products and np.add.at."""
    n, K, D, C = 5, 40, 32, 6
    desc = _int_scene(n, K, D, 1)
    desc[2, 7] = desc[2, 3]                                   # repeated rows
    counts = np.array([40, 17, 40, 0, 3], np.int32)
    cents = retr_ref.train(desc, counts, C, 3, 2)
    rows = [(i, r) for i in range(n) for r in range(0, counts[i], 2)]
    M = len(rows)
    x = np.stack([desc[i, r] for i, r in rows]).astype(np.float64)
    mu = np.stack([x[(c * M) // C] for c in range(C)]).astype(np.float32)
    assert np.array_equal(cents[0], mu)
    for step in range(3):
        m64 = mu.astype(np.float64)
        a = retr_ref.assign(x.astype(np.float32), mu)
        if step == 0:                                          # integer centroids: the expanded form and pairwise sums are exact as well
            d2 = (x * x).sum(1)[:, None] - 2.0 * (x @ m64.T) + (m64 * m64).sum(1)[None, :]
            assert np.array_equal(d2.argmin(1), a) and np.array_equal(((x[:, None, :] - m64[None, :, :]) ** 2).sum(2).argmin(1), a)
        S = np.zeros((C, D))
        np.add.at(S, a, x)
        cnt = np.bincount(a, minlength=C)
        new = mu.copy()
        new[cnt > 0] = (S[cnt > 0] / cnt[cnt > 0, None]).astype(np.float32)
        assert np.array_equal(new, cents[step + 1])
        mu = new
    # segment sums and the residual of VLAD are exact too; the norm is not, so G and sim agree to the precision of their formats
    G = retr_ref.encode(desc, counts, mu)
    sim = retr_ref.similarity(G, D)
    Gi = np.zeros_like(G)
    for i in range(n):
        xi = desc[i, :counts[i]].astype(np.float64)
        ai = retr_ref.assign(desc[i, :counts[i]], mu)
        S = np.zeros((C, D))
        np.add.at(S, ai, xi)
        V = S - np.bincount(ai, minlength=C)[:, None] * mu.astype(np.float64)
        Vp = np.sign(V) * np.sqrt(np.abs(V))
        nrm = np.linalg.norm(Vp)
        Gi[i] = (Vp / nrm).reshape(-1) if nrm else 0
    assert np.abs(G - Gi).max() <= 2.0 ** -24 and not G[3].any()        # |G| <= 1: half an ulp of float32 at 1, twice over
    assert np.abs(sim - G.astype(np.float64) @ G.astype(np.float64).T).max() <= C * D * 2.0 ** -52


def test_tie_rules():
    mu = np.array([[0, 0], [2, 0], [2, 0], [0, 2]], np.float32)
    x = np.array([[1, 0], [2, 0], [1, 1], [0, 1], [5, 5]], np.float32)
    assert retr_ref.assign(x, mu).tolist() == [0, 1, 0, 0, 1]
    sim = np.array([[9, 1, 1, 0], [1, 9, 5, 5], [1, 5, 9, 5], [0, 5, 5, 9]], np.float64)
    assert retr_ref.top_k(sim, 2).tolist() == [[1, 2], [2, 3], [1, 3], [1, 2]]
    assert retr_ref.top_k(sim, 9).shape == (4, 3) and retr_ref.top_k(sim[:1, :1], 3).shape == (1, 0)
    # an empty cluster keeps its centroid: rows 0 and 1 are equal, so centroid 1 never wins a row
    desc = np.array([[[1, 1], [1, 1], [4, 4], [9, 9]]], np.float32)
    cents = retr_ref.train(desc, None, 4, 2, 1)
    assert np.array_equal(cents[0], desc[0]) and np.array_equal(cents[2][1], desc[0, 1]) and np.array_equal(cents[2][0], desc[0, 0])
    with pytest.raises(ValueError):
        retr_ref.train(desc, np.array([3], np.int32), 4, 1, 1)
    assert retr_ref.auto_stride(1000, 4096) == 16 and retr_ref.auto_stride(12, 48) == 1
    assert [r.tolist() for r in retr_ref.training_rows(np.array([5, 0, 2], np.int32), 3, 8, 3)] == [[0, 3], [], [0]]


def test_golden_file_reproduces():
    want = _maker().make()
    got = np.load(GOLDEN)
    assert sorted(got.files) == sorted(want)
    for k in want:
        assert got[k].dtype == np.asarray(want[k]).dtype and got[k].tobytes() == np.asarray(want[k]).tobytes(), k
    assert os.path.getsize(GOLDEN) < 400 * 1024


def test_pair_lists_are_ascending_unique_symmetric_and_cover_the_grid():
    from reconstructor_amd.matcher import all_pairs
    g = np.load(GOLDEN)
    n = int(g["params"][0])
    for k in (1, 3, n - 1, n + 5):
        nbr = retr_ref.top_k(g["sim"], k)
        p = retr_ref.pairs(nbr, 7)
        keys = [tuple(q) for q in p.tolist()]
        assert keys == sorted(set(keys)) and (p[:, 0] < p[:, 1]).all() and p.min() >= 7 and p.max() < 7 + n
        partners = {i: set() for i in range(n)}
        for a, b in keys:
            partners[a - 7].add(b - 7)
            partners[b - 7].add(a - 7)
        assert all(set(nbr[i].tolist()) <= partners[i] for i in range(n))           # every neighbour is a partner, both ways round
        if k >= n - 1:
            assert np.array_equal(p - 7, all_pairs(n))
    assert np.array_equal(retr_ref.pairs(retr_ref.top_k(g["sim"], 3), 100), g["pairs"])
    assert retr_ref.pairs(np.zeros((1, 0), np.int32)).shape == (0, 2)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quality_on_ring_scenes(seed):
    n, K, D, step, k = 24, 64, 32, 16, 4
    scene = retr_ref.ring_scene(n, K, D, step, 0.05, seed)
    mu = retr_ref.train(scene, None, 8, 5)[-1]
    sim = retr_ref.similarity(retr_ref.encode(scene, None, mu), D)
    nbr = retr_ref.top_k(sim, k + 1)
    p = {tuple(q) for q in retr_ref.pairs(nbr[:, :k]).tolist()}
    assert all(retr_ref.ring_distance(a, b, n) <= 3 for a, b in p)                   # the two images overlap
    assert all((min(i, (i + 1) % n), max(i, (i + 1) % n)) in p for i in range(n))    # every ring-distance-1 pair
    assert min(sim[i, nbr[i, k - 1]] - sim[i, nbr[i, k]] for i in range(n)) > 1e-4   # rank k against rank k + 1


def test_scene_of_the_package_is_the_scene_of_the_restatement():
    from reconstructor_amd import retrieval
    assert np.array_equal(retrieval.ring_scene(6, 20, 8, 5, 0.05, 3), retr_ref.ring_scene(6, 20, 8, 5, 0.05, 3))


def test_driver_builds_without_gpu():
    """The adapter header and its driver build with plain g++ against include/rcn.h."""
    import __graft_entry__ as g
    g.build_cpp_tests()
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "retrieval_adapter_test"))
