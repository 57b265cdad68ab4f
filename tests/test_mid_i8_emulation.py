"""CPU suite: the integer threshold of the middle tier's int8 sweep (csrc/match.hip mid_thr_acc, csrc/mid_i8.h k_mid_eval_i8),
emulated in numpy on top of tests/int8_emu.py.

A row that leaves the re-rank undecided carries eb, the larger of its two coarse candidates' exact distances, and the sweep keeps
the train rows whose INTEGER accumulator is at most
    thr_acc = floor(accof(eb (1 + slack) + slack (|q|^2 + Nmax^2)) + E(q)) + 1,      accof(d2) = BIAS + (s^2 / 2)(d2 - |q|^2).
For every such row of every set below:
  * the kept rows contain every train row whose canonical fp64 distance is <= eb (so the exact two nearest neighbours are among them),
  * they contain both coarse candidates (so every row has at least two),
  * the (value, index)-ordered top-2 of the kept rows, through the ratio test, is the oracle's decision,
and on the benchmark's data no row keeps more than RCN_MIDCAP = 32 rows (a longer list overflows to the brute-force kernel: right,
but slow)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_emu as emu  # noqa: E402
from oracle import orc  # noqa: E402
from reconstructor_amd import synth  # noqa: E402

MIDCAP = 32
REL_SLACK = 1e-9          # ScaleDev::rel_slack, as int8_emu.decide_pair has it


def fast_accumulators(qq, tq, hn):
    """emu.accumulators through the fp64 BLAS: products of at most 127^2 summed 256 times stay far below 2^53, so the result is exact"""
    return hn[None, :] - np.rint(qq.astype(np.float64) @ tq.astype(np.float64).T).astype(np.int64)


def exact_d2(q, t):
    """row pairs, ascending k like the canonical chain (tests/test_int8_emulation.py)"""
    d = q.astype(np.float64) - t.astype(np.float64)
    acc = np.zeros(d.shape[0])
    for k in range(d.shape[1]):
        acc += d[:, k] * d[:, k]
    return acc


def exact_row_d2(qrow, t):
    """one query row against every train row, the same chain"""
    d = qrow.astype(np.float64)[None, :] - t.astype(np.float64)
    acc = np.zeros(t.shape[0])
    for k in range(t.shape[1]):
        acc += d[:, k] * d[:, k]
    return acc


def thr_acc_of(eb, nq2, E, S):
    d2 = eb * (1.0 + REL_SLACK) + REL_SLACK * (nq2 + S["n_max"] ** 2)
    return np.floor(S["bias"] + 0.5 * S["s"] ** 2 * (d2 - nq2) + E) + 1.0


def check_set(images, pairs, monkeypatch, cap=None):
    """returns the list sizes of the rows past the re-rank that carry an integer threshold"""
    monkeypatch.setattr(emu, "accumulators", fast_accumulators)
    S = emu.fix_scale(images)
    assert S is not None
    quant = [emu.quantise(im, S["s"]) for im in images]
    hns = [emu.half_norms(im, S) for im in images]
    rho = max(float(r.max()) for _, r, _ in quant if r.size) * (1 + 1e-6) + 1e-6
    tau = max(float(n.max()) for _, _, n in quant if n.size) * (1 + 1e-6)
    sizes = []
    for i, j in pairs:
        q, t = images[i], images[j]
        if q.shape[0] == 0 or t.shape[0] <= 2:
            continue                                              # (fewer than three train rows: no integer threshold, the fp32 sweep)
        res, tier = emu.decide_pair(q, t, S, rho, tau, exact_d2)
        rows = np.nonzero(tier == 2)[0]
        if rows.size == 0:
            continue
        qq, rq, nq = quant[i]
        acc = fast_accumulators(qq[rows], quant[j][0], hns[j])
        keys = emu.keys_top2(acc)
        i0, i1 = (keys[:, 0] & 0xFFF).astype(np.int64), (keys[:, 1] & 0xFFF).astype(np.int64)
        nq2 = (q[rows].astype(np.float64) ** 2).sum(1)
        E = (nq[rows] * rho + rq[rows] * (tau + rho)) * (1.0 + 1e-9) + 0.5 + 1.0e-3
        eb = np.maximum(exact_d2(q[rows], t[i0]), exact_d2(q[rows], t[i1]))
        thr = thr_acc_of(eb, nq2, E, S)
        assert (thr < emu.PAD_ACC).all() and np.isfinite(eb).all()
        idx, d2o = orc.knn2(q[rows], t)
        want = np.where(emu.ratio_pass(d2o[:, 0], d2o[:, 1]), idx[:, 0], -1)
        for n, r in enumerate(rows):
            kept = np.nonzero(acc[n] <= thr[n])[0]
            d2 = exact_row_d2(q[r], t)
            inside = np.nonzero(d2 <= eb[n])[0]
            assert np.isin(inside, kept).all(), (i, j, int(r), "a row within eb is not under the integer threshold")
            assert i0[n] in kept and i1[n] in kept, (i, j, int(r), "a coarse candidate is not under its own threshold")
            order = np.lexsort((kept, d2[kept]))                   # by (value, index)
            b0, b1 = kept[order[0]], kept[order[1]]
            got = b0 if emu.ratio_pass(d2[b0], d2[b1]) else -1
            assert got == want[n], (i, j, int(r), int(got), int(want[n]))
            sizes.append(kept.size)
    if cap is not None:
        assert max(sizes, default=0) <= cap, ("a list longer than RCN_MIDCAP", max(sizes))
    return sizes


def test_bench_data_keeps_short_lists(monkeypatch):
    """the benchmark's generator, K = 4096, 7 images, all 21 pairs: a superset of the rows within eb, never more than RCN_MIDCAP of them"""
    K = 4096
    pool = synth.world_pool("superpoint", 4 * K, seed=1234)
    ims = [synth.image_descriptors("superpoint", i, K, pool, seed=1234) for i in range(7)]
    pairs = [(i, j) for i in range(7) for j in range(i + 1, 7)]
    sizes = check_set(ims, pairs, monkeypatch, cap=MIDCAP)
    print("bench data: %d rows past the re-rank, %d-%d rows under the threshold, mean %.2f" % (len(sizes), min(sizes), max(sizes), float(np.mean(sizes))))
    assert len(sizes) > 0


def test_near_duplicates(monkeypatch):
    """sixteen train rows within the error band of each other (tests/test_int8_emulation.py): every one of them is kept"""
    rng = np.random.default_rng(8)
    base = rng.standard_normal((40, 256)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    t = np.repeat(base, 16, axis=0) + (rng.standard_normal((640, 256)) * 1e-5).astype(np.float32)
    q = base + (rng.standard_normal((40, 256)) * 1e-5).astype(np.float32)
    sizes = check_set([q, t], [(0, 1)], monkeypatch)
    assert len(sizes) > 0 and min(sizes) >= 2


def test_integer_rows_with_exact_ties(monkeypatch):
    """exact duplicates among the train rows (tests/test_int8_emulation.py): a tie at eb is inside the threshold, and the index decides"""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, (600, 256)).astype(np.float32)
    t[300:330] = t[:30]
    q = t[rng.permutation(600)[:400]].copy()
    q[::3, :8] += 1.0
    sizes = check_set([q, t], [(0, 1), (1, 0), (1, 1)], monkeypatch)
    assert len(sizes) > 0 and min(sizes) >= 2
