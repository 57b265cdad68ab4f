"""CPU suite: the int8 coarse pass, emulated in numpy with exact integer accumulators (tests/int8_emu.py restates fix_scale, the
quantisation, the key and the two certificates of k_filter / certify), against the oracle's exact 2-NN.

A CERTIFIED decision must equal the oracle's -- on the benchmark's data and on every kind of data the device must refuse (it keeps
the fp16 pass: asserted) or survive if it did not (the same emulation with the refusal overridden: still no wrong decision, because
the certificates price every row's residual exactly; the refusal is about speed).  On the benchmark's data the share of rows that
need the exact tiers is bounded: at most 2 % to the re-rank, at most 0.2 % past it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_emu as emu  # noqa: E402
from oracle import orc  # noqa: E402
from reconstructor_amd import synth  # noqa: E402


def truth_of(q, t):
    """the oracle's decision per query row before uniqueness: nearest neighbour if the ratio test passes, else -1"""
    if q.shape[0] == 0 or t.shape[0] < 2:
        return np.full(q.shape[0], -1, np.int64)
    idx, d2 = orc.knn2(q, t)
    return np.where(emu.ratio_pass(d2[:, 0], d2[:, 1]), idx[:, 0], -1).astype(np.int64)


def exact_d2(q, t):
    """squared distances of row pairs in fp64, ascending k like the canonical chain (whose fma rounds once per term where this rounds
    twice: a last-bit difference that no integer-valued or tied case has, and that the certificates' slack covers elsewhere)"""
    d = q.astype(np.float64) - t.astype(np.float64)
    acc = np.zeros(d.shape[0])
    for k in range(d.shape[1]):
        acc += d[:, k] * d[:, k]
    return acc


def run_set(images, pairs, force=False):
    """emulate the resident set; returns (scale record or None, rows, rows to the re-rank, rows past it, wrong certified decisions)"""
    S = emu.fix_scale(images, force=force)
    if S is None:
        return None, 0, 0, 0, 0
    quant = [emu.quantise(im, S["s"]) for im in images]
    rho = max((float(r.max()) for _, r, _ in quant if r.size), default=0.0) * (1 + 1e-6) + 1e-6
    tau = max((float(n.max()) for _, _, n in quant if n.size), default=0.0) * (1 + 1e-6)
    assert rho <= emu.RES_MAX and tau <= S["M"]
    rows = k2 = past = wrong = 0
    for i, j in pairs:
        q, t = images[i], images[j]
        res, tier = emu.decide_pair(q, t, S, rho, tau, exact_d2)
        want = truth_of(q, t)
        dec = res != -2
        wrong += int((res[dec] != want[dec]).sum())
        rows += q.shape[0]
        k2 += int((tier >= 1).sum())
        past += int((tier == 2).sum())
    return S, rows, k2, past, wrong


def test_bench_data_certifies_and_stays_under_the_caps():
    K = 4096
    pool = synth.world_pool("superpoint", 4 * K, seed=1234)
    ims = [synth.image_descriptors("superpoint", i, K, pool, seed=1234) for i in range(3)]
    S, rows, k2, past, wrong = run_set(ims, [(0, 1), (0, 2), (2, 1)])
    assert S is not None and 4.0 < S["peak"] < emu.PEAK_MAX, S      # (three images: their maximum is 4.9 rms; a thousand images reach 6)
    print("bench data: peak %.2f, s Nmax %.1f, %d rows, %.3f %% to the re-rank, %.4f %% past it" % (S["peak"], S["s"] * S["n_max"], rows, 100.0 * k2 / rows, 100.0 * past / rows))
    assert wrong == 0
    assert k2 <= 0.02 * rows, (k2, rows)
    assert past <= 0.002 * rows, (past, rows)


def heavy_tailed(rng, K):
    x = rng.standard_t(2.5, (K, 256)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def one_huge(rng, K):
    x = rng.standard_normal((K, 256)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[K // 3, 17] = 40.0
    return x


@pytest.mark.parametrize("kind", ["heavy_tailed", "one_huge"])
def test_peaked_data_is_refused_and_would_still_be_right(kind):
    rng = np.random.default_rng(21)
    gen = {"heavy_tailed": heavy_tailed, "one_huge": one_huge}[kind]
    ims = [gen(rng, 700), gen(rng, 640)]
    ims[1][:200] = ims[0][:200] + (rng.standard_normal((200, 256)) * 0.02).astype(np.float32)      # true matches among the rows
    assert emu.fix_scale(ims) is None, "the device must keep the fp16 pass on %s rows" % kind
    S, rows, k2, past, wrong = run_set(ims, [(0, 1), (1, 0)], force=True)
    assert S is not None and S["peak"] >= emu.PEAK_MAX
    assert wrong == 0 and rows == 1340


def test_integer_rows_with_exact_ties():
    """small integers: the scale cap applies (s Nmax = 711.5, not 127 / max |x|), every residual is tiny but not zero (s is no
    integer), and exact ties between train rows must never be decided by the coarse pair"""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 4, (600, 256)).astype(np.float32)
    t[300:330] = t[:30]                                            # exact duplicates: ties for the nearest neighbour
    q = t[rng.permutation(600)[:400]].copy()
    q[::3, :8] += 1.0
    S, rows, k2, past, wrong = run_set([q, t], [(0, 1), (1, 0), (1, 1)])
    assert S is not None and abs(S["s"] * S["n_max"] - (emu.M_MAX - 8.5)) < 1e-9, S
    assert wrong == 0 and rows == 1600


def test_rows_at_the_maximum_fill_the_key_without_overflow():
    """rows whose elements all equal the maximum: the largest accumulators the scale rule admits (decide_pair asserts the range)"""
    x = np.full((64, 256), 0.37, np.float32)
    x[1::2] *= -1.0
    x[2::4, :3] = 0.0
    S, rows, k2, past, wrong = run_set([x, x[:50].copy()], [(0, 1), (1, 0), (0, 0)])
    assert S is not None and S["M"] <= emu.M_MAX + 1e-9
    assert 2 * S["M"] ** 2 + emu.RES_MAX * S["M"] + 4 < emu.PAD_ACC
    assert wrong == 0


def test_near_duplicates_go_to_the_exact_tiers():
    """the set of test_match_gpu.py::test_adversarial_near_duplicates: sixteen train rows within the error band of each other"""
    rng = np.random.default_rng(8)
    base = rng.standard_normal((40, 256)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    t = np.repeat(base, 16, axis=0) + (rng.standard_normal((640, 256)) * 1e-5).astype(np.float32)
    q = base + (rng.standard_normal((40, 256)) * 1e-5).astype(np.float32)
    S, rows, k2, past, wrong = run_set([q, t], [(0, 1)])
    assert S is not None and wrong == 0
    assert k2 == 40                                                 # no row is decided by the coarse pair


@pytest.mark.parametrize("K", [0, 1, 2, 63, 513])
def test_small_and_empty_images_and_zero_rows(K):
    rng = np.random.default_rng(100 + K)
    a = synth.descriptor_set("superpoint", 2, [max(K, 1), 300], n_world=700, seed=9)
    q = a[0][:K].copy()
    t = a[1].copy()
    t[5] = 0.0
    if K > 3:
        q[3] = 0.0
    q2 = rng.standard_normal((K, 256)).astype(np.float32) * 0.05
    S, rows, k2, past, wrong = run_set([q, t, q2], [(0, 1), (1, 0), (2, 0), (0, 2), (2, 2)])
    assert S is not None and wrong == 0
