"""CPU suite: the stress sets of tests/coarse_stress.py do what they claim.  The GPU test and tools/mfma_error_stress.py run the
hardware on these sets; every check here is a condition on the INPUTS, so that the hardware cannot pass vacuously: the aligned set
does reach the bound in emulation, the accumulation-only operands are exact, the misranked queries are misranked, the band rows
sit in the band."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import coarse_stress as cs  # noqa: E402
from oracle import orc  # noqa: E402


def _pairs(g):
    return [(g["images"][a], g["images"][b], inf) for (a, b), inf in zip(g["pairs"], g["info"])]


def _shapes_ok(g):
    for q, t, _ in _pairs(g):
        assert 1 <= len(q) <= 128 and 3 <= len(t) <= 256 and q.dtype == np.float32 and t.dtype == np.float32


def test_eps_is_the_formula_of_the_emulation_test():
    """One Python copy of the bound, not two: coarse_stress.eps equals tests/test_error_bound.py::_emulate's, term for term."""
    import test_error_bound as teb
    from reconstructor_amd import synth
    for kind, D in (("orb", 32), ("sift", 128), ("superpoint", 256)):
        ims = synth.descriptor_set(kind, 2, 70, n_world=150, seed=2)
        acc0, exact0, eps0, s0, bias0 = teb._emulate(ims[0], ims[1])
        mdl = cs.model(ims)
        acc, exact = cs.emulate(ims[0], ims[1], mdl)
        assert mdl["s"] == s0 and mdl["bias"] == bias0 and mdl["DP"] == D
        assert np.array_equal(acc, acc0) and np.array_equal(exact, exact0)
        assert np.allclose(cs.eps(mdl, cs.qnorm(ims[0])), eps0, rtol=1e-14, atol=0)
        assert (cs.eps_acc(mdl, cs.qnorm(ims[0])) < 0.2 * eps0).all()


@pytest.mark.parametrize("D", cs.DIMS)
def test_aligned_set_reaches_the_bound_in_emulation(D):
    g = cs.aligned(D)
    _shapes_ok(g)
    peak = 0.0
    for q, t, inf in _pairs(g):
        mdl = cs.model([q, t], D)
        assert mdl == cs.model(g["images"], D)                 # every pair alone has the scale of the whole set
        assert mdl["DP"] == cs.padded(D)
        acc, exact = cs.emulate(q, t, mdl)
        r = (acc - exact) / cs.eps(mdl, cs.qnorm(q))[:, None]
        assert np.abs(r).max() <= 1.0, (D, np.abs(r).max())
        rows = np.arange(len(q))
        sign = 1.0 if inf["type"] == "down" else -1.0          # down-type: both operands lose u, the product is too small, acc too large
        tw = sign * r[rows, inf["twin"]]
        assert tw[inf["full_norm"]].min() >= 0.85, (D, inf["type"], tw[inf["full_norm"]].min())
        assert (tw > 0.25).all()                                # the short queries err the same way, against a bound the half-norm dominates
        assert (sign * r[rows, inf["mirror"]] < -0.25).all()    # the mirror: the other end
        assert (acc[rows, inf["twin"]] == acc.min(1)).all() and (acc[rows, inf["mirror"]] == acc.max(1)).all()
        nq = cs.qnorm(q) / mdl["nmax"]
        assert all(np.isclose(nq, v, rtol=0.05).any() for v in (1.0, 0.25, 1.0 / 64))
        peak = max(peak, float(np.abs(r).max()))
    assert 0.85 <= peak <= 1.0


@pytest.mark.parametrize("D", cs.DIMS)
def test_a_truncating_conversion_exceeds_the_bound(D):
    """Control (CPU emulation only): the instrument sees a conversion fault."""
    g = cs.truncation_control(D)
    q, t, inf = _pairs(g)[0]
    mdl = cs.model([q, t], D)
    e = cs.eps(mdl, cs.qnorm(q))[:, None]
    acc, exact = cs.emulate(q, t, mdl)
    assert (np.abs(acc - exact) / e).max() < 0.01               # round-to-nearest: these magnitudes are 2^-20 from an fp16 number
    acc, exact = cs.emulate(q, t, mdl, convert=cs.trunc_f16)
    assert ((np.abs(acc - exact) / e)[np.arange(len(q)), inf["twin"]] > 1.5).all()


@pytest.mark.parametrize("D", cs.DIMS)
def test_accumulation_only_operands_are_exact(D):
    g = cs.accumulation_only(D)
    _shapes_ok(g)
    for q, t, _ in _pairs(g):
        mdl = cs.model([q, t], D)
        for x in (q, t):
            sx = mdl["s"] * x.astype(np.float64)
            assert np.array_equal(cs.rne_f16(sx).astype(np.float64), sx)                   # operand error exactly zero
            bits = cs.rne_f16(sx).view(np.uint16)
            assert (bits & 1).all() and ((bits >> 10) & 31).min() >= 1                      # all 11 significand bits in use, no subnormal
        acc, exact = cs.emulate(q, t, mdl)
        ea = cs.eps_acc(mdl, cs.qnorm(q))
        assert (np.abs(acc - exact) <= ea[:, None]).all()
        assert (ea < 0.2 * cs.eps(mdl, cs.qnorm(q))).all()      # the part is small next to the whole: judging against eps would hide it
        # a query and its two partners share signs
        assert (np.sign(t[0:2 * len(q):2]) == np.sign(q)).all() and (np.sign(t[1:2 * len(q):2]) == np.sign(q)).all()


def _exact_top2(q, t):
    """Independent of the oracle: float64 distances in numpy, ties by index."""
    d = ((q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]) ** 2).sum(2)
    idx = np.argsort(d, axis=1, kind="stable")[:, :2]
    return idx, np.take_along_axis(d, idx, 1)


def _exact_table(q, t):
    idx, dd = _exact_top2(q, t)
    return np.where(cs.ratio_pass(dd[:, 0], dd[:, 1]), idx[:, 0], -1)


@pytest.mark.parametrize("D,peaked", [(D, False) for D in cs.DIMS] + [(256, True)])
def test_misranked_set_misranks(D, peaked):
    g = cs.misranked(D, peaked)
    _shapes_ok(g)
    mdl = cs.model(g["images"], D)
    n_mis, sides, wrong_small = 0, [0, 0], 0
    for q, t, inf in _pairs(g):
        if not peaked:
            assert cs.model([q, t], D) == mdl
        acc, exact = cs.emulate(q, t, mdl)
        c0, c1, mask = cs.coarse_top2(acc, len(t))
        idx, dd = orc.knn2(q, t)
        idx2, dd2 = _exact_top2(q, t)
        assert np.array_equal(idx, idx2) and np.allclose(dd, dd2, rtol=1e-12, atol=0)      # the oracle's decision, reproduced
        assert np.array_equal(idx[:, 0], inf["T1"]) and np.array_equal((c0 & mask).astype(np.int64), inf["T1"])
        mis = (c1 & mask).astype(np.int64) != idx[:, 1]
        assert np.array_equal(idx[mis, 1], inf["T3"][mis]) and np.array_equal((c1 & mask).astype(np.int64)[mis], inf["T2"][mis])
        passes = cs.ratio_pass(dd[:, 0], dd[:, 1])
        n_mis += int(mis.sum())
        sides[0] += int((mis & passes).sum())
        sides[1] += int((mis & ~passes).sum())
        assert np.array_equal(np.where(passes, idx[:, 0], -1), _exact_table(q, t))
        assert np.array_equal(orc.match_pair(q, t)[0], _exact_table(q, t))      # (no two queries of a pair share a nearest row)
        # the ratio sits within the bound of the line: |d0^2 - 0.49 d1^2| <= 1.3 E for every query
        E = 2.0 * cs.eps(mdl, cs.qnorm(q)) / mdl["s"] ** 2
        assert (np.abs(dd[:, 0] - 0.49 * dd[:, 1]) <= 1.3 * E).all()
        # with eps the certificates are right wherever they decide; with a quarter of it some misranked row is certified wrongly
        full = cs.pipeline_decisions(q, t, mdl, 1.0)
        assert ((full == -2) | (full == _exact_table(q, t))).all()
        small = cs.pipeline_decisions(q, t, mdl, 0.25)
        wrong_small += int(((small != -2) & (small != _exact_table(q, t))).sum())
    assert n_mis >= 8 and min(sides) >= 1, (D, n_mis, sides)
    assert wrong_small >= 1, "a bound four times too small would not show in this set's table"


@pytest.mark.parametrize("D,peaked", [(D, False) for D in cs.DIMS] + [(256, True)])
def test_band_rows_are_undecided_with_eps_and_decided_with_half(D, peaked):
    g = cs.band(D, peaked)
    _shapes_ok(g)
    mdl = cs.model(g["images"], D)
    rows, sides = 0, [0, 0]
    for q, t, _ in _pairs(g):
        assert not cs.band_status(q, t, mdl, 1.0).any()
        assert cs.band_status(q, t, mdl, 0.5).all()
        idx, dd = orc.knn2(q, t)
        idx2, dd2 = _exact_top2(q, t)
        assert np.array_equal(idx, idx2) and np.allclose(dd, dd2, rtol=1e-12, atol=0)
        table = _exact_table(q, t)
        assert np.array_equal(orc.match_pair(q, t)[0], table)
        rows += len(q)
        sides[0] += int((table >= 0).sum())
        sides[1] += int((table < 0).sum())
    assert rows >= 32 and min(sides) >= 8, (D, rows, sides)
    if peaked:
        assert max(float(np.abs(im).max()) for im in g["images"]) * 16.0 / mdl["nmax"] >= 8.0       # fix_scale's peak test refuses int8


def test_err_bound_d2_is_eps_at_the_largest_norm():
    mdl = cs.model(cs.aligned(64)["images"], 64)
    assert cs.err_bound_d2(mdl) == 2.0 * float(cs.eps(mdl, mdl["nmax"])) / mdl["s"] ** 2
    assert 2.0 ** -10 * 2 * mdl["nmax"] ** 2 < cs.err_bound_d2(mdl) < 1.1 * 2.0 ** -10 * 2 * mdl["nmax"] ** 2
