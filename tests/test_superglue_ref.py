"""CPU suite of SuperGlue's optimal-matching layer: the float64 reference tests/sg_ref.py against the
fp32 torch transcription of the published forward (this MEASURES dev32, the figure the GPU test's tolerance is four times
of), its marginals, the implicit-dustbin form against the bordered matrix, the lowest-index tie rule, the cap on undecided
rows of the shared cases, and the golden file."""
import functools
import os

import numpy as np
import pytest

import sg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV32 = 2.55e-5            # max |logP_fp32 - logP_f64| over CASES as measured by test_fp32_transcription_deviation (printed there)
TOL = 4 * DEV32            # what the GPU test allows (reduction order, 1-2 ulp expf / logf against libm's < 1)
CASES = sg_ref.SHAPES + [(272, 272)]


@functools.lru_cache(maxsize=None)
def case(m, n):
    d0, d1, target = sg_ref.planted_case(m, n, sg_ref.case_seed(m, n))
    S = sg_ref.scores(d0, d1).astype(np.float32)
    logP, u, v = sg_ref.assign(S)
    for a in (S, logP, u, v, target):
        a.setflags(write=False)
    return S, logP, u, v, target


def row_residual(S, u, v, alpha=1.0):
    """u - u_next: what one more row update would change (the convergence of the iteration on this case)."""
    m, n = S.shape
    log_mu = sg_ref.marginals(m, n)[1]
    Z = np.full((m + 1, n + 1), alpha)
    Z[:m, :n] = S
    return u - (log_mu - sg_ref._lse(Z + v[None, :], 1))


def test_fp32_transcription_deviation():
    worst = 0.0
    for m, n in CASES:
        S, logP = case(m, n)[:2]
        dev = float(np.abs(sg_ref.assign_torch32(S.copy()).astype(np.float64) - logP).max())
        print("dev32 (%4d, %4d) = %.3g   scores in [%.1f, %.1f]" % (m, n, dev, S.min(), S.max()))
        worst = max(worst, dev)
    print("dev32 = %.3g (constant in the tests: %.3g)" % (worst, DEV32))
    # the constant is a measurement; another libm or vector width may move it a little, not by a factor
    assert DEV32 / 2 <= worst <= DEV32 * 2


@pytest.mark.parametrize("m,n", CASES)
def test_marginals(m, n):
    S, logP, u, v, _ = case(m, n)
    norm, log_mu, log_nu = sg_ref.marginals(m, n)
    P = np.exp(logP + norm)
    assert np.abs(P.sum(0) / np.exp(log_nu) - 1).max() <= 1e-12          # v was updated last: columns are exact
    # rows: off by exactly what the next u update would change, sum_j P[i][j] = mu[i] exp(u[i] - u_next[i])
    res = row_residual(S, u, v)
    assert np.abs(P.sum(1) / np.exp(log_mu) - np.exp(res)).max() <= 1e-12
    print("(%d, %d): max |u_next - u| after 100 iterations = %.3g" % (m, n, np.abs(res).max()))


@pytest.mark.parametrize("m,n", [(1, 1), (7, 3), (33, 47), (200, 257)])
def test_implicit_dustbin_equals_bordered(m, n):
    S, logP = case(m, n)[:2]
    assert np.abs(sg_ref.assign_bordered(S) - logP).max() <= 1e-12


def tie_case():
    """(33, 47) with row c2 of d1 a copy of the planted row c1 < c2: columns c1 and c2 of S are identical."""
    d0, d1, target = sg_ref.planted_case(33, 47, 7)
    d1 = d1.copy()
    i = 3
    c1 = int(target[i])
    c2 = c1 + 5 if c1 + 5 < 47 and (c1 + 5) not in target else [c for c in range(c1 + 1, 47) if c not in target][0]
    d1[c2] = d1[c1]
    return d0, d1, i, c1, c2


def test_tie_goes_to_the_lowest_index():
    d0, d1, i, c1, c2 = tie_case()
    S = sg_ref.scores(d0, d1).astype(np.float32)
    assert np.array_equal(S[:, c1], S[:, c2])
    logP = sg_ref.assign(S)[0]
    assert np.array_equal(logP[:, c1], logP[:, c2])
    sel = sg_ref.select(logP)
    assert sel["matches0"][i] == c1 and sel["matches1"][c1] == i and sel["matches1"][c2] == -1 and sel["mscores1"][c2] == 0
    assert 0.2 + TOL < sel["mscores0"][i] < 0.5 + 0.01          # the row's mass is split between the two columns


def test_cases_stay_inside_the_undecided_cap():
    for m, n in CASES:
        S, logP, _, _, target = case(m, n)
        rows, cols = sg_ref.undecided(logP, TOL)
        assert rows.sum() <= 0.02 * m and cols.sum() <= 0.02 * n, (m, n, rows.sum(), cols.sum())
        sel = sg_ref.select(logP)
        planted = target >= 0
        assert ((sel["table"] == target) & planted & ~rows).sum() >= 0.5 * planted.sum(), (m, n)


def test_golden_file():
    g = np.load(os.path.join(ROOT, "tests", "golden", "superglue_small.npz"))
    for m, n in [tuple(s) for s in g["shapes"]]:
        S, logP = case(m, n)[:2]
        assert np.array_equal(g["S_%d_%d" % (m, n)], S), "the case generator moved"
        assert np.abs(g["logP_%d_%d" % (m, n)] - logP).max() <= 1e-12
        sel = sg_ref.select(logP)
        assert np.array_equal(g["table_%d_%d" % (m, n)], sel["table"])
