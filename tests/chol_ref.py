"""What the tests of the dense Cholesky as a unit (csrc/chol.hip behind chol.h, driven by tools/chol_solve_check) are judged against:
test matrices with known properties, a reference solution in extended precision, the error measures, numpy models of the
right-hand-side row and of a broken pivot, the case lists, and the reader / writer of the tool's files.  numpy and scipy only.

The reference: LAPACK's Cholesky (scipy cho_factor) gives x_lap, four steps of iterative refinement with the residual and the iterate in
np.longdouble (x87 extended, 64-bit significand: x86-64 is assumed) give x_ref.  With kappa u << 1 every step gains a factor ~ kappa u,
so x_ref is accurate to a few long-double ulps of the exact solution of the float64 system: it judges LAPACK and the GPU alike.

Parameter sets are seven values in the order of tools/chol_solve_check's case lines: (tl_g, tl_min, pair, pair_min, pipe_min,
head_small, fuse_tail); plan_array() turns one into the thirteen of rcn_ba_factor_plan."""
import collections
import os

import numpy as np
import scipy.linalg as sla

U = 2.0 ** -53          # unit roundoff of float64
BETA = 1.0e200          # RCN_RHS_BETA of csrc/chol.h
BLOCK = 128
LD = np.longdouble

SHIP = (4, 40, 1, 24, 32, 1, 1)      # the defaults of chol::Params (tests/test_chol_plan.py checks that NULL means exactly these)
# nblk -> n of the regime cases, shipping parameters: the smallest sizes at which each path of the plan appears
REGIMES = [(1, 100), (2, 200), (3, 300), (6, 700), (27, 3400), (34, 4300), (48, 6100)]
# the same kernels at the smallest shapes, thresholds shrunk: (nblk, parameters)
SHRUNK = [
    (7, (0, 40, 1, 2, 2, 1, 1)),        # TRSM_PIPE; bulk updates of one panel and of two
    (12, (2, 4, 1, 2, 2, 1, 1)),        # 8 two-level steps of g = 2, both inverse buffers, 3 fused tails
    (16, (4, 4, 1, 2, 2, 1, 1)),        # rolled K = 512 update, g = 4 inverse, fused tail
    (12, (2, 4, 1, 2, 2, 0, 0)),        # ... the pipelined forms of the head product, the product as a launch of its own
    (16, (4, 4, 1, 2, 2, 0, 0)),
]


def plan_array(prm):
    tl_g, tl_min, pair, pair_min, pipe_min, head_small, fuse_tail = prm
    return (tl_g, tl_min, pair, pair_min, pipe_min, 0, fuse_tail, head_small, 0, 0, 0, 0, 0)


# every (nblk, thirteen values) the GPU test runs: tests/test_chol_plan.py executes each of them in numpy
GPU_PLAN_CASES = [(nblk, plan_array(SHIP)) for nblk, _ in REGIMES] + [(nblk, plan_array(p)) for nblk, p in SHRUNK]


# ---------------------------------------------------------------------------------------------------------------------
# matrices
def _reflect(A, v):
    """H A H with H = I - 2 v v' (|v| = 1), in O(n^2)"""
    Av = A @ v
    A = A - 2.0 * np.outer(v, Av) - 2.0 * np.outer(Av, v) + (4.0 * (v @ Av)) * np.outer(v, v)
    return A


def spd_spectrum(n, kappa, seed):
    """H2 H1 diag(lambda) H1 H2, lambda log-spaced in [1 / kappa, 1] and shuffled: dense, and its 2-norm condition number is kappa"""
    rng = np.random.default_rng(seed)
    lam = np.logspace(-np.log10(kappa), 0.0, n) if n > 1 else np.ones(1)
    rng.shuffle(lam)
    A = np.diag(lam)
    for _ in range(2):
        v = rng.standard_normal(n)
        A = _reflect(A, v / np.linalg.norm(v))
    return 0.5 * (A + A.T)


def spd_wishart(n, seed):
    assert n <= 2048
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    return G @ G.T / n + 0.1 * np.eye(n)


def graded(S, lo, hi):
    """D S D, D log-spaced from lo to hi: columns that differ by many orders of magnitude (camera blocks with Jacobi scaling off)"""
    d = np.logspace(np.log10(lo), np.log10(hi), S.shape[0])
    return S * d[:, None] * d[None, :]


def rhs(n, seed):
    return np.random.default_rng(seed + 7919).standard_normal(n)


# ---------------------------------------------------------------------------------------------------------------------
# reference and measures
def _matvec_ld(S, x):
    """S x with the products and sums in long double, 256 rows at a time (a long-double copy of a 6144 x 6144 S would be 600 MB).
    Each row is summed PAIRWISE (numpy's sum along the contiguous axis), not left to right as the long-double `@` does: the rounding
    of the partial sums then costs O(log n) ulps instead of O(n), which at n = 300 is the difference between a residual that shows
    the rounding of x to long double and one that shows its own evaluation (measured: ten times larger)."""
    x = np.asarray(x, dtype=LD)
    out = np.empty(S.shape[0], dtype=LD)
    for r in range(0, S.shape[0], 256):
        out[r:r + 256] = (S[r:r + 256].astype(LD) * x[None, :]).sum(axis=1)
    return out


def residual_ld(S, b, x):
    return np.asarray(b, dtype=LD) - _matvec_ld(S, x)


def ref_solve(S, b, steps=4):
    """(x_lap: LAPACK's solution in float64, x_ref: the same after `steps` of refinement in long double)"""
    assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the x87 extended format"
    cf = sla.cho_factor(S, lower=True)
    x_lap = sla.cho_solve(cf, b)
    x = x_lap.astype(LD)
    for _ in range(steps):
        r = residual_ld(S, b, x)
        x = x + sla.cho_solve(cf, r.astype(np.float64)).astype(LD)
    return x_lap, x


def norm_inf_ld(S):
    return np.abs(S).sum(axis=1, dtype=LD).max()


def fwd(x, x_ref):
    x = np.asarray(x, dtype=LD)
    return float(np.abs(x - x_ref).max() / np.abs(x_ref).max())


def bwd(S, b, x, s_norm=None):
    s_norm = norm_inf_ld(S) if s_norm is None else s_norm
    x = np.asarray(x, dtype=LD)
    return float(np.abs(residual_ld(S, b, x)).max() / (s_norm * np.abs(x).max() + np.abs(np.asarray(b, dtype=LD)).max()))


# ---------------------------------------------------------------------------------------------------------------------
# models
def padded_model(S, b, beta=BETA):
    """The right-hand side as row n of the system: the factor of [[S, b], [b', beta]] has L^-1 b in row n.  Returns that row."""
    n = S.shape[0]
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = S
    A[n, :n] = b
    A[:n, n] = b
    A[n, n] = beta
    return np.linalg.cholesky(A)[n, :n].copy()


def break_pivot(S, i):
    """S with S[i, i] lowered by twice the i-th squared pivot of its factor: steps 0 .. i - 1 of a factorisation are unchanged, pivot i
    comes out as minus what it was"""
    L = np.linalg.cholesky(S)
    B = S.copy()
    B[i, i] -= 2.0 * L[i, i] ** 2
    return B


# ---------------------------------------------------------------------------------------------------------------------
# the tool's files
Case = collections.namedtuple("Case", "name system n mode safe trsv_chain dump prm", defaults=(0, 1, 0, SHIP))


def write_system(d, system, S, b):
    n = S.shape[0]
    assert S.shape == (n, n) and b.shape == (n,)
    np.ascontiguousarray(S, dtype="<f8").tofile(os.path.join(d, system + ".S"))
    np.ascontiguousarray(b, dtype="<f8").tofile(os.path.join(d, system + ".b"))


def read_system(d, system, n):
    S = np.fromfile(os.path.join(d, system + ".S"), dtype="<f8")
    b = np.fromfile(os.path.join(d, system + ".b"), dtype="<f8")
    assert S.size == n * n and b.size == n
    return S.reshape(n, n), b


def write_cases(d, cases):
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("# name system n mode safe trsv_chain dump tl_g tl_min pair pair_min pipe_min head_small fuse_tail\n")
        for c in cases:
            assert c.mode in ("plain", "row", "fused") and len(c.prm) == 7 and (c.mode == "plain" or c.n % BLOCK != 0)
            f.write(" ".join(str(v) for v in (c.name, c.system, c.n, c.mode, int(c.safe), int(c.trsv_chain), int(c.dump)) + tuple(c.prm)) + "\n")


def read_cases(d):
    out = []
    with open(os.path.join(d, "cases.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            w = line.split()
            out.append(Case(w[0], w[1], int(w[2]), w[3], int(w[4]), int(w[5]), int(w[6]), tuple(int(v) for v in w[7:14])))
    return out


def read_result(d, case):
    """what the tool left for a case: x, flag, nblk, schedule, wall_ms and, if the case asked for them, L, Sf, Linv"""
    with open(os.path.join(d, case.name + ".out")) as f:
        w = f.read().split()
    r = dict(flag=int(w[0]), nblk=int(w[1]), schedule=int(w[2]), wall_ms=float(w[3]))
    r["x"] = np.fromfile(os.path.join(d, case.name + ".x"), dtype="<f8")
    assert r["x"].size == case.n
    if case.dump:
        npad = r["nblk"] * BLOCK
        for k, shape in (("L", (npad, npad)), ("Sf", (npad, npad)), ("Linv", (r["nblk"], BLOCK, BLOCK))):
            r[k] = np.fromfile(os.path.join(d, case.name + "." + k), dtype="<f8").reshape(shape)
    return r


def assemble_factor(res, n):
    """F (n x n) from the tool's buffers: sub-diagonal tiles from L, diagonal tile k as the triangular inverse of Linv[k]; the tile
    factors themselves come back too"""
    nblk = res["nblk"]
    F = np.zeros((nblk * BLOCK, nblk * BLOCK))
    tiles = []
    for k in range(nblk):
        r = slice(k * BLOCK, (k + 1) * BLOCK)
        Fkk = sla.solve_triangular(np.tril(res["Linv"][k]), np.eye(BLOCK), lower=True)
        tiles.append(np.tril(Fkk))
        F[r, r] = tiles[-1]
        F[(k + 1) * BLOCK:, r] = res["L"][(k + 1) * BLOCK:, r]
    return F[:n, :n], tiles
