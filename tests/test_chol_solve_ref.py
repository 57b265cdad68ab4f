"""tests/chol_ref.py judges the dense Cholesky on the GPU (tests/test_chol_solve_gpu.py); this is what judges chol_ref.py, without a GPU:
the matrices have the properties they claim, the refined solution is far better than LAPACK's own, the numpy models of the
right-hand-side row and of a broken pivot do what the GPU test relies on, and the tool's files round-trip bit for bit."""
import numpy as np
import pytest
import scipy.linalg as sla

import chol_ref as R


@pytest.mark.parametrize("n,kappa", [(2, 1e1), (100, 1e2), (300, 1e4), (300, 1e8), (257, 1e10)])
def test_spd_spectrum_has_the_condition_number_it_claims(n, kappa):
    S = R.spd_spectrum(n, kappa, seed=n)
    assert np.array_equal(S, S.T)
    # (the eigenvalues of a symmetric matrix move by at most |E|_2 ~ n u under rounding: relative to the smallest one, n u kappa)
    assert abs(np.linalg.cond(S) / kappa - 1.0) <= 1e-12 + 16 * n * R.U * kappa
    assert np.count_nonzero(S) == n * n or n < 3


def families():
    yield "spectrum 1e2", R.spd_spectrum(300, 1e2, 1)
    yield "spectrum 1e8", R.spd_spectrum(300, 1e8, 2)
    yield "spectrum 1e10", R.spd_spectrum(300, 1e10, 3)
    yield "wishart", R.spd_wishart(257, 4)
    yield "graded wishart", R.graded(R.spd_wishart(300, 5), 1e-6, 1e6)
    yield "wishart 1e12", R.spd_wishart(129, 6) * 1e12
    yield "wishart 1e-12", R.spd_wishart(129, 7) * 1e-12


def test_refinement_beats_lapack_by_three_orders_on_every_family():
    for name, S in families():
        b = R.rhs(S.shape[0], 11)
        x_lap, x_ref = R.ref_solve(S, b)
        r_lap = np.abs(R.residual_ld(S, b, x_lap)).max()
        r_ref = np.abs(R.residual_ld(S, b, x_ref)).max()
        assert r_ref * 1e3 <= r_lap, (name, float(r_ref), float(r_lap))
        assert R.fwd(x_ref, x_ref) == 0.0 and R.fwd(x_lap, x_ref) < 1e-6, name
        assert R.bwd(S, b, x_lap) <= S.shape[0] * R.U, name


def test_measures_see_a_wrong_entry():
    S = R.spd_wishart(100, 8)
    b = R.rhs(100, 8)
    x_lap, x_ref = R.ref_solve(S, b)
    x = x_lap.copy()
    x[37] *= 1.0 + 1e-9
    assert R.fwd(x, x_ref) > 1e3 * R.fwd(x_lap, x_ref) and R.bwd(S, b, x) > 1e3 * R.bwd(S, b, x_lap)


@pytest.mark.parametrize("n", [1, 17, 127, 300])
def test_padded_model_row_is_the_forward_substitution(n):
    S = R.spd_wishart(n, 20 + n)
    b = R.rhs(n, n)
    y = R.padded_model(S, b)
    want = sla.solve_triangular(np.linalg.cholesky(S), b, lower=True)
    assert np.abs(y - want).max() <= 8 * n * R.U * np.abs(want).max()


def chol_columns(A):
    """plain column Cholesky; stops at the first pivot that is not positive: (index of that pivot or n, the columns before it)"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return j, L
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return n, L


@pytest.mark.parametrize("i", [0, 15, 16, 127, 128, 299])
def test_break_pivot_breaks_exactly_pivot_i(i):
    S = R.spd_wishart(300, 31)
    B = R.break_pivot(S, i)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(B)
    assert np.array_equal(B - np.diag(np.diag(B)), S - np.diag(np.diag(S))) and np.flatnonzero(np.diag(B) != np.diag(S)).tolist() == [i]
    # the same column algorithm on both: it stops at pivot i of B, and everything before is bit-equal to the unbroken factor
    stop_s, Ls = chol_columns(S)
    stop_b, Lb = chol_columns(B)
    assert stop_s == 300 and stop_b == i
    assert Lb[:, :i].tobytes() == Ls[:, :i].tobytes()
    assert np.array_equal(np.linalg.cholesky(B[:i, :i]), np.linalg.cholesky(S[:i, :i])) or i == 0
    assert B[i, i] - Ls[i, :i] @ Ls[i, :i] < 0.0


def test_file_round_trip_is_bit_exact(tmp_path):
    d = str(tmp_path)
    S = R.graded(R.spd_wishart(33, 9), 1e-6, 1e6)
    S[3, 4] = np.nan
    b = R.rhs(33, 9) * 1e-300
    R.write_system(d, "sys", S, b)
    S2, b2 = R.read_system(d, "sys", 33)
    assert S.tobytes() == S2.tobytes() and b.tobytes() == b2.tobytes()
    cases = [R.Case("a", "sys", 33, "fused"), R.Case("b", "sys", 33, "plain", safe=1, trsv_chain=0, dump=1, prm=(2, 4, 1, 2, 2, 0, 0))]
    R.write_cases(d, cases)
    assert R.read_cases(d) == cases
    # what the tool writes for a case, read back
    x = R.rhs(33, 10)
    x.astype("<f8").tofile(str(tmp_path / "b.x"))
    L = np.arange(128.0 * 128).reshape(128, 128)
    for k in ("L", "Sf", "Linv"):
        (L + len(k)).astype("<f8").tofile(str(tmp_path / ("b." + k)))
    (tmp_path / "b.out").write_text("1 1 0 0.125000\n")
    r = R.read_result(d, cases[1])
    assert (r["flag"], r["nblk"], r["schedule"], r["wall_ms"]) == (1, 1, 0, 0.125)
    assert r["x"].tobytes() == x.tobytes() and np.array_equal(r["Linv"][0], L + 4) and np.array_equal(r["Sf"], L + 2)


def test_assemble_factor_inverts_what_the_kernel_stores():
    S = R.spd_wishart(200, 12)
    Lc = np.linalg.cholesky(S)
    Lp = np.eye(256)
    Lp[:200, :200] = Lc
    Linv = np.stack([np.linalg.inv(Lp[k * 128:(k + 1) * 128, k * 128:(k + 1) * 128]) for k in range(2)])
    F, tiles = R.assemble_factor(dict(nblk=2, L=np.tril(Lp, -1), Linv=Linv), 200)
    assert np.abs(F - Lc).max() <= 1e-12 and len(tiles) == 2


def test_every_gpu_parameter_set_is_executed_in_numpy_too():
    import test_chol_plan as P
    assert R.GPU_PLAN_CASES == P.GPU_SOLVE_CASES and all(len(prm) == 13 for _, prm in P.GPU_SOLVE_CASES)
    assert all(c in P.CASES for c in P.GPU_SOLVE_CASES)      # list order and the static check; any order: the test over GPU_SOLVE_CASES
    assert R.plan_array(R.SHIP) == P.SHIPPING
