"""The LAPACK boundary of the reference — LAPACK.potrf!('U', ·) / LAPACK.potrs!('U', ·, ·) at
src/backward_pass.jl:69-73 — held against the REAL LAPACK (scipy.linalg.lapack.dpotrf / dpotrs, OpenBLAS).

Stated bars, on 1 000 random SPD matrices per size (condition number ≤ ~1e3):
    potrf  m ∈ {1, 2}  (acrobot: nu = 1, car: nu = 2 — the BASELINE headline configs)   bitwise
           m ∈ {5, 8}  OpenBLAS accumulates its dot products in SIMD/FMA order            ≤ 5e-12 · max|U|
    potrs  m = 1       (OpenBLAS's trsm multiplies by the inverted diagonal; so does the oracle)   bitwise
           m ∈ {2, 5, 8}  on LAPACK's own factor                                           ≤ 1e-13 · max|X|
and the reference's behaviour on a matrix that is NOT positive definite (return code ignored, src/backward_pass.jl:69): potrs
then solves with the half-factored matrix dpotf2 leaves behind, and THAT solution is the K and k the recursion goes on with. The
same three bars hold there, for m ∈ {1, 2, 3, 4, 5, 8, 16} and every failing pivot j = 1..m, on 100 `_spd` matrices per (m, j)
whose diagonal entry j is replaced by a value in [-6, -5] (the bad pivot the solves divide by twice stays of order 1):
    potrf  info equal; upper triangle bitwise for m ≤ 2, otherwise ≤ 5e-12 · max|U|   observed: 0 for j ≤ 2 (any m), 1.2e-15 at worst (m = 16, j = 14)
    potrs  on LAPACK's own half-factored matrix  ≤ 1e-13 · max|X|                      observed: 7.5e-16 at worst (m = 16)
    factor + solve, end to end                   ≤ 1e-10 · max|X|                      observed: 1.2e-14 at worst (m = 16, j = 16)
with max|X| between 0.1 and 9: the generator needed no change. A NaN pivot is where the diagnostics part: OpenBLAS's dpotrf
returns info = 0 (its test is `ajj <= 0`, false for NaN; netlib's dpotf2 adds disnan and returns j) while the oracle and the
device report info = j; the solution is NaN in every entry on both sides.
"""
import numpy as np
import pytest
from scipy.linalg import lapack


def _spd(rng, m):
    A = rng.standard_normal((m, m + 3))
    return A @ A.T + 0.1 * np.eye(m)


def _orc(oracle, S, Bm):
    L = oracle.lib()
    m = S.shape[0]
    a = np.asfortranarray(S.copy())
    info = L.orc_potrf_U(a.ctypes.data_as(oracle.c_double_p), m)
    b = np.asfortranarray(Bm.copy())
    L.orc_potrs_U(a.ctypes.data_as(oracle.c_double_p), m, b.ctypes.data_as(oracle.c_double_p), Bm.shape[1])
    return a, b, info


@pytest.mark.parametrize("m", [1, 2, 5, 8])
def test_oracle_potrf_potrs_vs_scipy_lapack(oracle, m):
    rng = np.random.default_rng(100 + m)
    iu = np.triu_indices(m)
    worst_u, worst_x, worst_end = 0.0, 0.0, 0.0
    for _ in range(1000):
        S = _spd(rng, m)
        Bm = rng.standard_normal((m, 4))
        U, info = lapack.dpotrf(np.asfortranarray(S), lower=0, clean=0)
        X, _ = lapack.dpotrs(U, np.asfortranarray(Bm), lower=0)
        a, b, oinfo = _orc(oracle, S, Bm)
        assert info == 0 and oinfo == 0
        if m <= 2:
            assert np.array_equal(U[iu], a[iu])
        worst_u = max(worst_u, np.abs(U[iu] - a[iu]).max() / np.abs(U).max())
        # solve with LAPACK's own factor so that only the triangular solves are compared
        b2 = np.asfortranarray(Bm.copy())
        oracle.lib().orc_potrs_U(np.asfortranarray(U).ctypes.data_as(oracle.c_double_p), m,
                                 b2.ctypes.data_as(oracle.c_double_p), 4)
        if m == 1:
            assert np.array_equal(X, b2) and np.array_equal(X, b)
        worst_x = max(worst_x, np.abs(X - b2).max() / np.abs(X).max())
        worst_end = max(worst_end, np.abs(X - b).max() / np.abs(X).max())       # factor + solve, end to end
    assert worst_u <= 5e-12, worst_u
    assert worst_x <= 1e-13, worst_x
    assert worst_end <= 1e-10, worst_end


def test_failed_factorisation_matches_lapack_info(oracle):
    """Quu not positive definite: LAPACK returns info = j (first bad leading minor) and the reference carries on
    (src/backward_pass.jl:69). The oracle reports the same info and leaves the same leading rows."""
    S = np.array([[4.0, 2.0, 1.0], [2.0, 1.0, 3.0], [1.0, 3.0, 5.0]])        # 2x2 leading minor is singular
    U, info = lapack.dpotrf(np.asfortranarray(S), lower=0, clean=0)
    a, _, oinfo = _orc(oracle, S, np.ones((3, 1)))
    assert info == oinfo == 2
    assert np.array_equal(U[0], a[0])                                          # the completed first row


FAILED = [(m, j) for m in (1, 2, 3, 4, 5, 8, 16) for j in range(1, m + 1)]


@pytest.mark.parametrize("m,j", FAILED, ids=["m%d-pivot%d" % mj for mj in FAILED])
def test_failed_pivot_factor_and_solve_vs_scipy_lapack(oracle, m, j):
    """Pivot j fails (diagonal entry j of order -1): the oracle's half-factored matrix is LAPACK's over the WHOLE upper triangle, its
    potrs on LAPACK's own half-factored matrix is LAPACK's potrs, and so is factor + solve end to end: the K, k of
    src/backward_pass.jl:69-73 after an ignored failure. Bars as on positive definite input (module docstring)."""
    rng = np.random.default_rng(1000 * m + j)
    iu = np.triu_indices(m)
    worst_u, worst_x, worst_end = 0.0, 0.0, 0.0
    for _ in range(100):
        S = _spd(rng, m)
        S[j - 1, j - 1] = -5.0 - rng.random()
        Bm = rng.standard_normal((m, 4))
        U, info = lapack.dpotrf(np.asfortranarray(S), lower=0, clean=0)
        X, _ = lapack.dpotrs(U, np.asfortranarray(Bm), lower=0)
        a, b, oinfo = _orc(oracle, S, Bm)
        assert info == j and oinfo == j
        if m <= 2:
            assert np.array_equal(U[iu], a[iu])
        worst_u = max(worst_u, np.abs(U[iu] - a[iu]).max() / np.abs(U[iu]).max())
        b2 = np.asfortranarray(Bm.copy())                       # LAPACK's own half-factored matrix: only the solves are compared
        oracle.lib().orc_potrs_U(np.asfortranarray(U).ctypes.data_as(oracle.c_double_p), m,
                                 b2.ctypes.data_as(oracle.c_double_p), 4)
        worst_x = max(worst_x, np.abs(X - b2).max() / np.abs(X).max())
        worst_end = max(worst_end, np.abs(X - b).max() / np.abs(X).max())
    print("m=%d j=%d: potrf %.2e  potrs %.2e  end to end %.2e" % (m, j, worst_u, worst_x, worst_end))
    assert worst_u <= 5e-12, worst_u
    assert worst_x <= 1e-13, worst_x
    assert worst_end <= 1e-10, worst_end


NAN = [(m, j) for m in (1, 2, 4) for j in range(1, m + 1)]


@pytest.mark.parametrize("m,j", NAN, ids=["m%d-pivot%d" % mj for mj in NAN])
def test_nan_pivot_gives_an_all_nan_solution_on_both_sides(oracle, m, j):
    """A NaN on diagonal entry j: every entry of the solution is NaN, with LAPACK and with the oracle. What LAPACK's info says
    depends on its build (OpenBLAS: 0; netlib: j) and is not asserted; the oracle's, like the device's, is j."""
    rng = np.random.default_rng(7000 + 10 * m + j)
    S = _spd(rng, m)
    S[j - 1, j - 1] = np.nan
    Bm = rng.standard_normal((m, 4))
    U, info = lapack.dpotrf(np.asfortranarray(S), lower=0, clean=0)
    X, _ = lapack.dpotrs(U, np.asfortranarray(Bm), lower=0)
    _, b, oinfo = _orc(oracle, S, Bm)
    print("m=%d j=%d: LAPACK info %d, oracle info %d" % (m, j, info, oinfo))
    assert oinfo == j
    assert np.isnan(X).all() and np.isnan(b).all()
