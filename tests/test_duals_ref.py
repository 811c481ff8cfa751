"""tests/duals_ref.py without a GPU. (1) The loop composed from the oracle's exported steps, started from the cold values λ = 0,
ρ = ρ0, reproduces oracle.Solver.solve() exactly: the yardstick of ilqr_solve_warm is tied to the oracle. (2) The inputs the GPU
tests use (duals_ref.small_case) make a warm start worth having, on the oracle alone. (3) The numpy shift does what its formulas
say. (4) The new entry points are exported, declared, bound, and refuse what needs no handle.

The inputs picked: car_obs (5 stage rows, 4 terminal rows, T = 51) under workloads.make_parameters, instances 0..4 of
workloads.make_inputs (pcg64, the default seed), default options. The oracle's cold first solve takes 2, 2, 2, 2, 6 outer
iterations; after a one-step shift of trajectory, parameters and duals (hold, keep) the cold re-solve takes 2, 2, 2, 2, 6 again and
the warm one 1 on every instance."""
import os
import re

import numpy as np
import pytest

import duals_ref as D
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ["ilqr_shift_duals", "ilqr_shift_duals_device", "ilqr_solve_warm"]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_composed_loop_from_cold_values_is_the_oracles_solve(pkg, oracle):
    c = D.small_case(pkg, oracle)
    ref = oracle.solve_batch(c["model"], c["T"], c["x1"], c["ub"], options=c["options"], w=c["w"], nthreads=4)
    got = c["first"]
    for f in ("x", "u", "K", "k"):
        assert np.array_equal(got[f], ref[f]), f
    for f in ref["stats"]:
        assert np.array_equal(got["stats"][f], ref["stats"][f]), (f, got["stats"][f], ref["stats"][f])
    # the duals of the solve, too (solve_batch does not return them): one instance on a Solver of its own
    pr = oracle.Problem(c["model"], c["T"])
    s = oracle.Solver(pr, c["options"], w=c["w"][4])
    s.initialize_controls(c["ub"][4]); s.initialize_states(pr.rollout(c["x1"][4], c["ub"][4], c["w"][4]))
    s.solve()
    assert np.array_equal(s.buffer("constraint_dual"), got["lam"][4]) and np.array_equal(s.buffer("constraint_penalty"), got["rho"][4])
    assert s.stats().outer_iterations == got["stats"]["outer_iterations"][4] > 1


def test_the_inputs_make_a_warm_start_worth_having(pkg, oracle):
    c = D.small_case(pkg, oracle)
    cold, warm, tol = c["cold"]["stats"], c["warm"]["stats"], c["options"].constraint_tolerance
    print("\nouter iterations cold %s warm %s; iterations cold %s warm %s" % (cold["outer_iterations"], warm["outer_iterations"],
                                                                            cold["iterations"], warm["iterations"]))
    assert (warm["outer_iterations"] <= cold["outer_iterations"]).all()
    assert (warm["outer_iterations"] < cold["outer_iterations"]).any()
    assert (cold["max_violation"] <= tol).all() and (warm["max_violation"] <= tol).all()
    # the shifted duals are not trivial: multipliers of active rows, penalties above ρ0
    assert (np.abs(c["lam"]).max(1) > 0).all() and (c["rho"].max(1) > c["options"].initial_constraint_penalty).all()


@pytest.mark.parametrize("ncs,nct,N", [(5, 4, 11), (0, 4, 7), (10, 3, 6), (3, 0, 4)])
def test_numpy_shift_against_the_formulas(ncs, nct, N):
    rng = np.random.default_rng(7)
    Cn = N * ncs + nct
    lam, rho = rng.standard_normal((3, Cn)), 1.0 + rng.uniform(size=(3, Cn))
    for k in (0, 1, 2, N - 1, N):
        for tail in ("hold", "zero"):
            for penalty in ("keep", "reset"):
                l, r = D.shift_duals(lam, rho, ncs, nct, k, tail, penalty, rho0=0.5)
                for b in range(3):
                    for t in range(N):
                        for i in range(ncs):
                            src = t + k if t < N - k else N - 1
                            held = t < N - k or tail == "hold" or k == 0
                            assert l[b, t * ncs + i] == (lam[b, src * ncs + i] if held else 0.0)
                            want = 0.5 if penalty == "reset" else (rho[b, src * ncs + i] if held else 0.5)
                            assert r[b, t * ncs + i] == want
                    assert np.array_equal(l[b, N * ncs:], lam[b, N * ncs:])
                    assert np.array_equal(r[b, N * ncs:], np.full(nct, 0.5) if penalty == "reset" else rho[b, N * ncs:])
    l, r = D.shift_duals(lam, rho, ncs, nct, 0)
    assert np.array_equal(l, lam) and np.array_equal(r, rho)


def test_exported_declared_and_bound(pkg):
    L = pkg._ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    for fn in FNS:
        assert hasattr(L, fn) and fn in pkg._ffi.SYMBOLS and re.search(r"\bint %s\(" % fn, hdr) and ":%s, LIB[]" % fn in jl, fn
    for name, value in (("TAIL_HOLD", 0), ("TAIL_ZERO", 1), ("PENALTY_KEEP", 0), ("PENALTY_RESET", 1)):
        assert re.search(r"#define\s+ILQR_DUALS_%s\s+%d\b" % (name, value), hdr), name
    assert "src/solve.jl:95-103" in hdr and "not a reference behaviour" in hdr
    assert callable(pkg.Solver.shift_duals_) and callable(pkg.Solver.shift_duals_device_) and callable(pkg.Solver.solve_warm_)
    assert '#include "ilqr_device_duals.hpp"' in dev and "launch_shift_duals" in dev and re.search(r"\bint warm_duals;", dev)
    assert int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 16
    # the flag is the solve kernels' and the launcher's: not part of the options struct, which is mirrored in ctypes and Julia
    assert "warm_duals" not in hdr and "warm_duals" not in open(os.path.join(ROOT, "iterativelqr.jl_amd", "_ffi.py")).read()


def test_refusals_that_need_no_handle(pkg):
    L = pkg._ffi.lib()
    for call in (lambda: L.ilqr_shift_duals(None, 1, 0, 0), lambda: L.ilqr_shift_duals_device(None, 1, 0, 0), lambda: L.ilqr_solve_warm(None)):
        assert call() == -1 and b"null handle" in L.ilqr_last_error()
