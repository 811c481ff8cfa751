"""ilqr_rollout_policy without a GPU: the symbol is exported, declared and mirrored, the argument refusals that need no handle
hold, and the two readings of the reference the GPU test compares against (tests/policy_ref.py: the oracle's rollout! driven
off-nominal, and a plain loop over the same formula) agree with each other on acrobot and car."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import policy_ref as R
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), "ilqr_rollout_policy"), "the library has no ilqr_rollout_policy: nothing here has a subject"
    return p


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_hip.h")).read(), flags=re.S)
    L = pkg._ffi.lib()
    for name in ("ilqr_rollout_policy", "ilqr_rollout_policy_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        res, args = pkg._ffi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 10 and args[1] is C.c_int32 and args[2] is C.c_double
    assert callable(pkg.Solver.rollout_policy) and callable(pkg.Solver.rollout_policy_device)
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    assert "function rollout_policy(" in jl and ":ilqr_rollout_policy, LIB[]" in jl


@pytest.mark.parametrize("fn", ["ilqr_rollout_policy", "ilqr_rollout_policy_device"])
def test_argument_refusals_need_no_device(pkg, fn):
    """samples < 1, a null x1 and a null cost are refused before the handle is looked at (so: on a machine with no device, where
    no handle can exist); the refusals that need a handle — w on a model without parameters, no policy yet — are in the GPU file."""
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(pkg._ffi.c_double_p) if fn == "ilqr_rollout_policy" else C.c_void_p(buf.ctypes.data)
    for samples, x1, cost, msg in [(0, p, p, b"samples must be >= 1"), (-3, p, p, b"samples must be >= 1"),
                                   (1, None, p, b"null x1"), (1, p, None, b"null cost"), (1, p, p, b"null handle")]:
        assert f(None, samples, 0.0, x1, None, cost, None, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


@pytest.mark.parametrize("name", ["acrobot", "car"])
def test_the_two_readings_of_the_reference_agree(pkg, oracle, name):
    """The oracle's rollout!(1.0) with nominal_states[0] <- x1, k_0 = K_0 (x1 − x̄_1), k_t = 0 against the plain loop
    u_t = ū_t + K_t x_t − K_t x̄_t (α = 0) stepping a T = 2 oracle problem: same states and actions to 1e-12 (they differ in
    the first step only, where the oracle adds K_0 (x1 − x̄_1) + K_0 x1 − K_0 x1 and the loop K_0 x1 − K_0 x̄_1), every sample
    finite. With x1 = x̄_1 and k as solved, the loop equals the oracle's unmodified rollout!(α) bit for bit."""
    cfg, T, size = R.CASES[name]
    B, S = 2, 70
    model, T_, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T_ == T
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=2)
    for b in range(B):
        xb, u, K, k = ref["x"][b], ref["u"][b], ref["K"][b], ref["k"][b]
        x1s = R.perturbed_starts(xb[0], S, size)
        for s in range(S):
            a = R.oracle_reading(oracle, model, T, xb, u, K, x1s[s])
            c = R.numpy_reading(oracle, model, T, xb, u, K, k, x1s[s], 0.0)
            assert a["first_nonfinite"] == -1 and c["first_nonfinite"] == -1, (b, s)
            assert R.rel(c["x"], a["x"]) < 1e-12 and R.rel(c["u"], a["u"]) < 1e-12, (b, s, R.rel(c["x"], a["x"]))
            assert np.isfinite(a["cost"]) and a["max_violation"] >= 0.0
        for alpha in (1.0, 0.5):
            a = R.oracle_rollout_bang(oracle, model, T, xb, u, K, k, alpha)
            c = R.numpy_reading(oracle, model, T, xb, u, K, k, xb[0], alpha)
            assert np.array_equal(a["x"], c["x"]) and np.array_equal(a["u"], c["u"]), (b, alpha)
    # the allowance of the GPU parity test is ten times the oracle's own spread under a 1e-15 move of x1, where that exceeds
    # the forward-stage bound 1e-10: it does not (measured 1.2e-14 acrobot, 5.7e-15 car)
    assert R.spread(oracle, model, T, ref["x"][0], ref["u"][0], ref["K"][0], R.perturbed_starts(ref["x"][0][0], 8, size)) < 1e-11
