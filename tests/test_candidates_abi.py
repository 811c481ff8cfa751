"""ilqr_initialize_rollout_candidates without a GPU: the symbols are exported, declared and mirrored, the argument refusals that need
no handle hold, the selection rule of the yardstick (tests/candidates_ref.py) does what the header says on hand-made score tables,
and the inputs of the GPU test (tests/test_gpu_candidates.py) have the properties that test relies on — measured on the oracle
alone: the spread of the open-loop recursion under a 1e-15 move of its inputs stays below a tenth of the parity bound, and the
best and second-best eligible scores of every instance lie further apart than four times that bound."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import candidates_ref as R
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ["ilqr_initialize_rollout_candidates", "ilqr_initialize_rollout_candidates_device"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), FNS[0]), "the library has no %s: nothing here has a subject" % FNS[0]
    return p


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_hip.h")).read(), flags=re.S)
    L = pkg._ffi.lib()
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        res, args = pkg._ffi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 9 and args[1] is C.c_int32 and args[2] is C.c_double
    assert callable(pkg.Solver.initialize_rollout_candidates_) and callable(pkg.Solver.initialize_rollout_candidates_device_)
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    assert "function initialize_rollout_candidates!(" in jl and ":ilqr_initialize_rollout_candidates, LIB[]" in jl
    assert os.path.exists(os.path.join(ROOT, "examples", "candidate_init.c"))


@pytest.mark.parametrize("fn", FNS)
def test_argument_refusals_need_no_device(pkg, fn):
    """candidates < 1, a null x1 or u and a negative or non-finite violation_weight are refused before the handle is looked at
    (so: on a machine with no device, where no handle can exist), each with the function's name in the message."""
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(pkg._ffi.c_double_p) if fn == FNS[0] else C.c_void_p(buf.ctypes.data)
    for cand, weight, x1, u, msg in [(0, 0.0, p, p, b"candidates must be >= 1"), (-3, 0.0, p, p, b"candidates must be >= 1"),
                                     (1, 0.0, None, p, b"null x1"), (1, 0.0, p, None, b"null u"),
                                     (1, -1.0, p, p, b"violation_weight"), (1, math.nan, p, p, b"violation_weight"),
                                     (1, math.inf, p, p, b"violation_weight"), (1, 0.0, p, p, b"null handle"), (4, 2.5, p, p, b"null handle")]:
        assert f(None, cand, weight, x1, u, None, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_the_selection_rule_on_hand_made_tables():
    nan, inf = math.nan, math.inf
    ok = [-1] * 4
    assert R.select([3.0, 1.0, 2.0, 1.5], [0.0] * 4, ok) == 1
    assert R.select([2.0, 1.0, 1.0, 1.0], [0.0] * 4, ok) == 1                              # ties: the lowest index
    assert R.select([1.0, 1.0, 1.0, 1.0], [0.0] * 4, ok) == 0
    assert R.select([nan, 5.0, -inf, inf], [0.0] * 4, ok) == 1                             # NaN and ±Inf scores never win
    assert R.select([1.0, 5.0, 2.0, 3.0], [0.0] * 4, [7, -1, 0, -1]) == 3                  # a non-finite state disqualifies
    assert R.select([nan, inf, 1.0, -inf], [0.0] * 4, [-1, -1, 4, -1]) == -1               # nobody eligible
    assert R.select([nan], [0.0], [-1]) == -1 and R.select([0.5], [0.0], [-1]) == 0
    # the weight: 0 ignores the violation altogether (an infinite violation does not disqualify), otherwise cost + weight · violation
    assert R.select([1.0, 2.0], [inf, 0.0], [-1, -1], 0.0) == 0 and R.select([1.0, 2.0], [inf, 0.0], [-1, -1], 1.0) == 1
    assert R.select([1.0, 2.0, 3.0], [0.5, 0.1, 0.0], [-1] * 3, 0.0) == 0
    assert R.select([1.0, 2.0, 3.0], [0.5, 0.1, 0.0], [-1] * 3, 5.0) == 1                  # 3.5, 2.5, 3.0
    assert R.select([1.0, 2.0, 3.0], [0.5, 0.1, 0.0], [-1] * 3, 100.0) == 2
    assert R.select([1.0, 2.0], [nan, 0.0], [-1, -1], 1.0) == 1
    assert R.gap([3.0, 1.0, 2.0], [0.0] * 3, [-1] * 3) == 1.0 and R.gap([1.0, nan], [0.0] * 2, [-1] * 2) == math.inf
    assert R.gap([1.0, 1.0], [0.0] * 2, [-1] * 2) == 0.0


def test_candidate_lists_share_their_prefix():
    ub = np.linspace(-1.0, 1.0, 20).reshape(10, 2)
    a, b = R.candidates(ub, 9, 0.1, b=1), R.candidates(ub, 70, 0.1, b=1)
    assert np.array_equal(a, b[:9]) and np.array_equal(a[0], ub) and not np.array_equal(a[1], R.candidates(ub, 2, 0.1, b=2)[1])


@pytest.mark.parametrize("name", ["acrobot", "car", "car_obs", "particle", "synth12"])
def test_the_gpu_tests_inputs_on_the_oracle(pkg, oracle, name):
    """What tests/test_gpu_candidates.py relies on, from the oracle alone: spread < 1e-10 (a tenth of the parity bound 1e-9), and
    per instance the two best eligible scores further apart than 4e-9 · max(1, |score|), for both weights used there."""
    cfg, T, size = R.CASES[name]
    B, S = (3, 70) if name != "synth12" else (2, 70)
    model, T_, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T_ == T and (T - 1) % 8 != 0
    w = pkg.workloads.make_parameters(cfg, B) if name == "car_obs" else None
    worst = 0.0
    for b in range(B):
        u = R.candidates(ub[b], S, size, b)
        wb = None if w is None else w[b]
        r = R.score_all(oracle, model, T, x1[b], u, wb)
        worst = max(worst, R.spread(oracle, model, T, x1[b], u, wb))
        for weight in (0.0, 1.0e6):
            assert R.select(r["cost"], r["max_violation"], r["first_nonfinite"], weight) >= 0
            assert R.gap(r["cost"], r["max_violation"], r["first_nonfinite"], weight) > 4e-9, (b, weight)
    print("candidate spread %s: %.2e" % (name, worst))
    assert worst < 1e-10, worst
