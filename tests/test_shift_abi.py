"""ilqr_shift_horizon without a GPU: the symbols are exported, declared and mirrored, the refusals that need no handle hold, the
numpy yardstick (tests/shift_ref.py) slices as the header says on hand-made arrays, and the inputs of the GPU test
(tests/test_gpu_shift.py) have the properties that test relies on — on the oracle alone: the two readings of the closed-loop head
agree, every start stays finite, and ten times the rounding spread of the head under a 1e-15 move of x1 stays below the parity
bound 1e-10."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import policy_ref as P
import shift_ref as R
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ["ilqr_shift_horizon", "ilqr_shift_horizon_device"]
# the instances the GPU parity test looks at (B = 70: both waves, the ragged one included; synth12: B = 2) and its steps
INSTANCES = {"acrobot": (0, 63, 64, 69), "car_obs": (0, 63, 64, 69), "synth12": (0, 1)}
STEPS = (1, 3)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), FNS[0]), "the library has no %s: nothing here has a subject" % FNS[0]
    return p


def test_symbols_are_exported_declared_and_mirrored(pkg):
    raw = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = pkg._ffi.lib()
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        res, args = pkg._ffi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 6 and args[1] is C.c_int32 and args[2] is C.c_int32 and args[3] is C.c_int32
    assert re.search(r"#define\s+ILQR_SHIFT_TAIL_HOLD\s+0\b", hdr) and re.search(r"#define\s+ILQR_SHIFT_TAIL_ZERO\s+1\b", hdr)
    assert callable(pkg.Solver.shift_horizon_) and callable(pkg.Solver.shift_horizon_device_)
    assert pkg.Solver._TAILS == {"hold": 0, "zero": 1}
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    assert "function shift_horizon!(" in jl and ":ilqr_shift_horizon, LIB[]" in jl and "shift_horizon!," in jl.split("const LIB")[0]
    assert os.path.exists(os.path.join(ROOT, "examples", "mpc_shift.c"))
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    assert '#include "ilqr_device_shift.hpp"' in dev and "launch_shift" in dev
    assert int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 14


@pytest.mark.parametrize("fn", FNS)
def test_argument_refusals_need_no_device(pkg, fn):
    """Negative steps, an unknown tail, w_tail with steps == 0 and a null handle are refused before the handle is looked at (so: on a
    machine with no device, where no handle can exist), each with the function's name in the message. The refusals that need a
    handle — steps > T−1, w_tail on a model without parameters, a lowered handle, feedback without a policy, the device form on a
    sharded handle — are in the GPU file."""
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(pkg._ffi.c_double_p) if fn == FNS[0] else C.c_void_p(buf.ctypes.data)
    for steps, tail, feedback, x1, w_tail, msg in [(-1, 0, 0, None, None, b"steps must lie in 0 .. T-1"), (-7, 1, 1, p, p, b"steps must lie in 0 .. T-1"),
                                                   (1, 2, 0, None, None, b"unknown tail"), (1, -1, 0, p, None, b"unknown tail"),
                                                   (0, 0, 0, None, p, b"w_tail given with steps == 0"), (0, 1, 1, p, p, b"w_tail given with steps == 0"),
                                                   (0, 0, 0, None, None, b"null handle"), (1, 0, 0, None, None, b"null handle"),
                                                   (3, 1, 1, p, p, b"null handle")]:
        assert f(None, steps, tail, feedback, x1, w_tail) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_shifted_inputs_on_hand_made_arrays():
    T, n, m, nw = 6, 2, 2, 3
    N = T - 1
    xb = np.arange(T * n, dtype=np.float64).reshape(T, n) + 100.0
    ub = np.arange(N * m, dtype=np.float64).reshape(N, m) + 1.0
    w = np.arange(T * nw, dtype=np.float64).reshape(T, nw) + 1000.0
    # k = 0: everything stays, whatever the tail
    for tail in ("hold", "zero"):
        x1p, up, wp = R.shifted_inputs(xb, ub, w, 0, tail)
        assert np.array_equal(x1p, xb[0]) and np.array_equal(up, ub) and np.array_equal(wp, w)
    # k = 1
    x1p, up, wp = R.shifted_inputs(xb, ub, w, 1, "hold")
    assert np.array_equal(x1p, xb[1]) and np.array_equal(up[:N - 1], ub[1:]) and np.array_equal(up[N - 1], ub[N - 1])
    assert np.array_equal(wp[:T - 1], w[1:]) and np.array_equal(wp[T - 1], w[T - 1])        # the terminal row is what is held
    x1p, up, wp = R.shifted_inputs(xb, ub, w, 1, "zero", x1=[7.0, 8.0], w_tail=[[1.0, 2.0, 3.0]])
    assert np.array_equal(x1p, [7.0, 8.0]) and np.array_equal(up[:N - 1], ub[1:]) and np.array_equal(up[N - 1], [0.0, 0.0])
    assert not np.signbit(up[N - 1]).any()
    assert np.array_equal(wp[:T - 1], w[1:]) and np.array_equal(wp[T - 1], [1.0, 2.0, 3.0])
    # k = 3 with a tail of three rows: they enter in order, behind the old terminal row
    wt = -np.arange(3 * nw, dtype=np.float64).reshape(3, nw)
    x1p, up, wp = R.shifted_inputs(xb, ub, w, 3, "hold", w_tail=wt)
    assert np.array_equal(up, np.stack([ub[3], ub[4], ub[4], ub[4], ub[4]]))
    assert np.array_equal(wp, np.concatenate([w[3:], wt])) and np.array_equal(wp[T - 4], w[T - 1])
    # k = T − 1: nothing of ū but its last row survives, the state is the old terminal state
    x1p, up, wp = R.shifted_inputs(xb, ub, w, T - 1, "hold")
    assert np.array_equal(x1p, xb[T - 1]) and np.array_equal(up, np.tile(ub[N - 1], (N, 1))) and np.array_equal(wp, np.tile(w[T - 1], (T, 1)))
    x1p, up, wp = R.shifted_inputs(xb, ub, None, T - 1, "zero")
    assert wp is None and np.array_equal(up, np.zeros((N, m)))
    # the inputs are not written to
    assert xb[0, 0] == 100.0 and ub[0, 0] == 1.0 and w[0, 0] == 1000.0
    assert np.array_equal(R.time_varying(np.zeros((2, 4, 3)))[1, :, 2], [0.0, 0.01, 0.02, 0.03])


def _oracle_case(pkg, oracle, name):
    """the workload of the GPU test solved on the oracle, instance by instance: (model, T, size, [(b, xb, ub, K, w)])"""
    cfg, T, size = P.CASES[name]
    out = []
    opts = oracle.default_options(**pkg.workloads.CONFIG_OPTIONS.get(cfg, {}))
    for b in INSTANCES[name]:
        model, T_, x1, ub = pkg.workloads.make_inputs(cfg, 1, offset=b)
        assert T_ == T
        w = R.time_varying(pkg.workloads.make_parameters(cfg, 1, offset=b)) if name == "car_obs" else None
        ref = oracle.solve_batch(model, T, x1, ub, options=opts, w=w)
        out.append((b, ref["x"][0], ref["u"][0], ref["K"][0], None if w is None else w[0]))
    return model, T, size, out


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_the_gpu_tests_inputs_on_the_oracle(pkg, oracle, name):
    """Per instance and per k of the GPU parity test, with its starts x1 = x̄_k + size · N(0, 1): the oracle's rollout! driven
    off-nominal on the slices and the plain loop agree to 1e-12 and stay finite; ten times the head's rounding spread stays below
    1e-10, the forward-stage bound of tests/test_gpu_parity.py and of the policy tests. The figure goes into the GPU file's docstring."""
    model, T, size, insts = _oracle_case(pkg, oracle, name)
    worst = 0.0
    for b, xb, ub, K, w in insts:
        for k in STEPS:
            _, _, wp = R.shifted_inputs(xb, ub, w, k)
            x1 = R.measured_start(xb[k], size, b, k)
            a = R.feedback_head(oracle, model, T, xb, ub, K, wp, k, x1)
            c = R.feedback_head_numpy(oracle, model, T, xb, ub, K, wp, k, x1)
            assert a["first_nonfinite"] == -1 and c["first_nonfinite"] == -1, (b, k)
            assert a["x"].shape == (T - k, xb.shape[1]) and a["u"].shape == (T - k - 1, ub.shape[1])
            assert np.array_equal(a["x"][0], x1)
            assert P.rel(c["x"], a["x"]) < 1e-12 and P.rel(c["u"], a["u"]) < 1e-12, (b, k, P.rel(c["x"], a["x"]), P.rel(c["u"], a["u"]))
            assert np.abs(a["u"] - ub[k:]).max() > 1e-6                   # the feedback does something at this perturbation
            worst = max(worst, R.head_spread(oracle, model, T, xb, ub, K, wp, k, [x1]))
    print("shift head spread %s: %.2e" % (name, worst))
    assert 10.0 * worst < 1e-10, worst
