"""ilqr_plant_score, ilqr_plant_score_device and ilqr_mpc_run_preview without a GPU: the symbols are exported, declared, mirrored and
in the Julia file; every refusal that needs no handle holds (so: on a machine with no device), each with the function's name in the
message; the Python mirror rejects wrong shapes before any call. The refusals that need a handle are in
tests/test_gpu_mpc_preview.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_FNS = ["ilqr_plant_score", "ilqr_plant_score_device"]
FNS = SCORE_FNS + ["ilqr_mpc_run_preview"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    for fn in FNS:
        assert hasattr(p._ffi.lib(), fn), "the library has no %s: nothing here has a subject" % fn
    return p


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = S.strip_comments(open(os.path.join(ROOT, "include", "ilqr_hip.h")).read())
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert pkg._ffi.SYMBOLS[name][0] is C.c_int
    for name in SCORE_FNS:         # handle, steps, w_plant, x, u, cost, violation
        assert S.H_PROTOS[name][1] == ["ptr:void", "i32"] + ["ptr:f64"] * 5
        assert len(pkg._ffi.SYMBOLS[name][1]) == 7 and pkg._ffi.SYMBOLS[name][1][1] is C.c_int32
    # ilqr_mpc_run's arguments with w_preview behind w_plant and the two scores at the end
    assert S.H_PROTOS["ilqr_mpc_run_preview"][1] == ["ptr:void", "ptr:struct:ilqr_mpc_desc"] + ["ptr:f64"] * 6 + ["ptr:i32"] + ["ptr:f64"] * 2
    assert S.H_PROTOS["ilqr_mpc_run"][1] == ["ptr:void", "ptr:struct:ilqr_mpc_desc"] + ["ptr:f64"] * 5 + ["ptr:i32"]       # unchanged
    assert S.H_DEFINES["ILQR_MPC_LOG_W"] == 9 and C.sizeof(pkg._ffi.MpcDesc) == 56                                        # unchanged
    assert callable(pkg.Solver.plant_score_) and callable(pkg.Solver.plant_score_device_)
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    assert ":ilqr_plant_score, LIB[]" in jl and ":ilqr_plant_score_device, LIB[]" in jl and ":ilqr_mpc_run_preview" in jl
    for fn in ("plant_score!,", "plant_score_device!,", "mpc_run_preview!,"):
        assert fn in jl.split("const LIB")[0], fn
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    assert '#include "ilqr_device_score.hpp"' in dev and "launch_plant_score" in dev
    assert int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 18
    assert os.path.exists(os.path.join(ROOT, "examples", "mpc_tracking.c"))


@pytest.mark.parametrize("fn", SCORE_FNS)
def test_plant_score_refusals_need_no_device(pkg, fn):
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(pkg._ffi.c_double_p) if fn == SCORE_FNS[0] else C.c_void_p(buf.ctypes.data)
    for steps, x, u, cost, msg in [(0, p, p, p, b"steps must lie in 1 .. T-1"), (-2, p, p, p, b"steps must lie in 1 .. T-1"),
                                   (1, None, p, p, b"null x"), (1, p, None, p, b"null u"), (1, p, p, None, b"null cost"),
                                   (1, p, p, p, b"null handle"), (2 ** 20, p, p, p, b"null handle")]:
        assert f(None, steps, None, x, u, cost, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_mpc_run_preview_refusals_need_no_device(pkg):
    L = pkg._ffi.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(pkg._ffi.c_double_p)

    def desc(**kw):
        base = dict(periods=2, steps=1, plant_feedback=0, shift_feedback=0, shift_tail=0, warm=0, duals_tail=0, duals_penalty=0, seed=1,
                    first_instance=0, sigma_x=None)
        base.update(kw)
        return pkg._ffi.MpcDesc(**base)

    for d, cost, viol, msg in [(None, None, None, b"null descriptor"), (desc(periods=0), p, p, b"periods must be >= 1"),
                               (desc(), None, p, b"cl_violation without cl_cost"), (desc(steps=0), p, None, b"steps must lie in 1 .. T-1"),
                               (desc(periods=2 ** 19 + 1, steps=2), None, None, b"beyond 2^20"), (desc(first_instance=-1), p, p, b"first_instance must lie"),
                               (desc(), None, None, b"null handle"), (desc(), p, p, b"null handle")]:
        assert L.ilqr_mpc_run_preview(None, C.byref(d) if d is not None else None, None, None, p, None, None, None, None, cost, viol) == -1
        err = L.ilqr_last_error()
        assert msg in err and b"ilqr_mpc_run_preview" in err, err
    # the old entry point keeps its own name in its messages
    assert L.ilqr_mpc_run(None, C.byref(desc()), None, None, None, None, None, None) == -1
    assert b"ilqr_mpc_run: null handle" in L.ilqr_last_error()


class _Shape:
    """what the shape checks of the Python mirror read of a Solver: no handle, so nothing reaches the library"""
    B, T, nx, nu, num_user_parameter = 3, 11, 3, 2, 2
    _TAILS, _PENALTIES = {"hold": 0, "zero": 1}, {"keep": 0, "reset": 1}


def test_python_mirror_rejects_wrong_shapes(pkg):
    s = _Shape()
    s._plant_arguments = lambda *a: pkg.Solver._plant_arguments(s, *a)
    score, run = pkg.Solver.plant_score_, pkg.Solver.mpc_run_
    x, u = np.zeros((3, 3, 3)), np.zeros((3, 2, 2))
    for bad_x, bad_u, w, msg in [(x, np.zeros((3, 2, 3)), None, r"u must have shape"), (x, np.zeros((2, 2, 2)), None, r"u must have shape"),
                                 (x, np.zeros((3, 2)), None, r"u must have shape"), (np.zeros((3, 2, 3)), u, None, r"x must have shape"),
                                 (np.zeros((3, 3, 2)), u, None, r"x must have shape"), (x, u, np.zeros((3, 3, 2)), r"w_plant must have shape"),
                                 (x, u, np.zeros((3, 2, 1)), r"w_plant must have shape"), (x, np.zeros((3, 11, 2)), None, r"steps must lie in 1 .. T-1")]:
        with pytest.raises(ValueError, match=msg):
            score(s, bad_x, bad_u, w_plant=w)
    for kw, msg in [(dict(w_preview=np.zeros((3, 5, 2))), r"w_preview must have shape \[B, 6,"), (dict(w_preview=np.zeros((3, 6, 1))), r"w_preview must have shape"),
                    (dict(w_preview=np.zeros((6, 3, 2))), r"w_preview must have shape"), (dict(w_plant=np.zeros((3, 5, 2)), score=True), r"w_plant must have shape")]:
        with pytest.raises(ValueError, match=msg):
            run(s, 2, 3, **kw)
