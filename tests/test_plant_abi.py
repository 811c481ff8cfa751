"""ilqr_plant_step and ilqr_mpc_run without a GPU: the symbols are exported, declared, mirrored and in the Julia file; ilqr_mpc_desc
has the header's size and field offsets in ctypes; every refusal that needs no handle holds (so: on a machine with no device), each
with the function's name in the message. The refusals that need a handle are in tests/test_gpu_mpc_loop.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_FNS = ["ilqr_plant_step", "ilqr_plant_step_device"]
FNS = STEP_FNS + ["ilqr_mpc_run"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), FNS[0]), "the library has no %s: nothing here has a subject" % FNS[0]
    return p


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = S.strip_comments(open(os.path.join(ROOT, "include", "ilqr_hip.h")).read())
    L = pkg._ffi.lib()
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert pkg._ffi.SYMBOLS[name][0] is C.c_int
    for name in STEP_FNS:      # the argument order of the issue: handle, steps, feedback, seed, first_instance, step0, sigma_x, then six arrays
        args = pkg._ffi.SYMBOLS[name][1]
        assert len(args) == 12 and args[1:6] == [C.c_int32, C.c_int32, C.c_uint64, C.c_int64, C.c_int32] and args[6] is pkg._ffi.c_double_p
        assert S.H_PROTOS[name][1][:7] == ["ptr:void", "i32", "i32", "u64", "i64", "i32", "ptr:f64"]
    assert S.H_PROTOS["ilqr_mpc_run"][1] == ["ptr:void", "ptr:struct:ilqr_mpc_desc"] + ["ptr:f64"] * 5 + ["ptr:i32"]
    assert S.H_DEFINES["ILQR_MPC_LOG_W"] == 9 == pkg._ffi.MPC_LOG_W == len(pkg._ffi.MPC_LOG_COLUMNS)
    assert list(pkg._ffi.MPC_LOG_COLUMNS) == [f for f, _ in pkg._ffi.Stats._fields_ if f != "reserved"]
    assert callable(pkg.Solver.plant_step_) and callable(pkg.Solver.plant_step_device_) and callable(pkg.Solver.mpc_run_)
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    assert "function plant_step!(" in jl and ":ilqr_plant_step, LIB[]" in jl and "function mpc_run!(" in jl and ":ilqr_mpc_run" in jl
    assert "plant_step!," in jl.split("const LIB")[0] and "mpc_run!," in jl.split("const LIB")[0]
    assert os.path.exists(os.path.join(ROOT, "examples", "mpc_closed_loop.c"))
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    assert '#include "ilqr_device_plant.hpp"' in dev and "launch_plant" in dev
    assert int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 17


def test_mpc_desc_layout(pkg):
    """sizeof and field offsets in ctypes equal the header's under the natural-alignment rules; the Julia struct lists the same fields"""
    D = pkg._ffi.MpcDesc
    offs, size = S.c_layout(S.H_STRUCTS["ilqr_mpc_desc"])
    assert [f[0] for f in D._fields_] == [o[0] for o in offs]
    assert [getattr(D, nm).offset for nm, _ in offs] == [o for _, o in offs]
    assert C.sizeof(D) == size == 56
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    body = re.search(r"struct MpcDesc\n(.*?)\nend", jl, flags=re.S).group(1)
    fields = [ln.strip().split("::") for ln in body.splitlines()]
    jt = {"Int32": "i32", "UInt64": "u64", "Int64": "i64", "Ptr{Float64}": "ptr:f64"}
    assert [(f, jt[t]) for f, t in fields] == [(nm, t) for nm, t, _ in S.H_STRUCTS["ilqr_mpc_desc"]]


@pytest.mark.parametrize("fn", STEP_FNS)
def test_plant_step_refusals_need_no_device(pkg, fn):
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    buf = np.zeros(8)
    pd = buf.ctypes.data_as(pkg._ffi.c_double_p)
    p = pd if fn == STEP_FNS[0] else C.c_void_p(buf.ctypes.data)
    nan = np.array([np.nan]).ctypes.data_as(pkg._ffi.c_double_p)
    neg = np.array([-0.5]).ctypes.data_as(pkg._ffi.c_double_p)
    for steps, first, step0, sigma, x, msg in [(1, 0, 0, None, None, b"null x"), (0, 0, 0, None, p, b"steps must lie in 1 .. T-1"),
                                               (-3, 0, 0, pd, p, b"steps must lie in 1 .. T-1"), (1, 0, -1, None, p, b"step0 >= 0"),
                                               (2, 0, 2 ** 20 - 1, None, p, b"beyond 2^20"), (1, -1, 0, None, p, b"first_instance must lie"),
                                               (1, 2 ** 23, 0, None, p, b"first_instance must lie"), (1, 0, 0, nan, p, b"sigma_x must be finite"),
                                               (1, 0, 0, neg, p, b"sigma_x must be finite"), (1, 0, 0, None, p, b"null handle"),
                                               (3, 5, 2 ** 20 - 3, pd, p, b"null handle")]:
        assert f(None, steps, 0, 1, first, step0, sigma, None, x, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_mpc_run_refusals_need_no_device(pkg):
    L = pkg._ffi.lib()
    nan = np.array([np.inf])

    def desc(**kw):
        base = dict(periods=2, steps=1, plant_feedback=0, shift_feedback=0, shift_tail=0, warm=0, duals_tail=0, duals_penalty=0, seed=1,
                    first_instance=0, sigma_x=None)
        base.update(kw)
        return pkg._ffi.MpcDesc(**base)

    for d, msg in [(None, b"null descriptor"), (desc(periods=0), b"periods must be >= 1"), (desc(periods=-2), b"periods must be >= 1"),
                   (desc(steps=0), b"steps must lie in 1 .. T-1"), (desc(periods=2 ** 19 + 1, steps=2), b"beyond 2^20"),
                   (desc(first_instance=-1), b"first_instance must lie"), (desc(sigma_x=nan.ctypes.data_as(pkg._ffi.c_double_p)), b"sigma_x must be finite"),
                   (desc(), b"null handle"), (desc(periods=2 ** 20, steps=1, warm=1), b"null handle")]:
        assert L.ilqr_mpc_run(None, C.byref(d) if d is not None else None, None, None, None, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and b"ilqr_mpc_run" in err, err
