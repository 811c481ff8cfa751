"""ilqr_plant_step_limited, ilqr_plant_measure (host and device forms) and ilqr_mpc_run_io without a GPU: the symbols are exported,
declared, mirrored and in the Julia file; ilqr_plant_io has the header's layout in ctypes and in Julia; every refusal that needs no
handle holds on a machine with no device (of a vector: its first entry — the rest needs the handle's dimensions and is in
tests/test_gpu_plant_io.py, as is the refusal of the device forms on a sharded handle; no built-in model has more than 16 actions, so
the nu > 16 refusal has no handle to be shown on); the Python mirror rejects wrong shapes before any call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_FNS = ["ilqr_plant_step_limited", "ilqr_plant_step_limited_device"]
MEASURE_FNS = ["ilqr_plant_measure", "ilqr_plant_measure_device"]
FNS = STEP_FNS + MEASURE_FNS + ["ilqr_mpc_run_io"]
NAN, INF = float("nan"), float("inf")


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
        assert len(pkg._ffi.SYMBOLS[name][1]) == len(S.H_PROTOS[name][1]), name
    for name in STEP_FNS:          # ilqr_plant_step's arguments with the limits behind sigma_x and saturated at the end
        assert S.H_PROTOS[name][1] == ["ptr:void", "i32", "i32", "u64", "i64", "i32"] + ["ptr:f64"] * 7 + ["ptr:i32"] * 2
    for name in MEASURE_FNS:
        assert S.H_PROTOS[name][1] == ["ptr:void", "u64", "i64", "i32"] + ["ptr:f64"] * 3
    assert S.H_PROTOS["ilqr_mpc_run_io"][1] == (["ptr:void", "ptr:struct:ilqr_mpc_desc", "ptr:struct:ilqr_plant_io"] + ["ptr:f64"] * 6 + ["ptr:i32"]
                                                + ["ptr:f64"] * 3 + ["ptr:i32"])
    # the older entry points keep their signatures
    assert S.H_PROTOS["ilqr_plant_step"][1] == ["ptr:void", "i32", "i32", "u64", "i64", "i32"] + ["ptr:f64"] * 5 + ["ptr:i32"]
    assert S.H_PROTOS["ilqr_mpc_run_preview"][1] == ["ptr:void", "ptr:struct:ilqr_mpc_desc"] + ["ptr:f64"] * 6 + ["ptr:i32"] + ["ptr:f64"] * 2
    assert C.sizeof(pkg._ffi.MpcDesc) == 56
    for fn in ("plant_measure_", "plant_measure_device_"):
        assert callable(getattr(pkg.Solver, fn)), fn
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    plant = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device_plant.hpp")).read()
    assert "launch_plant_measure" in dev and int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 19
    assert "static_assert(sizeof(PlantArgs) <= 4096" in plant and "plant_measure_kernel" in plant
    assert os.path.exists(os.path.join(ROOT, "examples", "mpc_limits.c")) and os.path.exists(os.path.join(ROOT, "tools", "mpc_io_time.py"))


def test_plant_io_layout_in_header_ctypes_and_julia(pkg):
    fields = S.H_STRUCTS["ilqr_plant_io"]
    assert fields == [("u_min", "ptr:f64", None), ("u_max", "ptr:f64", None), ("sigma_y", "ptr:f64", None), ("delay", "i32", None), ("reserved", "i32", None)]
    offs, size = S.c_layout(fields)
    assert offs == [("u_min", 0), ("u_max", 8), ("sigma_y", 16), ("delay", 24), ("reserved", 28)] and size == 32
    P = pkg._ffi.PlantIO
    assert P is pkg._ffi.ilqr_plant_io and P.__name__ == "ilqr_plant_io"
    assert [f[0] for f in P._fields_] == [o[0] for o in offs] and [getattr(P, nm).offset for nm, _ in offs] == [o for _, o in offs]
    assert C.sizeof(P) == size
    # the Julia struct, field for field, and the three bindings
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    m = re.search(r"struct PlantIO\s*(.*?)\bend\b", jl, flags=re.S)
    assert m, "no struct PlantIO in the Julia file"
    got = [tuple(s.strip() for s in line.split("::")) for line in m.group(1).splitlines() if "::" in line]
    assert got == [("u_min", "Ptr{Float64}"), ("u_max", "Ptr{Float64}"), ("sigma_y", "Ptr{Float64}"), ("delay", "Int32"), ("reserved", "Int32")]
    assert ":ilqr_plant_step_limited, LIB[]" in jl and ":ilqr_plant_measure, LIB[]" in jl and ":ilqr_mpc_run_io" in jl
    assert "Ref{MpcDesc}, Ref{PlantIO}" in jl
    for fn in ("plant_measure!,", "mpc_run_io!,", "PlantIO,"):
        assert fn in jl.split("const LIB")[0], fn
    # the ccalls the static check parses agree with the header (the file's own test, on the new symbols)
    calls = {c[0]: c for c in S.parse_julia()[0]}
    for name in ("ilqr_plant_step_limited", "ilqr_plant_measure"):
        _, ret, argt, _ = calls[name]
        assert [S.jl_type(a) for a in argt] == S.H_PROTOS[name][1] and S.jl_type(ret) == "i32", name


def _vec(*v):
    return np.array(v, dtype=np.float64)


@pytest.mark.parametrize("fn", STEP_FNS)
def test_limited_step_refusals_need_no_device(pkg, fn):
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    F64 = pkg._ffi.c_double_p
    buf = np.zeros(8)
    x = buf.ctypes.data_as(F64) if fn == STEP_FNS[0] else C.c_void_p(buf.ctypes.data)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    for steps, step0, sig, lo, hi, xx, msg in [
            (1, 0, None, _vec(NAN), None, x, b"limit of the actuator is NaN"), (1, 0, None, None, _vec(NAN), x, b"limit of the actuator is NaN"),
            (1, 0, None, _vec(1.0), _vec(0.5), x, b"u_min must not exceed u_max"), (1, 0, None, _vec(INF), _vec(-INF), x, b"u_min must not exceed u_max"),
            (0, 0, None, _vec(0.0), _vec(1.0), x, b"steps must lie in 1 .. T-1"), (1, 2 ** 20, None, None, None, x, b"beyond 2^20"),
            (1, 0, _vec(-1.0), None, None, x, b"sigma_x must be finite"), (1, 0, None, _vec(0.0), _vec(1.0), None, b"null x"),
            (1, 0, None, _vec(-INF), _vec(INF), x, b"null handle"), (1, 0, None, _vec(0.5), _vec(0.5), x, b"null handle")]:
        assert f(None, steps, 0, 0, 0, step0, p(sig), p(lo), p(hi), None, xx, None, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


@pytest.mark.parametrize("fn", MEASURE_FNS)
def test_measure_refusals_need_no_device(pkg, fn):
    L = pkg._ffi.lib()
    f = getattr(L, fn)
    F64 = pkg._ffi.c_double_p
    buf = np.zeros(8)
    x = buf.ctypes.data_as(F64) if fn == MEASURE_FNS[0] else C.c_void_p(buf.ctypes.data)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    for first, step, sig, xx, yy, msg in [(0, -1, None, x, x, b"measurement step"), (0, 2 ** 20, None, x, x, b"measurement step"),
                                          (-1, 0, None, x, x, b"first_instance must lie"), (2 ** 23, 0, None, x, x, b"first_instance must lie"),
                                          (0, 0, _vec(-0.5), x, x, b"sigma_y must be finite"), (0, 0, _vec(INF), x, x, b"sigma_y must be finite"),
                                          (0, 0, _vec(NAN), x, x, b"sigma_y must be finite"), (0, 0, None, None, x, b"null x or y"),
                                          (0, 0, None, x, None, b"null x or y"), (0, 2 ** 20 - 1, _vec(0.0), x, x, b"null handle")]:
        assert f(None, 1, first, step, p(sig), xx, yy) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_mpc_run_io_refusals_need_no_device(pkg):
    L = pkg._ffi.lib()
    F64 = pkg._ffi.c_double_p
    p = lambda a: None if a is None else a.ctypes.data_as(F64)

    def desc(**kw):
        base = dict(periods=2, steps=1, plant_feedback=0, shift_feedback=0, shift_tail=0, warm=0, duals_tail=0, duals_penalty=0, seed=1,
                    first_instance=0, sigma_x=None)
        base.update(kw)
        return pkg._ffi.MpcDesc(**base)

    def io(u_min=None, u_max=None, sigma_y=None, delay=0):
        keep = (u_min, u_max, sigma_y)
        s = pkg._ffi.PlantIO(p(u_min), p(u_max), p(sigma_y), delay, 0)
        s._keep = keep
        return s

    full = 2 ** 20
    for d, i, msg in [(desc(), io(delay=2), b"delay must be 0 or 1"), (desc(), io(delay=-1), b"delay must be 0 or 1"),
                      (desc(), io(u_min=_vec(NAN)), b"limit of the actuator is NaN"), (desc(), io(u_max=_vec(NAN), delay=1), b"limit of the actuator is NaN"),
                      (desc(), io(u_min=_vec(2.0), u_max=_vec(1.0)), b"u_min must not exceed u_max"),
                      (desc(), io(sigma_y=_vec(-1.0)), b"sigma_y must be finite"), (desc(), io(sigma_y=_vec(INF), delay=1), b"sigma_y must be finite"),
                      # delay 0 measures after the last plant step, at P·k: one step less fits than the plant alone allows
                      (desc(periods=full, steps=1), io(sigma_y=_vec(0.1)), b"measurement step"),
                      (desc(periods=full // 2, steps=2), io(u_max=_vec(1.0)), b"measurement step"),
                      (desc(periods=full, steps=1), io(delay=1), b"null handle"),                   # delay 1: the last one at (P−1)·k
                      (desc(periods=full, steps=1), io(), b"null handle"),                          # nothing measured: ilqr_mpc_run's rule
                      (desc(periods=full + 1, steps=1), io(delay=1), b"measurement step"), (desc(periods=full + 1, steps=1), io(), b"beyond 2^20"),
                      (None, io(), b"null descriptor"), (desc(periods=0), io(), b"periods must be >= 1"), (desc(steps=0), io(delay=1), b"steps must lie in 1 .. T-1"),
                      (desc(), None, b"null handle"), (desc(), io(u_min=_vec(-1.0), u_max=_vec(1.0), sigma_y=_vec(0.0), delay=1), b"null handle")]:
        assert L.ilqr_mpc_run_io(None, C.byref(d) if d is not None else None, C.byref(i) if i is not None else None, None, None, None, None, None, None,
                                 None, None, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and b"ilqr_mpc_run_io" in err, (msg, err)
    buf = np.zeros(8)
    assert L.ilqr_mpc_run_io(None, C.byref(desc()), None, None, None, None, None, None, None, None, None, p(buf), None, None) == -1
    assert b"cl_violation without cl_cost" in L.ilqr_last_error()
    # the older entry points keep their own names in their messages
    assert L.ilqr_mpc_run_preview(None, C.byref(desc()), None, None, None, None, None, None, None, None, None) == -1
    assert b"ilqr_mpc_run_preview: null handle" in L.ilqr_last_error()
    assert L.ilqr_plant_step(None, 1, 0, 0, 0, 0, None, None, p(buf), None, None, None) == -1
    assert b"ilqr_plant_step: null handle" in L.ilqr_last_error()


class _Shape:
    """what the shape checks of the Python mirror read of a Solver: no handle, so nothing reaches the library"""
    B, T, nx, nu, num_user_parameter = 3, 11, 3, 2, 2
    _TAILS, _PENALTIES = {"hold": 0, "zero": 1}, {"keep": 0, "reset": 1}


def test_python_mirror_rejects_wrong_shapes(pkg):
    s = _Shape()
    s._plant_arguments = lambda *a: pkg.Solver._plant_arguments(s, *a)
    x = np.zeros((3, 3))
    for kw, msg in [(dict(u_min=[0.0]), "u_min must have nu entries"), (dict(u_max=[0.0, 1.0, 2.0]), "u_max must have nu entries"),
                    (dict(u_min=np.zeros((2, 1))), "u_min must have nu entries")]:
        with pytest.raises(ValueError, match=msg):
            pkg.Solver.plant_step_(s, x, **kw)
        with pytest.raises(ValueError, match=msg):
            pkg.Solver.mpc_run_(s, 2, **kw)
    for kw, msg in [(dict(sigma_y=[0.0, 1.0]), "sigma_y must have nx entries"), (dict(delay=2), "delay must be 0 or 1"), (dict(delay=-1), "delay must be 0 or 1")]:
        with pytest.raises(ValueError, match=msg):
            pkg.Solver.mpc_run_(s, 2, **kw)
    with pytest.raises(ValueError, match="sigma_y must have nx entries"):
        pkg.Solver.plant_measure_(s, x, sigma_y=np.zeros(4))
    with pytest.raises(ValueError, match=r"x must have shape \[B, nx\]"):
        pkg.Solver.plant_measure_(s, np.zeros((3, 2)))
