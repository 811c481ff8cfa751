"""ilqr_estimate_update_linear, ilqr_plant_measure_linear (host and device forms) and ilqr_mpc_run_sensor without a GPU: the symbols
are exported, declared, mirrored and in the Julia file; ilqr_sensor has the header's layout in ctypes and in Julia; every refusal
that needs no handle holds on a machine with no device (a non-finite entry of a host-side H needs the handle's dimensions and is
in tests/test_gpu_sensor.py, as is the refusal of the device forms on a sharded handle; nx > 64 cannot be shown: no built-in
model has more than 64 states); the Python mirror rejects wrong shapes before any call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE_FNS = ["ilqr_estimate_update_linear", "ilqr_estimate_update_linear_device"]
MEASURE_FNS = ["ilqr_plant_measure_linear", "ilqr_plant_measure_linear_device"]
FNS = UPDATE_FNS + MEASURE_FNS + ["ilqr_mpc_run_sensor"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    for fn in FNS:
        assert hasattr(p._ffi.lib(), fn), "the library has no %s: nothing here has a subject" % fn
    return p


def _vec(*v):
    return np.array(v, dtype=np.float64)


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = S.strip_comments(open(os.path.join(ROOT, "include", "ilqr_hip.h")).read())
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert pkg._ffi.SYMBOLS[name][0] is C.c_int and len(pkg._ffi.SYMBOLS[name][1]) == len(S.H_PROTOS[name][1]), name
    for name in UPDATE_FNS:
        assert S.H_PROTOS[name][1] == ["ptr:void", "i32", "i32"] + ["ptr:f64"] * 8 + ["ptr:i32"]
    for name in MEASURE_FNS:
        assert S.H_PROTOS[name][1] == ["ptr:void", "u64", "i64", "i32", "i32"] + ["ptr:f64"] * 4
    assert pkg._ffi.SYMBOLS[MEASURE_FNS[1]][1][5] is C.c_void_p and pkg._ffi.SYMBOLS[MEASURE_FNS[0]][1][5] is pkg._ffi.c_double_p      # H: device / host
    assert S.H_PROTOS["ilqr_mpc_run_sensor"][1] == (["ptr:void", "ptr:struct:ilqr_mpc_desc", "ptr:struct:ilqr_plant_io", "ptr:struct:ilqr_sensor"]
                                                    + ["ptr:f64"] * 8 + ["ptr:i32"] + ["ptr:f64"] * 3 + ["ptr:i32"] + ["ptr:f64"] * 3)
    # the older entry points keep their signatures
    assert S.H_PROTOS["ilqr_estimate_update"][1] == ["ptr:void", "ptr:i32"] + ["ptr:f64"] * 6 + ["ptr:i32"]
    assert S.H_PROTOS["ilqr_plant_measure"][1] == ["ptr:void", "u64", "i64", "i32"] + ["ptr:f64"] * 3
    assert S.H_PROTOS["ilqr_mpc_run_est"][1] == (["ptr:void", "ptr:struct:ilqr_mpc_desc", "ptr:struct:ilqr_plant_io", "ptr:struct:ilqr_estimator"]
                                                 + ["ptr:f64"] * 8 + ["ptr:i32"] + ["ptr:f64"] * 3 + ["ptr:i32"] + ["ptr:f64"] * 3)
    for fn in ("estimate_update_linear_", "estimate_update_linear_device_", "plant_measure_linear_", "plant_measure_linear_device_"):
        assert callable(getattr(pkg.Solver, fn)), fn
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    sen = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device_sensor.hpp")).read()
    assert "&launch_sensor_update<M>" in dev and "&launch_plant_measure_linear<M>" in dev
    assert int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 21
    assert "static_assert(sizeof(SensorArgs) <= 4096" in sen
    for kernel in ("sensor_update_kernel", "sensor_update_large_kernel", "plant_measure_linear_kernel"):
        assert kernel in sen, kernel
    assert os.path.exists(os.path.join(ROOT, "examples", "mpc_sensor.c")) and os.path.exists(os.path.join(ROOT, "tools", "sensor_time.py"))


def test_sensor_layout_in_header_ctypes_and_julia(pkg):
    fields = S.H_STRUCTS["ilqr_sensor"]
    assert fields == [("ny", "i32", None), ("reserved", "i32", None), ("H", "ptr:f64", None), ("r", "ptr:f64", None), ("q", "ptr:f64", None),
                      ("sigma_y", "ptr:f64", None)]
    Sen = pkg._ffi.Sensor
    offs, size = S.c_layout(fields)
    assert Sen.__name__ == "ilqr_sensor" and [f[0] for f in Sen._fields_] == [o[0] for o in offs]
    assert [getattr(Sen, nm).offset for nm, _ in offs] == [o for _, o in offs] and C.sizeof(Sen) == size == 40
    jl = open(S.JULIA).read()
    m = re.search(r"struct Sensor\s*(.*?)\bend\b", jl, flags=re.S)
    assert m and [ln.strip() for ln in m.group(1).strip().splitlines()] == ["ny::Int32", "reserved::Int32", "H::Ptr{Float64}", "r::Ptr{Float64}",
                                                                              "q::Ptr{Float64}", "sigma_y::Ptr{Float64}"]
    for name in ("ilqr_estimate_update_linear", "ilqr_plant_measure_linear", "ilqr_mpc_run_sensor"):
        assert ":" + name in jl, name
    for fn in ("estimate_update_linear!", "plant_measure_linear!", "mpc_run_sensor!"):
        assert "function " + fn in jl and re.search(r"^export .*\b%s" % re.escape(fn), jl, flags=re.M), fn


@pytest.mark.parametrize("fn", UPDATE_FNS)
def test_update_refusals_need_no_device(pkg, fn):
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p
    buf = np.zeros(8)
    host = fn == UPDATE_FNS[0]
    x = buf.ctypes.data_as(F64) if host else C.c_void_p(buf.ctypes.data)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    for ny, per, H, r, yy, xx, pp, msg in [
            (1, 0, None, _vec(1.0), x, x, x, b"null H, r, y, xhat or P"), (1, 0, x, None, x, x, x, b"null H, r, y, xhat or P"),
            (1, 0, x, _vec(1.0), None, x, x, b"null H, r, y, xhat or P"), (1, 0, x, _vec(1.0), x, None, x, b"null H, r, y, xhat or P"),
            (1, 0, x, _vec(1.0), x, x, None, b"null H, r, y, xhat or P"),
            (0, 0, x, _vec(1.0), x, x, x, b"ny must lie in 1 .. 64"), (65, 0, x, np.ones(65), x, x, x, b"ny must lie in 1 .. 64"),
            (-1, 0, x, _vec(1.0), x, x, x, b"ny must lie in 1 .. 64"), (1, 2, x, _vec(1.0), x, x, x, b"per_instance_H must be 0 or 1"),
            (1, 0, x, _vec(0.0), x, x, x, b"r must be finite and > 0"), (1, 0, x, _vec(-1.0), x, x, x, b"r must be finite and > 0"),
            (1, 0, x, _vec(NAN), x, x, x, b"r must be finite and > 0"), (2, 0, x, _vec(1.0, INF), x, x, x, b"r must be finite and > 0"),
            (2, 1, x, _vec(1.0, 2.0), x, x, x, b"null handle")]:
        assert getattr(L, fn)(None, ny, per, H, p(r), yy, None, xx, pp, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


@pytest.mark.parametrize("fn", MEASURE_FNS)
def test_measure_refusals_need_no_device(pkg, fn):
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p
    buf = np.zeros(8)
    host = fn == MEASURE_FNS[0]
    x = buf.ctypes.data_as(F64) if host else C.c_void_p(buf.ctypes.data)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    ph = lambda a: None if a is None else (a.ctypes.data_as(F64) if host else C.c_void_p(a.ctypes.data))
    for first, step, ny, H, sy, xx, yy, msg in [
            (0, 0, 1, None, None, x, x, b"null H, x or y"), (0, 0, 1, buf, None, None, x, b"null H, x or y"), (0, 0, 1, buf, None, x, None, b"null H, x or y"),
            (0, 0, 0, buf, None, x, x, b"ny must lie in 1 .. 64"), (0, 0, 65, buf, None, x, x, b"ny must lie in 1 .. 64"),
            (0, -1, 1, buf, None, x, x, b"the measurement step must lie in 0 .. 2^20 - 1"), (0, 1 << 20, 1, buf, None, x, x, b"the measurement step must lie in"),
            (-1, 0, 1, buf, None, x, x, b"first_instance must lie in 0 .. 2^23 - 1"), (1 << 23, 0, 1, buf, None, x, x, b"first_instance must lie in"),
            (0, 0, 1, buf, _vec(-1.0), x, x, b"sigma_y must be finite and >= 0"), (0, 0, 2, buf, _vec(0.0, NAN), x, x, b"sigma_y must be finite and >= 0"),
            (0, 0, 1, buf, _vec(INF), x, x, b"sigma_y must be finite and >= 0"), (0, 0, 1, buf, _vec(0.5), x, x, b"null handle")]:
        assert getattr(L, fn)(None, 1, first, step, ny, ph(H), p(sy), xx, yy) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_mpc_run_sensor_refusals_need_no_device(pkg):
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    buf = np.zeros(8)
    d = pkg._ffi.MpcDesc(2, 1, 0, 0, 0, 0, 0, 0, 1, 0, None)

    def sen(ny=1, H=buf, r=_vec(1.0), q=None, sy=None):
        s = pkg._ffi.Sensor(ny, 0, p(H), p(r), p(q), p(sy))
        s._keep = (H, r, q, sy)
        return s

    def call(s, io=None, xhat0=None, Pc=buf, xhat_cl=None, pdiag_cl=None, nis_cl=None, desc=d):
        return L.ilqr_mpc_run_sensor(None, C.byref(desc) if desc is not None else None, C.byref(io) if io is not None else None,
                                     C.byref(s) if s is not None else None, None, p(xhat0), p(Pc), None, None, None, None, None, None, None, None, None,
                                     None, p(xhat_cl), p(pdiag_cl), p(nis_cl))
    noisy = pkg._ffi.PlantIO(None, None, p(buf), 0, 0)
    for kw, msg in [(dict(s=None, Pc=None, xhat_cl=buf), b"without an estimator"), (dict(s=None, Pc=None, nis_cl=buf), b"without an estimator"),
                    (dict(s=None), b"without an estimator"), (dict(s=None, Pc=None, xhat0=buf), b"without an estimator"),
                    (dict(s=sen(), Pc=None), b"a sensor with a null P"), (dict(s=sen(), io=noisy), b"io->sigma_y together with a sensor"),
                    (dict(s=sen(H=None)), b"null H or r"), (dict(s=sen(r=None)), b"null H or r"),
                    (dict(s=sen(ny=0)), b"ny must lie in 1 .. 64"), (dict(s=sen(ny=65, r=np.ones(65))), b"ny must lie in 1 .. 64"),
                    (dict(s=sen(r=_vec(0.0))), b"r must be finite and > 0"), (dict(s=sen(ny=2, r=_vec(1.0, NAN))), b"r must be finite and > 0"),
                    (dict(s=sen(q=_vec(-1.0))), b"q must be finite and >= 0"), (dict(s=sen(sy=_vec(-1.0))), b"sigma_y must be finite and >= 0"),
                    (dict(s=sen(ny=2, r=_vec(1.0, 1.0), sy=_vec(0.0, INF))), b"sigma_y must be finite and >= 0"),
                    (dict(s=sen(), io=pkg._ffi.PlantIO(None, None, None, 2, 0)), b"delay must be 0 or 1"),
                    (dict(s=sen(), desc=None), b"null descriptor"), (dict(s=sen()), b"null handle")]:
        assert call(**kw) == -1
        err = L.ilqr_last_error()
        assert msg in err and b"ilqr_mpc_run_sensor" in err, (msg, err)
    # sensor NULL and nothing of the filter asked for: ilqr_mpc_run_io's own refusals, under this entry point's name
    assert call(None, Pc=None) == -1 and b"ilqr_mpc_run_sensor: null handle" in L.ilqr_last_error()


class _Shape:
    B, T, nx, nu, num_user_parameter = 3, 11, 3, 2, 2
    _TAILS, _PENALTIES = {"hold": 0, "zero": 1}, {"keep": 0, "reset": 1}


def test_python_mirror_rejects_wrong_shapes(pkg):
    s = _Shape()
    for fn in ("_plant_arguments", "_estimate_arrays", "_sensor"):
        setattr(s, fn, (lambda f: lambda *a, **k: getattr(pkg.Solver, f)(s, *a, **k))(fn))
    x, Pm, H = np.zeros((3, 3)), np.zeros((3, 3, 3)), np.zeros((2, 3))
    with pytest.raises(ValueError, match=r"H must have shape \[ny, nx\] or \[B, ny, nx\]"):
        pkg.Solver.estimate_update_linear_(s, x, Pm, np.zeros((3, 2)), np.zeros((2, 4)), 1.0)
    with pytest.raises(ValueError, match=r"H must have shape \[ny, nx\] or \[B, ny, nx\]"):
        pkg.Solver.estimate_update_linear_(s, x, Pm, np.zeros((3, 2)), np.zeros((4, 2, 3)), 1.0)
    with pytest.raises(ValueError, match=r"y must have shape \[B, ny\]"):
        pkg.Solver.estimate_update_linear_(s, x, Pm, np.zeros((3, 3)), H, 1.0)
    with pytest.raises(ValueError, match=r"yhat must have shape \[B, ny\]"):
        pkg.Solver.estimate_update_linear_(s, x, Pm, np.zeros((3, 2)), H, 1.0, yhat=np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"x must have shape \[B, nx\]"):
        pkg.Solver.plant_measure_linear_(s, np.zeros((3, 2)), H)
    with pytest.raises(ValueError, match="one sensor for the batch"):
        pkg.Solver.plant_measure_linear_(s, x, np.zeros((3, 2, 3)))
    with pytest.raises(ValueError, match="one sensor for the batch"):
        pkg.Solver.mpc_run_(s, 2, estimator=dict(H=np.zeros((3, 2, 3)), r=1.0, P0=Pm))
    with pytest.raises(ValueError, match="exclude each other"):
        pkg.Solver.mpc_run_(s, 2, estimator=dict(H=H, measured=[1, 1, 0], r=1.0, P0=Pm))
    with pytest.raises(ValueError, match="replaces the loop's"):
        pkg.Solver.mpc_run_(s, 2, sigma_y=np.full(3, 0.1), estimator=dict(H=H, r=1.0, P0=Pm))
    with pytest.raises(ValueError, match="estimator needs r and P0"):
        pkg.Solver.mpc_run_(s, 2, estimator=dict(H=H, r=1.0))
    with pytest.raises(ValueError, match="unknown keys"):
        pkg.Solver.mpc_run_(s, 2, estimator=dict(H=H, r=1.0, P0=Pm, sigma=1.0))
