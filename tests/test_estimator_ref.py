"""The yardstick of the extended Kalman filter (tests/estimator_ref.py) without a GPU, on the inputs of tests/test_gpu_estimator.py:

  1. the complex-capable restatements of car and acrobot are the real callables of plant_ref on real states, and the complex-step
     Jacobian agrees with a central difference of the real callable;
  2. the sequential update and the textbook batch update (scipy, Joseph form) agree on x̂, P and nis within a tenth of TOL_XU = 1e-10
     relative to max(1, max |reference|) — so the GPU bound TOL_XU is an honest one (measured: printed per model);
  3. P stays symmetric and positive semi-definite (smallest eigenvalue >= −1e-12 · largest) through every step of every case;
  4. the properties the GPU test asserts hold on the yardstick with a factor of two to spare: a measured component without process
     noise has a smaller variance after the update; the filter beats the raw measurement on the positions and prediction alone on the
     velocities (tests/test_gpu_estimator.py, "it filters");
  5. every refusal of ilqr_estimate_predict / _update (both forms) and ilqr_mpc_run_est that needs no handle returns ILQR_ERR_INVALID
     on a machine with no device, and the symbols are exported, declared and mirrored."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_XU = 1e-10
FNS = ["ilqr_estimate_predict", "ilqr_estimate_predict_device", "ilqr_estimate_update", "ilqr_estimate_update_device", "ilqr_mpc_run_est"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    for fn in FNS:
        assert hasattr(p._ffi.lib(), fn), "the library has no %s: the yardstick has no subject" % fn
    return p


def _cases(pkg, name, B=3):
    """(x̂, P, y, xb, ub, w, k, mask) of every case of one model: the plan is the workload's inputs (no feedback: that needs a solve)"""
    x1, ub, w = R.inputs(pkg.workloads, name, B)
    n = x1.shape[1]
    xh, y = E.start(x1, n)
    xb = np.zeros((R.T, n))
    for k in R.STEPS:
        for mask in E.masks(name, n):
            yield xh, E.p_start(B, n), y, xb, ub, w, k, mask


@pytest.mark.parametrize("name", ["car_obs", "acrobot"])
def test_restated_dynamics_are_the_real_ones(pkg, name):
    x1, ub, w = R.inputs(pkg.workloads, name, 3)
    f, fc = R.dynamics(name), E.dynamics_complex(name)
    for b in range(3):
        wi = None if w is None else w[b, 0]
        a, c = np.asarray(f(x1[b], ub[b, 0], wi, 0)), np.asarray(fc(x1[b].astype(np.complex128), ub[b, 0], wi, 0))
        assert np.abs(c.imag).max() == 0.0 and P.rel(c.real, a) < 1e-15, (name, b)


@pytest.mark.parametrize("name", E.MODELS)
def test_complex_step_jacobian_against_a_central_difference(pkg, name):
    x1, ub, w = R.inputs(pkg.workloads, name, 3)
    f = R.dynamics(name)
    for b in range(3):
        wi = np.zeros(0) if w is None else w[b, 0]
        F = E.jacobian(name, x1[b], ub[b, 0], wi)
        h = 1e-6
        D = np.stack([(np.asarray(f(x1[b] + h * e, ub[b, 0], wi, 0)) - np.asarray(f(x1[b] - h * e, ub[b, 0], wi, 0))) / (2 * h) for e in np.eye(len(x1[b]))], axis=1)
        assert np.abs(F - D).max() < 1e-8, (name, b, np.abs(F - D).max())


@pytest.mark.parametrize("name", E.MODELS)
def test_sequential_and_batch_update_agree_and_p_stays_psd(pkg, name):
    worst = 0.0
    u_min, u_max = IO.LIMITS[name]
    for xh, Ps, y, xb, ub, w, k, mask in _cases(pkg, name):
        n = xh.shape[1]
        for b in range(xh.shape[0]):
            trace = []
            x, Pp = E.predict(name, xb, ub[b], None, None if w is None else w[b], xh[b], Ps[b], k, u_min=u_min, u_max=u_max, q=E.q(n), trace=trace)
            seq = E.update_sequential(x, Pp, y[b], E.r(n), mask, trace=trace)
            bat = E.update_batch(x, Pp, y[b], E.r(n), mask)
            assert seq["first_bad"] == -1
            d = max(P.rel(seq["xhat"], bat["xhat"]), P.rel(seq["P"], bat["P"]), abs(seq["nis"] - bat["nis"]) / max(1.0, abs(bat["nis"])))
            worst = max(worst, d)
            assert d <= 0.1 * TOL_XU, (name, k, b, d)
            for Q in trace:
                ev = np.linalg.eigvalsh(Q)
                assert np.array_equal(Q, Q.T) and ev[0] >= -1e-12 * ev[-1], (name, k, b, ev[0], ev[-1])
            # a measured component without process noise: the update shrinks its variance, with a factor of two to spare on the gap
            assert mask[0] == 1 and E.q(n)[0] == 0.0 and seq["P"][0, 0] < Pp[0, 0] and Pp[0, 0] - seq["P"][0, 0] > 2e-10 * Pp[0, 0]
            # the unmeasured components of y are not read
            yn = y[b].copy(); yn[mask == 0] = NAN
            again = E.update_sequential(x, Pp, yn, E.r(n), mask)
            assert np.array_equal(again["xhat"], seq["xhat"]) and np.array_equal(again["P"], seq["P"])
    print("sequential against batch %s: worst relative difference %.2e (bound %.1e)" % (name, worst, 0.1 * TOL_XU))


def test_a_bad_pivot_is_skipped_and_marked():
    Pm = np.diag([1.0, NAN, 1.0]); y = np.array([1.0, 1.0, 1.0])
    u = E.update_sequential(np.zeros(3), Pm, y, np.ones(3))
    assert u["first_bad"] == 1 and u["innovation"][1] == 0.0 and u["xhat"][0] == 0.5 and u["xhat"][2] == 0.5 and u["nis"] == 1.0


def test_the_yardstick_filters(pkg):
    F = E.FILTER
    x1, ub, _ = R.inputs(pkg.workloads, F["name"], F["B"])
    z = pkg.candidate_noise(F["seed"], F["B"], *IO.measure_shape(F["periods"] * F["k"]))
    pos_hat, pos_y, vel_hat, vel_open = E.filter_scores(E.filter_run(ub, x1, z))
    print("filter on the yardstick: positions %.3e (measurement %.3e), velocities %.3e (prediction alone %.3e)" % (pos_hat, pos_y, vel_hat, vel_open))
    assert 2.0 * pos_hat < pos_y and 2.0 * vel_hat < vel_open


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = S.strip_comments(open(os.path.join(ROOT, "include", "ilqr_hip.h")).read())
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert pkg._ffi.SYMBOLS[name][0] is C.c_int and len(pkg._ffi.SYMBOLS[name][1]) == len(S.H_PROTOS[name][1]), name
    assert S.H_PROTOS["ilqr_estimate_predict"][1] == ["ptr:void", "i32", "i32"] + ["ptr:f64"] * 5
    assert S.H_PROTOS["ilqr_estimate_update"][1] == ["ptr:void", "ptr:i32"] + ["ptr:f64"] * 6 + ["ptr:i32"]
    assert S.H_PROTOS["ilqr_mpc_run_est"][1] == (["ptr:void", "ptr:struct:ilqr_mpc_desc", "ptr:struct:ilqr_plant_io", "ptr:struct:ilqr_estimator"]
                                                 + ["ptr:f64"] * 8 + ["ptr:i32"] + ["ptr:f64"] * 3 + ["ptr:i32"] + ["ptr:f64"] * 3)
    fields = S.H_STRUCTS["ilqr_estimator"]
    assert fields == [("measured", "ptr:i32", None), ("q", "ptr:f64", None), ("r", "ptr:f64", None)]
    Est = pkg._ffi.Estimator
    assert Est.__name__ == "ilqr_estimator" and [f[0] for f in Est._fields_] == ["measured", "q", "r"] and C.sizeof(Est) == 24
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    est = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device_estimate.hpp")).read()
    assert "launch_estimate_update<M>}" in dev and int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) >= 20
    assert "static_assert(sizeof(EstArgs) <= 4096" in est
    for fn in ("estimate_predict_", "estimate_predict_device_", "estimate_update_", "estimate_update_device_"):
        assert callable(getattr(pkg.Solver, fn)), fn


def _vec(*v):
    return np.array(v, dtype=np.float64)


@pytest.mark.parametrize("fn", FNS[:2])
def test_predict_refusals_need_no_device(pkg, fn):
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p
    buf = np.zeros(8)
    x = buf.ctypes.data_as(F64) if fn == FNS[0] else C.c_void_p(buf.ctypes.data)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    for steps, lo, hi, q, xx, pp, msg in [
            (1, None, None, None, None, x, b"null xhat or P"), (1, None, None, None, x, None, b"null xhat or P"),
            (1, None, None, _vec(-1.0), x, x, b"q must be finite and >= 0"), (1, None, None, _vec(NAN), x, x, b"q must be finite and >= 0"),
            (1, None, None, _vec(INF), x, x, b"q must be finite and >= 0"), (0, None, None, None, x, x, b"steps must lie in 1 .. T-1"),
            (1, _vec(NAN), None, None, x, x, b"limit of the actuator is NaN"), (1, _vec(1.0), _vec(0.5), None, x, x, b"u_min must not exceed u_max"),
            (1, _vec(0.0), _vec(1.0), _vec(0.0), x, x, b"null handle")]:
        assert getattr(L, fn)(None, steps, 0, p(lo), p(hi), p(q), xx, pp) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


@pytest.mark.parametrize("fn", FNS[2:4])
def test_update_refusals_need_no_device(pkg, fn):
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    buf = np.zeros(8)
    x = buf.ctypes.data_as(F64) if fn == FNS[2] else C.c_void_p(buf.ctypes.data)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    one, zero, two = (np.array([v], dtype=np.int32) for v in (1, 0, 2))
    for mask, r, yy, xx, pp, msg in [
            (None, _vec(1.0), None, x, x, b"null xhat, P or y"), (None, _vec(1.0), x, None, x, b"null xhat, P or y"), (None, _vec(1.0), x, x, None, b"null xhat, P or y"),
            (None, None, x, x, x, b"null r"), (two, _vec(1.0), x, x, x, b"a mask entry must be 0 or 1"),
            (None, _vec(0.0), x, x, x, b"r must be finite and > 0"), (one, _vec(-1.0), x, x, x, b"r must be finite and > 0"),
            (one, _vec(NAN), x, x, x, b"r must be finite and > 0"), (None, _vec(INF), x, x, x, b"r must be finite and > 0"),
            (zero, _vec(NAN), x, x, x, b"null handle"), (None, _vec(1.0), x, x, x, b"null handle")]:
        assert getattr(L, fn)(None, None if mask is None else mask.ctypes.data_as(I32), p(r), yy, xx, pp, None, None, None) == -1
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_mpc_run_est_refusals_need_no_device(pkg):
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    p = lambda a: None if a is None else a.ctypes.data_as(F64)
    buf = np.zeros(8)
    d = pkg._ffi.MpcDesc(2, 1, 0, 0, 0, 0, 0, 0, 1, 0, None)

    def est(mask=None, q=None, r=None):
        e = pkg._ffi.Estimator(None if mask is None else mask.ctypes.data_as(I32), p(q), p(r))
        e._keep = (mask, q, r)
        return e

    def call(e, io=None, xhat0=None, Pc=buf, xhat_cl=None, pdiag_cl=None, nis_cl=None, desc=d):
        return L.ilqr_mpc_run_est(None, C.byref(desc) if desc is not None else None, C.byref(io) if io is not None else None, C.byref(e) if e is not None else None,
                                  None, p(xhat0), p(Pc), None, None, None, None, None, None, None, None, None, None, p(xhat_cl), p(pdiag_cl), p(nis_cl))
    two = np.array([2], dtype=np.int32)
    for kw, msg in [(dict(e=None, Pc=None, xhat_cl=buf), b"without an estimator"), (dict(e=None, Pc=None, pdiag_cl=buf), b"without an estimator"),
                    (dict(e=None, Pc=None, nis_cl=buf), b"without an estimator"), (dict(e=None), b"without an estimator"),
                    (dict(e=est(r=_vec(1.0)), Pc=None), b"an estimator with a null P"), (dict(e=est()), b"null r"),
                    (dict(e=est(r=_vec(0.0))), b"r must be finite and > 0"), (dict(e=est(q=_vec(-1.0), r=_vec(1.0))), b"q must be finite and >= 0"),
                    (dict(e=est(mask=two, r=_vec(1.0))), b"a mask entry must be 0 or 1"),
                    (dict(e=est(r=_vec(1.0)), io=pkg._ffi.PlantIO(None, None, None, 2, 0)), b"delay must be 0 or 1"),
                    (dict(e=est(r=_vec(1.0)), desc=None), b"null descriptor"), (dict(e=est(r=_vec(1.0))), b"null handle")]:
        assert call(**kw) == -1
        err = L.ilqr_last_error()
        assert msg in err and b"ilqr_mpc_run_est" in err, (msg, err)
    # est NULL and nothing of the filter asked for: ilqr_mpc_run_io's own refusals, under this entry point's name
    assert call(None, Pc=None) == -1 and b"ilqr_mpc_run_est: null handle" in L.ilqr_last_error()


class _Shape:
    B, T, nx, nu, num_user_parameter = 3, 11, 3, 2, 2
    _TAILS, _PENALTIES = {"hold": 0, "zero": 1}, {"keep": 0, "reset": 1}


def test_python_mirror_rejects_wrong_shapes(pkg):
    s = _Shape()
    s._plant_arguments = lambda *a: pkg.Solver._plant_arguments(s, *a)
    s._estimate_arrays = lambda *a: pkg.Solver._estimate_arrays(s, *a)
    x, Pm = np.zeros((3, 3)), np.zeros((3, 3, 3))
    with pytest.raises(ValueError, match=r"xhat must have shape \[B, nx\]"):
        pkg.Solver.estimate_predict_(s, np.zeros((3, 2)), Pm)
    with pytest.raises(ValueError, match=r"P must have shape \[B, nx, nx\]"):
        pkg.Solver.estimate_predict_(s, x, np.zeros((3, 3, 2)))
    with pytest.raises(ValueError, match="measured must have nx entries"):
        pkg.Solver.estimate_update_(s, x, Pm, x, 1.0, measured=[1, 0])
    with pytest.raises(ValueError, match=r"y must have shape \[B, nx\]"):
        pkg.Solver.estimate_update_(s, x, Pm, np.zeros((3, 4)), 1.0)
    with pytest.raises(ValueError, match="estimator needs r and P0"):
        pkg.Solver.mpc_run_(s, 2, estimator=dict(r=1.0))
    with pytest.raises(ValueError, match="unknown keys"):
        pkg.Solver.mpc_run_(s, 2, estimator=dict(r=1.0, P0=Pm, sigma=1.0))
