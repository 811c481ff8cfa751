"""The yardstick of the compiled nonlinear sensor y = h(x, s) + v (tests/test_sensor_nl_ref.py, tests/test_sensor_codegen.py,
tests/test_gpu_sensor_nl.py): ilqr_sensor_linearise, ilqr_plant_measure_sensor and ilqr_estimate_update_sensor as include/ilqr_hip.h
defines them, in plain fp64 numpy —

    linearise:  H = ∂h/∂x at x_lin;  ŷ_j = h_j(x_lin, s), with x_prior given + Σ_k H_jk (x_prior_k − x_lin_k) over ascending k from h_j
    measure:    y_j = h_j(x, s) + sigma_y[j] · z[5 + j // 16, step, j % 16]
    update:     iteration 0: (H, ŷ) at x̂₀, sensor_ref.update_sequential(x̂₀, P₀, y, H, r, ŷ); iteration i >= 1: (H, ŷ) at the estimate of
                iteration i − 1 with x_prior = x̂₀, the same update from (x̂₀, P₀) again; the last iteration's outputs

ONE definition per sensor, `h(x, s, m)` over a module m that supplies sin, cos, tanh and sqrt: sympy traces it for the code
generator (`symbolic`), numpy evaluates it here. THE JACOBIAN of the yardstick is the complex-step derivative of the numpy form,
Im h(x + i·1e-30·e_k) / 1e-30: exact to rounding and from nothing the device runs (the device compiles sympy's symbolic derivative).
`iekf_textbook` is the Gauss-Newton iterated filter written out on its own: x_{i+1} = x̂₀ + K_i (y − h(x_i) − H_i (x̂₀ − x_i)),
K_i = P₀ H_iᵀ (H_i P₀ H_iᵀ + R)⁻¹ through LAPACK, Joseph-form covariance."""
import numpy as np

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import sensor_ref as S

SEED = R.SEED
STEP = 1.0e-30


# ------------------------------------------------------------------------------------------------------------- the sensors
def _range_heading(x, s, m):
    return [m.sqrt(x[0] * x[0] + x[1] * x[1]), x[2]]


def _beacons2(x, s, m):
    return [m.sqrt((x[0] - s[0]) * (x[0] - s[0]) + (x[1] - s[1]) * (x[1] - s[1])),
            m.sqrt((x[0] - s[2]) * (x[0] - s[2]) + (x[1] - s[3]) * (x[1] - s[3]))]


def _encoder(x, s, m):
    return [m.sin(x[0]), m.cos(x[0]), x[0] + x[1]]


def _mix12(x, s, m):
    """ny = 13 > nx: tanh and products, row 11 a plain selection (one non-zero partial), row 12 dense"""
    rows = [m.tanh(x[j]) * x[j + 1] + s[0] * x[j] for j in range(11)]
    rows.append(x[5])
    acc = 0.0 * x[0]
    for k in range(12):
        acc = acc + float(np.cos(0.4 * (k + 1))) * x[k]
    rows.append(m.tanh(s[1] * acc))
    return rows


def _mix32(x, s, m):
    rows = [m.sin(x[j]) + s[0] * x[(j + 1) % 32] * x[(j + 5) % 32] for j in range(32)]
    acc = 0.0 * x[0]
    for k in range(32):
        acc = acc + x[k]
    rows.append(m.tanh(0.1 * acc))
    return rows


def _wide12(x, s, m):
    return [m.sin(0.1 * (j + 1) * x[j % 12]) + x[(j + 3) % 12] * x[(j + 7) % 12] for j in range(64)]


# key -> (model whose handle it runs on, nx, ny, ns, h)
SENSORS = {
    "range_heading": ("car_obs", 3, 2, 0, _range_heading),
    "beacons2": ("car_obs", 3, 2, 4, _beacons2),
    "encoder": ("acrobot", 4, 3, 0, _encoder),
    "mix12": ("synth12", 12, 13, 2, _mix12),
    "wide12": ("synth12", 12, 64, 0, _wide12),
    "mix32": ("synth32", 32, 33, 1, _mix32),
}
BY_MODEL = {"car_obs": ("range_heading", "beacons2"), "acrobot": ("encoder",), "synth12": ("mix12", "wide12"), "synth32": ("mix32",)}
# Further tables of the same rows (tests/sensor_nl_sizes.py) are looked up by the same functions once registered. A row may carry a
# sixth field, a dict: "sym", what h is traced over in place of the sympy module; "h" and "jacobian", (x, s) -> fp64 arrays from
# another high-precision method, in place of the numpy evaluation and the complex step (a real x only).
_TABLES = [SENSORS]


def register(table):
    assert all(k not in t for t in _TABLES for k in table if t is not table)
    if not any(t is table for t in _TABLES):
        _TABLES.append(table)


def entry(key):
    for t in _TABLES:
        if key in t:
            return t[key]
    raise KeyError(key)


def _other(key):
    e = entry(key)
    return e[5] if len(e) > 5 else {}


def dims(key):
    return entry(key)[1:4]


def symbolic(key):
    """h(x, s) on sympy symbols, as codegen.generate_sensor_source / api.compile_sensor take it"""
    import sympy as sp
    f, m = entry(key)[4], _other(key).get("sym", sp)
    return lambda x, s: f(x, s, m)


_COMPILED = {}


def compiled(pkg, key):
    """the registered name of the sensor's module, compiled (or found in the module cache) once per process"""
    if key not in _COMPILED:
        nx, _, ns = dims(key)
        _COMPILED[key] = pkg.compile_sensor("nl_" + key, symbolic(key), nx, ns)[0]
    return _COMPILED[key]


# A sensor written by hand in C that leans on the contract "dydx arrives zeroed": it ACCUMULATES into dydx and reads a partial it never
# wrote back into y. acrobot, nx = 4, ny = 2, ns = 0: y_0 = x_0 + dydx[3] (= x_0), y_1 = x_1 x_2 with its partials added in two halves.
READBACK_SOURCE = """
ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s) {
    if (j == 0) {
        dydx[0] += 1.0;
        *y = x[0] + dydx[3];
    } else {
        dydx[1] += 0.5 * x[2]; dydx[1] += 0.5 * x[2];
        dydx[2] += x[1];
        *y = x[1] * x[2];
    }
}
"""


def compiled_readback(pkg):
    if "readback" not in _COMPILED:
        _COMPILED["readback"] = pkg.compile_sensor_source("nl_readback", 4, 2, 0, READBACK_SOURCE)[0]
    return _COMPILED["readback"]


def s_shared(key):
    """[ns]: beacon positions away from the car's paths; gains of order one"""
    ns = dims(key)[2]
    return {"beacons2": np.array([3.0, 2.0, -2.0, 3.0])}.get(key, 0.5 + 0.25 * np.cos(1.0 + np.arange(ns)))


def s_instances(key, B):
    """[B, ns]: instance b's parameters off by up to a tenth"""
    s = s_shared(key)
    return s[None, :] * (1.0 + 0.1 * np.arange(B)[:, None] / B) + 0.05 * np.sin(np.arange(B)[:, None] + np.arange(len(s))[None, :])


def r(ny):
    return S.r(ny)


def sigma_y(ny):
    return S.sigma_y(ny)


def readings(key, states, s):
    """y [B, ny] = h(the states E.start gives as its measurement) + a fixed pattern; s [ns] or [B, ns]"""
    B = states.shape[0]
    ny = dims(key)[1]
    y = np.stack([h(key, states[b], s if np.ndim(s) == 1 else s[b]) for b in range(B)])
    return y + 0.01 * np.sin(0.3 + np.arange(B)[:, None] + 2.0 * np.arange(ny)[None, :])


# ------------------------------------------------------------------------------------------------------------- the operation
def h(key, x, s):
    """y [ny] of one instance (real or complex x)"""
    if "h" in _other(key):
        return _other(key)["h"](np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64))
    with np.errstate(all="ignore"):
        return np.array(entry(key)[4](np.asarray(x), np.asarray(s, dtype=np.float64), np), dtype=np.asarray(x).dtype)


def jacobian(key, x, s):
    """H [ny, nx] by the complex step"""
    if "jacobian" in _other(key):
        return _other(key)["jacobian"](np.asarray(x, dtype=np.float64), np.asarray(s, dtype=np.float64))
    n = len(x)
    H = np.zeros((dims(key)[1], n))
    for k in range(n):
        z = np.array(x, dtype=np.complex128)
        z[k] += 1j * STEP
        H[:, k] = np.imag(h(key, z, s)) / STEP
    return H


def linearise(key, x_lin, s, x_prior=None):
    """one instance -> (H [ny, nx], ŷ [ny])"""
    x_lin = np.asarray(x_lin, dtype=np.float64)
    H, yhat = jacobian(key, x_lin, s), h(key, x_lin, s).astype(np.float64)
    if x_prior is not None:
        with np.errstate(all="ignore"):
            for j in range(H.shape[0]):
                acc = yhat[j]
                for k in range(H.shape[1]):
                    acc = acc + H[j, k] * (x_prior[k] - x_lin[k])
                yhat[j] = acc
    return H, yhat


def measure(key, x, s, sigma, z, step):
    """y [ny] of one instance; z [>= 9, > step, 16] of this instance (None allowed when sigma is None)"""
    y = h(key, np.asarray(x, dtype=np.float64), s).astype(np.float64)
    for j in range(len(y)):
        if sigma is not None and sigma[j] != 0.0:
            y[j] = y[j] + sigma[j] * z[IO.MEASURE_ROW0 + j // 16, step, j % 16]
    return y


def update(key, xhat, P, y, s, rr, iterations=1):
    """one instance -> dict(xhat, P, innovation, nis, first_bad) of the last iteration"""
    x0, P0 = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64)
    xi, out = x0, None
    for i in range(iterations):
        H, yhat = linearise(key, xi, s, x0 if i else None)
        out = S.update_sequential(x0, P0, y, H, rr, yhat)
        xi = out["xhat"]
    return out


def iekf_textbook(key, xhat, P, y, s, rr, iterations):
    """the Gauss-Newton iterated extended Kalman filter -> dict(xhat, P)"""
    import scipy.linalg
    x0, P0 = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64)
    Rm, n = np.diag(np.asarray(rr, dtype=np.float64)), len(x0)
    xi = x0.copy()
    for _ in range(iterations):
        Hi = jacobian(key, xi, s)
        cho = scipy.linalg.cho_factor(Hi @ P0 @ Hi.T + Rm, lower=True)
        Kg = scipy.linalg.cho_solve(cho, Hi @ P0).T
        xi = x0 + Kg @ (np.asarray(y) - h(key, xi, s) - Hi @ (x0 - xi))
    A = np.eye(n) - Kg @ Hi
    return dict(xhat=xi, P=A @ P0 @ A.T + Kg @ Rm @ Kg.T)


# ------------------------------------------------------------------------------------------------------------- "it filters"
# car_obs with ranges to two beacons and NO heading reading, a fixed plan (the nominal actions, no feedback, no re-solve). The prior
# is wide and off by decimetres, so the first linearisation is poor: that is where iterating pays.
FILTER = dict(name="car_obs", key="beacons2", B=70, periods=4, k=2, seed=SEED, sigma=0.01, q=1.0e-8)


def filter_inputs(x0):
    """(s [4], sigma_y [2], r [2], q [3], x̂_0 [B, 3], P0 [B, 3, 3]) from the plant's first states x0 [B, 3]"""
    B = x0.shape[0]
    sy = np.full(2, FILTER["sigma"])
    xh = x0 + np.array([0.4, -0.3, 0.2])[None, :] * (1.0 + 0.2 * np.cos(np.arange(B)))[:, None]
    return s_shared("beacons2"), sy, sy ** 2, np.full(3, FILTER["q"]), xh, np.stack([np.diag([0.5, 0.5, 0.2])] * B)


def filter_run(ub, w, x0, z, iterations):
    """the yardstick's run -> dict(x, xhat, open: prediction alone from x̂_0), each [B, periods, 3]"""
    F = FILTER
    s, sy, rr, qq, xh0, P0 = filter_inputs(x0)
    f = R.dynamics(F["name"])
    B, k = x0.shape[0], F["k"]
    xs, hs, os_ = [], [], []
    for b in range(B):
        xb = np.zeros((ub.shape[1] + 1, 3))
        wb = None if w is None else w[b]
        x, xh, P, xo = x0[b].copy(), xh0[b].copy(), P0[b].copy(), xh0[b].copy()
        rx, rh, ro = [], [], []
        for p in range(F["periods"]):
            x = IO.plant_step(f, xb, ub[b], None, wb, x, k)["x"][-1]
            y = measure(F["key"], x, s, sy, z[b], (p + 1) * k)
            xh, P = E.predict(F["name"], xb, ub[b], None, wb, xh, P, k, q=qq)
            u = update(F["key"], xh, P, y, s, rr, iterations)
            xh, P = u["xhat"], u["P"]
            xo = IO.plant_step(f, xb, ub[b], None, wb, xo, k)["x"][-1]
            rx.append(x); rh.append(xh); ro.append(xo)
        xs.append(rx); hs.append(rh); os_.append(ro)
    return dict(x=np.array(xs), xhat=np.array(hs), open=np.array(os_))


def filter_scores(run_):
    """mean squared position errors: (the estimate, prediction alone)"""
    e = lambda a: float(((a[..., :2] - run_["x"][..., :2]) ** 2).mean())
    return e(run_["xhat"]), e(run_["open"])
