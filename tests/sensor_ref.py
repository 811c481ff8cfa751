"""The yardstick of the linear sensor y = H x + v, v ~ N(0, diag(r)) (tests/test_sensor_ref.py, tests/test_gpu_sensor.py):
ilqr_estimate_update_linear, ilqr_plant_measure_linear and the loop of ilqr_mpc_run_sensor as include/ilqr_hip.h defines them, in
plain fp64 numpy —

    update, per row j in increasing order:  d = P h_jᵀ, s = h_j·d + r_j, ν = (y_j − c_j) − h_j·x̂, g = d / s, x̂ ← x̂ + g ν,
                        P_ab ← P_ab − g_a d_b (a >= b, mirrored), nis += ν² / s;  c_j = 0, or ŷ_j − h_j·x̂₀ with ŷ given
    measure:            y_j = Σ_k H_jk x_k + sigma_y[j] · z[5 + j // 16, step, j % 16]

`update_batch` is the textbook form — K = P Hᵀ S⁻¹ with S = H P Hᵀ + R through scipy.linalg (LAPACK), Joseph-form covariance — which
the sequential form equals because R is diagonal. The time update, the loop orders and the states, estimates and covariances the
tests start from are tests/estimator_ref.py's (predict, run, start, p_start, q). The sensors of the GPU test live here."""
import numpy as np
import scipy.linalg

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R

MODELS = E.MODELS
SEED = R.SEED
# ny per model: fewer than nx, nx + 1 (redundant), and where the large kernel has another edge — 64, the bound (synth12), 33, past
# lane 32 and one tile (synth32)
NY = {"car_obs": (2, 4), "acrobot": (2, 5), "synth12": (2, 13, 64), "synth32": (2, 33)}


# ------------------------------------------------------------------------------------------------------------- the operation
def update_sequential(xhat, P, y, H, r, yhat=None):
    """one instance -> dict(xhat, P, innovation [ny], nis, first_bad)"""
    x, P, H = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64), np.asarray(H, dtype=np.float64)
    ny = H.shape[0]
    c = np.zeros(ny) if yhat is None else np.asarray(yhat, dtype=np.float64) - H @ x
    inn, nis, bad = np.zeros(ny), 0.0, -1
    with np.errstate(all="ignore"):
        for j in range(ny):
            h = H[j]
            d = P @ h
            s = h @ d + r[j]
            nu = (y[j] - c[j]) - h @ x
            if not (np.isfinite(s) and s > 0.0):
                bad = j if bad < 0 else bad
                continue
            g = d / s
            x = x + g * nu
            P = E.mirror(P - np.outer(g, d))
            nis += nu * nu / s
            inn[j] = nu
    return dict(xhat=x, P=P, innovation=inn, nis=nis, first_bad=bad)


def update_batch(xhat, P, y, H, r, yhat=None):
    """the textbook update: K = P Hᵀ S⁻¹, Joseph form -> dict(xhat, P, nis)"""
    x, P, H = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64), np.asarray(H, dtype=np.float64)
    n = len(x)
    Rm = np.diag(np.asarray(r, dtype=np.float64))
    nu = np.asarray(y, dtype=np.float64) - (H @ x if yhat is None else np.asarray(yhat, dtype=np.float64))
    S = H @ P @ H.T + Rm
    cho = scipy.linalg.cho_factor(S, lower=True)
    Kg = scipy.linalg.cho_solve(cho, H @ P).T
    A = np.eye(n) - Kg @ H
    return dict(xhat=x + Kg @ nu, P=A @ P @ A.T + Kg @ Rm @ Kg.T, nis=float(nu @ scipy.linalg.cho_solve(cho, nu)))


def measure(x, H, sigma_y, z, step):
    """y [ny] of one instance; z [>= 9, > step, 16] of this instance (None allowed when sigma_y is None)"""
    H = np.asarray(H, dtype=np.float64)
    y = np.zeros(H.shape[0])
    for j in range(H.shape[0]):
        acc = 0.0
        for k in range(H.shape[1]):
            acc += H[j, k] * x[k]
        if sigma_y is not None and sigma_y[j] != 0.0:
            acc = acc + sigma_y[j] * z[IO.MEASURE_ROW0 + j // 16, step, j % 16]
        y[j] = acc
    return y


# ------------------------------------------------------------------------------------------------- the inputs of the GPU test
def sensor(n, ny):
    """H [ny, n]: row j reads component j mod n and a little of every other one; full column rank once ny >= n"""
    j, k = np.arange(ny)[:, None], np.arange(n)[None, :]
    return np.eye(n)[np.arange(ny) % n] + 0.25 * np.cos(1.0 + 0.7 * j + 1.3 * k)


def sensors(n, ny, B):
    """[B, ny, n]: one sensor per instance, instance b's gains off by up to a tenth"""
    j, k = np.arange(ny)[:, None], np.arange(n)[None, :]
    return np.stack([sensor(n, ny) * (1.0 + 0.1 * b / B) + 0.05 * np.sin(b + 0.3 * j + 0.9 * k) for b in range(B)])


def r(ny):
    """measurement noise variances, >= 1e-3"""
    return 1.0e-3 * (1.0 + np.arange(ny) % 4)


def sigma_y(ny):
    """a different size per output, one of them zero"""
    s = 5.0e-3 * (2.0 + np.arange(ny) % 7) / 7.0
    s[(ny // 2 + 1) % ny] = 0.0
    return s


def readings(H, states):
    """y [B, ny] = H_b (the states E.start gives as its measurement) + a fixed pattern; H [ny, n] or [B, ny, n]"""
    B = states.shape[0]
    Hb = np.broadcast_to(H, (B,) + H.shape[-2:])
    ny = Hb.shape[1]
    return np.einsum("bjk,bk->bj", Hb, states) + 0.01 * np.sin(0.3 + np.arange(B)[:, None] + 2.0 * np.arange(ny)[None, :])


def some_yhat(y):
    """an arbitrary linearisation output ŷ [B, ny] near y (the arithmetic does not ask where it comes from)"""
    B, ny = y.shape
    return y - 0.02 * np.cos(0.7 + 2.0 * np.arange(B)[:, None] + np.arange(ny)[None, :])


def selection(mask):
    """the rows of the identity a 0/1 mask selects"""
    return np.eye(len(mask))[np.flatnonzero(np.asarray(mask))]


def range_sensor(xhat, x_true):
    """car_obs (px, py, θ): the range to the origin and the heading, linearised on the host at x̂ [B, 3]
    -> (H [B, 2, 3] = ∂h/∂x at x̂, ŷ [B, 2] = h(x̂), y [B, 2] = h(x_true) + a fixed pattern, r [2])"""
    B = xhat.shape[0]
    rho = np.hypot(xhat[:, 0], xhat[:, 1])
    H = np.zeros((B, 2, 3))
    H[:, 0, 0], H[:, 0, 1], H[:, 1, 2] = xhat[:, 0] / rho, xhat[:, 1] / rho, 1.0
    yhat = np.stack([rho, xhat[:, 2]], axis=1)
    y = np.stack([np.hypot(x_true[:, 0], x_true[:, 1]), x_true[:, 2]], axis=1) + 0.01 * np.sin(1.0 + np.arange(B))[:, None]
    return H, yhat, y, np.array([1.0e-3, 2.0e-3])


# "it filters": acrobot, the first encoder reads q1 and the second the absolute link angle q1 + q2; a fixed plan (the nominal
# actions, no feedback, no re-solve)
FILTER = dict(name="acrobot", B=70, periods=8, k=2, seed=SEED, sigma=0.02, q=1.0e-8)
FILTER_H = np.array([[1.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]])


def filter_inputs(x0):
    """(sigma_y [2], r [2], q [4], x̂_0, P0) of the filtering test from the plant's first states x0 [B, 4]"""
    _, _, _, _, xh, P0 = E.filter_inputs(x0)
    sy = np.full(2, FILTER["sigma"])
    return sy, sy ** 2, np.full(4, FILTER["q"]), xh, P0


def raw_angles(y):
    """what the two encoders say about (q1, q2) without a filter: y_0 and y_1 − y_0"""
    return np.stack([y[..., 0], y[..., 1] - y[..., 0]], axis=-1)


def filter_run(ub, x0, z):
    """the yardstick's run of the filtering test, as estimator_ref.filter_run with the two-row sensor
    -> dict(x [B, periods, 4], y [B, periods, 2], xhat, open: prediction alone from x̂_0)"""
    F = FILTER
    sy, rr, qq, xh0, P0 = filter_inputs(x0)
    f = R.dynamics(F["name"])
    B, k = x0.shape[0], F["k"]
    xs, ys, hs, os_ = [], [], [], []
    for b in range(B):
        xb = np.zeros((ub.shape[1] + 1, 4))
        x, xh, P, xo = x0[b].copy(), xh0[b].copy(), P0[b].copy(), xh0[b].copy()
        rx, ry, rh, ro = [], [], [], []
        for p in range(F["periods"]):
            x = IO.plant_step(f, xb, ub[b], None, None, x, k)["x"][-1]
            y = measure(x, FILTER_H, sy, z[b], (p + 1) * k)
            xh, P = E.predict(F["name"], xb, ub[b], None, None, xh, P, k, q=qq)
            u = update_sequential(xh, P, y, FILTER_H, rr)
            xh, P = u["xhat"], u["P"]
            xo = IO.plant_step(f, xb, ub[b], None, None, xo, k)["x"][-1]
            rx.append(x); ry.append(y); rh.append(xh); ro.append(xo)
        xs.append(rx); ys.append(ry); hs.append(rh); os_.append(ro)
    return dict(x=np.array(xs), y=np.array(ys), xhat=np.array(hs), open=np.array(os_))


def filter_scores(run_):
    """mean squared errors: (x̂ on q1, the raw sensor on q1, x̂ on q2, the raw sensor on q2, x̂ on the velocities, prediction alone on
    the velocities)"""
    e = lambda a, cols: float(((a[..., cols] - run_["x"][..., cols]) ** 2).mean())
    raw = raw_angles(run_["y"])
    return (e(run_["xhat"], [0]), float(((raw[..., 0] - run_["x"][..., 0]) ** 2).mean()), e(run_["xhat"], [1]),
            float(((raw[..., 1] - run_["x"][..., 1]) ** 2).mean()), e(run_["xhat"], [2, 3]), e(run_["open"], [2, 3]))
