"""The yardstick of the extended Kalman filter (tests/test_estimator_ref.py, tests/test_gpu_estimator.py): ilqr_estimate_predict,
ilqr_estimate_update and the two loop orders of ilqr_mpc_run_est as include/ilqr_hip.h defines them, in plain fp64 numpy over
plant_ref.dynamics(name) and plant_io_ref.plant_step —

    predict, per step:  u_i = the action plant_io_ref.plant_step applies from x̂;  F = ∂f/∂x (x̂, u_i, w_i);  x̂ ← f(x̂, u_i, w_i);
                        P ← F P Fᵀ + diag(q), the lower triangle mirrored
    update, per measured j in increasing order:  ν = y_j − x̂_j, s = P_jj + r_j, g = P[:, j] / s, x̂ ← x̂ + g ν,
                        P_ab ← P_ab − g_a P_jb (a >= b, mirrored), nis += ν² / s

THE JACOBIAN is the complex-step derivative of the numpy dynamics, Im f(x + i h e_j) / h at h = 1e-30: exact to rounding, and from
nothing the device runs (the device differentiates its generated model symbolically). The synth models' callables take complex
states as they are; car and acrobot are written with math.sin / math.cos in mpc_ref / plant_ref, so the same formulas stand here
once more over numpy's functions (`_car_midpoint`, `_acrobot_midpoint`), and tests/test_estimator_ref.py holds them to the real
callables on real states.

`update_batch` is the textbook form — K = P Hᵀ S⁻¹ with S = H P Hᵀ + R through scipy.linalg, Joseph-form covariance — which the
sequential form equals because R is diagonal. `run` extends plant_io_ref.run by the filter. The inputs of the GPU test live here too."""
import numpy as np
import scipy.linalg

import mpc_ref as M
import plant_io_ref as IO
import plant_ref as R

MODELS = IO.MODELS
STEP = 1.0e-30
SEED = R.SEED


# ------------------------------------------------------------------------------------------------------------- the Jacobian
def _car_midpoint(x, u, h=0.1):
    c = lambda z: np.array([u[0] * np.cos(z[2]), u[0] * np.sin(z[2]), u[1] + 0.0 * z[2]])
    k1 = c(x)
    return x + h * c(x + 0.5 * h * k1)


def _acrobot_c(x, u):
    m1, i1, l1, lc1, m2, i2, lc2, g, f1, f2 = 1.0, 0.33, 1.0, 0.5, 1.0, 0.33, 0.5, 9.81, 0.1, 0.1
    a = i1 + i2 + m2 * l1 * l1 + 2.0 * m2 * l1 * lc2 * np.cos(x[1])
    b = i2 + m2 * l1 * lc2 * np.cos(x[1])
    c = i2
    s = 1.0 / (a * c - b * b)
    t0 = -1.0 * m1 * g * lc1 * np.sin(x[0]) - m2 * g * (l1 * np.sin(x[0]) + lc2 * np.sin(x[0] + x[1]))
    t1 = -1.0 * m2 * g * lc2 * np.sin(x[0] + x[1])
    c00 = -2.0 * m2 * l1 * lc2 * np.sin(x[1]) * x[3]
    c01 = -1.0 * m2 * l1 * lc2 * np.sin(x[1]) * x[3]
    c10 = m2 * l1 * lc2 * np.sin(x[1]) * x[2]
    r0 = -1.0 * (c00 * x[2] + c01 * x[3]) + t0 - f1 * x[2]
    r1 = -1.0 * (c10 * x[2]) + t1 + u[0] - f2 * x[3]
    return np.array([x[2], x[3], s * c * r0 + s * (-b) * r1, s * (-b) * r0 + s * a * r1])


def _acrobot_midpoint(x, u, h=0.1):
    k1 = _acrobot_c(x, u)
    return x + h * _acrobot_c(x + 0.5 * h * k1, u)


def dynamics_complex(name):
    """f(x, u, w, t) of the model that takes a complex state"""
    if name == "car_obs":
        return lambda x, u, w, t: _car_midpoint(x, u)
    if name == "acrobot":
        return lambda x, u, w, t: _acrobot_midpoint(x, u)
    return R.dynamics(name)


def jacobian(name, x, u, w, t=0):
    """F [n, n], F[r, c] = ∂f_r / ∂x_c at (x, u, w)"""
    f, n = dynamics_complex(name), len(x)
    F = np.zeros((n, n))
    for c in range(n):
        z = np.array(x, dtype=np.complex128)
        z[c] += 1j * STEP
        F[:, c] = np.imag(np.asarray(f(z, np.asarray(u, dtype=np.float64), w, t))) / STEP
    return F


def mirror(P):
    """the lower triangle, copied to its mirror"""
    L = np.tril(P)
    return L + np.tril(P, -1).T


# ------------------------------------------------------------------------------------------------------------- the operation
def predict(name, xb, ub, K, w, xhat, P, steps, feedback=False, u_min=None, u_max=None, q=None, trace=None):
    """one instance -> (x̂ [n], P [n, n]); trace: a list that receives P after every step"""
    f = R.dynamics(name)
    x, P = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64)
    n = len(x)
    qv = np.zeros(n) if q is None else np.asarray(q, dtype=np.float64)
    for i in range(steps):
        one = IO.plant_step(f, xb[i:], ub[i:], None if K is None else K[i:], None if w is None else w[i:], x, 1, feedback, u_min=u_min, u_max=u_max)
        wi = M._NONE if w is None else np.array(w[i], dtype=np.float64)
        F = jacobian(name, x, one["u"][0], wi, i)
        x = one["x"][1]
        P = mirror(F @ P @ F.T + np.diag(qv))
        if trace is not None:
            trace.append(P.copy())
    return x, P


def update_sequential(xhat, P, y, r, measured=None, trace=None):
    """one instance -> dict(xhat, P, innovation, nis, first_bad)"""
    x, P = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64)
    n = len(x)
    inn, nis, bad = np.zeros(n), 0.0, -1
    for j in range(n):
        if measured is not None and not measured[j]:
            continue
        nu, s = y[j] - x[j], P[j, j] + r[j]
        if not (np.isfinite(s) and s > 0.0):
            bad = j if bad < 0 else bad
            continue
        row, g = P[j, :].copy(), P[:, j] / s
        x = x + g * nu
        P = mirror(P - np.outer(g, row))
        nis += nu * nu / s
        inn[j] = nu
        if trace is not None:
            trace.append(P.copy())
    return dict(xhat=x, P=P, innovation=inn, nis=nis, first_bad=bad)


def update_batch(xhat, P, y, r, measured=None):
    """the textbook update: K = P Hᵀ S⁻¹, Joseph form -> dict(xhat, P, nis)"""
    x, P = np.array(xhat, dtype=np.float64), np.array(P, dtype=np.float64)
    n = len(x)
    idx = np.arange(n) if measured is None else np.flatnonzero(np.asarray(measured))
    H = np.eye(n)[idx]
    Rm = np.diag(np.asarray(r, dtype=np.float64)[idx])
    nu = np.asarray(y, dtype=np.float64)[idx] - x[idx]
    S = H @ P @ H.T + Rm
    cho = scipy.linalg.cho_factor(S, lower=True)
    Kg = scipy.linalg.cho_solve(cho, H @ P).T
    A = np.eye(n) - Kg @ H
    return dict(xhat=x + Kg @ nu, P=A @ P @ A.T + Kg @ Rm @ Kg.T, nis=float(nu @ scipy.linalg.cho_solve(cho, nu)))


def run(x0, xhat0, P0, periods, k, delay, plant, measure_, predict_, update_, resolve):
    """plant_io_ref.run with the filter: predict_(x̂, P, p) -> (x̂, P) k steps on under the plan in flight; update_(x̂, P, y) -> a dict
    as update_sequential's. -> dict(x, y [periods, ...], xhat, pdiag, nis)"""
    x, xh, P = np.array(x0, dtype=np.float64), np.array(xhat0, dtype=np.float64), np.array(P0, dtype=np.float64)
    xs, ys, hs, ds, ns = [x[None]], [], [], [], []
    for p in range(periods):
        if delay:
            y = measure_(x, p * k)
            u = update_(xh, P, y)
            xh, P = predict_(u["xhat"], u["P"], p)
        seg = plant(x, p)
        x = np.array(seg[-1])
        xs.append(seg[1:])
        if not delay:
            y = measure_(x, (p + 1) * k)
            xh, P = predict_(xh, P, p)
            u = update_(xh, P, y)
            xh, P = u["xhat"], u["P"]
        ys.append(np.array(y)); hs.append(np.array(xh)); ds.append(np.diag(P).copy()); ns.append(u["nis"])
        resolve(xh, p)
    return dict(x=np.concatenate(xs, axis=0), y=np.stack(ys), xhat=np.stack(hs), pdiag=np.stack(ds), nis=np.array(ns), P=P)


# ------------------------------------------------------------------------------------------------- the inputs of the GPU test
def p0(n):
    """P0 = diag"""
    return np.diag(1.0e-2 * (1.0 + np.arange(n) / n))


def q(n):
    """process noise variances; component 0 (measured under both masks) has none"""
    v = 1.0e-4 * (1.0 + np.arange(n) % 3)
    v[0] = 0.0
    return v


def r(n):
    """measurement noise variances, >= 1e-4"""
    return 1.0e-3 * (1.0 + np.arange(n) % 4)


def masks(name, n):
    """(a mask that leaves components unmeasured, the all-measured mask): the positions of car_obs and acrobot, two of three on synth"""
    part = {"car_obs": np.array([1, 1, 0]), "acrobot": np.array([1, 1, 0, 0])}.get(name)
    if part is None:
        part = (np.arange(n) % 3 != 2).astype(np.int64)
    return part.astype(np.int32), np.ones(n, dtype=np.int32)


def start(x, n):
    """(x̂ [B, n], y [B, n]) around the states x: an estimate off by a fixed pattern, a measurement off by another"""
    B = x.shape[0]
    off = 0.02 * np.cos(1.0 + np.arange(B)[:, None] + 2.0 * np.arange(n)[None, :])
    return x + off, x + 0.03 * np.sin(0.5 + 3.0 * np.arange(B)[:, None] + np.arange(n)[None, :])


def p_start(B, n):
    """[B, n, n]: P0, instance b scaled by 1 + b / B and given a symmetric off-diagonal part (positive definite: diagonally dominant)"""
    i = np.arange(n)
    C = 1.0e-3 * np.cos(i[:, None] + i[None, :]) / n
    np.fill_diagonal(C, 0.0)
    return np.stack([(1.0 + b / B) * (p0(n) + C) for b in range(B)])


# "it filters": acrobot, positions measured, a fixed plan (the nominal actions, no feedback, no re-solve)
FILTER = dict(name="acrobot", B=70, periods=5, k=2, seed=SEED, sigma_pos=0.05, q=1.0e-8, p0=1.0e-2)


def filter_inputs(x0):
    """(sigma_y, r, q, measured, x̂_0, P0) of the filtering test from the plant's first states x0 [B, 4]"""
    B = x0.shape[0]
    sy = np.array([FILTER["sigma_pos"], FILTER["sigma_pos"], 0.0, 0.0])
    rr = np.array([sy[0] ** 2, sy[1] ** 2, 1.0, 1.0])
    xh = x0 + np.array([0.05, -0.05, 0.3, -0.3])[None, :] * (1.0 + 0.1 * np.cos(np.arange(B)))[:, None]
    return sy, rr, np.full(4, FILTER["q"]), np.array([1, 1, 0, 0], dtype=np.int32), xh, np.stack([np.diag([FILTER["p0"], FILTER["p0"], 0.1, 0.1])] * B)


def filter_run(ub, x0, z):
    """the yardstick's run of the filtering test: plant step / measure / predict / update per period under the fixed plan ū [B, T-1, m]
    — no shift between the periods, so every period applies the head ū_0 .. ū_{k−1} of the plan, as the device calls do.
    -> dict(x, y, xhat [B, periods, 4], open [B, periods, 4]: prediction alone from x̂_0)"""
    F = FILTER
    sy, rr, qq, mk, xh0, P0 = filter_inputs(x0)
    f = R.dynamics(F["name"])
    B, k = x0.shape[0], F["k"]
    xs, ys, hs, os_ = [], [], [], []
    for b in range(B):
        xb = np.zeros((ub.shape[1] + 1, 4))
        x, xh, P, xo = x0[b].copy(), xh0[b].copy(), P0[b].copy(), xh0[b].copy()
        rx, ry, rh, ro = [], [], [], []
        for p in range(F["periods"]):
            sl = slice(0, None)
            x = IO.plant_step(f, xb[sl], ub[b][sl], None, None, x, k)["x"][-1]
            y = IO.measure(x, sy, z[b], (p + 1) * k)
            xh, P = predict(F["name"], xb[sl], ub[b][sl], None, None, xh, P, k, q=qq)
            u = update_sequential(xh, P, y, rr, mk)
            xh, P = u["xhat"], u["P"]
            xo = IO.plant_step(f, xb[sl], ub[b][sl], None, None, xo, k)["x"][-1]
            rx.append(x); ry.append(y); rh.append(xh); ro.append(xo)
        xs.append(rx); ys.append(ry); hs.append(rh); os_.append(ro)
    return dict(x=np.array(xs), y=np.array(ys), xhat=np.array(hs), open=np.array(os_))


def filter_scores(run_):
    """(mse of x̂ on the positions, mse of y on the positions, mse of x̂ on the velocities, mse of prediction alone on the velocities)"""
    e = lambda a, cols: float(((a[..., cols] - run_["x"][..., cols]) ** 2).mean())
    return e(run_["xhat"], [0, 1]), e(run_["y"], [0, 1]), e(run_["xhat"], [2, 3]), e(run_["open"], [2, 3])
