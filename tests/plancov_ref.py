"""The yardstick of the plan covariance (tests/test_plancov_ref.py, tests/test_gpu_plancov.py, tests/test_gpu_plancov_sizes.py):
ilqr_plan_covariance as include/ilqr_hip.h defines it, in plain fp64 numpy over estimator_ref.jacobian and its counterpart in u —

    A = ∂f/∂x, Bm = ∂f/∂u at (x̄_t, ū_t, θ_t);  Φ = A + Bm K_t (feedback) or A;  udiag_t[r] = K_t[r] Σ_t K_t[r]ᵀ (feedback) or 0;
    Σ_{t+1} = Φ Σ_t Φᵀ + diag(q), the lower triangle mirrored;  Σ_0 = the lower triangle of P0, mirrored

THE JACOBIANS are complex-step derivatives of the numpy dynamics (estimator_ref.dynamics_complex), Im f(x, u + i h e_j) / h at
h = 1e-30 for the action: exact to rounding, and from nothing the device runs. tests/test_plancov_ref.py holds the action Jacobian to
central differences of the real callables.

Form (a), `recursion`, is the recursion above. Form (b), `transition_form`, is Σ_t = Ψ_{t,0} Σ_0 Ψ_{t,0}ᵀ + Σ_{s<t} Ψ_{t,s+1} diag(q)
Ψ_{t,s+1}ᵀ with Ψ_{t,s} = Φ_{t−1} ··· Φ_s; its action variances go through scipy: Σ_i λ_i (v_iᵀ K_t[r]ᵀ)² over the
eigenpairs of Σ_t (scipy.linalg.eigh; a Cholesky factor does not exist where the closed loop has contracted Σ_t to rounding).
The two agree within a tenth of TOL_XU = 1e-10 (asserted by tests/test_plancov_ref.py), so the GPU bound TOL_XU is an honest one.

Arrays are one instance's: xb [T, n], ub [T-1, m], K [T-1, n, m] (as get_policy returns it: K[t, j, r] = K_t(r, j)), w None or [T, nw].

THE SAMPLED COVARIANCE (`sampled`, test 5 of tests/test_gpu_plancov.py): with q = 0 and P0 = L Lᵀ, the 2 n closed-loop rollouts from
x̄_0 ± ε L e_j give d_j(t) = (x_t⁺ − x_t⁻) / (2 ε), Σ̂_t = Σ_j d_j d_jᵀ, and the same for the actions; Σ̂_t is Σ_t up to the second-order
remainder of the central difference, O((ε ‖L‖)²), and its rounding, O(1e-16 / (ε ‖L‖)). Measured entirely in numpy
(plant_ref.plant_step's nonlinear rollouts against form (a), tests/test_plancov_ref.py, which asserts it), on car_obs, acrobot and
synth12 at T = 11, three instances, under LQR gains of the plan (`lqr_gains`), as max |Σ̂ − Σ| / max |Σ| over the horizon:

    ε = FD_EPS = 1e-3;  measured: car_obs 2.5e-12, acrobot 2.89e-8, synth12 9.7e-11;  FD_MEASURED = 2.9e-8 (<= 1e-6, as the measurement
    was asked to be);  FD_BOUND = 10 · FD_MEASURED = 2.9e-7

FD_BOUND is the bar of the GPU test: the margin covers the device's different rounding of the same remainder and its own gains."""
import numpy as np
import scipy.linalg

import estimator_ref as E
import plant_ref as R

STEP = E.STEP
FD_EPS = 1.0e-3
FD_MEASURED = 2.9e-8          # the worst value seen on the CPU (acrobot 2.89e-8, car_obs 2.5e-12, synth12 9.7e-11), rounded up;
                              # tests/test_plancov_ref.py prints the three and holds them to it
FD_BOUND = 10.0 * FD_MEASURED


# ------------------------------------------------------------------------------------------------------------- the Jacobians
def action_jacobian(name, x, u, w, t=0):
    """Bm [n, m], Bm[r, c] = ∂f_r / ∂u_c at (x, u, w)"""
    f, m = E.dynamics_complex(name), len(u)
    xc = np.array(x, dtype=np.complex128)
    cols = []
    for c in range(m):
        z = np.array(u, dtype=np.complex128)
        z[c] += 1j * STEP
        cols.append(np.imag(np.asarray(f(xc, z, w, t))) / STEP)
    return np.stack(cols, axis=1)


def _w(w, t):
    return np.zeros(0) if w is None else np.array(w[t], dtype=np.float64)


def transitions(name, xb, ub, K, w, steps, feedback):
    """[Φ_0 .. Φ_{steps−1}] and [K_0 .. ] as m x n matrices (None without feedback: K is not read)"""
    Phi, Ks = [], []
    for t in range(steps):
        A = E.jacobian(name, xb[t], ub[t], _w(w, t), t)
        if feedback:
            Kt = np.asarray(K[t], dtype=np.float64).T
            Phi.append(A + action_jacobian(name, xb[t], ub[t], _w(w, t), t) @ Kt)
            Ks.append(Kt)
        else:
            Phi.append(A)
            Ks.append(None)
    return Phi, Ks


# ------------------------------------------------------------------------------------------------------------- form (a)
def recursion(name, xb, ub, K, w, P0, steps, feedback=True, q=None):
    """one instance -> dict(sigma [S+1, n, n], sdiag [S+1, n], udiag [S, m], P [n, n], first_nonfinite)"""
    n, m = xb.shape[1], ub.shape[1]
    qv = np.zeros(n) if q is None else np.asarray(q, dtype=np.float64)
    Phi, Ks = transitions(name, xb, ub, K, w, steps, feedback)
    S = E.mirror(np.array(P0, dtype=np.float64))
    sig, ud = [S], []
    for t in range(steps):
        ud.append(np.einsum("ra,ab,rb->r", Ks[t], S, Ks[t]) if feedback else np.zeros(m))
        S = E.mirror(Phi[t] @ S @ Phi[t].T + np.diag(qv))
        sig.append(S)
    sig = np.stack(sig)
    sd = np.diagonal(sig, axis1=1, axis2=2).copy()
    bad = ~np.isfinite(sd).all(axis=1)
    return dict(sigma=sig, sdiag=sd, udiag=np.stack(ud), P=sig[-1], first_nonfinite=int(np.argmax(bad)) if bad.any() else -1)


# ------------------------------------------------------------------------------------------------------------- form (b)
def transition_form(name, xb, ub, K, w, P0, steps, feedback=True, q=None):
    """the same through the transition matrices -> dict(sigma, sdiag, udiag)"""
    n, m = xb.shape[1], ub.shape[1]
    Q = np.diag(np.zeros(n) if q is None else np.asarray(q, dtype=np.float64))
    Phi, Ks = transitions(name, xb, ub, K, w, steps, feedback)
    S0 = E.mirror(np.array(P0, dtype=np.float64))
    sig = []
    for t in range(steps + 1):
        psi = [np.eye(n)]                     # psi[i] = Ψ_{t, t−i}
        for s in range(t - 1, -1, -1):
            psi.append(psi[-1] @ Phi[s])
        St = psi[t] @ S0 @ psi[t].T
        for s in range(t):
            St = St + psi[t - s - 1] @ Q @ psi[t - s - 1].T
        sig.append(0.5 * (St + St.T))
    ud = []
    for t in range(steps):
        if feedback:
            ev, V = scipy.linalg.eigh(sig[t])
            ud.append((ev[:, None] * scipy.linalg.blas.dgemm(1.0, V, Ks[t], trans_a=True, trans_b=True) ** 2).sum(axis=0))
        else:
            ud.append(np.zeros(m))
    sig = np.stack(sig)
    return dict(sigma=sig, sdiag=np.diagonal(sig, axis1=1, axis2=2).copy(), udiag=np.stack(ud))


# ------------------------------------------------------------------------------------------------- the sampled covariance
def sample_starts(x0, P0, eps=FD_EPS):
    """[2 n, n]: x̄_0 + ε L e_j (rows 0 .. n−1) and x̄_0 − ε L e_j (rows n .. 2n−1), P0 = L Lᵀ"""
    L = np.linalg.cholesky(E.mirror(np.array(P0, dtype=np.float64)))
    return np.concatenate([x0[None, :] + eps * L.T, x0[None, :] - eps * L.T])


def sampled(xs, us, eps=FD_EPS):
    """the rollouts xs [2 n, T, n], us [2 n, T−1, m] of sample_starts -> (Σ̂ [T, n, n], the actions' variances [T−1, m])"""
    n = xs.shape[0] // 2
    dx, du = (xs[:n] - xs[n:]) / (2.0 * eps), (us[:n] - us[n:]) / (2.0 * eps)
    return np.einsum("jta,jtb->tab", dx, dx), (du * du).sum(axis=0)


def rel_cov(a, b):
    """max |a − b| relative to the largest reference entry"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def sampled_against_recursion(name, xb, ub, K, w, P0, eps=FD_EPS):
    """the comparison of test 5 entirely in numpy: plant_ref.plant_step's closed-loop rollouts against form (a) -> (state, action)"""
    f, N = R.dynamics(name), ub.shape[0]
    runs = [R.plant_step(f, xb, ub, K, w, x, N, True) for x in sample_starts(xb[0], P0, eps)]
    Sh, Uh = sampled(np.stack([r["x"] for r in runs]), np.stack([r["u"] for r in runs]), eps)
    ref = recursion(name, xb, ub, K, w, P0, N, True, None)
    return rel_cov(Sh, ref["sigma"]), rel_cov(Uh, ref["udiag"])


# ------------------------------------------------------------------------------------------------- a plan without a device
def nominal(name, x1, ub, w):
    """x̄ [T, n]: the open-loop rollout of ū from x1"""
    return R.plant_step(R.dynamics(name), np.zeros((ub.shape[0] + 1, len(x1))), ub, None, w, x1, ub.shape[0])["x"]


def lqr_gains(name, xb, ub, w, qx=1.0, ru=0.1):
    """K [T-1, n, m] in get_policy's layout: the time-varying LQR gains of the plan's own linearisation (cost qx ‖δx‖² + ru ‖δu‖²) —
    stabilising gains of a realistic size for the CPU tests, which have no solve"""
    N, n, m = ub.shape[0], xb.shape[1], ub.shape[1]
    Pm, out = qx * np.eye(n), [None] * N
    for t in range(N - 1, -1, -1):
        A, Bm = E.jacobian(name, xb[t], ub[t], _w(w, t), t), action_jacobian(name, xb[t], ub[t], _w(w, t), t)
        Kt = -scipy.linalg.solve(ru * np.eye(m) + Bm.T @ Pm @ Bm, Bm.T @ Pm @ A, assume_a="pos")
        Pm = qx * np.eye(n) + A.T @ Pm @ (A + Bm @ Kt)
        Pm = 0.5 * (Pm + Pm.T)
        out[t] = Kt.T
    return np.stack(out)
