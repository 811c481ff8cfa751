"""The yardstick of the plant step (tests/test_plant_ref.py, tests/test_gpu_mpc_loop.py): ilqr_plant_step as include/ilqr_hip.h defines
it, written as plain fp64 numpy loops over callables (x, u, w, t) in the form of tests/mpc_ref.py —

    u_i[r] = ū_i[r]                                                   (no feedback)
    u_i[r] = (ū_i[r] + Σ_j K[i, j, r] · x[j]) − Σ_j K[i, j, r] · x̄_i[j]   (feedback; sums in ascending j: mpc_ref.policy_rollout at α = 0)
    w_i    = the user's columns of w_plant[i] if given, else of θ_i; selector columns are θ_i's
    x      ← f(x, u_i, w_i),  then  x[j] ← x[j] + sigma_x[j] · z[1 + j // 16, step0 + i, j % 16]   where sigma_x[j] != 0

with z one instance's block of ilqr_candidate_noise(seed, first_instance, B, 1 + ceil(nx / 16), step0 + steps, 16).

The dynamics of the built-in models the GPU test runs come from mpc_ref where it has them (car, car_obs, synth12); acrobot and
synth32 are written here from the models' formulas (test/acrobot.jl of the reference), in plain numpy / math,
from nothing the device runs. The inputs of the GPU test live here too, so that the CPU check of the inputs and the GPU test use
the same arrays.

Arrays are one instance's: xb [T, n], ub [T-1, m], K [T-1, n, m] (as get_policy returns it), w None or [T, nw]."""
import math

import numpy as np

import mpc_ref as M
import policy_ref

T = 11
BATCHES = {"car": (3, 70), "car_obs": (3, 70), "acrobot": (3, 70), "synth12": (3, 70), "synth32": (3,)}
STEPS, STEP0S = (1, 3), (0, 5)
SEED = 20261019
# a solve short enough to be quick: the plant step needs a policy, not a converged one
SOLVE = dict(max_iterations=5, max_dual_updates=2)
CONFIG = {"car": "car", "car_obs": "car_obs", "acrobot": "acrobot51", "synth12": "synth12", "synth32": "synth32"}


# ------------------------------------------------------------------------------------------------------------- the operation
def noise_slot(j):
    """(candidate row, column) of ilqr_candidate_noise that state component j draws from: row 0 is zero by contract"""
    return 1 + j // 16, j % 16


def noise_shape(nx, step0, steps):
    """(candidates, steps, nu) to ask ilqr_candidate_noise for"""
    return 1 + (nx + 15) // 16, step0 + steps, 16


def plant_step(f, xb, ub, K, w, x, steps, feedback=False, sigma_x=None, z=None, step0=0, w_plant=None):
    """-> dict(x [steps + 1, n] (row 0 = the input state), u [steps, m], first_nonfinite: −1 or the first i with a non-finite state
    after step i). z: [candidates, >= step0 + steps, 16] of this instance."""
    xb, ub = np.asarray(xb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    n, m = xb.shape[1], ub.shape[1]
    xs, us = np.zeros((steps + 1, n)), np.zeros((steps, m))
    xs[0] = x
    nf = -1
    with np.errstate(all="ignore"):
        for i in range(steps):
            for r in range(m):
                v = ub[i, r]
                if feedback:
                    a1 = 0.0
                    for j in range(n):
                        a1 += K[i, j, r] * xs[i, j]
                    v = v + a1
                    a2 = 0.0
                    for j in range(n):
                        a2 += K[i, j, r] * xb[i, j]
                    v = v - a2
                us[i, r] = v
            wi = M._NONE if w is None else np.array(w[i], dtype=np.float64)
            if w_plant is not None:
                wi[:len(w_plant[i])] = w_plant[i]
            y = np.array(f(xs[i], us[i], wi, i), dtype=np.float64)
            if sigma_x is not None:
                for j in range(n):
                    if sigma_x[j] != 0.0:
                        row, col = noise_slot(j)
                        y[j] = y[j] + sigma_x[j] * z[row, step0 + i, col]
            xs[i + 1] = y
            if nf < 0 and not np.isfinite(y).all():
                nf = i
    return dict(x=xs, u=us, first_nonfinite=nf)


def spread(f, xb, ub, K, w, x, steps, **kw):
    """How far the yardstick's own recursion moves when x moves by one part in 1e15: |Δx|, |Δu| relative to max(1, max |.|)"""
    a = plant_step(f, xb, ub, K, w, x, steps, **kw)
    b = plant_step(f, xb, ub, K, w, np.asarray(x) * (1.0 + 1.0e-15), steps, **kw)
    return max(policy_ref.rel(b["x"], a["x"]), policy_ref.rel(b["u"], a["u"]))


# ----------------------------------------------------------------------------------------------- callables of the built-in models
def _acrobot_c(x, u):
    m1, i1, l1, lc1, m2, i2, lc2, g, f1, f2 = 1.0, 0.33, 1.0, 0.5, 1.0, 0.33, 0.5, 9.81, 0.1, 0.1
    a = i1 + i2 + m2 * l1 * l1 + 2.0 * m2 * l1 * lc2 * math.cos(x[1])
    b = i2 + m2 * l1 * lc2 * math.cos(x[1])
    c = i2
    s = 1.0 / (a * c - b * b)
    t0 = -1.0 * m1 * g * lc1 * math.sin(x[0]) - m2 * g * (l1 * math.sin(x[0]) + lc2 * math.sin(x[0] + x[1]))
    t1 = -1.0 * m2 * g * lc2 * math.sin(x[0] + x[1])
    c00 = -2.0 * m2 * l1 * lc2 * math.sin(x[1]) * x[3]
    c01 = -1.0 * m2 * l1 * lc2 * math.sin(x[1]) * x[3]
    c10 = m2 * l1 * lc2 * math.sin(x[1]) * x[2]
    r0 = -1.0 * (c00 * x[2] + c01 * x[3]) + t0 - f1 * x[2]
    r1 = -1.0 * (c10 * x[2]) + t1 + u[0] - f2 * x[3]
    return (x[2], x[3], s * c * r0 + s * (-b) * r1, s * (-b) * r0 + s * a * r1)


def acrobot_midpoint(x, u, h=0.1):
    if not all(math.isfinite(float(v)) for v in x):
        return np.full(4, math.nan)
    k1 = _acrobot_c(x, u)
    k2 = _acrobot_c([x[i] + 0.5 * h * k1[i] for i in range(4)], u)
    return np.array([x[i] + h * k2[i] for i in range(4)])


def synth_f(n, m, h=0.05):
    """x⁺ = x + h(Ax + Bu + 0.1 sin x), A_ij = −δ_ij + 0.3 cos(i + 2j) / n, B_ij = sin(3i + j) / √n (1-based)"""
    A = np.array([[(-1.0 if i == j else 0.0) + 0.3 * math.cos(float((i + 1) + 2 * (j + 1))) / float(n) for j in range(n)] for i in range(n)])
    Bm = np.array([[math.sin(float(3 * (i + 1) + (j + 1))) / math.sqrt(float(n)) for j in range(m)] for i in range(n)])
    return lambda x, u, w, t: x + h * (A @ x + Bm @ u + 0.1 * np.sin(x))


_F = {}


def dynamics(name):
    if name not in _F:
        _F[name] = {"car": lambda: M.car().f, "car_obs": lambda: M.car_obs().f, "synth12": lambda: M.synth12().f,
                    "acrobot": lambda: (lambda x, u, w, t: acrobot_midpoint(x, u)), "synth32": lambda: synth_f(32, 8)}[name]()
    return _F[name]


# ------------------------------------------------------------------------------------------------- the inputs of the GPU test
def inputs(workloads, name, B):
    """(x1 [B, n], ū [B, T-1, m], θ None or [B, T, nw]) at T = 11: the head of the workload's own inputs"""
    _, _, x1, ub = workloads.make_inputs(CONFIG[name], B)
    w = workloads.make_parameters("car_obs", B)[:, :T].copy() if name == "car_obs" else None
    return x1, np.ascontiguousarray(ub[:, :T - 1]), w


def plant_starts(xb):
    """x [B, n]: x̄_0 moved by half the SIZE_X1 move of mpc_ref"""
    return M.measured_starts(xb, 0, 0.5 * M.SIZE_X1)


def sigma_x(n):
    """a different size per state component, one of them zero (that component draws nothing)"""
    s = 1.0e-2 * (1.0 + np.arange(n)) / n
    s[n // 2] = 0.0
    return s


def plant_parameters(w, steps):
    """the plant's own parameters: the handle's first `steps` rows, moved"""
    return None if w is None else np.ascontiguousarray(w[:, :steps] + 0.01 * (1.0 + np.arange(w.shape[2])))


def cases():
    """(k, feedback, noise, step0) of the GPU test: every combination"""
    return [(k, fb, ns, s0) for k in STEPS for fb in (0, 1) for ns in (0, 1) for s0 in STEP0S]


def reference(name, xb, ub, K, w, x, k, fb, sig, z, s0, wp):
    """every instance: a list of plant_step dicts"""
    f = dynamics(name)
    return [plant_step(f, xb[b], ub[b], K[b], None if w is None else w[b], x[b], k, bool(fb), sig, None if z is None else z[b], s0,
                       None if wp is None else wp[b]) for b in range(xb.shape[0])]
