"""Inputs of tests/test_gpu_failed_pivot.py (TEST INFRASTRUCTURE), kept apart from it so that tests/test_failed_pivot_inputs.py can
check their conditioning on the CPU: which stage kernel meets which model and pivot, where the bad diagonal entries go, and the
small parametrised model whose stage cost makes a pivot fail by itself.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

B = 3                       # two failing instances and one healthy
HORIZONS = (6, 7)           # the first step taken is an even / an odd entry of the unrolled loops
ORACLE_MODELS = {"car": (3, 2), "synth12": (12, 5), "synth32": (32, 8)}

# (stage kernel, kernel variant, model, pivot (1-based)); a model is an oracle model's name or (nx, nu) of the synth family
STAGE_CASES = (
    [("K_STAGE", "auto", "car", j) for j in (1, 2)] + [("K_STAGE", "auto", (4, 3), j) for j in (1, 2, 3)] +
    [("K_STAGE", "auto", nm, j) for nm in ((3, 4), (4, 4)) for j in (1, 2, 3, 4)] +
    [("K_STAGE_SLIM", "throughput", "car", 2), ("K_STAGE_SLIM", "throughput", (4, 4), 1), ("K_STAGE_SLIM", "throughput", (4, 4), 4)] +
    [("K_STAGE_MID", "mid", "synth12", 1), ("K_STAGE_MID", "mid", "synth12", 5)] + [("K_STAGE_MID", "mid", (16, 16), j) for j in (1, 9, 16)] +
    [("four-wave", "auto", (17, 2), 2), ("four-wave", "auto", "synth32", 8), ("four-wave", "auto", (64, 8), 1), ("four-wave", "auto", (64, 8), 8)])
# one NaN pivot per stage kernel, at the middle step
NAN_CASES = [("K_STAGE", "auto", (4, 3), 2), ("K_STAGE_SLIM", "throughput", (4, 4), 4), ("K_STAGE_MID", "mid", "synth12", 1),
             ("four-wave", "auto", (64, 8), 8)]


def case_id(case):
    kernel, _, model, pivot = case
    return "%s-%s-pivot%d" % (kernel, model if isinstance(model, str) else "synth%dx%d" % model, pivot)


def dims(model):
    return ORACLE_MODELS[model] if isinstance(model, str) else model


def start(model, T):
    """x1 [B, n], ū [B, T-1, m]: small enough that a healthy pass stays well conditioned, across the action box of the synth family."""
    n, m = dims(model)
    rng = np.random.default_rng(1000 * n + 10 * m + T)
    return 0.5 * rng.standard_normal((B, n)), 0.4 * rng.standard_normal((B, T - 1, m)) + 0.3


def failing_steps(T):
    """the first step the pass takes, a middle one, and the last"""
    return (T - 2, (T - 2) // 2, 0)


def inject(guu, T, m, pivot, value=None):
    """guu [B, (T-1)*m*m] as the handle holds it -> a copy with diagonal entry `pivot` of instances 0 and 1 replaced: by -5 - b at
    failing_steps(T), or by `value` (NaN) at the middle step alone. Instance 2 stays as it is."""
    g = np.array(guu, dtype=np.float64).reshape(B, T - 1, m, m).copy()
    for b in range(2):
        for t in (failing_steps(T) if value is None else failing_steps(T)[1:2]):
            g[b, t, pivot - 1, pivot - 1] = (-5.0 - b) if value is None else value
    return g.reshape(B, -1)


# ------------------------------------------------------------------ the model that fails by itself (fused kernels, packed kernel)
FUSED_SIZES = {(3, 2): 0, (4, 4): 3}          # (nx, nu) -> j: the stage cost carries w0 u_j^2, pivot j + 1 fails for w0 of order -1
FUSED_HORIZONS = (2, 3, 6, 7)
FUSED_B = 5                                   # a full packed wave (four instances) and a ragged one
FUSED_FAILING = ((1,), (0, 2, 4))
H_STEP = 0.1


def _coefficients(n, m):
    A = [[(-0.5 if i == j else 0.0) + 0.2 * np.cos(1.0 + i + 2 * j) for j in range(n)] for i in range(n)]
    Bm = [[np.sin(1.0 + 3 * i + j) for j in range(m)] for i in range(n)]
    return A, Bm


def w0_model(mod, n, m):
    """A small-path model with one parameter per timestep, written once for the product's symbolic generator (mod = the package) and
    for the restatement's (mod = reference_restatement): x+ = x + h (A x + B u + 0.3 sin x), stage cost
    0.5 |x|^2 + 0.05 sum (1 + i) u_i^2 + 0.01 u_0 u_{m-1} + w0 u_j^2, a box on u_0 and a terminal goal on x_0.
    guu_jj = 0.1 (1 + j) + 2 w0: healthy for w0 = +1, a failed pivot j + 1 at every step for w0 of order -1 (fu'P fu is O(h^2 |P|))."""
    import sympy as sp
    j = FUSED_SIZES[(n, m)]
    A, Bm = _coefficients(n, m)
    f = lambda x, u, w: [x[i] + H_STEP * (sum(A[i][c] * x[c] for c in range(n)) + sum(Bm[i][c] * u[c] for c in range(m)) + 0.3 * sp.sin(x[i]))
                         for i in range(n)]
    stage = lambda x, u, w: (0.5 * sum(xi * xi for xi in x) + 0.05 * sum((1 + i) * u[i] * u[i] for i in range(m))
                             + 0.01 * u[0] * u[m - 1] + w[0] * u[j] * u[j])
    return dict(dynamics=mod.Dynamics(f, n, m, num_parameter=1), cost_stage=mod.Cost(stage, n, m, num_parameter=1),
                cost_term=mod.Cost(lambda x, u, w: 5.0 * sum(xi * xi for xi in x), n, 0, num_parameter=1),
                con_stage=mod.Constraint(lambda x, u, w: [u[0] - 0.8, -0.8 - u[0]], n, m, indices_inequality=[1, 2], num_parameter=1),
                con_term=mod.Constraint(lambda x, u, w: [x[0] - 0.3], n, 0, num_parameter=1))


_W0 = {}


def w0_problem(mod, n, m, T):
    if (mod.__name__, n, m) not in _W0:
        _W0[(mod.__name__, n, m)] = w0_model(mod, n, m)
    d = _W0[(mod.__name__, n, m)]
    return [d["dynamics"]] * (T - 1), [d["cost_stage"]] * (T - 1) + [d["cost_term"]], [d["con_stage"]] * (T - 1) + [d["con_term"]]


def w0_inputs(n, m, T, failing):
    """x1 [B, n], ū [B, T-1, m], w [B, T, 1]: w0 = +1, and -1.5 - 0.1 b on the failing instances b"""
    rng = np.random.default_rng(100 * n + 10 * m + T)
    x1 = 0.3 * rng.standard_normal((FUSED_B, n)); ub = 0.3 * rng.standard_normal((FUSED_B, T - 1, m))
    w = np.ones((FUSED_B, T, 1))
    for b in failing:
        w[b] = -1.5 - 0.1 * b
    return x1, ub, w
