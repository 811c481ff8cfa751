"""The yardstick of the policy-rollout tests (tests/test_policy_rollout_abi.py, tests/test_gpu_policy_rollout.py): two readings of

    x_1 = x1,   u_t = ū_t + K_t (x_t − x̄_t) + α k_t,   x_{t+1} = f(x_t, u_t, w_t)                      (src/rollout.jl:19-30)

on the CPU oracle. Arrays are one instance's: xb [T, n], ub [T-1, m], K [T-1, n, m] (column-major m×n blocks, as get_policy
returns them), k [T-1, m], w None or [T, nw].
"""
import numpy as np

# per-model workloads of the tests: (workloads config, horizon, size of the x1 perturbation, oracle model of the same name)
CASES = {"acrobot": ("acrobot", 101, 0.05), "car": ("car", 51, 0.05), "car_obs": ("car_obs", 51, 0.05),
         "particle": ("particle", 11, 0.1), "synth12": ("synth12", 101, 0.02)}
SEED = 20251017


def perturbed_starts(xb1, S, size, seed=SEED):
    """x1[s] = x̄_1 + size · N(0, 1), sample 0 exactly x̄_1; a fixed seed."""
    rng = np.random.default_rng(seed)
    x1 = np.asarray(xb1, dtype=np.float64)[None, :] + size * rng.standard_normal((S, len(xb1)))
    x1[0] = xb1
    return x1


def sample_parameters(w, S, size=0.02, seed=SEED + 1):
    """the instance's parameters [T, nw], moved per sample"""
    rng = np.random.default_rng(seed)
    return np.asarray(w)[None] + size * rng.standard_normal((S,) + np.asarray(w).shape)


def first_nonfinite(x):
    bad = ~np.isfinite(np.asarray(x)).all(axis=-1)
    return int(np.argmax(bad)) if bad.any() else -1


def oracle_reading(O, model, T, xb, ub, K, x1, w=None):
    """orc_rollout_bang driven to start at x1: nominal_states[0] <- x1, k_0 = K_0 (x1 − x̄_1), k_t = 0 otherwise, rollout!(1.0);
    cost and violation with zeroed duals and penalties through cost!(:current). Returns dict(x, u, cost, max_violation, first_nonfinite)."""
    pr = O.Problem(model, T)
    n, m = pr.nx, pr.nu
    xb, ub, K = np.asarray(xb, dtype=np.float64).reshape(T, n), np.asarray(ub, dtype=np.float64).reshape(T - 1, m), np.asarray(K, dtype=np.float64).reshape(T - 1, n, m)
    s = O.Solver(pr, O.default_options(), w=w)
    s.set_buffer("nominal_actions", ub)
    s.set_buffer("K", K)
    xs = xb.copy()
    xs[0] = x1
    s.set_buffer("nominal_states", xs)
    k = np.zeros((T - 1, m))
    d = np.asarray(x1, dtype=np.float64) - xb[0]
    for i in range(m):
        acc = 0.0
        for j in range(n):
            acc += K[0, j, i] * d[j]
        k[0, i] = acc
    s.set_buffer("k", k)
    s.call("rollout_bang", 1.0)
    return _finish(s, T, n, m)


def oracle_rollout_bang(O, model, T, xb, ub, K, k, alpha, w=None):
    """the oracle's UNMODIFIED rollout!(policy, problem; step_size = alpha) from x̄_1"""
    pr = O.Problem(model, T)
    s = O.Solver(pr, O.default_options(), w=w)
    s.set_buffer("nominal_actions", ub); s.set_buffer("nominal_states", xb); s.set_buffer("K", K); s.set_buffer("k", k)
    s.call("rollout_bang", float(alpha))
    return _finish(s, T, pr.nx, pr.nu)


def _finish(s, T, n, m):
    x, u = s.buffer("states").reshape(T, n), s.buffer("actions").reshape(T - 1, m)
    try:
        s.set_buffer("constraint_dual", np.zeros_like(s.buffer("constraint_dual")))
        s.set_buffer("constraint_penalty", np.zeros_like(s.buffer("constraint_penalty")))
    except KeyError:
        pass
    s.call("cost_bang", 1)
    st = s.stats()
    return dict(x=x, u=u, cost=st.objective, max_violation=st.max_violation, first_nonfinite=first_nonfinite(x))


def numpy_reading(O, model, T, xb, ub, K, k, x1, alpha=0.0, w=None):
    """the same formula as a plain loop, in the operation order of src/rollout.jl:24-28, the dynamics stepped by a T = 2 oracle problem"""
    pr2 = O.Problem(model, 2)
    n, m = pr2.nx, pr2.nu
    xb, ub, K, k = np.asarray(xb).reshape(T, n), np.asarray(ub).reshape(T - 1, m), np.asarray(K).reshape(T - 1, n, m), np.asarray(k).reshape(T - 1, m)
    x, u = np.zeros((T, n)), np.zeros((T - 1, m))
    x[0] = x1
    for t in range(T - 1):
        for i in range(m):
            v = k[t, i]
            v = v * alpha
            v = v + ub[t, i]
            a1 = 0.0
            for j in range(n):
                a1 += K[t, j, i] * x[t, j]
            v = v + a1
            a2 = 0.0
            for j in range(n):
                a2 += K[t, j, i] * xb[t, j]
            u[t, i] = v + -1.0 * a2
        wt = None if w is None else np.ascontiguousarray(np.stack([w[t], w[t]]))
        x[t + 1] = pr2.rollout(x[t], u[t:t + 1], w=wt)[1]
    return dict(x=x, u=u, first_nonfinite=first_nonfinite(x))


def spread(O, model, T, xb, ub, K, x1s, ws=None):
    """How far the oracle's own recursion moves when x1 moves by one part in 1e15: max |Δx|, |Δu| over the samples, relative to
    max(1, max |x|) resp. max(1, max |u|) — the rounding amplification of the perturbed closed loop, from the oracle alone."""
    worst = 0.0
    for s, x1 in enumerate(x1s):
        w = None if ws is None else ws[s]
        a = oracle_reading(O, model, T, xb, ub, K, x1, w)
        b = oracle_reading(O, model, T, xb, ub, K, np.asarray(x1) * (1.0 + 1.0e-15), w)
        worst = max(worst, rel(b["x"], a["x"]), rel(b["u"], a["u"]))
    return worst


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))
