"""The yardstick of the candidate-initialiser tests (tests/test_candidates_abi.py, tests/test_gpu_candidates.py), on the CPU oracle:
for one instance and one candidate action sequence u_s

    x = rollout(dynamics, x1, u_s)   (src/rollout.jl:33-42),   cost = Σ cost   (src/costs.jl:48-55),
    max_violation = constraint_violation   (src/data/constraints.jl:23-39)

read off the oracle's own cost!(:current) with zeroed duals and penalties, as tests/policy_ref.py::_finish does; the selection
rule is plain Python. Arrays are one instance's: x1 [n], u [S, T-1, m], w None or [T, nw].
"""
import math

import numpy as np

from policy_ref import first_nonfinite

# per-model workloads of the tests: (workloads config, horizon, size of the noise added to the scaled ū)
CASES = {"acrobot": ("acrobot", 101, 0.2), "car": ("car", 51, 0.004), "car_obs": ("car_obs", 51, 0.004),
         "particle": ("particle", 11, 0.05), "synth12": ("synth12", 101, 0.05)}
SEED = 20261019


def candidates(ub, S, size, b=0, seed=SEED):
    """u[s] for one instance: candidate 0 is the workload's own ū, candidate s >= 1 is ū · scale_s + size · N(0, 1) with the scales
    spread over [0, 1.5]. Candidate s depends on (seed, b, s) only — not on S — so the first candidates of a longer list are the
    shorter list."""
    ub = np.asarray(ub, dtype=np.float64)
    u = np.empty((S,) + ub.shape)
    u[0] = ub
    for s in range(1, S):
        rng = np.random.default_rng([seed, b, s])
        u[s] = ub * (1.5 * ((s - 1) % 16) / 15.0) + size * rng.standard_normal(ub.shape)
    return u


def score_one(O, model, T, x1, u_s, w=None, constrained=True):
    """One candidate on the oracle: dict(x, cost, max_violation, first_nonfinite)."""
    pr = O.Problem(model, T)
    u_s = np.ascontiguousarray(u_s, dtype=np.float64).reshape(T - 1, pr.nu)
    x = pr.rollout(x1, u_s, w=w)
    s = O.Solver(pr, O.default_options(), w=w)
    s.set_buffer("states", x)
    s.set_buffer("actions", u_s)
    try:
        s.set_buffer("constraint_dual", np.zeros_like(s.buffer("constraint_dual")))
        s.set_buffer("constraint_penalty", np.zeros_like(s.buffer("constraint_penalty")))
    except KeyError:
        pass
    s.call("cost_bang", 1)
    st = s.stats()
    return dict(x=x, cost=float(st.objective), max_violation=float(st.max_violation) if constrained else 0.0, first_nonfinite=first_nonfinite(x))


def score_all(O, model, T, x1, u, w=None, constrained=True):
    """Every candidate of one instance: dict(cost [S], max_violation [S], first_nonfinite [S])."""
    rs = [score_one(O, model, T, x1, u_s, w, constrained) for u_s in u]
    return dict(cost=np.array([r["cost"] for r in rs]), max_violation=np.array([r["max_violation"] for r in rs]),
                first_nonfinite=np.array([r["first_nonfinite"] for r in rs], dtype=np.int32))


def scores(cost, max_violation, weight):
    """score = cost when weight == 0 (no multiplication), else cost + weight · max_violation"""
    return [float(c) if weight == 0 else float(c) + weight * float(v) for c, v in zip(cost, max_violation)]


def select(cost, max_violation, nonfinite, weight=0.0):
    """The eligible candidate (finite score, first_nonfinite == -1) with the lowest score, ties to the lowest index; -1 if none."""
    best, best_score = -1, None
    for s, sc in enumerate(scores(cost, max_violation, weight)):
        if not math.isfinite(sc) or int(nonfinite[s]) != -1:
            continue
        if best < 0 or sc < best_score:
            best, best_score = s, sc
    return best


def gap(cost, max_violation, nonfinite, weight=0.0):
    """(second-best − best eligible score) / max(1, |best|); inf with fewer than two eligible candidates"""
    el = sorted(sc for s, sc in enumerate(scores(cost, max_violation, weight)) if math.isfinite(sc) and int(nonfinite[s]) == -1)
    return math.inf if len(el) < 2 else (el[1] - el[0]) / max(1.0, abs(el[0]))


def spread(O, model, T, x1, u, w=None):
    """How far the oracle's own open-loop recursion moves the cost and the violation when its inputs move by one part in 1e15 —
    x1 · (1 + 1e-15), and (x1 is zero in some workloads) u · (1 + 1e-15) as well: the worst |Δ| over the candidates and the two
    moves relative to max(1, |value|) — the rounding amplification of the rollout, from the oracle alone."""
    worst = 0.0
    for u_s in u:
        a = score_one(O, model, T, x1, u_s, w)
        for x1p, up in ((np.asarray(x1) * (1.0 + 1.0e-15), u_s), (x1, np.asarray(u_s) * (1.0 + 1.0e-15))):
            b = score_one(O, model, T, x1p, up, w)
            worst = max(worst, abs(b["cost"] - a["cost"]) / max(1.0, abs(a["cost"])),
                        abs(b["max_violation"] - a["max_violation"]) / max(1.0, abs(a["max_violation"])))
    return worst
