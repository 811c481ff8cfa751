"""The yardstick of the plant score (tests/test_plant_score_ref.py, tests/test_gpu_mpc_preview.py): ilqr_plant_score as
include/ilqr_hip.h defines it, in plain fp64 over the cost_s / con_s / ineq_s objects of tests/mpc_ref.py —

    w_i          = the user's columns of w_plant[i] if given, else of θ_i; selector columns are θ_i's (the yardstick's callables take
                   the step index instead of selectors, so only the user's columns exist here)
    cost[i]      = cost_s(x_i, u_i, w_i, i)                                   one stage term, no terminal term
    violation[i] = mpc_ref.violation(0, con_s(x_i, u_i, w_i, i), ineq_s(i))   0 without stage rows or on an unconstrained handle

— and a numpy restatement of the parameter rows of the horizon shift, on which the closed form of the preview is asserted. Nothing
here comes from the library.

Arrays are one instance's: x [steps + 1, n] (the last row is not read), u [steps, m], w None or [T, nw], w_plant None or [steps, nwu]."""
import numpy as np

import mpc_ref as M


def plant_score(p, x, u, w=None, w_plant=None, constrained=True):
    """-> dict(cost [steps], violation [steps])"""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    steps = u.shape[0]
    cost, viol = np.zeros(steps), np.zeros(steps)
    with np.errstate(all="ignore"):
        for i in range(steps):
            wi = M._NONE if w is None else np.array(w[i], dtype=np.float64)
            if w_plant is not None:
                wi[:len(w_plant[i])] = w_plant[i]
            cost[i] = float(p.cost_s(x[i], u[i], wi, i))
            if constrained and p.con_s is not None:
                viol[i] = M.violation(0.0, p.con_s(x[i], u[i], wi, i), M._rows(p.ineq_s, i))
    return dict(cost=cost, violation=viol)


def spread(p, x, u, w=None, w_plant=None):
    """How far the yardstick's own score moves when x and u move by one part in 1e15: dict(cost: |Δ| / |value|, viol: |Δ| / max(1, |v|)),
    the worst over the steps"""
    a = plant_score(p, x, u, w, w_plant)
    b = plant_score(p, np.asarray(x) * (1.0 + 1.0e-15), np.asarray(u) * (1.0 + 1.0e-15), w, w_plant)
    return dict(cost=float(np.max(np.abs(b["cost"] - a["cost"]) / np.abs(a["cost"]))),
                viol=float(np.max(np.abs(b["violation"] - a["violation"]) / np.maximum(1.0, np.abs(a["violation"])))))


_P = {}


def problem(name, T=11):
    """the Problem of a case; synth32: the independent restatement's objects (mpc_ref.synth), whose horizon enters its object lists"""
    if name not in _P:
        _P[name] = {"car": M.car, "car_obs": M.car_obs, "synth12": M.synth12, "synth5w": M.synth5w, "synth32": lambda: M.synth(T, 32, 8)[0]}[name]()
    return _P[name]


# ------------------------------------------------------------------------------------------------ the preview, restated
def shifted_parameters(w, steps, w_tail=None):
    """θ' of ilqr_shift_horizon for one instance: θ'_t = θ_{t+steps} while t + steps <= T − 1, then w_tail's rows, or θ_{T−1} held"""
    w = np.asarray(w, dtype=np.float64)
    T = w.shape[0]
    tail = np.repeat(w[T - 1:T], steps, axis=0) if w_tail is None else np.asarray(w_tail, dtype=np.float64)
    assert tail.shape == (steps,) + w.shape[1:]
    return np.concatenate([w[steps:], tail], axis=0)


def previewed_parameters(w, periods, steps, w_preview):
    """θ after `periods` shifts by `steps`, each fed rows p · steps .. of w_preview [periods · steps, nw]"""
    for p in range(periods):
        w = shifted_parameters(w, steps, w_preview[p * steps:(p + 1) * steps])
    return w


def preview_closed_form(w, periods, steps, w_preview):
    """the same in closed form: row t is the original θ_{t + P·k} while t + P·k <= T − 1, else w_preview[t + P·k − T]"""
    w, w_preview = np.asarray(w, dtype=np.float64), np.asarray(w_preview, dtype=np.float64)
    T, R = w.shape[0], periods * steps
    return np.stack([w[t + R] if t + R <= T - 1 else w_preview[t + R - T] for t in range(T)])


def distinct_preview(B, rows, nw):
    """w_preview [B, rows, nw] with a different value per (b, row, column): a transposed or misaligned stride cannot pass"""
    b, r, c = np.meshgrid(np.arange(B), np.arange(rows), np.arange(nw), indexing="ij")
    return 0.3 + 0.011 * r + 0.0013 * c + 0.00017 * b
