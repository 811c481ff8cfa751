"""The model-agnostic yardstick of the MPC-side kernels (tests/test_mpc_ref.py, tests/test_gpu_mpc_sweep.py): the closed-loop policy
rollout, the open-loop candidate score and the closed-loop head of the horizon shift written ONCE as plain fp64 loops over
callables, in the operation order include/ilqr_hip.h documents —

    x_1 = x1,   u_t[i] = ((k_t[i] · α + ū_t[i]) + Σ_j K[t, j, i] · x_t[j]) − Σ_j K[t, j, i] · x̄_t[j]   (sums in ascending j),
    x_{t+1} = f(x_t, u_t, w_t),   cost = Σ_t cost (in timestep order),
    max_violation = max(0, c) on inequality rows, |c| on equality rows (NaN-propagating)

— so that the sizes of the synth family the C++ oracle has no twin for, and lowered problems whose objects differ from step to
step, have a reference. The callables take (x, u, w, t): per-step objects and padded dimensions fit. They come from two places:
the objects of the independent restatement (tests/golden/reference_restatement.py, `from_restatement`), and the small numpy
functions below, written from the models' formulas (test/car.jl of the reference, iterativelqr.jl_amd/models.py) and from nothing
the device runs. Selection, blend and the open-loop shift are candidates_ref.select / scores, sample_ref.noise / blend_weights /
blend_actions and shift_ref.shifted_inputs, unchanged.

The input generators of the GPU sweep live here too, so that the CPU check of the inputs (every sample finite on the yardstick,
ten times the yardstick's own spread under the bound) and the GPU tests use the same arrays.

Arrays are one instance's: xb [T, n], ub [T-1, m], K [T-1, n, m] (as get_policy returns it), k [T-1, m], w None or [T, nw]."""
import collections
import math
import os
import sys

import numpy as np

import policy_ref
import shift_ref

Problem = collections.namedtuple("Problem", "f cost_s cost_t con_s con_t ineq_s ineq_t")
_NONE = np.zeros(0)


# --------------------------------------------------------------------------------------------------------------- the operations
def _rows(ineq, t):
    return ineq(t) if callable(ineq) else ineq


def _nanmax(a, b):
    return math.nan if (a != a or b != b) else max(a, b)


def violation(v, c, ineq):
    """v raised by the rows c: max(0, c_i) for i in ineq (0-based), |c_i| otherwise; NaN-propagating"""
    ineq = set(ineq)
    for i, ci in enumerate(c):
        ci = float(ci)
        v = _nanmax(v, _nanmax(0.0, ci) if i in ineq else abs(ci))
    return v


def _wt(w, t):
    return _NONE if w is None else w[t]


def _score(p, x, u, w):
    """cost and max_violation of a trajectory, terms in timestep order"""
    T = x.shape[0]
    J, v = 0.0, 0.0
    for t in range(T - 1):
        J += float(p.cost_s(x[t], u[t], _wt(w, t), t))
        if p.con_s is not None:
            v = violation(v, p.con_s(x[t], u[t], _wt(w, t), t), _rows(p.ineq_s, t))
    J += float(p.cost_t(x[T - 1], _NONE, _wt(w, T - 1), T - 1))
    if p.con_t is not None:
        v = violation(v, p.con_t(x[T - 1], _NONE, _wt(w, T - 1), T - 1), _rows(p.ineq_t, T - 1))
    return J, v


def policy_rollout(f, cost_s, cost_t, con_s, con_t, ineq_s, ineq_t, xb, ub, K, k, x1, alpha, w):
    """-> dict(x [T, n], u [T-1, m], cost, max_violation, first_nonfinite)"""
    p = Problem(f, cost_s, cost_t, con_s, con_t, ineq_s, ineq_t)
    xb, ub, K, k = (np.asarray(a, dtype=np.float64) for a in (xb, ub, K, k))
    T, n = xb.shape
    m = ub.shape[1]
    x, u = np.zeros((T, n)), np.zeros((T - 1, m))
    x[0] = x1
    with np.errstate(all="ignore"):
        for t in range(T - 1):
            for i in range(m):
                v = k[t, i] * alpha
                v = v + ub[t, i]
                a1 = 0.0
                for j in range(n):
                    a1 += K[t, j, i] * x[t, j]
                v = v + a1
                a2 = 0.0
                for j in range(n):
                    a2 += K[t, j, i] * xb[t, j]
                u[t, i] = v - a2
            x[t + 1] = f(x[t], u[t], _wt(w, t), t)
        J, viol = _score(p, x, u, w)
    return dict(x=x, u=u, cost=J, max_violation=viol, first_nonfinite=policy_ref.first_nonfinite(x))


def score_candidate(f, cost_s, cost_t, con_s, con_t, ineq_s, ineq_t, x1, u, w):
    """the same open-loop: -> dict(x, cost, max_violation, first_nonfinite)"""
    p = Problem(f, cost_s, cost_t, con_s, con_t, ineq_s, ineq_t)
    u = np.asarray(u, dtype=np.float64)
    T = u.shape[0] + 1
    x = np.zeros((T, len(x1)))
    x[0] = x1
    with np.errstate(all="ignore"):
        for t in range(T - 1):
            x[t + 1] = f(x[t], u[t], _wt(w, t), t)
        J, viol = _score(p, x, u, w)
    return dict(x=x, cost=J, max_violation=viol, first_nonfinite=policy_ref.first_nonfinite(x))


def score_all(p, x1, us, w=None):
    """every candidate of one instance, as candidates_ref.score_all: dict(cost [S], max_violation [S], first_nonfinite [S])"""
    rs = [score_candidate(*p, x1, u_s, w) for u_s in us]
    return dict(cost=np.array([r["cost"] for r in rs]), max_violation=np.array([r["max_violation"] for r in rs]),
                first_nonfinite=np.array([r["first_nonfinite"] for r in rs], dtype=np.int32))


def shift_head(p, xb, ub, K, wp, steps, x1):
    """The closed-loop head of a shift by `steps`: policy_rollout with α = 0, k = 0 on the slices xb[steps:], ub[steps:],
    K[steps:], w'[:T − steps] (the callables see the SHIFTED step index: use it on problems whose objects do not depend on t, or
    with steps = 0). -> dict(x [T − steps, n], u [T − steps − 1, m], first_nonfinite)"""
    xs, us, Ks = np.asarray(xb)[steps:], np.asarray(ub)[steps:], np.asarray(K)[steps:]
    ws = None if wp is None else np.asarray(wp)[:xs.shape[0]]
    r = policy_rollout(*p, xs, us, Ks, np.zeros_like(us), x1, 0.0, ws)
    return dict(x=r["x"], u=r["u"], first_nonfinite=r["first_nonfinite"])


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def spread(p, xb, ub, K, k, x1s, alpha=0.0, ws=None):
    """How far the yardstick's own closed-loop recursion moves when x1 moves by one part in 1e15 (policy_ref.spread on the
    callables): the worst over the samples of dict(xu: |Δx|, |Δu| relative to max(1, max |x|) resp. max(1, max |u|); cost, viol:
    |Δ| relative to max(1, |value|))."""
    worst = dict(xu=0.0, cost=0.0, viol=0.0)
    for s, x1 in enumerate(x1s):
        w = None if ws is None else ws[s]
        a = policy_rollout(*p, xb, ub, K, k, x1, alpha, w)
        b = policy_rollout(*p, xb, ub, K, k, np.asarray(x1) * (1.0 + 1.0e-15), alpha, w)
        worst["xu"] = max(worst["xu"], policy_ref.rel(b["x"], a["x"]), policy_ref.rel(b["u"], a["u"]))
        worst["cost"] = max(worst["cost"], _rel(b["cost"], a["cost"]))
        worst["viol"] = max(worst["viol"], _rel(b["max_violation"], a["max_violation"]))
    return worst


def score_spread(p, x1, us, w=None):
    """candidates_ref.spread on the callables: the open-loop score under x1 · (1 + 1e-15) and under u · (1 + 1e-15)"""
    worst = dict(cost=0.0, viol=0.0)
    for u_s in us:
        a = score_candidate(*p, x1, u_s, w)
        for x1p, up in ((np.asarray(x1) * (1.0 + 1.0e-15), u_s), (x1, np.asarray(u_s) * (1.0 + 1.0e-15))):
            b = score_candidate(*p, x1p, up, w)
            worst["cost"] = max(worst["cost"], _rel(b["cost"], a["cost"]))
            worst["viol"] = max(worst["viol"], _rel(b["max_violation"], a["max_violation"]))
    return worst


# ------------------------------------------------------------------------------------------- callables: the restatement's objects
def restatement():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import reference_restatement
    return reference_restatement


def from_restatement(dynamics, costs, constraints):
    """(dynamics[T-1], costs[T], constraints[T]) of tests/golden/reference_restatement.py as a Problem"""
    T = len(costs)

    def rows(c, x, u, w):
        return c.evaluate(x, u, w) if c.num_constraint else _NONE

    # the terminal objects are the last ones whatever t says: the head of a shift ends before the horizon does
    return Problem(lambda x, u, w, t: dynamics[t].evaluate(x, u, w), lambda x, u, w, t: costs[t].evaluate(x, u, w),
                   lambda x, u, w, t: costs[T - 1].evaluate(x, u, w), lambda x, u, w, t: rows(constraints[t], x, u, w),
                   lambda x, u, w, t: rows(constraints[T - 1], x, u, w), lambda t: constraints[t].indices_inequality,
                   constraints[T - 1].indices_inequality)


_SYNTH = {}


def synth(T, n, m):
    """the restatement's synth family (synth32_problem(T, n, m)) as a Problem and its objects; built once per size"""
    if (T, n, m) not in _SYNTH:
        objs = restatement().synth32_problem(T, n, m)
        _SYNTH[(T, n, m)] = (from_restatement(*objs), objs)
    return _SYNTH[(T, n, m)]


# ------------------------------------------------------------------------- callables: plain numpy, from the models' formulas
CAR_XT, CAR_OBS, CAR_R = (1.0, 1.0, 0.0), (0.5, 0.5), 0.1


def _car_c(x, u):
    return (u[0] * math.cos(x[2]), u[0] * math.sin(x[2]), u[1])


def car_midpoint(x, u, h=0.1):
    k1 = _car_c(x, u)
    k2 = _car_c([x[i] + 0.5 * h * k1[i] for i in range(3)], u)
    return np.array([x[i] + h * k2[i] for i in range(3)])


def car_euler(x, u, h=0.05):
    k1 = _car_c(x, u)
    return np.array([x[i] + h * k1[i] for i in range(3)])


def _car_goal2(x):
    return sum((x[i] - CAR_XT[i]) ** 2 for i in range(3))


def car_stage_cost(x, u, r=1.0e-2):
    return 1.0 * _car_goal2(x) + r * (u[0] * u[0] + u[1] * u[1])


def car_term_cost(x):
    return 1000.0 * _car_goal2(x)


def _car_clear(x, p):
    return CAR_R ** 2.0 - ((x[0] - p[0]) ** 2 + (x[1] - p[1]) ** 2)


def car_stage_rows(x, u, p=CAR_OBS):
    return np.array([-5.0 - u[0], -5.0 - u[1], u[0] - 5.0, u[1] - 5.0, _car_clear(x, p)])


def car_term_rows(x, p=CAR_OBS):
    return np.array([x[0] - CAR_XT[0], x[1] - CAR_XT[1], x[2] - CAR_XT[2], _car_clear(x, p)])


def car():
    """test/car.jl"""
    return Problem(lambda x, u, w, t: car_midpoint(x, u), lambda x, u, w, t: car_stage_cost(x, u), lambda x, u, w, t: car_term_cost(x),
                   lambda x, u, w, t: car_stage_rows(x, u), lambda x, u, w, t: car_term_rows(x), (0, 1, 2, 3, 4), (3,))


def car_obs(action_weight=lambda t: 1.0e-2):
    """car with the obstacle centre in θ_t = (p_x, p_y); action_weight(t): the weight of ‖u‖² in the stage cost of step t"""
    return Problem(lambda x, u, w, t: car_midpoint(x, u), lambda x, u, w, t: car_stage_cost(x, u, action_weight(t)),
                   lambda x, u, w, t: car_term_cost(x), lambda x, u, w, t: car_stage_rows(x, u, w), lambda x, u, w, t: car_term_rows(x, w),
                   (0, 1, 2, 3, 4), (3,))


def car_tv(T):
    """models.car_tv: the dynamics by t % 3 (Euler h = 0.05 at 2, else midpoint h = 0.1), the stage cost by halves of the horizon,
    the stage constraint by t % 4 (five inequalities / none / one equality / none); every step has its own rows"""
    q, xg, r = (5.0, 2.0, 0.5), (0.9, 1.1, 0.2), (0.05, 0.02)

    def cost(x, u, w, t):
        if 2 * t >= T - 1:
            return sum(q[i] * (x[i] - xg[i]) ** 2 for i in range(3)) + sum(r[j] * u[j] ** 2 for j in range(2))
        return car_stage_cost(x, u)

    def rows(x, u, w, t):
        return car_stage_rows(x, u) if t % 4 == 0 else (np.array([u[1] - 0.3 * x[2] - 0.05]) if t % 4 == 2 else _NONE)

    return Problem(lambda x, u, w, t: car_euler(x, u) if t % 3 == 2 else car_midpoint(x, u), cost, lambda x, u, w, t: car_term_cost(x),
                   rows, lambda x, u, w, t: car_term_rows(x), lambda t: (0, 1, 2, 3, 4) if t % 4 == 0 else (), (3,))


def synth12():
    """models.synth12: x⁺ = x + h(Ax + Bu + 0.1 sin x + 0.02 x_i u_{i mod m}), n = 12, m = 5, an action box, x_{0..2} = 0.1 at the end"""
    n, m, h, xg = 12, 5, 0.05, 0.5
    A = np.array([[(-1.0 if i == j else 0.0) + 0.3 * math.cos(float((i + 1) + 2 * (j + 1))) / 12.0 for j in range(n)] for i in range(n)])
    Bm = np.array([[math.sin(float(3 * (i + 1) + (j + 1))) / math.sqrt(12.0) for j in range(m)] for i in range(n)])
    own = np.arange(n) % m

    def f(x, u, w, t):
        return x + h * (A @ x + Bm @ u + 0.1 * np.sin(x) + 0.02 * (x * u[own]))

    return Problem(f, lambda x, u, w, t: 0.1 * float(((x - xg) ** 2).sum()) + 0.01 * float((u * u).sum()),
                   lambda x, u, w, t: 10.0 * float(((x - xg) ** 2).sum()), lambda x, u, w, t: np.concatenate([-1.0 - u, u - 1.0]),
                   lambda x, u, w, t: x[:3] - 0.1, tuple(range(2 * m)), ())


# ---------------------------------------------------------------- a large-form model with a user parameter (nx = 5, nu = 1)
def synth5w_functions(sin):
    """The synth family at (5, 1) with one user parameter θ_t = (w,): a drift w on every state row and a goal of 0.5 + w —
    x⁺ = x + h(Ax + Bu + 0.1 sin x + w), ℓ = 0.1 Σ (x_i − 0.5 − w)² + r u² (r: the stage kind), ℓ_T = 10 Σ (x_i − 0.5 − w)², the
    action box. Plain arithmetic on sequences, so the same formulas trace symbolically (sin = sympy.sin: the device's and the
    restatement's objects) and evaluate numerically (sin = math.sin: the yardstick). -> (f, stage(r), term, box), each (x, u, w)."""
    n, m, h = 5, 1, 0.05
    A = [[(-1.0 if i == j else 0.0) + 0.3 * math.cos(float((i + 1) + 2 * (j + 1))) / float(n) for j in range(n)] for i in range(n)]
    Bm = [[math.sin(float(3 * (i + 1) + (j + 1))) / math.sqrt(float(n)) for j in range(m)] for i in range(n)]
    f = lambda x, u, w: [x[i] + h * (sum(A[i][j] * x[j] for j in range(n)) + Bm[i][0] * u[0] + 0.1 * sin(x[i]) + w[0]) for i in range(n)]
    stage = lambda r: (lambda x, u, w: 0.1 * sum((x[i] - 0.5 - w[0]) * (x[i] - 0.5 - w[0]) for i in range(n)) + r * u[0] * u[0])
    term = lambda x, u, w: 10.0 * sum((x[i] - 0.5 - w[0]) * (x[i] - 0.5 - w[0]) for i in range(n))
    box = lambda x, u, w: [-1.0 - u[0], u[0] - 1.0]
    return f, stage, term, box


SYNTH5W_WEIGHTS = (0.01, 0.03)          # the two stage kinds, alternating: even steps, odd steps


def synth5w():
    f, stage, term, box = synth5w_functions(math.sin)
    kinds = [stage(r) for r in SYNTH5W_WEIGHTS]
    return Problem(lambda x, u, w, t: np.array(f(x, u, w)), lambda x, u, w, t: kinds[t % 2](x, u, w), lambda x, u, w, t: term(x, u, w),
                   lambda x, u, w, t: np.array(box(x, u, w)), None, (0, 1), ())


def synth5w_parameters(B=None, T=None):
    """w [B, T, 1], different from row to row and from instance to instance"""
    B, T = B_SWEEP if B is None else B, T_SWEEP if T is None else T
    return (0.1 + 0.01 * np.arange(T)[None, :] + 0.02 * np.arange(B)[:, None])[:, :, None]


def synth5w_restatement_policy(B=None, T=None):
    """the restatement's solve of the alternating-kind problem under synth5w_parameters, from the (5, 1) sweep inputs"""
    B, T = B_SWEEP if B is None else B, T_SWEEP if T is None else T
    R = restatement()
    import sympy as sp
    f, stage, term, box = synth5w_functions(sp.sin)
    dyn = R.Dynamics(f, 5, 1, num_parameter=1)
    kinds = [R.Cost(stage(r), 5, 1, num_parameter=1) for r in SYNTH5W_WEIGHTS]
    con = R.Constraint(box, 5, 1, indices_inequality=[1, 2], num_parameter=1)
    dynamics, costs = [dyn] * (T - 1), [kinds[t % 2] for t in range(T - 1)] + [R.Cost(term, 5, 0, num_parameter=1)]
    x1, ub = sweep_inputs(5, 1, B, T)
    w = synth5w_parameters(B, T)
    out = []
    for b in range(B):
        s = R.Solver(dynamics, costs, [con] * (T - 1) + [R.Constraint()], parameters=list(w[b]))
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dynamics, x1[b], ub[b], list(w[b])))
        s.solve()
        out.append((np.stack(s.nominal_states), np.stack(s.nominal_actions[:-1]), np.stack([Kt.T for Kt in s.K]), np.stack(s.k)))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


# ------------------------------------------------------------------------------- ragged: time-varying dimensions, zero-padded
T_RAGGED = 9


def ragged(T=T_RAGGED):
    """the restatement's ragged_problem on arrays padded to the largest dimensions (padded next-state rows are 0, padded actions
    cost u² / 2 on the device and are 0 here) -> (Problem, objects, state_dims, action_dims)"""
    R = restatement()
    rd, rc, rk = R.ragged_problem(T)
    n_t, m_t = [R.RAGGED_N[t % 8] for t in range(T)], [R.RAGGED_M[t % 8] for t in range(T - 1)]
    n, last = max(n_t), T - 1

    def f(x, u, w, t):
        out = np.zeros(n)
        y = rd[t].evaluate(x[:n_t[t]], u[:m_t[t]], [])
        out[:len(y)] = y
        return out

    p = Problem(f, lambda x, u, w, t: rc[t].evaluate(x[:n_t[t]], u[:m_t[t]], []), lambda x, u, w, t: rc[last].evaluate(x[:n_t[last]], [], []),
                None, lambda x, u, w, t: rk[last].evaluate(x[:n_t[last]], [], []), (), ())
    return p, (rd, rc, rk), n_t, m_t


def ragged_inputs(n_t, m_t, B=None, S=70):
    """padded (x1 [B, n], ū [B, T-1, m], candidates [B, S, T-1, m]): noise on the real entries only, candidate 0 exactly ū"""
    B = B_SWEEP if B is None else B
    n, m, N = max(n_t), max(m_t), len(m_t)
    rng = np.random.default_rng(5)
    x1 = np.zeros((B, n)); x1[:, :n_t[0]] = 0.5 * rng.standard_normal((B, n_t[0]))
    ub = np.zeros((B, N, m))
    for t in range(N):
        ub[:, t, :m_t[t]] = 0.2 * rng.standard_normal((B, m_t[t]))
    u = ub[:, None] + np.zeros((1, S, 1, 1))
    noise = 0.05 * np.random.default_rng(policy_ref.SEED + 1).standard_normal(u.shape)
    for t in range(N):
        u[:, 1:, t, :m_t[t]] += noise[:, 1:, t, :m_t[t]]
    return x1, ub, u


def ragged_starts(xb, n0, S=70):
    """x1 [B, S, n] around x̄_1, the real entries moved by 0.05 · N(0, 1), sample 0 exactly x̄_1"""
    starts = np.repeat(np.asarray(xb)[:, None, 0], S, axis=1)
    starts[:, 1:, :n0] += 0.05 * np.random.default_rng(policy_ref.SEED).standard_normal((starts.shape[0], S - 1, n0))
    return starts


def ragged_restatement_policy(B=None, T=T_RAGGED):
    """the restatement's solve of the ragged problem from ragged_inputs, padded: (x̄, ū, K, k), batched"""
    R = restatement()
    p, (rd, rc, rk), n_t, m_t = ragged(T)
    n, m = max(n_t), max(m_t)
    x1, ub, _ = ragged_inputs(n_t, m_t, B, 1)
    out = []
    for b in range(x1.shape[0]):
        s = R.Solver(rd, rc, rk)
        s.initialize_controls([ub[b, t, :m_t[t]] for t in range(T - 1)])
        s.initialize_states(R.rollout(rd, x1[b, :n_t[0]], [ub[b, t, :m_t[t]] for t in range(T - 1)]))
        s.solve()
        xb, us, K, k = np.zeros((T, n)), np.zeros((T - 1, m)), np.zeros((T - 1, n, m)), np.zeros((T - 1, m))
        for t in range(T):
            xb[t, :n_t[t]] = s.nominal_states[t]
        for t in range(T - 1):
            us[t, :m_t[t]] = s.nominal_actions[t]; k[t, :m_t[t]] = s.k[t]; K[t, :n_t[t], :m_t[t]] = s.K[t].T
        out.append((xb, us, K, k))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


# ------------------------------------------------------------------------------------------------- the inputs of the GPU sweep
T_SWEEP, B_SWEEP = 21, 3
# the perturbation of the starts and the candidates' noise. 0.5 is the scale of the sweep's x1 itself: a solved policy holds its
# saturated actions a hair inside the box with next to no gain on them, so a small move can leave every sample of a size feasible
# and the violation rule idle there (tests/test_mpc_ref.py asserts that 0.5 crosses the box at every size, and shows on the
# yardstick that 0.02 does not at (16, 16)). The synth dynamics contract (A ≈ −I), so every sample stays finite.
SIZE_X1, SIZE_U = 0.5, 0.2
SEED = 20261101
SMALL = [(1, 1), (4, 3), (2, 4)]
LARGE = [(5, 1), (9, 3), (16, 16), (17, 2), (32, 8), (33, 2), (40, 6), (64, 8)]
SIZES = SMALL + LARGE
SHIFTS = (1, 3)


def samples(n, m):
    """S: the small path runs one sample per lane (70: two waves, the second ragged), the large path one wave per sample"""
    return 70 if (n <= 4 and m <= 4) else 5


def module_name(n, m):
    """the names under which the solve kernels' sweeps compile the same models: one module cache"""
    return "synth%d" % n if n >= 40 else "sweep%d_%d" % (n, m)


def sweep_inputs(n, m, B=B_SWEEP, T=T_SWEEP):
    """(x1 [B, n], ū [B, T-1, m]) of test_dimension_sweep_against_the_independent_restatement: x1 = 0.5 z, ū = 0.4 z + 0.9, across
    the action box"""
    rng = np.random.default_rng(100 * n + m)
    return 0.5 * rng.standard_normal((B, n)), 0.4 * rng.standard_normal((B, T - 1, m)) + 0.9


def rollout_starts(xb, S, size=SIZE_X1):
    """x1 [B, S, n]: policy_ref.perturbed_starts around x̄_1 of every instance, sample 0 exactly x̄_1"""
    return np.stack([policy_ref.perturbed_starts(xb[b, 0], S, size, seed=policy_ref.SEED + b) for b in range(xb.shape[0])])


def candidate_set(ub, S, size=SIZE_U):
    """u [B, S, T-1, m] = ū + size · N(0, 1), candidate 0 exactly ū"""
    ub = np.asarray(ub, dtype=np.float64)
    u = ub[:, None] + size * np.random.default_rng([SEED, ub.shape[2]]).standard_normal((ub.shape[0], S) + ub.shape[1:])
    u[:, 0] = ub
    return u


def sigma(m, size=SIZE_U):
    """a different, non-zero size per action component"""
    return size * (1.0 + np.arange(m)) / m


def measured_starts(xb, steps, size=SIZE_X1):
    """x1 [B, n] of a shift by `steps`: shift_ref.measured_start around x̄_steps"""
    return np.stack([shift_ref.measured_start(xb[b, steps], size, b, steps) for b in range(xb.shape[0])])


def restatement_policy(n, m, B=B_SWEEP, T=T_SWEEP):
    """A solved policy of the sweep's inputs without a device: the restatement's solve per instance -> (x̄, ū, K, k), batched"""
    R = restatement()
    _, (dyn, costs, cons) = synth(T, n, m)
    x1, ub = sweep_inputs(n, m, B, T)
    out = []
    for b in range(B):
        s = R.Solver(dyn, costs, cons)
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dyn, x1[b], ub[b]))
        s.solve()
        out.append((np.stack(s.nominal_states), np.stack(s.nominal_actions[:-1]), np.stack([Kt.T for Kt in s.K]), np.stack(s.k)))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))
