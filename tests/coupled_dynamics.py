"""A problem family whose DYNAMICS couple the states nonlinearly (TEST INFRASTRUCTURE), the dynamics counterpart of
tests/coupled_problem.py. Every other large-path model of the suite has the synth dynamics x⁺ = x + h(Ax + Bu + 0.1 sin x) (synth12
adds 0.02 x_i u_{i mod m}): the state-dependent entries of ∂f/∂x lie on the diagonal and the nonlinear remainder of row i reads no
state but x_i. Here row i is

    x⁺_i = x_i + h[(Ax)_i + (Bu)_i + 0.1 sin x_i + C1 sin(x_i − x_{s(i)}) + C2 x_{r(i)} u_{i mod m}],   h = 0.05,
    s(i) = (i + 1 + n // 3) mod n,   r(i) = (i + n − 1) mod n

with A and B of models.synth_nm. The state-dependent entries of ∂f/∂x are then the n diagonal ones, (i, s(i)) — a trig argument
that is an affine form of two states — and (i, r(i)), which depends on u and on nothing else; those of ∂f/∂u are (i, i mod m). The
off-diagonal set is not closed under transposition, and for n > 16 it spans several 16 x 16 tiles. Costs and the action box are the
synth family's: this family is about the dynamics.

The dynamics are stated ONCE as plain arithmetic on sequences with the sine passed in, and read three ways: symbolically (sympy.sin:
the product's Dynamics and the restatement's), numerically (math.sin / numpy.sin: the yardsticks mpc_ref, plant_ref, plant_io_ref,
estimator_ref) and on complex states (numpy.sin: estimator_ref.jacobian's complex-step derivative).

C1, C2, the seeds and the scales are problem data, chosen on the CPU so that the restatement's solves have the properties
tests/test_coupled_dynamics.py asserts; they are not tolerances. C1 = 0.08 and C2 = 0.03 are the values the family was proposed with."""
import math

import numpy as np

H, C1, C2 = 0.05, 0.08, 0.03
XG = 0.5
T, BATCH, BATCH_MPC = 11, 5, 3      # five instances for the solves and stages, three for the MPC-side and filter kernels
# (5, 2) the first large size, one tile; (12, 5) one tile that is no multiple of 16 (the one-wave `mid` variant exists); (17, 3) odd,
# two tiles, split rows, dense JAC_NVAR = 340 > 256; (33, 2) unsplit rows, three tiles, mask word 1
SIZES = [(5, 2), (12, 5), (17, 3), (33, 2)]
C_SIZES = [(12, 5), (17, 3)]        # the sizes that also go the C-callable route, probed and dense
MPC_SIZES = [(5, 2), (17, 3), (33, 2)]
IDS = ["%dx%d" % nm for nm in SIZES]


def s_of(i, n):
    """the state row i is coupled to inside the sine"""
    return (i + 1 + n // 3) % n


def r_of(i, n):
    """the state row i multiplies its action with"""
    return (i + n - 1) % n


def tables(n, m):
    A = [[(-1.0 if i == j else 0.0) + 0.3 * math.cos(float((i + 1) + 2 * (j + 1))) / float(n) for j in range(n)] for i in range(n)]
    Bm = [[math.sin(float(3 * (i + 1) + (j + 1))) / math.sqrt(float(n)) for j in range(m)] for i in range(n)]
    return A, Bm


def dynamics(n, m, sin):
    """f(x, u) -> list of n entries; x, u any sequences of numbers or symbols, sin the sine that fits them"""
    A, Bm = tables(n, m)

    def f(x, u):
        out = []
        for i in range(n):
            acc = 0.0
            for j in range(n):
                acc = acc + A[i][j] * x[j]
            for j in range(m):
                acc = acc + Bm[i][j] * u[j]
            acc = acc + 0.1 * sin(x[i]) + C1 * sin(x[i] - x[s_of(i, n)]) + C2 * x[r_of(i, n)] * u[i % m]
            out.append(x[i] + H * acc)
        return out
    return f


def stage_cost(x, u):
    return 0.1 * sum((xi - XG) * (xi - XG) for xi in x) + 0.01 * sum(uj * uj for uj in u)


def terminal_cost(x, u):
    return 10.0 * sum((xi - XG) * (xi - XG) for xi in x)


def box(m):
    return (lambda x, u: [-1.0 - u[j] for j in range(m)] + [u[j] - 1.0 for j in range(m)]), list(range(1, 2 * m + 1))


def name(n, m):
    return "cdyn%d_%d" % (n, m)


# ------------------------------------------------------------------------------------------ the three readers
_NUMPY, _RESTATEMENT = {}, {}


def numpy_f(n, m):
    """f(x, u, w, t) -> ndarray, the form of mpc_ref / plant_ref; takes complex states"""
    if (n, m) not in _NUMPY:
        f = dynamics(n, m, np.sin)
        _NUMPY[(n, m)] = lambda x, u, w, t: np.array(f(x, u))
    return _NUMPY[(n, m)]


def register_yardstick(n, m):
    """make the family known to plant_ref.dynamics (and so to estimator_ref.predict / jacobian) under its module name"""
    import plant_ref
    plant_ref._F[name(n, m)] = numpy_f(n, m)
    return name(n, m)


def mpc_problem(n, m):
    """mpc_ref.Problem over plain numbers"""
    import mpc_ref
    rows, _ = box(m)
    return mpc_ref.Problem(numpy_f(n, m), lambda x, u, w, t: stage_cost(x, u), lambda x, u, w, t: terminal_cost(x, u),
                           lambda x, u, w, t: np.array(rows(x, u)), None, tuple(range(2 * m)), ())


def restatement_problem(R, n, m, T=T):
    """(dynamics, costs, constraints) for reference_restatement.Solver; the objects are built once per size"""
    import sympy as sp
    if (n, m) not in _RESTATEMENT:
        rows, ineq = box(m)
        _RESTATEMENT[(n, m)] = (R.Dynamics(dynamics(n, m, sp.sin), n, m), R.Cost(stage_cost, n, m), R.Cost(terminal_cost, n, 0),
                                R.Constraint(rows, n, m, indices_inequality=ineq))
    d, cs, ct, con = _RESTATEMENT[(n, m)]
    return [d] * (T - 1), [cs] * (T - 1) + [ct], [con] * (T - 1) + [R.Constraint()]


def product_objects(pkg, n, m):
    """dict(dynamics, cost_stage, cost_term, con_stage) of the product's symbolic objects"""
    import sympy as sp
    rows, ineq = box(m)
    return dict(dynamics=pkg.Dynamics(dynamics(n, m, sp.sin), n, m), cost_stage=pkg.Cost(stage_cost, n, m),
                cost_term=pkg.Cost(terminal_cost, n, 0), con_stage=pkg.Constraint(rows, n, m, indices_inequality=ineq))


def product_problem(pkg, n, m, T=T):
    """(dynamics, costs, constraints, name) for the product's Solver"""
    o = product_objects(pkg, n, m)
    return [o["dynamics"]] * (T - 1), [o["cost_stage"]] * (T - 1) + [o["cost_term"]], [o["con_stage"]] * (T - 1) + [pkg.Constraint()], name(n, m)


def c_source(pkg, n, m):
    """the family as C callables for ilqr_compile_model, printed from the same symbolic objects"""
    o, cg = product_objects(pkg, n, m), pkg.codegen
    return (cg.c_dynamics("dynamics", o["dynamics"]) + cg.c_cost("cost_stage", o["cost_stage"]) +
            cg.c_cost("cost_terminal", o["cost_term"], terminal=True) + cg.c_constraint("constraint_stage", o["con_stage"]))


def c_dims(n, m):
    """(nx, nu, nw, nc_stage, nc_term, ineq_stage, ineq_term) of ilqr_model_source"""
    return (n, m, 0, 2 * m, 0, (1 << (2 * m)) - 1, 0)


def structure(n, m):
    """(fx set, fu set) of the state-dependent Jacobian entries, as (row, column) pairs, from the family's definition"""
    fx = {(i, i) for i in range(n)} | {(i, s_of(i, n)) for i in range(n)} | {(i, r_of(i, n)) for i in range(n)}
    return fx, {(i, i % m) for i in range(n)}


# ------------------------------------------------------------------------------------------ inputs
# seed per size, searched on the CPU for the properties tests/test_coupled_dynamics.py asserts of the restatement's solves
SEEDS = {(5, 2): 1, (12, 5): 1, (17, 3): 1, (33, 2): 1}
SCALE_X, SCALE_U, SHIFT_U = 0.5, 0.4, 0.5          # x1 = 0.5 z, ū = 0.4 z + 0.5: a good part of the plan starts outside the action box


def inputs(n, m, batch=BATCH, T=T):
    """x1 [B, n], ū [B, T−1, m]; the first BATCH_MPC instances of the batch of five are the batch of three"""
    rng = np.random.default_rng([SEEDS[(n, m)], n, m])
    x1, ub = SCALE_X * rng.standard_normal((BATCH, n)), SCALE_U * rng.standard_normal((BATCH, T - 1, m)) + SHIFT_U
    return x1[:batch], ub[:batch]


def restatement_solve(R, problem, x1, ub):
    dyn, costs, cons = problem
    s = R.Solver(dyn, costs, cons)
    s.initialize_controls(ub); s.initialize_states(R.rollout(dyn, x1, ub))
    s.solve()
    return s


def stage_round(R, n, m, it):
    """nominal trajectory number `it` of the linearisation test: (x [B, T, n], u [B, T-1, m]), a rollout of moved inputs"""
    dyn = restatement_problem(R, n, m)[0]
    x1, ub = inputs(n, m)
    us = [ub[b] * (1.0 - 0.5 * it) + 0.25 * it * np.sin(1.0 + it + np.arange(ub[b].size).reshape(ub[b].shape)) for b in range(BATCH)]
    xs = [np.stack(R.rollout(dyn, x1[b] * (1.0 - 0.2 * it), us[b])) for b in range(BATCH)]
    return np.stack(xs), np.stack(us)


def restatement_policy(R, n, m, B=BATCH_MPC):
    """a solved policy of the inputs without a device -> (x̄, ū, K, k), batched, in the layout of get_trajectory / get_policy"""
    pr = restatement_problem(R, n, m)
    x1, ub = inputs(n, m, B)
    out = []
    for b in range(B):
        s = restatement_solve(R, pr, x1[b], ub[b])
        out.append((np.stack(s.nominal_states), np.stack(s.nominal_actions[:-1]), np.stack([Kt.T for Kt in s.K]), np.stack(s.k)))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def control_flow(s):
    """(iterations, outer iterations, rollouts, the accepted step size of every inner iteration)"""
    return s.iterations, s.outer_iterations, s.rollouts, tuple(row[5] for row in s.trace)


# limits of the filter tests: (u_min, u_max) per size — a component clamped from each side and one left alone where there are
# three; tests/test_coupled_dynamics.py asserts on the yardstick that they bind and that no raw action lies within
# plant_io_ref.MARGIN of a limit
INF = float("inf")
LIMITS = {(5, 2): (np.array([-INF, -0.2]), np.array([0.6, INF])),
          (17, 3): (np.array([-INF, -0.2, -INF]), np.array([0.6, INF, INF])),
          (33, 2): (np.array([-INF, -0.2]), np.array([0.6, INF]))}
