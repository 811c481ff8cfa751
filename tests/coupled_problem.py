"""A problem family whose cost Hessians are coupled and depend on the state and the action (TEST INFRASTRUCTURE), stated once as
plain callables f(x, u) that both the product's symbolic constructors (Cost / Constraint of iterativelqr.jl_amd/codegen.py) and the
independent restatement's (tests/golden/reference_restatement.py) accept.

The dynamics are the synth family's (models.synth_nm / reference_restatement.synth32_problem; tests/coupled_dynamics.py is the
family with coupled DYNAMICS), the base cost is theirs
(0.1 Σ(x_i − x_g)² + 0.01 Σ u_j², terminal 10 Σ(x_i − x_g)²) and the base constraint is the action box. On top, each a convex
function of an affine form (so the cost Hessian stays positive semidefinite and 0.01·I keeps Quu factorable), except the small
bilinear e·u_0·u_{m−1}, which the 2(0.01 + a) on the diagonal of guu dominates:

    a Σ_j (u_j − κ x_{p(j)})²                constant gux, one entry per row (rectangular, not symmetric)
    b Σ_{(i,k)} (x_i − x_k)⁴                 state-dependent off-diagonal gxx; (0, n−1) lies in tiles (0,1) and (1,0) for n > 16
    d Σ_j (u_j + κ₂ x_{q(j)})⁴               guu, gux, gxx that depend on x and u
    e u_0 u_{m−1}   (m ≥ 2)                  off-diagonal guu
    f (x_0 − x_{n−1})⁴   (terminal)          off-diagonal terminal gxx
    |u_0 − 0.5 x_1| ≤ BAND  beside the box   two coupled inequality rows: Gauss-Newton AL term cuᵀ Iρ cx in gux and off the
                                             diagonals; a band rather than one far row, so that one of the two binds at the solution

The coefficients are problem data (chosen on the CPU so that the restatement's solves have the properties
tests/test_coupled_problem.py asserts), not tolerances."""
import numpy as np

XG = 0.5
A, KAPPA, B4, D4, KAPPA2, E, F = 0.05, 0.7, 0.02, 0.03, 0.5, 0.005, 2.0
BAND = 0.05

T, BATCH = 11, 5                    # five instances: one full pack of four and a ragged one
# (n, m, T, constrained): every size the GPU module runs; the small path takes n, m <= 4
SMALL = [(2, 1, 11, True), (3, 2, 11, True), (2, 3, 11, True), (4, 4, 11, True), (3, 2, 10, True), (3, 2, 11, False)]
LARGE = [(5, 2, 11, True), (12, 5, 11, True), (16, 16, 11, True), (17, 3, 11, True)]
CASES = SMALL + LARGE


def p_of(j, n):
    """state that action j is tied to in the quadratic coupling"""
    return j % n


def q_of(j, n):
    """state that action j is tied to in the quartic coupling"""
    return (n - 1 - j) % n


def pairs(n):
    """state pairs of the quartic difference term: a neighbouring pair, (0, n−1), and one from the middle; never i == k"""
    out = []
    for i, k in ((0, 1), (0, n - 1), (n // 2, n - 1)):
        if i != k and (i, k) not in out:
            out.append((i, k))
    return out


def stage_cost(n, m):
    def f(x, u):
        J = 0.1 * sum((xi - XG) * (xi - XG) for xi in x) + 0.01 * sum(uj * uj for uj in u)
        J = J + A * sum((u[j] - KAPPA * x[p_of(j, n)]) ** 2 for j in range(m))
        J = J + B4 * sum((x[i] - x[k]) ** 4 for i, k in pairs(n))
        J = J + D4 * sum((u[j] + KAPPA2 * x[q_of(j, n)]) ** 4 for j in range(m))
        if m >= 2:
            J = J + E * u[0] * u[m - 1]
        return J
    return f


def terminal_cost(n):
    def f(x, u):
        return 10.0 * sum((xi - XG) * (xi - XG) for xi in x) + F * (x[0] - x[n - 1]) ** 4
    return f


def stage_rows(n, m):
    """the action box and the two coupled rows of the band; all 2 m + 2 rows are inequalities"""
    def f(x, u):
        return ([-1.0 - u[j] for j in range(m)] + [u[j] - 1.0 for j in range(m)] +
                [u[0] - 0.5 * x[1] - BAND, 0.5 * x[1] - u[0] - BAND])
    return f, list(range(1, 2 * m + 3))


def restatement_problem(R, n, m, T, constrained=True):
    """(dynamics, costs, constraints or None) for reference_restatement.Solver"""
    dyn = R.synth32_problem(T, n, m)[0]
    costs = [R.Cost(stage_cost(n, m), n, m)] * (T - 1) + [R.Cost(terminal_cost(n), n, 0)]
    if not constrained:
        return dyn, costs, None
    rows, ineq = stage_rows(n, m)
    return dyn, costs, [R.Constraint(rows, n, m, indices_inequality=ineq)] * (T - 1) + [R.Constraint()]


def product_objects(pkg, n, m, constrained=True):
    """dict(dynamics, cost_stage, cost_term, con_stage) of the product's symbolic objects (con_stage None when unconstrained)"""
    rows, ineq = stage_rows(n, m)
    return dict(dynamics=pkg.models.synth_nm(n, m)["dynamics"], cost_stage=pkg.Cost(stage_cost(n, m), n, m),
                cost_term=pkg.Cost(terminal_cost(n), n, 0),
                con_stage=pkg.Constraint(rows, n, m, indices_inequality=ineq) if constrained else None)


def product_problem(pkg, n, m, T, constrained=True):
    """(dynamics, costs, constraints or None, name) for the product's Solver"""
    o = product_objects(pkg, n, m, constrained)
    cons = [o["con_stage"]] * (T - 1) + [pkg.Constraint()] if constrained else None
    return [o["dynamics"]] * (T - 1), [o["cost_stage"]] * (T - 1) + [o["cost_term"]], cons, "coupled%d_%d%s" % (n, m, "" if constrained else "u")


def c_source(pkg, n, m):
    """the constrained family as C callables for ilqr_compile_model, printed from the same symbolic objects"""
    o, cg = product_objects(pkg, n, m), pkg.codegen
    return (cg.c_dynamics("dynamics", o["dynamics"]) + cg.c_cost("cost_stage", o["cost_stage"]) +
            cg.c_cost("cost_terminal", o["cost_term"], terminal=True) + cg.c_constraint("constraint_stage", o["con_stage"]))


# seed and scales (x1, ū) per case, searched on the CPU for the properties tests/test_coupled_problem.py asserts of the restatement's solves
SEEDS = {(2, 1, 11, True): 2}
SCALES = {True: (0.5, 0.3), False: (0.8, 0.8)}      # without the box and the band only wide starts make the line search reject a trial
UNCONSTRAINED_SEED = 3


def inputs(n, m, T, constrained=True, batch=BATCH):
    """x1 [B, n], ū [B, T−1, m]: most instances start outside the band |u_0 − 0.5 x_1| <= BAND, so the coupled rows are active from
    the first linearisation on"""
    rng = np.random.default_rng(SEEDS.get((n, m, T, constrained), 1) if constrained else UNCONSTRAINED_SEED)
    xs, us = SCALES[constrained]
    return xs * rng.standard_normal((batch, n)), us * rng.standard_normal((batch, T - 1, m))


def restatement_solve(R, problem, x1, ub, hooks=None):
    dyn, costs, cons = problem
    s = R.Solver(dyn, costs, cons)
    if hooks:
        s.hooks.update(hooks)
    s.initialize_controls(ub); s.initialize_states(R.rollout(dyn, x1, ub))
    s.solve()
    return s
