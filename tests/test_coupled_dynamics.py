"""The coupled-dynamics family of tests/coupled_dynamics.py, proven suitable on the CPU before tests/test_gpu_coupled_dynamics.py
asserts any device number on it: the generator's and the host structure probe's state-dependent Jacobian sets are the ones sympy
gives (n diagonal entries, 2n off-diagonal ones that span several tiles for n > 16 and are not closed under transposition, n entries
of fu; neither the Jacobian patch nor the remainder elementwise); the two references agree (complex step against the restatement's
sympy Jacobian); every patched off-diagonal entry is large enough and moves enough to be seen; the restatement's control flow does
not change under a relative perturbation of 1e-13; the limits of the filter tests bind; and the yardsticks of the MPC-side and
filter quantities keep everything finite and move, under a change of their inputs by one part in 1e15, by less than a tenth of the
bounds the GPU module holds the device to (printed with pytest -s, recorded in that module's docstring)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import sympy as sp

import coupled_dynamics as CD
import estimator_ref as E
import mpc_ref as M
import plant_io_ref as IO
import plant_ref as PR
import policy_ref as P
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iterativelqr.jl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import reference_restatement as R  # noqa: E402

TOL_XU, TOL_COST, TOL_VIOL, TOL_EST = 1e-10, 1e-9, 1e-9, 1e-10      # the bounds of test_gpu_mpc_sweep.py, test_gpu_plant_io.py, test_gpu_estimator.py
MPC_IDS = ["%dx%d" % nm for nm in CD.MPC_SIZES]


# ------------------------------------------------------------------ the state-dependent Jacobian sets
@functools.lru_cache(maxsize=None)
def _sympy_sets(n, m):
    """(fx, fu): the (row, column) pairs whose derivative still holds a symbol"""
    x = [sp.Symbol("x%d" % i, real=True) for i in range(n)]
    u = [sp.Symbol("u%d" % i, real=True) for i in range(m)]
    y = [sp.sympify(e) for e in CD.dynamics(n, m, sp.sin)(x, u)]
    fx = {(i, j) for i in range(n) for j in range(n) if sp.diff(y[i], x[j]).free_symbols}
    fu = {(i, j) for i in range(n) for j in range(m) if sp.diff(y[i], u[j]).free_symbols}
    return fx, fu


def _indices(n, fx, fu):
    """the sets as indices into [fx (n·n) | fu (n·m)], both column-major, ascending"""
    return sorted(c * n + r for r, c in fx) + sorted(n * n + c * n + r for r, c in fu)


@functools.lru_cache(maxsize=None)
def _generated(n, m):
    pkg = load_package()
    o = CD.product_objects(pkg, n, m)
    return pkg.codegen.generate_model_source("cdyn", o["dynamics"], o["cost_stage"], o["cost_term"], o["con_stage"], None)[1]


def _table(src, name):
    return [int(v) for v in re.search(r"static constexpr int %s\[\d+\] = \{([^}]*)\};" % name, src).group(1).split(",")]


@pytest.mark.parametrize("nm", CD.SIZES, ids=CD.IDS)
def test_generated_jacobian_structure_is_the_sympy_set(nm):
    n, m = nm
    fx, fu = _sympy_sets(n, m)
    assert (fx, fu) == CD.structure(n, m)
    off = {(r, c) for r, c in fx if r != c}
    assert len(fx) == 3 * n and len(off) == 2 * n and len(fu) == n
    assert off == {(i, CD.s_of(i, n)) for i in range(n)} | {(i, CD.r_of(i, n)) for i in range(n)}
    assert {(c, r) for r, c in off} != off and not all((c, r) in off for r, c in off)        # not closed under transposition
    tiles = {(r // 16, c // 16) for r, c in off}
    assert len(tiles) > 1 if n > 16 else tiles == {(0, 0)}
    if n == 17:
        assert tiles == {(0, 0), (0, 1), (1, 0)}
    src = _generated(n, m)
    assert "JAC_VAR_ELEMENTWISE = false;" in src and "DYN_REM_ELEMENTWISE = false;" in src
    assert int(re.search(r"JAC_NVAR = (\d+);", src).group(1)) == 4 * n
    idx = _table(src, "JAC_VAR_IDX")
    assert sorted(i for i in idx if i < n * n) == _indices(n, fx, set()) and sorted(i for i in idx if i >= n * n) == _indices(n, set(), fu)
    assert len(idx) == len(set(idx)) == 4 * n


def test_host_structure_probe_finds_the_jacobian_sets(tmp_path):
    """the family as C callables (what ilqr_compile_model is given), probed by the host-only model compiler: the state-dependent
    Jacobian entries are sympy's, and the compact Hessian row is the cost's two diagonals"""
    pkg = load_package()
    exe = str(tmp_path / "model_compile_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "model_compile_check.cpp"),
                           os.path.join(CSRC, "ilqr_model_compile.cpp"), "-o", exe, "-ldl"])
    scratch = tmp_path / "models"
    scratch.mkdir()
    args = []
    for n, m in CD.C_SIZES:
        fx, fu = _sympy_sets(n, m)
        tn = (n + 15) // 16
        tile = lambda e: ((e % n) // 16) * tn + (e // n) // 16
        xx = sorted((j * n + j for j in range(n)), key=lambda e: (tile(e), e))
        starts = [sum(1 for e in xx if tile(e) < q) for q in range(tn * tn + 1)]
        uu = [j * m + j for j in range(m)]
        source, expect = tmp_path / ("cdyn%d.c" % n), tmp_path / ("cdyn%d.txt" % n)
        source.write_text(CD.c_source(pkg, n, m))
        expect.write_text("%d %d %d\n%d %d 0\n%s\n%s\n%s\n" % (n, m, 2 * m, n, m, " ".join(map(str, xx + uu)), " ".join(map(str, starts)),
                                                             " ".join(map(str, _indices(n, fx, fu)))))
        args += [str(source), str(expect)]
    env = {k: v for k, v in os.environ.items() if k != "ILQR_NO_STRUCTURE_PROBE"}
    out = subprocess.run([exe, "--probe", str(scratch)] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d checks passed" % (len(lines) - 1) and len(lines) - 1 == 2 * 6


# ------------------------------------------------------------------ the two references agree
@pytest.mark.parametrize("nm", CD.SIZES, ids=CD.IDS)
def test_complex_step_jacobian_is_the_restatements(nm):
    """estimator_ref.jacobian over the numpy callable against the restatement's sympy Jacobian at random points: neither is the code
    under test, and the family's one text reads the same all three ways"""
    n, m = nm
    name = CD.register_yardstick(n, m)
    d = CD.restatement_problem(R, n, m)[0][0]
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(4):
        x, u = rng.standard_normal(n), rng.standard_normal(m)
        Fc, Fs = E.jacobian(name, x, u, M._NONE), d.jacobian_state(x, u, [])
        worst = max(worst, np.abs(Fc - Fs).max() / np.abs(Fs).max())
        # (sympy reorders the n + m + 3 terms of a row: a few roundings of 2^-53 |y| each)
        assert np.abs(np.asarray(PR.dynamics(name)(x, u, M._NONE, 0)) - d.evaluate(x, u, [])).max() < 1e-14
    print("coupled-dynamics %dx%d complex step against sympy: %.2e" % (n, m, worst))
    assert worst < 1e-15


# ------------------------------------------------------------------ the inputs of the GPU module
@pytest.mark.parametrize("nm", CD.SIZES, ids=CD.IDS)
def test_every_patched_off_diagonal_entry_matters(nm):
    """At the trajectories the linearisation test compares: every patched off-diagonal entry of fx reaches 1e-4, which is seven
    orders above the bound it is held to, and moves along the horizon by more than 1e-7 (every time step is compared); the (i, r(i))
    entries, which depend on u alone, differ between the two rounds' actions at the same states. A patch that lands anywhere else, or that is
    computed from a stale x or u, moves an entry by far more than the bound."""
    n, m = nm
    d = CD.restatement_problem(R, n, m)[0][0]
    (xa, ua), (_, ub) = CD.stage_round(R, n, m, 0), CD.stage_round(R, n, m, 1)
    steps = range(CD.T - 1)
    for b in range(CD.BATCH):
        F = np.stack([d.jacobian_state(xa[b, t], ua[b, t], []) for t in steps])
        Fu = np.stack([d.jacobian_state(xa[b, t], ub[b, t], []) for t in steps])             # the same states, the other round's actions
        for i in range(n):
            s, r = CD.s_of(i, n), CD.r_of(i, n)
            assert np.abs(F[:, i, s]).max() >= 1e-4 and np.abs(F[:, i, r]).max() >= 1e-4, (b, i)
            assert F[:, i, s].max() - F[:, i, s].min() > 1e-7 and F[:, i, r].max() - F[:, i, r].min() > 1e-7, (b, i)
            assert np.abs(F[:, i, r] - Fu[:, i, r]).max() > 1e-7 and np.array_equal(Fu[:, i, s], F[:, i, s]), (b, i)
        assert np.abs(F[0] - F[0].T).max() > 1e-3


@functools.lru_cache(maxsize=None)
def _solved(n, m):
    pr = CD.restatement_problem(R, n, m)
    x1, ub = CD.inputs(n, m)
    return pr, x1, ub, [CD.restatement_solve(R, pr, x1[b], ub[b]) for b in range(CD.BATCH)]


@pytest.mark.parametrize("nm", CD.SIZES, ids=CD.IDS)
def test_control_flow_survives_a_relative_perturbation_of_1e_13(nm):
    """what lets the GPU module demand the restatement's control flow on every instance: iterations, outer iterations, rollouts and
    every accepted step size. One instance at least rejects a line-search trial and ends with a positive dual on a box row."""
    pr, x1, ub, out = _solved(*nm)
    rng = np.random.default_rng(13)
    both = False
    for b, s in enumerate(out):
        assert s.potrf_info == 0 and s.iterations >= 3 and s.outer_iterations >= 1 and np.isfinite(s.objective), b
        xp = x1[b] * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], size=x1[b].shape))
        up = ub[b] * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], size=ub[b].shape))
        assert CD.control_flow(CD.restatement_solve(R, pr, xp, up)) == CD.control_flow(s), b
        both = both or (s.rollouts > s.iterations and max(float(lam.max()) for lam in s.constraint_dual[:-1]) > 0.0)
    assert both
    assert (np.abs(ub) > 1.0).any()


# ------------------------------------------------------------------ the yardsticks of the MPC-side and filter quantities
def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("nm", CD.MPC_SIZES, ids=MPC_IDS)
def test_the_mpc_side_inputs_are_finite_and_the_bounds_stand(nm):
    n, m = nm
    B, S, T = CD.BATCH_MPC, 5, CD.T
    name = CD.register_yardstick(n, m)
    f, p = PR.dynamics(name), CD.mpc_problem(n, m)
    x1, ub0 = CD.inputs(n, m, B)
    xb, ub, K, k = CD.restatement_policy(R, n, m)
    assert np.array_equal(xb[:, 0], x1) and np.isfinite(K).all() and np.abs(k).max() > 0.0
    starts, cands = M.rollout_starts(xb, S), M.candidate_set(ub0, S)
    worst = dict(policy=0.0, cost=0.0, viol=0.0, shift=0.0, plant=0.0, predict=0.0)
    violated = False
    for b in range(B):
        for alpha in (0.0, 0.5):
            for s in range(S):
                r = M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], starts[b, s], alpha, None)
                assert r["first_nonfinite"] == -1 and np.isfinite([r["cost"], r["max_violation"]]).all(), (nm, b, s)
                violated |= r["max_violation"] > 0
            sp_ = M.spread(p, xb[b], ub[b], K[b], k[b], starts[b], alpha)
            worst["policy"], worst["cost"], worst["viol"] = max(worst["policy"], sp_["xu"]), max(worst["cost"], sp_["cost"]), max(worst["viol"], sp_["viol"])
        sc = M.score_all(p, x1[b], cands[b])
        assert (sc["first_nonfinite"] == -1).all() and np.isfinite(sc["cost"]).all() and np.isfinite(sc["max_violation"]).all(), (nm, b)
        sp_ = M.score_spread(p, x1[b], cands[b])
        worst["cost"], worst["viol"] = max(worst["cost"], sp_["cost"]), max(worst["viol"], sp_["viol"])
        for steps in M.SHIFTS:
            start = M.measured_starts(xb, steps)[b]
            r = M.shift_head(p, xb[b], ub[b], K[b], None, steps, start)
            assert r["first_nonfinite"] == -1 and np.abs(r["u"] - ub[b, steps:]).max() > 1e-6, (nm, b, steps)
            worst["shift"] = max(worst["shift"], M.spread(p, xb[b, steps:], ub[b, steps:], K[b, steps:], np.zeros_like(ub[b, steps:]), [start])["xu"])
    assert violated
    # the plant step and the filter's time update, with the limits: they bind, and not by a hair
    u_min, u_max = CD.LIMITS[nm]
    x0 = PR.plant_starts(xb)
    xh, _ = E.start(x0, n)
    Ps = E.p_start(B, n)
    z = np.random.default_rng(3).standard_normal((B,) + PR.noise_shape(n, 0, 3))
    kw = dict(u_min=u_min, u_max=u_max)
    refs, seen = [], 0.0
    for b in range(B):
        one = IO.plant_step(f, xb[b], ub[b], K[b], None, xh[b], 1, True, **kw)
        if one["saturated"]:                      # what a Jacobian taken at the RAW action would do to P after one step
            Fr, Fc = E.jacobian(name, xh[b], one["raw"][0], M._NONE), E.jacobian(name, xh[b], one["u"][0], M._NONE)
            seen = max(seen, P.rel(Fr @ Ps[b] @ Fr.T, Fc @ Ps[b] @ Fc.T))
        a = IO.plant_step(f, xb[b], ub[b], K[b], None, x0[b], 3, True, PR.sigma_x(n), z[b], 0, None, **kw)
        c = IO.plant_step(f, xb[b], ub[b], K[b], None, x0[b] * (1.0 + 1.0e-15), 3, True, PR.sigma_x(n), z[b], 0, None, **kw)
        assert a["first_nonfinite"] == -1
        worst["plant"] = max(worst["plant"], P.rel(c["x"], a["x"]), P.rel(c["u"], a["u"]))
        for steps, fb in ((1, True), (3, True), (3, False)):
            refs.append([IO.plant_step(f, xb[b], ub[b], K[b], None, xh[b], steps, fb, **kw)])
            xa, Pa = E.predict(name, xb[b], ub[b], K[b], None, xh[b], Ps[b], steps, fb, q=E.q(n), **kw)
            xc, Pc = E.predict(name, xb[b], ub[b], K[b], None, xh[b] * (1.0 + 1.0e-15), Ps[b] * (1.0 + 1.0e-15), steps, fb, q=E.q(n), **kw)
            assert np.isfinite(xa).all() and np.isfinite(Pa).all() and np.array_equal(Pa, Pa.T)
            worst["predict"] = max(worst["predict"], P.rel(xc, xa), P.rel(Pc, Pa))
    low, high, alone, nearest = IO.conditions(refs, u_min, u_max)
    assert low and high and alone and nearest > IO.MARGIN, (low, high, alone, nearest)
    print("coupled-dynamics spread %dx%d: %s | nearest raw action to a limit %.1e | P under F at the raw action %.1e" %
          (n, m, ", ".join("%s %.1e" % kv for kv in sorted(worst.items())), nearest, seen))
    assert seen > 100.0 * TOL_EST                 # an unclamped u handed to the filter's Jacobian cannot hide under the bound
    assert 10.0 * max(worst["policy"], worst["shift"], worst["plant"]) < TOL_XU
    assert 10.0 * worst["cost"] < TOL_COST and 10.0 * worst["viol"] < TOL_VIOL
    assert 10.0 * worst["predict"] < TOL_EST
