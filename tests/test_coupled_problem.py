"""The coupled-Hessian family of tests/coupled_problem.py, proven suitable on the CPU before tests/test_gpu_coupled_hessians.py
asserts any device number on it: what the independent restatement does on every size and input set the GPU module uses (every
factorisation succeeds, several inner and outer iterations, a rejected line-search trial, control flow that a relative 1e-13
perturbation of the inputs does not change), that the Hessians are what the family is for (a rectangular, non-symmetric gux; an
accumulated Hessian that is not k times one value; four gxx tiles at n = 17), and that the generator's and the host structure
probe's compact Hessian tables are the sparsity sets sympy gives for the same callables."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import sympy as sp

import coupled_problem as CP
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iterativelqr.jl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import reference_restatement as R  # noqa: E402

IDS = ["%dx%d-T%d%s" % (n, m, T, "" if con else "-unconstrained") for n, m, T, con in CP.CASES]


def _snapshot(store):
    def hook(s, outer, inner):
        store.setdefault((outer, inner), tuple(np.stack(h).copy() for h in (s.gxx[:-1], s.guu, s.gux)))
    return hook


@functools.lru_cache(maxsize=None)
def _solved(case):
    """the restatement's solves of a case, with the accumulated stage Hessians after the first two linearisations"""
    n, m, T, con = case
    pr = CP.restatement_problem(R, n, m, T, con)
    x1, ub = CP.inputs(n, m, T, con)
    out = []
    for b in range(CP.BATCH):
        snaps = {}
        s = CP.restatement_solve(R, pr, x1[b], ub[b], hooks={"after_backward": _snapshot(snaps)})
        out.append((s, snaps))
    return pr, x1, ub, out


@pytest.mark.parametrize("case", CP.CASES, ids=IDS)
def test_restatement_behaviour_on_the_gpu_inputs(case):
    con = case[3]
    _, _, _, out = _solved(case)
    for b, (s, _) in enumerate(out):
        assert s.potrf_info == 0, b
        assert s.iterations >= 3, (b, s.iterations)
        assert s.outer_iterations >= 2 if con else s.outer_iterations == 0, (b, s.outer_iterations)
        assert np.isfinite(s.objective)
    assert any(s.rollouts > s.iterations for s, _ in out)            # a rejected line-search trial somewhere in the batch


@pytest.mark.parametrize("case", CP.CASES, ids=IDS)
def test_control_flow_survives_a_relative_perturbation_of_1e_13(case):
    """what lets the GPU module demand the restatement's control flow on every instance"""
    pr, x1, ub, out = _solved(case)
    rng = np.random.default_rng(13)
    for b, (s, _) in enumerate(out):
        xp = x1[b] * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], size=x1[b].shape))
        up = ub[b] * (1.0 + 1e-13 * rng.choice([-1.0, 1.0], size=ub[b].shape))
        p = CP.restatement_solve(R, pr, xp, up)
        assert (p.iterations, p.outer_iterations, p.rollouts) == (s.iterations, s.outer_iterations, s.rollouts), b


@pytest.mark.parametrize("case", CP.CASES, ids=IDS)
def test_the_hessians_are_coupled_and_not_constant(case):
    n, m, T, con = case
    _, _, _, out = _solved(case)
    first = 1 if con else 0
    for b, (s, snaps) in enumerate(out):
        gux = np.stack(s.gux)                                        # [t][action][state]
        nz = np.abs(gux).max(0) > 0
        assert nz.any(1).sum() >= min(2, m) and nz.any(0).sum() >= 2, b
        if m >= 2:                                                   # (with one action the two layouts are the same list)
            device_layout = gux.transpose(0, 2, 1).reshape(T - 1, -1)            # nu x nx column-major blocks
            assert np.abs(device_layout - gux.reshape(T - 1, -1)).max() > 1e-3 * np.abs(gux).max(), b
        one, two = snaps[(first, 0)], snaps[(first, 1)]
        for name, h1, h2 in zip(("gxx", "guu", "gux"), one, two):
            assert np.abs(h2 - 2.0 * h1).max() > 1e-6 * np.abs(h1).max(), (b, name)
        if n == 17:
            gxx = np.stack(s.gxx[:-1])
            for rows in (slice(0, 16), slice(16, 17)):
                for cols in (slice(0, 16), slice(16, 17)):
                    assert np.abs(gxx[:, rows, cols]).max() > 0


# ------------------------------------------------------------------ the compact Hessian tables
def _sympy_structure(n, m):
    """(gxx set in tile order, guu set, gux set, tile starts) from sympy's Hessians of the family's callables and from the rows of
    its constraint Jacobians; indices are column-major inside each matrix (gux: column = state, row = action)"""
    x = [sp.Symbol("x%d" % i, real=True) for i in range(n)]
    u = [sp.Symbol("u%d" % i, real=True) for i in range(m)]
    ls, lt = sp.sympify(CP.stage_cost(n, m)(x, u)), sp.sympify(CP.terminal_cost(n)(x, u))
    rows, _ = CP.stage_rows(n, m)
    xx, uu, ux = set(), set(), set()
    for j in range(n):
        for i in range(n):
            if sp.diff(ls, x[i], x[j]) != 0 or sp.diff(lt, x[i], x[j]) != 0:
                xx.add(j * n + i)
    for j in range(m):
        for i in range(m):
            if sp.diff(ls, u[i], u[j]) != 0:
                uu.add(j * m + i)
    for j in range(n):
        for i in range(m):
            if sp.diff(ls, u[i], x[j]) != 0:
                ux.add(j * m + i)
    for c in rows(x, u):                       # Gauss-Newton terms: the variables of one row couple with each other
        c = sp.sympify(c)
        sx = [j for j in range(n) if sp.diff(c, x[j]) != 0]
        su = [j for j in range(m) if sp.diff(c, u[j]) != 0]
        xx.update(a * n + b for a in sx for b in sx)
        uu.update(a * m + b for a in su for b in su)
        ux.update(a * m + b for a in sx for b in su)
    tn = (n + 15) // 16
    tile = lambda e: ((e % n) // 16) * tn + (e // n) // 16
    xx = sorted(xx, key=lambda e: (tile(e), e))
    starts = [sum(1 for e in xx if tile(e) < q) for q in range(tn * tn + 1)]
    return xx, sorted(uu), sorted(ux), starts


def _table(src, name):
    return [int(v) for v in re.search(r"static constexpr int %s\[\d+\] = \{([^}]*)\};" % name, src).group(1).split(",")]


@pytest.mark.parametrize("nm", [(12, 5), (17, 3)])
def test_generated_compact_hessian_tables_are_the_sympy_sparsity_sets(nm):
    n, m = nm
    pkg = load_package()
    o = CP.product_objects(pkg, n, m)
    _, src = pkg.codegen.generate_model_source("coupled", o["dynamics"], o["cost_stage"], o["cost_term"], o["con_stage"], None)
    xx, uu, ux, starts = _sympy_structure(n, m)
    sizes = re.search(r"HESS_NXX = (\d+), HESS_NUU = (\d+), HESS_NUX = (\d+);", src)
    assert tuple(int(v) for v in sizes.groups()) == (len(xx), len(uu), len(ux))
    assert _table(src, "HESS_IDX") == xx + uu + ux
    assert _table(src, "HESS_XX_TILE_START") == starts
    assert len(ux) >= m + 1 and len(uu) > m and len(xx) > n          # something beside the diagonals, and a gux at all
    if n == 17:
        assert all(b > a for a, b in zip(starts, starts[1:]))        # every one of the four tiles holds entries


def test_host_structure_probe_finds_the_sympy_sparsity_sets(tmp_path):
    """the family as C callables (what ilqr_compile_model is given), probed by the host-only model compiler"""
    pkg = load_package()
    exe = str(tmp_path / "model_compile_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "model_compile_check.cpp"),
                           os.path.join(CSRC, "ilqr_model_compile.cpp"), "-o", exe, "-ldl"])
    scratch = tmp_path / "models"
    scratch.mkdir()
    args = []
    for n, m in ((12, 5), (17, 3)):
        xx, uu, ux, starts = _sympy_structure(n, m)
        source, expect = tmp_path / ("coupled%d.c" % n), tmp_path / ("coupled%d.txt" % n)
        source.write_text(CP.c_source(pkg, n, m))
        expect.write_text("%d %d %d\n%d %d %d\n%s\n%s\n" % (n, m, 2 * m + 2, len(xx), len(uu), len(ux), " ".join(map(str, xx + uu + ux)),
                                                           " ".join(map(str, starts))))
        args += [str(source), str(expect)]
    env = {k: v for k, v in os.environ.items() if k != "ILQR_NO_STRUCTURE_PROBE"}
    out = subprocess.run([exe, "--probe", str(scratch)] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d checks passed" % (len(lines) - 1) and len(lines) - 1 == 2 * 5
