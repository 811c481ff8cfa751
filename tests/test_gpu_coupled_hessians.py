"""GPU: coupled and state-dependent cost Hessians on every kernel family, against the independent restatement run live.

Every other model of the GPU suite has diagonal, constant cost Hessians and (one equality row of car_tv aside) a zero gux (the
dynamics counterpart, state-coupled Jacobians, is tests/test_gpu_coupled_dynamics.py). The
family of tests/coupled_problem.py has a rectangular gux, off-diagonal gxx / guu, Hessians that depend on x and u (so that the
reference's accumulation, hessian[t] .+= ..., src/costs.jl:74-80, SURVEY quirk Q1, is not "k times one number"), an off-diagonal
terminal gxx and two coupled inequality rows whose Gauss-Newton term cuᵀ Iρ cx lands in gux (src/gradients.jl:79).
tests/test_coupled_problem.py proves the inputs suitable on the CPU, including that the restatement's control flow does not
change under a relative perturbation of 1e-13 — which is why control flow is demanded exact on every instance here.

Bars, the project's own (header of tests/test_gpu_parity.py): 2e-11 relative for the linearisation outputs, 1e-9 relative for
one Riccati pass from identical inputs (test_large_path_odd_dimensions_and_terminal_constraint); whole solve as
test_dimension_sweep_against_the_independent_restatement: iterations and outer iterations equal on every instance, |Δx|, |Δu| < 1e-8,
|ΔK| <= 1e-7 max(1, |K|), objective to 1e-9 relative, and the final accumulated Hessians to 1e-8 relative. gux is compared
element by element in its documented layout (nu x nx column-major blocks: [t][state][action])."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import coupled_problem as CP
from ilqr_amd_loader import load_package

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_LIN, TOL_RIC, TOL_X, TOL_K, TOL_J, TOL_H = 2e-11, 1e-9, 1e-8, 1e-7, 1e-9, 1e-8
C_CASE = (12, 5, 11, True)
IDS = ["%dx%d-T%d%s" % (n, m, T, "" if con else "-unconstrained") for n, m, T, con in CP.CASES]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    return p


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _variants(case, stage=False):
    n, m = case[:2]
    if n <= 4 and m <= 4:
        return ("latency", "throughput") if stage else ("latency", "throughput", "packed1", "packed2")
    return ("latency", "mid") if n <= 16 else ("latency",)


def _check(worst, what, value, bar):
    """print the figure (the module's output is where the observed values are read from), then hold it to the bar"""
    print("coupled-hessians %-40s %.3e (bar %.0e)" % (what, value, bar))
    worst.append((what, value, bar))


def _assert_all(worst):
    bad = [w for w in worst if not w[1] <= w[2]]
    assert not bad, bad


# ------------------------------------------------------------------ the references, computed once and left unchanged
def _device_layout(s, T):
    """the restatement's buffers the way the C-ABI lays them out: column-major blocks per timestep"""
    return dict(hessian_state_state=np.concatenate([h.T.ravel() for h in s.gxx]), hessian_action_action=np.concatenate([h.T.ravel() for h in s.guu]),
                hessian_action_state=np.concatenate([h.T.ravel() for h in s.gux]),          # [state][action]: nu x nx column-major
                gradient_state=np.concatenate(s.gx), gradient_action=np.concatenate(s.gu))


@functools.lru_cache(maxsize=None)
def _stage_reference(case):
    """three linearisations at three different nominal trajectories without a reset in between (duals and penalties non-trivial
    from the second on), then one Riccati pass: per instance the inputs of every round and the restatement's outputs"""
    n, m, T, con = case
    pr = CP.restatement_problem(R, n, m, T, con)
    x1, ub = CP.inputs(n, m, T, con)
    nc = 2 * m + 2 if con else 0
    rounds = [[] for _ in range(3)]
    last = []
    for b in range(CP.BATCH):
        s = R.Solver(*pr)
        for it in range(3):
            u = ub[b] * (1.0 + 0.4 * it) + 0.25 * it * np.sin(1.0 + it + np.arange(ub[b].size).reshape(ub[b].shape))
            x = np.stack(R.rollout(pr[0], x1[b] * (1.0 - 0.2 * it), u))
            lam = rho = np.zeros(0)
            if con:
                idx = np.arange((T - 1) * nc, dtype=np.float64)
                lam = np.zeros_like(idx) if it == 0 else 0.4 * it * np.maximum(0.0, np.sin(1.0 + idx))      # half of them zero: rows can be inactive
                rho = np.ones_like(idx) if it == 0 else 1.0 + 4.5 * ((idx + it) % 3)
                for t in range(T - 1):
                    s.constraint_dual[t][:] = lam[t * nc:(t + 1) * nc]; s.constraint_penalty[t][:] = rho[t * nc:(t + 1) * nc]
            s.initialize_controls(u); s.initialize_states(x)
            for t in range(T):
                s.states[t][:] = x[t]
                if t < T - 1:
                    s.actions[t][:] = u[t]
            s.cost_bang("nominal"); s.gradients_bang("nominal")
            rounds[it].append(dict(x=x.copy(), u=u.copy(), lam=lam, rho=rho, out=_device_layout(s, T)))
        s.backward_pass_bang()
        assert s.potrf_info == 0
        last.append(dict(K=np.concatenate([k.T.ravel() for k in s.K]), k=np.concatenate(s.k),
                         P=np.concatenate([p.T.ravel() for p in s.P]), p=np.concatenate(s.p)))
    return rounds, last


@functools.lru_cache(maxsize=None)
def _solve_reference(case):
    n, m, T, con = case
    pr = CP.restatement_problem(R, n, m, T, con)
    x1, ub = CP.inputs(n, m, T, con)
    return x1, ub, [CP.restatement_solve(R, pr, x1[b], ub[b]) for b in range(CP.BATCH)]


# ------------------------------------------------------------------ the device side
def _symbolic_solver(pkg, case, variant):
    n, m, T, con = case
    dyn, costs, cons, name = CP.product_problem(pkg, n, m, T, con)
    sol = pkg.Solver(dyn, costs, cons, batch=CP.BATCH, options=pkg.Options(verbose=0), name=name)
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 2 * m + 2 if con else 0)
    sol.set_kernel_variant_(variant)
    return sol


class _Src(C.Structure):
    _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]


def _c_solver(pkg, probe, monkeypatch):
    """the family at (12, 5) handed over as C callables (ilqr_compile_model), with the host structure probe or with dense tables"""
    n, m, T, _ = C_CASE
    if probe:
        monkeypatch.delenv("ILQR_NO_STRUCTURE_PROBE", raising=False)
    else:
        monkeypatch.setenv("ILQR_NO_STRUCTURE_PROBE", "1")
    L = pkg._ffi.lib()
    ms = _Src(b"coupled12_c", n, m, 0, 2 * m + 2, 0, (1 << (2 * m + 2)) - 1, 0, CP.c_source(pkg, n, m).encode())
    name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
    assert L.ilqr_compile_model(C.byref(ms), name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
    jv, hs = C.c_int32(), C.c_int32()
    assert L.ilqr_model_compact_sizes(name.value, C.byref(jv), C.byref(hs)) == 0
    if not probe:
        assert (jv.value, hs.value) == (n * (n + m), n * n + m * m + m * n)
    else:
        assert hs.value < n * n + m * m + m * n and hs.value > n + 2 * m
    sol = pkg.Solver(model=name.value.decode(), horizon=T, batch=CP.BATCH, options=pkg.Options(verbose=0))
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 2 * m + 2)
    return sol


HESSIANS = ("hessian_state_state", "hessian_action_action", "hessian_action_state")


def _stagewise(sol, case, label, worst):
    n, m, T, con = case
    rounds, last = _stage_reference(case)
    for it, per_instance in enumerate(rounds):
        x = np.stack([r["x"] for r in per_instance]); u = np.stack([r["u"] for r in per_instance])
        for name, v in (("nominal_states", x), ("states", x), ("nominal_actions", u), ("actions", u)):
            sol.set_buffer(name, v)
        if con:
            sol.set_buffer("constraint_dual", np.stack([r["lam"] for r in per_instance]))
            sol.set_buffer("constraint_penalty", np.stack([r["rho"] for r in per_instance]))
        sol.run_stage_("cost_nominal"); sol.run_stage_("gradients")
        for name in HESSIANS + ("gradient_state", "gradient_action"):
            got = sol.buffer(name)
            want = np.stack([r["out"][name] for r in per_instance])
            _check(worst, "%s round %d %s" % (label, it, name), max(_rel(got[b], want[b]) for b in range(CP.BATCH)), TOL_LIN)
            if name == "hessian_action_state":                        # element by element in [t][state][action]: a transpose cannot pass
                g, w = got.reshape(CP.BATCH, T - 1, n, m), want.reshape(CP.BATCH, T - 1, n, m)
                assert (np.abs(g - w) <= TOL_LIN * max(1.0, np.abs(w).max())).all(), (label, it)
                assert np.abs(w).max() > 0
    sol.run_stage_("backward_pass")
    for name in ("K", "k", "P", "p"):
        got = sol.buffer(name)
        _check(worst, "%s riccati %s" % (label, name), max(_rel(got[b], last[b][name]) for b in range(CP.BATCH)), TOL_RIC)


def _solve(sol, case):
    x1, ub, _ = _solve_reference(case)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy()
    out = dict(x=x, u=u, K=K, k=k, st=sol.stats(), kernel=sol.resolved_kernel_variant())
    out.update({name: sol.buffer(name) for name in HESSIANS})
    return out


def _against_the_restatement(res, case, label, worst):
    n, m, T, con = case
    _, _, refs = _solve_reference(case)
    st = res["st"]
    for b, s in enumerate(refs):
        assert st["iterations"][b] == s.iterations and st["outer_iterations"][b] == s.outer_iterations, \
            (label, b, st["iterations"][b], s.iterations, st["outer_iterations"][b], s.outer_iterations)
    dx = max(np.abs(res["x"][b] - np.stack(s.nominal_states)).max() for b, s in enumerate(refs))
    du = max(np.abs(res["u"][b] - np.stack(s.nominal_actions[:-1])).max() for b, s in enumerate(refs))
    dK = max(_rel(res["K"][b], np.stack([Kt.T for Kt in s.K])) for b, s in enumerate(refs))
    dJ = max(abs(st["objective"][b] - s.objective) / max(1.0, abs(s.objective)) for b, s in enumerate(refs))
    _check(worst, label + " solve |dx|", dx, TOL_X); _check(worst, label + " solve |du|", du, TOL_X)
    _check(worst, label + " solve |dK|/max(1,|K|)", dK, TOL_K); _check(worst, label + " solve |dJ|/max(1,|J|)", dJ, TOL_J)
    for name in HESSIANS:
        want = [_device_layout(s, T)[name] for s in refs]
        _check(worst, "%s solve final %s" % (label, name), max(_rel(res[name][b], want[b]) for b in range(CP.BATCH)), TOL_H)
        if name == "hessian_action_state":
            w = np.stack(want).reshape(CP.BATCH, T - 1, n, m)
            assert (np.abs(res[name].reshape(w.shape) - w) <= TOL_H * max(1.0, np.abs(w).max())).all(), label


_DEVICE_SOLVES = {}


def _device_solves(pkg, case):
    """every variant's whole solve of a case, run once and shared by the tests below"""
    if case not in _DEVICE_SOLVES:
        res = {}
        for v in _variants(case):
            sol = _symbolic_solver(pkg, case, v)
            res[v] = _solve(sol, case)
            sol.close()
            assert res[v]["kernel"] == v, (v, res[v]["kernel"])
        _DEVICE_SOLVES[case] = res
    return _DEVICE_SOLVES[case]


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", CP.CASES, ids=IDS)
def test_linearisations_accumulate_and_one_riccati_pass(pkg, case):
    """Stage level, every kernel family that has stage kernels: cost_nominal, gradients (three times, Hessians accumulating over
    three different trajectories) and backward_pass from identical inputs."""
    worst = []
    for v in _variants(case, stage=True):
        sol = _symbolic_solver(pkg, case, v)
        _stagewise(sol, case, v, worst)
        sol.close()
    _assert_all(worst)


@pytest.mark.parametrize("case", CP.CASES, ids=IDS)
def test_whole_solve_against_the_restatement(pkg, case):
    worst = []
    for v, res in _device_solves(pkg, case).items():
        _against_the_restatement(res, case, v, worst)
    _assert_all(worst)


@pytest.mark.parametrize("case", CP.CASES, ids=IDS)
def test_every_variant_of_a_size_gives_the_same_bits(pkg, case):
    """Small path: whichever kernel linearises an instance, the accumulated Hessians are the same bits (gradients_small in
    ilqr_device.hpp), and so are the trajectories and policies; large path: the one-wave variant is the four-wave kernel's
    arithmetic (test_one_wave_variant_of_the_large_path_equals_the_four_wave_kernel)."""
    res = _device_solves(pkg, case)
    base = res["latency"]
    for v, r in res.items():
        for key in ("iterations", "outer_iterations", "rollouts", "status"):
            assert np.array_equal(base["st"][key], r["st"][key]), (v, key)
        for key in HESSIANS + ("x", "u", "K", "k"):
            assert np.array_equal(base[key], r[key], equal_nan=True), (v, key, np.abs(base[key] - r[key]).max())


@pytest.mark.parametrize("probe", [True, False], ids=["probed", "dense"])
def test_c_callables_with_coupled_hessians(pkg, probe, monkeypatch):
    """The family at (12, 5) as C callables through ilqr_compile_model, with the host structure probe (the gux set and the
    off-diagonal entries found by probing) and without it (dense tables): stage level and whole solve like the symbolic route."""
    worst = []
    label = "c-%s" % ("probed" if probe else "dense")
    sol = _c_solver(pkg, probe, monkeypatch)
    _stagewise(sol, C_CASE, label, worst)
    sol.close()
    sol = _c_solver(pkg, probe, monkeypatch)
    res = _solve(sol, C_CASE)
    sol.close()
    _against_the_restatement(res, C_CASE, label, worst)
    _assert_all(worst)
