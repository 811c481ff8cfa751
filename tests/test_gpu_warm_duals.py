"""ilqr_shift_duals and ilqr_solve_warm on the GPU against tests/duals_ref.py (the numpy shift; the warm solve composed from the CPU
oracle's exported steps — both checked without a GPU in tests/test_duals_ref.py, which also qualifies the inputs of test 3).

Bounds, fixed before the kernels ran. The shift is a copy: bitwise. A warm solve started from the cold values λ = 0, ρ = ρ0 runs the
same instructions on the same numbers as ilqr_solve: bitwise, on every kernel variant. Device chains that differ only in where the
duals were shifted: bitwise. Against the composed oracle loop (test 3) the bars are those of the whole-solve test of that model,
tests/test_gpu_parity.py::test_parameters_car_obs, taken over unchanged: control flow (iterations and rollouts) identical on >= 99 %
of the instances — all five here — and |Δx|, |Δu| < 1e-7 on those; outer_iterations equal wherever the inner counts agree.
"""
import os
import subprocess

import numpy as np
import pytest

import duals_ref as D
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = ["nominal_states", "nominal_actions", "states", "actions", "jacobian_state", "jacobian_action", "gradient_state", "gradient_action",
         "hessian_state_state", "hessian_action_action", "hessian_action_state", "K", "k", "P", "p", "gradient_state_lagrangian",
         "gradient_action_lagrangian", "violations", "constraint_dual", "constraint_penalty", "active_set", "parameters", "_scalars"]
DUALS = ("constraint_dual", "constraint_penalty")
# name -> (config, T): stage and terminal rows; terminal rows only; the large path; N·ncs = 250 > the copy workgroup's 128 lanes > k·ncs
SHAPES = {"car_obs12": ("car_obs", 12), "acrobot": ("acrobot51", 9), "synth12": ("synth12", 11), "car_obs51": ("car_obs", 51)}


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    assert hasattr(p._ffi.lib(), "ilqr_solve_warm"), "the library has no ilqr_solve_warm"
    return p


def _inputs(pkg, config, B, T=None):
    model, T0, x1, ub = pkg.workloads.make_inputs(config, B)
    T = T0 if T is None else T
    w = pkg.workloads.make_parameters(config, B)[:, :T] if model == "car_obs" else None
    return model, T, x1, np.ascontiguousarray(ub[:, :T - 1]), None if w is None else np.ascontiguousarray(w)


def _handle(pkg, config, model, T, B, w, variant=None, **kw):
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(config, {})), **kw)
    if variant is not None:
        sol.set_kernel_variant_(variant)
    if w is not None:
        sol.set_parameters_(w)
    return sol


def _solved(pkg, config, B, T=None, variant=None, **kw):
    model, T, x1, ub, w = _inputs(pkg, config, B, T)
    sol = _handle(pkg, config, model, T, B, w, variant, **kw)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol


def _result(sol):
    """what a solve leaves: trajectory, policy, duals, statistics"""
    st = sol.stats()
    return sol.get_trajectory() + sol.get_policy() + (sol.buffer(DUALS[0]), sol.buffer(DUALS[1])) + tuple(st[f] for f in sorted(st))


def _eq(p, q):
    return len(p) == len(q) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, q))


def _first_difference(p, q):
    return [i for i, (a, b) in enumerate(zip(p, q)) if not np.array_equal(a, b, equal_nan=True)]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_shift_is_exact(pkg, shape):
    """1. steps in {0, 1, 2, N−1, N}, both tails, both penalty modes: constraint_dual / constraint_penalty are bitwise duals_ref's, every
    other named buffer and _scalars are bitwise what they were. The duals are the solve's plus a ramp (written back through
    set_buffer), so that every entry is distinct and a misplaced copy shows."""
    config, T = SHAPES[shape]
    B, N = 5, T - 1
    sol = _solved(pkg, config, B, T)
    ncs, nct, rho0 = sol.nc_stage, sol.nc_term, 0.5
    sol.options.initial_constraint_penalty = rho0
    C = N * ncs + nct
    ramp = 1.0e-3 * (1.0 + np.arange(B * C, dtype=np.float64).reshape(B, C))
    lam0, rho0s = sol.buffer(DUALS[0]) + ramp, sol.buffer(DUALS[1]) + 7.0 * ramp
    assert lam0.shape == (B, C) and (shape != "car_obs51" or (N * ncs > 128 > ncs))
    for k in (0, 1, 2, N - 1, N):
        for tail in ("hold", "zero"):
            for penalty in ("keep", "reset"):
                sol.set_buffer(DUALS[0], lam0); sol.set_buffer(DUALS[1], rho0s)
                before = {nm: sol.buffer(nm) for nm in NAMED}
                sol.shift_duals_(k, tail=tail, penalty=penalty)
                after = {nm: sol.buffer(nm) for nm in NAMED}
                want = dict(zip(DUALS, D.shift_duals(lam0, rho0s, ncs, nct, k, tail, penalty, rho0)))
                for nm in NAMED:
                    ref = want.get(nm, before[nm])
                    assert np.array_equal(after[nm], ref, equal_nan=True), (shape, k, tail, penalty, nm, np.argwhere(after[nm] != ref)[:4])
    sol.close()


@pytest.mark.parametrize("config,variant,B", [("car_obs", 1, 6), ("car_obs", 2, 6), ("car_obs", 5, 7), ("car_obs", 6, 7),
                                              ("synth12", 1, 6), ("synth12", 4, 6)])
def test_a_warm_solve_from_cold_values_is_the_cold_solve(pkg, config, variant, B):
    """2. initialize_rollout_, then λ = 0, ρ = ρ0 written with set_buffer, then solve_warm_: trajectories, policy, duals, statistics
    and trace are bitwise those of solve_ on a twin handle, on every kernel variant the model has (7 instances on the packed
    ones: the last pack is ragged). Cannot pass without the feature."""
    model, T, x1, ub, w = _inputs(pkg, config, B, 31 if config == "synth12" else None)
    out = []
    for warm in (False, True):
        sol = _handle(pkg, config, model, T, B, w, variant)
        sol.enable_trace_(256)
        sol.initialize_rollout_(x1, ub)
        if warm:
            C = (T - 1) * sol.nc_stage + sol.nc_term
            sol.set_buffer(DUALS[0], np.zeros((B, C)))
            sol.set_buffer(DUALS[1], np.full((B, C), sol.options.initial_constraint_penalty))
            sol.solve_warm_()
        else:
            sol.solve_()
        outer = sol.stats()["outer_iterations"]
        out.append(_result(sol) + (sol.trace(), sol.scalar("trace_len")))
        sol.close()
    assert outer.max() >= 2, "no instance of the cold solve updates its duals: the comparison would not see a refilled λ"
    assert _eq(out[0], out[1]), _first_difference(out[0], out[1])


def test_a_warm_solve_from_shifted_duals_matches_the_composed_oracle_loop(pkg, oracle):
    """3. The inputs tests/test_duals_ref.py qualifies (the oracle's solve shifted by one period, duals shifted with hold / keep):
    the device's warm solve against the composed oracle loop under the bars of tests/test_gpu_parity.py::test_parameters_car_obs."""
    c = D.small_case(pkg, oracle)
    sol = _handle(pkg, "car_obs", c["model"], c["T"], c["B"], c["ws"])
    sol.initialize_rollout_(c["x1s"], c["ubs"])
    sol.set_buffer(DUALS[0], c["lam"]); sol.set_buffer(DUALS[1], c["rho"])
    sol.solve_warm_()
    x, u = sol.get_trajectory(); st = sol.stats()
    sol.close()
    ref = c["warm"]
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    dx, du = np.abs(x - ref["x"])[same].max(), np.abs(u - ref["u"])[same].max()
    print("\ncontrol flow identical on %d of %d; max |dx| %.2e |du| %.2e; outer iterations device %s oracle %s (cold oracle %s)"
          % (same.sum(), len(same), dx, du, st["outer_iterations"], ref["stats"]["outer_iterations"], c["cold"]["stats"]["outer_iterations"]))
    assert same.mean() >= 0.99
    assert dx < 1e-7 and du < 1e-7
    assert np.array_equal(st["outer_iterations"][same], ref["stats"]["outer_iterations"][same])
    assert (st["max_violation"] <= c["options"].constraint_tolerance)[same].all()


@pytest.mark.parametrize("config", ["car_obs", "synth12"])
def test_the_device_chain_is_the_chain_with_the_duals_shifted_on_the_host(pkg, config):
    """4. solve_ -> shift_horizon_ -> shift_duals_ -> solve_warm_ is bitwise the same chain with the dual shift done as buffer ->
    numpy -> set_buffer."""
    B, T = 5, (31 if config == "synth12" else None)
    out = []
    for on_device in (True, False):
        sol = _solved(pkg, config, B, T)
        sol.shift_horizon_(1)
        if on_device:
            sol.shift_duals_(1)
        else:
            lam, rho = D.shift_duals(sol.buffer(DUALS[0]), sol.buffer(DUALS[1]), sol.nc_stage, sol.nc_term, 1, "hold", "keep",
                                     sol.options.initial_constraint_penalty)
            sol.set_buffer(DUALS[0], lam); sol.set_buffer(DUALS[1], rho)
        mid = (sol.buffer(DUALS[0]), sol.buffer(DUALS[1]))
        sol.solve_warm_()
        out.append(mid + _result(sol))
        sol.close()
    assert np.abs(out[0][0]).max() > 0 and out[0][1].max() > 1.0            # there was something to shift
    assert _eq(out[0], out[1]), _first_difference(out[0], out[1])


def test_hand_over_does_not_show_in_a_warm_solve(pkg, oracle):
    """5. On the one-wave packed variant a warm solve with ilqr_set_handover(h, 2) and one with the hand-over off: bitwise equal.
    Inputs: the shifted trajectories and multipliers of test 3 with the penalties back at ρ0, so that instances need a second outer
    iteration and leave the packed kernel at its start (asserted on the run without hand-over) — with non-zero λ, which a finisher
    that refilled the duals would destroy."""
    c = D.small_case(pkg, oracle)
    B = 7
    reps = (np.arange(B) % c["B"])
    out, stats = [], []
    for handover in (0, 2):
        sol = _handle(pkg, "car_obs", c["model"], c["T"], B, c["ws"][reps], variant=5)
        sol.set_handover_(handover)
        if handover == 0:
            sol.set_handover_live_(0)
        sol.initialize_rollout_(c["x1s"][reps], c["ubs"][reps])
        sol.set_buffer(DUALS[0], c["lam"][reps]); sol.set_buffer(DUALS[1], np.full_like(c["rho"][reps], c["options"].initial_constraint_penalty))
        sol.solve_warm_()
        out.append(_result(sol))
        stats.append((sol.stats(), sol.handover_stats(), sol.scalar("resume")))
        sol.close()
    print("\nouter iterations %s; hand-over queue (queued, marked) %s" % (stats[0][0]["outer_iterations"], stats[1][1]))
    assert (stats[0][0]["outer_iterations"] >= 2).any(), "no instance enters outer iteration 2: nothing is handed over"
    assert (stats[1][2] == 0).all()                                          # everything handed over was finished
    assert _eq(out[0], out[1]), _first_difference(out[0], out[1])


def test_a_sharded_handle_gives_the_single_handles_results(pkg):
    """6. devices = [0, 0]: the shift and the warm solve, bitwise."""
    B = 5
    out = []
    for kw in ({}, dict(devices=[0, 0])):
        sol = _solved(pkg, "car_obs", B, **kw)
        sol.shift_horizon_(1)
        sol.shift_duals_(1, tail="zero")
        mid = (sol.buffer(DUALS[0]), sol.buffer(DUALS[1]))
        sol.solve_warm_()
        out.append(mid + _result(sol))
        if kw:
            with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
                sol.shift_duals_device_(1)
        sol.close()
    assert _eq(out[0], out[1]), _first_difference(out[0], out[1])


def test_refusals_leave_the_handle_alone(pkg):
    """7. Every refusal, each with the handle's buffers untouched; has_duals is cleared by reset_ and set by a host write of
    constraint_penalty."""
    L = pkg._ffi.lib()
    B = 3
    model, T, x1, ub, w = _inputs(pkg, "car_obs", B, 12)
    sol = _handle(pkg, "car_obs", model, T, B, w)
    sol.initialize_rollout_(x1, ub)

    def snap(s):
        return [s.buffer(nm) for nm in NAMED]

    def refused(s, call, match):
        before = snap(s)
        with pytest.raises(pkg._ffi.IlqrError, match=match):
            call()
        assert _eq(before, snap(s)), match

    # no duals yet: a fresh handle, and again after reset_
    refused(sol, lambda: sol.solve_warm_(), "holds no duals")
    refused(sol, lambda: sol.shift_duals_(1), "holds no duals")
    refused(sol, lambda: sol.shift_duals_device_(1), "holds no duals")
    sol.solve_()
    for bad, match in ((dict(steps=-1), "steps must lie"), (dict(steps=T), "steps must lie"), (dict(tail=2), "unknown tail"), (dict(penalty=2), "unknown penalty")):
        args = dict(steps=1, tail=0, penalty=0); args.update(bad)
        for fn in (L.ilqr_shift_duals, L.ilqr_shift_duals_device):
            refused(sol, lambda: pkg._ffi.check(fn(sol._h, args["steps"], args["tail"], args["penalty"])), match)
    with pytest.raises(ValueError):
        sol.shift_duals_(1, tail="up")
    with pytest.raises(ValueError):
        sol.shift_duals_(1, penalty="double")
    sol.shift_duals_(1); sol.shift_duals_device_(0, penalty="reset"); sol.solve_warm_()          # accepted once duals are held
    sol.reset_()
    sol.initialize_rollout_(x1, ub)
    refused(sol, lambda: sol.solve_warm_(), "holds no duals")
    sol.set_buffer(DUALS[0], np.zeros((B, (T - 1) * 5 + 4)))                                       # the multipliers alone do not count
    refused(sol, lambda: sol.shift_duals_(0), "holds no duals")
    sol.set_buffer(DUALS[1], np.ones((B, (T - 1) * 5 + 4)))
    sol.shift_duals_(0); sol.solve_warm_()
    sol.reset_(); sol.initialize_rollout_(x1, ub)
    sol.run_stage_("al_begin")                                                                     # the host-stepped loop's opening stage counts
    sol.solve_warm_()
    sol.close()
    # a handle created unconstrained
    free = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0), constraints=False)
    free.set_parameters_(w); free.initialize_rollout_(x1, ub); free.solve_()
    refused(free, lambda: free.solve_warm_(), "unconstrained")
    refused(free, lambda: free.shift_duals_(1), "unconstrained")
    refused(free, lambda: free.shift_duals_device_(1), "unconstrained")
    free.close()
    # stage selectors: the structure of a lowered problem belongs to horizon positions
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    dynamics, costs, constraints = pkg.models.car_tv(51)
    low = pkg.Solver(stage_sources=pkg.lowering.c_stage_sources(dynamics, costs, constraints), batch=B, options=pkg.Options(verbose=0),
                     name="car_tv_c")
    low.initialize_rollout_(x1, ub); low.solve_()
    refused(low, lambda: low.shift_duals_(1), "stage selectors")
    low.shift_duals_(0, penalty="reset"); low.solve_warm_()                                         # steps == 0 moves nothing across positions
    low.close()
    # a sharded handle whose shards hold no duals
    model, T, x1, ub, w = _inputs(pkg, "car_obs", B, 12)
    sh = _handle(pkg, "car_obs", model, T, B, w, devices=[0, 0])
    sh.initialize_rollout_(x1, ub)
    refused(sh, lambda: sh.solve_warm_(), "holds no duals")
    sh.solve_(); sh.shift_duals_(1); sh.solve_warm_()
    sh.close()


def test_plain_c_caller_of_the_warm_loop(pkg, tmp_path):
    """8. examples/mpc_warm.c: solve, then per period shift_horizon -> shift_duals -> solve_warm, from plain C."""
    exe = str(tmp_path / "mpc_warm")
    libdir = os.path.join(ROOT, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mpc_warm.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe, "37"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mpc warm check passed" in out.stdout and out.stdout.count("period") == 5
