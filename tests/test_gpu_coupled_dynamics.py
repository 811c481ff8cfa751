"""GPU: state-coupled dynamics Jacobians on the large-model kernels, against the independent restatement run live and the numpy
yardsticks. Every other large-path model of the GPU suite has the synth dynamics: the state-dependent entries of ∂f/∂x lie on the
diagonal and the nonlinear remainder of row i reads x_i alone, so a transposed or mis-tiled Jacobian patch (JAC_VAR_IDX), a wrong
owner lane or fu filter in the filter's est_jacobian_large, a cooperative trig form whose argument spans two states, and a stale u
in an entry off the diagonal were all invisible. The family of tests/coupled_dynamics.py has 2n patched off-diagonal entries, not
closed under transposition, in several tiles for n > 16; half of them depend on u alone. tests/test_coupled_dynamics.py proves the
inputs suitable on the CPU, including that the restatement's control flow does not change under a relative perturbation of 1e-13 —
which is why control flow is demanded exact on every instance here.

Sizes: (5, 2), (12, 5), (17, 3), (33, 2); T = 11; B = 5 for stages and solves, 3 for the MPC-side and filter kernels. Variants:
latency everywhere, mid where nx <= 16 (bitwise the four-wave kernel). Routes: symbolic at every size; C callables at (12, 5) and
(17, 3), with the host structure probe (JV = 4n: the unrolled owner-lane branch of est_jacobian_large) and with dense tables
(JV = n(n + m): 204 at (12, 5), 340 > 256 at (17, 3), the runtime loop, and the fu filter on most entries).

Bars, the project's own. Stages and solves (header of tests/test_gpu_coupled_hessians.py): 2e-11 relative for the linearisation
outputs, 1e-9 relative for one Riccati pass from identical inputs; whole solve: iterations and outer iterations equal on every
instance, |Δx|, |Δu| < 1e-8, |ΔK| <= 1e-7 max(1, |K|), objective to 1e-9 relative; the Armijo slope of one forward pass 1e-10
relative (tests/test_gpu_reference.py), its accepted step size equal. fx and fu are compared element by element in
their documented layout (column-major blocks per time step). MPC side (tests/test_gpu_mpc_sweep.py, tests/test_gpu_plant_io.py):
x, u 1e-10 relative to max(1, max |reference|), cost and max_violation 1e-9; filter (tests/test_gpu_estimator.py): 1e-10. Whether
these stand on this family was decided on the yardsticks alone (tests/test_coupled_dynamics.py, which asserts it): run a second time
with the inputs moved by one part in 1e15 they move

    (nx, nu)   policy x, u / cost / viol      shift head   plant step   predict x̂, P
    (5, 2)     2.7e-15 / 1.5e-15 / 2.7e-15    2.7e-15      1.0e-15      8.9e-16
    (17, 3)    4.5e-15 / 1.6e-15 / 5.3e-15    3.3e-15      2.1e-15      1.2e-15
    (33, 2)    3.6e-15 / 1.4e-15 / 4.4e-15    2.0e-15      1.2e-15      1.2e-15

(cost and viol: the worse of the policy rollout and the candidates). Ten times that is four orders below every bar, so the bars
stand. No sample, candidate, shift head or covariance is left out: the same file asserts that the yardsticks keep all of them
finite. The limits of the filter tests (coupled_dynamics.LIMITS) clamp an action from each side on the yardstick, no raw action
within 1e-2 of a limit; that is what makes the u-dependent off-diagonal entries of F see the CLAMPED u."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import coupled_dynamics as CD
import estimator_ref as E
import mpc_ref as M
import plant_io_ref as IO
import plant_ref as PR
import policy_ref as P
from ilqr_amd_loader import load_package

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_LIN, TOL_RIC, TOL_X, TOL_K, TOL_J = 2e-11, 1e-9, 1e-8, 1e-7, 1e-9
TOL_DELTA = 1e-10               # the Armijo slope ∇Lᵀ·Δz, relative: the bar of tests/test_gpu_reference.py
TOL_XU, TOL_COST, TOL_VIOL, TOL_EST = 1e-10, 1e-9, 1e-9, 1e-10
T = CD.T
MPC_IDS = ["%dx%d" % nm for nm in CD.MPC_SIZES]
C_IDS = ["%dx%d-%s" % (n, m, "probed" if probe else "dense") for n, m in CD.C_SIZES for probe in (True, False)]
C_CASES = [(nm, probe) for nm in CD.C_SIZES for probe in (True, False)]
SEED = PR.SEED
_MODELS = {}


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    return p


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _variants(nm):
    return ("latency", "mid") if nm[0] <= 16 else ("latency",)


def _check(worst, what, value, bar):
    """print the figure (the module's output is where the observed values are read from), then hold it to the bar"""
    print("coupled-dynamics %-44s %.3e (bar %.0e)" % (what, value, bar))
    worst.append((what, value, bar))


def _assert_all(worst):
    bad = [w for w in worst if not w[1] <= w[2]]
    assert not bad, bad


# ------------------------------------------------------------------ the device side
def _symbolic_solver(pkg, nm, variant=None, B=CD.BATCH):
    """traced once per size and process (the symbolic Jacobians of 33 states take ten seconds), then loaded by its registered name"""
    n, m = nm
    if nm in _MODELS:
        sol = pkg.Solver(model=_MODELS[nm], horizon=T, batch=B, options=pkg.Options(verbose=0))
    else:
        dyn, costs, cons, name = CD.product_problem(pkg, n, m)
        sol = pkg.Solver(dyn, costs, cons, batch=B, options=pkg.Options(verbose=0), name=name)
        _MODELS[nm] = sol.model
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 2 * m)
    if variant is not None:
        sol.set_kernel_variant_(variant)
    return sol


class _Src(C.Structure):
    _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]


@functools.lru_cache(maxsize=None)
def _c_text(n, m):
    return CD.c_source(load_package(), n, m).encode()


def _c_solver(pkg, nm, probe, monkeypatch, B=CD.BATCH):
    """the family handed over as C callables (ilqr_compile_model), with the host structure probe or with dense tables"""
    n, m = nm
    if probe:
        monkeypatch.delenv("ILQR_NO_STRUCTURE_PROBE", raising=False)
    else:
        monkeypatch.setenv("ILQR_NO_STRUCTURE_PROBE", "1")
    L = pkg._ffi.lib()
    ms = _Src((CD.name(n, m) + "_c").encode(), *CD.c_dims(n, m), _c_text(n, m))
    name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
    assert L.ilqr_compile_model(C.byref(ms), name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
    jv, hs = C.c_int32(), C.c_int32()
    assert L.ilqr_model_compact_sizes(name.value, C.byref(jv), C.byref(hs)) == 0
    assert jv.value == (4 * n if probe else n * (n + m)), jv.value           # what the probe found: 3n entries of fx, n of fu
    if not probe and nm == (17, 3):
        assert jv.value > 256                                                # the runtime loop of est_jacobian_large
    sol = pkg.Solver(model=name.value.decode(), horizon=T, batch=B, options=pkg.Options(verbose=0))
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 2 * m)
    return sol


# ------------------------------------------------------------------ the references, computed once and left unchanged
def _device_layout(s):
    """the restatement's buffers the way the C-ABI lays them out: column-major blocks per timestep"""
    return dict(jacobian_state=np.concatenate([f.T.ravel() for f in s.fx]), jacobian_action=np.concatenate([f.T.ravel() for f in s.fu]),
                gradient_state=np.concatenate(s.gx), gradient_action=np.concatenate(s.gu))


LIN = ("jacobian_state", "jacobian_action", "gradient_state", "gradient_action")


@functools.lru_cache(maxsize=None)
def _stage_reference(nm):
    """two linearisations at two different nominal trajectories (duals and penalties non-trivial in the second), then one Riccati
    pass: per instance the inputs of every round and the restatement's outputs"""
    n, m = nm
    pr = CD.restatement_problem(R, n, m)
    nc = 2 * m
    rounds = [[] for _ in range(2)]
    last = []
    traj = [CD.stage_round(R, n, m, it) for it in range(2)]
    for b in range(CD.BATCH):
        s = R.Solver(*pr)
        for it in range(2):
            x, u = traj[it][0][b], traj[it][1][b]
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
            rounds[it].append(dict(x=x.copy(), u=u.copy(), lam=lam, rho=rho, out=_device_layout(s)))
        s.backward_pass_bang()
        assert s.potrf_info == 0
        out = dict(K=np.concatenate([k.T.ravel() for k in s.K]), k=np.concatenate(s.k),
                   P=np.concatenate([p.T.ravel() for p in s.P]), p=np.concatenate(s.p))
        s.forward_pass_bang()                                         # the Armijo slope reads fx and fu once more (fw_delta_wave)
        out.update(delta=s.last_forward["delta_grad_product"], step_size=s.step_size)
        last.append(out)
    return rounds, last


@functools.lru_cache(maxsize=None)
def _solve_reference(nm):
    n, m = nm
    pr = CD.restatement_problem(R, n, m)
    x1, ub = CD.inputs(n, m)
    return x1, ub, [CD.restatement_solve(R, pr, x1[b], ub[b]) for b in range(CD.BATCH)]


def _stagewise(sol, nm, label, worst):
    n, m = nm
    rounds, last = _stage_reference(nm)
    off = [(i, c) for i in range(n) for c in (CD.s_of(i, n), CD.r_of(i, n))]
    for it, per_instance in enumerate(rounds):
        x = np.stack([r["x"] for r in per_instance]); u = np.stack([r["u"] for r in per_instance])
        for name, v in (("nominal_states", x), ("states", x), ("nominal_actions", u), ("actions", u)):
            sol.set_buffer(name, v)
        sol.set_buffer("constraint_dual", np.stack([r["lam"] for r in per_instance]))
        sol.set_buffer("constraint_penalty", np.stack([r["rho"] for r in per_instance]))
        sol.run_stage_("cost_nominal"); sol.run_stage_("gradients")
        for name in LIN:
            got = sol.buffer(name)                                    # (large path: the full-array mirror, mirror_large_kernel)
            want = np.stack([r["out"][name] for r in per_instance])
            _check(worst, "%s round %d %s" % (label, it, name), max(_rel(got[b], want[b]) for b in range(CD.BATCH)), TOL_LIN)
            if name.startswith("jacobian"):                           # element by element, [t][column][row]: a transpose cannot pass
                cols = n if name == "jacobian_state" else m
                g, w = got.reshape(CD.BATCH, T - 1, cols, n), want.reshape(CD.BATCH, T - 1, cols, n)
                assert (np.abs(g - w) <= TOL_LIN * max(1.0, np.abs(w).max())).all(), (label, it, name)
                if name == "jacobian_state":                          # the patched off-diagonal entries themselves, F(i, c) = w[t][c][i]
                    d = max(np.abs(g[:, :, c, i] - w[:, :, c, i]).max() for i, c in off)
                    _check(worst, "%s round %d patched off-diagonal fx" % (label, it), d, TOL_LIN)
                    assert min(np.abs(w[:, :, c, i]).max() for i, c in off) >= 1e-4
    sol.run_stage_("backward_pass")
    for name in ("K", "k", "P", "p"):
        got = sol.buffer(name)
        _check(worst, "%s riccati %s" % (label, name), max(_rel(got[b], last[b][name]) for b in range(CD.BATCH)), TOL_RIC)
    sol.run_stage_("forward_pass")
    delta, st = sol.scalar("delta_grad_product"), sol.stats()
    _check(worst, "%s forward pass slope" % label, max(abs(delta[b] - last[b]["delta"]) / abs(last[b]["delta"]) for b in range(CD.BATCH)), TOL_DELTA)
    assert [st["step_size"][b] for b in range(CD.BATCH)] == [last[b]["step_size"] for b in range(CD.BATCH)], label


def _solve(sol, nm):
    x1, ub, _ = _solve_reference(nm)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy()
    return dict(x=x, u=u, K=K, k=k, st=sol.stats(), kernel=sol.resolved_kernel_variant(),
                fx=sol.buffer("jacobian_state"), fu=sol.buffer("jacobian_action"))


def _against_the_restatement(res, nm, label, worst):
    _, _, refs = _solve_reference(nm)
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


_DEVICE_SOLVES = {}


def _device_solves(pkg, nm):
    """every variant's whole solve of a size, run once and shared by the tests below"""
    if nm not in _DEVICE_SOLVES:
        res = {}
        for v in _variants(nm):
            sol = _symbolic_solver(pkg, nm, v)
            res[v] = _solve(sol, nm)
            sol.close()
            assert res[v]["kernel"] == v, (v, res[v]["kernel"])
        _DEVICE_SOLVES[nm] = res
    return _DEVICE_SOLVES[nm]


# ------------------------------------------------------------------ stages and solves
@pytest.mark.parametrize("nm", CD.SIZES, ids=CD.IDS)
def test_linearisations_and_one_riccati_pass(pkg, nm):
    """Stage level: cost_nominal and gradients at two different nominal trajectories — fx and fu element by element, the gradients —
    and backward_pass and forward_pass from identical inputs."""
    worst = []
    for v in _variants(nm):
        sol = _symbolic_solver(pkg, nm, v)
        _stagewise(sol, nm, v, worst)
        sol.close()
    _assert_all(worst)


@pytest.mark.parametrize("nm", CD.SIZES, ids=CD.IDS)
def test_whole_solve_against_the_restatement(pkg, nm):
    worst = []
    for v, res in _device_solves(pkg, nm).items():
        _against_the_restatement(res, nm, v, worst)
    _assert_all(worst)


@pytest.mark.parametrize("nm", [nm for nm in CD.SIZES if nm[0] <= 16], ids=[i for i, nm in zip(CD.IDS, CD.SIZES) if nm[0] <= 16])
def test_every_variant_of_a_size_gives_the_same_bits(pkg, nm):
    """the one-wave variant is the four-wave kernel's arithmetic (test_one_wave_variant_of_the_large_path_equals_the_four_wave_kernel)"""
    res = _device_solves(pkg, nm)
    base = res["latency"]
    assert set(res) == {"latency", "mid"}
    for v, r in res.items():
        for key in ("iterations", "outer_iterations", "rollouts", "status"):
            assert np.array_equal(base["st"][key], r["st"][key]), (v, key)
        for key in ("x", "u", "K", "k", "fx", "fu"):
            assert np.array_equal(base[key], r[key], equal_nan=True), (v, key, np.abs(base[key] - r[key]).max())


@pytest.mark.parametrize("nm,probe", C_CASES, ids=C_IDS)
def test_c_callables_with_coupled_dynamics(pkg, nm, probe, monkeypatch):
    """The family as C callables through ilqr_compile_model, with the host structure probe (the 4n state-dependent entries found
    by probing, patched through the adapter's table) and without it (dense tables): stage level and whole solve like the symbolic
    route."""
    worst = []
    label = "c-%dx%d-%s" % (nm + ("probed" if probe else "dense",))
    sol = _c_solver(pkg, nm, probe, monkeypatch)
    _stagewise(sol, nm, label, worst)
    sol.close()
    sol = _c_solver(pkg, nm, probe, monkeypatch)
    res = _solve(sol, nm)
    sol.close()
    _against_the_restatement(res, nm, label, worst)
    _assert_all(worst)


# ------------------------------------------------------------------ the MPC-side and filter kernels
def _solved_mpc(pkg, nm, make=None):
    """a solved handle at B = 3 and what the kernels read of it: (sol, x̄, ū, K, k)"""
    sol = _symbolic_solver(pkg, nm, B=CD.BATCH_MPC) if make is None else make()
    x1, ub = CD.inputs(*nm, CD.BATCH_MPC)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return (sol,) + sol.get_trajectory() + sol.get_policy()


def _relv(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("nm", CD.MPC_SIZES, ids=MPC_IDS)
def test_mpc_side_entry_points_on_coupled_dynamics(pkg, nm):
    """rollout_policy (step sizes 0 and 0.5), initialize_rollout_candidates_, shift_horizon_ (feedback, steps 1 and 3) and
    plant_step_ (feedback, process noise, limits): dyn_row with the generated dyn_rem_wave whose trig arguments span two states"""
    n, m = nm
    B, S = CD.BATCH_MPC, 5
    name = CD.register_yardstick(n, m)
    f, p = PR.dynamics(name), CD.mpc_problem(n, m)
    sol, xb, ub, K, k = _solved_mpc(pkg, nm)
    worst = []
    x1 = M.rollout_starts(xb, S)
    for alpha in (0.0, 0.5):
        out = sol.rollout_policy(x1, step_size=alpha, trajectories=True)
        w = dict(x=0.0, u=0.0, cost=0.0, viol=0.0)
        for b in range(B):
            for s in range(S):
                ref = M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], x1[b, s], alpha, None)
                assert ref["first_nonfinite"] == -1 and out["first_nonfinite"][b, s] == -1 and np.array_equal(out["x"][b, s, 0], x1[b, s])
                w["x"] = max(w["x"], P.rel(out["x"][b, s], ref["x"])); w["u"] = max(w["u"], P.rel(out["u"][b, s], ref["u"]))
                w["cost"] = max(w["cost"], _relv(out["cost"][b, s], ref["cost"])); w["viol"] = max(w["viol"], _relv(out["max_violation"][b, s], ref["max_violation"]))
        for key, bar in (("x", TOL_XU), ("u", TOL_XU), ("cost", TOL_COST), ("viol", TOL_VIOL)):
            _check(worst, "%dx%d policy rollout step %.1f %s" % (n, m, alpha, key), w[key], bar)
    x0, ub0 = CD.inputs(n, m, B)
    cands = M.candidate_set(ub0, S)
    other = _symbolic_solver(pkg, nm, B=B)
    got = other.initialize_rollout_candidates_(x0, cands)
    w = dict(cost=0.0, viol=0.0)
    for b in range(B):
        ref = M.score_all(p, x0[b], cands[b])
        assert (ref["first_nonfinite"] == -1).all() and np.array_equal(got["first_nonfinite"][b], ref["first_nonfinite"])
        w["cost"] = max(w["cost"], max(_relv(got["cost"][b, s], ref["cost"][s]) for s in range(S)))
        w["viol"] = max(w["viol"], max(_relv(got["max_violation"][b, s], ref["max_violation"][s]) for s in range(S)))
    _check(worst, "%dx%d candidates cost" % nm, w["cost"], TOL_COST); _check(worst, "%dx%d candidates viol" % nm, w["viol"], TOL_VIOL)
    other.close()
    N = T - 1
    for steps in M.SHIFTS:
        start = M.measured_starts(xb, steps)
        sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ub)
        sol.shift_horizon_(steps, x1=start, feedback=True)
        xs, us = sol.get_trajectory()
        assert np.array_equal(xs[:, 0], start)
        w = dict(x=0.0, u=0.0)
        for b in range(B):
            r = M.shift_head(p, xb[b], ub[b], K[b], None, steps, start[b])
            assert r["first_nonfinite"] == -1 and np.abs(us[b, :N - steps] - ub[b, steps:]).max() > 1e-6
            w["x"] = max(w["x"], P.rel(xs[b, :T - steps], r["x"])); w["u"] = max(w["u"], P.rel(us[b, :N - steps], r["u"]))
        _check(worst, "%dx%d shift head k=%d x" % (n, m, steps), w["x"], TOL_XU); _check(worst, "%dx%d shift head k=%d u" % (n, m, steps), w["u"], TOL_XU)
    sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ub)
    u_min, u_max = CD.LIMITS[nm]
    xp, sig = PR.plant_starts(xb), PR.sigma_x(n)
    runs = []
    for steps, s0 in ((1, 0), (3, 5)):
        out = sol.plant_step_(xp, steps=steps, feedback=True, sigma_x=sig, seed=SEED, step0=s0, u_min=u_min, u_max=u_max)
        z = pkg.candidate_noise(SEED, B, *PR.noise_shape(n, s0, steps))
        refs = [IO.plant_step(f, xb[b], ub[b], K[b], None, xp[b], steps, True, sig, z[b], s0, None, u_min, u_max) for b in range(B)]
        runs.append(refs)
        assert np.array_equal(out["saturated"], [r["saturated"] for r in refs]) and (out["first_nonfinite"] == -1).all()
        _check(worst, "%dx%d plant step k=%d x" % (n, m, steps), max(P.rel(out["x"][b], refs[b]["x"]) for b in range(B)), TOL_XU)
        _check(worst, "%dx%d plant step k=%d u" % (n, m, steps), max(P.rel(out["u"][b], refs[b]["u"]) for b in range(B)), TOL_XU)
    low, high, _, nearest = IO.conditions(runs, u_min, u_max)
    assert low and high and nearest > IO.MARGIN, (low, high, nearest)
    sol.close()
    _assert_all(worst)


def _predict_against_the_yardstick(sol, nm, xb, ub, K, label, worst):
    """estimate_predict_ against estimator_ref.predict with the complex-step Jacobian: steps 1 and 3, feedback on and off, with
    limits that bind (asserted on the yardstick): x̂, the full P (both triangles), P exactly symmetric"""
    n, m = nm
    B = CD.BATCH_MPC
    name = CD.register_yardstick(n, m)
    f = PR.dynamics(name)
    u_min, u_max = CD.LIMITS[nm]
    xh, _ = E.start(PR.plant_starts(xb), n)
    Ps = E.p_start(B, n)
    clamped = False
    for steps, fb, lim in ((1, True, True), (3, True, True), (3, False, True), (3, True, False), (1, False, False)):
        lims = dict(u_min=u_min, u_max=u_max) if lim else {}
        x1, P1 = sol.estimate_predict_(xh, Ps, steps=steps, feedback=fb, q=E.q(n), **lims)
        assert np.array_equal(P1, P1.transpose(0, 2, 1))
        assert np.array_equal(x1, sol.plant_step_(xh, steps=steps, feedback=fb, **lims)["x"][:, -1])           # the plant step's bits
        ex = eP = eL = 0.0
        for b in range(B):
            rx, rP = E.predict(name, xb[b], ub[b], K[b], None, xh[b], Ps[b], steps, fb, q=E.q(n), **lims)
            assert np.isfinite(rP).all()
            ex, eP = max(ex, P.rel(x1[b], rx)), max(eP, P.rel(P1[b], rP))
            eL = max(eL, P.rel(np.tril(P1[b]), np.tril(rP)), P.rel(np.triu(P1[b]), np.triu(rP)))
            if lim:
                clamped = clamped or IO.plant_step(f, xb[b], ub[b], K[b], None, xh[b], steps, fb, **lims)["saturated"] > 0
        tag = "%s predict k=%d fb=%d lim=%d" % (label, steps, fb, lim)
        _check(worst, tag + " xhat", ex, TOL_EST); _check(worst, tag + " P", max(eP, eL), TOL_EST)
    assert clamped


@pytest.mark.parametrize("nm", CD.MPC_SIZES, ids=MPC_IDS)
def test_estimate_predict_on_coupled_dynamics(pkg, nm):
    """est_jacobian_large's non-elementwise branch with off-diagonal targets in several tiles, and entries that depend on the clamped u"""
    sol, xb, ub, K, _ = _solved_mpc(pkg, nm)
    worst = []
    _predict_against_the_yardstick(sol, nm, xb, ub, K, "%dx%d" % nm, worst)
    sol.close()
    _assert_all(worst)


@pytest.mark.parametrize("probe", [True, False], ids=["probed", "dense"])
def test_estimate_predict_on_the_c_route(pkg, probe, monkeypatch):
    """(17, 3) through the adapter: dense tables take the JV > 256 runtime loop and drop 51 fu entries at the filter, probed tables
    take the unrolled owner-lane branch"""
    nm = (17, 3)
    sol, xb, ub, K, _ = _solved_mpc(pkg, nm, make=lambda: _c_solver(pkg, nm, probe, monkeypatch, B=CD.BATCH_MPC))
    worst = []
    _predict_against_the_yardstick(sol, nm, xb, ub, K, "c-17x3-%s" % ("probed" if probe else "dense"), worst)
    sol.close()
    _assert_all(worst)
