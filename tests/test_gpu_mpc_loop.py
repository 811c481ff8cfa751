"""ilqr_plant_step and ilqr_mpc_run on the GPU. T = 11, built-in models.

1. The plant step against tests/plant_ref.py (plain fp64 numpy loops; the noise from ilqr_candidate_noise) on car (3 x 2, small form;
   the unconstrained handle too), car_obs (user parameters: w_plant), acrobot (4 x 1), synth12 (large form, one tile) and synth32
   (32 x 8: state rows beyond lane 15, noise rows 1 and 2); B = 3 and 70 (a second, ragged wave of the one-lane-per-instance kernel;
   synth32: 3), k in {1, 3}, feedback, noise with one zero sigma, step0 in {0, 5}. The handle is solved first (five inner, two outer
   iterations: the plant needs a policy, not a converged one); the plant starts half a SIZE_X1 move off x̄_0.
   Bound on x, u: the project's own, 1e-10 relative to max(1, max |reference|) — TOL_XU of tests/test_gpu_mpc_sweep.py, not
   re-tuned. tests/test_plant_ref.py asserts on the oracle's solve of the same inputs that ten times the yardstick's own spread under
   a 1e-15 move of x stays below it (acrobot 1.6e-15, car 1.3e-15, car_obs 1.1e-15, synth12 1.8e-15, synth32 1.5e-15) and that
   every plant state is finite. first_nonfinite: equal.
2. A NaN instance is marked at step 0 and its neighbours' outputs are bitwise those of a run without it.
3. The call reads the handle: every named buffer, the scalars and the resident inputs are bitwise unchanged.
4. ilqr_mpc_run against the same sequence stepped from Python through the host forms, bitwise: same kernels, same inputs.
5. A sharded handle equals the single one bitwise, noise included (first_instance + lo).
6. The refusals that need a handle, each leaving the handle's buffers untouched.
7. The staging of the run reused across runs of different length, against fresh handles.
"""
import ctypes as C

import numpy as np
import pytest

import plant_ref as R
import policy_ref as P
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU = 1e-10
T = R.T
NAMED = ["nominal_states", "nominal_actions", "states", "actions", "jacobian_state", "jacobian_action", "gradient_state", "gradient_action",
         "hessian_state_state", "hessian_action_action", "hessian_action_state", "K", "k", "P", "p", "gradient_state_lagrangian",
         "gradient_action_lagrangian", "violations", "constraint_dual", "constraint_penalty", "active_set", "parameters", "_scalars"]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_plant_step", "ilqr_plant_step_device", "ilqr_mpc_run"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


def _solved(pkg, name, B, constrained=True, variant=None, **kw):
    """a handle of the case solved from the workload's inputs, every one prepared the same way"""
    sol = pkg.Solver(model=name, horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE), constraints=constrained, **kw)
    if variant is not None:
        sol.set_kernel_variant_(variant)
    x1, ub, w = R.inputs(pkg.workloads, name, B)
    if w is not None:
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol, w


def _snapshot(sol):
    return {nm: sol.buffer(nm) for nm in NAMED}


def _unchanged(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]


def _differ(pkg, one, two):
    """the named buffers in which two handles differ. Of the scalar block the slots ilqr_get_stats and the initialisers report
    (objective .. states_eq_nominal) count; the rest is bookkeeping of how a launch ran (timestamps, hardware ids, hand-over marks),
    never the same for two launches."""
    a, b = _snapshot(one), _snapshot(two)
    keep = pkg._ffi.lib().ilqr_scalar_slot(b"states_eq_nominal") + 1
    assert keep == 10
    a["_scalars"], b["_scalars"] = a["_scalars"][:, :keep], b["_scalars"][:, :keep]
    return _unchanged(a, b)


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name,constrained", [("car", True), ("car", False), ("car_obs", True), ("acrobot", True), ("synth12", True), ("synth32", True)])
def test_plant_step_against_the_reference(pkg, name, constrained):
    worst = dict(x=0.0, u=0.0)
    for B in R.BATCHES[name]:
        sol, w = _solved(pkg, name, B, constrained)
        (xb, ub), (K, _) = sol.get_trajectory(), sol.get_policy()
        x0 = R.plant_starts(xb)
        sig = R.sigma_x(sol.nx)
        for k, fb, ns, s0 in R.cases():
            wp = R.plant_parameters(w, k)
            out = sol.plant_step_(x0, steps=k, feedback=bool(fb), sigma_x=sig if ns else None, seed=R.SEED, step0=s0, w_plant=wp)
            z = pkg.candidate_noise(R.SEED, B, *R.noise_shape(sol.nx, s0, k)) if ns else None
            refs = R.reference(name, xb, ub, K, w, x0, k, fb, sig if ns else None, z, s0, wp)
            assert np.array_equal(out["x"][:, 0], x0), (name, B, k, fb, ns, s0)
            assert np.array_equal(out["first_nonfinite"], [r["first_nonfinite"] for r in refs]), (name, B, k, fb, ns, s0)
            for b, r in enumerate(refs):
                ex, eu = P.rel(out["x"][b], r["x"]), P.rel(out["u"][b], r["u"])
                worst["x"], worst["u"] = max(worst["x"], ex), max(worst["u"], eu)
                assert ex < TOL_XU and eu < TOL_XU, (name, B, k, fb, ns, s0, b, ex, eu)
            if ns:                  # the zero sigma draws nothing; the others do
                quiet = sol.plant_step_(x0, steps=1, feedback=bool(fb), step0=s0, w_plant=R.plant_parameters(w, 1))
                one = out["x"][:, 1] != quiet["x"][:, 1]
                assert not one[:, sol.nx // 2].any() and np.delete(one, sol.nx // 2, axis=1).all(), (name, B, k, fb, s0)
        sol.close()
    print("plant step %s%s: worst relative error x %.2e, u %.2e" % (name, "" if constrained else " (unconstrained)", worst["x"], worst["u"]))


# ----------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name,B,bad", [("car_obs", 70, 65), ("synth12", 3, 1)])
def test_non_finite_instances_stay_contained(pkg, name, B, bad):
    sol, w = _solved(pkg, name, B)
    x0 = R.plant_starts(sol.get_trajectory()[0])
    kw = dict(steps=3, feedback=True, sigma_x=R.sigma_x(sol.nx), seed=R.SEED, step0=5)
    clean = sol.plant_step_(x0, **kw)
    xn = x0.copy(); xn[bad, 0] = np.nan
    out = sol.plant_step_(xn, **kw)
    assert out["first_nonfinite"][bad] == 0 and np.isnan(out["x"][bad, 1:]).any()
    others = np.arange(B) != bad
    assert (clean["first_nonfinite"] == -1).all() and (out["first_nonfinite"][others] == -1).all()
    for key in ("x", "u"):
        assert np.array_equal(out[key][others], clean[key][others]), key
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_the_call_reads_the_handle(pkg, name):
    B = 3
    sol, w = _solved(pkg, name, B)
    twin, _ = _solved(pkg, name, B)
    before = _snapshot(sol)
    x0 = R.plant_starts(sol.get_trajectory()[0])
    sol.plant_step_(x0, steps=3, feedback=True, sigma_x=R.sigma_x(sol.nx), seed=R.SEED, w_plant=R.plant_parameters(w, 3))
    assert _unchanged(before, _snapshot(sol)) == []
    # the resident inputs: replayed, they install what the twin's replay installs
    sol.initialize_rollout_resident_(); twin.initialize_rollout_resident_()
    sol.synchronize(); twin.synchronize()
    assert _differ(pkg, sol, twin) == []
    sol.close(); twin.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
def _host_stepped(sol, x0, periods, k, warm, w_plant, **kw):
    """ilqr_mpc_run's definition, stepped from Python through the host forms"""
    x, xs, us, logs = x0.copy(), [x0[:, None]], [], []
    for p in range(periods):
        wp = None if w_plant is None else w_plant[:, p * k:(p + 1) * k]
        out = sol.plant_step_(x, steps=k, step0=p * k, w_plant=wp, **kw)
        x = out["x"][:, -1].copy()
        xs.append(out["x"][:, 1:]); us.append(out["u"])
        sol.shift_horizon_(k, x1=x)
        if warm:
            sol.shift_duals_(k)
            sol.solve_warm_()
        else:
            sol.solve_()
        logs.append(sol.stats())
    return np.concatenate(xs, axis=1), np.concatenate(us, axis=1), {f: np.stack([l[f] for l in logs], axis=1) for f in logs[0]}


@pytest.mark.parametrize("name,constrained,variant", [("car_obs", True, 1), ("car_obs", True, 5), ("car", False, None), ("synth12", True, None)])
@pytest.mark.parametrize("k", [1, 2])
def test_mpc_run_is_the_host_stepped_composition_bitwise(pkg, name, constrained, variant, k):
    B, periods = 5, 3
    a, w = _solved(pkg, name, B, constrained, variant)
    b, _ = _solved(pkg, name, B, constrained, variant)
    x0 = R.plant_starts(a.get_trajectory()[0])
    w_plant = R.plant_parameters(np.concatenate([w, w], axis=1), periods * k) if w is not None else None
    kw = dict(sigma_x=R.sigma_x(a.nx), seed=R.SEED)
    res = a.mpc_run_(periods, k, x0=x0, warm=constrained, w_plant=w_plant, **kw)
    x, u, log = _host_stepped(b, x0, periods, k, constrained, w_plant, **kw)
    assert np.array_equal(res.x, x) and np.array_equal(res.u, u) and (res.first_nonfinite == -1).all()
    assert sorted(res.log) == sorted(log)
    for f in log:
        assert np.array_equal(res.log[f], log[f], equal_nan=True), f
    assert (res.log["iterations"] > 0).all()
    assert _differ(pkg, a, b) == []          # trajectory, policy, duals, penalties, parameters, scalars: everything named
    a.initialize_rollout_resident_(); b.initialize_rollout_resident_()
    a.synchronize(); b.synchronize()
    assert _differ(pkg, a, b) == []
    a.close(); b.close()


def test_mpc_run_without_x0_starts_at_the_nominal_state_with_feedback(pkg):
    """x0 = NULL is x̄_0; both feedbacks on: the plant's and the shift's"""
    B, periods, k = 5, 2, 1
    a, w = _solved(pkg, "car_obs", B)
    b, _ = _solved(pkg, "car_obs", B)
    xb0 = a.get_trajectory()[0][:, 0].copy()
    res = a.mpc_run_(periods, k, plant_feedback=True, shift_feedback=True, sigma_x=R.sigma_x(3), seed=3, duals_tail="zero")
    x = xb0
    for p in range(periods):
        out = b.plant_step_(x, steps=k, feedback=True, sigma_x=R.sigma_x(3), seed=3, step0=p * k)
        x = out["x"][:, -1].copy()
        assert np.array_equal(res.x[:, p * k:(p + 1) * k + 1], out["x"]) and np.array_equal(res.u[:, p * k:(p + 1) * k], out["u"])
        b.shift_horizon_(k, x1=x, feedback=True); b.shift_duals_(k, tail="zero"); b.solve_warm_()
    assert np.array_equal(res.x[:, 0], xb0) and _differ(pkg, a, b) == []
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
def test_sharded_handle_equals_the_single_one(pkg):
    B, periods, k = 7, 2, 2
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    x0 = R.plant_starts(one.get_trajectory()[0])
    kw = dict(steps=3, feedback=True, sigma_x=R.sigma_x(3), seed=R.SEED, first_instance=11, step0=5, w_plant=R.plant_parameters(w, 3))
    p1, p2 = one.plant_step_(x0, **kw), two.plant_step_(x0, **kw)
    for key in p1:
        assert np.array_equal(p1[key], p2[key]), key
    w_plant = R.plant_parameters(w, periods * k)
    r1, r2 = (s.mpc_run_(periods, k, x0=x0, sigma_x=R.sigma_x(3), seed=R.SEED, first_instance=11, w_plant=w_plant) for s in (one, two))
    assert np.array_equal(r1.x, r2.x) and np.array_equal(r1.u, r2.u) and np.array_equal(r1.first_nonfinite, r2.first_nonfinite)
    for f in r1.log:
        assert np.array_equal(r1.log[f], r2.log[f], equal_nan=True), f
    assert not np.array_equal(r1.x[0], r1.x[4] - x0[4] + x0[0])     # instances of the second shard draw their own noise
    assert _differ(pkg, one, two) == []
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
def test_refusals_that_need_a_handle(pkg):
    B = 3
    Err = pkg._ffi.IlqrError
    L = pkg._ffi.lib()

    def refused(sol, call, match):
        before = _snapshot(sol)
        with pytest.raises(Err, match=match):
            call()
        assert _unchanged(before, _snapshot(sol)) == []

    car, _ = _solved(pkg, "car", B)
    x0 = car.get_trajectory()[0][:, 0].copy()
    buf = np.zeros((B, T + 2, 3))
    F64 = pkg._ffi.c_double_p
    before = _snapshot(car)
    assert L.ilqr_plant_step(car._h, T, 0, 0, 0, 0, None, None, buf.ctypes.data_as(F64), None, None, None) == -1         # steps > T − 1
    assert b"steps must lie in 1 .. T-1" in L.ilqr_last_error() and _unchanged(before, _snapshot(car)) == []
    refused(car, lambda: car.plant_step_(x0, w_plant=np.zeros((B, 1, 2))), "no parameters")
    refused(car, lambda: car.mpc_run_(2, w_plant=np.zeros((B, 2, 2))), "no parameters")
    car.reset_()
    refused(car, lambda: car.plant_step_(x0, feedback=True), "no policy")
    refused(car, lambda: car.mpc_run_(2, plant_feedback=True, warm=False), "no policy")
    refused(car, lambda: car.mpc_run_(2, shift_feedback=True, warm=False), "no policy")
    refused(car, lambda: car.mpc_run_(2), "holds no duals")                       # warm on a handle without duals
    car.close()
    free, _ = _solved(pkg, "car", B, constrained=False)
    refused(free, lambda: free.mpc_run_(2), "unconstrained")
    free.close()
    sh, _ = _solved(pkg, "car", B, devices=[0, 0])
    refused(sh, lambda: sh.plant_step_device_(buf.ctypes.data), "sharded handle")
    sh.close()
    # a lowered problem: its structure belongs to horizon positions
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    dynamics, costs, constraints = pkg.models.car_tv(51)
    low = pkg.Solver(stage_sources=pkg.lowering.c_stage_sources(dynamics, costs, constraints), batch=B, options=pkg.Options(verbose=0, **R.SOLVE),
                     name="car_tv_c")
    low.initialize_rollout_(x1, ub)
    low.solve_()
    refused(low, lambda: low.mpc_run_(2, warm=False), "stage selectors")
    out = low.plant_step_(x1, steps=2)                                            # the plant step itself reads positions 0 .. k−1: allowed
    assert (out["first_nonfinite"] == -1).all() and np.array_equal(out["u"], low.get_trajectory()[1][:, :2])
    low.close()


# ----------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_staging_reuse(pkg, name):
    """One handle runs P·k = 2, then 12, then 2, with the optional outputs null and given; each run is bitwise a fresh handle's run.
    The handles are re-solved from the same inputs before every run, so that the runs are comparable."""
    B = 2
    L = pkg._ffi.lib()
    F64, I32 = pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    one, w = _solved(pkg, name, B)
    x1, ub, _ = R.inputs(pkg.workloads, name, B)
    warm = 1
    for periods, k in ((2, 1), (4, 3), (1, 2)):
        for full in (False, True):
            fresh, _ = _solved(pkg, name, B)
            one.reset_()
            if w is not None:
                one.set_parameters_(w)                    # the last run shifted them
            one.initialize_rollout_(x1, ub); one.solve_()
            x0 = R.plant_starts(fresh.get_trajectory()[0])
            sig = R.sigma_x(one.nx)
            d = pkg._ffi.MpcDesc(periods, k, 1, 0, 0, warm, 0, 0, R.SEED, 0, sig.ctypes.data_as(F64))
            outs = []
            for sol, fill in ((one, 1.5), (fresh, -2.5)):
                Rr = periods * k
                x, u = np.full((B, Rr + 1, sol.nx), fill), np.full((B, Rr, sol.nu), fill)
                log, nf = np.full((B, periods, 9), fill), np.full(B, int(fill * 2), dtype=np.int32)
                pkg._ffi.check(L.ilqr_mpc_run(sol._h, C.byref(d), x0.ctypes.data_as(F64), None, x.ctypes.data_as(F64) if full else None,
                                              u.ctypes.data_as(F64) if full else None, log.ctypes.data_as(F64) if full else None,
                                              nf.ctypes.data_as(I32) if full else None))
                outs.append((x, u, log, nf) if full else ())
            for p, q in zip(*outs):
                assert np.array_equal(p, q, equal_nan=True), (periods, k, full)
            assert _differ(pkg, one, fresh) == [], (periods, k, full)
            fresh.close()
    one.close()
