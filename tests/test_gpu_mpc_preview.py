"""ilqr_plant_score and ilqr_mpc_run_preview on the GPU. T = 11 (the closed form: 9), built-in models and the (5, 1) synth model with a
user parameter.

1. The score against tests/plant_score_ref.py (plain fp64 over mpc_ref's cost_s / con_s / ineq_s) on plant steps taken by plant_step_
   with feedback and sigma_x: car_obs at B = 70 (a ragged second wave of the one-lane-per-element kernel), k = 3, under the handle's θ
   and under w_plant; car created unconstrained (violation ≡ 0); synth5w (large form, one user parameter in front of two selector
   columns) and synth12 at B = 3; synth32 at B = 2, k = 1.
   Bounds: the project's standing ones, cost 1e-9 relative, violation 1e-9 per max(1, |v|) — TOL_COST, TOL_VIOL of
   tests/test_gpu_mpc_sweep.py, not re-tuned. tests/test_plant_score_ref.py asserts that ten times the yardstick's own spread under a
   1e-15 move of x and u stays below them; measured there: car_obs cost 1.4e-15, violation 6.2e-15; synth5w cost 1.4e-15, violation
   1.6e-15; synth12 cost 1.9e-15, violation 1.6e-15. Every model stays under the bounds.
2. Element independence: an instance scored alone (B = 1) and in its batch, a step scored with k = 1 and as step i of k = 3: same bits.
3. Containment: one instance with NaN state rows has NaN elements; every other element is bitwise the clean run's.
4. The call reads the handle: every named buffer, the scalars and the resident inputs are bitwise unchanged.
5. mpc_run_(w_preview, score=True) against the same sequence stepped from Python through the host forms — plant_step_, plant_score_,
   shift_horizon_(w_tail = the period's rows), shift_duals_, solve_warm_ — bitwise: car_obs on the latency (1) and the packed (5)
   variant, synth5w (one stage kind: a handle with selectors cannot be shifted) on the large path, k in {1, 3}.
6. The closed form of the preview at T = 9, k = 3, P = 4: every previewed row travels the whole horizon, is applied by the plant and
   scored under; w_preview holds a different value per (b, row, column).
7. ilqr_mpc_run_preview with its three new pointers NULL is mpc_run_ on a twin handle, bitwise.
8. A sharded handle equals the single one bitwise.
9. The refusals that need a handle, each leaving the handle's buffers untouched.
"""
import ctypes as C

import numpy as np
import pytest

import mpc_ref as M
import plant_ref as R
import plant_score_ref as SR
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_COST, TOL_VIOL = 1e-9, 1e-9
T = R.T
NAMED = ["nominal_states", "nominal_actions", "states", "actions", "jacobian_state", "jacobian_action", "gradient_state", "gradient_action",
         "hessian_state_state", "hessian_action_action", "hessian_action_state", "K", "k", "P", "p", "gradient_state_lagrangian",
         "gradient_action_lagrangian", "violations", "constraint_dual", "constraint_penalty", "active_set", "parameters", "_scalars"]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_plant_score", "ilqr_plant_score_device", "ilqr_mpc_run_preview"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


# ------------------------------------------------------------------------------------------------------------------ helpers
def _synth5w(pkg, B, alternating, horizon=T):
    """mpc_ref.synth5w as the device's objects (nx = 5: the LARGE form, one user parameter). alternating: the two stage-cost kinds of
    the yardstick, lowered onto selector columns; else kind 0 at every step (no selectors: the handle can be shifted)"""
    import sympy as sp
    f, stage, term, box = M.synth5w_functions(sp.sin)
    dyn = pkg.Dynamics(f, 5, 1, num_parameter=1)
    kinds = [pkg.Cost(stage(r), 5, 1, num_parameter=1) for r in M.SYNTH5W_WEIGHTS]
    con = pkg.Constraint(box, 5, 1, indices_inequality=[1, 2], num_parameter=1)
    costs = [kinds[t % 2 if alternating else 0] for t in range(horizon - 1)] + [pkg.Cost(term, 5, 0, num_parameter=1)]
    return pkg.Solver([dyn] * (horizon - 1), costs, [con] * (horizon - 1) + [pkg.Constraint()], batch=B,
                      options=pkg.Options(verbose=0, **R.SOLVE), name="synth5w_alt" if alternating else "synth5w_one")


def _solved(pkg, name, B, constrained=True, variant=None, horizon=T, **kw):
    """a handle of the case solved from the workload's inputs, every one prepared the same way -> (sol, θ or None)"""
    if name.startswith("synth5w"):
        sol = _synth5w(pkg, B, name == "synth5w", horizon)
        x1, ub = M.sweep_inputs(5, 1, B, horizon)
        w = M.synth5w_parameters(B, horizon)
    else:
        sol = pkg.Solver(model=name, horizon=horizon, batch=B, options=pkg.Options(verbose=0, **R.SOLVE), constraints=constrained, **kw)
        x1, ub, w = R.inputs(pkg.workloads, name, B)
        ub, w = np.ascontiguousarray(ub[:, :horizon - 1]), None if w is None else np.ascontiguousarray(w[:, :horizon])
    if variant is not None:
        sol.set_kernel_variant_(variant)
    if w is not None:
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol, w


def _steps(sol, w, k, plant_w):
    """plant steps to score: feedback and sigma_x, from a state half a SIZE_X1 move off x̄_0 -> (x, u, w_plant)"""
    x0 = R.plant_starts(sol.get_trajectory()[0])
    wp = R.plant_parameters(w, k) if plant_w else None
    out = sol.plant_step_(x0, steps=k, feedback=True, sigma_x=R.sigma_x(sol.nx), seed=R.SEED, w_plant=wp)
    assert (out["first_nonfinite"] == -1).all()
    return out["x"], out["u"], wp


def _snapshot(sol):
    return {nm: sol.buffer(nm) for nm in NAMED}


def _unchanged(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]


def _differ(pkg, one, two):
    """the named buffers in which two handles differ; of the scalar block the slots ilqr_get_stats and the initialisers report"""
    a, b = _snapshot(one), _snapshot(two)
    keep = pkg._ffi.lib().ilqr_scalar_slot(b"states_eq_nominal") + 1
    a["_scalars"], b["_scalars"] = a["_scalars"][:, :keep], b["_scalars"][:, :keep]
    return _unchanged(a, b)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _against_the_yardstick(got, refs, tag):
    worst = dict(cost=0.0, viol=0.0)
    for b, ref in enumerate(refs):
        assert np.isfinite(ref["cost"]).all() and (ref["cost"] > 0).all(), (tag, b)
        worst["cost"] = max(worst["cost"], float(np.max(np.abs(got["cost"][b] - ref["cost"]) / np.abs(ref["cost"]))))
        worst["viol"] = max(worst["viol"], float(np.max(np.abs(got["violation"][b] - ref["violation"]) / np.maximum(1.0, np.abs(ref["violation"])))))
    print("plant score %s: worst cost %.2e (relative), violation %.2e (per max(1, |v|))" % (tag, worst["cost"], worst["viol"]))
    assert worst["cost"] < TOL_COST and worst["viol"] < TOL_VIOL, (tag, worst)


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name,B,k,constrained,plant_w", [("car_obs", 70, 3, True, False), ("car_obs", 70, 3, True, True), ("car", 3, 3, False, False),
                                                          ("synth5w", 3, 3, True, True), ("synth12", 3, 3, True, False), ("synth32", 2, 1, True, False)])
def test_score_against_the_yardstick(pkg, name, B, k, constrained, plant_w):
    sol, w = _solved(pkg, name, B, constrained)
    x, u, wp = _steps(sol, w, k, plant_w)
    got = sol.plant_score_(x, u, w_plant=wp)
    assert got["cost"].shape == got["violation"].shape == (B, k)
    p = SR.problem(name, T)
    refs = [SR.plant_score(p, x[b], u[b], None if w is None else w[b], None if wp is None else wp[b], constrained) for b in range(B)]
    _against_the_yardstick(got, refs, "%s B=%d k=%d%s%s" % (name, B, k, "" if constrained else " unconstrained", " w_plant" if plant_w else ""))
    if not constrained:
        assert not got["violation"].any()
    if name == "synth5w":           # the selector columns stayed the handle's: the rows alternate between the two stage kinds
        assert sol._selectors.shape == (T, 2) and np.array_equal(sol.buffer("parameters").reshape(B, T, 3)[:, :, 1:], np.broadcast_to(sol._selectors, (B, T, 2)))
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name,B,b", [("car_obs", 70, 65), ("synth12", 3, 1)])
def test_an_element_depends_on_its_own_rows_only(pkg, name, B, b):
    k = 3
    sol, w = _solved(pkg, name, B)
    x, u, wp = _steps(sol, w, k, name == "car_obs")
    full = sol.plant_score_(x, u, w_plant=wp)
    # alone: a handle of one instance that holds the same θ (the score reads nothing else of it)
    alone = pkg.Solver(model=name, horizon=T, batch=1, options=pkg.Options(verbose=0))
    if w is not None:
        alone.set_parameters_(w[b:b + 1])
    one = alone.plant_score_(x[b:b + 1], u[b:b + 1], w_plant=None if wp is None else wp[b:b + 1])
    for key in full:
        assert _same(one[key][0], full[key][b]), key
    alone.close()
    # step i of k = 3 and the same rows scored with k = 1: under explicit parameters (position 0 of the handle is another θ row)
    for i in range(k):
        step = sol.plant_score_(x[:, i:i + 2], u[:, i:i + 1], w_plant=None if wp is None else wp[:, i:i + 1])
        for key in full:
            assert _same(step[key][:, 0], full[key][:, i]), (key, i)
    # the handle's own θ rows given as w_plant are the handle's θ rows
    if w is not None:
        own, given = sol.plant_score_(x, u), sol.plant_score_(x, u, w_plant=np.ascontiguousarray(w[:, :k]))
        first = sol.plant_score_(x[:, :2], u[:, :1])
        for key in own:
            assert _same(own[key], given[key]) and _same(first[key][:, 0], own[key][:, 0]), key
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name,B,bad", [("car_obs", 70, 65), ("synth12", 3, 1)])
def test_non_finite_rows_stay_contained(pkg, name, B, bad):
    sol, w = _solved(pkg, name, B)
    x, u, wp = _steps(sol, w, 3, False)
    clean = sol.plant_score_(x, u)
    xn = x.copy(); xn[bad, :, 0] = np.nan
    out = sol.plant_score_(xn, u)
    others = np.arange(B) != bad
    assert np.isnan(out["cost"][bad]).all() and np.isfinite(clean["cost"]).all()
    if name == "car_obs":           # its clearance row reads x_0; synth12's rows read the actions only
        assert np.isnan(out["violation"][bad]).all()
    else:
        assert _same(out["violation"][bad], clean["violation"][bad])
    for key in clean:
        assert _same(out[key][others], clean[key][others]), key
    # one row: its element alone
    xn = x.copy(); xn[bad, 1, 0] = np.nan
    out = sol.plant_score_(xn, u)
    assert np.isnan(out["cost"][bad, 1]) and _same(np.delete(out["cost"], 1, axis=1), np.delete(clean["cost"], 1, axis=1))
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_the_call_reads_the_handle(pkg, name):
    B = 3
    sol, w = _solved(pkg, name, B)
    twin, _ = _solved(pkg, name, B)
    x, u, wp = _steps(sol, w, 3, True)
    before = _snapshot(sol)
    sol.plant_score_(x, u, w_plant=wp)
    sol.plant_score_(x, u)
    assert _unchanged(before, _snapshot(sol)) == []
    # the resident inputs: replayed, they install what the twin's replay installs
    sol.initialize_rollout_resident_(); twin.initialize_rollout_resident_()
    sol.synchronize(); twin.synchronize()
    assert _differ(pkg, sol, twin) == []
    sol.close(); twin.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
def _host_stepped(sol, x0, periods, k, warm, w_plant, w_preview, **kw):
    """ilqr_mpc_run_preview's definition, stepped from Python through the host forms"""
    x, xs, us, logs, costs, viols = x0.copy(), [x0[:, None]], [], [], [], []
    for p in range(periods):
        rows = slice(p * k, (p + 1) * k)
        wp = None if w_plant is None else np.ascontiguousarray(w_plant[:, rows])
        out = sol.plant_step_(x, steps=k, step0=p * k, w_plant=wp, **kw)
        sc = sol.plant_score_(out["x"], out["u"], w_plant=wp)
        x = out["x"][:, -1].copy()
        xs.append(out["x"][:, 1:]); us.append(out["u"]); costs.append(sc["cost"]); viols.append(sc["violation"])
        sol.shift_horizon_(k, x1=x, w_tail=None if w_preview is None else np.ascontiguousarray(w_preview[:, rows]))
        if warm:
            sol.shift_duals_(k)
            sol.solve_warm_()
        else:
            sol.solve_()
        logs.append(sol.stats())
    cat = lambda parts: np.concatenate(parts, axis=1)
    return cat(xs), cat(us), {f: np.stack([l[f] for l in logs], axis=1) for f in logs[0]}, cat(costs), cat(viols)


def _preview_of(w, rows):
    """the stream a run follows: rows in the size of the handle's own θ, different per (b, row, column)"""
    B, _, nw = w.shape
    return SR.distinct_preview(B, rows, nw) + (0.0 if nw == 2 else -0.2)


@pytest.mark.parametrize("name,variant", [("car_obs", 1), ("car_obs", 5), ("synth5w_one", None)])
@pytest.mark.parametrize("k", [1, 3])
def test_mpc_run_preview_is_the_host_stepped_composition_bitwise(pkg, name, variant, k):
    B, periods = 5, 3
    a, w = _solved(pkg, name, B, True, variant)
    b, _ = _solved(pkg, name, B, True, variant)
    if name == "synth5w_one":
        assert a._selectors is None and a.nx == 5
    x0 = R.plant_starts(a.get_trajectory()[0])
    w_plant = R.plant_parameters(np.concatenate([w, w], axis=1), periods * k)
    w_preview = _preview_of(w, periods * k)
    kw = dict(sigma_x=R.sigma_x(a.nx), seed=R.SEED)
    res = a.mpc_run_(periods, k, x0=x0, w_plant=w_plant, w_preview=w_preview, score=True, **kw)
    x, u, log, cost, viol = _host_stepped(b, x0, periods, k, True, w_plant, w_preview, **kw)
    assert _same(res.x, x) and _same(res.u, u) and (res.first_nonfinite == -1).all()
    assert sorted(res.log) == sorted(log)
    for f in log:
        assert _same(res.log[f], log[f]), f
    assert res.cl_cost.shape == res.cl_violation.shape == (B, periods * k)
    assert _same(res.cl_cost, cost) and _same(res.cl_violation, viol)
    assert np.isfinite(res.cl_cost).all() and (res.log["iterations"] > 0).all()
    assert _differ(pkg, a, b) == []          # trajectory, policy, duals, penalties, parameters, scalars: everything named
    a.initialize_rollout_resident_(); b.initialize_rollout_resident_()
    a.synchronize(); b.synchronize()
    assert _differ(pkg, a, b) == []
    # the preview arrived: the last k rows of θ are the run's last k rows
    assert _same(a.buffer("parameters").reshape(w.shape)[:, T - k:], w_preview[:, (periods - 1) * k:])
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
def test_closed_form_of_the_preview(pkg):
    Tc, k, P, B = 9, 3, 4, 3
    sol, w = _solved(pkg, "car_obs", B, horizon=Tc)
    w_preview = SR.distinct_preview(B, P * k, 2)
    assert len(np.unique(w_preview)) == w_preview.size
    res = sol.mpc_run_(P, k, w_preview=w_preview, score=True, sigma_x=R.sigma_x(3), seed=R.SEED)
    theta = sol.buffer("parameters").reshape(B, Tc, 2)
    for b in range(B):
        assert np.array_equal(theta[b], SR.preview_closed_form(w[b], P, k, w_preview[b])), b
    assert np.array_equal(theta, w_preview[:, P * k - Tc:])        # T <= P·k: every row of the horizon is a previewed one
    # the last period's plant steps ran, and were scored, under previewed rows: θ_0 .. θ_{k−1} after P − 1 periods
    assert (res.first_nonfinite == -1).all() and np.isfinite(res.x).all()
    p = SR.problem("car_obs")
    for q in range(P):
        held = [SR.preview_closed_form(w[b], q, k, w_preview[b]) for b in range(B)]
        if q == P - 1:                  # (P − 1) · k = T: by then every row the plant runs under is a previewed one
            assert all(np.array_equal(held[b], w_preview[b, :Tc]) for b in range(B))
        got = dict(cost=res.cl_cost[:, q * k:(q + 1) * k], violation=res.cl_violation[:, q * k:(q + 1) * k])
        refs = [SR.plant_score(p, res.x[b, q * k:(q + 1) * k + 1], res.u[b, q * k:(q + 1) * k], held[b]) for b in range(B)]
        _against_the_yardstick(got, refs, "closed form, period %d" % q)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 7
def test_null_preview_and_scores_are_mpc_run(pkg):
    B, periods, k = 5, 2, 2
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    a, w = _solved(pkg, "car_obs", B)
    b, _ = _solved(pkg, "car_obs", B)
    x0 = R.plant_starts(a.get_trajectory()[0])
    w_plant = R.plant_parameters(w, periods * k)
    sig = R.sigma_x(3)
    Rr = periods * k
    x, u, log, nf = np.empty((B, Rr + 1, 3)), np.empty((B, Rr, 2)), np.empty((B, periods, 9)), np.empty(B, dtype=np.int32)
    d = pkg._ffi.MpcDesc(periods, k, 0, 0, 0, 1, 0, 0, R.SEED, 0, sig.ctypes.data_as(F64))
    pkg._ffi.check(L.ilqr_mpc_run_preview(a._h, C.byref(d), x0.ctypes.data_as(F64), w_plant.ctypes.data_as(F64), None, x.ctypes.data_as(F64),
                                          u.ctypes.data_as(F64), log.ctypes.data_as(F64), nf.ctypes.data_as(I32), None, None))
    res = b.mpc_run_(periods, k, x0=x0, w_plant=w_plant, sigma_x=sig, seed=R.SEED)
    assert res.cl_cost is None and res.cl_violation is None
    assert _same(x, res.x) and _same(u, res.u) and _same(nf, res.first_nonfinite)
    for c, f in enumerate(pkg._ffi.MPC_LOG_COLUMNS):
        assert _same(log[:, :, c], res.log[f].astype(np.float64)), f
    assert _differ(pkg, a, b) == []
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 8
def test_sharded_handle_equals_the_single_one(pkg):
    B, periods, k = 7, 2, 2
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    x, u, wp = _steps(one, w, 3, True)
    s1, s2 = one.plant_score_(x, u, w_plant=wp), two.plant_score_(x, u, w_plant=wp)
    for key in s1:
        assert _same(s1[key], s2[key]), key
    x0 = R.plant_starts(one.get_trajectory()[0])
    kw = dict(x0=x0, sigma_x=R.sigma_x(3), seed=R.SEED, first_instance=11, w_plant=R.plant_parameters(w, periods * k),
              w_preview=_preview_of(w, periods * k), score=True)
    r1, r2 = (s.mpc_run_(periods, k, **kw) for s in (one, two))
    for f in ("x", "u", "first_nonfinite", "cl_cost", "cl_violation"):
        assert _same(getattr(r1, f), getattr(r2, f)), f
    for f in r1.log:
        assert _same(r1.log[f], r2.log[f]), f
    assert _differ(pkg, one, two) == []
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 9
def test_refusals_that_need_a_handle(pkg):
    B = 3
    Err = pkg._ffi.IlqrError
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p

    def refused(sol, call, match):
        before = _snapshot(sol)
        with pytest.raises(Err, match=match):
            call()
        assert _unchanged(before, _snapshot(sol)) == []

    car, _ = _solved(pkg, "car", B)
    x, u, _ = _steps(car, None, 2, False)
    refused(car, lambda: car.plant_score_(x, u, w_plant=np.zeros((B, 2, 2))), "no parameters")
    refused(car, lambda: car.mpc_run_(2, w_preview=np.zeros((B, 2, 2))), "w_preview given, but this model has no parameters")
    refused(car, lambda: car.mpc_run_(2, w_plant=np.zeros((B, 2, 2)), score=True), "no parameters")
    before = _snapshot(car)
    buf = np.zeros((B, T + 2, 3))
    assert L.ilqr_plant_score(car._h, T, None, buf.ctypes.data_as(F64), buf.ctypes.data_as(F64), buf.ctypes.data_as(F64), None) == -1     # steps > T − 1
    assert b"steps must lie in 1 .. T-1" in L.ilqr_last_error()
    d = pkg._ffi.MpcDesc(2, 1, 0, 0, 0, 1, 0, 0, 1, 0, None)
    assert L.ilqr_mpc_run_preview(car._h, C.byref(d), None, None, None, None, None, None, None, None, buf.ctypes.data_as(F64)) == -1
    assert b"cl_violation without cl_cost" in L.ilqr_last_error() and _unchanged(before, _snapshot(car)) == []
    car.close()
    sh, _ = _solved(pkg, "car", B, devices=[0, 0])
    refused(sh, lambda: sh.plant_score_device_(2, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data), "sharded handle")
    sh.close()
    # a lowered problem: its structure belongs to horizon positions — the run is refused, the score itself reads positions 0 .. k−1
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    dynamics, costs, constraints = pkg.models.car_tv(51)
    low = pkg.Solver(stage_sources=pkg.lowering.c_stage_sources(dynamics, costs, constraints), batch=B, options=pkg.Options(verbose=0, **R.SOLVE),
                     name="car_tv_c")
    low.initialize_rollout_(x1, ub)
    low.solve_()
    refused(low, lambda: low.mpc_run_(2, warm=False, score=True), "stage selectors")
    out = low.plant_step_(x1, steps=2)
    sc = low.plant_score_(out["x"], out["u"])
    assert np.isfinite(sc["cost"]).all() and sc["cost"].shape == (B, 2)
    low.close()
