"""ilqr_plant_step_limited, ilqr_plant_measure and ilqr_mpc_run_io on the GPU. T = 11, built-in models car_obs (3 x 2, small form, user
parameters), acrobot (4 x 1), synth12 (large form) and synth32 (32 x 8: rows beyond lane 15); B = 3 and 70 (synth32: 3), handles solved
as in tests/test_gpu_mpc_loop.py (five inner, two outer iterations). Limits, sigma_y and the cases: tests/plant_io_ref.py.

1. The limited plant step against the yardstick: x, u within TOL_XU = 1e-10 relative to max(1, max |reference|), the project's own
   bound of the unlimited step (tests/test_plant_io_ref.py: ten times the yardstick's spread stays below it); where the yardstick
   clamps, u_out IS the limit; saturated exact. The two input conditions of tests/test_plant_io_ref.py are asserted again on the
   device's own plan.
2. Limits of ∓Inf, and null limits, are ilqr_plant_step bit for bit.
3. A NaN instance keeps its NaN through the clamp, is marked, counts nothing as saturated and changes no other instance's bits.
4. The measurement: y against x + sigma_y · z of ilqr_candidate_noise rows 5 .. within TOL_XU (the bound the process noise is held
   to); zero-sigma components and a null sigma_y are bitwise copies; the handle is untouched.
5. ilqr_mpc_run_io is, bit for bit, the device entry points called one by one from the host; delay 0 and 1, k in {1, 2}, warm and
   cold, the latency (1) and the packed (5) variant, a large model; a sharded handle [0, 0] equals the single one.
6. A null io (and an io of null pointers, delay 0) is ilqr_mpc_run_preview on every output and on the handle's final state.
7. Without sigma_x, sigma_y and w_plant the delay 1 run is the delay 0 run bit for bit; with sigma_x, row p of y_cl differs from
   x_cl[(p+1)·k] and is the yardstick's prediction within TOL_XU.
8. The device forms are refused on a sharded handle; the refusals that need a handle's dimensions.
"""
import ctypes as C

import numpy as np
import pytest

import plant_io_ref as IO
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
    for fn in ("ilqr_plant_step_limited", "ilqr_plant_step_limited_device", "ilqr_plant_measure", "ilqr_plant_measure_device", "ilqr_mpc_run_io"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


def _solved(pkg, name, B, variant=None, **kw):
    """a handle of the case solved from the workload's inputs, every one prepared the same way"""
    sol = pkg.Solver(model=name, horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE), **kw)
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
    """the named buffers in which two handles differ; of the scalar block the slots ilqr_get_stats and the initialisers report"""
    a, b = _snapshot(one), _snapshot(two)
    keep = pkg._ffi.lib().ilqr_scalar_slot(b"states_eq_nominal") + 1
    a["_scalars"], b["_scalars"] = a["_scalars"][:, :keep], b["_scalars"][:, :keep]
    return _unchanged(a, b)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _plan(sol, w):
    (xb, ub), (K, _) = sol.get_trajectory(), sol.get_policy()
    return xb, ub, K, w


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", IO.MODELS)
def test_limited_plant_step_against_the_yardstick(pkg, name):
    u_min, u_max = IO.LIMITS[name]
    worst = dict(x=0.0, u=0.0)
    for B in R.BATCHES[name]:
        sol, w = _solved(pkg, name, B)
        xb, ub, K, _ = _plan(sol, w)
        x0 = R.plant_starts(xb)
        sig = R.sigma_x(sol.nx)
        runs = []
        for k, fb, ns, s0 in IO.CASES:
            wp = R.plant_parameters(w, k)
            out = sol.plant_step_(x0, steps=k, feedback=bool(fb), sigma_x=sig if ns else None, seed=R.SEED, step0=s0, w_plant=wp, u_min=u_min, u_max=u_max)
            z = pkg.candidate_noise(R.SEED, B, *R.noise_shape(sol.nx, s0, k)) if ns else None
            refs = IO.reference(name, xb, ub, K, w, x0, k, fb, sig if ns else None, z, s0, wp, u_min, u_max)
            runs.append(refs)
            tag = (name, B, k, fb, ns, s0)
            assert np.array_equal(out["x"][:, 0], x0), tag
            assert np.array_equal(out["first_nonfinite"], [r["first_nonfinite"] for r in refs]), tag
            assert np.array_equal(out["saturated"], [r["saturated"] for r in refs]), tag
            for b, r in enumerate(refs):
                ex, eu = P.rel(out["x"][b], r["x"]), P.rel(out["u"][b], r["u"])
                worst["x"], worst["u"] = max(worst["x"], ex), max(worst["u"], eu)
                assert ex < TOL_XU and eu < TOL_XU, tag + (b, ex, eu)
                hit = r["side"] != 0
                assert np.array_equal(out["u"][b][hit], r["u"][hit]), tag + (b,)              # the limit itself, bit for bit
        low, high, alone, nearest = IO.conditions(runs, u_min, u_max)
        assert low and high and alone and nearest > IO.MARGIN, (name, B, low, high, alone, nearest)
        sol.close()
    print("limited plant step %s: worst relative error x %.2e, u %.2e" % (name, worst["x"], worst["u"]))


# ----------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", IO.MODELS)
def test_infinite_and_null_limits_are_the_unlimited_step(pkg, name):
    B = max(R.BATCHES[name])
    sol, w = _solved(pkg, name, B)
    x0 = R.plant_starts(sol.get_trajectory()[0])
    kw = dict(steps=3, feedback=True, sigma_x=R.sigma_x(sol.nx), seed=R.SEED, step0=5, w_plant=R.plant_parameters(w, 3))
    plain = sol.plant_step_(x0, **kw)
    inf = sol.plant_step_(x0, u_min=np.full(sol.nu, -np.inf), u_max=np.full(sol.nu, np.inf), **kw)
    half = sol.plant_step_(x0, u_max=np.full(sol.nu, np.inf), **kw)
    for out in (inf, half):
        for key in plain:
            assert np.array_equal(out[key], plain[key]), key
        assert not out["saturated"].any()
    # null limits through the new entry point itself
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    x, xo, uo = x0.copy(), np.empty_like(plain["x"]), np.empty_like(plain["u"])
    nf, sat = np.empty(B, dtype=np.int32), np.full(B, 7, dtype=np.int32)
    sig, wp = kw["sigma_x"], kw["w_plant"]
    pkg._ffi.check(L.ilqr_plant_step_limited(sol._h, 3, 1, R.SEED, 0, 5, sig.ctypes.data_as(F64), None, None, wp.ctypes.data_as(F64) if wp is not None else None,
                                             x.ctypes.data_as(F64), xo.ctypes.data_as(F64), uo.ctypes.data_as(F64), nf.ctypes.data_as(I32), sat.ctypes.data_as(I32)))
    assert np.array_equal(xo, plain["x"]) and np.array_equal(uo, plain["u"]) and np.array_equal(nf, plain["first_nonfinite"]) and not sat.any()
    assert np.array_equal(x, plain["x"][:, -1])
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name,B,bad", [("car_obs", 70, 65), ("synth12", 3, 1)])
def test_a_nan_instance_keeps_its_nan_through_the_clamp(pkg, name, B, bad):
    u_min, u_max = IO.LIMITS[name]
    lo, hi = np.where(np.isfinite(u_min), u_min, -1.0e3), np.where(np.isfinite(u_max), u_max, 1.0e3)    # every component limited
    sol, w = _solved(pkg, name, B)
    x0 = R.plant_starts(sol.get_trajectory()[0])
    kw = dict(steps=3, feedback=True, sigma_x=R.sigma_x(sol.nx), seed=R.SEED, step0=5, u_min=lo, u_max=hi)
    clean = sol.plant_step_(x0, **kw)
    xn = x0.copy(); xn[bad, :] = np.nan
    out = sol.plant_step_(xn, **kw)
    assert np.isnan(out["u"][bad]).all() and np.isnan(out["x"][bad, 1:]).all()       # K (x − x̄) of a NaN state: no min / max swallowed it
    assert out["first_nonfinite"][bad] == 0 and out["saturated"][bad] == 0
    others = np.arange(B) != bad
    assert (clean["first_nonfinite"] == -1).all() and (out["first_nonfinite"][others] == -1).all()
    for key in ("x", "u", "saturated"):
        assert np.array_equal(out[key][others], clean[key][others]), key
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", IO.MODELS)
def test_measurement_against_the_host_twin(pkg, name):
    for B in R.BATCHES[name]:
        sol, w = _solved(pkg, name, B)
        before = _snapshot(sol)
        n = sol.nx
        x = R.plant_starts(sol.get_trajectory()[0])
        sy = IO.sigma_y(n)
        quiet = np.flatnonzero(sy == 0.0)
        for step, first in ((0, 0), (7, 11)):
            y = sol.plant_measure_(x, step=step, sigma_y=sy, seed=R.SEED, first_instance=first)
            z = pkg.candidate_noise(R.SEED, B, *IO.measure_shape(step), first_instance=first)
            ref = np.stack([IO.measure(x[b], sy, z[b], step) for b in range(B)])
            assert P.rel(y, ref) < TOL_XU, (name, B, step, P.rel(y, ref))
            assert np.array_equal(y[:, quiet], x[:, quiet]) and (np.delete(y, quiet, axis=1) != np.delete(x, quiet, axis=1)).all()
            # the noise itself, not only the sum: (y − x) / sigma_y is z up to the rounding of the sum
            loud = np.flatnonzero(sy != 0.0)
            zz = np.stack([[z[b, IO.MEASURE_ROW0 + j // 16, step, j % 16] for j in loud] for b in range(B)])
            assert np.abs((y - x)[:, loud] / sy[loud] - zz).max() < 1e-9
        assert np.array_equal(sol.plant_measure_(x, step=3), x)                        # null sigma_y: a copy
        assert _unchanged(before, _snapshot(sol)) == []
        sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
def _device_stepped(pkg, sol, x0, periods, k, warm, w_plant, delay, u_min, u_max, sigma_y, sigma_x, seed, feedback, first_instance=0):
    """ilqr_mpc_run_io's definition: the device entry points called one by one from the host, on device arrays of the caller"""
    import torch
    B, n, m = sol.B, sol.nx, sol.nu
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
        xp, xc = torch.from_numpy(x0.copy()).to(dev), torch.zeros(B, n, **f64)
        xo, uo = torch.zeros(B, k + 1, n, **f64), torch.zeros(B, k, m, **f64)
        nf, sat = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        wps = None if w_plant is None else [torch.from_numpy(np.ascontiguousarray(w_plant[:, p * k:(p + 1) * k])).to(dev) for p in range(periods)]
    torch.cuda.synchronize()
    xs, us, ys, logs, nfs, sats = [x0[:, None]], [], [], [], [], np.zeros(B, dtype=np.int64)
    lim = dict(u_min=u_min, u_max=u_max)
    for p in range(periods):
        if delay:
            sol.plant_measure_device_(xp.data_ptr(), xc.data_ptr(), step=p * k, sigma_y=sigma_y, seed=seed, first_instance=first_instance)
            sol.plant_step_device_(xc.data_ptr(), steps=k, feedback=feedback, seed=seed, first_instance=first_instance, step0=p * k, **lim)
        sol.plant_step_device_(xp.data_ptr(), steps=k, feedback=feedback, sigma_x=sigma_x, seed=seed, first_instance=first_instance, step0=p * k,
                               d_w_plant_ptr=None if wps is None else wps[p].data_ptr(), d_x_out_ptr=xo.data_ptr(), d_u_out_ptr=uo.data_ptr(),
                               d_first_nonfinite_ptr=nf.data_ptr(), d_saturated_ptr=sat.data_ptr(), **lim)
        if not delay:
            sol.plant_measure_device_(xp.data_ptr(), xc.data_ptr(), step=(p + 1) * k, sigma_y=sigma_y, seed=seed, first_instance=first_instance)
        sol.shift_horizon_device_(k, xc.data_ptr())
        if warm:
            sol.shift_duals_(k)
            sol.solve_warm_()
        else:
            sol.solve_()
        sol.synchronize()
        xs.append(xo.cpu().numpy()[:, 1:]); us.append(uo.cpu().numpy()); ys.append(xc.cpu().numpy()[:, None])
        nfs.append(nf.cpu().numpy()); sats += sat.cpu().numpy()
        logs.append(sol.stats())
    log = {f: np.stack([l[f] for l in logs], axis=1) for f in logs[0]}
    return np.concatenate(xs, axis=1), np.concatenate(us, axis=1), np.concatenate(ys, axis=1), log, np.stack(nfs, axis=1), sats


@pytest.mark.parametrize("name,variant,warm", [("car_obs", 1, True), ("car_obs", 5, True), ("car_obs", 1, False), ("synth12", None, True)])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("delay", [0, 1])
def test_mpc_run_io_is_the_device_entry_points_one_by_one(pkg, name, variant, warm, k, delay):
    B, periods = 5, 3
    a, w = _solved(pkg, name, B, variant)
    b, _ = _solved(pkg, name, B, variant)
    x0 = R.plant_starts(a.get_trajectory()[0])
    w_plant = R.plant_parameters(np.concatenate([w, w], axis=1), periods * k) if w is not None else None
    u_min, u_max = IO.LIMITS[name]
    kw = dict(sigma_x=R.sigma_x(a.nx), seed=R.SEED, u_min=u_min, u_max=u_max, sigma_y=IO.sigma_y(a.nx), delay=delay)
    res = a.mpc_run_(periods, k, x0=x0, warm=warm, w_plant=w_plant, plant_feedback=True, **kw)
    x, u, y, log, nf, sat = _device_stepped(pkg, b, x0, periods, k, warm, w_plant, feedback=True, **kw)
    assert np.array_equal(res.x, x) and np.array_equal(res.u, u) and np.array_equal(res.y_cl, y)
    assert (res.first_nonfinite == -1).all() and (nf == -1).all()
    assert np.array_equal(res.saturated, sat) and sat.any()
    for f in log:
        assert _same(res.log[f], log[f]), f
    assert (res.log["iterations"] > 0).all()
    assert ((res.u >= u_min) & (res.u <= u_max)).all()                       # the actuator delivered nothing beyond its limits
    assert _differ(pkg, a, b) == []
    a.initialize_rollout_resident_(); b.initialize_rollout_resident_()
    a.synchronize(); b.synchronize()
    assert _differ(pkg, a, b) == []
    a.close(); b.close()


@pytest.mark.parametrize("delay", [0, 1])
def test_sharded_handle_equals_the_single_one(pkg, delay):
    B, periods, k = 7, 2, 2
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    x0 = R.plant_starts(one.get_trajectory()[0])
    u_min, u_max = IO.LIMITS["car_obs"]
    kw = dict(steps=3, feedback=True, sigma_x=R.sigma_x(3), seed=R.SEED, first_instance=11, step0=5, w_plant=R.plant_parameters(w, 3), u_min=u_min, u_max=u_max)
    p1, p2 = one.plant_step_(x0, **kw), two.plant_step_(x0, **kw)
    for key in p1:
        assert np.array_equal(p1[key], p2[key]), key
    m1, m2 = (s.plant_measure_(x0, step=4, sigma_y=IO.sigma_y(3), seed=R.SEED, first_instance=11) for s in (one, two))
    assert np.array_equal(m1, m2) and not np.array_equal(m1[0] - x0[0], m1[4] - x0[4])       # the second shard draws its own noise
    r1, r2 = (s.mpc_run_(periods, k, x0=x0, sigma_x=R.sigma_x(3), seed=R.SEED, first_instance=11, w_plant=R.plant_parameters(w, periods * k),
                         plant_feedback=True, score=True, u_min=u_min, u_max=u_max, sigma_y=IO.sigma_y(3), delay=delay) for s in (one, two))
    for key in ("x", "u", "first_nonfinite", "cl_cost", "cl_violation", "y_cl", "saturated"):
        assert _same(getattr(r1, key), getattr(r2, key)), key
    for f in r1.log:
        assert _same(r1.log[f], r2.log[f]), f
    assert _differ(pkg, one, two) == []
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
@pytest.mark.parametrize("empty_io", [False, True])
def test_null_io_is_mpc_run_preview(pkg, name, empty_io):
    B, periods, k = 5, 2, 2
    a, w = _solved(pkg, name, B)
    b, _ = _solved(pkg, name, B)
    x0 = R.plant_starts(a.get_trajectory()[0])
    Rr = periods * k
    w_plant = R.plant_parameters(w, Rr) if w is not None else None
    w_preview = None if w is None else np.ascontiguousarray(w[:, :Rr] + 0.05)
    sig = R.sigma_x(a.nx)
    want = b.mpc_run_(periods, k, x0=x0, sigma_x=sig, seed=R.SEED, w_plant=w_plant, w_preview=w_preview, score=True, plant_feedback=True)
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    d = pkg._ffi.MpcDesc(periods, k, 1, 0, 0, 1, 0, 0, R.SEED, 0, sig.ctypes.data_as(F64))
    io = pkg._ffi.PlantIO(None, None, None, 0, 0)
    x, u = np.empty((B, Rr + 1, a.nx)), np.empty((B, Rr, a.nu))
    log, nf, cost, viol = np.empty((B, periods, 9)), np.empty(B, dtype=np.int32), np.empty((B, Rr)), np.empty((B, Rr))
    p = lambda arr: None if arr is None else arr.ctypes.data_as(F64)
    pkg._ffi.check(L.ilqr_set_options(a._h, C.byref(a.options)))
    pkg._ffi.check(L.ilqr_mpc_run_io(a._h, C.byref(d), C.byref(io) if empty_io else None, p(x0), p(w_plant), p(w_preview), p(x), p(u), p(log),
                                     nf.ctypes.data_as(I32), p(cost), p(viol), None, None))
    assert np.array_equal(x, want.x) and np.array_equal(u, want.u) and np.array_equal(nf, want.first_nonfinite)
    assert _same(cost, want.cl_cost) and _same(viol, want.cl_violation)
    for c, f in enumerate(pkg._ffi.MPC_LOG_COLUMNS):
        assert _same(log[:, :, c], want.log[f].astype(np.float64)), f
    assert _differ(pkg, a, b) == []
    a.initialize_rollout_resident_(); b.initialize_rollout_resident_()
    a.synchronize(); b.synchronize()
    assert _differ(pkg, a, b) == []
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_delay_matters_exactly_when_it_should(pkg, name):
    B, periods, k = 5, 3, 2
    u_min, u_max = IO.LIMITS[name]
    base = dict(x0=None, plant_feedback=True, u_min=u_min, u_max=u_max)
    # nothing separates the plant from the controller's model: the prediction is the same kernel on the same bits
    runs = []
    for delay in (0, 1):
        sol, w = _solved(pkg, name, B)
        base["x0"] = R.plant_starts(sol.get_trajectory()[0])
        res = sol.mpc_run_(periods, k, delay=delay, **base)
        runs.append((res, _snapshot(sol)))
        sol.close()
    (r0, s0), (r1, s1) = runs
    for key in ("x", "u", "y_cl", "saturated", "first_nonfinite"):
        assert np.array_equal(getattr(r0, key), getattr(r1, key)), key
    for f in r0.log:
        assert _same(r0.log[f], r1.log[f]), f
    keep = pkg._ffi.lib().ilqr_scalar_slot(b"states_eq_nominal") + 1
    s0["_scalars"], s1["_scalars"] = s0["_scalars"][:, :keep], s1["_scalars"][:, :keep]
    assert _unchanged(s0, s1) == []
    assert np.array_equal(r0.y_cl, r0.x[:, k::k])                              # and what the controller was given is the plant state
    # process noise: the prediction cannot know it. Row p of y_cl is the yardstick's prediction from x_cl[p·k] under the plan in
    # flight, which a twin handle re-solved from the same y_cl holds
    a, w = _solved(pkg, name, B)
    twin, _ = _solved(pkg, name, B)
    res = a.mpc_run_(periods, k, delay=1, sigma_x=R.sigma_x(a.nx), seed=R.SEED, **base)
    assert (res.y_cl != res.x[:, k::k]).any(axis=2).all()
    f = R.dynamics(name)
    plans = []

    def predict(y, p):
        xb, ub, K, _ = _plan(twin, w)
        th = None if w is None else twin.buffer("parameters").reshape(B, T, -1)
        plans.append(p)
        return np.stack([IO.plant_step(f, xb[b], ub[b], K[b], None if th is None else th[b], y[b], k, True, u_min=u_min, u_max=u_max)["x"][-1]
                         for b in range(B)])

    def resolve(xc, p):
        twin.shift_horizon_(k, x1=res.y_cl[:, p]); twin.shift_duals_(k); twin.solve_warm_()

    ref = IO.run(res.x[:, 0], periods, k, 1, plant=lambda x, p: np.moveaxis(res.x[:, p * k:(p + 1) * k + 1], 1, 0), measure_=lambda x, step: x,
                 predict=predict, resolve=resolve)
    got, want = res.y_cl, np.moveaxis(ref["y"], 0, 1)
    worst = max(P.rel(got[b], want[b]) for b in range(B))
    print("delay 1 prediction %s: worst relative error %.2e" % (name, worst))
    assert plans == list(range(periods)) and worst < TOL_XU, worst
    assert _differ(pkg, a, twin) == []
    a.close(); twin.close()


# ----------------------------------------------------------------------------------------------------------------------- 8
def test_refusals_that_need_a_handle(pkg):
    B = 3
    Err = pkg._ffi.IlqrError

    def refused(sol, call, match):
        before = _snapshot(sol)
        with pytest.raises(Err, match=match):
            call()
        assert _unchanged(before, _snapshot(sol)) == []

    sh, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    buf = np.zeros((B, 3))
    refused(sh, lambda: sh.plant_step_device_(buf.ctypes.data, u_min=[-1.0, -1.0]), "sharded handle")
    refused(sh, lambda: sh.plant_measure_device_(buf.ctypes.data, buf.ctypes.data), "sharded handle")
    # what only the handle's dimensions decide: the entries behind the first
    x0 = sh.get_trajectory()[0][:, 0].copy()
    for kw, match in [(dict(u_min=[0.0, np.nan]), "NaN"), (dict(u_max=[0.0, np.nan]), "NaN"), (dict(u_min=[0.0, 1.0], u_max=[1.0, 0.5]), "u_min must not exceed u_max")]:
        refused(sh, lambda: sh.plant_step_(x0, **kw), match)
        refused(sh, lambda: sh.mpc_run_(2, **kw), match)
    for bad in (-1.0, np.inf, np.nan):
        refused(sh, lambda: sh.plant_measure_(x0, sigma_y=[0.0, 0.0, bad]), "sigma_y must be finite")
        refused(sh, lambda: sh.mpc_run_(2, sigma_y=[0.0, 0.0, bad]), "sigma_y must be finite")
    refused(sh, lambda: sh.plant_measure_(x0, first_instance=2 ** 23 - 2), "first_instance \\+ batch")
    sh.close()
