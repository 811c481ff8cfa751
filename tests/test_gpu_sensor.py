"""ilqr_estimate_update_linear, ilqr_plant_measure_linear and ilqr_mpc_run_sensor on the GPU. T = 11, built-in models car_obs (3 x 2),
acrobot (4 x 1), synth12 (large form, one tile) and synth32 (two tile panels); B = 3 and 70 (synth32: 3), handles solved as in
tests/test_gpu_estimator.py. Sensors, r and the readings: tests/sensor_ref.py (ny = 2, nx + 1, and 64 on synth12, 33 on synth32); the
bound TOL_XU = 1e-10 relative to max(1, max |reference|) is the project's own (tests/test_sensor_ref.py: the yardstick's two forms
agree within a tenth of it).

1. The update against the yardstick: every model, every ny, shared and per-instance H, with and without ŷ, and the range sensor of
   car_obs linearised on the host; P out is bit for bit symmetric, first_bad == −1.
2. With H the selection rows and the matching r the result is estimate_update_'s within TOL_XU (printed: whether bit for bit).
3. plant_measure_linear_ against the yardstick; with H = I, sigma_y and the same seed it is plant_measure_ bit for bit.
4. An instance's bits are the same at B = 3 and inside B = 70, and through the host and device forms; two device-form calls in a row
   with different r / sigma_y, their host arrays overwritten at once, give each its own values.
5. A NaN in one instance's P: first_bad is the first row whose s is bad there (the yardstick's), every other instance bit for bit; a
   non-finite entry of a host-side H is refused by the update, the measurement and the loop; a non-finite row of a per-instance H
   on the device stays inside its instance.
6. mpc_run_(estimator=dict(H=...)) is, bit for bit, the device entry points called one by one (delay 0 and 1; acrobot and synth12),
   and its xhat and pdiag are the yardstick loop's within TOL_XU when that loop is fed the device's own plans.
7. Without H mpc_run_ is what it was; with sensor NULL ilqr_mpc_run_sensor is ilqr_mpc_run_io.
8. A sharded handle [0, 0] equals the single one, also with a shared H and with every input and output array of the loop passed at
   once; the device forms are refused on it.
9. It filters: acrobot, H = [[1,0,0,0],[1,1,0,0]] — the estimate beats the raw encoders on both angles and prediction alone on the
   velocities (the conditions tests/test_sensor_ref.py shows on the yardstick with a factor of two to spare)."""
import numpy as np
import pytest

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
import sensor_ref as S
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU = 1e-10
T = R.T


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_estimate_update_linear", "ilqr_estimate_update_linear_device", "ilqr_plant_measure_linear", "ilqr_plant_measure_linear_device",
               "ilqr_mpc_run_sensor"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


def _solved(pkg, name, B, **kw):
    sol = pkg.Solver(model=name, horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE), **kw)
    x1, ub, w = R.inputs(pkg.workloads, name, B)
    if w is not None:
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol, w


def _plan(sol):
    (xb, ub), (K, _) = sol.get_trajectory(), sol.get_policy()
    return xb, ub, K


def _inputs(sol):
    """(x̂ [B, n], P [B, n, n], the states the readings are taken of)"""
    xb = sol.get_trajectory()[0]
    xh, ys = E.start(R.plant_starts(xb), sol.nx)
    return xh, E.p_start(sol.B, sol.nx), ys


def _errs(out, ref, b):
    return [P.rel(out["xhat"][b], ref["xhat"]), P.rel(out["P"][b], ref["P"]), P.rel(out["innovation"][b], ref["innovation"]),
            abs(out["nis"][b] - ref["nis"]) / max(1.0, abs(ref["nis"]))]


def _some(B):
    return range(B) if B <= 3 else (0, 1, 63, 64, 69)


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", S.MODELS)
def test_update_against_the_yardstick(pkg, name):
    worst = 0.0
    for B in R.BATCHES[name]:
        sol, _ = _solved(pkg, name, B)
        n = sol.nx
        xh, Ps, ys = _inputs(sol)
        for ny in S.NY[name]:
            for H in (S.sensor(n, ny), S.sensors(n, ny, B)):
                y = S.readings(H, ys)
                for yhat in (None, S.some_yhat(y)):
                    out = sol.estimate_update_linear_(xh, Ps, y, H, S.r(ny), yhat=yhat)
                    assert np.array_equal(out["P"], out["P"].transpose(0, 2, 1)) and (out["first_bad"] == -1).all()
                    for b in _some(B):
                        ref = S.update_sequential(xh[b], Ps[b], y[b], H if H.ndim == 2 else H[b], S.r(ny), None if yhat is None else yhat[b])
                        errs = _errs(out, ref, b)
                        worst = max(worst, max(errs))
                        print("sensor %s B=%d ny=%d H%dd yhat=%d b=%d: %s" % (name, B, ny, H.ndim, yhat is not None, b, " ".join("%.2e" % e for e in errs)))
                        assert max(errs) < TOL_XU, (name, B, ny, H.ndim, yhat is not None, b, errs)
        if name == "car_obs":                      # the range to the origin and the heading, linearised on the host at x̂
            H, yhat, y, rr = S.range_sensor(xh, ys)
            out = sol.estimate_update_linear_(xh, Ps, y, H, rr, yhat=yhat)
            assert np.array_equal(out["P"], out["P"].transpose(0, 2, 1)) and (out["first_bad"] == -1).all()
            for b in _some(B):
                errs = _errs(out, S.update_sequential(xh[b], Ps[b], y[b], H[b], rr, yhat[b]), b)
                worst = max(worst, max(errs))
                print("sensor car_obs range B=%d b=%d: %s" % (B, b, " ".join("%.2e" % e for e in errs)))
                assert max(errs) < TOL_XU, (B, b, errs)
        sol.close()
    print("sensor %s: worst relative error %.2e" % (name, worst))


# ----------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", S.MODELS)
def test_selection_rows_are_estimate_update(pkg, name):
    B = R.BATCHES[name][-1]
    sol, _ = _solved(pkg, name, B)
    n = sol.nx
    xh, Ps, y = _inputs(sol)
    for mask in E.masks(name, n):
        idx = np.flatnonzero(mask)
        lin = sol.estimate_update_linear_(xh, Ps, np.ascontiguousarray(y[:, idx]), S.selection(mask), E.r(n)[idx])
        sel = sol.estimate_update_(xh, Ps, y, E.r(n), measured=mask)
        errs = [P.rel(lin["xhat"], sel["xhat"]), P.rel(lin["P"], sel["P"]), P.rel(lin["innovation"], sel["innovation"][:, idx]),
                P.rel(lin["nis"], sel["nis"])]
        same = all(np.array_equal(lin[k], sel[k]) for k in ("xhat", "P", "nis")) and np.array_equal(lin["innovation"], sel["innovation"][:, idx])
        print("selection %s B=%d measured=%d: %s, bit for bit: %s" % (name, B, len(idx), " ".join("%.2e" % e for e in errs), same))
        assert max(errs) < TOL_XU and np.array_equal(lin["first_bad"], sel["first_bad"]), (name, errs)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", S.MODELS)
def test_measurement_against_the_yardstick(pkg, name):
    step, first = 7, 5
    for B in R.BATCHES[name]:
        sol, _ = _solved(pkg, name, B)
        n = sol.nx
        x = R.plant_starts(sol.get_trajectory()[0])
        z = pkg.candidate_noise(R.SEED, first + B, *IO.measure_shape(step))[first:]
        for ny in S.NY[name]:
            H, sy = S.sensor(n, ny), S.sigma_y(ny)
            y = sol.plant_measure_linear_(x, H, step=step, sigma_y=sy, seed=R.SEED, first_instance=first)
            y0 = sol.plant_measure_linear_(x, H, step=step)
            for b in _some(B):
                e, e0 = P.rel(y[b], S.measure(x[b], H, sy, z[b], step)), P.rel(y0[b], S.measure(x[b], H, None, None, step))
                print("measure %s B=%d ny=%d b=%d: %.2e %.2e" % (name, B, ny, b, e, e0))
                assert e < TOL_XU and e0 < TOL_XU, (name, B, ny, b, e, e0)
            assert np.array_equal(y[:, sy == 0.0], y0[:, sy == 0.0]) and not np.array_equal(y[:, sy != 0.0], y0[:, sy != 0.0])
        sy = IO.sigma_y(n)
        assert np.array_equal(sol.plant_measure_linear_(x, np.eye(n), step=step, sigma_y=sy, seed=R.SEED, first_instance=first),
                              sol.plant_measure_(x, step=step, sigma_y=sy, seed=R.SEED, first_instance=first))
        sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["car_obs", "acrobot", "synth12"])
def test_an_instance_does_not_depend_on_its_batch_or_on_the_form(pkg, name):
    import torch
    big, _ = _solved(pkg, name, 70)
    small, _ = _solved(pkg, name, 3)
    n = big.nx
    ny = S.NY[name][1]
    xh, Ps, ys = _inputs(big)
    H, rr, sy = S.sensors(n, ny, 70), S.r(ny), S.sigma_y(ny)
    y = S.readings(H, ys)
    yhat = S.some_yhat(y)
    o70 = big.estimate_update_linear_(xh, Ps, y, H, rr, yhat=yhat)
    o3 = small.estimate_update_linear_(xh[:3], Ps[:3], y[:3], H[:3], rr, yhat=yhat[:3])
    for key in o3:
        assert np.array_equal(o70[key][:3], o3[key]), key
    m70 = big.plant_measure_linear_(xh, H[0], step=3, sigma_y=sy, seed=R.SEED)
    assert np.array_equal(m70[:3], small.plant_measure_linear_(xh[:3], H[0], step=3, sigma_y=sy, seed=R.SEED))
    # the device forms, on the caller's device arrays
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(big.stream_ptr())):
        dx, dP, dy, dyh, dH, dH0 = (torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev) for a in (xh, Ps, y, yhat, H, H[0]))
        dinn, dnis = torch.zeros(70, ny, dtype=torch.float64, device=dev), torch.zeros(70, dtype=torch.float64, device=dev)
        dbad, dm = torch.zeros(70, dtype=torch.int32, device=dev), torch.zeros(70, ny, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    big.plant_measure_linear_device_(dx.data_ptr(), dm.data_ptr(), dH0.data_ptr(), ny, step=3, sigma_y=sy, seed=R.SEED)
    big.estimate_update_linear_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), dH.data_ptr(), ny, rr, per_instance_H=True, d_yhat_ptr=dyh.data_ptr(),
                                       d_innovation_ptr=dinn.data_ptr(), d_nis_ptr=dnis.data_ptr(), d_first_bad_ptr=dbad.data_ptr())
    big.synchronize()
    assert np.array_equal(dm.cpu().numpy(), m70)
    for key, t in (("xhat", dx), ("P", dP), ("innovation", dinn), ("nis", dnis), ("first_bad", dbad)):
        assert np.array_equal(t.cpu().numpy(), o70[key]), key
    # a shared H through the device form against the host form
    with torch.cuda.stream(torch.cuda.ExternalStream(big.stream_ptr())):
        dx.copy_(torch.from_numpy(xh)); dP.copy_(torch.from_numpy(Ps))
    torch.cuda.synchronize()
    big.estimate_update_linear_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), dH0.data_ptr(), ny, rr)
    big.synchronize()
    shared = big.estimate_update_linear_(xh, Ps, y, H[0], rr)
    assert np.array_equal(dx.cpu().numpy(), shared["xhat"]) and np.array_equal(dP.cpu().numpy(), shared["P"])
    # r and sigma_y of a device form are read when the call is made: two calls with different values and nothing between them, from
    # host arrays that are overwritten as soon as the call returns
    with torch.cuda.stream(torch.cuda.ExternalStream(big.stream_ptr())):
        dx.copy_(torch.from_numpy(xh)); dP.copy_(torch.from_numpy(Ps))
        dx2, dP2, dm2 = dx.clone(), dP.clone(), torch.zeros_like(dm)
    torch.cuda.synchronize()
    r1, r2, s1, s2 = rr.copy(), 3.0 * rr, sy.copy(), 2.0 * sy
    big.estimate_update_linear_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), dH0.data_ptr(), ny, r1)
    r1[:] = 7.0
    big.estimate_update_linear_device_(dx2.data_ptr(), dP2.data_ptr(), dy.data_ptr(), dH0.data_ptr(), ny, r2)
    r2[:] = 7.0
    big.plant_measure_linear_device_(dx.data_ptr(), dm.data_ptr(), dH0.data_ptr(), ny, step=3, sigma_y=s1, seed=R.SEED)
    s1[:] = 0.5
    big.plant_measure_linear_device_(dx.data_ptr(), dm2.data_ptr(), dH0.data_ptr(), ny, step=3, sigma_y=s2, seed=R.SEED)
    s2[:] = 0.5
    big.synchronize()
    other = big.estimate_update_linear_(xh, Ps, y, H[0], 3.0 * rr)
    assert np.array_equal(dx.cpu().numpy(), shared["xhat"]) and np.array_equal(dP.cpu().numpy(), shared["P"])
    assert np.array_equal(dx2.cpu().numpy(), other["xhat"]) and np.array_equal(dP2.cpu().numpy(), other["P"])
    assert np.array_equal(dm.cpu().numpy(), big.plant_measure_linear_(shared["xhat"], H[0], step=3, sigma_y=sy, seed=R.SEED))
    assert np.array_equal(dm2.cpu().numpy(), big.plant_measure_linear_(shared["xhat"], H[0], step=3, sigma_y=2.0 * sy, seed=R.SEED))
    big.close(); small.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name,B", [("car_obs", 70), ("acrobot", 3), ("synth12", 3), ("synth32", 3)])
def test_a_bad_instance_stays_alone(pkg, name, B):
    sol, _ = _solved(pkg, name, B)
    n = sol.nx
    ny = S.NY[name][1]
    xh, Ps, ys = _inputs(sol)
    H, rr = S.sensors(n, ny, B), S.r(ny)
    y = S.readings(H, ys)
    clean = sol.estimate_update_linear_(xh, Ps, y, H, rr)
    bad_b = B - 2
    others = np.arange(B) != bad_b
    Pn = Ps.copy(); Pn[bad_b, 1, 1] = np.nan
    out = sol.estimate_update_linear_(xh, Pn, y, H, rr)
    ref = S.update_sequential(xh[bad_b], Pn[bad_b], y[bad_b], H[bad_b], rr)
    assert ref["first_bad"] >= 0 and out["first_bad"][bad_b] == ref["first_bad"] and out["innovation"][bad_b, ref["first_bad"]] == 0.0
    assert (out["first_bad"][others] == -1).all()
    for key in clean:
        assert np.array_equal(out[key][others], clean[key][others]), key
    # a non-finite entry of an H given on the host is refused before any launch: per instance, shared, the measurement, the loop
    import torch
    Hn = H.copy(); Hn[bad_b, 1, :] = np.inf
    H1 = H[0].copy(); H1[ny - 1, n - 1] = np.nan
    for call in (lambda: sol.estimate_update_linear_(xh, Ps, y, Hn, rr), lambda: sol.estimate_update_linear_(xh, Ps, y, H1, rr),
                 lambda: sol.plant_measure_linear_(xh, Hn[bad_b]), lambda: sol.plant_measure_linear_(xh, H1),
                 lambda: sol.mpc_run_(1, 1, estimator=dict(H=Hn[bad_b], r=rr, P0=Ps)), lambda: sol.mpc_run_(1, 1, estimator=dict(H=H1, r=rr, P0=Ps))):
        with pytest.raises(pkg._ffi.IlqrError, match="non-finite entry of H"):
            call()
    again = sol.estimate_update_linear_(xh, Ps, y, H, rr)                     # nothing was launched or changed by the refused calls
    for key in clean:
        assert np.array_equal(again[key], clean[key]), key
    # a non-finite row of one instance's H through the device form, which cannot look at a device array
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
        dx, dP, dy, dH = (torch.from_numpy(a.copy()).to(dev) for a in (xh, Ps, y, Hn))
        dbad = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sol.estimate_update_linear_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), dH.data_ptr(), ny, rr, per_instance_H=True, d_first_bad_ptr=dbad.data_ptr())
    sol.synchronize()
    assert dbad.cpu().numpy()[bad_b] == 1 and (dbad.cpu().numpy()[others] == -1).all()
    assert np.array_equal(dx.cpu().numpy()[others], clean["xhat"][others]) and np.array_equal(dP.cpu().numpy()[others], clean["P"][others])
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
def _device_stepped(sol, x0, xhat0, P0, periods, k, delay, sens, seed):
    """ilqr_mpc_run_sensor's definition: the device entry points called one by one from the host"""
    import torch
    B, n, m, ny = sol.B, sol.nx, sol.nu, sens["H"].shape[0]
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
        xp, xh, Pc, dH = (torch.from_numpy(a.copy()).to(dev) for a in (x0, xhat0, P0, sens["H"]))
        y, nis = torch.zeros(B, ny, **f64), torch.zeros(B, **f64)
        xo, uo = torch.zeros(B, k + 1, n, **f64), torch.zeros(B, k, m, **f64)
    torch.cuda.synchronize()
    xs, us, ys, hs, ds, ns, plans = [x0[:, None]], [], [], [], [], [], []
    upd = lambda: sol.estimate_update_linear_device_(xh.data_ptr(), Pc.data_ptr(), y.data_ptr(), dH.data_ptr(), ny, sens["r"], d_nis_ptr=nis.data_ptr())
    prd = lambda: sol.estimate_predict_device_(xh.data_ptr(), Pc.data_ptr(), steps=k, feedback=True, q=sens["q"])
    msr = lambda step: sol.plant_measure_linear_device_(xp.data_ptr(), y.data_ptr(), dH.data_ptr(), ny, step=step, sigma_y=sens["sigma_y"], seed=seed)
    for p in range(periods):
        plans.append(_plan(sol))
        if delay:
            msr(p * k); upd(); prd()
        sol.plant_step_device_(xp.data_ptr(), steps=k, feedback=True, seed=seed, step0=p * k, d_x_out_ptr=xo.data_ptr(), d_u_out_ptr=uo.data_ptr())
        if not delay:
            msr((p + 1) * k); prd(); upd()
        sol.shift_horizon_device_(k, xh.data_ptr())
        sol.shift_duals_(k)
        sol.solve_warm_()
        sol.synchronize()
        xs.append(xo.cpu().numpy()[:, 1:]); us.append(uo.cpu().numpy()); ys.append(y.cpu().numpy()[:, None]); hs.append(xh.cpu().numpy()[:, None])
        ds.append(np.diagonal(Pc.cpu().numpy(), axis1=1, axis2=2)[:, None].copy()); ns.append(nis.cpu().numpy()[:, None])
    cat = lambda a: np.concatenate(a, axis=1)
    return dict(x=cat(xs), u=cat(us), y_cl=cat(ys), xhat=cat(hs), pdiag=cat(ds), nis=cat(ns), P=Pc.cpu().numpy()), plans


@pytest.mark.parametrize("name", ["acrobot", "synth12"])
@pytest.mark.parametrize("delay", [0, 1])
def test_mpc_run_sensor_is_the_device_entry_points_one_by_one(pkg, name, delay):
    B, periods, k = 3, 3, 2
    a, _ = _solved(pkg, name, B)
    b, _ = _solved(pkg, name, B)
    n = a.nx
    ny = S.NY[name][1]
    x0 = R.plant_starts(a.get_trajectory()[0])
    xh0, _ = E.start(x0, n)
    P0 = E.p_start(B, n)
    sens = dict(H=S.sensor(n, ny), r=S.r(ny), q=E.q(n), sigma_y=S.sigma_y(ny))
    res = a.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, delay=delay, estimator=dict(xhat0=xh0, P0=P0, **sens))
    one, plans = _device_stepped(b, x0, xh0, P0, periods, k, delay, sens, R.SEED)
    assert res.y_cl.shape == (B, periods, ny)
    for key, val in one.items():
        assert np.array_equal(getattr(res, key), val, equal_nan=True), key
    assert (res.log["iterations"] > 0).all() and (res.nis > 0.0).all()
    # the yardstick loop, fed the device's own plans
    z = pkg.candidate_noise(R.SEED, B, *IO.measure_shape(periods * k))
    f = R.dynamics(name)
    for i in range(B):
        plan = lambda p: tuple(arr[i] for arr in plans[p])
        ref = E.run(x0[i], xh0[i], P0[i], periods, k, delay,
                    lambda x, p: IO.plant_step(f, *plan(p), None, x, k, True)["x"],
                    lambda x, step: S.measure(x, sens["H"], sens["sigma_y"], z[i], step),
                    lambda xh, Pc, p: E.predict(name, *plan(p), None, xh, Pc, k, True, q=sens["q"]),
                    lambda xh, Pc, y: S.update_sequential(xh, Pc, y, sens["H"], sens["r"]),
                    lambda xc, p: None)
        ex, ed = P.rel(res.xhat[i], ref["xhat"]), P.rel(res.pdiag[i], ref["pdiag"])
        print("sensor loop %s delay %d instance %d: xhat %.2e pdiag %.2e" % (name, delay, i, ex, ed))
        assert ex < TOL_XU and ed < TOL_XU, (name, delay, i, ex, ed)
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 7, 8
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_no_sensor_is_mpc_run_io(pkg, name):
    import ctypes as C
    B, periods, k = 5, 2, 2
    a, _ = _solved(pkg, name, B)
    b, _ = _solved(pkg, name, B)
    c, _ = _solved(pkg, name, B)
    n = a.nx
    x0 = R.plant_starts(a.get_trajectory()[0])
    u_min, u_max = IO.LIMITS[name]
    sy = IO.sigma_y(n)
    want = b.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, sigma_y=sy, delay=1, u_min=u_min, u_max=u_max)
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    p = lambda arr: None if arr is None else arr.ctypes.data_as(F64)
    d = pkg._ffi.MpcDesc(periods, k, 1, 0, 0, 1, 0, 0, R.SEED, 0, None)
    io = pkg._ffi.PlantIO(p(u_min), p(u_max), p(sy), 1, 0)
    Rr = periods * k
    x, u, log = np.empty((B, Rr + 1, n)), np.empty((B, Rr, a.nu)), np.empty((B, periods, 9))
    nf, sat, ycl = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32), np.empty((B, periods, n))
    pkg._ffi.check(L.ilqr_set_options(a._h, C.byref(a.options)))
    pkg._ffi.check(L.ilqr_mpc_run_sensor(a._h, C.byref(d), C.byref(io), None, p(x0), None, None, None, None, p(x), p(u), p(log), nf.ctypes.data_as(I32),
                                         None, None, p(ycl), sat.ctypes.data_as(I32), None, None, None))
    assert np.array_equal(x, want.x) and np.array_equal(u, want.u) and np.array_equal(ycl, want.y_cl)
    assert np.array_equal(nf, want.first_nonfinite) and np.array_equal(sat, want.saturated)
    for col, f in enumerate(pkg._ffi.MPC_LOG_COLUMNS):
        assert np.array_equal(log[:, :, col], want.log[f].astype(np.float64), equal_nan=True), f
    # the selection filter of mpc_run_(estimator=dict(measured=...)) equals the sensor path with the selection rows within TOL_XU
    mask = E.masks(name, n)[0]
    idx = np.flatnonzero(mask)
    xh0, _ = E.start(x0, n)
    # (no measurement noise: output j of the sensor draws from the key of j, not of the state component it selects)
    b.close()
    b, _ = _solved(pkg, name, B)                   # a fresh handle: the same plan as c's
    sel = b.mpc_run_(1, k, x0=x0, seed=R.SEED, estimator=dict(measured=mask, q=E.q(n), r=E.r(n), xhat0=xh0, P0=E.p_start(B, n)))
    lin = c.mpc_run_(1, k, x0=x0, seed=R.SEED, estimator=dict(H=S.selection(mask), q=E.q(n), r=E.r(n)[idx], xhat0=xh0, P0=E.p_start(B, n)))
    assert P.rel(lin.xhat, sel.xhat) < TOL_XU and P.rel(lin.pdiag, sel.pdiag) < TOL_XU and np.array_equal(lin.x, sel.x)
    with pytest.raises(ValueError, match="exclude each other"):
        c.mpc_run_(1, k, estimator=dict(H=S.selection(mask), measured=mask, r=E.r(n)[idx], P0=E.p_start(B, n)))
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("delay", [0, 1])
def test_sharded_handle_equals_the_single_one(pkg, delay):
    B, periods, k = 7, 2, 2
    one, _ = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    n, ny = one.nx, 4
    x0 = R.plant_starts(one.get_trajectory()[0])
    xh, Ps, ys = _inputs(one)
    H = S.sensors(n, ny, B)
    y = S.readings(H, ys)
    u1, u2 = (s.estimate_update_linear_(xh, Ps, y, H, S.r(ny), yhat=S.some_yhat(y)) for s in (one, two))
    for key in u1:
        assert np.array_equal(u1[key], u2[key]), key
    m1, m2 = (s.plant_measure_linear_(x0, H[0], step=3, sigma_y=S.sigma_y(ny), seed=R.SEED, first_instance=11) for s in (one, two))
    assert np.array_equal(m1, m2)
    est = dict(H=H[0], q=E.q(n), r=S.r(ny), sigma_y=S.sigma_y(ny), xhat0=xh, P0=Ps)
    r1, r2 = (s.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, first_instance=11, delay=delay, estimator=est) for s in (one, two))
    for key in ("x", "u", "y_cl", "saturated", "xhat", "pdiag", "nis", "P"):
        assert np.array_equal(getattr(r1, key), getattr(r2, key), equal_nan=True), key
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        two.estimate_update_linear_device_(1, 1, 1, 1, ny, S.r(ny))
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        two.plant_measure_linear_device_(1, 1, 1, ny)
    one.close(); two.close()


def test_sharded_loop_with_every_array_equals_the_single_one(pkg):
    """every input and output array of ilqr_mpc_run_sensor at once, and the update with an H the batch shares (it is not sliced):
    B = 7 (shards of 4 and 3), ny = 3"""
    B, periods, k = 7, 2, 2
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    n, ny = one.nx, 3
    x0 = R.plant_starts(one.get_trajectory()[0])
    xh, Ps, ys = _inputs(one)
    H = S.sensors(n, ny, B)[1]
    y = S.readings(H, ys)
    u1, u2 = (s.estimate_update_linear_(xh, Ps, y, H, S.r(ny)) for s in (one, two))
    for key in u1:
        assert np.array_equal(u1[key], u2[key]), key
    u_min, u_max = IO.LIMITS["car_obs"]
    wp = R.plant_parameters(w, periods * k)
    est = dict(H=H, q=E.q(n), r=S.r(ny), sigma_y=S.sigma_y(ny), xhat0=xh, P0=Ps)
    r1, r2 = (s.mpc_run_(periods, k, x0=x0, plant_feedback=True, sigma_x=R.sigma_x(n), seed=R.SEED, first_instance=11, w_plant=wp,
                         w_preview=np.ascontiguousarray(wp[:, ::-1]), score=True, u_min=u_min, u_max=u_max, estimator=est) for s in (one, two))
    for key in ("x", "u", "first_nonfinite", "cl_cost", "cl_violation", "y_cl", "saturated", "xhat", "pdiag", "nis", "P"):
        assert np.array_equal(getattr(r1, key), getattr(r2, key), equal_nan=True), key
    for f in r1.log:
        assert np.array_equal(r1.log[f], r2.log[f], equal_nan=True), f
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 9
def test_it_filters(pkg):
    F = S.FILTER
    B, k = F["B"], F["k"]
    sol = pkg.Solver(model=F["name"], horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE))
    x1, ub, _ = R.inputs(pkg.workloads, F["name"], B)
    sol.initialize_rollout_(x1, ub)                # the fixed plan: the nominal actions, no feedback, no re-solve
    sy, rr, qq, xh, Pc = S.filter_inputs(x1)
    x, xo = x1.copy(), xh.copy()
    xs, ys, hs, os_ = [], [], [], []
    for p in range(F["periods"]):
        x = sol.plant_step_(x, steps=k)["x"][:, -1]
        y = sol.plant_measure_linear_(x, S.FILTER_H, step=(p + 1) * k, sigma_y=sy, seed=F["seed"])
        xh, Pc = sol.estimate_predict_(xh, Pc, steps=k, q=qq)
        out = sol.estimate_update_linear_(xh, Pc, y, S.FILTER_H, rr)
        xh, Pc = out["xhat"], out["P"]
        xo = sol.plant_step_(xo, steps=k)["x"][:, -1]
        xs.append(x); ys.append(y); hs.append(xh); os_.append(xo)
    run = {key: np.stack(v, axis=1) for key, v in (("x", xs), ("y", ys), ("xhat", hs), ("open", os_))}
    q1_hat, q1_raw, q2_hat, q2_raw, vel_hat, vel_open = S.filter_scores(run)
    print("filter on the device: q1 %.3e (raw %.3e), q2 %.3e (raw %.3e), velocities %.3e (prediction alone %.3e)"
          % (q1_hat, q1_raw, q2_hat, q2_raw, vel_hat, vel_open))
    assert q1_hat < q1_raw and q2_hat < q2_raw and vel_hat < vel_open
    sol.close()
