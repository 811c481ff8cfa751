"""ilqr_sensor_linearise, ilqr_plant_measure_sensor, ilqr_estimate_update_sensor and ilqr_mpc_run_nlsensor on the GPU. T = 11, the
handles of tests/test_gpu_sensor.py (car_obs, acrobot, synth12, synth32; B = 3 and 70, synth32: 3), the sensors, parameters and
readings of tests/sensor_nl_ref.py, compiled by api.compile_sensor (served from the module cache the build leaves).

1. Linearise and measure against the yardstick: H, ŷ and y of every sensor within 1e-12 relative to max(1, max |reference|), the
   stage-wise bound of tests/test_gpu_parity.py for generated function values (the worst figure is printed); with sigma_y None the
   measurement is the linearisation's ŷ bit for bit; with noise y − h(x) is sigma_y · z of candidate_noise to the rounding of one add;
   range + heading reproduces sensor_ref.range_sensor's host arrays.
2. estimate_update_sensor_(iterations=1) is sensor_linearise_device_ followed by estimate_update_linear_device_(per_instance_H,
   yhat) bit for bit; for range + heading it is estimate_update_linear_ fed the host arrays within TOL_XU; P out is symmetric.
3. iterations = 3 against the yardstick's iterated filter within TOL_XU = 1e-10; x_prior = x_lin given explicitly changes ŷ by at
   most the rounding of a chain of zero corrections (here: nothing).
4. An instance's bits are the same at B = 3 and inside B = 70, through the host and the device forms, and with a shared s or a
   per-instance s whose rows are all equal.
5. A NaN in one instance's x̂ or s row: that instance's first_bad is the yardstick's, every other instance bit for bit; a non-finite
   host s, a wrong nx, an unknown name and iterations 0 or 9 are refused by the call and by the loop.
6. mpc_run_(estimator=dict(sensor=...)) is bit for bit the device entry points called one by one (delay 0 and 1; acrobot and
   synth12; iterations 1 and 2); without `sensor` it is what it was; with the struct NULL ilqr_mpc_run_nlsensor is ilqr_mpc_run_io.
7. A sharded handle [0, 0] equals the single one; the device forms are refused on it.
8. It filters: car_obs, two beacon ranges and no heading reading — the estimate beats prediction alone, and with the wide P0 three
   iterations are no worse than one (tests/test_sensor_nl_ref.py shows both on the yardstick with a factor of two to spare)."""
import numpy as np
import pytest

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
import sensor_nl_ref as N
import sensor_ref as S
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_F = 1e-12
TOL_XU = 1e-10
T = R.T
KEYS = sorted(N.SENSORS)


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_sensor_linearise", "ilqr_plant_measure_sensor", "ilqr_estimate_update_sensor", "ilqr_estimate_update_sensor_device",
               "ilqr_mpc_run_nlsensor"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


def _solved(pkg, name, B, **kw):
    sol = pkg.Solver(model=name, horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE), **kw)
    x1, ub, w = R.inputs(pkg.workloads, name, B)
    if w is not None:
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol


def _inputs(sol):
    """(x̂ [B, n], P [B, n, n], the states the readings are taken of)"""
    xb = sol.get_trajectory()[0]
    xh, ys = E.start(R.plant_starts(xb), sol.nx)
    return xh, E.p_start(sol.B, sol.nx), ys


def _some(B):
    return range(B) if B <= 3 else (0, 1, 63, 64, 69)


def _sb(s, b):
    return s if s.ndim == 1 else s[b]


def _dev(sol, *arrays):
    import torch
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
        out = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev) for a in arrays]
    torch.cuda.synchronize()
    return out


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("key", KEYS)
def test_linearise_and_measure_against_the_yardstick(pkg, key):
    name, _, ny, _, _ = N.SENSORS[key]
    sens = N.compiled(pkg, key)
    step, first = 7, 5
    worst = 0.0
    for B in R.BATCHES[name]:
        sol = _solved(pkg, name, B)
        xh, _, ys = _inputs(sol)
        z = pkg.candidate_noise(R.SEED, first + B, *IO.measure_shape(step))[first:]
        sy = N.sigma_y(ny)
        for s in (N.s_shared(key), N.s_instances(key, B)):
            H, yhat = sol.sensor_linearise_(sens, xh, s=s)
            Hp, yp = sol.sensor_linearise_(sens, xh, s=s, x_prior=ys)
            y0 = sol.plant_measure_sensor_(sens, xh, s=s, step=step)
            y = sol.plant_measure_sensor_(sens, xh, s=s, step=step, sigma_y=sy, seed=R.SEED, first_instance=first)
            assert np.array_equal(y0, yhat) and np.array_equal(Hp, H)
            assert np.array_equal(y[:, sy == 0.0], y0[:, sy == 0.0]) and not np.array_equal(y[:, sy != 0.0], y0[:, sy != 0.0])
            for b in _some(B):
                Hr, yr = N.linearise(key, xh[b], _sb(s, b))
                _, ypr = N.linearise(key, xh[b], _sb(s, b), ys[b])
                errs = [P.rel(H[b], Hr), P.rel(yhat[b], yr), P.rel(yp[b], ypr), P.rel(y[b], N.measure(key, xh[b], _sb(s, b), sy, z[b], step))]
                worst = max(worst, max(errs))
                print("sensor %s B=%d s%dd b=%d: H %.2e yhat %.2e yhat(prior) %.2e y %.2e" % ((key, B, s.ndim, b) + tuple(errs)))
                assert max(errs) < TOL_F, (key, B, s.ndim, b, errs)
                # the noise is sigma_y · z to the rounding of one add (one ulp of the larger of y and h(x)); z itself is the host twin's
                # within a few ulp (ilqr_device_sample.hpp: libm's log and cos against the device's), taken as 1e-14 of the noise
                noise = np.array([sy[j] * z[b][IO.MEASURE_ROW0 + j // 16, step, j % 16] for j in range(ny)])
                assert (np.abs((y[b] - y0[b]) - noise) <= 2.0 ** -52 * np.maximum(np.abs(y[b]), np.abs(y0[b])) + 1e-14 * np.abs(noise)).all(), (key, b)
        if key == "range_heading":
            Hh, yh, _, _ = S.range_sensor(xh, ys)
            H, yhat = sol.sensor_linearise_(sens, xh)
            assert P.rel(H, Hh) < TOL_F and P.rel(yhat, yh) < TOL_F
        sol.close()
    print("sensor %s: worst relative error %.2e (bound %.1e)" % (key, worst, TOL_F))


def test_dydx_arrives_zeroed_in_both_kernels(pkg):
    """a hand-written sensor that accumulates into dydx and reads an unwritten partial back into y (sensor_nl_ref.READBACK_SOURCE):
    exact in the linearisation and in the measurement alike, lanes past a wave boundary included"""
    sens = N.compiled_readback(pkg)
    sol = _solved(pkg, "acrobot", 70)
    xh, _, _ = _inputs(sol)
    H, yhat = sol.sensor_linearise_(sens, xh)
    y = sol.plant_measure_sensor_(sens, xh, step=2)
    want = np.zeros((70, 2, 4))
    want[:, 0, 0], want[:, 1, 1], want[:, 1, 2] = 1.0, 0.5 * xh[:, 2] + 0.5 * xh[:, 2], xh[:, 1]
    assert np.array_equal(H, want) and np.array_equal(yhat, np.stack([xh[:, 0], xh[:, 1] * xh[:, 2]], axis=1)) and np.array_equal(y, yhat)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 2, 3
@pytest.mark.parametrize("key", KEYS)
def test_update_is_the_composition_and_the_iterated_filter_the_yardstick(pkg, key):
    import torch
    name, _, ny, _, _ = N.SENSORS[key]
    sens = N.compiled(pkg, key)
    B = R.BATCHES[name][-1]
    sol = _solved(pkg, name, B)
    n = sol.nx
    xh, Ps, ys = _inputs(sol)
    rr = N.r(ny)
    for s in (N.s_shared(key), N.s_instances(key, B)):
        y = N.readings(key, ys, s)
        one = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s)
        assert np.array_equal(one["P"], one["P"].transpose(0, 2, 1)) and (one["first_bad"] == -1).all()
        # the two existing device calls in sequence
        dx, dP, dy = _dev(sol, xh, Ps, y)
        ds = _dev(sol, s)[0] if s.size else None
        f64 = dict(dtype=torch.float64, device=dx.device)
        dH, dyh, dinn, dnis = torch.zeros(B, ny, n, **f64), torch.zeros(B, ny, **f64), torch.zeros(B, ny, **f64), torch.zeros(B, **f64)
        dbad = torch.zeros(B, dtype=torch.int32, device=dx.device)
        torch.cuda.synchronize()
        sp = None if ds is None else ds.data_ptr()
        sol.sensor_linearise_device_(sens, dx.data_ptr(), dH.data_ptr(), dyh.data_ptr(), d_s_ptr=sp, per_instance_s=s.ndim == 2)
        sol.estimate_update_linear_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), dH.data_ptr(), ny, rr, per_instance_H=True, d_yhat_ptr=dyh.data_ptr(),
                                           d_innovation_ptr=dinn.data_ptr(), d_nis_ptr=dnis.data_ptr(), d_first_bad_ptr=dbad.data_ptr())
        sol.synchronize()
        for k, t in (("xhat", dx), ("P", dP), ("innovation", dinn), ("nis", dnis), ("first_bad", dbad)):
            assert np.array_equal(t.cpu().numpy(), one[k]), (key, s.ndim, k)
        # the device form of the composite call
        dx2, dP2 = _dev(sol, xh, Ps)
        sol.estimate_update_sensor_device_(dx2.data_ptr(), dP2.data_ptr(), dy.data_ptr(), sens, rr, d_s_ptr=sp, per_instance_s=s.ndim == 2)
        sol.synchronize()
        assert np.array_equal(dx2.cpu().numpy(), one["xhat"]) and np.array_equal(dP2.cpu().numpy(), one["P"])
        # x_prior = x̂ given explicitly: a chain of zero corrections
        H0, yh0 = sol.sensor_linearise_(sens, xh, s=s)
        H1, yh1 = sol.sensor_linearise_(sens, xh, s=s, x_prior=xh)
        assert np.array_equal(H0, H1) and np.array_equal(yh0, yh1)
        three = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=3)
        assert np.array_equal(three["P"], three["P"].transpose(0, 2, 1)) and (three["first_bad"] == -1).all()
        dx3, dP3 = _dev(sol, xh, Ps)
        sol.estimate_update_sensor_device_(dx3.data_ptr(), dP3.data_ptr(), dy.data_ptr(), sens, rr, d_s_ptr=sp, per_instance_s=s.ndim == 2, iterations=3)
        sol.synchronize()
        assert np.array_equal(dx3.cpu().numpy(), three["xhat"]) and np.array_equal(dP3.cpu().numpy(), three["P"])
        for it, out in ((1, one), (3, three)):
            for b in _some(B):
                ref = N.update(key, xh[b], Ps[b], y[b], _sb(s, b), rr, it)
                errs = [P.rel(out["xhat"][b], ref["xhat"]), P.rel(out["P"][b], ref["P"]), P.rel(out["innovation"][b], ref["innovation"]),
                        abs(out["nis"][b] - ref["nis"]) / max(1.0, abs(ref["nis"]))]
                print("update %s s%dd iterations=%d b=%d: %s" % (key, s.ndim, it, b, " ".join("%.2e" % e for e in errs)))
                assert max(errs) < TOL_XU, (key, s.ndim, it, b, errs)
    if key == "range_heading":
        Hh, yh, y, r2 = S.range_sensor(xh, ys)
        lin, nl = sol.estimate_update_linear_(xh, Ps, y, Hh, r2, yhat=yh), sol.estimate_update_sensor_(xh, Ps, y, sens, r2)
        errs = [P.rel(nl[k], lin[k]) for k in ("xhat", "P", "innovation", "nis")]
        print("range + heading against the host linearisation: %s" % " ".join("%.2e" % e for e in errs))
        assert max(errs) < TOL_XU and np.array_equal(nl["first_bad"], lin["first_bad"])
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("key", ["beacons2", "encoder", "mix12", "wide12"])
def test_an_instance_does_not_depend_on_its_batch_or_on_the_form(pkg, key):
    import torch
    name, _, ny, ns, _ = N.SENSORS[key]
    sens = N.compiled(pkg, key)
    big, small = _solved(pkg, name, 70), _solved(pkg, name, 3)
    n = big.nx
    xh, Ps, ys = _inputs(big)
    s, rr, sy = N.s_instances(key, 70), N.r(ny), N.sigma_y(ny)
    y = N.readings(key, ys, s)
    for it in (1, 2):
        o70, o3 = big.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=it), small.estimate_update_sensor_(xh[:3], Ps[:3], y[:3], sens, rr, s=s[:3], iterations=it)
        for k in o3:
            assert np.array_equal(o70[k][:3], o3[k]), (key, it, k)
    H70, yh70 = big.sensor_linearise_(sens, xh, s=s, x_prior=ys)
    H3, yh3 = small.sensor_linearise_(sens, xh[:3], s=s[:3], x_prior=ys[:3])
    m70 = big.plant_measure_sensor_(sens, xh, s=s, step=3, sigma_y=sy, seed=R.SEED)
    assert np.array_equal(H70[:3], H3) and np.array_equal(yh70[:3], yh3)
    assert np.array_equal(m70[:3], small.plant_measure_sensor_(sens, xh[:3], s=s[:3], step=3, sigma_y=sy, seed=R.SEED))
    # a shared s and a per-instance s whose rows are all equal
    sh = N.s_shared(key)
    rows = np.ascontiguousarray(np.broadcast_to(sh, (70, ns)))
    a, c = big.estimate_update_sensor_(xh, Ps, y, sens, rr, s=sh, iterations=2), big.estimate_update_sensor_(xh, Ps, y, sens, rr, s=rows if ns else None, iterations=2)
    for k in a:
        assert np.array_equal(a[k], c[k]), (key, k)
    assert np.array_equal(big.plant_measure_sensor_(sens, xh, s=sh, step=3), big.plant_measure_sensor_(sens, xh, s=rows if ns else None, step=3))
    # the device forms, on the caller's device arrays
    dx, dxp, ds, dP, dy = _dev(big, xh, ys, s if ns else np.zeros(1), Ps, y)
    f64 = dict(dtype=torch.float64, device=dx.device)
    dH, dyh, dm = torch.zeros(70, ny, n, **f64), torch.zeros(70, ny, **f64), torch.zeros(70, ny, **f64)
    torch.cuda.synchronize()
    sp = ds.data_ptr() if ns else None
    big.sensor_linearise_device_(sens, dx.data_ptr(), dH.data_ptr(), dyh.data_ptr(), d_s_ptr=sp, per_instance_s=True, d_x_prior_ptr=dxp.data_ptr())
    big.plant_measure_sensor_device_(sens, dx.data_ptr(), dm.data_ptr(), d_s_ptr=sp, per_instance_s=True, step=3, sigma_y=sy, seed=R.SEED)
    big.synchronize()
    assert np.array_equal(dH.cpu().numpy(), H70) and np.array_equal(dyh.cpu().numpy(), yh70) and np.array_equal(dm.cpu().numpy(), m70)
    big.close(); small.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("key,B", [("beacons2", 70), ("mix12", 3), ("mix32", 3)])
def test_a_bad_instance_stays_alone_and_bad_arguments_are_refused(pkg, key, B):
    name, _, ny, ns, _ = N.SENSORS[key]
    sens = N.compiled(pkg, key)
    sol = _solved(pkg, name, B)
    xh, Ps, ys = _inputs(sol)
    s, rr = N.s_instances(key, B), N.r(ny)
    y = N.readings(key, ys, s)
    bad_b = B - 2
    others = np.arange(B) != bad_b
    for it in (1, 2):
        clean = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=it)
        xn = xh.copy(); xn[bad_b, 1] = np.nan
        out = sol.estimate_update_sensor_(xn, Ps, y, sens, rr, s=s, iterations=it)
        ref = N.update(key, xn[bad_b], Ps[bad_b], y[bad_b], s[bad_b], rr, it)
        assert ref["first_bad"] >= 0 and out["first_bad"][bad_b] == ref["first_bad"], (key, it, out["first_bad"][bad_b], ref["first_bad"])
        assert (out["first_bad"][others] == -1).all()
        for k in clean:
            assert np.array_equal(out[k][others], clean[k][others]), (key, it, k)
    # a NaN in one instance's s row reaches the device through the device form, which cannot look at a device array
    import torch
    sn = s.copy(); sn[bad_b, 0] = np.nan
    dx, dP, dy, ds = _dev(sol, xh, Ps, y, sn)
    dbad = torch.zeros(B, dtype=torch.int32, device=dx.device)
    torch.cuda.synchronize()
    sol.estimate_update_sensor_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), sens, rr, d_s_ptr=ds.data_ptr(), per_instance_s=True, d_first_bad_ptr=dbad.data_ptr())
    sol.synchronize()
    clean = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s)
    ref = N.update(key, xh[bad_b], Ps[bad_b], y[bad_b], sn[bad_b], rr, 1)
    assert ref["first_bad"] >= 0 and dbad.cpu().numpy()[bad_b] == ref["first_bad"] and (dbad.cpu().numpy()[others] == -1).all()
    assert np.array_equal(dx.cpu().numpy()[others], clean["xhat"][others]) and np.array_equal(dP.cpu().numpy()[others], clean["P"][others])
    # refused before any launch, by the call and by the loop
    E_ = pkg._ffi.IlqrError
    other = N.compiled(pkg, "encoder")             # a sensor of another nx (4), without parameters
    est = lambda **kw: dict(dict(sensor=sens, s=s, r=rr, P0=Ps), **kw)
    for call, msg in [(lambda: sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=sn), "non-finite entry of s"),
                      (lambda: sol.sensor_linearise_(sens, xh, s=sn), "non-finite entry of s"),
                      (lambda: sol.plant_measure_sensor_(sens, xh, s=sn), "non-finite entry of s"),
                      (lambda: sol.mpc_run_(1, 1, estimator=est(s=sn)), "non-finite entry of s"),
                      (lambda: sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=0), "iterations must lie in 1 .. 8"),
                      (lambda: sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=9), "iterations must lie in 1 .. 8"),
                      (lambda: sol.mpc_run_(1, 1, estimator=est(iterations=0)), "iterations must lie in 1 .. 8"),
                      (lambda: sol.mpc_run_(1, 1, estimator=est(iterations=9)), "iterations must lie in 1 .. 8"),
                      (lambda: sol.mpc_run_(1, 1, estimator=est(r=-rr)), "r must be finite and > 0"),
                      (lambda: pkg._ffi.check(pkg._ffi.lib().ilqr_sensor_linearise(sol._h, other.encode(), 0, None, xh.ctypes.data_as(pkg._ffi.c_double_p), None,
                                                                                  xh.ctypes.data_as(pkg._ffi.c_double_p), xh.ctypes.data_as(pkg._ffi.c_double_p))),
                       "the sensor's nx is not the handle's"),
                      (lambda: sol.estimate_update_sensor_device_(1, 1, 1, "no_such_sensor_x", rr), "unknown sensor")]:
        with pytest.raises(E_, match=msg):
            call()
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p
    import ctypes as C
    d = pkg._ffi.MpcDesc(1, 1, 0, 0, 0, 1, 0, 0, 0, 0, None)
    for sname, msg in ((b"no_such_sensor", b"unknown sensor"), (other.encode(), b"the sensor's nx is not the handle's")):
        nl = pkg._ffi.NlSensor(sname, 0, np.ones(64).ctypes.data_as(F64), np.ones(64).ctypes.data_as(F64), None, None, 1)
        assert L.ilqr_mpc_run_nlsensor(sol._h, C.byref(d), None, C.byref(nl), None, None, Ps.ctypes.data_as(F64), *([None] * 13)) == -1
        assert msg in L.ilqr_last_error(), L.ilqr_last_error()
    again = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s)                     # nothing was launched or changed by the refused calls
    for k in clean:
        assert np.array_equal(again[k], clean[k]), k
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
def _device_stepped(sol, x0, xhat0, P0, periods, k, delay, sens, est, seed):
    """ilqr_mpc_run_nlsensor's definition: the device entry points called one by one from the host"""
    import torch
    B, n, m = sol.B, sol.nx, sol.nu
    _, ny, ns = load_package().sensor_dims(sens)
    xp, xh, Pc = _dev(sol, x0, xhat0, P0)
    ds = _dev(sol, est["s"])[0] if ns else None
    f64 = dict(dtype=torch.float64, device=xp.device)
    y, nis = torch.zeros(B, ny, **f64), torch.zeros(B, **f64)
    xo, uo = torch.zeros(B, k + 1, n, **f64), torch.zeros(B, k, m, **f64)
    torch.cuda.synchronize()
    sp, per = (ds.data_ptr() if ns else None), bool(ns) and est["s"].ndim == 2
    xs, us, ys, hs, dg, ns_ = [x0[:, None]], [], [], [], [], []
    upd = lambda: sol.estimate_update_sensor_device_(xh.data_ptr(), Pc.data_ptr(), y.data_ptr(), sens, est["r"], d_s_ptr=sp, per_instance_s=per,
                                                     iterations=est["iterations"], d_nis_ptr=nis.data_ptr())
    prd = lambda: sol.estimate_predict_device_(xh.data_ptr(), Pc.data_ptr(), steps=k, feedback=True, q=est["q"])
    msr = lambda step: sol.plant_measure_sensor_device_(sens, xp.data_ptr(), y.data_ptr(), d_s_ptr=sp, per_instance_s=per, step=step, sigma_y=est["sigma_y"], seed=seed)
    for p in range(periods):
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
        dg.append(np.diagonal(Pc.cpu().numpy(), axis1=1, axis2=2)[:, None].copy()); ns_.append(nis.cpu().numpy()[:, None])
    cat = lambda a: np.concatenate(a, axis=1)
    return dict(x=cat(xs), u=cat(us), y_cl=cat(ys), xhat=cat(hs), pdiag=cat(dg), nis=cat(ns_), P=Pc.cpu().numpy())


@pytest.mark.parametrize("key", ["encoder", "mix12"])
@pytest.mark.parametrize("delay,iterations", [(0, 1), (1, 2), (0, 2), (1, 1)])
def test_mpc_run_nlsensor_is_the_device_entry_points_one_by_one(pkg, key, delay, iterations):
    name, _, ny, ns, _ = N.SENSORS[key]
    sens = N.compiled(pkg, key)
    B, periods, k = 3, 3, 2
    a, b = _solved(pkg, name, B), _solved(pkg, name, B)
    n = a.nx
    x0 = R.plant_starts(a.get_trajectory()[0])
    xh0, _ = E.start(x0, n)
    P0 = E.p_start(B, n)
    est = dict(s=N.s_instances(key, B) if delay else N.s_shared(key), r=N.r(ny), q=E.q(n), sigma_y=N.sigma_y(ny), iterations=iterations)
    res = a.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, delay=delay, estimator=dict(sensor=sens, xhat0=xh0, P0=P0, **est))
    one = _device_stepped(b, x0, xh0, P0, periods, k, delay, sens, est, R.SEED)
    assert res.y_cl.shape == (B, periods, ny)
    for k_, val in one.items():
        assert np.array_equal(getattr(res, k_), val, equal_nan=True), (key, delay, iterations, k_)
    assert (res.log["iterations"] > 0).all() and (res.nis > 0.0).all()
    a.close(); b.close()


@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_no_sensor_is_mpc_run_io(pkg, name):
    import ctypes as C
    B, periods, k = 5, 2, 2
    a, b = _solved(pkg, name, B), _solved(pkg, name, B)
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
    pkg._ffi.check(L.ilqr_mpc_run_nlsensor(a._h, C.byref(d), C.byref(io), None, p(x0), None, None, None, None, p(x), p(u), p(log), nf.ctypes.data_as(I32),
                                           None, None, p(ycl), sat.ctypes.data_as(I32), None, None, None))
    assert np.array_equal(x, want.x) and np.array_equal(u, want.u) and np.array_equal(ycl, want.y_cl)
    assert np.array_equal(nf, want.first_nonfinite) and np.array_equal(sat, want.saturated)
    for col, f in enumerate(pkg._ffi.MPC_LOG_COLUMNS):
        assert np.array_equal(log[:, :, col], want.log[f].astype(np.float64), equal_nan=True), f
    with pytest.raises(ValueError, match="excludes"):
        a.mpc_run_(1, k, estimator=dict(sensor="x", H=np.eye(n), r=1.0, P0=E.p_start(B, n)))
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("delay", [0, 1])
def test_sharded_handle_equals_the_single_one(pkg, delay):
    key, B, periods, k = "beacons2", 7, 2, 2
    sens = N.compiled(pkg, key)
    one, two = _solved(pkg, "car_obs", B), _solved(pkg, "car_obs", B, devices=[0, 0])
    n, ny = one.nx, 2
    x0 = R.plant_starts(one.get_trajectory()[0])
    xh, Ps, ys = _inputs(one)
    for s in (N.s_shared(key), N.s_instances(key, B)):
        y = N.readings(key, ys, s)
        u1, u2 = (h.estimate_update_sensor_(xh, Ps, y, sens, N.r(ny), s=s, iterations=2) for h in (one, two))
        for k_ in u1:
            assert np.array_equal(u1[k_], u2[k_]), k_
        l1, l2 = (h.sensor_linearise_(sens, xh, s=s, x_prior=ys) for h in (one, two))
        m1, m2 = (h.plant_measure_sensor_(sens, x0, s=s, step=3, sigma_y=N.sigma_y(ny), seed=R.SEED, first_instance=11) for h in (one, two))
        assert np.array_equal(l1[0], l2[0]) and np.array_equal(l1[1], l2[1]) and np.array_equal(m1, m2)
        est = dict(sensor=sens, s=s, q=E.q(n), r=N.r(ny), sigma_y=N.sigma_y(ny), xhat0=xh, P0=Ps, iterations=2)
        r1, r2 = (h.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, first_instance=11, delay=delay, estimator=est) for h in (one, two))
        for k_ in ("x", "u", "y_cl", "saturated", "xhat", "pdiag", "nis", "P"):
            assert np.array_equal(getattr(r1, k_), getattr(r2, k_), equal_nan=True), k_
    for call in (lambda: two.sensor_linearise_device_(sens, 1, 1, 1, d_s_ptr=1), lambda: two.plant_measure_sensor_device_(sens, 1, 1, d_s_ptr=1),
                 lambda: two.estimate_update_sensor_device_(1, 1, 1, sens, N.r(ny), d_s_ptr=1)):
        with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
            call()
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 8
def test_it_filters(pkg):
    F = N.FILTER
    B, k = F["B"], F["k"]
    sens = N.compiled(pkg, F["key"])
    sol = pkg.Solver(model=F["name"], horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE))
    x1, ub, w = R.inputs(pkg.workloads, F["name"], B)
    sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)                # the fixed plan: the nominal actions, no feedback, no re-solve
    s, sy, rr, qq, xh0, P0 = N.filter_inputs(x1)
    scores = {}
    for it in (1, 3):
        x, xh, Pc, xo = x1.copy(), xh0.copy(), P0.copy(), xh0.copy()
        xs, hs, os_ = [], [], []
        for p in range(F["periods"]):
            x = sol.plant_step_(x, steps=k)["x"][:, -1]
            y = sol.plant_measure_sensor_(sens, x, s=s, step=(p + 1) * k, sigma_y=sy, seed=F["seed"])
            xh, Pc = sol.estimate_predict_(xh, Pc, steps=k, q=qq)
            out = sol.estimate_update_sensor_(xh, Pc, y, sens, rr, s=s, iterations=it)
            xh, Pc = out["xhat"], out["P"]
            xo = sol.plant_step_(xo, steps=k)["x"][:, -1]
            xs.append(x); hs.append(xh); os_.append(xo)
        scores[it] = N.filter_scores({key: np.stack(v, axis=1) for key, v in (("x", xs), ("xhat", hs), ("open", os_))})
    (e1, open_), (e3, _) = scores[1], scores[3]
    print("filter on the device: position mse %.3e with one iteration, %.3e with three, prediction alone %.3e" % (e1, e3, open_))
    assert e1 < open_ and e3 < open_ and e3 <= e1
    sol.close()
