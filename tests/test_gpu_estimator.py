"""ilqr_estimate_predict, ilqr_estimate_update and ilqr_mpc_run_est on the GPU. T = 11, built-in models car_obs (3 x 2, user
parameters), acrobot (4 x 1), synth12 (large form) and synth32 (32 x 8); B = 3 and 70 (synth32: 3), handles solved as in
tests/test_gpu_plant_io.py. Inputs, masks, q, r and P0: tests/estimator_ref.py; the bound TOL_XU = 1e-10 relative to
max(1, max |reference|) is the project's own (tests/test_estimator_ref.py: the yardstick's two forms agree within a tenth of it).

1. Predict and update against the yardstick: every model, both masks, feedback on and off, with and without limits, k in {1, 3};
   P out is bit for bit symmetric.
2. Predict's estimate is plant_step_'s state bit for bit (same flag and limits, no noise).
3. An instance's bits are the same at B = 3 and inside B = 70, and through the host and device forms.
4. NaN in the unmeasured components of y changes nothing; a measured component without process noise has a smaller variance after.
5. A NaN in one instance's P_jj: first_bad == j there, every other instance bit for bit.
6. mpc_run_(estimator=...) is, bit for bit, the device entry points called one by one (delay 0 and 1; acrobot and synth12), and its
   xhat and pdiag are the yardstick loop's within TOL_XU when that loop is fed the device's own plans.
7. estimator=None is mpc_run_ bit for bit.
8. A sharded handle [0, 0] equals the single one, also with every input and output array of the loop passed at once.
9. It filters: acrobot, positions measured — the estimate beats the measurement on the positions and prediction alone on the
   velocities (the conditions tests/test_estimator_ref.py shows on the yardstick with a factor of two to spare)."""
import numpy as np
import pytest

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU = 1e-10
T = R.T


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_estimate_predict", "ilqr_estimate_predict_device", "ilqr_estimate_update", "ilqr_estimate_update_device", "ilqr_mpc_run_est"):
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


def _plan(sol, w):
    (xb, ub), (K, _) = sol.get_trajectory(), sol.get_policy()
    return xb, ub, K, w


def _inputs(sol):
    xb = sol.get_trajectory()[0]
    xh, y = E.start(R.plant_starts(xb), sol.nx)
    return xh, E.p_start(sol.B, sol.nx), y


# ----------------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("name", E.MODELS)
def test_predict_and_update_against_the_yardstick(pkg, name):
    u_min, u_max = IO.LIMITS[name]
    worst = 0.0
    for B in R.BATCHES[name]:
        sol, w = _solved(pkg, name, B)
        xb, ub, K, _ = _plan(sol, w)
        n = sol.nx
        xh, Ps, y = _inputs(sol)
        part, full = E.masks(name, n)
        for k, fb, lim, mask in [(1, 1, 1, part), (3, 0, 0, full), (3, 1, 1, full), (3, 1, 0, part), (1, 0, 1, full)]:
            lims = dict(u_min=u_min, u_max=u_max) if lim else {}
            x1, P1 = sol.estimate_predict_(xh, Ps, steps=k, feedback=bool(fb), q=E.q(n), **lims)
            step = sol.plant_step_(xh, steps=k, feedback=bool(fb), **lims)
            assert np.array_equal(x1, step["x"][:, -1]), (name, B, k, fb, lim)                      # 2: the plant step's bits
            out = sol.estimate_update_(x1, P1, y, E.r(n), measured=mask)
            assert np.array_equal(P1, P1.transpose(0, 2, 1)) and np.array_equal(out["P"], out["P"].transpose(0, 2, 1))
            assert (out["first_bad"] == -1).all()
            for b in (range(B) if B <= 3 else (0, 1, 63, 64, 69)):
                rx, rP = E.predict(name, xb[b], ub[b], K[b], None if w is None else w[b], xh[b], Ps[b], k, bool(fb), q=E.q(n),
                                   **({k_: v for k_, v in lims.items()}))
                ref = E.update_sequential(rx, rP, y[b], E.r(n), mask)
                errs = [P.rel(x1[b], rx), P.rel(P1[b], rP), P.rel(out["xhat"][b], ref["xhat"]), P.rel(out["P"][b], ref["P"]),
                        P.rel(out["innovation"][b], ref["innovation"]), abs(out["nis"][b] - ref["nis"]) / max(1.0, abs(ref["nis"]))]
                worst = max(worst, max(errs))
                print("estimator %s B=%d k=%d fb=%d lim=%d b=%d: %s" % (name, B, k, fb, lim, b, " ".join("%.2e" % e for e in errs)))
                assert max(errs) < TOL_XU, (name, B, k, fb, lim, b, errs)
        sol.close()
    print("estimator %s: worst relative error %.2e" % (name, worst))


# ----------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["car_obs", "acrobot", "synth12"])
def test_an_instance_does_not_depend_on_its_batch_or_on_the_form(pkg, name):
    import torch
    big, w = _solved(pkg, name, 70)
    small, _ = _solved(pkg, name, 3)
    n = big.nx
    for b in range(3):                             # the two handles hold the same plans for the first three instances
        assert np.array_equal(big.get_trajectory()[1][b], small.get_trajectory()[1][b])
    xh, Ps, y = _inputs(big)
    mask = E.masks(name, n)[0]
    u_min, u_max = IO.LIMITS[name]
    kw = dict(steps=3, feedback=True, q=E.q(n), u_min=u_min, u_max=u_max)
    x70, P70 = big.estimate_predict_(xh, Ps, **kw)
    x3, P3 = small.estimate_predict_(xh[:3], Ps[:3], **kw)
    assert np.array_equal(x70[:3], x3) and np.array_equal(P70[:3], P3)
    o70, o3 = big.estimate_update_(x70, P70, y, E.r(n), measured=mask), small.estimate_update_(x3, P3, y[:3], E.r(n), measured=mask)
    for key in o3:
        assert np.array_equal(o70[key][:3], o3[key]), key
    # the device forms, on the caller's device arrays
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(big.stream_ptr())):
        dx, dP, dy = (torch.from_numpy(a.copy()).to(dev) for a in (xh, Ps, y))
        dinn, dnis = torch.zeros(70, n, dtype=torch.float64, device=dev), torch.zeros(70, dtype=torch.float64, device=dev)
        dbad = torch.zeros(70, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    big.estimate_predict_device_(dx.data_ptr(), dP.data_ptr(), **kw)
    big.synchronize()
    assert np.array_equal(dx.cpu().numpy(), x70) and np.array_equal(dP.cpu().numpy(), P70)
    big.estimate_update_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), E.r(n), measured=mask, d_innovation_ptr=dinn.data_ptr(),
                                d_nis_ptr=dnis.data_ptr(), d_first_bad_ptr=dbad.data_ptr())
    big.synchronize()
    for key, t in (("xhat", dx), ("P", dP), ("innovation", dinn), ("nis", dnis), ("first_bad", dbad)):
        assert np.array_equal(t.cpu().numpy(), o70[key]), key
    big.close(); small.close()


# ----------------------------------------------------------------------------------------------------------------------- 4, 5
@pytest.mark.parametrize("name,B", [("car_obs", 70), ("acrobot", 3), ("synth12", 3), ("synth32", 3)])
def test_unmeasured_components_and_a_skipped_update(pkg, name, B):
    sol, w = _solved(pkg, name, B)
    n = sol.nx
    xh, Ps, y = _inputs(sol)
    mask = E.masks(name, n)[0]
    x1, P1 = sol.estimate_predict_(xh, Ps, steps=1, q=E.q(n))
    clean = sol.estimate_update_(x1, P1, y, E.r(n), measured=mask)
    yn = y.copy(); yn[:, mask == 0] = np.nan
    out = sol.estimate_update_(x1, P1, yn, E.r(n), measured=mask)
    for key in clean:
        assert np.array_equal(out[key], clean[key]), key
    assert np.isfinite(out["xhat"]).all() and (out["innovation"][:, mask == 0] == 0.0).all()
    assert mask[0] == 1 and E.q(n)[0] == 0.0 and (clean["P"][:, 0, 0] < P1[:, 0, 0]).all()
    # 5: a NaN pivot in one instance
    bad_b, j = B - 2, 1
    Pn = P1.copy(); Pn[bad_b, j, j] = np.nan
    out = sol.estimate_update_(x1, Pn, y, E.r(n), measured=mask)
    assert out["first_bad"][bad_b] == j and out["innovation"][bad_b, j] == 0.0
    others = np.arange(B) != bad_b
    assert (out["first_bad"][others] == -1).all()
    for key in clean:
        assert np.array_equal(out[key][others], clean[key][others]), key
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
def _device_stepped(sol, x0, xhat0, P0, periods, k, delay, sigma_y, est, seed):
    """ilqr_mpc_run_est's definition: the device entry points called one by one from the host"""
    import torch
    B, n, m = sol.B, sol.nx, sol.nu
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
        xp, xh, Pc = (torch.from_numpy(a.copy()).to(dev) for a in (x0, xhat0, P0))
        y, nis = torch.zeros(B, n, **f64), torch.zeros(B, **f64)
        xo, uo = torch.zeros(B, k + 1, n, **f64), torch.zeros(B, k, m, **f64)
    torch.cuda.synchronize()
    xs, us, ys, hs, ds, ns, plans = [x0[:, None]], [], [], [], [], [], []
    upd = lambda: sol.estimate_update_device_(xh.data_ptr(), Pc.data_ptr(), y.data_ptr(), est["r"], measured=est["measured"], d_nis_ptr=nis.data_ptr())
    prd = lambda: sol.estimate_predict_device_(xh.data_ptr(), Pc.data_ptr(), steps=k, feedback=True, q=est["q"])
    for p in range(periods):
        plans.append(_plan(sol, None)[:3])
        if delay:
            sol.plant_measure_device_(xp.data_ptr(), y.data_ptr(), step=p * k, sigma_y=sigma_y, seed=seed)
            upd(); prd()
        sol.plant_step_device_(xp.data_ptr(), steps=k, feedback=True, seed=seed, step0=p * k, d_x_out_ptr=xo.data_ptr(), d_u_out_ptr=uo.data_ptr())
        if not delay:
            sol.plant_measure_device_(xp.data_ptr(), y.data_ptr(), step=(p + 1) * k, sigma_y=sigma_y, seed=seed)
            prd(); upd()
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
def test_mpc_run_est_is_the_device_entry_points_one_by_one(pkg, name, delay):
    B, periods, k = 3, 3, 2
    a, w = _solved(pkg, name, B)
    b, _ = _solved(pkg, name, B)
    n = a.nx
    x0 = R.plant_starts(a.get_trajectory()[0])
    xh0, _ = E.start(x0, n)
    P0 = E.p_start(B, n)
    est = dict(measured=E.masks(name, n)[0], q=E.q(n), r=E.r(n))
    sy = IO.sigma_y(n)
    res = a.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, sigma_y=sy, delay=delay, estimator=dict(xhat0=xh0, P0=P0, **est))
    one, plans = _device_stepped(b, x0, xh0, P0, periods, k, delay, sy, est, R.SEED)
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
                    lambda x, step: IO.measure(x, sy, z[i], step),
                    lambda xh, Pc, p: E.predict(name, *plan(p), None, xh, Pc, k, True, q=est["q"]),
                    lambda xh, Pc, y: E.update_sequential(xh, Pc, y, est["r"], est["measured"]),
                    lambda xc, p: None)
        ex, ed = P.rel(res.xhat[i], ref["xhat"]), P.rel(res.pdiag[i], ref["pdiag"])
        print("loop %s delay %d instance %d: xhat %.2e pdiag %.2e" % (name, delay, i, ex, ed))
        assert ex < TOL_XU and ed < TOL_XU, (name, delay, i, ex, ed)
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 7, 8
@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_no_estimator_is_mpc_run(pkg, name):
    import ctypes as C
    B, periods, k = 5, 2, 2
    a, w = _solved(pkg, name, B)
    b, _ = _solved(pkg, name, B)
    x0 = R.plant_starts(a.get_trajectory()[0])
    u_min, u_max = IO.LIMITS[name]
    sy = IO.sigma_y(a.nx)
    want = b.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, sigma_y=sy, delay=1, u_min=u_min, u_max=u_max)
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    p = lambda arr: None if arr is None else arr.ctypes.data_as(F64)
    d = pkg._ffi.MpcDesc(periods, k, 1, 0, 0, 1, 0, 0, R.SEED, 0, None)
    io = pkg._ffi.PlantIO(p(u_min), p(u_max), p(sy), 1, 0)
    Rr = periods * k
    x, u, log = np.empty((B, Rr + 1, a.nx)), np.empty((B, Rr, a.nu)), np.empty((B, periods, 9))
    nf, sat, ycl = np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32), np.empty((B, periods, a.nx))
    pkg._ffi.check(L.ilqr_set_options(a._h, C.byref(a.options)))
    pkg._ffi.check(L.ilqr_mpc_run_est(a._h, C.byref(d), C.byref(io), None, p(x0), None, None, None, None, p(x), p(u), p(log), nf.ctypes.data_as(I32),
                                      None, None, p(ycl), sat.ctypes.data_as(I32), None, None, None))
    assert np.array_equal(x, want.x) and np.array_equal(u, want.u) and np.array_equal(ycl, want.y_cl)
    assert np.array_equal(nf, want.first_nonfinite) and np.array_equal(sat, want.saturated)
    for c, f in enumerate(pkg._ffi.MPC_LOG_COLUMNS):
        assert np.array_equal(log[:, :, c], want.log[f].astype(np.float64), equal_nan=True), f
    a.close(); b.close()


@pytest.mark.parametrize("delay", [0, 1])
def test_sharded_handle_equals_the_single_one(pkg, delay):
    B, periods, k = 7, 2, 2
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    n = one.nx
    x0 = R.plant_starts(one.get_trajectory()[0])
    xh, Ps, y = _inputs(one)
    mask = E.masks("car_obs", n)[0]
    p1, p2 = (s.estimate_predict_(xh, Ps, steps=3, feedback=True, q=E.q(n)) for s in (one, two))
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])
    u1, u2 = (s.estimate_update_(p1[0], p1[1], y, E.r(n), measured=mask) for s in (one, two))
    for key in u1:
        assert np.array_equal(u1[key], u2[key]), key
    est = dict(measured=mask, q=E.q(n), r=E.r(n), xhat0=xh, P0=Ps)
    r1, r2 = (s.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=R.SEED, first_instance=11, sigma_y=IO.sigma_y(n), delay=delay, estimator=est)
              for s in (one, two))
    for key in ("x", "u", "y_cl", "saturated", "xhat", "pdiag", "nis", "P"):
        assert np.array_equal(getattr(r1, key), getattr(r2, key), equal_nan=True), key
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        two.estimate_predict_device_(1, 1)
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        two.estimate_update_device_(1, 1, 1, E.r(n))
    one.close(); two.close()


def test_sharded_loop_with_every_array_equals_the_single_one(pkg):
    """every input and output array of ilqr_mpc_run_est at once: each is sliced per shard (B = 7: shards of 4 and 3)"""
    B, periods, k = 7, 2, 2
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    n = one.nx
    x0 = R.plant_starts(one.get_trajectory()[0])
    xh, Ps, _ = _inputs(one)
    u_min, u_max = IO.LIMITS["car_obs"]
    wp = R.plant_parameters(w, periods * k)
    est = dict(measured=E.masks("car_obs", n)[0], q=E.q(n), r=E.r(n), xhat0=xh, P0=Ps)
    r1, r2 = (s.mpc_run_(periods, k, x0=x0, plant_feedback=True, sigma_x=R.sigma_x(n), seed=R.SEED, first_instance=11, w_plant=wp,
                         w_preview=np.ascontiguousarray(wp[:, ::-1]), score=True, u_min=u_min, u_max=u_max, sigma_y=IO.sigma_y(n), estimator=est)
              for s in (one, two))
    for key in ("x", "u", "first_nonfinite", "cl_cost", "cl_violation", "y_cl", "saturated", "xhat", "pdiag", "nis", "P"):
        assert np.array_equal(getattr(r1, key), getattr(r2, key), equal_nan=True), key
    for f in r1.log:
        assert np.array_equal(r1.log[f], r2.log[f], equal_nan=True), f
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 9
def test_it_filters(pkg):
    F = E.FILTER
    B, k = F["B"], F["k"]
    sol = pkg.Solver(model=F["name"], horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE))
    x1, ub, _ = R.inputs(pkg.workloads, F["name"], B)
    sol.initialize_rollout_(x1, ub)                # the fixed plan: the nominal actions, no feedback, no re-solve
    sy, rr, qq, mk, xh, Pc = E.filter_inputs(x1)
    x, xo = x1.copy(), xh.copy()
    xs, ys, hs, os_ = [], [], [], []
    for p in range(F["periods"]):
        x = sol.plant_step_(x, steps=k)["x"][:, -1]
        y = sol.plant_measure_(x, step=(p + 1) * k, sigma_y=sy, seed=F["seed"])
        xh, Pc = sol.estimate_predict_(xh, Pc, steps=k, q=qq)
        out = sol.estimate_update_(xh, Pc, y, rr, measured=mk)
        xh, Pc = out["xhat"], out["P"]
        xo = sol.plant_step_(xo, steps=k)["x"][:, -1]
        xs.append(x); ys.append(y); hs.append(xh); os_.append(xo)
    run = {key: np.stack(v, axis=1) for key, v in (("x", xs), ("y", ys), ("xhat", hs), ("open", os_))}
    pos_hat, pos_y, vel_hat, vel_open = E.filter_scores(run)
    print("filter on the device: positions %.3e (measurement %.3e), velocities %.3e (prediction alone %.3e)" % (pos_hat, pos_y, vel_hat, vel_open))
    assert pos_hat < pos_y and vel_hat < vel_open
    sol.close()
