"""The compiled nonlinear sensor — sensor_linearise_kernel<S, JAC> behind ilqr_sensor_linearise, ilqr_plant_measure_sensor,
ilqr_estimate_update_sensor and ilqr_mpc_run_nlsensor — at the model sizes and over the function families its own test
(tests/test_gpu_sensor_nl.py: nx in {3, 4, 12, 32}, ns <= 4, sin, cos, tanh, sqrt) never ran. The tables, their inputs and their
yardsticks are tests/sensor_nl_sizes.py's: seven sensors on the synth family of the MPC sweep (tests/test_gpu_mpc_sweep.py's modules
under their registered names) from a (1, 1) grid to ny = ns = nx = 64, held to the complex-step yardstick of tests/sensor_nl_ref.py,
and family3 on car_obs (atan2, exp, log, Abs, pow, Piecewise, Max, asin, sinh, atan, rationals, a constant row), held to mpmath at
50 digits. T = 21; B = 70 for linearise, measure and update (the handle is created, not solved: none of them reads a policy), B = 3
with a brief solve for the loop. Compiled through api.compile_sensor, served from the module cache the build leaves.

1. Linearise (with and without x_prior) and measure (with and without sigma_y, first_instance 5) against the yardstick within
   TOL_F = 1e-12 on instances 0, 1, 63, 64, 69 (family3: also 2 .. 7, the hand-placed bearings); sigma_y None: the measurement is ŷ bit
   for bit; the noise is sigma_y · z to the rounding of one add; H at structurally zero entries is exactly 0.0 in an array that
   held NaN (the device form).
2. estimate_update_sensor_(iterations=1) is sensor_linearise_device_ + estimate_update_linear_device_(per_instance_H, yhat) bit for
   bit; the host form is the device form at 1 and 3 iterations; P out is symmetric.
3. 1 and 3 iterations against the yardstick's update within TOL_XU = 1e-10.
4. An instance's bits at B = 70 are those in a B = 3 handle (one1, mix33, wide64); a per-instance s with equal rows gives the bits
   of the shared one (fan1, wide64).
5. A NaN in one instance's x̂ (fan1; wide64: in x_33, which no row below 32 reads, so first_bad = 32 lies in mask word 1): the
   yardstick's first_bad there, every other instance bit for bit the clean run.
6. mpc_run_(estimator=dict(sensor=...)) at (5, 1), (33, 2) and (64, 8) — the predict launch above 64 KiB of LDS and the growth of
   the H buffer inside the one enqueue — is test_gpu_sensor_nl._device_stepped bit for bit; nis > 0 throughout.

The bounds are the project's own and were decided on the yardstick alone (tests/test_sensor_nl_sizes_ref.py asserts it): with x̂
and s moved by one part in 1e15 the references move by

    key       H        ŷ, y     ŷ(prior) | x̂        P        innovation  nis
    one1      1.1e-15  6.7e-16  7.6e-17  | 4.3e-16  1.4e-17  7.8e-16     3.0e-15
    fan1      1.0e-15  1.2e-15  6.0e-16  | 1.1e-15  1.9e-19  2.0e-15     1.4e-14
    mix5      1.2e-15  1.8e-15  7.8e-16  | 1.1e-15  6.2e-17  2.2e-15     7.3e-15
    mix17     1.2e-15  2.3e-15  3.8e-16  | 6.7e-16  1.9e-17  3.1e-15     2.0e-14
    mix33     2.3e-15  2.7e-15  8.9e-16  | 1.1e-15  4.5e-17  2.4e-15     1.7e-14
    one64     8.9e-16  5.6e-16  3.3e-16  | 1.4e-15  2.1e-17  6.1e-16     9.4e-16
    wide64    1.4e-15  2.4e-15  1.1e-15  | 1.2e-15  5.2e-17  3.6e-15     1.4e-14
    family3   6.4e-15  4.7e-15  1.0e-15  | 1.9e-15  5.2e-17  1.4e-14     7.7e-14

relative to max(1, max |reference|): ten times that is below TOL_F on the left and TOL_XU on the right at every entry.

Measured on the MI355X (worst relative error per entry, over shared and per-instance s and the instances compared; the tests print
them):

    key       linearise and measure (bound 1e-12)   update, 1 and 3 iterations (bound 1e-10)
    one1      2.2e-16                               4.3e-16
    fan1      4.4e-16                               7.4e-15
    mix5      1.9e-16                               1.4e-15
    mix17     1.1e-16                               2.7e-15
    mix33     1.1e-16                               5.7e-15
    one64     2.2e-16                               4.5e-16
    wide64    4.4e-16                               4.3e-15
    family3   3.9e-16                               3.0e-14"""
import numpy as np
import pytest

import estimator_ref as E
import mpc_ref as M
import plant_io_ref as IO
import plant_ref as PR
import policy_ref as P
import sensor_nl_ref as N
import sensor_nl_sizes as Z
import test_gpu_mpc_sweep as SW
import test_gpu_sensor_nl as GS
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_F = 1e-12
TOL_XU = 1e-10
T = M.T_SWEEP
SEED = PR.SEED
B = Z.B


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    return p


def _handle(pkg, key, batch, solve=False):
    """a handle the sensor runs on: the sweep's module of that size (traced once per size and process, together with the sweep and
    the closed-loop sizes: their table of registered names), car_obs for the family; solved briefly where a policy is needed"""
    where = N.entry(key)[0]
    opts = pkg.Options(verbose=0, **PR.SOLVE)
    if isinstance(where, str):
        sol = pkg.Solver(model=where, horizon=T, batch=batch, options=opts)
    elif where in SW._MODELS:
        sol = pkg.Solver(model=SW._MODELS[where], horizon=T, batch=batch, options=opts)
    else:
        mdl = pkg.models.synth_nm(*where)
        sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                         [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=batch, options=opts, name=M.module_name(*where))
        SW._MODELS[where] = sol.model
    assert (sol.nx, sol.B) == (N.dims(key)[0], batch)
    if solve:
        x1, ub = M.sweep_inputs(sol.nx, sol.nu, batch, T)
        sol.initialize_rollout_(x1, ub)
        sol.solve_()
        assert np.isfinite(sol.get_policy()[0]).all()
    return sol


def _forms(key):
    """s shared, s per instance (one form where the sensor has no parameters)"""
    return (Z.s_shared(key), Z.s_instances(key, B)) if N.dims(key)[2] else (Z.s_shared(key),)


_ZERO = {}


def _structural_zeros(pkg, key):
    if key not in _ZERO:
        nx, _, ns = N.dims(key)
        _ZERO[key] = np.array([[d == 0 for d in row] for row in pkg.codegen.sensor_expressions(N.symbolic(key), nx, ns)[3]])
    return _ZERO[key]


_sb = GS._sb
_dev = GS._dev


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("key", Z.KEYS)
def test_linearise_and_measure_over_the_sizes_and_the_family(pkg, key):
    import torch
    nx, ny, ns = N.dims(key)
    sens = N.compiled(pkg, key)
    sol = _handle(pkg, key, B)
    xh, _, xp, _ = Z.inputs(key)
    step, first = 7, 5
    z = pkg.candidate_noise(SEED, first + B, *IO.measure_shape(step))[first:]
    sy = N.sigma_y(ny)
    loud = sy != 0.0
    zero = _structural_zeros(pkg, key)
    worst = 0.0
    for s in _forms(key):
        H, yhat = sol.sensor_linearise_(sens, xh, s=s)
        Hp, yp = sol.sensor_linearise_(sens, xh, s=s, x_prior=xp)
        y0 = sol.plant_measure_sensor_(sens, xh, s=s, step=step)
        y = sol.plant_measure_sensor_(sens, xh, s=s, step=step, sigma_y=sy, seed=SEED, first_instance=first)
        assert np.array_equal(y0, yhat) and np.array_equal(Hp, H) and not np.array_equal(yp, yhat)
        assert np.array_equal(y[:, ~loud], y0[:, ~loud]) and (not loud.any() or (y[:, loud] != y0[:, loud]).all())
        assert (H[:, zero] == 0.0).all() and np.isfinite(H).all()
        # the device form into arrays that hold NaN: the kernel's zero fill is the only writer of a structurally zero entry
        dx, dxp = _dev(sol, xh, xp)
        ds = _dev(sol, s)[0] if ns else None
        dH = torch.full((B, ny, nx), float("nan"), dtype=torch.float64, device=dx.device)
        dyh = torch.full((B, ny), float("nan"), dtype=torch.float64, device=dx.device)
        torch.cuda.synchronize()
        sol.sensor_linearise_device_(sens, dx.data_ptr(), dH.data_ptr(), dyh.data_ptr(), d_s_ptr=ds.data_ptr() if ns else None, per_instance_s=s.ndim == 2,
                                     d_x_prior_ptr=dxp.data_ptr())
        sol.synchronize()
        Hd = dH.cpu().numpy()
        assert (Hd[:, zero] == 0.0).all() and np.array_equal(Hd, H) and np.array_equal(dyh.cpu().numpy(), yp), (key, s.ndim)
        for b in Z.some(key, B):
            Hr, yr = N.linearise(key, xh[b], _sb(s, b))
            ypr = N.linearise(key, xh[b], _sb(s, b), xp[b])[1]
            errs = [P.rel(H[b], Hr), P.rel(yhat[b], yr), P.rel(yp[b], ypr), P.rel(y[b], N.measure(key, xh[b], _sb(s, b), sy, z[b], step))]
            worst = max(worst, max(errs))
            print("sensor %s s%dd b=%d: H %.2e yhat %.2e yhat(prior) %.2e y %.2e" % ((key, s.ndim, b) + tuple(errs)))
            assert max(errs) < TOL_F, (key, s.ndim, b, errs)
            # the noise is sigma_y · z to the rounding of one add (one ulp of the larger of y and h(x)); z itself is the host twin's
            # within a few ulp (ilqr_device_sample.hpp: libm's log and cos against the device's), taken as 1e-14 of the noise
            noise = np.array([sy[j] * z[b][IO.MEASURE_ROW0 + j // 16, step, j % 16] for j in range(ny)])
            assert (np.abs((y[b] - y0[b]) - noise) <= 2.0 ** -52 * np.maximum(np.abs(y[b]), np.abs(y0[b])) + 1e-14 * np.abs(noise)).all(), (key, b)
    print("sensor sizes %s: linearise and measure, worst relative error %.2e (bound %.1e)" % (key, worst, TOL_F))
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 2, 3
@pytest.mark.parametrize("key", Z.KEYS)
def test_update_is_the_composition_and_the_yardsticks_over_the_sizes(pkg, key):
    import torch
    nx, ny, ns = N.dims(key)
    sens = N.compiled(pkg, key)
    sol = _handle(pkg, key, B)
    xh, Ps, _, ys = Z.inputs(key)
    rr = N.r(ny)
    worst = 0.0
    for s in _forms(key):
        y = Z.readings(key, ys, s)
        one = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s)
        three = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=3)
        for out in (one, three):
            assert np.array_equal(out["P"], out["P"].transpose(0, 2, 1)) and (out["first_bad"] == -1).all(), (key, s.ndim)
        # the two existing device calls in sequence
        dx, dP, dy = _dev(sol, xh, Ps, y)
        ds = _dev(sol, s)[0] if ns else None
        f64 = dict(dtype=torch.float64, device=dx.device)
        dH, dyh, dinn, dnis = torch.zeros(B, ny, nx, **f64), torch.zeros(B, ny, **f64), torch.zeros(B, ny, **f64), torch.zeros(B, **f64)
        dbad = torch.zeros(B, dtype=torch.int32, device=dx.device)
        torch.cuda.synchronize()
        sp, per = (ds.data_ptr() if ns else None), s.ndim == 2
        sol.sensor_linearise_device_(sens, dx.data_ptr(), dH.data_ptr(), dyh.data_ptr(), d_s_ptr=sp, per_instance_s=per)
        sol.estimate_update_linear_device_(dx.data_ptr(), dP.data_ptr(), dy.data_ptr(), dH.data_ptr(), ny, rr, per_instance_H=True, d_yhat_ptr=dyh.data_ptr(),
                                           d_innovation_ptr=dinn.data_ptr(), d_nis_ptr=dnis.data_ptr(), d_first_bad_ptr=dbad.data_ptr())
        sol.synchronize()
        for k, t in (("xhat", dx), ("P", dP), ("innovation", dinn), ("nis", dnis), ("first_bad", dbad)):
            assert np.array_equal(t.cpu().numpy(), one[k]), (key, s.ndim, k)
        # the device form of the composite call
        for it, out in ((1, one), (3, three)):
            dx2, dP2 = _dev(sol, xh, Ps)
            dinn2, dnis2 = torch.zeros(B, ny, **f64), torch.zeros(B, **f64)
            torch.cuda.synchronize()
            sol.estimate_update_sensor_device_(dx2.data_ptr(), dP2.data_ptr(), dy.data_ptr(), sens, rr, d_s_ptr=sp, per_instance_s=per, iterations=it,
                                               d_innovation_ptr=dinn2.data_ptr(), d_nis_ptr=dnis2.data_ptr())
            sol.synchronize()
            for k, t in (("xhat", dx2), ("P", dP2), ("innovation", dinn2), ("nis", dnis2)):
                assert np.array_equal(t.cpu().numpy(), out[k]), (key, s.ndim, it, k)
            for b in Z.some(key, B):
                ref = N.update(key, xh[b], Ps[b], y[b], _sb(s, b), rr, it)
                errs = [P.rel(out["xhat"][b], ref["xhat"]), P.rel(out["P"][b], ref["P"]), P.rel(out["innovation"][b], ref["innovation"]),
                        abs(out["nis"][b] - ref["nis"]) / max(1.0, abs(ref["nis"]))]
                worst = max(worst, max(errs))
                print("update %s s%dd iterations=%d b=%d: %s" % (key, s.ndim, it, b, " ".join("%.2e" % e for e in errs)))
                assert ref["first_bad"] == -1 and max(errs) < TOL_XU, (key, s.ndim, it, b, errs)
    print("sensor sizes %s: update, worst relative error %.2e (bound %.1e)" % (key, worst, TOL_XU))
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("key", ["one1", "fan1", "mix33", "wide64"])
def test_an_instance_does_not_depend_on_its_batch_over_the_sizes(pkg, key):
    nx, ny, ns = N.dims(key)
    sens = N.compiled(pkg, key)
    big = _handle(pkg, key, B)
    xh, Ps, xp, ys = Z.inputs(key)
    s, rr, sy = Z.s_instances(key, B), N.r(ny), N.sigma_y(ny)
    y = Z.readings(key, ys, s)
    if key != "fan1":                              # B = 70 against a B = 3 handle of the same size
        small = _handle(pkg, key, 3)
        for it in (1, 2):
            o70, o3 = big.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=it), small.estimate_update_sensor_(xh[:3], Ps[:3], y[:3], sens, rr, s=s[:3], iterations=it)
            for k in o3:
                assert np.array_equal(o70[k][:3], o3[k]), (key, it, k)
        H70, yh70 = big.sensor_linearise_(sens, xh, s=s, x_prior=xp)
        H3, yh3 = small.sensor_linearise_(sens, xh[:3], s=s[:3], x_prior=xp[:3])
        assert np.array_equal(H70[:3], H3) and np.array_equal(yh70[:3], yh3)
        assert np.array_equal(big.plant_measure_sensor_(sens, xh, s=s, step=3, sigma_y=sy, seed=SEED)[:3],
                              small.plant_measure_sensor_(sens, xh[:3], s=s[:3], step=3, sigma_y=sy, seed=SEED))
        small.close()
    if key in ("fan1", "wide64"):                  # a shared s and a per-instance s whose rows are all equal
        sh = Z.s_shared(key)
        rows = np.ascontiguousarray(np.broadcast_to(sh, (B, ns)))
        a, c = big.estimate_update_sensor_(xh, Ps, y, sens, rr, s=sh, iterations=2), big.estimate_update_sensor_(xh, Ps, y, sens, rr, s=rows, iterations=2)
        for k in a:
            assert np.array_equal(a[k], c[k]), (key, k)
        la, lc = big.sensor_linearise_(sens, xh, s=sh, x_prior=xp), big.sensor_linearise_(sens, xh, s=rows, x_prior=xp)
        assert np.array_equal(la[0], lc[0]) and np.array_equal(la[1], lc[1])
        assert np.array_equal(big.plant_measure_sensor_(sens, xh, s=sh, step=3, sigma_y=sy, seed=SEED), big.plant_measure_sensor_(sens, xh, s=rows, step=3, sigma_y=sy, seed=SEED))
    big.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("key,component,first_bad", [("fan1", 0, 0), ("wide64", Z.WIDE64_LATE, 32)])
def test_a_bad_instance_stays_alone_at_the_edge_sizes(pkg, key, component, first_bad):
    """a NaN in one instance's x̂: an input the update is built to contain"""
    nx, ny, ns = N.dims(key)
    sens = N.compiled(pkg, key)
    sol = _handle(pkg, key, B)
    xh, Ps, _, ys = Z.inputs(key)
    s, rr = Z.s_instances(key, B), N.r(ny)
    y = Z.readings(key, ys, s)
    bad_b = B - 2
    others = np.arange(B) != bad_b
    xn = xh.copy(); xn[bad_b, component] = np.nan
    for it in (1, 2):
        clean = sol.estimate_update_sensor_(xh, Ps, y, sens, rr, s=s, iterations=it)
        out = sol.estimate_update_sensor_(xn, Ps, y, sens, rr, s=s, iterations=it)
        ref = N.update(key, xn[bad_b], Ps[bad_b], y[bad_b], s[bad_b], rr, it)
        # (the second iteration linearises at the first one's estimate, by then NaN throughout: every row is bad, the first is 0)
        assert ref["first_bad"] == (first_bad if it == 1 else 0) and out["first_bad"][bad_b] == ref["first_bad"], (key, it, out["first_bad"][bad_b], ref["first_bad"])
        assert (out["first_bad"][others] == -1).all()
        for k in clean:
            assert np.array_equal(out[k][others], clean[k][others]), (key, it, k)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("key", ["mix5", "mix33", "wide64"])
@pytest.mark.parametrize("delay,iterations", [(0, 1), (1, 2)])
def test_mpc_run_nlsensor_over_the_sizes(pkg, key, delay, iterations):
    nx, ny, ns = N.dims(key)
    sens = N.compiled(pkg, key)
    batch, periods, k = 3, 2, 2
    a, b = _handle(pkg, key, batch, solve=True), _handle(pkg, key, batch, solve=True)
    x0 = PR.plant_starts(a.get_trajectory()[0])
    xh0, _ = E.start(x0, nx)
    P0 = E.p_start(batch, nx)
    est = dict(s=Z.s_instances(key, batch) if delay else Z.s_shared(key), r=N.r(ny), q=E.q(nx), sigma_y=N.sigma_y(ny), iterations=iterations)
    res = a.mpc_run_(periods, k, x0=x0, plant_feedback=True, seed=SEED, delay=delay, estimator=dict(sensor=sens, xhat0=xh0, P0=P0, **est))
    one = GS._device_stepped(b, x0, xh0, P0, periods, k, delay, sens, est, SEED)
    assert res.y_cl.shape == (batch, periods, ny)
    for k_, val in one.items():
        assert np.isfinite(val).all() and np.array_equal(getattr(res, k_), val), (key, delay, iterations, k_)
    assert (res.log["iterations"] > 0).all() and (res.nis > 0.0).all()
    print("sensor sizes %s delay=%d iterations=%d: the loop is the entry points one by one; nis in [%.3g, %.3g]" % (key, delay, iterations, res.nis.min(), res.nis.max()))
    a.close(); b.close()
