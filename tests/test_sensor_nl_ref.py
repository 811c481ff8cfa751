"""The yardstick of the compiled nonlinear sensor (tests/sensor_nl_ref.py) held to itself, on the CPU: what
tests/test_gpu_sensor_nl.py compares the device with has to be right first.

1. The complex-step Jacobian of every test sensor equals sympy's symbolic one (lambdify) within 1e-13, and the range + heading
   sensor reproduces sensor_ref.range_sensor's H and ŷ.
2. update(iterations = 1) is sensor_ref.update_sequential fed the yardstick's own H and ŷ, bit for bit.
3. The IEKF form — ŷ with the x_prior term, the update run from the prior again — equals the textbook Gauss-Newton IEKF written on
   its own (sensor_nl_ref.iekf_textbook) within a tenth of TOL_XU = 1e-10, the rule tests/test_sensor_ref.py sets for the
   yardstick's two forms; iterations 2 and 3, every sensor, shared and per-instance s.
4. x_prior = x_lin changes ŷ by nothing.
5. The filter conditions of the car_obs test (two beacon ranges, no heading reading): the estimate's position error is below that
   of prediction alone, and with the wide P0 three iterations are no worse than one — both with a factor of two to spare."""
import numpy as np
import pytest

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
import sensor_nl_ref as N
import sensor_ref as S
from ilqr_amd_loader import load_package

TOL_XU = 1e-10


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), "ilqr_estimate_update_sensor"), "the library has no ilqr_estimate_update_sensor: the yardstick has no subject"
    return p


def _cases(pkg):
    """(key, B, x̂ [B, n], P [B, n, n], the states measured [B, n])"""
    for name in S.MODELS:
        for B in R.BATCHES[name]:
            x1, _, _ = R.inputs(pkg.workloads, name, B)
            n = x1.shape[1]
            xh, ys = E.start(x1, n)
            for key in N.BY_MODEL[name]:
                yield key, B, xh, E.p_start(B, n), ys


def test_complex_step_jacobian_is_the_symbolic_one(pkg):
    import sympy as sp
    worst = 0.0
    for key, B, xh, _, _ in _cases(pkg):
        if B != 3:
            continue
        _, nx, ny, ns, _ = N.SENSORS[key]
        x, s, rows, jac = pkg.codegen.sensor_expressions(N.symbolic(key), nx, ns)
        fj = sp.lambdify([x, s], sp.Matrix(jac), "numpy")
        for b in range(B):
            H, yhat = N.linearise(key, xh[b], N.s_shared(key))
            ref = np.array(fj(xh[b], N.s_shared(key)), dtype=np.float64).reshape(ny, nx)
            worst = max(worst, P.rel(H, ref))
    print("complex step against sympy: worst relative difference %.2e" % worst)
    assert worst < 1e-13
    x1, _, _ = R.inputs(pkg.workloads, "car_obs", 70)
    xh, ys = E.start(x1, 3)
    H, yhat, _, _ = S.range_sensor(xh, ys)
    for b in range(70):
        Hn, yn = N.linearise("range_heading", xh[b], N.s_shared("range_heading"))
        assert P.rel(Hn, H[b]) < 1e-14 and P.rel(yn, yhat[b]) < 1e-14, b


def test_one_iteration_is_the_linear_update_fed_the_linearisation(pkg):
    for key, B, xh, Ps, ys in _cases(pkg):
        s = N.s_shared(key)
        y = N.readings(key, ys, s)
        rr = N.r(N.dims(key)[1])
        for b in (0, B - 1):
            H, yhat = N.linearise(key, xh[b], s)
            a, c = N.update(key, xh[b], Ps[b], y[b], s, rr), S.update_sequential(xh[b], Ps[b], y[b], H, rr, yhat)
            for k in a:
                assert np.array_equal(a[k], c[k]), (key, b, k)
            assert a["first_bad"] == -1 and np.array_equal(a["P"], a["P"].T)
            # x_prior = the point of linearisation: the correction is a chain of exact zeros
            assert np.array_equal(N.linearise(key, xh[b], s, xh[b])[1], yhat)


@pytest.mark.parametrize("iterations", [2, 3])
def test_iterated_form_is_the_textbook_iekf(pkg, iterations):
    worst = 0.0
    for key, B, xh, Ps, ys in _cases(pkg):
        for s in (N.s_shared(key), N.s_instances(key, B)):
            y = N.readings(key, ys, s)
            rr = N.r(N.dims(key)[1])
            for b in range(B) if B <= 3 else (0, 1, 63, 64, 69):
                sb = s if s.ndim == 1 else s[b]
                a, t = N.update(key, xh[b], Ps[b], y[b], sb, rr, iterations), N.iekf_textbook(key, xh[b], Ps[b], y[b], sb, rr, iterations)
                d = max(P.rel(a["xhat"], t["xhat"]), P.rel(a["P"], t["P"]))
                worst = max(worst, d)
                assert a["first_bad"] == -1 and d <= 0.1 * TOL_XU, (key, B, b, d)
    print("IEKF form against the textbook, %d iterations: worst relative difference %.2e (bound %.1e)" % (iterations, worst, 0.1 * TOL_XU))


def test_the_yardstick_filters(pkg):
    F = N.FILTER
    x1, ub, w = R.inputs(pkg.workloads, F["name"], F["B"])
    z = pkg.candidate_noise(F["seed"], F["B"], *IO.measure_shape(F["periods"] * F["k"]))
    e1, open_ = N.filter_scores(N.filter_run(ub, w, x1, z, 1))
    e3, _ = N.filter_scores(N.filter_run(ub, w, x1, z, 3))
    print("filter on the yardstick: position mse %.3e with one iteration, %.3e with three, prediction alone %.3e" % (e1, e3, open_))
    assert 2.0 * e1 < open_ and 2.0 * e3 < open_ and 2.0 * e3 < e1
