"""The yardstick of the linear sensor (tests/sensor_ref.py) held to itself, on the CPU: what tests/test_gpu_sensor.py compares the
device with has to be right first.

1. update_sequential (the contract of include/ilqr_hip.h, literally) and update_batch (S = H P Hᵀ + R through LAPACK, Joseph form)
   agree within a tenth of TOL_XU = 1e-10 — the bound of tests/test_gpu_estimator.py, relative to max(1, max |reference|) — on the
   sensors, estimates and covariances the GPU test uses: every model, every ny, shared and per-instance H, with and without ŷ, and the
   range sensor of car_obs.
2. With H the selection rows of the identity it is estimator_ref.update_sequential with the matching mask.
3. measure with H = I is plant_io_ref.measure.
4. A bad pivot is skipped and marked.
5. The filter conditions of the acrobot test (the estimate beats the raw encoders on both angles and prediction alone on the
   velocities) hold on the yardstick with a factor of two to spare."""
import numpy as np
import pytest

import estimator_ref as E
import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
import sensor_ref as S
from ilqr_amd_loader import load_package

TOL_XU = 1e-10
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), "ilqr_estimate_update_linear"), "the library has no ilqr_estimate_update_linear: the yardstick has no subject"
    return p


def _agree(seq, bat):
    return max(P.rel(seq["xhat"], bat["xhat"]), P.rel(seq["P"], bat["P"]), abs(seq["nis"] - bat["nis"]) / max(1.0, abs(bat["nis"])))


@pytest.mark.parametrize("name", S.MODELS)
def test_sequential_and_batch_update_agree_and_p_stays_psd(pkg, name):
    worst = 0.0
    for B in R.BATCHES[name]:
        x1, _, _ = R.inputs(pkg.workloads, name, B)
        n = x1.shape[1]
        xh, ys = E.start(x1, n)
        Ps = E.p_start(B, n)
        for ny in S.NY[name]:
            for H in (S.sensor(n, ny), S.sensors(n, ny, B)):
                y = S.readings(H, ys)
                for yhat in (None, S.some_yhat(y)):
                    for b in range(B):
                        Hb = H if H.ndim == 2 else H[b]
                        yh = None if yhat is None else yhat[b]
                        seq = S.update_sequential(xh[b], Ps[b], y[b], Hb, S.r(ny), yh)
                        bat = S.update_batch(xh[b], Ps[b], y[b], Hb, S.r(ny), yh)
                        d = _agree(seq, bat)
                        worst = max(worst, d)
                        assert seq["first_bad"] == -1 and d <= 0.1 * TOL_XU, (name, B, ny, H.ndim, b, d)
                        ev = np.linalg.eigvalsh(seq["P"])
                        assert np.array_equal(seq["P"], seq["P"].T) and ev[0] >= -1e-12 * ev[-1], (name, ny, b, ev[0], ev[-1])
                        assert np.trace(seq["P"]) < np.trace(Ps[b])
    print("sequential against batch %s: worst relative difference %.2e (bound %.1e)" % (name, worst, 0.1 * TOL_XU))


def test_range_sensor_of_car_obs(pkg):
    for B in R.BATCHES["car_obs"]:
        x1, _, _ = R.inputs(pkg.workloads, "car_obs", B)
        xh, ys = E.start(x1, 3)
        H, yhat, y, rr = S.range_sensor(xh, ys)
        assert (np.hypot(xh[:, 0], xh[:, 1]) > 1e-3).all(), "the range sensor has no Jacobian at the origin"
        for b in range(B):
            seq = S.update_sequential(xh[b], E.p_start(B, 3)[b], y[b], H[b], rr, yhat[b])
            bat = S.update_batch(xh[b], E.p_start(B, 3)[b], y[b], H[b], rr, yhat[b])
            assert _agree(seq, bat) <= 0.1 * TOL_XU, (B, b, _agree(seq, bat))
            # linearised at the estimate on entry: the first innovation is y − h(x̂)
            assert abs(seq["innovation"][0] - (y[b, 0] - yhat[b, 0])) < 1e-15


@pytest.mark.parametrize("name", S.MODELS)
def test_selection_rows_are_the_selection_filter(pkg, name):
    x1, _, _ = R.inputs(pkg.workloads, name, 3)
    n = x1.shape[1]
    xh, y = E.start(x1, n)
    Ps = E.p_start(3, n)
    for mask in E.masks(name, n):
        idx = np.flatnonzero(mask)
        for b in range(3):
            a = S.update_sequential(xh[b], Ps[b], y[b, idx], S.selection(mask), E.r(n)[idx])
            e = E.update_sequential(xh[b], Ps[b], y[b], E.r(n), mask)
            assert P.rel(a["xhat"], e["xhat"]) < 1e-15 and P.rel(a["P"], e["P"]) < 1e-15 and abs(a["nis"] - e["nis"]) < 1e-13 * max(1.0, e["nis"])
            assert np.allclose(a["innovation"], e["innovation"][idx], rtol=0, atol=1e-15)


def test_measure_with_the_identity_is_the_plain_measurement(pkg):
    n, step = 12, 4
    z = pkg.candidate_noise(R.SEED, 2, *IO.measure_shape(step))
    x = np.cos(np.arange(2 * n, dtype=np.float64)).reshape(2, n)
    for b in range(2):
        assert np.array_equal(S.measure(x[b], np.eye(n), IO.sigma_y(n), z[b], step), IO.measure(x[b], IO.sigma_y(n), z[b], step))
        assert np.array_equal(S.measure(x[b], np.eye(n), None, None, step), x[b])
    H = S.sensor(n, 20)
    y = S.measure(x[0], H, S.sigma_y(20), z[0], step)
    j = 17                                         # past the first key field: row 5 + 1, column 1
    assert abs(y[j] - (H[j] @ x[0] + S.sigma_y(20)[j] * z[0][6, step, 1])) < 1e-15 and S.sigma_y(20)[j] != 0.0


def test_a_bad_pivot_is_skipped_and_marked():
    H = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    u = S.update_sequential(np.zeros(3), np.diag([1.0, -3.0, 1.0]), np.ones(4), H, np.ones(4))          # s_1 = −3 + 1
    assert u["first_bad"] == 1 and u["innovation"][1] == 0.0 and u["xhat"][1] == 0.0 and u["xhat"][2] == 0.5
    assert abs(u["xhat"][0] - (0.5 + 0.5 / 3.0)) < 1e-15 and abs(u["nis"] - (0.5 + 0.5 + 0.25 / 1.5)) < 1e-15
    # d = P h is a sum over every column, so a NaN in P reaches every row's s: all rows are skipped, the first one is marked
    u = S.update_sequential(np.zeros(3), np.diag([1.0, NAN, 1.0]), np.ones(4), H, np.ones(4))
    assert u["first_bad"] == 0 and not u["innovation"].any() and not u["xhat"].any() and u["nis"] == 0.0


def test_the_yardstick_filters(pkg):
    F = S.FILTER
    x1, ub, _ = R.inputs(pkg.workloads, F["name"], F["B"])
    z = pkg.candidate_noise(F["seed"], F["B"], *IO.measure_shape(F["periods"] * F["k"]))
    q1_hat, q1_raw, q2_hat, q2_raw, vel_hat, vel_open = S.filter_scores(S.filter_run(ub, x1, z))
    print("filter on the yardstick: q1 %.3e (raw %.3e), q2 %.3e (raw %.3e), velocities %.3e (prediction alone %.3e)"
          % (q1_hat, q1_raw, q2_hat, q2_raw, vel_hat, vel_open))
    assert 2.0 * q1_hat < q1_raw and 2.0 * q2_hat < q2_raw and 2.0 * vel_hat < vel_open
