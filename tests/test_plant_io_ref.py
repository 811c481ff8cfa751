"""The yardstick of the seam between plant and controller (tests/plant_io_ref.py) without a GPU: on hand-made arrays the clamp, the
measurement and the two loop orders are the definitions of include/ilqr_hip.h; without limits the limited step is plant_ref.plant_step
bit for bit; the measurement's noise rows keep clear of the process noise's. And the inputs of the GPU test
(tests/test_gpu_plant_io.py), solved on the oracle, have the two properties that test relies on, for every model and batch:

  1. some action component is clamped low, some clamped high and some left alone;
  2. no raw action lies within MARGIN = 1e-9 of a finite limit, so a last-bit difference between the device's action and the
     yardstick's cannot flip a clamp (measured here: the nearest is printed per model; all are above 1e-5).

Ten times the limited yardstick's own spread under a 1e-15 move of x stays below TOL_XU = 1e-10, the bound of the GPU file."""
import numpy as np
import pytest

import plant_io_ref as IO
import plant_ref as R
import policy_ref as P
from ilqr_amd_loader import load_package

TOL_XU = 1e-10          # tests/test_gpu_mpc_loop.py, tests/test_gpu_plant_io.py


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    for fn in ("ilqr_plant_step_limited", "ilqr_plant_measure", "ilqr_mpc_run_io"):
        assert hasattr(p._ffi.lib(), fn), "the library has no %s: the yardstick has no subject" % fn
    return p


def _toy():
    T, n, m = 4, 2, 2
    xb = np.arange(T * n, dtype=np.float64).reshape(T, n)
    ub = np.array([[1.0, -1.0], [2.0, -2.0], [3.0, -3.0]])
    K = np.zeros((T - 1, n, m)); K[:, 0, 0] = 0.5
    f = lambda x, u, w_, t: np.array([x[0] + u[0], x[1] + u[1]])
    return xb, ub, K, f


def test_clamp_on_hand_made_arrays():
    xb, ub, K, f = _toy()
    r = IO.plant_step(f, xb, ub, K, None, [1.0, 1.0], 3, u_min=[-IO.INF, -2.5], u_max=[1.5, IO.INF])
    assert np.array_equal(r["raw"], ub) and np.array_equal(r["u"], [[1.0, -1.0], [1.5, -2.0], [1.5, -2.5]])
    assert np.array_equal(r["side"], [[0, 0], [1, 0], [1, -1]]) and r["saturated"] == 3
    assert np.array_equal(r["x"], [[1.0, 1.0], [2.0, 0.0], [3.5, -2.0], [5.0, -4.5]])          # the dynamics ran under the applied action
    # feedback is clamped too: 1 + 0.5 (3 − 0) = 2.5 -> 2
    r = IO.plant_step(f, xb, ub, K, None, [3.0, 1.0], 1, feedback=True, u_max=[2.0, 0.0])
    assert r["raw"][0, 0] == 2.5 and r["u"][0, 0] == 2.0 and r["u"][0, 1] == -1.0 and r["saturated"] == 1
    # a limit that equals the action does not count; ∓Inf leaves every finite action alone; a NaN action stays NaN and is marked
    r = IO.plant_step(f, xb, ub, K, None, [1.0, 1.0], 3, u_min=[1.0, -IO.INF], u_max=[IO.INF, -1.0])
    assert np.array_equal(r["side"], [[0, 0], [0, 0], [0, 0]]) and r["saturated"] == 0
    r = IO.plant_step(f, xb, ub, K, None, [np.nan, 1.0], 2, feedback=True, u_min=[0.0, -9.0], u_max=[1.0, 9.0])
    assert np.isnan(r["u"][:, 0]).all() and r["first_nonfinite"] == 0 and r["saturated"] == 0
    assert IO.clamp(-0.0, 0.0, 1.0) == (-0.0, 0) and IO.clamp(2.0, 0.0, 1.0) == (1.0, 1) and IO.clamp(-2.0, 0.0, 1.0) == (0.0, -1)


def test_measurement_on_hand_made_arrays(pkg):
    z = np.zeros((9, 8, 16)); z[5, 7, 0], z[5, 7, 1], z[6, 7, 1], z[1, 7, 0] = 2.0, 3.0, 4.0, 100.0
    x = np.arange(18, dtype=np.float64)
    s = np.zeros(18); s[0], s[1], s[17] = 0.5, 0.0, 0.25
    y = IO.measure(x, s, z, 7)
    assert y[0] == 1.0 and y[1] == 1.0 and y[17] == 18.0 and np.array_equal(y[2:17], x[2:17])
    assert np.array_equal(IO.measure(x, None, None, 3), x)
    # rows 5 .. 8 of the host twin: the process noise (plant_ref.noise_slot: rows 1 .. 4 for nx <= 64) never draws from them
    assert IO.measure_shape(7) == (9, 8, 16) and max(R.noise_slot(j)[0] for j in range(64)) == 4 and IO.MEASURE_ROW0 + 63 // 16 == 8
    zz = pkg.candidate_noise(7, 2, *IO.measure_shape(3))
    assert zz.shape == (2, 9, 4, 16) and (zz[:, 5:] != 0.0).all()
    assert len({float(v) for v in zz[0, 1:, 3, 0]}) == 8             # eight different draws: no row repeats another


def test_the_two_loop_orders():
    """a scalar plant x ← x + plan + 0.5 (the 0.5 a disturbance the model does not know), a measurement that adds 0.25, a prediction
    that adds the plan in flight; the re-solve sets the plan to the state it is given"""
    for delay, want_x, want_y in ((0, [1.0, 2.5, 5.75, 12.25], [2.75, 6.0, 12.5]), (1, [1.0, 2.5, 5.25, 10.75], [2.25, 5.0, 10.5])):
        plan = [1.0]
        out = IO.run(np.array([1.0]), 3, 1, delay, plant=lambda x, p: np.stack([x, x + plan[0] + 0.5]), measure_=lambda x, step: x + 0.25,
                     predict=lambda y, p: y + plan[0], resolve=lambda xc, p: plan.__setitem__(0, float(xc[0])))
        assert np.array_equal(out["x"][:, 0], want_x) and np.array_equal(out["y"][:, 0], want_y), (delay, out)
    # k = 2: the measurement steps are 0, 2, 4 (delay 1) and 2, 4, 6 (delay 0)
    for delay, steps in ((1, [0, 2, 4]), (0, [2, 4, 6])):
        seen = []
        IO.run(np.zeros(1), 3, 2, delay, plant=lambda x, p: np.stack([x, x, x]), measure_=lambda x, step: (seen.append(step), x)[1],
               predict=lambda y, p: y, resolve=lambda xc, p: None)
        assert seen == steps


def _solved(pkg, oracle, name, B):
    x1, ub, w = R.inputs(pkg.workloads, name, B)
    ref = oracle.solve_batch(name, R.T, x1, ub, options=oracle.default_options(**R.SOLVE), w=w)
    return ref["x"], ref["u"], ref["K"], w


@pytest.mark.parametrize("name", IO.MODELS)
def test_the_gpu_tests_inputs_on_the_oracle(pkg, oracle, name):
    u_min, u_max = IO.LIMITS[name]
    f = R.dynamics(name)
    for B in R.BATCHES[name]:
        xb, ub, K, w = _solved(pkg, oracle, name, B)
        n = xb.shape[2]
        x = R.plant_starts(xb)
        sig = R.sigma_x(n)
        runs, worst = [], 0.0
        for k, fb, ns, s0 in IO.CASES:
            z = pkg.candidate_noise(R.SEED, B, *R.noise_shape(n, s0, k)) if ns else None
            wp = R.plant_parameters(w, k)
            refs = IO.reference(name, xb, ub, K, w, x, k, fb, sig if ns else None, z, s0, wp, u_min, u_max)
            free = R.reference(name, xb, ub, K, w, x, k, fb, sig if ns else None, z, s0, wp)
            for b, (r, q) in enumerate(zip(refs, free)):
                assert r["first_nonfinite"] == -1 and np.isfinite(r["x"]).all(), (name, B, k, fb, ns, s0, b)
                assert np.array_equal(r["raw"][0], q["u"][0])              # the first raw action is the unlimited step's
                assert r["saturated"] == int(((r["raw"] < u_min) | (r["raw"] > u_max)).sum())
            runs.append(refs)
            if B == min(R.BATCHES[name]):
                for b in range(B):
                    kw = dict(feedback=bool(fb), sigma_x=sig if ns else None, z=None if z is None else z[b], step0=s0,
                              w_plant=None if wp is None else wp[b], u_min=u_min, u_max=u_max)
                    wb = None if w is None else w[b]
                    a_, b_ = IO.plant_step(f, xb[b], ub[b], K[b], wb, x[b], k, **kw), IO.plant_step(f, xb[b], ub[b], K[b], wb, x[b] * (1.0 + 1.0e-15), k, **kw)
                    worst = max(worst, P.rel(b_["x"], a_["x"]), P.rel(b_["u"], a_["u"]))
        low, high, alone, nearest = IO.conditions(runs, u_min, u_max)
        print("plant io inputs %s B=%d: clamped low %s, high %s, left alone %s; nearest raw action to a limit %.2e; spread %.2e"
              % (name, B, low, high, alone, nearest, worst))
        assert low and high and alone, (name, B)                          # condition 1
        assert nearest > IO.MARGIN, (name, B, nearest)                    # condition 2
        assert 10.0 * worst < TOL_XU, (name, worst)
    # without limits the limited yardstick is plant_ref.plant_step, bit for bit
    refs = IO.reference(name, xb, ub, K, w, x, 3, 1, None, None, 0, None, None, None)
    free = R.reference(name, xb, ub, K, w, x, 3, 1, None, None, 0, None)
    for r, q in zip(refs, free):
        assert np.array_equal(r["x"], q["x"]) and np.array_equal(r["u"], q["u"]) and r["saturated"] == 0
    # sigma_y of the GPU test: one zero entry, the others positive and finite
    s = IO.sigma_y(n)
    assert (s >= 0).all() and np.isfinite(s).all() and (s == 0).sum() == 1
