"""The plant score's yardstick (tests/plant_score_ref.py) without a GPU: on hand-made arrays it is the definition of
include/ilqr_hip.h; on plant steps of the kind the GPU test scores (tests/test_gpu_mpc_preview.py: feedback, sigma_x, taken here from
a policy solved without a device) ten times the yardstick's own spread under a 1e-15 move of x and u stays below the project's
standing bounds, cost 1e-9 relative and violation 1e-9 per max(1, |v|); and the closed form of the preview holds on a numpy
restatement of the shift's parameter rows."""
import math

import numpy as np
import pytest

import mpc_ref as M
import plant_ref as R
import plant_score_ref as SR
from ilqr_amd_loader import load_package

TOL_COST, TOL_VIOL = 1e-9, 1e-9      # tests/test_gpu_mpc_preview.py, tests/test_gpu_mpc_sweep.py
B_CPU, STEPS = 3, 3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return load_package()


def test_hand_made_arrays():
    p = M.Problem(None, lambda x, u, w, t: x[0] * x[0] + 2.0 * u[0] + w[0] + 100.0 * t, None,
                  lambda x, u, w, t: np.array([u[0] - 1.0, x[1] - w[1]]), None, (0,), ())
    x = np.array([[1.0, 2.0], [3.0, -4.0], [99.0, 99.0]])          # the last row is not read
    u = np.array([[0.5], [3.0]])
    w = np.array([[10.0, 1.0], [20.0, 1.0], [30.0, 1.0]])
    r = SR.plant_score(p, x, u, w)
    assert np.array_equal(r["cost"], [1.0 + 1.0 + 10.0, 9.0 + 6.0 + 20.0 + 100.0])
    assert np.array_equal(r["violation"], [1.0, 5.0])               # step 0: max(0, −0.5) and |2 − 1|; step 1: max(0, 2) and |−4 − 1|
    # the plant's own parameters replace the columns they have; the others stay the handle's
    r = SR.plant_score(p, x, u, w, w_plant=np.array([[1000.0], [2000.0]]))
    assert np.array_equal(r["cost"], [1002.0, 2115.0]) and np.array_equal(r["violation"], [1.0, 5.0])
    r = SR.plant_score(p, x, u, w, constrained=False)
    assert np.array_equal(r["violation"], [0.0, 0.0])
    # a non-finite row stays in its own element
    xn = x.copy(); xn[1, 0] = np.nan
    r = SR.plant_score(p, xn, u, w)
    assert r["cost"][0] == 12.0 and math.isnan(r["cost"][1]) and np.array_equal(r["violation"], [1.0, 5.0])
    xn = x.copy(); xn[0, 1] = np.nan
    r = SR.plant_score(p, xn, u, w)
    assert math.isnan(r["violation"][0]) and r["violation"][1] == 5.0 and np.array_equal(r["cost"], [12.0, 135.0])


def _plant_steps(pkg, oracle, name):
    """(x [B, k + 1, n], u [B, k, m], w, w_plant) of plant steps with feedback and sigma_x under a policy solved without a device"""
    if name == "synth5w":
        xb, ub, K, _ = M.synth5w_restatement_policy(B_CPU)
        w = M.synth5w_parameters(B_CPU)
        f = M.synth5w().f
    else:
        x1, ub0, w = R.inputs(pkg.workloads, name, B_CPU)
        ref = oracle.solve_batch(name, R.T, x1, ub0, options=oracle.default_options(**R.SOLVE), w=w)
        xb, ub, K = ref["x"], ref["u"], ref["K"]
        f = R.dynamics(name)
    n = xb.shape[2]
    x0 = R.plant_starts(xb)
    z = pkg.candidate_noise(R.SEED, B_CPU, *R.noise_shape(n, 0, STEPS))
    wp = R.plant_parameters(w, STEPS)
    outs = [R.plant_step(f, xb[b], ub[b], K[b], None if w is None else w[b], x0[b], STEPS, True, R.sigma_x(n), z[b], 0,
                         None if wp is None else wp[b]) for b in range(B_CPU)]
    return np.stack([o["x"] for o in outs]), np.stack([o["u"] for o in outs]), w, wp


@pytest.mark.parametrize("name", ["car_obs", "synth5w", "synth12"])
def test_spread_of_the_yardstick_stays_below_the_bounds(pkg, oracle, name):
    x, u, w, wp = _plant_steps(pkg, oracle, name)
    p = SR.problem(name)
    worst = dict(cost=0.0, viol=0.0)
    for b in range(B_CPU):
        for plant_w in (None, wp):
            wb, wpb = None if w is None else w[b], None if plant_w is None else plant_w[b]
            r = SR.plant_score(p, x[b], u[b], wb, wpb)
            assert np.isfinite(r["cost"]).all() and np.isfinite(r["violation"]).all() and (r["cost"] > 0).all(), (name, b)
            s = SR.spread(p, x[b], u[b], wb, wpb)
            worst = {key: max(worst[key], s[key]) for key in worst}
    print("plant score spread %s: cost %.2e, violation %.2e" % (name, worst["cost"], worst["viol"]))
    assert 10.0 * worst["cost"] < TOL_COST and 10.0 * worst["viol"] < TOL_VIOL, (name, worst)


@pytest.mark.parametrize("T,k,P", [(9, 3, 4), (11, 1, 3), (11, 3, 2), (5, 4, 3)])
def test_closed_form_of_the_preview(T, k, P):
    """after P shifts by k, each fed its k rows of w_preview, row t is θ_{t + P·k} or w_preview[t + P·k − T]"""
    nw, B = 2, 3
    w = 7.0 + np.arange(B * T * nw, dtype=np.float64).reshape(B, T, nw)
    pre = SR.distinct_preview(B, P * k, nw)
    assert len(np.unique(pre)) == pre.size
    for b in range(B):
        got = SR.previewed_parameters(w[b], P, k, pre[b])
        assert np.array_equal(got, SR.preview_closed_form(w[b], P, k, pre[b])), (T, k, P, b)
        if P * k >= T:                      # every row of the horizon is a previewed one
            assert np.array_equal(got, pre[b, P * k - T:]), (T, k, P, b)
    # without a preview the last row is held
    assert np.array_equal(SR.shifted_parameters(w[0], k), np.concatenate([w[0, k:], np.repeat(w[0, -1:], k, axis=0)]))
