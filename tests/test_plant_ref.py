"""The plant step's yardstick (tests/plant_ref.py) without a GPU: on hand-made arrays it is the definition of include/ilqr_hip.h; with
feedback, no noise and x = x̄_0 it is mpc_ref.policy_rollout at α = 0; the noise index mapping keeps every drawn component out of row
0 of ilqr_candidate_noise; and the inputs of the GPU test (tests/test_gpu_mpc_loop.py), solved on the oracle, have the properties
that test relies on — the callables written here are the models' dynamics, every plant state stays finite, and ten times the
yardstick's own spread under a 1e-15 move of x stays below the bound of the GPU file, TOL_XU = 1e-10."""
import numpy as np
import pytest

import mpc_ref as M
import plant_ref as R
import policy_ref as P
from ilqr_amd_loader import load_package

TOL_XU = 1e-10          # tests/test_gpu_mpc_loop.py, tests/test_gpu_mpc_sweep.py
B_CPU = 3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return load_package()


def test_hand_made_arrays():
    T, n, m = 4, 2, 1
    xb = np.arange(T * n, dtype=np.float64).reshape(T, n)
    ub = np.array([[1.0], [2.0], [3.0]])
    K = np.zeros((T - 1, n, m)); K[:, 0, 0] = 0.5
    w = np.array([[10.0, 7.0], [20.0, 7.0], [30.0, 7.0], [40.0, 7.0]])
    f = lambda x, u, w_, t: np.array([x[0] + u[0], x[1] + w_[0]])
    r = R.plant_step(f, xb, ub, K, w, [1.0, 1.0], 2)
    assert np.array_equal(r["u"], [[1.0], [2.0]]) and np.array_equal(r["x"], [[1.0, 1.0], [2.0, 11.0], [4.0, 31.0]]) and r["first_nonfinite"] == -1
    # feedback: ū + K (x − x̄); the plant's own parameters replace the handle's first column only where given
    r = R.plant_step(f, xb, ub, K, w, [1.0, 1.0], 2, feedback=True, w_plant=np.array([[100.0], [200.0]]))
    assert np.array_equal(r["u"], [[1.5], [2.0 + 0.5 * (2.5 - 2.0)]]) and np.array_equal(r["x"][:, 1], [1.0, 101.0, 301.0])
    # noise: component j at global step step0 + i from row 1 + j // 16, column j % 16; a zero sigma draws nothing
    z = np.zeros((2, 8, 16)); z[1, 5, 0], z[1, 5, 1], z[1, 6, 0] = 2.0, 3.0, 4.0
    r = R.plant_step(f, xb, ub, K, w, [1.0, 1.0], 2, sigma_x=[0.5, 0.0], z=z, step0=5)
    assert np.array_equal(r["x"], [[1.0, 1.0], [2.0 + 1.0, 11.0], [3.0 + 2.0 + 2.0, 31.0]])
    # a non-finite state is marked at the step that produced it
    r = R.plant_step(f, xb, ub, K, w, [1.0, np.nan], 2)
    assert r["first_nonfinite"] == 0
    r = R.plant_step(lambda x, u, w_, t: x * (np.inf if t == 1 else 1.0), xb, ub, K, w, [1.0, 1.0], 3)
    assert r["first_nonfinite"] == 1


def test_noise_slot_keeps_out_of_row_zero(pkg):
    assert R.noise_slot(17) == (1 + 1, 1) and R.noise_slot(0) == (1, 0) and R.noise_slot(15) == (1, 15) and R.noise_slot(16) == (2, 0)
    assert R.noise_slot(63) == (4, 15)
    assert R.noise_shape(32, 5, 3) == (3, 8, 16) and R.noise_shape(3, 0, 1) == (2, 1, 16) and R.noise_shape(33, 0, 1) == (4, 1, 16)
    z = pkg.candidate_noise(7, 2, *R.noise_shape(32, 5, 3))
    assert z.shape == (2, 3, 8, 16) and not z[:, 0].any() and (z[:, 1:] != 0.0).all()


def _solved(pkg, oracle, name):
    x1, ub, w = R.inputs(pkg.workloads, name, B_CPU)
    ref = oracle.solve_batch(name, R.T, x1, ub, options=oracle.default_options(**R.SOLVE), w=w)
    return ref["x"], ref["u"], ref["K"], ref["k"], w


@pytest.mark.parametrize("name", sorted(R.BATCHES))
def test_the_gpu_tests_inputs_on_the_oracle(pkg, oracle, name):
    xb, ub, K, k, w = _solved(pkg, oracle, name)
    f = R.dynamics(name)
    n = xb.shape[2]
    # the callables are the model's dynamics: they reproduce the oracle's nominal trajectory
    for b in range(B_CPU):
        for t in range(R.T - 1):
            assert P.rel(f(xb[b, t], ub[b, t], None if w is None else w[b, t], t), xb[b, t + 1]) < 1e-12, (name, b, t)
    # feedback, no noise, x = x̄_0: mpc_ref.policy_rollout at α = 0, its first k + 1 states
    p = M.Problem(f, lambda x, u, w_, t: 0.0, lambda x, u, w_, t: 0.0, None, None, (), ())
    for b in range(B_CPU):
        wb = None if w is None else w[b]
        full = M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], xb[b, 0], 0.0, wb)
        for steps in R.STEPS:
            r = R.plant_step(f, xb[b], ub[b], K[b], wb, xb[b, 0], steps, feedback=True)
            assert np.array_equal(r["x"], full["x"][:steps + 1]) and np.array_equal(r["u"], full["u"][:steps])
    # the GPU test's cases: finite, and ten times the yardstick's own spread below the bound
    x = R.plant_starts(xb)
    sig = R.sigma_x(n)
    worst = 0.0
    for steps, fb, ns, s0 in R.cases():
        z = pkg.candidate_noise(R.SEED, B_CPU, *R.noise_shape(n, s0, steps)) if ns else None
        wp = R.plant_parameters(w, steps)
        refs = R.reference(name, xb, ub, K, w, x, steps, fb, sig if ns else None, z, s0, wp)
        for b, r in enumerate(refs):
            assert r["first_nonfinite"] == -1 and np.isfinite(r["x"]).all() and np.isfinite(r["u"]).all(), (name, steps, fb, ns, s0, b)
            worst = max(worst, R.spread(f, xb[b], ub[b], K[b], None if w is None else w[b], x[b], steps, feedback=bool(fb),
                                        sigma_x=sig if ns else None, z=None if z is None else z[b], step0=s0,
                                        w_plant=None if wp is None else wp[b]))
    print("plant step spread %s: %.2e" % (name, worst))
    assert 10.0 * worst < TOL_XU, (name, worst)
