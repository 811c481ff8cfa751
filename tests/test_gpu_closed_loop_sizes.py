"""The closed-loop kernels — plant step and measure, the filter's time and measurement updates, the linear sensor's update and
measure — at model sizes they have never run at. Their own GPU tests (test_gpu_mpc_loop.py, test_gpu_plant_io.py,
test_gpu_estimator.py, test_gpu_sensor.py) use the built-in models: nx in {3, 4, 12, 32}. Here the synth family of the MPC sweep
(tests/test_gpu_mpc_sweep.py: the same modules under the same names, nothing new to compile), T = 21:

    (1, 1)    the smallest small-form model                       (4, 3)   the largest; B = 70: two waves, the second ragged
    (5, 1)    the first large size, split rows, one tile          (17, 2)  odd, two tiles (NT = 2, NP = 32, ld = 48)
    (33, 2)   unsplit rows, NT = 3, word 1 of the update's mask, noise key fields 1 + j / 16 and 5 + j / 16 beyond the first two
    (64, 8)   every lane owns a row, NT = 4 and the ld = NP + 16 padding at NP = 64, the predict kernel's 124 KB of LDS (the
              function-attribute branch of est_launch), bit 31 of mask word 1

B = 3 on the large form. Inputs: estimator_ref's and sensor_ref's own generators (start, p_start, q, r, masks; sensor, sensors,
readings, some_yhat, r, sigma_y), plant_ref's starts and sigma_x, plant_io_ref's sigma_y. The noise of the yardsticks is numpy's
(sample_ref.noise), not the library's host twin. Bound: TOL_XU = 1e-10 relative to max(1, max |reference|), the four modules' own.
The yardsticks' sequential and textbook (LAPACK, Joseph form) updates are held to each other here at a tenth of it, as
tests/test_estimator_ref.py and tests/test_sensor_ref.py do at the built-in sizes."""
import numpy as np
import pytest

import estimator_ref as E
import mpc_ref as M
import plant_io_ref as IO
import plant_ref as PR
import policy_ref as P
import sample_ref as SR
import sensor_ref as S
import test_gpu_mpc_sweep as SW
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU = 1e-10
T = M.T_SWEEP
SEED = PR.SEED
SIZES = [(1, 1), (4, 3), (5, 1), (17, 2), (33, 2), (64, 8)]
IDS = ["%dx%d" % nm for nm in SIZES]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    return p


def _batch(n, m):
    return 70 if (n <= 4 and m <= 4) else 3


def _some(B):
    return range(B) if B <= 3 else (0, 1, 63, 64, 69)


def _solved(pkg, n, m):
    """a handle of the sweep's module for (n, m), solved briefly (the kernels need a policy, not a converged one), and its plan;
    the model is traced once per size and process, together with the sweep (its table of registered names)"""
    B = _batch(n, m)
    opts = pkg.Options(verbose=0, **PR.SOLVE)
    if (n, m) in SW._MODELS:
        sol = pkg.Solver(model=SW._MODELS[(n, m)], horizon=T, batch=B, options=opts)
    else:
        mdl = pkg.models.synth_nm(n, m)
        sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                         [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=opts, name=M.module_name(n, m))
        SW._MODELS[(n, m)] = sol.model
    assert (sol.nx, sol.nu, sol.B) == (n, m, B)
    x1, ub = M.sweep_inputs(n, m, B, T)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    (xb, ubs), (K, _) = sol.get_trajectory(), sol.get_policy()
    assert np.isfinite(K).all() and np.abs(K).max() > 0
    return sol, xb, ubs, K


def _name(n, m):
    """the size under a name estimator_ref.predict / jacobian can look up: plant_ref's numpy synth dynamics"""
    name = "synth_nm_%d_%d" % (n, m)
    PR._F.setdefault(name, PR.synth_f(n, m))
    return name


# ----------------------------------------------------------------------------------------------------------- plant step, measure
@pytest.mark.parametrize("nm", SIZES, ids=IDS)
def test_plant_step_and_measure_over_the_sizes(pkg, nm):
    n, m = nm
    sol, xb, ub, K = _solved(pkg, n, m)
    B = sol.B
    f = PR.dynamics(_name(n, m))
    x0, sig = PR.plant_starts(xb), PR.sigma_x(n)
    worst = dict(x=0.0, u=0.0, y=0.0)
    for k, s0 in ((1, 0), (3, 5)):
        out = sol.plant_step_(x0, steps=k, feedback=True, sigma_x=sig, seed=SEED, step0=s0)
        quiet = sol.plant_step_(x0, steps=k, feedback=True)
        z = SR.noise(SEED, B, *PR.noise_shape(n, s0, k))
        assert np.array_equal(out["x"][:, 0], x0) and (out["first_nonfinite"] == -1).all()
        loud = sig != 0.0
        assert (out["x"][:, 1][:, loud] != quiet["x"][:, 1][:, loud]).all() and np.array_equal(out["x"][:, 1][:, ~loud], quiet["x"][:, 1][:, ~loud])
        for b in _some(B):
            r = PR.plant_step(f, xb[b], ub[b], K[b], None, x0[b], k, True, sig, z[b], s0)
            worst["x"], worst["u"] = max(worst["x"], P.rel(out["x"][b], r["x"])), max(worst["u"], P.rel(out["u"][b], r["u"]))
            # the noise itself, component by component: its key fields 1 + j / 16 reach 5 at nx = 64
            zz = np.array([z[b][PR.noise_slot(j)[0], s0, PR.noise_slot(j)[1]] for j in np.flatnonzero(loud)])
            assert not loud.any() or np.abs((out["x"][b, 1] - quiet["x"][b, 1])[loud] / sig[loud] - zz).max() < 1e-9, (nm, b)     # (nx = 1: its one component is the quiet one)
    sy = IO.sigma_y(n)
    for step, first in ((0, 0), (7, 11)):
        y = sol.plant_measure_(x0, step=step, sigma_y=sy, seed=SEED, first_instance=first)
        z = SR.noise(SEED, B, *IO.measure_shape(step), first_instance=first)
        ref = np.stack([IO.measure(x0[b], sy, z[b], step) for b in range(B)])
        worst["y"] = max(worst["y"], P.rel(y, ref))
        assert np.array_equal(y[:, sy == 0.0], x0[:, sy == 0.0]) and (y[:, sy != 0.0] != x0[:, sy != 0.0]).all()
    print("closed-loop sizes %dx%d plant step and measure: %s" % (n, m, worst))
    assert max(worst.values()) < TOL_XU, (nm, worst)
    sol.close()


# ----------------------------------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("nm", SIZES, ids=IDS)
def test_predict_and_update_over_the_sizes(pkg, nm):
    """estimate_predict_ over two steps (at nx = 64 the first launch with more than 64 KiB of LDS) and estimate_update_ under both
    masks against the yardstick; the yardstick's textbook update agrees with its sequential one"""
    n, m = nm
    sol, xb, ub, K = _solved(pkg, n, m)
    B = sol.B
    name = _name(n, m)
    xh, y = E.start(PR.plant_starts(xb), n)
    Ps = E.p_start(B, n)
    worst, forms = 0.0, 0.0
    x1, P1 = sol.estimate_predict_(xh, Ps, steps=2, feedback=True, q=E.q(n))
    assert np.array_equal(P1, P1.transpose(0, 2, 1))
    assert np.array_equal(x1, sol.plant_step_(xh, steps=2, feedback=True)["x"][:, -1])
    refs = {b: E.predict(name, xb[b], ub[b], K[b], None, xh[b], Ps[b], 2, True, q=E.q(n)) for b in _some(B)}
    for b, (rx, rP) in refs.items():
        worst = max(worst, P.rel(x1[b], rx), P.rel(P1[b], rP))
    for mask in E.masks(name, n):
        out = sol.estimate_update_(x1, P1, y, E.r(n), measured=mask)
        assert np.array_equal(out["P"], out["P"].transpose(0, 2, 1)) and (out["first_bad"] == -1).all()
        assert (out["innovation"][:, mask == 0] == 0.0).all() and (out["innovation"][:, mask == 1] != 0.0).all()
        for b, (rx, rP) in refs.items():
            ref = E.update_sequential(rx, rP, y[b], E.r(n), mask)
            errs = [P.rel(out["xhat"][b], ref["xhat"]), P.rel(out["P"][b], ref["P"]), P.rel(out["innovation"][b], ref["innovation"]),
                    abs(out["nis"][b] - ref["nis"]) / max(1.0, abs(ref["nis"]))]
            worst = max(worst, max(errs))
            tb = E.update_batch(rx, rP, y[b], E.r(n), mask)
            forms = max(forms, P.rel(tb["xhat"], ref["xhat"]), P.rel(tb["P"], ref["P"]), abs(tb["nis"] - ref["nis"]) / max(1.0, abs(ref["nis"])))
    print("closed-loop sizes %dx%d predict and update: worst %.2e; the yardstick's two forms %.2e" % (n, m, worst, forms))
    assert worst < TOL_XU and forms < 0.1 * TOL_XU, (nm, worst, forms)
    sol.close()


@pytest.mark.parametrize("nm,j", [((33, 2), 32), ((64, 8), 32), ((64, 8), 63)], ids=["33x2-j32", "64x8-j32", "64x8-j63"])
def test_a_skipped_pivot_in_mask_word_one(pkg, nm, j):
    """One instance gets a non-positive P_jj + r_j at a measured j >= 32: that component alone is skipped there, first_bad == j, and
    the neighbouring instances are bit for bit what they are without it"""
    n, m = nm
    sol, xb, ub, K = _solved(pkg, n, m)
    B, bad_b = sol.B, sol.B - 2
    xh, y = E.start(PR.plant_starts(xb), n)
    Ps = E.p_start(B, n)
    mask = E.masks(_name(n, m), n)[1]
    assert mask[j] == 1
    clean = sol.estimate_update_(xh, Ps, y, E.r(n), measured=mask)
    Pn = Ps.copy(); Pn[bad_b, j, j] = -2.0 * E.r(n)[j]
    out = sol.estimate_update_(xh, Pn, y, E.r(n), measured=mask)
    ref = E.update_sequential(xh[bad_b], Pn[bad_b], y[bad_b], E.r(n), mask)
    assert ref["first_bad"] == j and out["first_bad"][bad_b] == j and out["innovation"][bad_b, j] == 0.0
    rest = np.arange(n) != j
    assert (out["innovation"][bad_b, rest] != 0.0).all()                    # that component alone
    errs = [P.rel(out["xhat"][bad_b], ref["xhat"]), P.rel(out["P"][bad_b], ref["P"]), P.rel(out["innovation"][bad_b], ref["innovation"]),
            abs(out["nis"][bad_b] - ref["nis"]) / max(1.0, abs(ref["nis"]))]
    print("closed-loop sizes %dx%d skipped pivot j=%d: %s" % (n, m, j, " ".join("%.2e" % e for e in errs)))
    assert max(errs) < TOL_XU, errs
    others = np.arange(B) != bad_b
    assert (out["first_bad"][others] == -1).all()
    for key in clean:
        assert np.array_equal(out[key][others], clean[key][others]), key
    sol.close()


# ----------------------------------------------------------------------------------------------------------- the linear sensor
@pytest.mark.parametrize("nm", SIZES, ids=IDS)
def test_linear_sensor_over_the_sizes(pkg, nm):
    """estimate_update_linear_ with ny in {2, nx + 1 (at most 64), 64}, a shared and a per-instance H, with and without ŷ, and
    plant_measure_linear_, against the yardstick"""
    n, m = nm
    sol, xb, ub, K = _solved(pkg, n, m)
    B = sol.B
    x0 = PR.plant_starts(xb)
    xh, ys = E.start(x0, n)
    Ps = E.p_start(B, n)
    worst, forms, meas = 0.0, 0.0, 0.0
    for ny in sorted({2, min(n + 1, 64), 64}):
        for H in (S.sensor(n, ny), S.sensors(n, ny, B)):
            y = S.readings(H, ys)
            for yhat in (None, S.some_yhat(y)):
                out = sol.estimate_update_linear_(xh, Ps, y, H, S.r(ny), yhat=yhat)
                assert np.array_equal(out["P"], out["P"].transpose(0, 2, 1)) and (out["first_bad"] == -1).all()
                for b in _some(B):
                    Hb, yb = (H if H.ndim == 2 else H[b]), (None if yhat is None else yhat[b])
                    ref = S.update_sequential(xh[b], Ps[b], y[b], Hb, S.r(ny), yb)
                    worst = max(worst, P.rel(out["xhat"][b], ref["xhat"]), P.rel(out["P"][b], ref["P"]), P.rel(out["innovation"][b], ref["innovation"]),
                                abs(out["nis"][b] - ref["nis"]) / max(1.0, abs(ref["nis"])))
                    tb = S.update_batch(xh[b], Ps[b], y[b], Hb, S.r(ny), yb)
                    forms = max(forms, P.rel(tb["xhat"], ref["xhat"]), P.rel(tb["P"], ref["P"]), abs(tb["nis"] - ref["nis"]) / max(1.0, abs(ref["nis"])))
        H, sy, step, first = S.sensor(n, ny), S.sigma_y(ny), 7, 5
        y = sol.plant_measure_linear_(x0, H, step=step, sigma_y=sy, seed=SEED, first_instance=first)
        y0 = sol.plant_measure_linear_(x0, H, step=step)
        z = SR.noise(SEED, B, *IO.measure_shape(step), first_instance=first)
        for b in _some(B):
            meas = max(meas, P.rel(y[b], S.measure(x0[b], H, sy, z[b], step)), P.rel(y0[b], S.measure(x0[b], H, None, None, step)))
        assert np.array_equal(y[:, sy == 0.0], y0[:, sy == 0.0]) and (y[:, sy != 0.0] != y0[:, sy != 0.0]).all()
    print("closed-loop sizes %dx%d linear sensor: update %.2e, measure %.2e; the yardstick's two forms %.2e" % (n, m, worst, meas, forms))
    assert worst < TOL_XU and meas < TOL_XU and forms < 0.1 * TOL_XU, (nm, worst, meas, forms)
    sol.close()
