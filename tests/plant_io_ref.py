"""The yardstick of the seam between plant and controller (tests/test_plant_io_ref.py, tests/test_gpu_plant_io.py): the actuator's
limits, the measurement and the two loop orders of ilqr_mpc_run_io as include/ilqr_hip.h defines them, in plain fp64 numpy over the
callables and arrays of tests/plant_ref.py —

    u_i[r]  = the action of plant_ref.plant_step, feedback included                                  (the RAW action)
    u_i[r] ← u_min[r] if u_i[r] < u_min[r] else (u_max[r] if u_i[r] > u_max[r] else u_i[r])           (plain comparisons: NaN passes)
    saturated = the number of (i, r) with u_i[r] < u_min[r] or u_i[r] > u_max[r]
    y[j]    = x[j] + sigma_y[j] · z[5 + j // 16, step, j % 16]   where sigma_y[j] != 0, else x[j]

with z one instance's block of ilqr_candidate_noise(seed, first_instance, B, 9, step + 1, 16): rows 5 .. 8, the process noise of
plant_ref.plant_step keeps rows 1 .. 4.

The loop (`run`) is written over callables, so that the re-solve — which no numpy loop restates — can be a handle's: per period p,
with k plant steps between re-solves,

    delay 0:  x ← plant(x, p);  xc = measure(x, (p+1)·k);                      plan ← resolve(xc)
    delay 1:  xc = predict(measure(x, p·k));  x ← plant(x, p);                 plan ← resolve(xc)

The limits of the GPU test live here (LIMITS), chosen per model so that on the yardstick every model has an action component
clamped low, one clamped high and one left alone, and no raw action within MARGIN of a limit: a last-bit difference cannot flip a
clamp. tests/test_plant_io_ref.py asserts both on the oracle's solve of the inputs, the GPU test on its own."""
import numpy as np

import mpc_ref as M
import plant_ref as R

MARGIN = 1.0e-9
MEASURE_ROW0 = 5
MODELS = ("car_obs", "acrobot", "synth12", "synth32")
# (k, feedback, process noise, step0) of the limited plant step on the GPU: both step counts, both action forms, both noise
# settings and a non-zero step0; not the full product of plant_ref.cases(), which the unlimited step already runs
CASES = [(1, 1, 0, 0), (3, 0, 0, 0), (3, 1, 0, 5), (3, 1, 1, 5), (3, 0, 1, 0)]
INF = float("inf")


def measure_shape(step):
    """(candidates, steps, nu) to ask ilqr_candidate_noise for"""
    return MEASURE_ROW0 + 4, step + 1, 16


def clamp(u, lo, hi):
    """-> (the action applied, −1 / 0 / +1: clamped low / left alone / clamped high); comparisons only, so NaN is left alone"""
    if u < lo:
        return lo, -1
    if u > hi:
        return hi, 1
    return u, 0


def plant_step(f, xb, ub, K, w, x, steps, feedback=False, sigma_x=None, z=None, step0=0, w_plant=None, u_min=None, u_max=None):
    """plant_ref.plant_step with the limits -> its dict, u the action APPLIED, and raw [steps, m] (the action before the clamp), side
    [steps, m] (−1 / 0 / +1), saturated. u_min / u_max None: no limit on that side."""
    xb, ub = np.asarray(xb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    n, m = xb.shape[1], ub.shape[1]
    lo = np.full(m, -INF) if u_min is None else np.asarray(u_min, dtype=np.float64)
    hi = np.full(m, INF) if u_max is None else np.asarray(u_max, dtype=np.float64)
    xs, us, raw, side = np.zeros((steps + 1, n)), np.zeros((steps, m)), np.zeros((steps, m)), np.zeros((steps, m), dtype=np.int64)
    xs[0] = x
    nf = -1
    with np.errstate(all="ignore"):
        for i in range(steps):
            for r in range(m):
                v = ub[i, r]
                if feedback:
                    a1 = 0.0
                    for j in range(n):
                        a1 += K[i, j, r] * xs[i, j]
                    v = v + a1
                    a2 = 0.0
                    for j in range(n):
                        a2 += K[i, j, r] * xb[i, j]
                    v = v - a2
                raw[i, r] = v
                us[i, r], side[i, r] = clamp(v, lo[r], hi[r])
            wi = M._NONE if w is None else np.array(w[i], dtype=np.float64)
            if w_plant is not None:
                wi[:len(w_plant[i])] = w_plant[i]
            y = np.array(f(xs[i], us[i], wi, i), dtype=np.float64)
            if sigma_x is not None:
                for j in range(n):
                    if sigma_x[j] != 0.0:
                        row, col = R.noise_slot(j)
                        y[j] = y[j] + sigma_x[j] * z[row, step0 + i, col]
            xs[i + 1] = y
            if nf < 0 and not np.isfinite(y).all():
                nf = i
    return dict(x=xs, u=us, raw=raw, side=side, first_nonfinite=nf, saturated=int((side != 0).sum()))


def measure(x, sigma_y, z, step):
    """y [n] of one instance; z [>= 9, > step, 16] of this instance (None allowed when sigma_y is None)"""
    y = np.array(x, dtype=np.float64)
    if sigma_y is not None:
        for j in range(len(y)):
            if sigma_y[j] != 0.0:
                y[j] = y[j] + sigma_y[j] * z[MEASURE_ROW0 + j // 16, step, j % 16]
    return y


def run(x0, periods, k, delay, plant, measure_, predict, resolve):
    """The two loop orders. plant(x, p) -> the states of period p [k + 1, ...] from x; measure_(x, step); predict(y, p) -> the state k
    steps on under the plan in flight; resolve(xc, p) installs the next plan. -> dict(x [periods·k + 1, ...], y [periods, ...])"""
    x = np.array(x0, dtype=np.float64)
    xs, ys = [x[None]], []
    for p in range(periods):
        if delay:
            xc = predict(measure_(x, p * k), p)
        seg = plant(x, p)
        x = np.array(seg[-1])
        xs.append(seg[1:])
        if not delay:
            xc = measure_(x, (p + 1) * k)
        ys.append(np.array(xc))
        resolve(xc, p)
    return dict(x=np.concatenate(xs, axis=0), y=np.stack(ys))


# ------------------------------------------------------------------------------------------------- the inputs of the GPU test
# (u_min, u_max) per model. A component with (−Inf, +Inf) is the one left alone where the model has more than one; acrobot's single
# action is left alone at some (instance, step) pairs and clamped at others.
LIMITS = {
    "car_obs": (np.array([4.0, -1.0]), np.array([INF, 6.0])),
    "acrobot": (np.array([-0.5]), np.array([0.3])),
    "synth12": (np.array([-0.5, -INF, -INF, -0.25, -INF]), np.array([INF, 0.3, INF, 0.75, INF])),
    "synth32": (np.array([-0.5, -INF, -INF, -0.05, -INF, -INF, -INF, -0.5]), np.array([INF, 0.25, INF, 0.6, INF, INF, 0.05, INF])),
}


def sigma_y(n):
    """a different size per state component, one of them zero (that component is copied)"""
    s = 5.0e-3 * (2.0 + np.arange(n)) / n
    s[(n // 2 + 1) % n] = 0.0
    return s


def reference(name, xb, ub, K, w, x, k, fb, sig, z, s0, wp, u_min, u_max):
    """every instance: a list of plant_step dicts"""
    f = R.dynamics(name)
    return [plant_step(f, xb[b], ub[b], K[b], None if w is None else w[b], x[b], k, bool(fb), sig, None if z is None else z[b], s0,
                       None if wp is None else wp[b], u_min, u_max) for b in range(xb.shape[0])]


def conditions(refs_per_case, u_min, u_max):
    """of the yardstick's runs of one model: (some action clamped low, some clamped high, some left alone, the smallest distance of a
    raw action to a finite limit)"""
    low = high = alone = False
    nearest = INF
    for refs in refs_per_case:
        for r in refs:
            low, high, alone = low or bool((r["side"] < 0).any()), high or bool((r["side"] > 0).any()), alone or bool((r["side"] == 0).any())
            for lim in (u_min, u_max):
                d = np.abs(r["raw"] - lim[None, :])
                nearest = min(nearest, float(d[np.isfinite(d)].min(initial=INF)))
    return low, high, alone, nearest
