"""The closed MPC loop enqueued once (ilqr_mpc_run) against the same loop stepped from the host, in the same process.

Workload: car_obs T=51 under workloads.make_parameters at B = 1024 and 8192 (--quick: a sixteenth of each batch), P = 20 periods of
one control step, sigma_x = 1e-3, warm duals. Both routes start from the same solved state (trajectory, parameters, duals and
penalties written back) and are timed with the wall clock around the whole loop, alternating, --reps times each after one warm-up:
  device  mpc_run_(P, 1)                                   one enqueue, one synchronise
  host    per period: get_trajectory, the plant on the host (x̄_1 plus a splitmix64 / Box-Muller disturbance, as examples/mpc_warm.c
          forms it), shift_horizon_(1, x1), shift_duals_(1), solve_warm_ — entry points that exist without ilqr_plant_step, so this
          route also runs on a build that lacks it (--host-only)
Reported per route: the median and the range of the time per period, and the warm re-solve's own time per period (the handle's
HIP-event timing: the solve launches only). The two plants draw different disturbances of the same size: the routes are compared
on time, not on numbers.

    python tools/mpc_run_time.py [--reps 5] [--quick] [--host-only]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, SIGMA = 20, 1.0e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of every batch (smoke run of the tool itself)")
    ap.add_argument("--host-only", action="store_true", help="the host-stepped route alone (a build without ilqr_mpc_run)")
    a = ap.parse_args()
    from ilqr_amd_loader import load_package
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("mpc_run_time.py needs a HIP device")
    cfg = "car_obs"
    print("%-8s %5s %5s %-7s %14s %10s %10s %16s" % ("model", "T", "B", "route", "median ms/per.", "min", "max", "solve ms/period"))
    for batch in (1024, 8192):
        B = max(1, batch // 16) if a.quick else batch
        model, T, x1, ub = pkg.workloads.make_inputs(cfg, B)
        w = pkg.workloads.make_parameters(cfg, B)
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.set_parameters_(w)
        sol.initialize_rollout_(x1, ub)
        sol.solve_()
        xb, ubs = sol.get_trajectory()
        lam, rho = sol.buffer("constraint_dual"), sol.buffer("constraint_penalty")
        rng = np.random.default_rng(20261019)

        def restore():
            sol.set_parameters_(w)
            sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ubs)
            sol.set_buffer("constraint_dual", lam); sol.set_buffer("constraint_penalty", rho)
            sol.initialize_rollout_(xb[:, 0], ubs)
            sol.timing_reset()

        def device():
            sol.mpc_run_(P, 1, sigma_x=SIGMA, seed=1)

        def host():
            for _ in range(P):
                x, _ = sol.get_trajectory()
                sol.shift_horizon_(1, x1=x[:, 1] + SIGMA * rng.standard_normal((B, sol.nx)))
                sol.shift_duals_(1)
                sol.solve_warm_()

        routes = (("host", host),) if a.host_only else (("device", device), ("host", host))
        ms, solve = {n: [] for n, _ in routes}, {}
        for rep in range(a.reps + 1):                    # repetition 0 warms both routes up
            for name, fn in routes:
                restore()
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3 / P
                if rep:
                    ms[name].append(dt)
                solve[name] = sol.timing()[0]
        for name, _ in routes:
            v = np.array(ms[name])
            print("%-8s %5d %5d %-7s %14.3f %10.3f %10.3f %16.3f" % (model, T, B, name, np.median(v), v.min(), v.max(), solve[name]), flush=True)
        if not a.host_only:
            print("         B=%d: host / device = %.2f (median time per period)" % (B, np.median(ms["host"]) / np.median(ms["device"])), flush=True)
        sol.close()


if __name__ == "__main__":
    main()
