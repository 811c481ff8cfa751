"""A period of ilqr_mpc_run_preview, with and without scoring, against ilqr_mpc_run on the same inputs, in the same process; and the
score kernel's own time.

Workload: car_obs T=51 under workloads.make_parameters at B = 1024 and 8192 (--quick: a sixteenth of each batch), P = 20 periods of
one control step, sigma_x = 1e-3, warm duals — the workload of tools/mpc_run_time.py. Every route starts from the same solved state
(trajectory, parameters, duals and penalties written back) and is timed with the wall clock around the whole loop, the routes
alternating, --reps times each after one warm-up:
  run       mpc_run_(P, 1)                                     ilqr_mpc_run: what the parent commit has (run this tool's `run` route
                                                               there, --run-only, for the figure of that build)
  preview   mpc_run_(P, 1, w_preview)                          the shift fed k rows per period: no launch more than `run`
  scored    mpc_run_(P, 1, w_preview, score=True)              one launch of plant_score_kernel more per period
Reported per route: the median and the range of the time per period. The preview holds the handle's own last parameter row, so the
three routes solve the same problems and differ in the loop's own work alone. The score kernel's own time: HIP events around
--score-reps back-to-back launches of ilqr_plant_score_device on device arrays of one period (B elements: launch latency) and of
P periods (B·P elements).

    python tools/mpc_preview_time.py [--reps 5] [--quick] [--run-only]
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
    ap.add_argument("--score-reps", type=int, default=200)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of every batch (smoke run of the tool itself)")
    ap.add_argument("--run-only", action="store_true", help="ilqr_mpc_run alone (a build without ilqr_mpc_run_preview)")
    a = ap.parse_args()
    import torch
    from ilqr_amd_loader import load_package
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("mpc_preview_time.py needs a HIP device")
    cfg = "car_obs"
    print("%-8s %5s %5s %-8s %14s %10s %10s" % ("model", "T", "B", "route", "median ms/per.", "min", "max"))
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
        held = np.ascontiguousarray(np.repeat(w[:, -1:], P, axis=1))          # what the shift would hold anyway

        def restore():
            sol.set_parameters_(w)
            sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ubs)
            sol.set_buffer("constraint_dual", lam); sol.set_buffer("constraint_penalty", rho)
            sol.initialize_rollout_(xb[:, 0], ubs)

        routes = [("run", lambda: sol.mpc_run_(P, 1, sigma_x=SIGMA, seed=1))]
        if not a.run_only:
            routes += [("preview", lambda: sol.mpc_run_(P, 1, sigma_x=SIGMA, seed=1, w_preview=held)),
                       ("scored", lambda: sol.mpc_run_(P, 1, sigma_x=SIGMA, seed=1, w_preview=held, score=True))]
        ms = {n: [] for n, _ in routes}
        for rep in range(a.reps + 1):                    # repetition 0 warms every route up
            for name, fn in routes:
                restore()
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3 / P
                if rep:
                    ms[name].append(dt)
        for name, _ in routes:
            v = np.array(ms[name])
            print("%-8s %5d %5d %-8s %14.3f %10.3f %10.3f" % (model, T, B, name, np.median(v), v.min(), v.max()), flush=True)
        if not a.run_only:
            base = np.median(ms["run"])
            print("         B=%d: preview / run = %.3f, scored / run = %.3f (median time per period)"
                  % (B, np.median(ms["preview"]) / base, np.median(ms["scored"]) / base), flush=True)
            # the kernel alone: events on the handle's stream around back-to-back launches
            restore()
            stream = torch.cuda.ExternalStream(sol.stream_ptr())
            for k in (1, P):
                x = torch.zeros((B, k + 1, sol.nx), dtype=torch.float64, device="cuda")
                u = torch.zeros((B, k, sol.nu), dtype=torch.float64, device="cuda")
                cost, viol = (torch.empty((B, k), dtype=torch.float64, device="cuda") for _ in range(2))
                torch.cuda.synchronize()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                for timed in (False, True):
                    with torch.cuda.stream(stream):
                        ev[0].record()
                        for _ in range(a.score_reps):
                            sol.plant_score_device_(k, x.data_ptr(), u.data_ptr(), cost.data_ptr(), viol.data_ptr())
                        ev[1].record()
                    sol.synchronize()
                print("         B=%d: plant_score_kernel, %d element(s) per instance: %.2f us per launch (%d back-to-back launches)"
                      % (B, k, ev[0].elapsed_time(ev[1]) * 1e3 / a.score_reps, a.score_reps), flush=True)
        sol.close()


if __name__ == "__main__":
    main()
