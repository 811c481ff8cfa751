"""Cold against warm re-solve after a one-step receding-horizon shift, in the same process.

Workload: car_obs T=51 under workloads.make_parameters at B = 1024 and 8192 (--quick: a sixteenth of each batch). One handle is solved
once; then, alternating, --reps times each after one warm-up of each, every repetition from that same solved state (trajectory,
parameters, duals and penalties written back):
  cold   shift_horizon_(1), solve_                        λ ← 0, ρ ← ρ0 as the reference opens every constrained solve
  warm   shift_horizon_(1), shift_duals_(1), solve_warm_  the duals and penalties of the first solve, moved along (hold, keep)
Reported per route: the median and the range of the solve's time over the repetitions — the handle's HIP-event timing, launches of
the solve only —, the mean and the maximum of outer_iterations and of iterations over the batch, the share of instances that end
within constraint_tolerance, and the time of the dual shift itself.

    python tools/warm_duals_time.py [--reps 7] [--quick]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of every batch (smoke run of the tool itself)")
    a = ap.parse_args()
    from ilqr_amd_loader import load_package
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("warm_duals_time.py needs a HIP device")
    cfg = "car_obs"
    print("%-8s %5s %5s %-6s %-10s %10s %10s %10s %12s %12s %8s" % ("model", "T", "B", "route", "kernel", "median ms", "min ms", "max ms",
                                                                    "outer mean/max", "inner mean/max", "within"))
    for batch in (1024, 8192):
        B = max(1, batch // 16) if a.quick else batch
        model, T, x1, ub = pkg.workloads.make_inputs(cfg, B)
        w = pkg.workloads.make_parameters(cfg, B)
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.set_parameters_(w)
        sol.initialize_rollout_(x1, ub)
        sol.solve_()
        first = sol.stats()
        xb, ubs = sol.get_trajectory()
        lam, rho = sol.buffer("constraint_dual"), sol.buffer("constraint_penalty")
        tol = sol.options.constraint_tolerance
        shift_ms = []

        def run(warm):
            sol.set_parameters_(w)
            sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ubs)
            sol.set_buffer("constraint_dual", lam); sol.set_buffer("constraint_penalty", rho)
            sol.shift_horizon_(1)
            if warm:
                t0 = time.perf_counter()
                sol.shift_duals_(1)
                shift_ms.append((time.perf_counter() - t0) * 1e3)
            sol.timing_reset()
            sol.solve_warm_() if warm else sol.solve_()
            return sol.timing()[0], sol.stats()

        routes = (("cold", False), ("warm", True))
        for _, warm in routes:
            run(warm)                                    # warm-up of both routes at this shape
        ms = {name: [] for name, _ in routes}
        st = {}
        for _ in range(a.reps):                          # alternating: other work shares the machine
            for name, warm in routes:
                t, st[name] = run(warm)
                ms[name].append(t)
        print("%-8s %5d %5d first solve: outer %.2f / %d, inner %.1f / %d" % (model, T, B, first["outer_iterations"].mean(),
              first["outer_iterations"].max(), first["iterations"].mean(), first["iterations"].max()), flush=True)
        for name, _ in routes:
            v, s = np.array(ms[name]), st[name]
            print("%-8s %5d %5d %-6s %-10s %10.3f %10.3f %10.3f %7.2f / %-4d %7.1f / %-4d %7.1f%%"
                  % (model, T, B, name, sol.resolved_kernel_variant(), np.median(v), v.min(), v.max(), s["outer_iterations"].mean(),
                     s["outer_iterations"].max(), s["iterations"].mean(), s["iterations"].max(), 100.0 * (s["max_violation"] <= tol).mean()), flush=True)
        print("         B=%d: cold / warm = %.2f (median solve time); shift_duals_ (host form, with its synchronise) median %.3f ms"
              % (B, np.median(ms["cold"]) / np.median(ms["warm"]), np.median(shift_ms)), flush=True)
        sol.close()


if __name__ == "__main__":
    main()
