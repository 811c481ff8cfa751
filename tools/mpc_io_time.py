"""Time of one control period of the device MPC loop with and without the seam between plant and controller, in the same process.

Workload: car_obs T=51, B=1024, 8 periods of one plant step each, warm re-solves, plant feedback, sigma_x = 1e-3, previewed parameters
and scores (ilqr_mpc_run_preview's full path). Routes, alternating, --reps times each after one warm-up of each; before every run the
handle is reset and solved from the same inputs (untimed), so that every run does the same work:
  null io            Solver.mpc_run_(w_preview, score=True): ilqr_mpc_run_preview — the path a null ilqr_plant_io takes
  limits + noise d0  the same with u_min, u_max = ∓4.9 and sigma_y = 1e-3 (ilqr_mpc_run_io, delay 0): one measurement launch and one
                     strided copy of y_cl more per period
  limits + noise d1  delay 1: one measurement and one prediction launch (the plant kernel without noise and outputs) more per period
Host clock around the call, which enqueues everything once and ends in its one stream synchronise; reported per period (total /
periods): the median and the range over the repetitions, in milliseconds. A library without ilqr_mpc_run_io (an older build named by
ILQR_LIB) runs the first route only: that is the A side of a comparison against it.

    python tools/mpc_io_time.py [--reps 7] [--batch 1024] [--periods 8] [--quick]
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--periods", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the batch (smoke run of the tool itself)")
    a = ap.parse_args()
    from ilqr_amd_loader import load_package
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("mpc_io_time.py needs a HIP device")
    B, P = (a.batch // 16 if a.quick else a.batch), a.periods
    model, T, x1, ub = pkg.workloads.make_inputs("car_obs", B)
    w = pkg.workloads.make_parameters("car_obs", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    nu, nx = sol.nu, sol.nx
    w_preview = np.ascontiguousarray(np.repeat(w[:, -1:], P, axis=1))
    base = dict(plant_feedback=True, sigma_x=np.full(nx, 1.0e-3), seed=7, w_preview=w_preview, score=True)
    seam = dict(u_min=np.full(nu, -4.9), u_max=np.full(nu, 4.9), sigma_y=np.full(nx, 1.0e-3))
    routes = [("null io", {})]
    if hasattr(pkg._ffi.lib(), "ilqr_mpc_run_io") and hasattr(pkg.Solver, "plant_measure_"):
        routes += [("limits + noise d0", dict(seam, delay=0)), ("limits + noise d1", dict(seam, delay=1))]

    def run(kw):
        sol.reset_()
        sol.set_parameters_(w)
        sol.initialize_rollout_(x1, ub)
        sol.solve_()
        t0 = time.perf_counter()
        res = sol.mpc_run_(P, 1, **base, **kw)
        ms = (time.perf_counter() - t0) * 1e3 / P
        assert (res.first_nonfinite == -1).all()
        return ms, res

    for _, kw in routes:
        run(kw)
    times = {name: [] for name, _ in routes}
    last = {}
    for _ in range(a.reps):
        for name, kw in routes:
            ms, last[name] = run(kw)
            times[name].append(ms)
    print("%-8s %4s %5s %7s  %-18s %10s %10s %10s" % ("model", "T", "B", "periods", "route", "median ms", "min ms", "max ms"))
    for name, _ in routes:
        t = np.array(times[name])
        print("%-8s %4d %5d %7d  %-18s %10.3f %10.3f %10.3f" % (model, T, B, P, name, np.median(t), t.min(), t.max()))
    for name, res in last.items():
        extra = "" if getattr(res, "saturated", None) is None else ", %d saturated" % int(res.saturated.sum())
        print("%-18s mean inner iterations per re-solve %.2f, mean realised stage cost %.6f%s"
              % (name, res.log["iterations"].mean(), res.cl_cost.mean(), extra))
    sol.close()


if __name__ == "__main__":
    main()
