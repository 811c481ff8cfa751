#!/usr/bin/env python3
"""Time the linear sensor of the MPC loop: per call, ilqr_estimate_update_linear_device and ilqr_plant_measure_linear_device on device
arrays against the selection update ilqr_estimate_update_device and ilqr_plant_measure_device of the same model and batch; and per
period inside the loop, mpc_run_ with estimator=dict(H=...) against estimator=dict(measured=...), for acrobot and synth32.

    python tools/sensor_time.py [--batch 1024] [--calls 50] [--periods 10] [--horizon 51]

The sensor has ny = nx + 1 rows (the identity and one combination), the selection filter measures every component. Prints one JSON
line per model: microseconds per call (wall clock around a stream synchronise, the median over the calls after a warm-up call) and
milliseconds per period of the two loops. Numbers belong into DESIGN_LOG.md with the command that produced them."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilqr_amd_loader import load_package  # noqa: E402


def timed(sol, fn, calls):
    t = []
    for i in range(calls + 1):
        sol.synchronize()
        t0 = time.perf_counter()
        fn()
        sol.synchronize()
        if i > 0:
            t.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--periods", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=51)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    for name, config in (("acrobot", "acrobot51"), ("synth32", "synth32")):
        sol = pkg.Solver(model=name, horizon=a.horizon, batch=a.batch, options=pkg.Options(verbose=0))
        _, _, x1, ub = pkg.workloads.make_inputs(config, a.batch)
        sol.initialize_rollout_(x1, np.ascontiguousarray(ub[:, :a.horizon - 1]))
        sol.solve_()
        n = sol.nx
        ny = n + 1
        H = np.concatenate([np.eye(n), np.full((1, n), 1.0 / n)])
        P0 = np.stack([1e-2 * np.eye(n)] * a.batch)
        q, r, rl = np.full(n, 1e-6), np.full(n, 1e-3), np.full(ny, 1e-3)
        dev = torch.device("cuda:0")
        with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
            xh = torch.from_numpy(sol.get_trajectory()[0][:, 0].copy()).to(dev)
            P = torch.from_numpy(P0).to(dev)
            y = xh.clone()
            yl = torch.zeros(a.batch, ny, dtype=torch.float64, device=dev)
            dH = torch.from_numpy(H).to(dev)
        torch.cuda.synchronize()
        out = dict(model=name, batch=a.batch, ny=ny, horizon=a.horizon, calls=a.calls, periods=a.periods)
        out["measure_us"] = timed(sol, lambda: sol.plant_measure_device_(xh.data_ptr(), y.data_ptr(), sigma_y=np.full(n, 1e-3)), a.calls)
        out["measure_linear_us"] = timed(sol, lambda: sol.plant_measure_linear_device_(xh.data_ptr(), yl.data_ptr(), dH.data_ptr(), ny, sigma_y=np.full(ny, 1e-3)), a.calls)
        out["update_us"] = timed(sol, lambda: sol.estimate_update_device_(xh.data_ptr(), P.data_ptr(), y.data_ptr(), r), a.calls)
        out["update_linear_us"] = timed(sol, lambda: sol.estimate_update_linear_device_(xh.data_ptr(), P.data_ptr(), yl.data_ptr(), dH.data_ptr(), ny, rl),
                                        a.calls)
        for key, est in (("loop_selection_ms", dict(r=r, q=q, P0=P0)), ("loop_linear_ms", dict(H=H, r=rl, q=q, P0=P0))):
            sol.initialize_rollout_(x1, np.ascontiguousarray(ub[:, :a.horizon - 1]))
            sol.solve_()
            sol.mpc_run_(1, 1, estimator=est)                                  # warm-up: the buffers of the run exist
            sol.synchronize()
            t0 = time.perf_counter()
            sol.mpc_run_(a.periods, 1, estimator=est)
            out[key] = 1e3 * (time.perf_counter() - t0) / a.periods
        print(json.dumps(out))
        sol.close()


if __name__ == "__main__":
    main()
