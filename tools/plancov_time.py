#!/usr/bin/env python3
"""Time the plan covariance against the re-solve it would sit beside in a control period: ilqr_plan_covariance_device over the whole
horizon on device arrays (sdiag, udiag and P_out asked for), and shift + warm solve of the same period, for acrobot and synth32.

    python tools/plancov_time.py [--batch 1024] [--steps 1] [--periods 20] [--horizon 51]

Prints one JSON line per model: milliseconds per period of the covariance and of the re-solve (wall clock around a stream
synchronise, the median over the periods after a warm-up period), and their ratio. Numbers belong into DESIGN_LOG.md with the
command that produced them."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilqr_amd_loader import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--periods", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=51)
    a = ap.parse_args()
    import torch
    pkg = load_package()
    for name, config in (("acrobot", "acrobot51"), ("synth32", "synth32")):
        sol = pkg.Solver(model=name, horizon=a.horizon, batch=a.batch, options=pkg.Options(verbose=0))
        _, _, x1, ub = pkg.workloads.make_inputs(config, a.batch)
        sol.initialize_rollout_(x1, np.ascontiguousarray(ub[:, :a.horizon - 1]))
        sol.solve_()
        n, m, S = sol.nx, sol.nu, a.horizon - 1
        dev = torch.device("cuda:0")
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
            xh = torch.from_numpy(sol.get_trajectory()[0][:, 0].copy()).to(dev)
            P0 = torch.from_numpy(np.stack([1e-2 * np.eye(n)] * a.batch)).to(dev)
            sd, ud, PS = torch.zeros(a.batch, S + 1, n, **f64), torch.zeros(a.batch, S, m, **f64), torch.zeros(a.batch, n, n, **f64)
        torch.cuda.synchronize()
        q = np.full(n, 1e-6)
        t_cov, t_solve = [], []
        for p in range(a.periods + 1):
            sol.synchronize()
            t0 = time.perf_counter()
            sol.plan_covariance_device_(P0.data_ptr(), feedback=True, q=q, d_sdiag_ptr=sd.data_ptr(), d_udiag_ptr=ud.data_ptr(), d_P_out_ptr=PS.data_ptr())
            sol.synchronize()
            t1 = time.perf_counter()
            sol.shift_horizon_device_(a.steps, xh.data_ptr())
            sol.shift_duals_(a.steps)
            sol.solve_warm_()
            sol.synchronize()
            t2 = time.perf_counter()
            if p > 0:
                t_cov.append(1e3 * (t1 - t0)); t_solve.append(1e3 * (t2 - t1))
        c, s = float(np.median(t_cov)), float(np.median(t_solve))
        print(json.dumps(dict(model=name, batch=a.batch, steps=a.steps, horizon=a.horizon, periods=a.periods, plan_covariance_ms=c, resolve_ms=s,
                              plan_covariance_over_resolve=c / s)))
        sol.close()


if __name__ == "__main__":
    main()
