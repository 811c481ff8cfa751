"""Throughput of ilqr_rollout_policy_device: the device form, timed with events on the handle's stream.

Workloads: acrobot T=101 B=1024 and car T=51 B=4096, S = 64, 256, 1024 samples per instance, with and without trajectory output.
Per row: milliseconds per call (median of --reps), sample-steps per second (B·S·(T-1) / time) and bytes written per second
(cost, max_violation, first_nonfinite and, when asked for, x and u). Beside them: the same recursion on the CPU oracle
(orc_rollout_bang + orc_cost_bang per sample, --cpu-threads worker threads, on --cpu-samples samples and scaled per sample-step).

    python tools/policy_rollout_time.py [--reps 5] [--cpu-threads 16] [--cpu-samples 256] [--quick]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_rate(O, R, model, T, xb, ub, K, x1s, threads):
    """sample-steps per second of the oracle's recursion (ctypes releases the GIL inside the oracle's calls)"""
    def one(i):
        R.oracle_reading(O, model, T, xb, ub, K, x1s[i])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(len(x1s))))
    return len(x1s) * (T - 1) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-samples", type=int, default=256)
    ap.add_argument("--quick", action="store_true", help="a tenth of the batch (smoke run of the tool itself)")
    a = ap.parse_args()
    import torch
    from ilqr_amd_loader import load_package
    from oracle import oracle as O
    import policy_ref as R
    pkg = load_package()
    dev = torch.device("cuda:0")
    print("%-8s %5s %5s %5s %5s %10s %14s %12s %16s" % ("model", "T", "B", "S", "traj", "ms/call", "sample-steps/s", "GB/s written", "CPU oracle st/s"))
    for cfg, B in (("acrobot", 1024), ("car", 4096)):
        if a.quick:
            B //= 10
        model, T, x1, ub = pkg.workloads.make_inputs(cfg, B, generator="splitmix64")
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.initialize_rollout_(x1, ub); sol.solve_()
        xb, ubar = sol.get_trajectory()
        K, _ = sol.get_policy()
        cpu = cpu_rate(O, R, model, T, xb[0], ubar[0], K[0], R.perturbed_starts(xb[0, 0], a.cpu_samples, 0.05), a.cpu_threads)
        stream = torch.cuda.ExternalStream(sol.stream_ptr())
        for S in (64, 256, 1024):
            rng = np.random.default_rng(S)
            xs = xb[:, None, 0, :] + 0.05 * rng.standard_normal((B, S, sol.nx))
            d_x1 = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
            cost = torch.empty(B, S, dtype=torch.float64, device=dev); viol = torch.empty_like(cost)
            nf = torch.empty(B, S, dtype=torch.int32, device=dev)
            for traj in (False, True):
                dx = torch.empty(B, S, T, sol.nx, dtype=torch.float64, device=dev) if traj else None
                du = torch.empty(B, S, T - 1, sol.nu, dtype=torch.float64, device=dev) if traj else None
                torch.cuda.synchronize()

                def call():
                    sol.rollout_policy_device(S, d_x1.data_ptr(), cost.data_ptr(), d_max_violation_ptr=viol.data_ptr(),
                                              d_first_nonfinite_ptr=nf.data_ptr(), d_x_ptr=dx.data_ptr() if traj else None,
                                              d_u_ptr=du.data_ptr() if traj else None)
                call(); sol.synchronize()                       # warm-up
                ms = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream); call(); e1.record(stream)
                    sol.synchronize()
                    ms.append(e0.elapsed_time(e1))
                t = float(np.median(ms)) * 1e-3
                written = B * S * (8 + 8 + 4) + (B * S * (T * sol.nx + (T - 1) * sol.nu) * 8 if traj else 0)
                print("%-8s %5d %5d %5d %5s %10.3f %14.3e %12.2f %16.3e" % (model, T, B, S, "yes" if traj else "no", t * 1e3,
                                                                          B * S * (T - 1) / t, written / t / 1e9, cpu), flush=True)
                del dx, du
        sol.close()


if __name__ == "__main__":
    main()
