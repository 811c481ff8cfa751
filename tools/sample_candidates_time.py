"""Time of ilqr_sample_rollout_candidates against the route it replaces — candidates drawn on the host and handed to
ilqr_initialize_rollout_candidates — in the same process, at the same B, S, T.

Workload: acrobot T=101, B=1024, S = 16 and 256 candidates per instance around the workload's ū, sigma = 0.2.
Per S, alternating, --reps times each after one warm-up of each:
  host candidates (host)    Solver.initialize_rollout_candidates_ on a ready [B][S][T-1][nu] host array (drawing it is NOT timed): the
                            copy, scoring, selection, installation; host clock around the call, which ends in a stream synchronise
  host candidates (device)  the device-pointer form on candidates already resident in HBM; device events on the handle's stream
  sampled (host)            Solver.sample_rollout_candidates_ (pick), scores returned, no candidates returned; host clock
  sampled (device)          the device-pointer form, no outputs; device events on the handle's stream
  sampled blend (device)    the same with mode="blend"
Reported: the median and the range over the repetitions in milliseconds. The candidates the first two routes score are the ones the
sampler draws (exported once, outside the timing), so that all routes do the same scoring work; that they choose the same
candidates is checked.

    python tools/sample_candidates_time.py [--reps 5] [--batch 1024] [--quick]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of the batch (smoke run of the tool itself)")
    a = ap.parse_args()
    import torch
    from ilqr_amd_loader import load_package
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("sample_candidates_time.py needs a HIP device")
    B = a.batch // 16 if a.quick else a.batch
    dev = torch.device("cuda:0")
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    old = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sigma, seed = np.full(sol.nu, 0.2), 1
    print("%-8s %5s %5s %5s %-26s %12s %12s %12s" % ("model", "T", "B", "S", "route", "median ms", "min ms", "max ms"))
    for S in (16, 256):
        u = sol.sample_rollout_candidates_(sigma, S, seed=seed, x1=x1, base_u=ub, return_candidates=True)["u"]
        d_x1, d_ub, d_u = torch.from_numpy(x1).to(dev), torch.from_numpy(ub).to(dev), torch.from_numpy(u).to(dev)
        d_chosen = torch.empty(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        picks = {}

        def events(handle, call):
            stream = torch.cuda.ExternalStream(handle.stream_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            handle.synchronize()
            return e0.elapsed_time(e1)

        def old_host():
            t0 = time.perf_counter()
            picks["old"] = old.initialize_rollout_candidates_(x1, u)
            return (time.perf_counter() - t0) * 1e3

        def old_device():
            return events(old, lambda: old.initialize_rollout_candidates_device_(S, d_x1.data_ptr(), d_u.data_ptr(), d_chosen_ptr=d_chosen.data_ptr()))

        def new_host():
            t0 = time.perf_counter()
            picks["new"] = sol.sample_rollout_candidates_(sigma, S, seed=seed, x1=x1, base_u=ub)
            return (time.perf_counter() - t0) * 1e3

        def new_device(mode="pick"):
            return events(sol, lambda: sol.sample_rollout_candidates_device_(sigma, S, seed=seed, mode=mode, temperature=10.0, d_x1_ptr=d_x1.data_ptr(),
                                                                             d_base_u_ptr=d_ub.data_ptr(), d_chosen_ptr=d_chosen.data_ptr()))

        routes = (("host candidates (host)", old_host), ("host candidates (device)", old_device), ("sampled (host)", new_host),
                  ("sampled (device)", new_device), ("sampled blend (device)", lambda: new_device("blend")))
        for _, f in routes:
            f()                                         # warm-up of every route at this shape
        ms = {name: [] for name, _ in routes}
        for _ in range(a.reps):                         # alternating: other work shares the machine
            for name, f in routes:
                ms[name].append(f())
        for name, _ in routes:
            v = np.array(ms[name])
            print("%-8s %5d %5d %5d %-26s %12.3f %12.3f %12.3f" % (model, T, B, S, name, np.median(v), v.min(), v.max()), flush=True)
        same = int((picks["new"]["chosen"] == picks["old"]["chosen"]).sum())
        print("         S=%d: %d of %d instances choose the same candidate on both routes; candidate array not sent: %.1f MB" %
              (S, same, B, u.nbytes / 1e6), flush=True)
    sol.close(); old.close()


if __name__ == "__main__":
    main()
