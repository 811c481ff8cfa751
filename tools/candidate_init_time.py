"""Time of ilqr_initialize_rollout_candidates against the only route without it, in the same process.

Workload: acrobot T=101, B=1024, S = 16 and 256 candidates per instance (ū · scale + noise, as tests/candidates_ref.py draws them).
Per S, alternating, --reps times each after one warm-up of each:
  candidates (host)    Solver.initialize_rollout_candidates_: one copy of [B][S][T-1][nu], scoring, selection, installation; host clock
                       around the call, which ends in a stream synchronise
  candidates (device)  the device-pointer form on resident candidates, device events on the handle's stream
  S rounds             per candidate: initialize_rollout_ + the cost stage + stats on an UNCONSTRAINED handle (so the stage's merit is the
                       plain objective), then argmin on the host and one more initialize_rollout_ of the winners; host clock
Reported: the median and the range over the repetitions in milliseconds; that the two routes choose the same candidates is checked.

    python tools/candidate_init_time.py [--reps 5] [--batch 1024] [--quick]
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
    import candidates_ref as R
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("candidate_init_time.py needs a HIP device")
    B = a.batch // 16 if a.quick else a.batch
    dev = torch.device("cuda:0")
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0), constraints=False)
    old = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0), constraints=False)
    stream = torch.cuda.ExternalStream(sol.stream_ptr())
    print("%-8s %5s %5s %5s %-20s %12s %12s %12s" % ("model", "T", "B", "S", "route", "median ms", "min ms", "max ms"))
    for S in (16, 256):
        rng = np.random.default_rng(S)
        scale = 1.5 * (np.arange(S) % 16) / 15.0
        u = ub[:, None] * scale[None, :, None, None] + 0.2 * rng.standard_normal((B, S, T - 1, sol.nu))
        u[:, 0] = ub
        d_x1, d_u = torch.from_numpy(x1).to(dev), torch.from_numpy(u).to(dev)
        d_chosen = torch.empty(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        picks = {}

        def host():
            t0 = time.perf_counter()
            picks["new"] = sol.initialize_rollout_candidates_(x1, u)
            return (time.perf_counter() - t0) * 1e3

        def device():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sol.initialize_rollout_candidates_device_(S, d_x1.data_ptr(), d_u.data_ptr(), d_chosen_ptr=d_chosen.data_ptr())
            e1.record(stream)
            sol.synchronize()
            return e0.elapsed_time(e1)

        def rounds():
            t0 = time.perf_counter()
            cost = np.empty((B, S))
            for s in range(S):
                old.initialize_rollout_(x1, u[:, s])
                old.run_stage_("cost_nominal")
                cost[:, s] = old.stats()["objective"]
            best = np.array([R.select(cost[b], np.zeros(S), np.full(S, -1)) for b in range(B)])
            old.initialize_rollout_(x1, u[np.arange(B), np.maximum(best, 0)])
            picks["old"], picks["old_cost"] = best, cost
            return (time.perf_counter() - t0) * 1e3

        routes = (("candidates (host)", host), ("candidates (device)", device), ("S rounds", rounds))
        for _, f in routes:
            f()                                         # warm-up of every route at this shape
        ms = {name: [] for name, _ in routes}
        for _ in range(a.reps):                         # alternating: other work shares the machine
            for name, f in routes:
                ms[name].append(f())
        new, best = picks["new"], picks["old"]
        finite = new["first_nonfinite"] == -1           # the stage route has no non-finite mark: compare where both are defined
        same = int((new["chosen"] == best).sum())
        err = np.abs(new["cost"] - picks["old_cost"])[finite].max()
        for name, _ in routes:
            v = np.array(ms[name])
            print("%-8s %5d %5d %5d %-20s %12.3f %12.3f %12.3f" % (model, T, B, S, name, np.median(v), v.min(), v.max()), flush=True)
        print("         S=%d: %d of %d instances choose the same candidate on both routes; max |cost difference| %.2e" % (S, same, B, err), flush=True)
    sol.close(); old.close()


if __name__ == "__main__":
    main()
