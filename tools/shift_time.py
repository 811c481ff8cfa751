"""Time of ilqr_shift_horizon against the host round trip it replaces, in the same process.

Workloads: acrobot T=101 at B = 1024 and 8192, synth12 T=101 at B = 1024 (--quick: a sixteenth of each batch). Per workload one
solved handle; per route, alternating, --reps times each after one warm-up of each, every repetition from the same solved state:
  shift open (device)     Solver.shift_horizon_device_(1, x1 resident): device events on the handle's stream
  shift closed (device)   the same with feedback=True
  shift open (host)       Solver.shift_horizon_(1, x1): one copy of [B][nx], the kernels, a stream synchronise; host clock
  shift closed (host)     the same with feedback=True
  host round trip         get_trajectory + get_policy + the shift in numpy + (models with parameters: set_parameters_) +
                          initialize_rollout_; host clock. The closed-loop warm start is not expressible on this route without a
                          host-side rollout of the model, so it is the open-loop shift that is timed.
Reported: the median and the range over the repetitions in milliseconds, and that the open-loop routes install the same state.

    python tools/shift_time.py [--reps 7] [--quick]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="a sixteenth of every batch (smoke run of the tool itself)")
    a = ap.parse_args()
    import torch
    from ilqr_amd_loader import load_package
    import shift_ref as R
    pkg = load_package()
    if pkg._ffi.lib().ilqr_device_count() < 1:
        raise SystemExit("shift_time.py needs a HIP device")
    dev = torch.device("cuda:0")
    print("%-8s %5s %5s %-22s %12s %12s %12s" % ("model", "T", "B", "route", "median ms", "min ms", "max ms"))
    for cfg, batch in (("acrobot", 1024), ("acrobot", 8192), ("synth12", 1024)):
        B = max(1, batch // 16) if a.quick else batch
        model, T, x1_0, ub_0 = pkg.workloads.make_inputs(cfg, B)
        opts = pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(cfg, {}))
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=opts)
        sol.initialize_rollout_(x1_0, ub_0)
        sol.solve_()
        xb, ub = sol.get_trajectory()
        x1 = xb[:, 1] + 0.01 * np.random.default_rng(1).standard_normal(xb[:, 1].shape)
        stream = torch.cuda.ExternalStream(sol.stream_ptr())
        d_x1 = torch.from_numpy(x1).to(dev)
        torch.cuda.synchronize()
        state = {}

        def restore():
            sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ub)

        def device(feedback):
            def f():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                sol.shift_horizon_device_(1, d_x1.data_ptr(), feedback=feedback)
                e1.record(stream)
                sol.synchronize()
                return e0.elapsed_time(e1)
            return f

        def host(feedback):
            def f():
                t0 = time.perf_counter()
                sol.shift_horizon_(1, x1=x1, feedback=feedback)
                ms = (time.perf_counter() - t0) * 1e3
                if not feedback:
                    state["new"] = sol.get_trajectory()
                return ms
            return f

        def round_trip():
            t0 = time.perf_counter()
            xs, us = sol.get_trajectory()
            sol.get_policy()
            up = np.empty_like(us)
            up[:, :-1] = us[:, 1:]; up[:, -1] = us[:, -1]
            if sol.num_user_parameter > 0:
                w = sol.buffer("parameters").reshape(B, T, -1)
                sol.set_parameters_(np.concatenate([w[:, 1:], w[:, -1:]], axis=1))
            sol.initialize_rollout_(x1, up)
            ms = (time.perf_counter() - t0) * 1e3
            state["old"] = sol.get_trajectory()
            return ms

        routes = (("shift open (device)", device(False)), ("shift closed (device)", device(True)), ("shift open (host)", host(False)),
                  ("shift closed (host)", host(True)), ("host round trip", round_trip))
        for _, f in routes:
            restore(); f()                              # warm-up of every route at this shape
        ms = {name: [] for name, _ in routes}
        for _ in range(a.reps):                         # alternating: other work shares the machine
            for name, f in routes:
                restore()
                ms[name].append(f())
        same = all(np.array_equal(p, q) for p, q in zip(state["new"], state["old"]))
        for name, _ in routes:
            v = np.array(ms[name])
            print("%-8s %5d %5d %-22s %12.3f %12.3f %12.3f" % (model, T, B, name, np.median(v), v.min(), v.max()), flush=True)
        med = {name: float(np.median(ms[name])) for name in ms}
        print("         B=%d: host round trip / shift open (device) = %.1f, / shift open (host) = %.1f; the open-loop routes install %s state"
              % (B, med["host round trip"] / med["shift open (device)"], med["host round trip"] / med["shift open (host)"],
                 "the same" if same else "A DIFFERENT"), flush=True)
        sol.close()


if __name__ == "__main__":
    main()
