#!/usr/bin/env python3
"""Time the compiled nonlinear sensor of the MPC loop: per call on device arrays, ilqr_sensor_linearise_device,
ilqr_plant_measure_sensor_device and ilqr_estimate_update_sensor_device (iterations 1 and 3) against
ilqr_estimate_update_linear_device fed a per-instance H of the same shape — what the composite call adds is the linearisation.

    python tools/sensor_nl_time.py [--batch 1024] [--calls 50] [--horizon 11] [--compile-only | --resources]

Two sensors: two beacon ranges on car_obs (nx = 3, ny = 2, ns = 4) and a 33-row sensor on synth32 (nx = 32: 32 sparse rows, one
dense). Prints one JSON line per sensor: microseconds per call (wall clock around a stream synchronise, the median over the calls
after a warm-up call), the bytes of H one linearisation stores and the rate that makes. --compile-only builds the two sensor modules
into the module cache and stops (no GPU needed). --resources (no GPU needed either) wraps every sensor's source as
ilqr_compile_sensor does, compiles the device code alone with the compiler's resource-usage remarks on and prints one line per kernel
instantiation — VGPRs, SGPRs, scratch bytes per lane, LDS bytes per workgroup, occupancy — for the two sensors here, the example's
(examples/mpc_range.c) and, where tests/sensor_nl_ref.py exists, the test sensors. Numbers belong into DESIGN_LOG.md with the command
that produced them."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilqr_amd_loader import load_package  # noqa: E402


def beacons(x, s):
    import sympy as sp
    return [sp.sqrt((x[0] - s[0]) ** 2 + (x[1] - s[1]) ** 2), sp.sqrt((x[0] - s[2]) ** 2 + (x[1] - s[3]) ** 2)]


def rows33(x, s):
    import sympy as sp
    return [sp.sin(x[j]) + s[0] * x[(j + 1) % 32] * x[(j + 5) % 32] for j in range(32)] + [sp.tanh(sum(x) / 10)]


SENSORS = (("time_beacons", beacons, "car_obs", "car_obs", 3, 4, np.array([3.0, 2.0, -2.0, 3.0])),
           ("time_rows33", rows33, "synth32", "synth32", 32, 1, np.array([0.5])))


WRAP = """#include "ilqr_sensor_adapter.hpp"
#pragma clang fp contract(off)
namespace user_t {
%s
}
struct Fns_t {
    ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s) { user_t::sensor_row(j, y, dydx, x, s); }
};
struct Sensor_t : ilqr::AdaptedSensor<Fns_t, %d, %d, %d> {
    static constexpr const char* NAME = "t";
};
ILQR_DEFINE_SENSOR(Sensor_t)
"""


def resources(pkg):
    import re
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jobs = []
    for key, h, _, _, nx, ns, _ in SENSORS:
        ny, src = pkg.codegen.generate_sensor_source(key, h, nx, ns)
        jobs.append((key, nx, ny, ns, src))
    lit = open(os.path.join(root, "examples", "mpc_range.c")).read().split("/* SENSOR SOURCE BEGIN */")[1].split("/* SENSOR SOURCE END */")[0]
    jobs.append(("range2 (examples/mpc_range.c)", 3, 2, 4, "".join(ln.replace("\\n", "\n") for ln in re.findall(r'"(.*)"', lit))))
    if os.path.exists(os.path.join(root, "tests", "sensor_nl_ref.py")):
        sys.path.insert(0, os.path.join(root, "tests"))
        import sensor_nl_ref as NL
        for key, (_, nx, _, ns, _) in NL.SENSORS.items():
            ny, src = pkg.codegen.generate_sensor_source(key, NL.symbolic(key), nx, ns)
            jobs.append(("nl_" + key, nx, ny, ns, src))
        jobs.append(("nl_readback", 4, 2, 0, NL.READBACK_SOURCE))
        if os.path.exists(os.path.join(root, "tests", "sensor_nl_sizes.py")):
            import sensor_nl_sizes as NZ
            for key in NZ.KEYS:
                nx, _, ns = NL.dims(key)
                ny, src = pkg.codegen.generate_sensor_source(key, NL.symbolic(key), nx, ns)
                jobs.append(("nl_" + key, nx, ny, ns, src))
    fields = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    with tempfile.TemporaryDirectory() as tmp:
        for key, nx, ny, ns, src in jobs:
            hip = os.path.join(tmp, "s.hip")
            open(hip, "w").write(WRAP % (src, nx, ny, ns))
            out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form",
                                  "-Wno-unused-parameter", "-I" + pkg._ffi.CSRC, "-c", hip, "-o", os.path.join(tmp, "s.o"),
                                  "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
            for part in out.split("Function Name: ")[1:]:
                jac = "linearise" if "Lb1E" in part.split()[0] else "measure"
                vals = [re.search(re.escape(f) + r": (\d+)", part).group(1) for f in fields]
                print("%-30s nx %2d ny %2d  %-9s  VGPRs %3s  SGPRs %3s  scratch %s  LDS %5s  occupancy %s" % ((key, nx, ny, jac) + tuple(vals)))


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
    ap.add_argument("--horizon", type=int, default=11)
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    pkg = load_package()
    if a.resources:
        resources(pkg)
        return
    names = {key: pkg.compile_sensor(key, h, nx, ns)[0] for key, h, _, _, nx, ns, _ in SENSORS}
    if a.compile_only:
        print(json.dumps(names))
        return
    import torch
    for key, _, model, config, n, ns, s in SENSORS:
        sens = names[key]
        ny = pkg.sensor_dims(sens)[1]
        B = a.batch
        sol = pkg.Solver(model=model, horizon=a.horizon, batch=B, options=pkg.Options(verbose=0))
        _, _, x1, _ = pkg.workloads.make_inputs(config, B)
        dev = torch.device("cuda:0")
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
            x0 = torch.from_numpy(x1 + 0.3).to(dev)
            xh, P0 = x0.clone(), torch.from_numpy(np.stack([1e-2 * np.eye(n)] * B)).to(dev)
            P = P0.clone()
            ds = torch.from_numpy(s).to(dev)
            H, yh, y = torch.zeros(B, ny, n, **f64), torch.zeros(B, ny, **f64), torch.zeros(B, ny, **f64)
        torch.cuda.synchronize()
        r = np.full(ny, 1e-3)

        def fresh():
            with torch.cuda.stream(torch.cuda.ExternalStream(sol.stream_ptr())):
                xh.copy_(x0); P.copy_(P0)

        def update(it):
            fresh()
            sol.estimate_update_sensor_device_(xh.data_ptr(), P.data_ptr(), y.data_ptr(), sens, r, d_s_ptr=ds.data_ptr(), iterations=it)

        def linear():
            fresh()
            sol.estimate_update_linear_device_(xh.data_ptr(), P.data_ptr(), y.data_ptr(), H.data_ptr(), ny, r, per_instance_H=True, d_yhat_ptr=yh.data_ptr())

        sol.plant_measure_sensor_device_(sens, x0.data_ptr(), y.data_ptr(), d_s_ptr=ds.data_ptr(), sigma_y=np.full(ny, 1e-2), seed=1)
        out = dict(sensor=key, model=model, batch=B, nx=n, ny=ny, calls=a.calls,
                   reset_us=timed(sol, fresh, a.calls),
                   linearise_us=timed(sol, lambda: sol.sensor_linearise_device_(sens, x0.data_ptr(), H.data_ptr(), yh.data_ptr(), d_s_ptr=ds.data_ptr()), a.calls),
                   linearise_prior_us=timed(sol, lambda: sol.sensor_linearise_device_(sens, x0.data_ptr(), H.data_ptr(), yh.data_ptr(), d_s_ptr=ds.data_ptr(),
                                                                                      d_x_prior_ptr=xh.data_ptr()), a.calls),
                   measure_us=timed(sol, lambda: sol.plant_measure_sensor_device_(sens, x0.data_ptr(), y.data_ptr(), d_s_ptr=ds.data_ptr(),
                                                                                  sigma_y=np.full(ny, 1e-2), seed=1), a.calls),
                   update_linear_us=timed(sol, linear, a.calls), update_sensor_1_us=timed(sol, lambda: update(1), a.calls),
                   update_sensor_3_us=timed(sol, lambda: update(3), a.calls))
        out["H_bytes"] = B * ny * n * 8
        out["H_store_GB_per_s"] = out["H_bytes"] / (1e3 * out["linearise_us"])
        print(json.dumps(out))
        sol.close()


if __name__ == "__main__":
    main()
