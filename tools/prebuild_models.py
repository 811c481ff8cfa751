"""Compile the C-source model modules and the sensor modules the examples and the GPU tests use (ilqr_compile_model, ilqr_compile_sensor: hipcc as a child process, no GPU
needed) into iterativelqr.jl_amd/lib/models/, the library's module cache — so that a GPU box that receives the tree finds them
built (the dense 64 x 16 module alone takes a minute). Called by __graft_entry__.build()."""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Src(C.Structure):
    _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]


def main(verbose=True):
    from ilqr_amd_loader import load_package
    pkg = load_package()
    L = pkg._ffi.lib()
    ex = lambda f: open(os.path.join(ROOT, "examples", f), "rb").read()
    jobs = [  # (name, dims, source, probe) exactly as tests/test_gpu_parity.py and tools/c_model_bench.py pass them
        (b"synth32_c", (32, 8, 0, 16, 0, (1 << 16) - 1, 0), ex("synth32_model.c"), True),
        (b"synth32_c", (32, 8, 0, 16, 0, (1 << 16) - 1, 0), ex("synth32_model.c"), False),
        (b"synth64_c", (64, 16, 0, 32, 0, (1 << 32) - 1, 0), pkg.models.synth_c_source(64, 16).encode(), True),
        (b"synth64_c", (64, 16, 0, 32, 0, (1 << 32) - 1, 0), pkg.models.synth_c_source(64, 16).encode(), False),
        (b"synth12_t", (12, 5, 0, 10, 3, (1 << 10) - 1, 0), ex("synth12_model.c"), True),
    ]
    # the coupled-Hessian family of tests/coupled_problem.py: (12, 5) as C callables here, every size through the symbolic generator
    # below. The family is the tests' own: a tree without that file builds everything else, and the tests compile on demand
    CP = None
    if os.path.exists(os.path.join(ROOT, "tests", "coupled_problem.py")):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import coupled_problem as CP
        for probe in (True, False):
            jobs.append((b"coupled12_c", (12, 5, 0, 12, 0, (1 << 12) - 1, 0), CP.c_source(pkg, 12, 5).encode(), probe))
    # the coupled-dynamics family of tests/coupled_dynamics.py the same way: (12, 5) and (17, 3) as C callables, probed and dense
    CD = None
    if os.path.exists(os.path.join(ROOT, "tests", "coupled_dynamics.py")):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import coupled_dynamics as CD
        for n, m in CD.C_SIZES:
            for probe in (True, False):
                jobs.append(((CD.name(n, m) + "_c").encode(), CD.c_dims(n, m), CD.c_source(pkg, n, m).encode(), probe))
    old = os.environ.get("ILQR_NO_STRUCTURE_PROBE")
    try:
        for name, dims, text, probe in jobs:
            if probe:
                os.environ.pop("ILQR_NO_STRUCTURE_PROBE", None)
            else:
                os.environ["ILQR_NO_STRUCTURE_PROBE"] = "1"
            ms = Src(name, *dims, text)
            reg = C.create_string_buffer(128); path = C.create_string_buffer(1024)
            rc = L.ilqr_compile_model(C.byref(ms), reg, 128, path, 1024)
            if rc != 0:
                raise RuntimeError("ilqr_compile_model(%s, probe=%s): %s" % (name.decode(), probe, L.ilqr_last_error().decode()[-600:]))
            if verbose:
                print("model module %s (%s tables): %s" % (reg.value.decode(), "probed" if probe else "dense", os.path.basename(path.value.decode())))
        # per-step objects through ilqr_compile_model_stages (the GPU tests' ragged_c and car_tv_c; horizon 41 / 51 as there)
        F = pkg._ffi
        for name, (kinds, src) in ((b"ragged_c", pkg.models.ragged_c_stages(41)), (b"car_tv_c", pkg.lowering.c_stage_sources(*pkg.models.car_tv(51)))):
            cap = kinds.horizon * (kinds.n_dynamics + kinds.n_costs + kinds.n_constraints)
            plan, sel = F.StagePlan(), (C.c_double * max(cap, 1))()
            reg = C.create_string_buffer(160); path = C.create_string_buffer(1024)
            rc = L.ilqr_compile_model_stages(name, C.byref(kinds), src.encode(), C.byref(plan), sel, cap, None, None, reg, 160, path, 1024)
            if rc != 0:
                raise RuntimeError("ilqr_compile_model_stages(%s): %s" % (name.decode(), L.ilqr_last_error().decode()[-600:]))
            if verbose:
                print("model module %s (per-step kinds): %s" % (reg.value.decode(), os.path.basename(path.value.decode())))
        # symbolic models (api.compile_model, as Solver(dynamics, costs, constraints) does): hipcc children, a few at a time
        from concurrent.futures import ThreadPoolExecutor
        lowered = []
        for n, m, T, con in sorted(set((n, m, 11, con) for n, m, _, con in (CP.CASES if CP else []))):       # (the horizon does not enter the module)
            dyn, costs, cons, name = CP.product_problem(pkg, n, m, T, con)
            low = pkg.lowering.lower(dyn, costs, cons)
            lowered.append((name, low["dynamics"], low["cost_stage"], low["cost_term"], low["con_stage"], low["con_term"]))
        for n, m in (CD.SIZES if CD else []):
            dyn, costs, cons, name = CD.product_problem(pkg, n, m)
            low = pkg.lowering.lower(dyn, costs, cons)
            lowered.append((name, low["dynamics"], low["cost_stage"], low["cost_term"], low["con_stage"], low["con_term"]))
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
            for reg, path in pool.map(lambda job: pkg.api.compile_model(*job), lowered):
                if verbose:
                    print("model module %s (symbolic): %s" % (reg, os.path.basename(path)))
        # sensor modules (ilqr_compile_sensor): the example's hand-written one, and the sensors of tests/sensor_nl_ref.py through the
        # symbolic generator. The family is the tests' own: a tree without that file builds everything else
        import re
        literal = ex("mpc_range.c").decode().split("/* SENSOR SOURCE BEGIN */")[1].split("/* SENSOR SOURCE END */")[0]
        text = "".join(line.replace("\\n", "\n") for line in re.findall(r'"(.*)"', literal))            # the C string, line by line
        reg, path = pkg.compile_sensor_source("range2", 3, 2, 4, text)
        if verbose:
            print("sensor module %s (C source): %s" % (reg, os.path.basename(path)))
        if os.path.exists(os.path.join(ROOT, "tests", "sensor_nl_ref.py")):
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import sensor_nl_ref as NL
            for key in NL.SENSORS:                 # (one after the other: a few seconds each, and the registry is not written from two threads)
                reg = NL.compiled(pkg, key)
                if verbose:
                    print("sensor module %s (symbolic)" % reg)
            reg = NL.compiled_readback(pkg)
            if verbose:
                print("sensor module %s (C source)" % reg)
            # the size sweep's and the function family's sensors (tests/sensor_nl_sizes.py) the same way; a dense switch of 64 cases
            # among them
            if os.path.exists(os.path.join(ROOT, "tests", "sensor_nl_sizes.py")):
                import sensor_nl_sizes as NZ
                for key in NZ.KEYS:
                    reg = NL.compiled(pkg, key)
                    if verbose:
                        print("sensor module %s (symbolic)" % reg)
    finally:
        if old is None:
            os.environ.pop("ILQR_NO_STRUCTURE_PROBE", None)
        else:
            os.environ["ILQR_NO_STRUCTURE_PROBE"] = old


if __name__ == "__main__":
    main()
