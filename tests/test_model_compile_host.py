"""The model compiler (csrc/ilqr_model_compile.cpp) is plain C++: built here with g++ next to a stub for the three things it takes
from the API unit, and checked on the host — the structure probe on examples/synth12_model.c (24 state-dependent Jacobian entries,
12 + 5 Hessian entries), the probe switched off, the probe cache (served from its .bin, a truncated one re-probed), the stage plan
of a hand-written kinds table and the source composed for it, which the probe then compiles and runs. No hipcc, no library, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iterativelqr.jl_amd", "csrc")


def test_model_compiler_on_the_host(tmp_path):
    exe = str(tmp_path / "model_compile_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "model_compile_check.cpp"),
                           os.path.join(CSRC, "ilqr_model_compile.cpp"), "-o", exe, "-ldl"])
    scratch = tmp_path / "models"
    scratch.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "ILQR_NO_STRUCTURE_PROBE"}
    out = subprocess.run([exe, os.path.join(ROOT, "examples", "synth12_model.c"), str(scratch)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d checks passed" % (len(lines) - 1) and len(lines) > 25


def test_model_compiler_needs_no_rocm_header():
    """g++ with no ROCm include path and every warning on: no diagnostics"""
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", os.path.join(CSRC, "ilqr_model_compile.cpp")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and out.stdout == b"", out.stdout.decode()
    api = open(os.path.join(CSRC, "ilqr_api.hip")).read()
    for word in ("posix_spawn", "waitpid", "probe_model_structure", "compose_stage_source"):
        assert word not in api, word
