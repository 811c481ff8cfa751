"""The launch plan (csrc/ilqr_launch_plan.hpp) is plain C++: compiled here with g++ and checked on the host against a table of
handle states and the launches written out by hand — which kernel (latency, throughput, one wave per instance, packed with one
or two waves per pack), its grid and LDS, the hand-over, the pool of the one-wave packed form (marks and vacated CUs only while
every workgroup of the launch is resident), the role slots, and the stage kernels' mapping."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_table(tmp_path):
    exe = str(tmp_path / "launch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "iterativelqr.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d rows checked" % (len(lines) - 1) and len(lines) > 60
