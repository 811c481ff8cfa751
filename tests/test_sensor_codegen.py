"""codegen.generate_sensor_source on the CPU: the `sensor_row` it emits for every test sensor (tests/sensor_nl_ref.py) is compiled for
the host by this test — g++, contraction off, the source wrapped as ilqr_compile_sensor wraps it for the device — and held to sympy's
own lambdify of h and of its Jacobian on random points, within 1e-13 relative to max(1, |reference|): both evaluate the same
expressions in fp64 and differ by the association common subexpressions change, a few ulp. A partial that is structurally zero is
not written at all: dydx keeps whatever it held there (the kernel hands over a zeroed row), and an unknown row index writes nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import policy_ref as P
import sensor_nl_ref as N
from ilqr_amd_loader import load_package

WRAP = """#include <cmath>
#include <math.h>
#define ILQR_SENSOR_FN inline
namespace ilqr_user {
using namespace std;
%s
}
extern "C" void row(int j, double* y, double* dydx, const double* x, const double* s) { ilqr_user::sensor_row(j, y, dydx, x, s); }
"""


@pytest.fixture(scope="module")
def codegen():
    return load_package().codegen


@pytest.mark.parametrize("key", sorted(N.SENSORS))
def test_generated_row_is_sympys_function_and_jacobian(codegen, key, tmp_path):
    import sympy as sp
    _, nx, ny, ns, _ = N.SENSORS[key]
    got_ny, src = codegen.generate_sensor_source(key, N.symbolic(key), nx, ns)
    assert got_ny == ny and "switch (j)" in src and src.count("case ") == ny and "ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s)" in src
    cpp, so = str(tmp_path / "row.cpp"), str(tmp_path / "row.so")
    open(cpp, "w").write(WRAP % src)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", cpp, "-o", so, "-lm"])
    fn = C.CDLL(so).row
    fn.restype, fn.argtypes = None, [C.c_int] + [C.POINTER(C.c_double)] * 4
    x, s, rows, jac = codegen.sensor_expressions(N.symbolic(key), nx, ns)
    fh, fj = sp.lambdify([x, s], sp.Matrix(rows), "numpy"), sp.lambdify([x, s], sp.Matrix(jac), "numpy")
    zero = np.array([[d == 0 for d in row] for row in jac])
    assert zero.any() or nx < 4
    rng = np.random.default_rng(5)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    worst = 0.0
    for _ in range(8):
        xv, sv = rng.uniform(-1.5, 1.5, nx), rng.uniform(0.5, 3.0, max(ns, 1))
        href, jref = np.array(fh(xv, sv[:ns]), dtype=np.float64).ravel(), np.array(fj(xv, sv[:ns]), dtype=np.float64).reshape(ny, nx)
        for j in range(ny):
            y, d = np.full(1, 7.5), np.zeros(nx)
            fn(j, p(y), p(d), p(xv), p(sv))
            worst = max(worst, abs(y[0] - href[j]) / max(1.0, abs(href[j])), P.rel(d, jref[j]))
            assert (d[zero[j]] == 0.0).all(), (key, j)
            d2 = np.full(nx, -3.25)                # rows not written stay as they were
            fn(j, p(y), p(d2), p(xv), p(sv))
            assert (d2[zero[j]] == -3.25).all() and np.array_equal(d2[~zero[j]], d[~zero[j]]), (key, j)
        y, d = np.full(1, 7.5), np.full(nx, -3.25)
        fn(ny, p(y), p(d), p(xv), p(sv))
        assert y[0] == 7.5 and (d == -3.25).all()
    print("generated sensor_row %s against lambdify: worst relative difference %.2e" % (key, worst))
    assert worst < 1e-13, (key, worst)


def test_structure_of_the_synth12_sensor(codegen):
    """one row with a single non-zero partial, one dense row"""
    _, _, _, jac = codegen.sensor_expressions(N.symbolic("mix12"), 12, 2)
    nnz = [sum(d != 0 for d in row) for row in jac]
    assert nnz[11] == 1 and nnz[12] == 12 and len(nnz) == 13


def test_dimensions_are_checked(codegen):
    with pytest.raises(ValueError):
        codegen.generate_sensor_source("wide", lambda x, s: [x[0]] * 65, 1, 0)
    with pytest.raises(ValueError):
        codegen.generate_sensor_source("none", lambda x, s: [], 2, 0)
