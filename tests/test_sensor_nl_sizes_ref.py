"""The tables of tests/sensor_nl_sizes.py on the CPU: what tests/test_gpu_sensor_nl_sizes.py compares the device with has to be right,
well conditioned and complete first.

1. Generated source against its references: every entry's `sensor_row` through the host compile of tests/test_sensor_codegen.py (its
   WRAP, g++ with contraction off) equals sympy's lambdify of h and of its Jacobian within that file's 1e-13; family3 also equals the
   mpmath reference within TOL_F; structurally zero partials are not written, an unknown row writes nothing.
2. The yardstick checks itself: on the size sensors the complex-step Jacobian equals mpmath.diff of the same h (the family's method,
   where both exist) within 1e-13; sensor_nl_ref.update and iekf_textbook agree at one iteration within a tenth of TOL_XU.
3. The bounds are decided without a device, as tests/test_mpc_ref.py decides the sweep's: each reference is evaluated again with x̂
   and s moved by one part in 1e15, and ten times what that moves stays under TOL_F = 1e-12 (H, ŷ, y) and TOL_XU = 1e-10 (x̂, P,
   innovation, nis), relative to max(1, max |reference|). The table is printed (pytest -s) and recorded in the GPU test's docstring.
4. No case is left out: on every instance the GPU test compares, with a shared and a per-instance s, at 1 and 3 iterations, the
   yardstick's update has first_bad == −1; every s[i] enters a value and a partial, every column of H is non-zero somewhere; the
   family's points keep 1e-3 from each kink, |0.3 x0| <= 0.45, and its bearing innovation stays inside (−π + 0.2, π − 0.2).
5. generate_sensor_source refuses, with a ValueError naming the construct, an h whose source C could not express; api.compile_sensor
   passes that on."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import policy_ref as P
import sensor_nl_ref as N
import sensor_nl_sizes as Z
import test_sensor_codegen as TC
from ilqr_amd_loader import load_package

TOL_F = 1e-12
TOL_XU = 1e-10
MOVE = 1.0 + 1.0e-15


@pytest.fixture(scope="module")
def pkg():
    return load_package()


# ----------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("key", Z.KEYS)
def test_generated_row_is_sympys_and_the_familys_is_mpmaths(pkg, key, tmp_path):
    import sympy as sp
    nx, ny, ns = N.dims(key)
    got_ny, src = pkg.codegen.generate_sensor_source(key, N.symbolic(key), nx, ns)
    assert got_ny == ny and src.count("case ") == ny
    cpp, so = str(tmp_path / "row.cpp"), str(tmp_path / "row.so")
    open(cpp, "w").write(TC.WRAP % src)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", cpp, "-o", so, "-lm"])
    fn = C.CDLL(so).row
    fn.restype, fn.argtypes = None, [C.c_int] + [C.POINTER(C.c_double)] * 4
    x, s, rows, jac = pkg.codegen.sensor_expressions(N.symbolic(key), nx, ns)
    fh, fj = sp.lambdify([x, s], sp.Matrix(rows), "numpy"), sp.lambdify([x, s], sp.Matrix(jac), "numpy")
    zero = np.array([[d == 0 for d in row] for row in jac])
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def host(xv, sv):
        """(h [ny], H [ny, nx]) of the compiled row, each row checked for what it must not write"""
        hh, HH = np.zeros(ny), np.zeros((ny, nx))
        for j in range(ny):
            y, d, d2 = np.full(1, 7.5), np.zeros(nx), np.full(nx, -3.25)
            fn(j, p(y), p(d), p(xv), p(sv))
            fn(j, p(y), p(d2), p(xv), p(sv))
            assert (d[zero[j]] == 0.0).all() and (d2[zero[j]] == -3.25).all() and np.array_equal(d2[~zero[j]], d[~zero[j]]), (key, j)
            hh[j], HH[j] = y[0], d
        y, d = np.full(1, 7.5), np.full(nx, -3.25)
        fn(ny, p(y), p(d), p(xv), p(sv))
        assert y[0] == 7.5 and (d == -3.25).all()
        return hh, HH

    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(4):
        xv, sv = rng.uniform(-1.5, 1.5, nx), rng.uniform(0.5, 3.0, max(ns, 1))
        hh, HH = host(xv, sv)
        href, jref = np.array(fh(xv, sv[:ns]), dtype=np.float64).ravel(), np.array(fj(xv, sv[:ns]), dtype=np.float64).reshape(ny, nx)
        worst = max(worst, max(abs(hh[j] - href[j]) / max(1.0, abs(href[j])) for j in range(ny)), max(P.rel(HH[j], jref[j]) for j in range(ny)))
    print("generated sensor_row %s against lambdify: worst relative difference %.2e" % (key, worst))
    assert worst < 1e-13, (key, worst)
    if key in Z.FAMILY:
        xh, _, _, _ = Z.inputs(key)
        s, worst = Z.s_instances(key, Z.B), 0.0
        assert zero[ny - 1].all()                  # the constant row: nothing but the kernel's zero fill writes its row of H
        for b in Z.some(key, Z.B):
            hh, HH = host(np.ascontiguousarray(xh[b]), np.ascontiguousarray(s[b]))
            worst = max(worst, P.rel(hh, Z.mp_h(key, xh[b], s[b])), P.rel(HH, Z.mp_jacobian(key, xh[b], s[b])))
        print("generated sensor_row %s against mpmath: worst relative difference %.2e (bound %.1e)" % (key, worst, TOL_F))
        assert worst < TOL_F, worst


# ----------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("key", list(Z.SIZE_SENSORS))
def test_complex_step_is_mpmaths_derivative(key):
    nx, ny, ns = N.dims(key)
    xh, _, _, _ = Z.inputs(key)
    s = Z.s_instances(key, Z.B)
    rows = sorted({0, 1 % ny, ny // 2, ny - 1})
    worst = 0.0
    for b in (0, 69):
        for j in rows:                             # a dense row costs nx evaluations of nx terms at 50 digits: the columns its neighbours read, and the ends
            cols = sorted({0, j % nx, (j + 1) % nx, (j + 5) % nx, (j + 37) % nx, nx - 1})
            H, Hm = N.jacobian(key, xh[b], s[b]), Z.mp_jacobian(key, xh[b], s[b], [j], cols)
            worst = max(worst, P.rel(H[j, cols], Hm[j, cols]))
        worst = max(worst, P.rel(N.h(key, xh[b], s[b]), Z.mp_h(key, xh[b], s[b])))
    print("complex step of %s against mpmath.diff: worst relative difference %.2e" % (key, worst))
    assert worst < 1e-13, (key, worst)


@pytest.mark.parametrize("key", Z.KEYS)
def test_one_iteration_is_the_textbook_update(key):
    ny = N.dims(key)[1]
    xh, Ps, _, ys = Z.inputs(key)
    worst = 0.0
    for s in (Z.s_shared(key), Z.s_instances(key, Z.B)):
        y = Z.readings(key, ys, s)
        for b in Z.some(key, Z.B):
            sb = s if s.ndim == 1 else s[b]
            a, t = _update(key, b, s.ndim, 1), N.iekf_textbook(key, xh[b], Ps[b], y[b], sb, N.r(ny), 1)
            worst = max(worst, P.rel(a["xhat"], t["xhat"]), P.rel(a["P"], t["P"]))
    print("update of %s against the textbook form, one iteration: worst relative difference %.2e (bound %.1e)" % (key, worst, 0.1 * TOL_XU))
    assert worst <= 0.1 * TOL_XU, (key, worst)


# ----------------------------------------------------------------------------------------------------------------------- 3, 4
_CACHE = {}


def _reference(key, b, sdim, move=1.0):
    """everything the GPU test asks the yardstick of instance b (s shared: sdim 1, per instance: 2), x̂ and s scaled by `move`;
    computed once per process"""
    at = (key, b, sdim, move)
    if at not in _CACHE:
        ny = N.dims(key)[1]
        xh, Ps, xp, ys = Z.inputs(key)
        s = Z.s_shared(key) if sdim == 1 else Z.s_instances(key, Z.B)
        y = Z.readings(key, ys, s)[b]              # the readings are inputs: they do not move
        sb = (s if sdim == 1 else s[b]) * move
        x = xh[b] * move
        H, yhat = N.linearise(key, x, sb)
        out = dict(H=H, yhat=yhat, yprior=N.linearise(key, x, sb, xp[b])[1])
        for it in (1, 3):
            out[it] = N.update(key, x, Ps[b], y, sb, N.r(ny), it)
        _CACHE[at] = out
    return _CACHE[at]


def _update(key, b, sdim, it):
    return _reference(key, b, sdim)[it]


def _moved(a, c):
    return float(np.abs(np.asarray(a) - np.asarray(c)).max() / max(1.0, np.abs(np.asarray(a)).max()))


@pytest.mark.parametrize("key", Z.KEYS)
def test_nobody_is_left_out_and_the_bounds_stand(key):
    nx, ny, ns = N.dims(key)
    worst = dict(H=0.0, yhat=0.0, yprior=0.0, xhat=0.0, P=0.0, innovation=0.0, nis=0.0)
    for sdim in ((1, 2) if ns else (1,)):
        for b in Z.some(key, Z.B):
            ref, mov = _reference(key, b, sdim), _reference(key, b, sdim, MOVE)
            for it in (1, 3):
                assert ref[it]["first_bad"] == -1 and np.isfinite(ref[it]["P"]).all() and ref[it]["nis"] > 0.0, (key, sdim, b, it)
                if key in Z.FAMILY:                # the bearing's innovation is a small angle: plain subtraction is the right one
                    assert abs(ref[it]["innovation"][0]) < np.pi - 0.2, (b, it, ref[it]["innovation"][0])
                for k in ("xhat", "P", "innovation", "nis"):
                    worst[k] = max(worst[k], _moved(ref[it][k], mov[it][k]))
            for k in ("H", "yhat", "yprior"):
                worst[k] = max(worst[k], _moved(ref[k], mov[k]))
    print("sensor_nl_sizes spread %-7s H %.1e  yhat, y %.1e  yhat(prior) %.1e | xhat %.1e  P %.1e  innovation %.1e  nis %.1e"
          % (key, worst["H"], worst["yhat"], worst["yprior"], worst["xhat"], worst["P"], worst["innovation"], worst["nis"]))
    assert 10.0 * max(worst[k] for k in ("H", "yhat", "yprior")) < TOL_F, (key, worst)
    assert 10.0 * max(worst[k] for k in ("xhat", "P", "innovation", "nis")) < TOL_XU, (key, worst)


@pytest.mark.parametrize("key", Z.KEYS)
def test_every_parameter_and_every_column_is_used(pkg, key):
    nx, ny, ns = N.dims(key)
    x, s, rows, jac = pkg.codegen.sensor_expressions(N.symbolic(key), nx, ns)
    assert len(rows) == ny
    for k in range(nx):
        assert any(jac[j][k] != 0 for j in range(ny)), (key, "column", k)
    for v in s:
        assert any(r.has(v) for r in rows) and any(d.has(v) for row in jac for d in row), (key, v)
    if key == "fan1":                              # s[j] is row j's alone: a wrong s_stride moves every output
        assert all(rows[j].free_symbols == {x[0], s[j]} for j in range(64))
    if key == "wide64":                            # the component a NaN is put in: no row below 32 reads it
        assert [j for j in range(ny) if jac[j][Z.WIDE64_LATE] != 0] == [32, 33, 60, 63]
        assert sum(d != 0 for d in jac[63]) == 64 and sum(d != 0 for d in jac[0]) == 63


def test_the_familys_points_keep_off_the_kinks():
    xh, _, _, _ = Z.inputs("family3")
    assert xh.shape == (70, 3) and (np.abs(xh) <= 1.5).all()
    s = Z.s_shared("family3")
    si = Z.s_instances("family3", Z.B)
    assert np.array_equal(si[:8, :2], np.broadcast_to(s[:2], (8, 2))) and not np.array_equal(si[8:, :2], np.broadcast_to(s[:2], (62, 2)))
    x = xh[list(Z.some("family3", Z.B))]
    m = Z.KINK_MARGIN
    assert (np.abs(x[:, 2]) >= m).all() and (np.abs(x[:, 0] - 0.3) >= m).all() and (np.abs(x[:, 0] - x[:, 1]) >= m).all()
    assert (np.abs(0.3 * x[:, 0]) <= Z.ASIN_ARGUMENT).all()
    dx, dy = xh[:8, 0] - s[0], xh[:8, 1] - s[1]
    assert [(a > 0, c > 0) for a, c in zip(dx[:4], dy[:4])] == [(True, True), (False, True), (False, False), (True, False)]
    assert dx[4] == 0.0 and dx[5] == 0.0 and dy[4] > 0 > dy[5]
    assert dx[6] < 0 and dx[7] < 0 and 0 < dy[6] < 2e-6 and -2e-6 < dy[7] < 0
    b = np.array([N.h("family3", xh[i], s)[0] for i in range(8)])
    assert abs(b[4] - np.pi / 2) < 1e-15 and abs(b[5] + np.pi / 2) < 1e-15 and b[6] > 3.14159 and b[7] < -3.14159


# ----------------------------------------------------------------------------------------------------------------------- 5
def test_what_c_cannot_express_is_refused(pkg):
    import sympy as sp
    with pytest.raises(ValueError, match="DiracDelta"):
        pkg.codegen.generate_sensor_source("kinked", lambda x, s: [sp.sign(x[0]) * x[1]], 2, 0)
    with pytest.raises(ValueError, match="besselj"):
        pkg.codegen.generate_sensor_source("bessel", lambda x, s: [x[1], sp.besselj(0, x[0])], 2, 0)
    with pytest.raises(ValueError, match="frobnicate"):
        pkg.codegen.generate_sensor_source("unknown", lambda x, s: [sp.Function("frobnicate")(x[0]) + s[0]], 1, 1)
    for h in (lambda x, s: [sp.sign(x[0]) * x[1]], lambda x, s: [sp.besselj(0, x[0]), x[1]]):
        with pytest.raises(ValueError, match="C cannot express"):
            pkg.compile_sensor("refused", h, 2)    # before anything is handed to the library
    ny, src = pkg.codegen.generate_sensor_source("fine", lambda x, s: [sp.sign(s[0]) * sp.Abs(x[1]) + x[0]], 2, 1)      # sign itself is C
    assert ny == 1 and "Not supported" not in src
