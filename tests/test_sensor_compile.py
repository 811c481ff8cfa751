"""ilqr_compile_sensor and the sensor registry without a GPU: a sensor written by hand in C is cross-compiled for gfx950 into the
module cache, registers itself and answers ilqr_sensor_dims; a second call is served from the cache (the file is not rewritten);
a changed source, name or dimension gives another tag; ilqr_load_sensor_library takes a module as a second process would; every
refusal of ilqr_compile_sensor, and every refusal of the handle entry points that needs no device, holds here. The symbols are
exported, declared, mirrored in ctypes and named in the Julia file."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ["ilqr_compile_sensor", "ilqr_load_sensor_library", "ilqr_register_sensor", "ilqr_sensor_count", "ilqr_sensor_name", "ilqr_sensor_dims",
       "ilqr_sensor_linearise", "ilqr_sensor_linearise_device", "ilqr_plant_measure_sensor", "ilqr_plant_measure_sensor_device",
       "ilqr_estimate_update_sensor", "ilqr_estimate_update_sensor_device", "ilqr_mpc_run_nlsensor"]
NAN, INF = float("nan"), float("inf")
# the bearing to a beacon and the squared speed: nx = 4, ny = 2, ns = 2
SOURCE = """
ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s) {
    if (j == 0) {
        const double dx = s[0] - x[0], dy = s[1] - x[1], d2 = dx * dx + dy * dy;
        *y = atan2(dy, dx);
        dydx[0] = dy / d2;
        dydx[1] = -dx / d2;
    } else {
        *y = x[2] * x[2] + x[3] * x[3];
        dydx[2] = 2.0 * x[2];
        dydx[3] = 2.0 * x[3];
    }
}
"""


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    for fn in FNS:
        assert hasattr(p._ffi.lib(), fn), "the library has no %s: nothing here has a subject" % fn
    return p


def _compile(pkg, name, nx, ny, ns, source, name_len=256, path_len=4096):
    reg, path = C.create_string_buffer(256), C.create_string_buffer(4096)
    src = pkg._ffi.SensorSource(name, nx, ny, ns, source, 0)
    rc = pkg._ffi.lib().ilqr_compile_sensor(C.byref(src), reg, name_len, path, path_len)
    return rc, reg.value.decode(), path.value.decode()


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = S.strip_comments(open(os.path.join(ROOT, "include", "ilqr_hip.h")).read())
    jl = open(S.JULIA).read()
    for name in FNS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert len(pkg._ffi.SYMBOLS[name][1]) == len(S.H_PROTOS[name][1]), name
        assert ":" + name in jl, name
    assert S.H_PROTOS["ilqr_mpc_run_nlsensor"][1] == (["ptr:void", "ptr:struct:ilqr_mpc_desc", "ptr:struct:ilqr_plant_io", "ptr:struct:ilqr_nl_sensor"]
                                                      + ["ptr:f64"] * 8 + ["ptr:i32"] + ["ptr:f64"] * 3 + ["ptr:i32"] + ["ptr:f64"] * 3)
    for cname, cls in (("ilqr_sensor_source", pkg._ffi.SensorSource), ("ilqr_nl_sensor", pkg._ffi.NlSensor)):
        offs, size = S.c_layout(S.H_STRUCTS[cname])
        assert cls.__name__ == cname and [f[0] for f in cls._fields_] == [o[0] for o in offs]
        assert [getattr(cls, nm).offset for nm, _ in offs] == [o for _, o in offs] and C.sizeof(cls) == size
    for fn in ("sensor_linearise_", "sensor_linearise_device_", "plant_measure_sensor_", "plant_measure_sensor_device_", "estimate_update_sensor_",
               "estimate_update_sensor_device_"):
        assert callable(getattr(pkg.Solver, fn)), fn
    nl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device_sensor_nl.hpp")).read()
    assert "static_assert(sizeof(SensorNlArgs) <= 4096" in nl and "__launch_bounds__(64) void sensor_linearise_kernel" in nl
    # the model side is what it was
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    assert int(re.search(r"#define ILQR_MODEL_ABI_VERSION (\d+)", dev).group(1)) == 21


def test_compile_cache_tags_and_dims(pkg):
    L = pkg._ffi.lib()
    rc, reg, path = _compile(pkg, b"bearing_speed", 4, 2, 2, SOURCE.encode())
    assert rc == 0, L.ilqr_last_error().decode()
    assert re.fullmatch(r"bearing_speed_c[0-9a-f]{16}", reg) and os.path.basename(path) == "libilqr_sensor_%s.so" % reg and os.path.exists(path)
    assert os.path.dirname(path) == os.path.join(pkg._ffi.LIB_DIR, "models")
    assert reg in [L.ilqr_sensor_name(i).decode() for i in range(L.ilqr_sensor_count())] and L.ilqr_sensor_name(L.ilqr_sensor_count()) is None
    assert pkg.sensor_dims(reg) == (4, 2, 2)
    assert L.ilqr_sensor_dims(b"no_such_sensor", None, None, None) == -1
    # served from the cache: the file is not rewritten
    before = os.stat(path)
    rc2, reg2, path2 = _compile(pkg, b"bearing_speed", 4, 2, 2, SOURCE.encode())
    after = os.stat(path)
    assert rc2 == 0 and (reg2, path2) == (reg, path) and (before.st_mtime_ns, before.st_ino) == (after.st_mtime_ns, after.st_ino)
    leftovers = [f for f in os.listdir(os.path.dirname(path)) if f.startswith("sensor_" + reg) or ".tmp" in f]
    assert not leftovers, leftovers
    # another source, name or dimension: another tag
    rc3, reg3, _ = _compile(pkg, b"bearing_speed", 4, 2, 2, SOURCE.replace("2.0 * x[3]", "x[3] + x[3]").encode())
    rc4, reg4, _ = _compile(pkg, b"bearing_speed", 4, 2, 3, SOURCE.encode())
    assert rc3 == 0 and rc4 == 0 and len({reg, reg3, reg4}) == 3 and pkg.sensor_dims(reg4) == (4, 2, 3)
    # a second process finds the cached module without a compiler
    code = ("import sys; sys.path.insert(0, %r)\nfrom ilqr_amd_loader import load_package\np = load_package(); L = p._ffi.lib()\n"
            "assert L.ilqr_sensor_count() == 0\nassert L.ilqr_load_sensor_library(%r) == 0, L.ilqr_last_error()\n"
            "assert p.sensor_dims(%r) == (4, 2, 2)\nassert L.ilqr_load_sensor_library(b'/no/such/file.so') != 0\nprint('loaded')\n"
            % (ROOT, path.encode(), reg))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ILQR_HIPCC="/no/such/compiler"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip() == "loaded", out.stderr.decode()
    # source that does not compile: ILQR_ERR_MODEL with the compiler's words, nothing left registered under the name
    rc5, _, _ = _compile(pkg, b"broken", 2, 1, 0, b"ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s) { *y = nope; }")
    assert rc5 == -3 and b"nope" in L.ilqr_last_error()
    assert not [f for f in os.listdir(os.path.dirname(path)) if "broken" in f], "a failed compilation leaves nothing in the module cache"


def test_compile_refusals(pkg):
    L = pkg._ffi.lib()
    src = SOURCE.encode()
    reg, path = C.create_string_buffer(256), C.create_string_buffer(4096)
    ok = pkg._ffi.SensorSource(b"fine", 4, 2, 2, src, 0)
    assert L.ilqr_compile_sensor(None, reg, 256, path, 4096) == -1 and b"null argument" in L.ilqr_last_error()
    assert L.ilqr_compile_sensor(C.byref(ok), None, 256, path, 4096) == -1 and L.ilqr_compile_sensor(C.byref(ok), reg, 256, None, 4096) == -1
    assert L.ilqr_compile_sensor(C.byref(pkg._ffi.SensorSource(None, 4, 2, 2, src, 0)), reg, 256, path, 4096) == -1
    assert L.ilqr_compile_sensor(C.byref(pkg._ffi.SensorSource(b"fine", 4, 2, 2, None, 0)), reg, 256, path, 4096) == -1
    for name in (b"two words", b"semi;colon", b"", b"9lives", b"a-b"):
        assert _compile(pkg, name, 4, 2, 2, src)[0] == -1 and b"C identifier" in L.ilqr_last_error(), name
    for nx, ny, ns in ((0, 2, 2), (65, 2, 2), (4, 0, 2), (4, 65, 2), (4, 2, -1), (4, 2, 65), (-3, 2, 2)):
        assert _compile(pkg, b"fine", nx, ny, ns, src)[0] == -1 and b"1 <= nx <= 64, 1 <= ny <= 64, 0 <= ns <= 64" in L.ilqr_last_error(), (nx, ny, ns)
    assert _compile(pkg, b"fine", 4, 2, 2, src, name_len=8)[0] == -1 and b"output buffers too small" in L.ilqr_last_error()
    assert _compile(pkg, b"fine", 4, 2, 2, src, path_len=16)[0] == -1 and b"output buffers too small" in L.ilqr_last_error()
    assert L.ilqr_load_sensor_library(None) == -1 and L.ilqr_register_sensor(None) == -1


def test_handle_entry_point_refusals_need_no_device(pkg):
    """what needs no handle is refused first: a null array, the name, per_instance_s, iterations, a null s, r, sigma_y, the noise key's
    fields; then the null handle itself"""
    L, F64 = pkg._ffi.lib(), pkg._ffi.c_double_p
    rc, reg, _ = _compile(pkg, b"bearing_speed", 4, 2, 2, SOURCE.encode())
    assert rc == 0
    name = reg.encode()
    buf = np.zeros(16)
    vec = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(F64)
    for host in (True, False):
        x = buf.ctypes.data_as(F64) if host else C.c_void_p(buf.ctypes.data)
        sfx = "" if host else "_device"
        lin, mea, upd = (getattr(L, "ilqr_" + f + sfx) for f in ("sensor_linearise", "plant_measure_sensor", "estimate_update_sensor"))
        cases = [(lambda: lin(None, name, 0, x, None, None, x, x), b"null x_lin, H_out or yhat_out"),
                 (lambda: lin(None, None, 0, x, x, None, x, x), b"null sensor name"),
                 (lambda: lin(None, b"no_such_sensor", 0, x, x, None, x, x), b"unknown sensor"),
                 (lambda: lin(None, name, 2, x, x, None, x, x), b"per_instance_s must be 0 or 1"),
                 (lambda: lin(None, name, 0, None, x, None, x, x), b"null s for a sensor with parameters"),
                 (lambda: lin(None, name, 1, x, x, None, x, x), b"null handle"),
                 (lambda: mea(None, name, 0, x, 1, 0, 0, None, None, x), b"null x or y"),
                 (lambda: mea(None, b"no_such_sensor", 0, x, 1, 0, 0, None, x, x), b"unknown sensor"),
                 (lambda: mea(None, name, 0, x, 1, 0, 0, vec(0.1, -1.0), x, x), b"sigma_y must be finite and >= 0"),
                 (lambda: mea(None, name, 0, x, 1, 0, 0, vec(NAN, 0.0), x, x), b"sigma_y must be finite and >= 0"),
                 (lambda: mea(None, name, 0, x, 1, 0, -1, None, x, x), b"the measurement step must lie in"),
                 (lambda: mea(None, name, 0, x, 1, 0, 1 << 20, None, x, x), b"the measurement step must lie in"),
                 (lambda: mea(None, name, 0, x, 1, -1, 0, None, x, x), b"first_instance must lie in"),
                 (lambda: mea(None, name, 0, x, 1, 0, 0, vec(0.1, 0.0), x, x), b"null handle"),
                 (lambda: upd(None, name, 0, x, 1, None, x, x, x, None, None, None), b"null r, y, xhat or P"),
                 (lambda: upd(None, name, 0, x, 1, vec(1.0, 1.0), x, None, x, None, None, None), b"null r, y, xhat or P"),
                 (lambda: upd(None, b"no_such_sensor", 0, x, 1, vec(1.0, 1.0), x, x, x, None, None, None), b"unknown sensor"),
                 (lambda: upd(None, name, 0, x, 0, vec(1.0, 1.0), x, x, x, None, None, None), b"iterations must lie in 1 .. 8"),
                 (lambda: upd(None, name, 0, x, 9, vec(1.0, 1.0), x, x, x, None, None, None), b"iterations must lie in 1 .. 8"),
                 (lambda: upd(None, name, 0, x, 1, vec(1.0, 0.0), x, x, x, None, None, None), b"r must be finite and > 0"),
                 (lambda: upd(None, name, 0, x, 1, vec(INF, 1.0), x, x, x, None, None, None), b"r must be finite and > 0"),
                 (lambda: upd(None, name, 0, x, 1, vec(1.0, NAN), x, x, x, None, None, None), b"r must be finite and > 0"),
                 (lambda: upd(None, name, 0, x, 8, vec(1.0, 1.0), x, x, x, None, None, None), b"null handle")]
        for call, msg in cases:
            assert call() == -1
            assert msg in L.ilqr_last_error(), (host, msg, L.ilqr_last_error())
    # the loop: what needs no handle of the sensor struct
    d = pkg._ffi.MpcDesc(1, 1, 0, 0, 0, 1, 0, 0, 0, 0, None)
    P0 = buf.ctypes.data_as(F64)
    run = lambda sens, io=None, P=P0: L.ilqr_mpc_run_nlsensor(None, C.byref(d), io, C.byref(sens), None, None, P, None, None, None, None, None, None, None,
                                                              None, None, None, None, None, None)
    r2, s2 = vec(1.0, 1.0), vec(1.0, 2.0)
    NL = pkg._ffi.NlSensor
    io = pkg._ffi.PlantIO(None, None, vec(0.1, 0.1, 0.1, 0.1), 0, 0)
    for sens, kw, msg in [(NL(name, 0, s2, r2, None, None, 1), dict(P=None), b"a sensor with a null P"),
                          (NL(name, 0, s2, r2, None, None, 1), dict(io=C.byref(io)), b"io->sigma_y together with a sensor"),
                          (NL(name, 0, s2, None, None, None, 1), {}, b"null r"),
                          (NL(b"no_such_sensor", 0, s2, r2, None, None, 1), {}, b"unknown sensor"),
                          (NL(name, 3, s2, r2, None, None, 1), {}, b"per_instance_s must be 0 or 1"),
                          (NL(name, 0, s2, r2, None, None, 0), {}, b"iterations must lie in 1 .. 8"),
                          (NL(name, 0, s2, r2, None, None, 9), {}, b"iterations must lie in 1 .. 8"),
                          (NL(name, 0, None, r2, None, None, 1), {}, b"null s for a sensor with parameters"),
                          (NL(name, 0, s2, vec(1.0, -2.0), None, None, 1), {}, b"r must be finite and > 0"),
                          (NL(name, 0, s2, r2, vec(-1.0), None, 1), {}, b"q must be finite and >= 0"),
                          (NL(name, 0, s2, r2, None, vec(0.1, INF), 1), {}, b"sigma_y must be finite and >= 0"),
                          (NL(name, 0, s2, r2, None, None, 2), {}, b"null handle")]:
        assert run(sens, **kw) == -1
        assert msg in L.ilqr_last_error() and b"ilqr_mpc_run_nlsensor" in L.ilqr_last_error(), (msg, L.ilqr_last_error())
    # the Python mirror rejects what it can before any call
    with pytest.raises(pkg._ffi.IlqrError, match="unknown sensor"):
        pkg.sensor_dims("no_such_sensor")
