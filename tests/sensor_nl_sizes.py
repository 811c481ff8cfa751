"""Two more tables of compiled nonlinear sensors for tests/sensor_nl_ref.py's yardstick (tests/test_sensor_nl_sizes_ref.py,
tests/test_gpu_sensor_nl_sizes.py), under that module's rule: ONE definition h(x, s, m) per sensor, traced by sympy for the code
generator and evaluated independently for the yardstick. Registered with sensor_nl_ref, so that its h, jacobian, linearise,
measure, update, iekf_textbook, symbolic and compiled take these keys as they take their own.

SIZE_SENSORS run on the synth family of the MPC sweep (tests/test_gpu_mpc_sweep.py: the same modules under the same names), at the
sizes where sensor_linearise_kernel, its launch and the update behind it change:

    handle   key     ny  ns   there for
    (1, 1)   one1     1   0   the (1, 1) grid; a one-term x_prior chain; a null s
    (1, 1)   fan1    64  64   ny far above nx; s[j] used by row j alone, so s_stride = 64 shows in every output; noise key fields
                              5 + j / 16 up to 8; 64 sequential scalar updates on one state
    (5, 1)   mix5     6   2   the first large-form size; ny = nx + 1
    (17, 2)  mix17   18   0   a chain of 2 · 8 + 1 terms; rows >= 16; a null s on the large form
    (33, 2)  mix33   34   1   a chain of 4 · 8 + 1 terms; rows >= 32: word 1 of the update's mask
    (64, 8)  one64    1   0   one dense row: the full 64-term chain on a single grid row
    (64, 8)  wide64  64  64   the measurement's 33 KB LDS sink, 4096 doubles of H per instance. Row 63 dense and row 0 dense but for
                              x_33, tanh(s_j · Σ c_k x_k); the others sin(s_j x_j) + x_{(j+1) % 64} x_{(j+37) % 64}

(Row 0 of wide64 leaves x_33 out on purpose: x_33 is then read by rows 32, 33, 60 and 63 only, which is what lets a NaN there be first
seen at a row of mask word 1.) Every s[i] enters some row's value and some partial, every column of H is non-zero in some row
(tests/test_sensor_nl_sizes_ref.py asserts both). Built from sin, tanh, products and s; the yardstick is the complex step.

FAMILY holds family3 on car_obs (nx = 3, ns = 3: a beacon at (s0, s1) and a gain s2): the functions a symbolic sensor may use beyond
those — atan2, exp, log, Abs, a 3/2 power, a Piecewise saturation, Max, a quotient, fifth powers, asin, sinh, atan, rationals and a
constant row. Its yardstick is mpmath at 50 digits: h through mpmath's functions, the Jacobian through mpmath.diff (numerical, so
independent of the symbolic derivative the device compiles), both rounded to fp64 once at the end. Its inputs are an explicit
[70, 3] array; instances 0 .. 7 sit by hand on the bearing (the four quadrants, x0 = s0 exactly, both sides of the branch cut)."""
import numpy as np

import estimator_ref as E
import mpc_ref as M
import sensor_nl_ref as N

DPS = 50


def _c(k):
    return float(np.cos(0.4 * (k + 1)))


def _dense(x, n, skip=()):
    acc = 0.0 * x[0]
    for k in range(n):
        if k not in skip:
            acc = acc + _c(k) * x[k]
    return acc


# ------------------------------------------------------------------------------------------------------------- the size sensors
def _one1(x, s, m):
    return [m.tanh(x[0]) * x[0] + m.sin(x[0])]


def _fan1(x, s, m):
    return [m.sin(s[j] * x[0]) + _c(j) * m.tanh(x[0]) for j in range(64)]


def _mix5(x, s, m):
    return [m.tanh(x[j]) * x[(j + 1) % 5] + s[0] * x[j] for j in range(5)] + [m.tanh(s[1] * _dense(x, 5))]


def _mix17(x, s, m):
    return [m.sin(x[j]) + x[(j + 1) % 17] * x[(j + 5) % 17] for j in range(17)] + [m.tanh(0.3 * _dense(x, 17))]


def _mix33(x, s, m):
    return [m.sin(x[j]) + s[0] * x[(j + 1) % 33] * x[(j + 5) % 33] for j in range(33)] + [m.tanh(0.2 * _dense(x, 33))]


def _one64(x, s, m):
    return [m.tanh(0.2 * _dense(x, 64)) + x[0] * x[63]]


WIDE64_LATE = 33                  # the component of wide64 that no row below 32 reads (rows 32, 33, 60 and 63 do)


def _wide64(x, s, m):
    rows = [m.tanh(s[0] * _dense(x, 64, skip=(WIDE64_LATE,)))]
    rows += [m.sin(s[j] * x[j]) + x[(j + 1) % 64] * x[(j + 37) % 64] for j in range(1, 63)]
    return rows + [m.tanh(s[63] * _dense(x, 64))]


# key -> ((nx, nu) of the sweep's handle it runs on, nx, ny, ns, h)
SIZE_SENSORS = {
    "one1": ((1, 1), 1, 1, 0, _one1),
    "fan1": ((1, 1), 1, 64, 64, _fan1),
    "mix5": ((5, 1), 5, 6, 2, _mix5),
    "mix17": ((17, 2), 17, 18, 0, _mix17),
    "mix33": ((33, 2), 33, 34, 1, _mix33),
    "one64": ((64, 8), 64, 1, 0, _one64),
    "wide64": ((64, 8), 64, 64, 64, _wide64),
}


# ------------------------------------------------------------------------------------------------------------- the function family
class _Sympy:
    """what family3 is traced over"""
    def __init__(self):
        import sympy as sp
        self.atan2, self.exp, self.log, self.abs, self.max, self.asin, self.sinh, self.atan = sp.atan2, sp.exp, sp.log, sp.Abs, sp.Max, sp.asin, sp.sinh, sp.atan
        self.pow32 = lambda v: v ** sp.Rational(3, 2)
        self.saturate = lambda v: sp.Piecewise((v, v < 0.3), (0.3 + 0.1 * (v - 0.3), True))
        self.third, self.seven = sp.Rational(1, 3), sp.Integer(7)


class _Mpmath:
    """what family3 is evaluated over: mpmath at the working precision of the caller"""
    def __init__(self):
        import mpmath as mp
        self.atan2, self.exp, self.log, self.abs, self.asin, self.sinh, self.atan = mp.atan2, mp.exp, mp.log, mp.fabs, mp.asin, mp.sinh, mp.atan
        self.max = lambda a, b: a if a > b else b
        self.pow32 = lambda v: mp.sqrt(v) ** 3
        self.saturate = lambda v: v if v < 0.3 else 0.3 + 0.1 * (v - 0.3)       # (0.3 and 0.1: the doubles the generated C holds)
        self.third, self.seven = mp.mpf(1) / 3, mp.mpf(7)


def _family3(x, s, m):
    dx, dy = x[0] - s[0], x[1] - s[1]
    r2 = dx * dx + dy * dy
    return [m.atan2(dy, dx),                       # the bearing of the beacon's line of sight
            s[2] * m.exp(-r2 / 2),
            m.log(1 + r2),
            m.abs(x[2]) * x[0],
            m.pow32(r2),
            m.saturate(x[0]),
            m.max(x[0], x[1]),
            x[0] / (1 + x[2] * x[2]),
            x[0] ** 5,
            (2 + x[1]) ** -5,
            m.asin(0.3 * x[0]),
            m.sinh(x[0]) + m.atan(x[1]),
            m.third * x[0] + m.third * x[1],
            m.seven]
FAMILY_NY = 14
KINK_MARGIN, ASIN_ARGUMENT = 1.0e-3, 0.45


def mp_h(key, x, s):
    """h [ny] of any sensor of the tables through mpmath at DPS digits, rounded to fp64 once"""
    import mpmath as mp
    with mp.workdps(DPS):
        m = _Mpmath() if key in FAMILY else mp
        rows = N.entry(key)[4]([mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in s], m)
        return np.array([float(v) for v in rows])


def mp_jacobian(key, x, s, rows=None, cols=None):
    """H [ny, nx] by mpmath.diff of the same h at DPS digits (the entries of `rows` x `cols` alone when given, the others 0),
    rounded to fp64 once"""
    import mpmath as mp
    nx, ny, _ = N.dims(key)
    H = np.zeros((ny, nx))
    with mp.workdps(DPS):
        m = _Mpmath() if key in FAMILY else mp
        f, sv, xv = N.entry(key)[4], [mp.mpf(float(v)) for v in s], [mp.mpf(float(v)) for v in x]
        for j in (range(ny) if rows is None else rows):
            for k in (range(nx) if cols is None else cols):
                H[j, k] = float(mp.diff(lambda t: f(xv[:k] + [t] + xv[k + 1:], sv, m)[j], xv[k]))
    return H


FAMILY = {"family3": ("car_obs", 3, FAMILY_NY, 3, _family3,
                      dict(sym=_Sympy(), h=lambda x, s: mp_h("family3", x, s), jacobian=lambda x, s: mp_jacobian("family3", x, s)))}
N.register(SIZE_SENSORS)
N.register(FAMILY)
KEYS = list(SIZE_SENSORS) + list(FAMILY)
B = 70


def family_states():
    """x [70, 3] in [-1.5, 1.5]³ from a fixed generator; instances 0 .. 7 placed on the bearing atan2(x1 − s1, x0 − s0) of the shared
    beacon: one per quadrant, x0 = s0 exactly (atan2(±d, 0)), and x0 − s0 < 0 with x1 − s1 = ±1e-6, the two sides of the branch cut"""
    x = np.random.default_rng(20261103).uniform(-1.5, 1.5, (B, 3))
    s0, s1 = N.s_shared("family3")[:2]
    x[:8] = [[s0 + 0.7, s1 + 0.5, 0.4], [s0 - 0.6, s1 + 0.8, -0.5], [s0 - 0.5, s1 - 0.9, 0.7], [s0 + 0.8, s1 - 0.4, -0.3],
             [s0, s1 + 0.6, 0.5], [s0, s1 - 0.6, -0.6], [s0 - 0.7, s1 + 1.0e-6, 0.3], [s0 - 0.7, s1 - 1.0e-6, -0.8]]
    return x


# ------------------------------------------------------------------------------------------------------------- the inputs
def some(key, B_):
    """the instances compared with the yardstick: the first and last of each wave; of the family also every hand-placed one"""
    if B_ <= 3:
        return tuple(range(B_))
    return tuple(range(8)) + (63, 64, 69) if key in FAMILY else (0, 1, 63, 64, 69)


def s_shared(key):
    return N.s_shared(key)


def s_instances(key, B_):
    """[B, ns] as sensor_nl_ref's; the family's hand-placed instances keep the shared beacon, which is what places them"""
    s = N.s_instances(key, B_)
    if key in FAMILY:
        s[:8, :2] = N.s_shared(key)[:2]
    return s


def inputs(key, B_=B):
    """(x̂ [B, nx], P [B, nx, nx], x_prior [B, nx], the states the readings are taken of [B, nx]) without a device: estimator_ref's
    start and p_start around the sweep's x1; the family's own states, read where they are (a state moved by 0.03 would cross the
    branch cut the inputs are placed on)"""
    nx = N.dims(key)[0]
    if key in FAMILY:
        xh = family_states()[:B_]
        return xh, E.p_start(B_, nx), E.start(xh, nx)[1], xh
    x1 = M.sweep_inputs(*SIZE_SENSORS[key][0], B=B, T=M.T_SWEEP)[0][:B_]
    xh, ys = E.start(x1, nx)
    return xh, E.p_start(B_, nx), ys, ys


def readings(key, states, s):
    """y [B, ny] as sensor_nl_ref.readings. The family's bearing instead reads 0.02 rad nearer to zero than h_0 of the state: the
    update then turns every estimate away from the cut at ±π, and the innovation stays a small angle the library may subtract plainly"""
    y = N.readings(key, states, s)
    if key in FAMILY:
        h0 = np.array([N.h(key, states[b], s if np.ndim(s) == 1 else s[b])[0] for b in range(states.shape[0])])
        y[:, 0] = h0 - 0.02 * np.sign(h0)
    return y
