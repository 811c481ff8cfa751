"""The device staging of the host forms — ilqr_rollout_policy, ilqr_initialize_rollout_candidates, ilqr_sample_rollout_candidates,
ilqr_shift_horizon — reused across calls of different size on ONE handle: sample / candidate counts 3, then 70 (a second wave;
every stage has to grow), then 3 again (every stage is larger than the call needs), each count once with every optional output
null and once with every optional output given. The null calls go through the C ABI directly: the wrappers always ask for the
scores.

Bound: none. Every call is compared with the same call on a fresh handle prepared identically, whose stages are allocated for
exactly that call, and the comparison is array_equal: the same kernels run on the same inputs with the same launch geometry, and
they use no atomics. The two handles' output arrays are pre-filled with different values, so an output that was not written at
all does not compare equal either.

Models: acrobot (small form) T = 6 and synth12 (large form) T = 4, B = 2. Neither has parameters, so the two stages that hold
parameters — the policy rollout's per-sample w and the shift's w_tail — are exercised on car_obs (two parameters), T = 6.
"""
import ctypes as C

import numpy as np
import pytest

import candidates_ref as CR
import policy_ref as P
import shift_ref as R
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
B = 2
HORIZON = {"acrobot": 6, "synth12": 4, "car_obs": 6}
COUNTS = (3, 70, 3)
I32, F64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    return p


def _inputs(pkg, name):
    """(x1 [B, nx], ū [B, T-1, nu], w [B, T, 2] or None): the workload's, cut to the short horizon"""
    T = HORIZON[name]
    _, _, x1, ub = pkg.workloads.make_inputs(name, B)
    w = np.ascontiguousarray(R.time_varying(pkg.workloads.make_parameters(name, B))[:, :T]) if name == "car_obs" else None
    return x1, np.ascontiguousarray(ub[:, :T - 1]), w


def _handle(pkg, name, solved=False):
    """a handle of the case, every one prepared the same way"""
    opts = pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(name, {}))
    sol = pkg.Solver(model=pkg.workloads.CONFIGS[name][0], horizon=HORIZON[name], batch=B, options=opts)
    x1, ub, w = _inputs(pkg, name)
    if w is not None:
        sol.set_parameters_(w)
    if solved:
        sol.initialize_rollout_(x1, ub)
        sol.solve_()
    return sol


def _ptr(out, key):
    a = out.get(key)
    return None if a is None else a.ctypes.data_as(I32 if a.dtype == np.int32 else F64)


def _in(a):
    return None if a is None else a.ctypes.data_as(F64)


def _outputs(shapes, full, required, fill):
    """the output arrays of one call, pre-filled: the required ones, and the optional ones when `full`"""
    return {k: np.full(shape, fill, dtype=dt) for k, (shape, dt) in shapes.items() if full or k in required}


def _installed(sol):
    return sol.get_trajectory() + (sol.buffer("parameters"), sol.buffer("states"), sol.scalar("states_eq_nominal"))


def _same(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in sorted(a) if not np.array_equal(a[k], b[k], equal_nan=True)]


def _eq(p, q):
    return len(p) == len(q) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, q))


def _rollout_policy(pkg, sol, x1, w, full, fill):
    S, T = x1.shape[1], sol.T
    out = _outputs(dict(cost=((B, S), np.float64), max_violation=((B, S), np.float64), first_nonfinite=((B, S), np.int32),
                        x=((B, S, T, sol.nx), np.float64), u=((B, S, T - 1, sol.nu), np.float64)), full, ("cost",), fill)
    p = lambda k: _ptr(out, k)
    pkg._ffi.check(pkg._ffi.lib().ilqr_rollout_policy(sol._h, S, 0.5, x1.ctypes.data_as(F64), None if w is None else w.ctypes.data_as(F64),
                                                      p("cost"), p("max_violation"), p("first_nonfinite"), p("x"), p("u")))
    return out


def _score_candidates(pkg, sol, x1, u, full, fill):
    S = u.shape[1]
    out = _outputs(dict(chosen=((B,), np.int32), cost=((B, S), np.float64), max_violation=((B, S), np.float64),
                        first_nonfinite=((B, S), np.int32)), full, (), fill)
    p = lambda k: _ptr(out, k)
    pkg._ffi.check(pkg._ffi.lib().ilqr_initialize_rollout_candidates(sol._h, S, 0.5, x1.ctypes.data_as(F64), u.ctypes.data_as(F64),
                                                                     p("chosen"), p("cost"), p("max_violation"), p("first_nonfinite")))
    return out


def _sample_candidates(pkg, sol, S, x1, base, sigma, full, fill):
    """x1, base: arrays, or None for the handle's resident inputs"""
    out = _outputs(dict(chosen=((B,), np.int32), cost=((B, S), np.float64), max_violation=((B, S), np.float64),
                        first_nonfinite=((B, S), np.int32), weights=((B, S), np.float64), u=((B, S, sol.T - 1, sol.nu), np.float64)), full, (), fill)
    p = lambda k: _ptr(out, k)
    pkg._ffi.check(pkg._ffi.lib().ilqr_sample_rollout_candidates(                    # blend: the weights are needed whether asked for or not
        sol._h, S, 1, 20251019, 0, sigma.ctypes.data_as(F64), 0.5, 1.0, _in(x1), _in(base),
        p("chosen"), p("cost"), p("max_violation"), p("first_nonfinite"), p("weights"), p("u")))
    return out


@pytest.mark.parametrize("name", ["acrobot", "synth12", "car_obs"])
def test_policy_rollout_reuses_its_staging(pkg, name):
    """x1, cost and (full calls) max_violation, first_nonfinite, x, u; on car_obs the full calls also bring per-sample w"""
    size = P.CASES[name][2]
    one = _handle(pkg, name, solved=True)
    xb = one.get_trajectory()[0]
    w = _inputs(pkg, name)[2]
    for call, S in enumerate(COUNTS):
        x1 = np.stack([P.perturbed_starts(xb[b, 0], S, size, seed=P.SEED + b) for b in range(B)])
        ws = None if w is None else np.stack([P.sample_parameters(w[b], S, seed=P.SEED + 100 + b) for b in range(B)])
        for full in (False, True):
            fresh = _handle(pkg, name, solved=True)
            got = _rollout_policy(pkg, one, x1, ws if full else None, full, -1)
            want = _rollout_policy(pkg, fresh, x1, ws if full else None, full, -2)
            assert _same(got, want) == [], (name, call, S, full)
            assert sorted(got) == (["cost", "first_nonfinite", "max_violation", "u", "x"] if full else ["cost"])
            fresh.close()
    one.close()


@pytest.mark.parametrize("name", ["acrobot", "synth12"])
def test_candidate_scoring_reuses_its_staging(pkg, name):
    """u and (full calls) chosen, cost, max_violation, first_nonfinite; the null calls score into the handle's own buffers —
    the same stages — and are seen through the state they install"""
    size = CR.CASES[name][2]
    x1, ub, _ = _inputs(pkg, name)
    one = _handle(pkg, name)
    for call, S in enumerate(COUNTS):
        u = np.stack([CR.candidates(ub[b], S, size, b) for b in range(B)])
        for full in (False, True):
            fresh = _handle(pkg, name)
            got = _score_candidates(pkg, one, x1, u, full, -3)
            want = _score_candidates(pkg, fresh, x1, u, full, -4)
            assert _same(got, want) == [], (name, call, S, full)
            assert len(got) == (4 if full else 0)
            assert _eq(_installed(one), _installed(fresh)), (name, call, S, full)
            fresh.close()
    one.close()


@pytest.mark.parametrize("name", ["acrobot", "synth12"])
def test_candidate_sampling_reuses_its_staging(pkg, name):
    """(full calls) chosen, cost, max_violation, first_nonfinite, weights and the candidates as drawn; the null calls are seen
    through the blend they install, which needs every score and weight of the handle's own buffers"""
    x1, ub, _ = _inputs(pkg, name)
    one = _handle(pkg, name)
    sigma = CR.CASES[name][2] * (1.0 + np.arange(one.nu))
    for call, S in enumerate(COUNTS):
        for full in (False, True):
            fresh = _handle(pkg, name)
            got = _sample_candidates(pkg, one, S, x1, ub, sigma, full, -5)
            want = _sample_candidates(pkg, fresh, S, x1, ub, sigma, full, -6)
            assert _same(got, want) == [], (name, call, S, full)
            assert len(got) == (6 if full else 0)
            assert _eq(_installed(one), _installed(fresh)), (name, call, S, full)
            got = _sample_candidates(pkg, one, S, None, None, sigma, full, -7)       # around the resident inputs: what was just installed
            want = _sample_candidates(pkg, fresh, S, None, None, sigma, full, -8)
            assert _same(got, want) == [] and _eq(_installed(one), _installed(fresh)), (name, call, S, full, "resident")
            fresh.close()
    one.close()


def test_shift_reuses_its_staging(pkg):
    """car_obs: x1 and w_tail given at steps 1, 3, 1 (w_tail is [B][steps][2]: grows, then is oversized), and both null"""
    name, size = "car_obs", P.CASES["car_obs"][2]
    one = _handle(pkg, name, solved=True)
    xb, ub = one.get_trajectory()
    w = _inputs(pkg, name)[2]
    for call, (steps, given) in enumerate(((1, True), (1, False), (3, True), (3, False), (1, True))):
        x1 = np.stack([R.measured_start(xb[b, steps], size, b, steps) for b in range(B)]) if given else None
        w_tail = w[:, -1:] + 0.03 * (1.0 + np.arange(steps))[None, :, None] if given else None
        fresh = _handle(pkg, name, solved=True)
        one.set_buffer("nominal_states", xb); one.set_buffer("nominal_actions", ub); one.set_parameters_(w)       # back to the solved state
        assert _eq(_installed(one)[:3], _installed(fresh)[:3])
        one.shift_horizon_(steps, x1=x1, w_tail=w_tail)
        fresh.shift_horizon_(steps, x1=x1, w_tail=w_tail)
        assert _eq(_installed(one), _installed(fresh)), (call, steps, given)
        if given:
            assert np.array_equal(one.get_trajectory()[0][:, 0], x1)
            assert np.array_equal(one.buffer("parameters").reshape(B, -1, 2)[:, -steps:], w_tail)
        fresh.close()
    one.close()
