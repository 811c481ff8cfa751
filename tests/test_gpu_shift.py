"""ilqr_shift_horizon on the GPU against the numpy slicing and the CPU oracle (tests/shift_ref.py; the yardstick itself and the
properties of the inputs used here are checked without a GPU in tests/test_shift_abi.py).

Bounds, fixed before the kernels ran. Open loop: everything is a copy followed by the existing init_rollout kernel, so the
installed state is array_equal to that of a second handle given the sliced inputs through set_parameters_ + initialize_rollout_.
Closed loop: u' and x' of the head within 1e-10 relative to max(1, max |reference|), the forward-stage bound of
tests/test_gpu_parity.py and of the policy tests. Whether the perturbed, shifted closed loop needs more was measured on the
oracle alone (tests/test_shift_abi.py): its recursion on the sliced arrays run a second time with x1 moved by one part in 1e15
moves x, u by at most 5.5e-15 (acrobot), 5.7e-15 (car_obs), 1.3e-15 (synth12) over the instances and steps used here; ten times that
stays far below 1e-10. The tail of u' is ū's last row (or 0) exactly. No instance looked at is left out: the perturbation
sizes (policy_ref.CASES) keep the oracle finite on all of them, which the test asserts.

One slot of the named scalars belongs to the installed state: states_eq_nominal is cleared by every initialiser, this one
included; it is compared with the second handle's. Every other scalar of the shifted handle is bitwise what it was.
"""
import os
import subprocess

import numpy as np
import pytest

import policy_ref as P
import shift_ref as R
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["acrobot", "car_obs", "synth12", "particle"]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    assert hasattr(p._ffi.lib(), "ilqr_shift_horizon"), "the library has no ilqr_shift_horizon"
    return p


def _user_particle(pkg, T, B, **kw):
    xT = [1.0, 0.0]
    dyn = pkg.Dynamics(lambda x, u: [x[0] + x[1], x[1] + u[0]], 2, 1)
    stage = pkg.Cost(lambda x, u: 0.1 * (x[0] * x[0] + x[1] * x[1]) + 0.1 * u[0] * u[0], 2, 1)
    term = pkg.Cost(lambda x, u: 0.1 * (x[0] * x[0] + x[1] * x[1]), 2, 0)
    goal = pkg.Constraint(lambda x, u: [x[0] - xT[0], x[1] - xT[1]], 2, 0)
    none = pkg.Constraint()
    return pkg.Solver([dyn] * (T - 1), [stage] * (T - 1) + [term], [none] * (T - 1) + [goal], batch=B,
                      options=pkg.Options(verbose=0), name="user_particle", **kw)


def _batch(name):
    return 2 if name == "synth12" else 70          # 70: a second, ragged wave of the one-lane-per-instance kernels


def _handle(pkg, name, B, **kw):
    cfg, T, size = P.CASES[name]
    model = pkg.workloads.CONFIGS[cfg][0]
    opts = pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(cfg, {}))
    return _user_particle(pkg, T, B, **kw) if name == "particle" else pkg.Solver(model=model, horizon=T, batch=B, options=opts, **kw)


def _solved(pkg, name, B, **kw):
    """a solved handle of the case: (sol, model, T, size, w); car_obs under time-varying parameters (the workload's + 0.01 · t)"""
    cfg, T, size = P.CASES[name]
    model, T_, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T_ == T
    sol = _handle(pkg, name, B, **kw)
    w = None
    if name == "car_obs":
        w = R.time_varying(pkg.workloads.make_parameters(cfg, B))
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol, model, T, size, w


class _Snapshot:
    """what a shift reads of a solved handle, and the way back to it"""

    def __init__(self, sol, w):
        self.xb, self.ub = sol.get_trajectory()
        self.K = sol.get_policy()[0]
        self.w = w

    def restore(self, sol):
        sol.set_buffer("nominal_states", self.xb)
        sol.set_buffer("nominal_actions", self.ub)
        if self.w is not None:
            sol.set_parameters_(self.w)

    def expected(self, k, tail, x1=None, w_tail=None):
        """shift_ref.shifted_inputs per instance: (x1' [B, n], u' [B, T-1, m], w' or None)"""
        B = self.xb.shape[0]
        rs = [R.shifted_inputs(self.xb[b], self.ub[b], None if self.w is None else self.w[b], k, tail,
                               None if x1 is None else x1[b], None if w_tail is None else w_tail[b]) for b in range(B)]
        return np.stack([r[0] for r in rs]), np.stack([r[1] for r in rs]), None if self.w is None else np.stack([r[2] for r in rs])


def _install(ref, x1p, up, wp):
    if wp is not None:
        ref.set_parameters_(wp)
    ref.initialize_rollout_(x1p, up)


def _installed(sol):
    return sol.get_trajectory() + (sol.buffer("parameters"), sol.buffer("states"), sol.scalar("states_eq_nominal"))


def _core(sol):
    """the installed state without `states` (the last line-search trial of the solve: handles that split the batch differently
    may run different solve kernels)"""
    v = _installed(sol)
    return v[:3] + v[4:]


def _untouched(sol, pkg):
    sc = sol.buffer("_scalars").copy()
    sc[:, pkg._ffi.lib().ilqr_scalar_slot(b"states_eq_nominal")] = 0.0
    return sol.get_policy() + (sol.buffer("constraint_dual"), sol.buffer("constraint_penalty"), sc)


def _eq(p, q):
    return len(p) == len(q) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, q))


def _starts(snap, k, size):
    return np.stack([R.measured_start(snap.xb[b, k], size, b, k) for b in range(snap.xb.shape[0])])


@pytest.mark.parametrize("name", NAMES)
def test_open_loop_is_bitwise(pkg, name):
    """k in {0, 1, 3, T−1}, both tails, x1 given and not, car_obs with and without w_tail: trajectory, parameters and states equal
    those of a second solved handle given shift_ref.shifted_inputs; K, k, duals, penalties and the scalars stay."""
    B = _batch(name)
    a, model, T, size, w = _solved(pkg, name, B)
    b, _, _, _, _ = _solved(pkg, name, B)
    snap = _Snapshot(a, w)
    assert np.array_equal(a.buffer("states"), b.buffer("states")) and np.array_equal(a.get_policy()[0], b.get_policy()[0])
    keep = _untouched(a, pkg)
    rng = np.random.default_rng(P.SEED)
    for k in (0, 1, 3, T - 1):
        for tail in ("hold", "zero"):
            for given in (False, True):
                for with_tail in ((False, True) if (w is not None and k > 0) else (False,)):
                    x1 = snap.xb[:, k] + size * rng.standard_normal(snap.xb[:, k].shape) if given else None
                    w_tail = 0.3 + 0.1 * rng.standard_normal((B, k, w.shape[2])) if with_tail else None
                    snap.restore(a)
                    a.shift_horizon_(k, x1=x1, tail=tail, w_tail=w_tail)
                    x1p, up, wp = snap.expected(k, tail, x1, w_tail)
                    _install(b, x1p, up, wp)
                    tag = (name, k, tail, given, with_tail)
                    assert _eq(_installed(a), _installed(b)), tag
                    assert np.array_equal(a.get_trajectory()[1], up) and np.array_equal(a.get_trajectory()[0][:, 0], x1p), tag
                    assert _eq(keep, _untouched(a, pkg)), tag
    a.close(); b.close()


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_replay_from_the_resident_inputs(pkg, name):
    B = _batch(name)
    a, model, T, size, w = _solved(pkg, name, B)
    snap = _Snapshot(a, w)
    a.shift_horizon_(3, x1=_starts(snap, 3, size), feedback=True)
    first = _installed(a)
    a.set_buffer("nominal_states", np.zeros_like(snap.xb)); a.set_buffer("nominal_actions", np.ones_like(snap.ub))
    a.initialize_rollout_resident_()
    assert _eq(first, _installed(a))
    a.reset_(); a.initialize_rollout_resident_()          # a fresh solver's state (the parameters stay), then the shifted inputs again
    assert _eq(first[:3], _installed(a)[:3])
    a.close()


@pytest.mark.parametrize("name", NAMES)
def test_closed_loop_parity_with_the_oracle(pkg, oracle, name):
    """x1 = x̄_k + size · N(0, 1), k in {1, 3}: the head of u' and x' against shift_ref.feedback_head on instances 0, 63, 64, 69
    (synth12: 0, 1), the tail equal to ū's last row, and the whole installed state that of initialize_rollout_(x1, u')."""
    B = _batch(name)
    a, model, T, size, w = _solved(pkg, name, B)
    ref = _handle(pkg, name, B)
    snap = _Snapshot(a, w)
    N = T - 1
    worst = dict(x=0.0, u=0.0)
    for k in (1, 3):
        x1 = _starts(snap, k, size)
        snap.restore(a)
        a.shift_horizon_(k, x1=x1, feedback=True)
        xs, us = a.get_trajectory()
        assert np.isfinite(xs).all() and np.isfinite(us).all()
        _, up, wp = snap.expected(k, "hold", x1)
        assert np.array_equal(xs[:, 0], x1) and np.array_equal(us[:, N - k:], up[:, N - k:])        # the tail: ū_{N-1}, no feedback
        if wp is not None:
            assert np.array_equal(a.buffer("parameters").reshape(wp.shape), wp)
        _install(ref, x1, us, wp)
        assert _eq(_installed(a)[:3], _installed(ref)[:3]), (name, k)
        for b in sorted({0, 63, 64, 69} & set(range(B)) | ({0, 1} if B == 2 else set())):
            r = R.feedback_head(oracle, model, T, snap.xb[b], snap.ub[b], snap.K[b], None if wp is None else wp[b], k, x1[b])
            assert r["first_nonfinite"] == -1, (name, k, b)          # the perturbation keeps the oracle finite: nobody is left out
            worst["x"] = max(worst["x"], P.rel(xs[b, :T - k], r["x"])); worst["u"] = max(worst["u"], P.rel(us[b, :N - k], r["u"]))
            assert np.abs(us[b, :N - k] - snap.ub[b, k:]).max() > 1e-6, (name, k, b)               # not the open-loop shift
    print("shift closed-loop parity %s: %s" % (name, worst))
    assert worst["x"] < TOL and worst["u"] < TOL, worst
    a.close(); ref.close()


@pytest.mark.parametrize("name", NAMES)
def test_feedback_from_the_nominal_state_reduces_to_the_open_loop_shift(pkg, name):
    B = _batch(name)
    a, model, T, size, w = _solved(pkg, name, B)
    snap = _Snapshot(a, w)
    for k, tail in ((0, "hold"), (1, "zero"), (3, "hold")):
        snap.restore(a)
        a.shift_horizon_(k, feedback=True, tail=tail)
        xs, us = a.get_trajectory()
        x1p, up, _ = snap.expected(k, tail)
        assert np.array_equal(xs[:, 0], x1p) and np.array_equal(us[:, T - 1 - k:], up[:, T - 1 - k:])
        assert P.rel(us, up) < TOL, (name, k, P.rel(us, up))       # the deviation term is rounding only
    a.close()


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_instances_are_independent(pkg, name):
    """Instance b of the batch and the same instance alone in a B = 1 handle (its x̄, ū, K, parameters loaded through set_buffer)
    install bitwise the same trajectory; a NaN in one instance's x1 leaves every other instance bitwise unchanged."""
    B = _batch(name)
    a, model, T, size, w = _solved(pkg, name, B)
    snap = _Snapshot(a, w)
    k = 2
    x1 = _starts(snap, k, size)
    a.shift_horizon_(k, x1=x1, feedback=True)
    full = _installed(a)[:3]
    one = _handle(pkg, name, 1)
    for b in sorted({0, 63, 64, 69} & set(range(B)) | ({1} if B == 2 else set())):
        one.set_buffer("nominal_states", snap.xb[b]); one.set_buffer("nominal_actions", snap.ub[b]); one.set_buffer("K", snap.K[b])
        if w is not None:
            one.set_parameters_(w[b:b + 1])
        one.shift_horizon_(k, x1=x1[b:b + 1], feedback=True)
        assert _eq([v[b:b + 1] for v in full], _installed(one)[:3]), (name, b)
    one.close()
    bad = B // 2
    x1n = x1.copy()
    x1n[bad, 0] = np.nan
    snap.restore(a)
    a.shift_horizon_(k, x1=x1n, feedback=True)
    out = _installed(a)[:3]
    others = np.arange(B) != bad
    assert _eq([v[others] for v in full], [v[others] for v in out])
    assert np.isnan(out[0][bad]).any() and np.isnan(out[1][bad]).any()
    a.close()


def test_host_form_device_form_and_sharded_handle_agree(pkg):
    import torch
    name, B, k = "car_obs", 5, 2
    sol, model, T, size, w = _solved(pkg, name, B)
    snap = _Snapshot(sol, w)
    x1 = _starts(snap, k, size)
    w_tail = 0.3 + 0.1 * np.random.default_rng(P.SEED).standard_normal((B, k, w.shape[2]))
    dv, _, _, _, _ = _solved(pkg, name, B)
    sh, _, _, _, _ = _solved(pkg, name, B, devices=[0, 0])
    for other in (dv, sh):
        assert _eq(other.get_trajectory() + other.get_policy(), sol.get_trajectory() + sol.get_policy())
    for feedback in (False, True):
        for s in (sol, dv, sh):
            snap.restore(s)
        sol.shift_horizon_(k, x1=x1, feedback=feedback, tail="zero", w_tail=w_tail)
        host = _core(sol)
        dev = torch.device("cuda:0")
        with torch.cuda.stream(torch.cuda.ExternalStream(dv.stream_ptr())):
            d_x1, d_wt = torch.from_numpy(x1).to(dev), torch.from_numpy(w_tail).to(dev)
        torch.cuda.synchronize()
        dv.shift_horizon_device_(k, d_x1.data_ptr(), feedback=feedback, tail="zero", d_w_tail_ptr=d_wt.data_ptr())
        dv.synchronize()
        assert _eq(host, _core(dv)), feedback
        sh.shift_horizon_(k, x1=x1, feedback=feedback, tail="zero", w_tail=w_tail)
        assert _eq(host, _core(sh)), feedback
        sh.set_buffer("nominal_actions", np.zeros_like(snap.ub)); sh.initialize_rollout_resident_()
        assert _eq(host[:3], _installed(sh)[:3]), feedback
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        sh.shift_horizon_device_(k, d_x1.data_ptr())
    sol.close(); dv.close(); sh.close()


def test_refusals_that_need_a_handle(pkg):
    B = 2
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub)
    before = sol.get_trajectory()
    L = pkg._ffi.lib()
    with pytest.raises(pkg._ffi.IlqrError, match="no policy"):
        sol.shift_horizon_(1, feedback=True)
    with pytest.raises(pkg._ffi.IlqrError, match="no parameters"):
        sol.shift_horizon_(1, w_tail=np.zeros((B, 1, 1)))
    assert L.ilqr_shift_horizon(sol._h, T, 0, 0, None, None) == -1 and b"steps must lie in 0 .. T-1" in L.ilqr_last_error()
    for bad in (dict(steps=T), dict(steps=-1), dict(tail="wrap"), dict(x1=np.zeros((B, sol.nx + 1)))):
        with pytest.raises(ValueError):
            sol.shift_horizon_(**bad)
    assert _eq(before, sol.get_trajectory())                     # a refused call leaves the handle alone
    sol.shift_horizon_(1)                                        # the open-loop shift needs no policy
    assert np.array_equal(sol.get_trajectory()[1][:, :-1], before[1][:, 1:])
    sol.run_stage_("cost_nominal"); sol.run_stage_("gradients"); sol.run_stage_("backward_pass")
    sol.shift_horizon_(1, feedback=True)                         # a backward-pass stage makes a policy
    sol.reset_()
    with pytest.raises(pkg._ffi.IlqrError, match="no policy"):
        sol.shift_horizon_(0, x1=x1, feedback=True)
    sol.close()
    # a lowered problem: its structure belongs to horizon positions
    Tl = 51
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    dynamics, costs, constraints = pkg.models.car_tv(Tl)
    low = pkg.Solver(stage_sources=pkg.lowering.c_stage_sources(dynamics, costs, constraints), batch=B, options=pkg.Options(verbose=0),
                     name="car_tv_c")
    low.initialize_rollout_(x1, ub)
    with pytest.raises(pkg._ffi.IlqrError, match="stage selectors"):
        low.shift_horizon_(1)
    low.shift_horizon_(0, x1=x1 + 0.01)                          # steps == 0 moves nothing across horizon positions
    assert np.array_equal(low.get_trajectory()[0][:, 0], x1 + 0.01) and np.array_equal(low.get_trajectory()[1], ub)
    low.close()


def test_plain_c_example(pkg, tmp_path):
    """examples/mpc_shift.c: five periods of solve, shift with the perturbed next state, re-solve — from plain C"""
    exe = str(tmp_path / "mpc_shift")
    libdir = os.path.join(ROOT, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "mpc_shift.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe, "16"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].startswith("period 0: first solve") and sum(l.startswith("period ") for l in lines) == 6
    assert "mpc shift check passed" in out.stdout
