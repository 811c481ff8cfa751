"""ilqr_rollout_policy on the GPU against the CPU oracle (tests/policy_ref.py; its two readings are checked against each other
without a GPU in tests/test_policy_rollout_abi.py).

Bounds, fixed before the kernel ran. States and actions: the forward-stage bound of tests/test_gpu_parity.py, 1e-10 relative to
max(1, max |reference|). Whether a perturbed closed loop needs more was measured on the oracle alone: its recursion run a second
time with x1 moved by one part in 1e15 moves x, u by at most 1.2e-14 (acrobot), 5.7e-15 (car), 5.7e-15 (car_obs), 3.9e-16
(particle), 2.0e-15 (synth12) over the samples used here; ten times that stays far below 1e-10, so 1e-10 holds for every model.
cost: 1e-9 relative — a sum of quadratics of x, u moves by at most twice their relative error per term, with a factor five for
cancellation between terms; max_violation: 1e-9 absolute per unit of max(1, |violation|), the constraints being as smooth.
first_nonfinite: equal. No sample is left out: the perturbation sizes (policy_ref.CASES) keep every oracle sample finite, which
the tests assert.
"""
import os
import subprocess

import numpy as np
import pytest

import policy_ref as R
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU, TOL_COST, TOL_VIOL = 1e-10, 1e-9, 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
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


def _solved(pkg, name, B, **kw):
    """a solved handle of the case and its inputs: (sol, model, T, size, w)"""
    cfg, T, size = R.CASES[name]
    model, T_, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T_ == T
    opts = pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(cfg, {}))
    sol = _user_particle(pkg, T, B, **kw) if name == "particle" else pkg.Solver(model=model, horizon=T, batch=B, options=opts, **kw)
    w = None
    if name == "car_obs":
        w = pkg.workloads.make_parameters(cfg, B)
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol, model, T, size, w


def _starts(sol, S, size):
    xb, _ = sol.get_trajectory()
    return np.stack([R.perturbed_starts(xb[b, 0], S, size, seed=R.SEED + b) for b in range(sol.B)])


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("name", ["acrobot", "car", "car_obs", "particle", "synth12"])
def test_parity_with_the_oracle(pkg, oracle, name):
    """Every sample of every instance: x, u, cost, max_violation, first_nonfinite against the oracle's rollout! driven off-nominal
    (bounds: module docstring). S = 70: two waves, the last one ragged."""
    B, S = (3, 70) if name != "synth12" else (2, 70)
    sol, model, T, size, w = _solved(pkg, name, B)
    xb, ub = sol.get_trajectory()
    K, _ = sol.get_policy()
    x1 = _starts(sol, S, size)
    ws = np.stack([R.sample_parameters(w[b], S, seed=R.SEED + 100 + b) for b in range(B)]) if w is not None else None
    out = sol.rollout_policy(x1, w=ws, trajectories=True)
    lean = sol.rollout_policy(x1, w=ws)
    assert set(lean) == {"cost", "max_violation", "first_nonfinite"} and _same(lean, {k: out[k] for k in lean})
    worst = dict(x=0.0, u=0.0, cost=0.0, viol=0.0)
    for b in range(B):
        for s in range(S):
            ref = R.oracle_reading(oracle, model, T, xb[b], ub[b], K[b], x1[b, s], None if ws is None else ws[b, s])
            assert ref["first_nonfinite"] == -1, (b, s)              # the perturbation keeps the oracle finite: nobody is left out
            assert out["first_nonfinite"][b, s] == -1, (b, s)
            assert np.array_equal(out["x"][b, s, 0], x1[b, s])
            worst["x"] = max(worst["x"], R.rel(out["x"][b, s], ref["x"])); worst["u"] = max(worst["u"], R.rel(out["u"][b, s], ref["u"]))
            worst["cost"] = max(worst["cost"], abs(out["cost"][b, s] - ref["cost"]) / max(1.0, abs(ref["cost"])))
            worst["viol"] = max(worst["viol"], abs(out["max_violation"][b, s] - ref["max_violation"]) / max(1.0, abs(ref["max_violation"])))
    print("policy rollout parity %s: %s" % (name, worst))
    assert worst["x"] < TOL_XU and worst["u"] < TOL_XU, worst
    assert worst["cost"] < TOL_COST and worst["viol"] < TOL_VIOL, worst
    if name != "particle":
        assert (out["max_violation"] > 0).any()                    # a constrained handle reports violations off the nominal path
    sol.close()


def test_unconstrained_handle_reports_zero_violation(pkg):
    B, S = 2, 5
    model, T, x1, ub = pkg.workloads.make_inputs("car", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0), constraints=False)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    out = sol.rollout_policy(_starts(sol, S, 0.05))
    assert (out["max_violation"] == 0.0).all() and np.isfinite(out["cost"]).all()
    sol.close()


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_reduces_to_the_references_rollout(pkg, oracle, alpha):
    """x1 = x̄_1 and step_size = α: the oracle's unmodified rollout!(α) after its backward pass, on identical inputs (x̄, ū, K, k
    copied from the oracle into the handle, as the stage parity test does)."""
    B = 2
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub)
    refs = []
    for b in range(B):
        pr = oracle.Problem(model, T)
        s = oracle.Solver(pr, oracle.default_options())
        s.initialize_controls(ub[b]); s.initialize_states(pr.rollout(x1[b], ub[b]))
        s.call("reset_model_objective"); s.call("cost_bang", 0); s.call("gradients"); s.call("backward_pass")
        refs.append(s)
    for nm in ("nominal_states", "nominal_actions", "K", "k"):
        sol.set_buffer(nm, np.stack([r.buffer(nm) for r in refs]))
    xb, _ = sol.get_trajectory()
    out = sol.rollout_policy(xb[:, :1, :], step_size=alpha, trajectories=True)
    for b, r in enumerate(refs):
        r.call("rollout_bang", alpha)
        assert R.rel(out["x"][b, 0].ravel(), r.buffer("states")) < TOL_XU and R.rel(out["u"][b, 0].ravel(), r.buffer("actions")) < TOL_XU
        assert np.abs(out["u"][b, 0].ravel() - r.buffer("nominal_actions")).max() > 1e-3        # k matters: not the tracking rollout
    sol.close()


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_samples_are_independent_and_calls_repeat(pkg, name):
    B, S = 2, 257 if name != "synth12" else 9
    sol, model, T, size, w = _solved(pkg, name, B)
    x1 = _starts(sol, S, size)
    ws = np.stack([R.sample_parameters(w[b], S) for b in range(B)]) if w is not None else None
    full = sol.rollout_policy(x1, w=ws, step_size=0.25, trajectories=True)
    assert _same(full, sol.rollout_policy(x1, w=ws, step_size=0.25, trajectories=True))
    for s in sorted({0, 63, 64, S // 2, S - 1} & set(range(S))):
        one = sol.rollout_policy(x1[:, s:s + 1], w=None if ws is None else ws[:, s:s + 1], step_size=0.25, trajectories=True)
        assert _same(one, {k: v[:, s:s + 1] for k, v in full.items()}), s
    sol.close()


def test_the_call_only_reads_the_handle(pkg):
    B, S = 6, 70
    a, model, T, size, _ = _solved(pkg, "car", B)
    b, _, _, _, _ = _solved(pkg, "car", B)
    snap = lambda s: (s.get_trajectory(), s.get_policy(), s.buffer("_scalars"), s.stats(), s.timing())
    before = snap(a)
    a.rollout_policy(_starts(a, S, size), step_size=0.5, trajectories=True)
    after = snap(a)
    for p, q in zip(before[:2], after[:2]):
        assert np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
    assert np.array_equal(before[2], after[2]) and before[4][1] == after[4][1]
    assert all(np.array_equal(before[3][k], after[3][k]) for k in before[3])
    a.solve_(); b.solve_()              # a second solve is what it would have been without the call
    assert np.array_equal(a.get_trajectory()[0], b.get_trajectory()[0]) and np.array_equal(a.get_policy()[0], b.get_policy()[0])
    sa, sb = a.stats(), b.stats()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    a.close(); b.close()


def test_a_non_finite_sample_is_contained(pkg, oracle):
    """One sample starts with joint velocities of 1e200: the squared velocities of the acrobot's dynamics overflow (arithmetic, no
    fault), in the oracle as well. It reports the oracle's first_nonfinite; every other sample is bitwise what it is without it."""
    B, S, bad = 2, 70, 37
    sol, model, T, size, _ = _solved(pkg, "acrobot", B)
    xb, ub = sol.get_trajectory()
    K, _ = sol.get_policy()
    x1 = _starts(sol, S, size)
    clean = sol.rollout_policy(x1, trajectories=True)
    x1b = x1.copy()
    x1b[:, bad, 2:] = 1.0e200
    out = sol.rollout_policy(x1b, trajectories=True)
    keep = np.arange(S) != bad
    assert _same({k: v[:, keep] for k, v in out.items()}, {k: v[:, keep] for k, v in clean.items()})
    for b in range(B):
        ref = R.oracle_reading(oracle, model, T, xb[b], ub[b], K[b], x1b[b, bad])
        assert ref["first_nonfinite"] >= 1                          # the oracle's recursion goes non-finite too
        assert out["first_nonfinite"][b, bad] == ref["first_nonfinite"], (b, out["first_nonfinite"][b, bad], ref["first_nonfinite"])
    assert (out["first_nonfinite"][:, keep] == -1).all()
    sol.close()


def test_refusals_that_need_a_handle(pkg):
    B = 2
    model, T, x1, ub = pkg.workloads.make_inputs("car", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub)
    with pytest.raises(pkg._ffi.IlqrError, match="no policy"):
        sol.rollout_policy(x1[:, None, :])
    sol.run_stage_("cost_nominal"); sol.run_stage_("gradients"); sol.run_stage_("backward_pass")
    assert sol.rollout_policy(x1[:, None, :])["cost"].shape == (B, 1)           # a backward-pass stage makes a policy
    with pytest.raises(pkg._ffi.IlqrError, match="no parameters"):
        sol.rollout_policy(x1[:, None, :], w=np.zeros((B, 1, T, 1)))
    sol.reset_()
    with pytest.raises(pkg._ffi.IlqrError, match="no policy"):
        sol.rollout_policy(x1[:, None, :])
    sol.close()


def test_host_form_device_form_and_sharded_handle_agree(pkg):
    import torch
    B, S = 5, 70
    sol, model, T, size, w = _solved(pkg, "car_obs", B)
    x1 = _starts(sol, S, size)
    ws = np.stack([R.sample_parameters(w[b], S) for b in range(B)])
    host = sol.rollout_policy(x1, w=ws, step_size=0.5, trajectories=True)
    dev = torch.device("cuda:0")
    d_x1, d_w = torch.from_numpy(x1).to(dev), torch.from_numpy(ws).to(dev)
    d = dict(cost=torch.zeros(B, S, dtype=torch.float64, device=dev), max_violation=torch.zeros(B, S, dtype=torch.float64, device=dev),
             first_nonfinite=torch.zeros(B, S, dtype=torch.int32, device=dev),
             x=torch.zeros(B, S, T, sol.nx, dtype=torch.float64, device=dev), u=torch.zeros(B, S, T - 1, sol.nu, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    sol.rollout_policy_device(S, d_x1.data_ptr(), d["cost"].data_ptr(), d_w_ptr=d_w.data_ptr(), step_size=0.5,
                              d_max_violation_ptr=d["max_violation"].data_ptr(), d_first_nonfinite_ptr=d["first_nonfinite"].data_ptr(),
                              d_x_ptr=d["x"].data_ptr(), d_u_ptr=d["u"].data_ptr())
    sol.synchronize()
    assert _same(host, {k: v.cpu().numpy() for k, v in d.items()})
    sh, _, _, _, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    assert np.array_equal(sh.get_policy()[0], sol.get_policy()[0])
    assert _same(host, sh.rollout_policy(x1, w=ws, step_size=0.5, trajectories=True))
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        sh.rollout_policy_device(S, d_x1.data_ptr(), d["cost"].data_ptr())
    sol.close(); sh.close()


def test_plain_c_example(pkg, tmp_path):
    """examples/policy_rollout.c: solve, then roll the policy out from perturbed starts, from plain C"""
    exe = str(tmp_path / "policy_rollout")
    libdir = os.path.join(ROOT, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "policy_rollout.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([exe, "32", "100"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "policy rollout check passed" in out.stdout
