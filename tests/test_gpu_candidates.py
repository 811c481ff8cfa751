"""ilqr_initialize_rollout_candidates on the GPU against the CPU oracle (tests/candidates_ref.py; its selection rule and the
properties of the inputs used here are checked without a GPU in tests/test_candidates_abi.py).

Bounds, fixed before the kernel ran. cost and max_violation: those of tests/test_gpu_policy_rollout.py, 1e-9 relative to
max(1, |reference|). They hold if the oracle's own open-loop recursion, run a second time with its inputs moved by one part in
1e15 (x1 · (1 + 1e-15), and — x1 is zero in three of the workloads — u · (1 + 1e-15)), moves cost and violation by less than a
tenth of that. Measured on the oracle alone over the candidates used here (S = 70, candidates_ref.SEED): 3.2e-11 (acrobot; the
swing-up under 1.5 × the workload's random torques is close to chaotic), 6.1e-16 (car), 6.1e-16 (car_obs), 2.7e-15 (particle),
4.4e-16 (synth12): all below 1e-10. first_nonfinite: equal — three acrobot candidates of instance 2 overflow in the oracle too, no
candidate is left out. chosen: equal for every instance; on the oracle the best and second-best eligible scores lie at least
9e-5 · max(1, |score|) apart for every instance and both weights (asserted > 4e-9 below and in the CPU file), so an error within
the bound cannot change the order.
"""
import os
import subprocess

import numpy as np
import pytest

import candidates_ref as R
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_COST, TOL_VIOL, TOL_GAP = 1e-9, 1e-9, 4e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["acrobot", "car", "car_obs", "particle", "synth12"]
_REF = {}          # (name, B, S) -> the oracle's scores: computed once, shared, never written to


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    assert hasattr(p._ffi.lib(), "ilqr_initialize_rollout_candidates"), "the library has no ilqr_initialize_rollout_candidates"
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


def _inputs(pkg, name, B, S, T=None):
    """(model, T, x1 [B, n], u [B, S, T-1, m], w or None) of the case; T: a shorter horizon of the same workload"""
    cfg, T_, size = R.CASES[name]
    model, T0, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T0 == T_
    w = pkg.workloads.make_parameters(cfg, B) if name == "car_obs" else None
    if T is not None:
        ub, T_ = ub[:, :T - 1], T
        w = None if w is None else w[:, :T]
    u = np.stack([R.candidates(ub[b], S, size, b) for b in range(B)])
    return model, T_, x1, u, w


def _handle(pkg, name, model, T, B, w=None, **kw):
    opts = pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(R.CASES[name][0], {}))
    sol = _user_particle(pkg, T, B, **kw) if name == "particle" else pkg.Solver(model=model, horizon=T, batch=B, options=opts, **kw)
    if w is not None:
        sol.set_parameters_(w)
    return sol


def _reference(oracle, name, model, T, x1, u, w):
    key = (name, u.shape[0], u.shape[1], T)
    if key not in _REF:
        _REF[key] = [R.score_all(oracle, model, T, x1[b], u[b], None if w is None else w[b]) for b in range(u.shape[0])]
        for r in _REF[key]:
            for v in r.values():
                v.setflags(write=False)
    return _REF[key]


def _same(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _state(sol):
    return sol.buffer("nominal_states"), sol.buffer("nominal_actions"), sol.buffer("_scalars")


def _solved(sol):
    st = sol.stats()
    return sol.get_trajectory() + sol.get_policy() + tuple(st[k] for k in sorted(st))


def _eq(p, q):
    return len(p) == len(q) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, q))


def _check_against(out, refs, weight, tag):
    B, S = out["cost"].shape
    worst = dict(cost=0.0, viol=0.0)
    for b in range(B):
        ref = refs[b]
        assert R.gap(ref["cost"], ref["max_violation"], ref["first_nonfinite"], weight) > TOL_GAP, (tag, b)   # on the oracle alone
        assert np.array_equal(out["first_nonfinite"][b], ref["first_nonfinite"]), (tag, b, out["first_nonfinite"][b], ref["first_nonfinite"])
        fin = ref["first_nonfinite"] == -1
        for s in np.flatnonzero(fin):
            worst["cost"] = max(worst["cost"], abs(out["cost"][b, s] - ref["cost"][s]) / max(1.0, abs(ref["cost"][s])))
            worst["viol"] = max(worst["viol"], abs(out["max_violation"][b, s] - ref["max_violation"][s]) / max(1.0, abs(ref["max_violation"][s])))
        assert np.isfinite(out["cost"][b, fin]).all() and np.isfinite(out["max_violation"][b, fin]).all(), (tag, b)
    print("candidates parity %s (weight %g): %s" % (tag, weight, worst))
    assert worst["cost"] < TOL_COST and worst["viol"] < TOL_VIOL, (tag, worst)
    for b in range(B):
        ref = refs[b]
        assert out["chosen"][b] == R.select(ref["cost"], ref["max_violation"], ref["first_nonfinite"], weight), (tag, b)


@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_oracle(pkg, oracle, name):
    """Every candidate of every instance: cost, max_violation, first_nonfinite and the choice against the oracle (bounds: module
    docstring). S = 70: two waves, the last one ragged; T - 1 is no multiple of 8: the last load tile is ragged."""
    B, S = (3, 70) if name != "synth12" else (2, 70)
    model, T, x1, u, w = _inputs(pkg, name, B, S)
    assert (T - 1) % 8 != 0
    refs = _reference(oracle, name, model, T, x1, u, w)
    sol = _handle(pkg, name, model, T, B, w)
    out = sol.initialize_rollout_candidates_(x1, u)
    _check_against(out, refs, 0.0, name)
    assert (out["max_violation"] > 0).any()
    sol.close()


@pytest.mark.parametrize("name", ["acrobot", "synth12"])
def test_installation_is_bitwise(pkg, name):
    """After the call the handle is what initialize_rollout_(x1, u[:, chosen]) makes of a second handle: buffers, scalars, the
    solve that follows, and the solve after initialize_rollout_resident_."""
    B, S = 2, 70
    model, T, x1, u, w = _inputs(pkg, name, B, S)
    a, b = _handle(pkg, name, model, T, B, w), _handle(pkg, name, model, T, B, w)
    out = a.initialize_rollout_candidates_(x1, u)
    assert (out["chosen"] >= 0).all()
    b.initialize_rollout_(x1, u[np.arange(B), out["chosen"]])
    assert _eq(_state(a), _state(b))
    assert np.array_equal(a.buffer("nominal_actions").reshape(B, T - 1, -1), u[np.arange(B), out["chosen"]])
    b_init = _handle(pkg, name, model, T, B, w)
    b_init.initialize_rollout_(x1, u[np.arange(B), out["chosen"]])
    a.solve_(); b.solve_()
    first = _solved(a)
    assert _eq(first, _solved(b))
    a.reset_(); a.initialize_rollout_resident_()          # a fresh solver's state, then the winners again from the resident inputs
    assert _eq(_state(a), _state(b_init))
    a.solve_()
    assert _eq(first, _solved(a))
    a.close(); b.close(); b_init.close()


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_candidates_are_independent_and_calls_repeat(pkg, name):
    """S = 257 crosses the 256-candidate workgroup of the scoring kernel and makes the select kernel combine several waves; the
    scores of the candidates it shares with the S = 70 call (synth12: S = 9) are bit for bit the same; S = 1 installs candidate 0."""
    B = 2
    S, S70 = 257 if name != "synth12" else 9, 70
    model, T, x1, u, w = _inputs(pkg, name, B, max(S, S70))
    sol = _handle(pkg, name, model, T, B, w)
    full = sol.initialize_rollout_candidates_(x1, u[:, :S])
    again = sol.initialize_rollout_candidates_(x1, u[:, :S])
    assert _same(full, again)
    part = sol.initialize_rollout_candidates_(x1, u[:, :S70])
    for k in ("cost", "max_violation", "first_nonfinite"):
        assert np.array_equal(part[k][:, :S], full[k][:, :S70], equal_nan=True), k
    for b in range(B):          # the device's choice is the rule applied to the device's own scores
        assert full["chosen"][b] == R.select(full["cost"][b], full["max_violation"][b], full["first_nonfinite"][b])
        assert part["chosen"][b] == R.select(part["cost"][b], part["max_violation"][b], part["first_nonfinite"][b])
    one = sol.initialize_rollout_candidates_(x1, u[:, :1])
    assert (one["chosen"] == 0).all() and np.array_equal(one["cost"], full["cost"][:, :1], equal_nan=True)
    ref = _handle(pkg, name, model, T, B, w)
    ref.initialize_rollout_(x1, u[:, 0])
    assert _eq(_state(sol), _state(ref))
    sol.close(); ref.close()


def test_ineligible_candidates(pkg, oracle):
    """A NaN in u[b][s][3] is data: first_nonfinite == 4 as on the oracle, that candidate never wins; an instance whose candidates
    all carry one gets chosen == -1 and candidate 0 installed; its neighbours are bitwise what they are without the poison."""
    name, B, S = "acrobot", 3, 70
    model, T, x1, u, w = _inputs(pkg, name, B, S)
    sol = _handle(pkg, name, model, T, B)
    clean = sol.initialize_rollout_candidates_(x1, u)
    up = u.copy()
    win = int(clean["chosen"][0])
    up[0, win, 3] = np.nan                       # instance 0: the winner is poisoned
    up[1, :, 3] = np.nan                         # instance 1: everybody is
    ref = R.score_one(oracle, model, T, x1[0], up[0, win])
    assert ref["first_nonfinite"] == 4
    out = sol.initialize_rollout_candidates_(x1, up)
    assert out["first_nonfinite"][0, win] == 4 and (out["first_nonfinite"][1] == 4).all()
    r0 = R.score_all(oracle, model, T, x1[0], up[0])
    assert out["chosen"][0] != win and out["chosen"][0] == R.select(r0["cost"], r0["max_violation"], r0["first_nonfinite"])
    assert out["chosen"][1] == -1
    assert out["chosen"][2] == clean["chosen"][2]
    keep = np.arange(S) != win
    for k in ("cost", "max_violation", "first_nonfinite"):
        assert np.array_equal(out[k][2], clean[k][2], equal_nan=True) and np.array_equal(out[k][0, keep], clean[k][0, keep], equal_nan=True), k
    other = _handle(pkg, name, model, T, B)
    pick = np.where(out["chosen"] >= 0, out["chosen"], 0)
    other.initialize_rollout_(x1, up[np.arange(B), pick])
    assert _eq(_state(sol), _state(other))        # NaN compares equal here: instance 1 holds candidate 0, NaN and all
    sol.close(); other.close()


def test_ties_and_weight(pkg, oracle):
    B, S = 3, 70
    model, T, x1, u, w = _inputs(pkg, "car_obs", B, S)
    refs = _reference(oracle, "car_obs", model, T, x1, u, w)
    pick = [[R.select(r["cost"], r["max_violation"], r["first_nonfinite"], wt) for r in refs] for wt in (0.0, 1.0e6)]
    assert any(p != q for p, q in zip(*pick)), pick          # on the oracle first: the weight changes the choice
    sol = _handle(pkg, "car_obs", model, T, B, w)
    for wt, want in zip((0.0, 1.0e6), pick):
        out = sol.initialize_rollout_candidates_(x1, u, violation_weight=wt)
        _check_against(out, refs, wt, "car_obs")
        assert list(out["chosen"]) == want
    # two identical candidates: the winner copied to a higher and to a lower index
    out = sol.initialize_rollout_candidates_(x1, u)
    ut = u.copy()
    for b in range(B):
        ut[b, S - 1] = u[b, int(out["chosen"][b])]
    tie = sol.initialize_rollout_candidates_(x1, ut)
    assert np.array_equal(tie["chosen"], out["chosen"]) and np.array_equal(tie["cost"][:, S - 1], out["cost"][np.arange(B), out["chosen"]])
    for b in range(B):
        ut[b, 0] = u[b, int(out["chosen"][b])]
    tie = sol.initialize_rollout_candidates_(x1, ut)
    assert (tie["chosen"] == 0).all()
    sol.close()


def test_minimal_horizon(pkg, oracle):
    """T = 2: one action, one (ragged) load tile"""
    B, S, T = 3, 70, 2
    model, T, x1, u, w = _inputs(pkg, "particle", B, S, T=T)
    refs = _reference(oracle, "particle", model, T, x1, u, w)
    sol = _handle(pkg, "particle", model, T, B)
    out = sol.initialize_rollout_candidates_(x1, u)
    _check_against(out, refs, 0.0, "particle T=2")
    sol.close()


def test_unconstrained_handle_reports_zero_violation(pkg):
    B, S = 2, 5
    model, T, x1, u, w = _inputs(pkg, "car", B, S)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0), constraints=False)
    out = sol.initialize_rollout_candidates_(x1, u, violation_weight=3.0)
    assert (out["max_violation"] == 0.0).all() and np.isfinite(out["cost"]).all() and (out["chosen"] >= 0).all()
    sol.close()


def test_host_form_device_form_and_sharded_handle_agree(pkg):
    import torch
    B, S = 5, 70
    model, T, x1, u, w = _inputs(pkg, "car_obs", B, S)
    sol = _handle(pkg, "car_obs", model, T, B, w)
    host = sol.initialize_rollout_candidates_(x1, u, violation_weight=2.0)
    host_state = _state(sol)
    dv = _handle(pkg, "car_obs", model, T, B, w)
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(dv.stream_ptr())):
        d_x1, d_u = torch.from_numpy(x1).to(dev), torch.from_numpy(u).to(dev)
        d = dict(chosen=torch.zeros(B, dtype=torch.int32, device=dev), cost=torch.zeros(B, S, dtype=torch.float64, device=dev),
                 max_violation=torch.zeros(B, S, dtype=torch.float64, device=dev), first_nonfinite=torch.zeros(B, S, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    dv.initialize_rollout_candidates_device_(S, d_x1.data_ptr(), d_u.data_ptr(), violation_weight=2.0, d_chosen_ptr=d["chosen"].data_ptr(),
                                             d_cost_ptr=d["cost"].data_ptr(), d_max_violation_ptr=d["max_violation"].data_ptr(),
                                             d_first_nonfinite_ptr=d["first_nonfinite"].data_ptr())
    dv.synchronize()
    assert _same(host, {k: v.cpu().numpy() for k, v in d.items()})
    assert _eq(host_state, _state(dv))
    dv.initialize_rollout_candidates_device_(S, d_x1.data_ptr(), d_u.data_ptr(), violation_weight=2.0)      # no outputs wanted
    dv.synchronize()
    assert _eq(host_state, _state(dv))
    sh = _handle(pkg, "car_obs", model, T, B, w, devices=[0, 0])
    assert _same(host, sh.initialize_rollout_candidates_(x1, u, violation_weight=2.0))
    assert _eq(host_state, _state(sh))
    sol.solve_(); sh.reset_(); sh.initialize_rollout_resident_(); sh.solve_()
    assert _eq(_solved(sol), _solved(sh))
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        sh.initialize_rollout_candidates_device_(S, d_x1.data_ptr(), d_u.data_ptr())
    sol.close(); dv.close(); sh.close()


def test_plain_c_example(pkg, tmp_path):
    """examples/candidate_init.c: score 8 candidates per acrobot, print the chosen index, solve — from plain C"""
    exe = str(tmp_path / "candidate_init")
    libdir = os.path.join(ROOT, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "candidate_init.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe, "16", "8"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    first = out.stdout.splitlines()[0]
    assert first.startswith("chosen candidate of instance 0: ") and 0 <= int(first.split(": ")[1].split()[0]) < 8, first
    assert "candidate init check passed" in out.stdout


def test_the_policy_stays_untouched(pkg):
    """Solve, then choose a new start: K, k, the duals and the trace are bitwise what they were."""
    B, S = 3, 70
    model, T, x1, u, w = _inputs(pkg, "car", B, S)
    sol = _handle(pkg, "car", model, T, B)
    sol.enable_trace_(64)
    sol.initialize_rollout_(x1, u[:, 0])
    sol.solve_()
    snap = lambda: sol.get_policy() + (sol.buffer("constraint_dual"), sol.buffer("constraint_penalty"), sol.trace())
    before = snap()
    out = sol.initialize_rollout_candidates_(x1, u)
    assert (out["chosen"] >= 0).all()
    assert _eq(before, snap())
    assert np.array_equal(sol.buffer("nominal_actions").reshape(B, T - 1, -1), u[np.arange(B), out["chosen"]])
    sol.close()
