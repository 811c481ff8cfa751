"""tests/mpc_ref.py without a GPU. (1) Where both exist, the model-agnostic yardstick is tied to the old ones: on car, car_obs under
per-sample parameters, synth12 and car_tv its closed loop equals policy_ref.oracle_reading and its open-loop score
candidates_ref.score_one on the C++ oracle, at the bounds of the GPU modules (x, u 1e-10; cost, max_violation 1e-9). (2) The input
sets of tests/test_gpu_mpc_sweep.py — the same generators, the policy taken from the independent restatement's solve instead of
the device's — are checked on the yardstick alone: every sample, candidate and shift head is finite (nobody is left out), and
ten times the yardstick's own spread under a move of its inputs by one part in 1e15 stays under the bound the GPU test uses. The
spreads are printed (pytest -s) and recorded in the docstring of tests/test_gpu_mpc_sweep.py."""
import numpy as np
import pytest

import candidates_ref as CR
import mpc_ref as M
import policy_ref as P
import shift_ref as SH
from ilqr_amd_loader import load_package

TOL_XU, TOL_COST, TOL_VIOL = 1e-10, 1e-9, 1e-9
T = M.T_SWEEP


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return load_package()


def _case(pkg, name):
    """(oracle model, T, problem, x1 [B, n], ū [B, T-1, m], w or None, size of the starts' noise, of the candidates' noise, options)"""
    B = 2
    if name == "car_tv":
        _, _, x1, ub = pkg.workloads.make_inputs("car", B)
        return "car_tv", T, M.car_tv(T), x1, np.ascontiguousarray(ub[:, :T - 1]), None, P.CASES["car"][2], CR.CASES["car"][2], {}
    cfg, T_, size = P.CASES[name]
    model, T0, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T0 == T_
    w = pkg.workloads.make_parameters(cfg, B) if name == "car_obs" else None
    return model, T_, dict(car=M.car, car_obs=M.car_obs, synth12=M.synth12)[name](), x1, ub, w, size, CR.CASES[name][2], \
        pkg.workloads.CONFIG_OPTIONS.get(cfg, {})


def _agree(a, ref, tag):
    assert a["first_nonfinite"] == ref["first_nonfinite"] == -1, tag
    if "u" in ref:
        assert P.rel(a["x"], ref["x"]) < TOL_XU and P.rel(a["u"], ref["u"]) < TOL_XU, (tag, P.rel(a["x"], ref["x"]), P.rel(a["u"], ref["u"]))
    else:
        assert P.rel(a["x"], ref["x"]) < TOL_XU, tag
    assert abs(a["cost"] - ref["cost"]) < TOL_COST * max(1.0, abs(ref["cost"])), (tag, a["cost"], ref["cost"])
    assert abs(a["max_violation"] - ref["max_violation"]) < TOL_VIOL * max(1.0, abs(ref["max_violation"])), (tag, a["max_violation"], ref["max_violation"])


@pytest.mark.parametrize("name", ["car", "car_obs", "synth12", "car_tv"])
def test_the_yardstick_agrees_with_the_oracle(pkg, oracle, name):
    model, T_, p, x1, ub, w, size, csize, kw = _case(pkg, name)
    B, S = x1.shape[0], 8
    sol = oracle.solve_batch(model, T_, x1, ub, options=oracle.default_options(**kw), nthreads=2, w=w)
    seen = 0.0
    for b in range(B):
        xb, u, K, k = sol["x"][b], sol["u"][b], sol["K"][b], sol["k"][b]
        starts = P.perturbed_starts(xb[0], S, size, seed=P.SEED + b)
        ws = P.sample_parameters(w[b], S, seed=P.SEED + 100 + b) if w is not None else None
        for s in range(S):
            ws_ = None if ws is None else ws[s]
            ref = P.oracle_reading(oracle, model, T_, xb, u, K, starts[s], ws_)
            _agree(M.policy_rollout(*p, xb, u, K, k, starts[s], 0.0, ws_), ref, (name, b, s))
            seen = max(seen, ref["max_violation"])
        for alpha in (1.0, 0.5):            # x1 = x̄_1 and k as solved: the oracle's unmodified rollout!(α)
            ref = P.oracle_rollout_bang(oracle, model, T_, xb, u, K, k, alpha, None if w is None else w[b])
            _agree(M.policy_rollout(*p, xb, u, K, k, xb[0], alpha, None if w is None else w[b]), ref, (name, b, alpha))
        cands = CR.candidates(ub[b], S, csize, b)
        for s in range(S):
            ref = CR.score_one(oracle, model, T_, x1[b], cands[s], None if w is None else w[b])
            _agree(M.score_candidate(*p, x1[b], cands[s], None if w is None else w[b]), ref, (name, b, s, "candidate"))
            seen = max(seen, ref["max_violation"])
    assert seen > 0.0                       # the violation rule is exercised


def test_violation_and_first_nonfinite_rules():
    assert M.violation(0.0, [-2.0, 0.5, -0.25], (0, 1)) == 0.5 and M.violation(0.0, [-2.0, 0.5, -0.75], (0, 1)) == 0.75
    assert M.violation(3.0, [1.0], ()) == 3.0 and np.isnan(M.violation(3.0, [np.nan], (0,))) and np.isnan(M.violation(np.nan, [1.0], ()))
    p = M.car()
    u = np.zeros((5, 2)); u[2, 0] = np.inf
    r = M.score_candidate(*p, np.zeros(3), u, None)
    assert r["first_nonfinite"] == 3 == P.first_nonfinite(r["x"])


def _fmt(d):
    return ", ".join("%s %.1e" % kv for kv in sorted(d.items()))


@pytest.mark.parametrize("nm", M.SIZES, ids=["%dx%d" % nm for nm in M.SIZES])
def test_the_sweeps_inputs_are_finite_and_the_bounds_stand(oracle, nm):
    """Per size: the starts, candidates and measured states of the GPU sweep on the yardstick, under the restatement's policy."""
    n, m = nm
    S, B = M.samples(n, m), M.B_SWEEP
    p, _ = M.synth(T, n, m)
    x1, ub0 = M.sweep_inputs(n, m)
    xb, ub, K, k = M.restatement_policy(n, m)
    assert np.array_equal(xb[:, 0], x1) and np.isfinite(K).all() and np.abs(k).max() > 0.0
    starts = M.rollout_starts(xb, S)
    cands = M.candidate_set(ub0, S)
    assert np.array_equal(starts[:, 0], xb[:, 0]) and np.array_equal(cands[:, 0], ub0) and (np.abs(ub0) > 1.0).any()
    sg = M.sigma(m)
    assert len(set(sg)) == m and (sg > 0).all()
    worst = dict(policy=dict(xu=0.0, cost=0.0, viol=0.0), candidates=dict(cost=0.0, viol=0.0), shift=dict(xu=0.0, cost=0.0, viol=0.0))
    violated = dict(policy=False, candidates=False)
    for b in range(B):
        for alpha in (0.0, 0.5):
            for s in range(S):
                r = M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], starts[b, s], alpha, None)
                assert r["first_nonfinite"] == -1 and np.isfinite([r["cost"], r["max_violation"]]).all(), (nm, b, s)
                violated["policy"] |= r["max_violation"] > 0
            sp = M.spread(p, xb[b], ub[b], K[b], k[b], starts[b], alpha)
            worst["policy"] = {q: max(worst["policy"][q], sp[q]) for q in sp}
        sc = M.score_all(p, x1[b], cands[b])
        assert (sc["first_nonfinite"] == -1).all() and np.isfinite(sc["cost"]).all() and np.isfinite(sc["max_violation"]).all(), (nm, b)
        violated["candidates"] |= bool((sc["max_violation"] > 0).any())
        sp = M.score_spread(p, x1[b], cands[b])
        worst["candidates"] = {q: max(worst["candidates"][q], sp[q]) for q in sp}
        for steps in M.SHIFTS:
            start = M.measured_starts(xb, steps)[b]
            r = M.shift_head(p, xb[b], ub[b], K[b], None, steps, start)
            assert r["first_nonfinite"] == -1 and r["x"].shape == (T - steps, n), (nm, b, steps)
            assert np.abs(r["u"] - ub[b, steps:]).max() > 1e-6                   # the measured start moves the head
            sp = M.spread(p, xb[b, steps:], ub[b, steps:], K[b, steps:], np.zeros_like(ub[b, steps:]), [start])
            worst["shift"] = {q: max(worst["shift"][q], sp[q]) for q in sp}
    print("mpc_ref spread %dx%d: policy %s | candidates %s | shift head %s" % (n, m, _fmt(worst["policy"]), _fmt(worst["candidates"]), _fmt(worst["shift"])))
    assert violated["policy"] and violated["candidates"]                         # the action box is crossed somewhere
    assert 10.0 * max(worst["policy"]["xu"], worst["shift"]["xu"]) < TOL_XU
    assert 10.0 * max(worst["policy"]["cost"], worst["candidates"]["cost"]) < TOL_COST
    assert 10.0 * max(worst["policy"]["viol"], worst["candidates"]["viol"]) < TOL_VIOL
    if nm == (16, 16):                      # why the starts move by 0.5: moved by 0.02, no sample of this size leaves the box
        near = M.rollout_starts(xb, S, 0.02)
        assert all(M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], near[b, s], 0.0, None)["max_violation"] == 0.0 for b in range(B) for s in range(S))
    if nm == (32, 8):                       # the size with an oracle twin: both yardsticks
        for b in range(B):
            for s in range(S):
                _agree(M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], starts[b, s], 0.0, None),
                       P.oracle_reading(oracle, "synth32", T, xb[b], ub[b], K[b], starts[b, s]), (nm, b, s))
                _agree(M.score_candidate(*p, x1[b], cands[b, s], None), CR.score_one(oracle, "synth32", T, x1[b], cands[b, s]), (nm, b, s))


@pytest.mark.parametrize("name", ["car_tv", "car_obs_alt"])
def test_the_lowered_cases_inputs_are_finite_and_the_bounds_stand(pkg, oracle, name):
    """The inputs of the lowered GPU cases (T = 21, B = 3, S = 70) on the yardstick. car_tv: under the oracle's policy. The
    alternating-cost car_obs has no oracle twin: the policy is the oracle's for the plain car_obs under the same parameters — any
    stabilising policy serves for asking whether the samples stay finite and how far rounding moves them."""
    B, S = M.B_SWEEP, 70
    src = "car" if name == "car_tv" else "car_obs"
    _, _, x1, ub = pkg.workloads.make_inputs(src, B)
    ub = np.ascontiguousarray(ub[:, :T - 1])
    w = None if name == "car_tv" else np.ascontiguousarray(SH.time_varying(pkg.workloads.make_parameters("car_obs", B))[:, :T])
    p = M.car_tv(T) if name == "car_tv" else M.car_obs(lambda t: 1.0e-2 if t % 2 == 0 else 2.0e-2)
    sol = oracle.solve_batch(src if name != "car_tv" else "car_tv", T, x1, ub, nthreads=2, w=w)
    size, csize = P.CASES[src][2], CR.CASES[src][2]
    worst = dict(policy=dict(xu=0.0, cost=0.0, viol=0.0), candidates=dict(cost=0.0, viol=0.0), shift=dict(xu=0.0, cost=0.0, viol=0.0))
    for b in range(B):
        xb, u, K, k = sol["x"][b], sol["u"][b], sol["K"][b], sol["k"][b]
        starts = P.perturbed_starts(xb[0], S, size, seed=P.SEED + b)
        ws = None if w is None else P.sample_parameters(w[b], S, seed=P.SEED + 100 + b)
        for alpha in (0.0, 0.5):
            for s in range(S):
                r = M.policy_rollout(*p, xb, u, K, k, starts[s], alpha, None if ws is None else ws[s])
                assert r["first_nonfinite"] == -1 and np.isfinite([r["cost"], r["max_violation"]]).all(), (name, b, s)
            sp = M.spread(p, xb, u, K, k, starts, alpha, ws)
            worst["policy"] = {q: max(worst["policy"][q], sp[q]) for q in sp}
        cands = CR.candidates(ub[b], S, csize, b)
        sc = M.score_all(p, x1[b], cands, None if w is None else w[b])
        assert (sc["first_nonfinite"] == -1).all() and np.isfinite(sc["cost"]).all(), (name, b)
        sp = M.score_spread(p, x1[b], cands, None if w is None else w[b])
        worst["candidates"] = {q: max(worst["candidates"][q], sp[q]) for q in sp}
        if name == "car_tv":
            start = SH.measured_start(xb[0], size, b, 0)
            assert M.shift_head(p, xb, u, K, None, 0, start)["first_nonfinite"] == -1
            sp = M.spread(p, xb, u, K, np.zeros_like(u), [start])
            worst["shift"] = {q: max(worst["shift"][q], sp[q]) for q in sp}
    print("mpc_ref spread %s: policy %s | candidates %s | shift head %s" % (name, _fmt(worst["policy"]), _fmt(worst["candidates"]), _fmt(worst["shift"])))
    assert 10.0 * max(worst["policy"]["xu"], worst["shift"]["xu"]) < TOL_XU
    assert 10.0 * max(worst["policy"]["cost"], worst["candidates"]["cost"]) < TOL_COST
    assert 10.0 * max(worst["policy"]["viol"], worst["candidates"]["viol"]) < TOL_VIOL


@pytest.mark.parametrize("name", ["synth5w_alt", "ragged"])
def test_the_restatement_solved_lowered_cases_are_finite_and_the_bounds_stand(name):
    """The two lowered GPU cases the oracle-side policies above do not reach, under the restatement's own solve of the actual
    problem: the large-form model with a user parameter and alternating stage kinds (per-sample w, candidates, the re-anchoring
    shift head), and ragged (T = 9, padded: policy rollout and candidates)."""
    B = M.B_SWEEP
    worst = dict(policy=dict(xu=0.0, cost=0.0, viol=0.0), candidates=dict(cost=0.0, viol=0.0), shift=dict(xu=0.0, cost=0.0, viol=0.0))
    if name == "synth5w_alt":
        p, S = M.synth5w(), M.samples(5, 1)
        x1, ub0 = M.sweep_inputs(5, 1)
        w = M.synth5w_parameters()
        xb, ub, K, k = M.synth5w_restatement_policy()
        starts, cands = M.rollout_starts(xb, S), M.candidate_set(ub0, S)
        ws = [P.sample_parameters(w[b], S, seed=P.SEED + 100 + b) for b in range(B)]
        alphas = (0.0, 0.5)
    else:
        p, _, n_t, m_t = M.ragged()
        S, w, ws, alphas = 70, None, None, (0.0,)
        x1, ub0, cands = M.ragged_inputs(n_t, m_t, B, S)
        xb, ub, K, k = M.ragged_restatement_policy(B)
        starts = M.ragged_starts(xb, n_t[0], S)
        for t in range(len(n_t)):
            assert (xb[:, t, n_t[t]:] == 0).all()
    assert np.array_equal(xb[:, 0], x1) and np.isfinite(K).all()
    violated = False
    for b in range(B):
        wb = None if w is None else w[b]
        for alpha in alphas:
            for s in range(S):
                r = M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], starts[b, s], alpha, wb if ws is None else ws[b][s])
                assert r["first_nonfinite"] == -1 and np.isfinite([r["cost"], r["max_violation"]]).all(), (name, b, s)
                violated |= r["max_violation"] > 0
            sp = M.spread(p, xb[b], ub[b], K[b], k[b], starts[b], alpha, None if ws is None else ws[b])
            worst["policy"] = {q: max(worst["policy"][q], sp[q]) for q in sp}
        sc = M.score_all(p, x1[b], cands[b], wb)
        assert (sc["first_nonfinite"] == -1).all() and np.isfinite(sc["cost"]).all() and np.isfinite(sc["max_violation"]).all(), (name, b)
        sp = M.score_spread(p, x1[b], cands[b], wb)
        worst["candidates"] = {q: max(worst["candidates"][q], sp[q]) for q in sp}
        if name == "synth5w_alt":
            start = M.measured_starts(xb, 0)[b]
            assert M.shift_head(p, xb[b], ub[b], K[b], wb, 0, start)["first_nonfinite"] == -1
            sp = M.spread(p, xb[b], ub[b], K[b], np.zeros_like(ub[b]), [start], 0.0, [wb])
            worst["shift"] = {q: max(worst["shift"][q], sp[q]) for q in sp}
    print("mpc_ref spread %s: policy %s | candidates %s | shift head %s" % (name, _fmt(worst["policy"]), _fmt(worst["candidates"]), _fmt(worst["shift"])))
    assert violated
    assert 10.0 * max(worst["policy"]["xu"], worst["shift"]["xu"]) < TOL_XU
    assert 10.0 * max(worst["policy"]["cost"], worst["candidates"]["cost"]) < TOL_COST
    assert 10.0 * max(worst["policy"]["viol"], worst["candidates"]["viol"]) < TOL_VIOL
