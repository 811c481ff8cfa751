"""The MPC-side kernels — ilqr_rollout_policy, ilqr_initialize_rollout_candidates, ilqr_sample_rollout_candidates, ilqr_shift_horizon,
each in its small-model and its large-model form — over the model sizes at which their tile geometry, lane bounds and half-row
guards change, and on lowered problems (stage selectors riding in θ), against the model-agnostic yardstick tests/mpc_ref.py (plain
fp64 loops over the independent restatement's objects; where the C++ oracle has a twin — synth32, car_tv, ragged — against it too).

Sizes (nx, nu) and what each is there for. Small form: (1, 1) WX = WU = 8, the smallest tiles; (4, 3) a 24-double run in a
32-lane group; (2, 4) nu = 4 and nu > nx. Large form: (5, 1) first large size, odd nx under the split rows, nu = 1; (9, 3) odd nx,
five state terms per half row; (16, 16) `lane < nu` at the nu limit and the sampling key's widest j; (17, 2) odd nx beyond one
16-row tile; (32, 8) the last split size (the built-in synth32: both yardsticks); (33, 2) the first size with one state row per
lane, odd; (40, 6) and (64, 8) unsplit, at 64 every lane owns a row. T = 21: tiles of 8, 8 and a ragged 4, a chunk of 16 and a
ragged 5. B = 3; S = 70 on the small path (two waves, the second ragged), S = 5 on the large path (one wave per sample).

Bounds: the project's own, from the module docstrings of test_gpu_policy_rollout.py, test_gpu_candidates.py, test_gpu_shift.py and
test_gpu_sample_candidates.py, not re-tuned here — x, u: 1e-10 relative to max(1, max |reference|); cost: 1e-9 relative;
max_violation: 1e-9 per max(1, |v|); noise 1e-13; blend 1e-11; first_nonfinite, chosen and everything called bitwise: equal.
Whether the larger sizes need more was decided on the yardstick alone, without a device (tests/test_mpc_ref.py, which asserts
it): its own recursion run a second time with x1 (for the candidates also u) moved by one part in 1e15 moves

    (nx, nu)    policy x, u / cost / viol      candidates cost / viol    shift head x, u
    (1, 1)      3.6e-15 / 2.6e-15 / 3.1e-15    1.7e-15 / 2.2e-15         1.8e-15
    (4, 3)      3.6e-15 / 2.2e-15 / 3.6e-15    2.1e-15 / 2.2e-15         2.2e-15
    (2, 4)      4.4e-15 / 4.2e-15 / 2.7e-15    3.7e-15 / 2.2e-15         1.4e-15
    (5, 1)      2.2e-15 / 1.0e-15 / 2.7e-15    8.0e-16 / 2.1e-15         1.5e-15
    (9, 3)      2.6e-15 / 1.4e-15 / 2.7e-15    1.2e-15 / 2.2e-15         1.4e-15
    (16, 16)    1.6e-15 / 1.1e-15 / 1.3e-15    8.7e-16 / 2.2e-15         1.2e-15
    (17, 2)     2.3e-15 / 9.6e-16 / 4.4e-15    6.7e-16 / 2.2e-15         3.6e-15
    (32, 8)     1.8e-15 / 1.4e-15 / 1.8e-15    5.0e-16 / 2.2e-15         1.5e-15
    (33, 2)     4.4e-15 / 8.8e-16 / 2.7e-15    6.4e-16 / 2.2e-15         3.1e-15
    (40, 6)     1.8e-15 / 9.6e-16 / 2.7e-15    7.5e-16 / 2.2e-15         1.5e-15
    (64, 8)     4.3e-15 / 1.0e-15 / 6.7e-16    6.3e-16 / 2.2e-15         1.7e-15
    car_tv      2.8e-15 / 7.4e-16 / 2.7e-15    4.4e-16 / 2.2e-16         8.5e-16
    car_obs_alt 4.3e-15 / 5.9e-16 / 3.6e-15    4.4e-16 / 2.2e-16         -
    synth5w_alt 2.2e-15 / 7.8e-16 / 3.6e-15    5.9e-16 / 2.1e-15         1.4e-15
    ragged      3.2e-15 / 3.1e-15 / 2.5e-16    3.0e-15 / 8.9e-16         -

(policy: the worse of step sizes 0 and 0.5; car_obs_alt: the lowered car_obs with alternating stage costs, under per-sample
parameters; synth5w_alt: its large-form counterpart, nx = 5 with one user parameter; ragged: T = 9, padded). Ten times that is four orders below every bound, so the bounds stand at every size. No sample, candidate or shift
head is left out: the same file asserts that the yardstick keeps every one of them finite.

What of the split rows a test can see. With nx <= 32 lane i + 32 takes the second half of row i's state terms: HX = (nx + 1) / 2
terms per lane, and at odd nx the last term of the upper half is a padding term that dyn_row's half-row guard sends to x_0
against a zero coefficient. A wrong HX or guard changes x_{t+1} on every stored row, which (5, 1), (9, 3) and (17, 2) compare
with the yardstick on all four entry points. The lane's own `xrow = SPLIT ? lane & 31 : lane` is different: on lanes 32.. of a
split model xl feeds nothing but that lane's own elementwise remainder, the sum of the halves is taken before it is added, and
only lanes < nx ever store xl (to LDS and to x) — so whether those lanes carry a copy of x_{lane − 32} or anything else finite
changes no output. Narrowing that one condition to nx <= 16 is an equivalent mutant; no test here or elsewhere can fail on it.
"""
import numpy as np
import pytest

import candidates_ref as CR
import mpc_ref as M
import policy_ref as P
import sample_ref as SR
import shift_ref as SH
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU, TOL_COST, TOL_VIOL, TOL_NOISE, TOL_BLEND = 1e-10, 1e-9, 1e-9, 1e-13, 1e-11
T, B = M.T_SWEEP, M.B_SWEEP
IDS = ["%dx%d" % nm for nm in M.SIZES]
_MODELS = {}


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_rollout_policy", "ilqr_initialize_rollout_candidates", "ilqr_sample_rollout_candidates", "ilqr_shift_horizon"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


# ------------------------------------------------------------------------------------------------------------------ helpers
def _handle(pkg, n, m):
    if (n, m) == (32, 8):
        return pkg.Solver(model="synth32", horizon=T, batch=B, options=pkg.Options(verbose=0))
    if (n, m) in _MODELS:           # traced and loaded once per size (the symbolic Jacobians of 64 states take half a minute): by its registered name
        sol = pkg.Solver(model=_MODELS[(n, m)], horizon=T, batch=B, options=pkg.Options(verbose=0))
    else:
        mdl = pkg.models.synth_nm(n, m)
        sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                         [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0), name=M.module_name(n, m))
        _MODELS[(n, m)] = sol.model
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 2 * m)
    return sol


def _solved(pkg, n, m):
    """a solved handle of the sweep's inputs and what the kernels read of it: (sol, x̄, ū, K, k)"""
    sol = _handle(pkg, n, m)
    x1, ub = M.sweep_inputs(n, m)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return (sol,) + sol.get_trajectory() + sol.get_policy()


def _state(sol):
    """what an initialiser installs (the other named scalars belong to the solve: a solved and a fresh handle differ in them)"""
    return sol.buffer("nominal_states"), sol.buffer("nominal_actions"), sol.scalar("states_eq_nominal")


def _eq(p, q):
    return len(p) == len(q) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, q))


def _same(a, b, keys=None):
    keys = sorted(a) if keys is None else keys
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _relv(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _check_rollouts(out, refs, x1, tag):
    """every sample of every instance against refs[b][s] (dicts of the yardstick or the oracle)"""
    worst = dict(x=0.0, u=0.0, cost=0.0, viol=0.0)
    nB, nS = out["cost"].shape
    for b in range(nB):
        for s in range(nS):
            ref = refs[b][s]
            assert ref["first_nonfinite"] == -1 and out["first_nonfinite"][b, s] == -1, (tag, b, s)
            assert np.array_equal(out["x"][b, s, 0], x1[b, s]), (tag, b, s)
            worst["x"] = max(worst["x"], P.rel(out["x"][b, s], ref["x"])); worst["u"] = max(worst["u"], P.rel(out["u"][b, s], ref["u"]))
            worst["cost"] = max(worst["cost"], _relv(out["cost"][b, s], ref["cost"]))
            worst["viol"] = max(worst["viol"], _relv(out["max_violation"][b, s], ref["max_violation"]))
    print("mpc sweep, policy rollout %s: %s" % (tag, worst))
    assert worst["x"] < TOL_XU and worst["u"] < TOL_XU, (tag, worst)
    assert worst["cost"] < TOL_COST and worst["viol"] < TOL_VIOL, (tag, worst)


def _check_scores(out, refs, tag, choice=True):
    """cost, max_violation, first_nonfinite of every candidate against refs[b] (score_all dicts); chosen is the rule applied to the
    DEVICE's scores, and the reference's own choice wherever its two best scores lie further apart than the cost bound"""
    worst = dict(cost=0.0, viol=0.0)
    nB, nS = out["cost"].shape
    for b in range(nB):
        ref = refs[b]
        assert (ref["first_nonfinite"] == -1).all(), (tag, b)                  # nobody is left out
        assert np.array_equal(out["first_nonfinite"][b], ref["first_nonfinite"]), (tag, b)
        for s in range(nS):
            worst["cost"] = max(worst["cost"], _relv(out["cost"][b, s], ref["cost"][s]))
            worst["viol"] = max(worst["viol"], _relv(out["max_violation"][b, s], ref["max_violation"][s]))
    print("mpc sweep, candidates %s: %s" % (tag, worst))
    assert worst["cost"] < TOL_COST and worst["viol"] < TOL_VIOL, (tag, worst)
    if choice:
        for b in range(nB):
            ref = refs[b]
            assert out["chosen"][b] == CR.select(out["cost"][b], out["max_violation"][b], out["first_nonfinite"][b]), (tag, b)
            if CR.gap(ref["cost"], ref["max_violation"], ref["first_nonfinite"]) > TOL_COST:
                assert out["chosen"][b] == CR.select(ref["cost"], ref["max_violation"], ref["first_nonfinite"]), (tag, b)


def _check_installation(a, b, x1, u_installed):
    """handle a is bitwise what initialize_rollout_(x1, u_installed) makes of handle b, and its resident inputs replay it"""
    b.initialize_rollout_(x1, u_installed)
    want = _state(b)
    assert _eq(_state(a), want)
    assert np.array_equal(a.buffer("nominal_actions").reshape(u_installed.shape), u_installed)
    a.set_buffer("nominal_states", np.zeros_like(want[0])); a.set_buffer("nominal_actions", np.ones_like(want[1]))
    a.initialize_rollout_resident_()
    assert _eq(_state(a), want)


def _check_sampling(a, b, x1, base, sg, tag, seed=M.SEED):
    """pick and blend on handle a; b: a second handle for the materialised path. Returns the pick call's outputs."""
    nB, N, m = base.shape
    S = M.samples(a.nx, m)
    z = SR.noise(seed, nB, S, N, m)
    u0 = a.sample_rollout_candidates_(sg, S, seed=seed, x1=x1, base_u=np.zeros_like(base), return_candidates=True)["u"]
    assert np.array_equal(u0[:, 0], np.zeros_like(base))
    err = np.abs(u0[:, 1:] / sg - z[:, 1:]).max() if S > 1 else 0.0
    print("mpc sweep, device noise against numpy %s: %.2e" % (tag, err))
    assert err <= TOL_NOISE, (tag, err)
    out = a.sample_rollout_candidates_(sg, S, seed=seed, x1=x1, base_u=base, return_candidates=True)
    # around a base: the noise bound scaled by sigma, and one rounding each of the product and of the sum
    want = base[:, None] + sg * z
    assert np.array_equal(out["u"][:, 0], base) and (np.abs(out["u"] - want) <= TOL_NOISE * sg + 2.0 ** -51 * np.maximum(1.0, np.abs(want))).all(), tag
    ref = b.initialize_rollout_candidates_(x1, out["u"])
    keys = ("cost", "max_violation", "first_nonfinite", "chosen")
    assert _same(out, ref, keys), (tag, {k: np.abs(out[k].astype(float) - ref[k]).max() for k in keys})
    assert (out["chosen"] >= 0).all()
    pick = np.zeros((nB, S)); pick[np.arange(nB), out["chosen"]] = 1.0
    assert np.array_equal(out["weights"], pick)
    assert _eq(_state(a), _state(b))
    fin = np.where(out["first_nonfinite"] == -1, out["cost"], np.nan)
    temperature = float(np.nanmax(np.nanmax(fin, axis=1) - np.nanmin(fin, axis=1)))
    assert temperature > 0.0
    bl = a.sample_rollout_candidates_(sg, S, seed=seed, mode="blend", temperature=temperature, x1=x1, base_u=base, return_candidates=True)
    assert _same(bl, out, keys + ("u",))
    got = a.buffer("nominal_actions").reshape(base.shape)
    worst = dict(w=0.0, u=0.0)
    for i in range(nB):
        chosen, wt = SR.blend_weights(bl["cost"][i], bl["max_violation"][i], bl["first_nonfinite"][i], 0.0, temperature)
        assert chosen == bl["chosen"][i]
        worst["w"] = max(worst["w"], np.abs(bl["weights"][i] - wt).max())
        want = SR.blend_actions(bl["u"][i], bl["weights"][i])
        worst["u"] = max(worst["u"], (np.abs(got[i] - want) / np.maximum(1.0, np.abs(want))).max())
    print("mpc sweep, blend %s: %s" % (tag, worst))
    assert worst["w"] <= TOL_BLEND and worst["u"] <= TOL_BLEND, (tag, worst)
    assert (np.count_nonzero(bl["weights"] > 1e-3, axis=1) > 1).all()              # a real blend
    b.initialize_rollout_(x1, got)
    assert _eq(_state(a), _state(b))
    return out


# ------------------------------------------------------------------------------------------------- the dimension sweep
@pytest.mark.parametrize("nm", M.SIZES, ids=IDS)
def test_policy_rollout_over_the_sizes(pkg, oracle, nm):
    """Every sample of every instance at step_size 0 and 0.5: x, u, cost, max_violation, first_nonfinite against the yardstick
    (synth32: against the oracle too); the lean call is bitwise the trajectory call."""
    n, m = nm
    S = M.samples(n, m)
    sol, xb, ub, K, k = _solved(pkg, n, m)
    p, _ = M.synth(T, n, m)
    x1 = M.rollout_starts(xb, S)
    outs = []
    for alpha in (0.0, 0.5):
        out = sol.rollout_policy(x1, step_size=alpha, trajectories=True)
        lean = sol.rollout_policy(x1, step_size=alpha)
        assert set(lean) == {"cost", "max_violation", "first_nonfinite"} and _same(lean, out, sorted(lean))
        refs = [[M.policy_rollout(*p, xb[b], ub[b], K[b], k[b], x1[b, s], alpha, None) for s in range(S)] for b in range(B)]
        _check_rollouts(out, refs, x1, "%dx%d step %.1f" % (n, m, alpha))
        assert (out["max_violation"] > 0).any()
        outs.append(out)
    assert not np.array_equal(outs[0]["u"], outs[1]["u"])                        # k matters
    if nm == (32, 8):
        refs = [[P.oracle_reading(oracle, "synth32", T, xb[b], ub[b], K[b], x1[b, s]) for s in range(S)] for b in range(B)]
        _check_rollouts(outs[0], refs, x1, "32x8 oracle")
    sol.close()


@pytest.mark.parametrize("nm", M.SIZES, ids=IDS)
def test_candidates_over_the_sizes(pkg, oracle, nm):
    n, m = nm
    S = M.samples(n, m)
    x1, ub = M.sweep_inputs(n, m)
    u = M.candidate_set(ub, S)
    p, _ = M.synth(T, n, m)
    a, b = _handle(pkg, n, m), _handle(pkg, n, m)
    out = a.initialize_rollout_candidates_(x1, u)
    _check_scores(out, [M.score_all(p, x1[i], u[i]) for i in range(B)], "%dx%d" % nm)
    if nm == (32, 8):
        _check_scores(out, [CR.score_all(oracle, "synth32", T, x1[i], u[i]) for i in range(B)], "32x8 oracle")
    assert (out["max_violation"] > 0).any() and (out["chosen"] >= 0).all()
    _check_installation(a, b, x1, u[np.arange(B), out["chosen"]])
    a.close(); b.close()


@pytest.mark.parametrize("nm", M.SIZES, ids=IDS)
def test_sampling_over_the_sizes(pkg, nm):
    """pick and blend with a different sigma per component: the candidates are base + sigma · the numpy noise, their scores
    bitwise those of the materialised path on them, the blend numpy's on the device's scores"""
    n, m = nm
    x1, ub = M.sweep_inputs(n, m)
    sg = M.sigma(m)
    assert len(set(sg)) == m and (sg > 0).all()
    a, b = _handle(pkg, n, m), _handle(pkg, n, m)
    _check_sampling(a, b, x1, ub, sg, "%dx%d" % nm)
    a.close(); b.close()


@pytest.mark.parametrize("nm", M.SIZES, ids=IDS)
def test_shift_over_the_sizes(pkg, nm):
    """k in {1, 3}, both tails: the open loop bitwise shift_ref.shifted_inputs; the closed loop from a measured start against the
    yardstick's head, its tail bitwise; feedback from x̄_k the open-loop shift to rounding"""
    n, m = nm
    N = T - 1
    a, xb, ub, K, _ = _solved(pkg, n, m)
    ref = _handle(pkg, n, m)
    p, _ = M.synth(T, n, m)

    def restore():
        a.set_buffer("nominal_states", xb); a.set_buffer("nominal_actions", ub)

    worst = dict(x=0.0, u=0.0, nominal=0.0)
    for k in M.SHIFTS:
        x1 = M.measured_starts(xb, k)
        for tail in ("hold", "zero"):
            want = [SH.shifted_inputs(xb[b], ub[b], None, k, tail) for b in range(B)]
            x1p, up = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
            restore()
            a.shift_horizon_(k, tail=tail)                                        # open loop
            xs, us = a.get_trajectory()
            assert np.array_equal(us, up) and np.array_equal(xs[:, 0], x1p), (nm, k, tail)
            ref.initialize_rollout_(x1p, up)
            assert _eq(_state(a)[:2], _state(ref)[:2]), (nm, k, tail)
            restore()
            a.shift_horizon_(k, x1=x1, feedback=True, tail=tail)                  # closed loop from a measured start
            xs, us = a.get_trajectory()
            assert np.array_equal(xs[:, 0], x1) and np.array_equal(us[:, N - k:], up[:, N - k:]), (nm, k, tail)
            ref.initialize_rollout_(x1, us)
            assert _eq(_state(a)[:2], _state(ref)[:2]), (nm, k, tail)
            for b in range(B):
                r = M.shift_head(p, xb[b], ub[b], K[b], None, k, x1[b])
                assert r["first_nonfinite"] == -1, (nm, k, b)
                worst["x"] = max(worst["x"], P.rel(xs[b, :T - k], r["x"])); worst["u"] = max(worst["u"], P.rel(us[b, :N - k], r["u"]))
                assert np.abs(us[b, :N - k] - ub[b, k:]).max() > 1e-6, (nm, k, b)  # not the open-loop shift
            restore()
            a.shift_horizon_(k, feedback=True, tail=tail)                         # feedback from x̄_k
            xs, us = a.get_trajectory()
            assert np.array_equal(xs[:, 0], x1p) and np.array_equal(us[:, N - k:], up[:, N - k:]), (nm, k, tail)
            worst["nominal"] = max(worst["nominal"], P.rel(us, up))
    print("mpc sweep, shift %dx%d: %s" % (n, m, worst))
    assert worst["x"] < TOL_XU and worst["u"] < TOL_XU and worst["nominal"] < TOL_XU, (nm, worst)
    a.close(); ref.close()


# --------------------------------------------------------------------------------------------------- lowered problems
def _selectors_stay(sol, w=None):
    """the parameter block of every instance: the user's columns, then the handle's selector table"""
    th = sol.buffer("parameters").reshape(sol.B, sol.T, -1)
    ns = sol._selectors.shape[1]
    assert th.shape[2] == sol.num_user_parameter + ns and ns > 0
    assert np.array_equal(th[:, :, th.shape[2] - ns:], np.broadcast_to(sol._selectors[None], (sol.B,) + sol._selectors.shape))
    if w is not None:
        assert np.array_equal(th[:, :, :th.shape[2] - ns], w)


@pytest.mark.parametrize("route", ["symbolic", "c_sources"])
def test_lowered_car_tv_on_the_four_entry_points(pkg, oracle, route):
    """car_tv: selectors in all three categories, no user parameters. Policy rollout and candidates against the oracle's genuinely
    per-step problem and the yardstick, sampling against the materialised path, the re-anchoring shift (steps = 0, feedback, a
    measured x1) against the yardstick's head; the selector columns are the handle's after every call."""
    S, size = 70, P.CASES["car"][2]
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    ub = np.ascontiguousarray(ub[:, :T - 1])
    dynamics, costs, constraints = pkg.models.car_tv(T)
    make = (lambda: pkg.Solver(dynamics, costs, constraints, batch=B, options=pkg.Options(verbose=0), name="car_tv")) if route == "symbolic" else \
           (lambda: pkg.Solver(stage_sources=pkg.lowering.c_stage_sources(dynamics, costs, constraints), batch=B, options=pkg.Options(verbose=0), name="car_tv_c"))
    sol, other = make(), make()
    assert (sol.nx, sol.nu, sol.num_user_parameter) == (3, 2, 0) and sol._selectors.shape[1] > 0
    p = M.car_tv(T)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    xb, ubs = sol.get_trajectory(); K, k = sol.get_policy()
    starts = np.stack([P.perturbed_starts(xb[b, 0], S, size, seed=P.SEED + b) for b in range(B)])
    out = sol.rollout_policy(starts, trajectories=True)
    _check_rollouts(out, [[P.oracle_reading(oracle, "car_tv", T, xb[b], ubs[b], K[b], starts[b, s]) for s in range(S)] for b in range(B)],
                    starts, "car_tv %s oracle" % route)
    for alpha in (0.0, 0.5):
        o = out if alpha == 0.0 else sol.rollout_policy(starts, step_size=alpha, trajectories=True)
        _check_rollouts(o, [[M.policy_rollout(*p, xb[b], ubs[b], K[b], k[b], starts[b, s], alpha, None) for s in range(S)] for b in range(B)],
                        starts, "car_tv %s step %.1f" % (route, alpha))
    assert (out["max_violation"] > 0).any()
    _selectors_stay(sol)
    u = np.stack([CR.candidates(ub[b], S, CR.CASES["car"][2], b) for b in range(B)])
    got = sol.initialize_rollout_candidates_(x1, u)
    _check_scores(got, [CR.score_all(oracle, "car_tv", T, x1[b], u[b]) for b in range(B)], "car_tv %s oracle" % route)
    _check_scores(got, [M.score_all(p, x1[b], u[b]) for b in range(B)], "car_tv %s" % route)
    _check_installation(sol, other, x1, u[np.arange(B), got["chosen"]])
    _selectors_stay(sol)
    _check_sampling(sol, other, x1, ub, np.array([0.004, 0.008]), "%s" % sol.model)
    _selectors_stay(sol); _selectors_stay(other)
    sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ubs)
    measured = M.measured_starts(xb, 0, size)
    sol.shift_horizon_(0, feedback=True, x1=measured)
    xs, us = sol.get_trajectory()
    assert np.array_equal(xs[:, 0], measured)
    worst = dict(x=0.0, u=0.0)
    for b in range(B):
        r = M.shift_head(p, xb[b], ubs[b], K[b], None, 0, measured[b])
        assert r["first_nonfinite"] == -1
        worst["x"] = max(worst["x"], P.rel(xs[b], r["x"])); worst["u"] = max(worst["u"], P.rel(us[b], r["u"]))
    print("mpc sweep, shift car_tv %s: %s" % (route, worst))
    assert worst["x"] < TOL_XU and worst["u"] < TOL_XU, worst
    other.initialize_rollout_(measured, us)
    assert _eq(_state(sol)[:2], _state(other)[:2])
    _selectors_stay(sol)
    with pytest.raises(pkg._ffi.IlqrError, match="stage selectors"):
        sol.shift_horizon_(1)
    sol.close(); other.close()


ALT_WEIGHT = lambda t: 1.0e-2 if t % 2 == 0 else 2.0e-2


def _car_obs_alternating(pkg):
    """car_obs's objects (two user parameters) with two stage-cost kinds alternating along the horizon: the model's own and the same
    with the action weight doubled — user columns and selector columns in θ at once"""
    mdl = pkg.models.car_obs()
    xT = [1.0, 1.0, 0.0]
    doubled = pkg.Cost(lambda x, u, w: 1.0 * sum((x[i] - xT[i]) * (x[i] - xT[i]) for i in range(3)) + 2.0e-2 * (u[0] * u[0] + u[1] * u[1]),
                       3, 2, num_parameter=2)
    costs = [mdl["cost_stage"] if t % 2 == 0 else doubled for t in range(T - 1)] + [mdl["cost_term"]]
    return lambda: pkg.Solver([mdl["dynamics"]] * (T - 1), costs, [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B,
                              options=pkg.Options(verbose=0), name="car_obs_alt")


def test_lowered_problem_with_user_parameters(pkg):
    """n_sel > 0 and user parameters at once: a policy rollout under per-sample w of the USER's two columns keeps the handle's
    selector column pair (the yardstick's stage cost picks its kind by t); candidates and sampling run under the handle's θ."""
    S, size = 70, P.CASES["car_obs"][2]
    _, _, x1, ub = pkg.workloads.make_inputs("car_obs", B)
    ub = np.ascontiguousarray(ub[:, :T - 1])
    w = np.ascontiguousarray(SH.time_varying(pkg.workloads.make_parameters("car_obs", B))[:, :T])
    make = _car_obs_alternating(pkg)
    sol, other = make(), make()
    assert (sol.nx, sol.nu, sol.num_user_parameter, sol.nw) == (3, 2, 2, 2) and sol._selectors.shape == (T, 2)
    assert np.array_equal(sol._selectors[:T - 1, 0], np.arange(T - 1) % 2 == 0)
    p = M.car_obs(ALT_WEIGHT)
    for s_ in (sol, other):
        s_.set_parameters_(w)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    xb, ubs = sol.get_trajectory(); K, k = sol.get_policy()
    starts = np.stack([P.perturbed_starts(xb[b, 0], S, size, seed=P.SEED + b) for b in range(B)])
    ws = np.stack([P.sample_parameters(w[b], S, seed=P.SEED + 100 + b) for b in range(B)])
    assert ws.shape == (B, S, T, 2)
    for alpha in (0.0, 0.5):
        out = sol.rollout_policy(starts, w=ws, step_size=alpha, trajectories=True)
        _check_rollouts(out, [[M.policy_rollout(*p, xb[b], ubs[b], K[b], k[b], starts[b, s], alpha, ws[b, s]) for s in range(S)] for b in range(B)],
                        starts, "car_obs_alt per-sample w, step %.1f" % alpha)
        assert (out["max_violation"] > 0).any()
        _selectors_stay(sol, w)
    plain = sol.rollout_policy(starts, trajectories=True)                           # the handle's own θ
    _check_rollouts(plain, [[M.policy_rollout(*p, xb[b], ubs[b], K[b], k[b], starts[b, s], 0.0, w[b]) for s in range(S)] for b in range(B)],
                    starts, "car_obs_alt handle w")
    # A third column per row is not the user's to give. The C ABI takes a bare pointer and no width, so it cannot refuse; the
    # wrapper takes [B][S][T][num_parameter] — the USER's width, not the template's — and its reshape refuses any other size.
    three = np.concatenate([ws, np.full(ws.shape[:3] + (1,), 7.0)], axis=3)
    assert three.shape[3] == sol.num_user_parameter + 1 == sol._selectors.shape[1] + 1        # (the template's width is 4)
    with pytest.raises(ValueError, match="cannot reshape array of size %d into shape \\(%d,%d,%d,2\\)" % (three.size, B, S, T)):
        sol.rollout_policy(starts, w=three, trajectories=True)
    _selectors_stay(sol, w)
    u = np.stack([CR.candidates(ub[b], S, CR.CASES["car_obs"][2], b) for b in range(B)])
    got = sol.initialize_rollout_candidates_(x1, u)
    _check_scores(got, [M.score_all(p, x1[b], u[b], w[b]) for b in range(B)], "car_obs_alt")
    assert (got["max_violation"] > 0).any()
    _check_installation(sol, other, x1, u[np.arange(B), got["chosen"]])
    _selectors_stay(sol, w)
    smp = _check_sampling(sol, other, x1, ub, np.array([0.004, 0.008]), "%s" % sol.model)
    _check_scores(smp, [M.score_all(p, x1[b], smp["u"][b], w[b]) for b in range(B)], "car_obs_alt sampled", choice=False)
    _selectors_stay(sol, w); _selectors_stay(other, w)
    sol.close(); other.close()


def _synth5w_alternating(pkg):
    """mpc_ref.synth5w as the device's objects: nx = 5 (the LARGE form), one user parameter, two stage-cost kinds alternating"""
    import sympy as sp
    f, stage, term, box = M.synth5w_functions(sp.sin)
    dyn = pkg.Dynamics(f, 5, 1, num_parameter=1)
    kinds = [pkg.Cost(stage(r), 5, 1, num_parameter=1) for r in M.SYNTH5W_WEIGHTS]
    con = pkg.Constraint(box, 5, 1, indices_inequality=[1, 2], num_parameter=1)
    costs = [kinds[t % 2] for t in range(T - 1)] + [pkg.Cost(term, 5, 0, num_parameter=1)]
    return lambda: pkg.Solver([dyn] * (T - 1), costs, [con] * (T - 1) + [pkg.Constraint()], batch=B, options=pkg.Options(verbose=0),
                              name="synth5w_alt")


def test_lowered_problem_with_user_parameters_on_the_large_form(pkg):
    """The same on the one-wave-per-sample kernels: nx = 5 with a user parameter that enters dynamics and costs, and two selector
    columns behind it. Under per-sample w the large policy kernel must take column 0 from the sample and columns 1, 2 from the
    handle — a sample's w has ONE column per row, so reading a selector from it picks up the next rows' parameters."""
    S = M.samples(5, 1)
    x1, ub = M.sweep_inputs(5, 1)
    w = M.synth5w_parameters()
    make = _synth5w_alternating(pkg)
    sol, other = make(), make()
    assert (sol.nx, sol.nu, sol.num_user_parameter, sol.nw) == (5, 1, 1, 1) and sol._selectors.shape == (T, 2)
    p = M.synth5w()
    for s_ in (sol, other):
        s_.set_parameters_(w)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    xb, ubs = sol.get_trajectory(); K, k = sol.get_policy()
    assert np.isfinite(K).all() and np.array_equal(xb[:, 0], x1)
    starts = M.rollout_starts(xb, S)
    ws = np.stack([P.sample_parameters(w[b], S, seed=P.SEED + 100 + b) for b in range(B)])
    assert ws.shape == (B, S, T, 1)
    for alpha in (0.0, 0.5):
        out = sol.rollout_policy(starts, w=ws, step_size=alpha, trajectories=True)
        assert _same(sol.rollout_policy(starts, w=ws, step_size=alpha), out, ("cost", "max_violation", "first_nonfinite"))
        _check_rollouts(out, [[M.policy_rollout(*p, xb[b], ubs[b], K[b], k[b], starts[b, s], alpha, ws[b, s]) for s in range(S)] for b in range(B)],
                        starts, "synth5w_alt per-sample w, step %.1f" % alpha)
        assert (out["max_violation"] > 0).any()
        _selectors_stay(sol, w)
    plain = sol.rollout_policy(starts, trajectories=True)                           # the handle's own θ
    _check_rollouts(plain, [[M.policy_rollout(*p, xb[b], ubs[b], K[b], k[b], starts[b, s], 0.0, w[b]) for s in range(S)] for b in range(B)],
                    starts, "synth5w_alt handle w")
    u = M.candidate_set(ub, S)
    got = sol.initialize_rollout_candidates_(x1, u)
    _check_scores(got, [M.score_all(p, x1[b], u[b], w[b]) for b in range(B)], "synth5w_alt")
    assert (got["max_violation"] > 0).any()
    _check_installation(sol, other, x1, u[np.arange(B), got["chosen"]])
    _selectors_stay(sol, w)
    smp = _check_sampling(sol, other, x1, ub, M.sigma(1), "synth5w_alt")
    _check_scores(smp, [M.score_all(p, x1[b], smp["u"][b], w[b]) for b in range(B)], "synth5w_alt sampled", choice=False)
    _selectors_stay(sol, w); _selectors_stay(other, w)
    sol.set_buffer("nominal_states", xb); sol.set_buffer("nominal_actions", ubs)
    measured = M.measured_starts(xb, 0)
    sol.shift_horizon_(0, feedback=True, x1=measured)                               # re-anchoring is allowed on a lowered handle
    xs, us = sol.get_trajectory()
    worst = dict(x=0.0, u=0.0)
    for b in range(B):
        r = M.shift_head(p, xb[b], ubs[b], K[b], w[b], 0, measured[b])
        assert r["first_nonfinite"] == -1
        worst["x"] = max(worst["x"], P.rel(xs[b], r["x"])); worst["u"] = max(worst["u"], P.rel(us[b], r["u"]))
    print("mpc sweep, shift synth5w_alt: %s" % worst)
    assert np.array_equal(xs[:, 0], measured) and worst["x"] < TOL_XU and worst["u"] < TOL_XU, worst
    _selectors_stay(sol, w)
    sol.close(); other.close()


def _ragged_score(O, pr, x1, u):
    """the oracle's open-loop rollout of the padded (x1, u) on its genuinely ragged problem: x (padded), cost, max_violation"""
    x = pr.rollout(x1, u)
    s = O.Solver(pr, O.default_options())
    s.set_buffer("states", pr.pack_states(x)); s.set_buffer("actions", pr.pack_actions(u))
    for nm in ("constraint_dual", "constraint_penalty"):
        s.set_buffer(nm, np.zeros_like(s.buffer(nm)))
    s.call("cost_bang", 1)
    st = s.stats()
    return x, float(st.objective), float(st.max_violation)


def test_lowered_ragged_dimensions(pkg, oracle):
    """Time-varying dimensions, zero-padded: policy rollout and candidates with padded x1 and u. The padding of x and u in the
    trajectories is exactly zero; the closed loop equals the yardstick on the restatement's per-step objects; cost and violation
    equal the oracle's on its ragged problem (padded actions carry u² / 2, which is 0 here)."""
    Tr, S = M.T_RAGGED, 70
    dynamics, costs, constraints, n_t, m_t = pkg.models.ragged(Tr)
    pr = oracle.Problem("ragged", Tr)
    p, _, rn_t, rm_t = M.ragged(Tr)
    assert (pr.state_dims, pr.action_dims) == (n_t, m_t) == (rn_t, rm_t)
    n, m = pr.nx, pr.nu
    x1, ub, u = M.ragged_inputs(n_t, m_t, B, S)
    make = lambda: pkg.Solver(dynamics, costs, constraints, batch=B, options=pkg.Options(verbose=0), name="ragged")
    sol, other = make(), make()
    assert (sol.nx, sol.nu, sol.state_dims, sol.action_dims) == (n, m, n_t, m_t)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    xb, ubs = sol.get_trajectory(); K, k = sol.get_policy()
    starts = M.ragged_starts(xb, n_t[0], S)
    out = sol.rollout_policy(starts, trajectories=True)
    _check_rollouts(out, [[M.policy_rollout(*p, xb[b], ubs[b], K[b], k[b], starts[b, s], 0.0, None) for s in range(S)] for b in range(B)],
                    starts, "ragged")
    for t in range(Tr):
        assert (out["x"][:, :, t, n_t[t]:] == 0).all()
    for t in range(Tr - 1):
        assert (out["u"][:, :, t, m_t[t]:] == 0).all()
    worst = dict(x=0.0, cost=0.0, viol=0.0)
    for b in range(B):
        for s in range(0, S, 7):
            x, J, v = _ragged_score(oracle, pr, starts[b, s], out["u"][b, s])
            worst["x"] = max(worst["x"], P.rel(out["x"][b, s], x))
            worst["cost"] = max(worst["cost"], _relv(out["cost"][b, s], J)); worst["viol"] = max(worst["viol"], _relv(out["max_violation"][b, s], v))
    print("mpc sweep, ragged policy rollout against the oracle: %s" % worst)
    assert worst["x"] < TOL_XU and worst["cost"] < TOL_COST and worst["viol"] < TOL_VIOL, worst
    assert (out["max_violation"] > 0).any()
    got = sol.initialize_rollout_candidates_(x1, u)
    refs = []
    for b in range(B):
        sc = [_ragged_score(oracle, pr, x1[b], u[b, s]) for s in range(S)]
        refs.append(dict(cost=np.array([r[1] for r in sc]), max_violation=np.array([r[2] for r in sc]),
                         first_nonfinite=np.array([P.first_nonfinite(r[0]) for r in sc], dtype=np.int32)))
    _check_scores(got, refs, "ragged oracle")
    _check_scores(got, [M.score_all(p, x1[b], u[b]) for b in range(B)], "ragged")
    _check_installation(sol, other, x1, u[np.arange(B), got["chosen"]])
    xs = sol.get_trajectory()[0]
    for t in range(Tr):
        assert (xs[:, t, n_t[t]:] == 0).all()
    sol.close(); other.close()
