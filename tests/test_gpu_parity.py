"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle (a restatement of the reference: "parity unpinned" by
reference output).

Tolerances (fp64), as asserted below: stage level 2e-11 relative for the linearisation (rounding only: FMA contraction, device
sincos, reduction order), 1e-8 for Riccati outputs after 50-100 recursion steps; whole solve on small models |Δx|, |Δu| ≤ 2e-8,
|ΔK| ≤ 1e-7·max|K|, |Δk| ≤ 1e-8·max|k| with control flow identical on ≥ 99.9 % of the instances of a batch (observed at BASELINE sizes,
profiles/r05_parity.txt: 100 %, 4e-9, 2e-8; |Δk| 1.1e-9); large models (synth32, synth12) |Δx|, |Δu| ≤ 1e-11, |ΔK| ≤ 1e-11·max|K|,
|Δk| ≤ 1e-13·max|k| on the literal BASELINE workload with control flow identical on every instance (observed 2e-15 / 1e-14 / 3e-15 / 1e-14).
Instances whose control flow differs must still end the reference's way (tests/parity_check.py). Whole solves run on both input
generators where bench.py's (splitmix64) differs from the profiles' (pcg64).
"""
import os
import sys

import numpy as np
import pytest

import parity_check
from oracle_sync import SYNC, sync_from_oracle as _sync_from_oracle  # noqa: F401
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    return p


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _oracle_solver(oracle, model, T, x1, ub):
    pr = oracle.Problem(model, T)
    xb = pr.rollout(x1, ub)
    s = oracle.Solver(pr, oracle.default_options())
    s.initialize_controls(ub); s.initialize_states(xb)
    return pr, s, xb


@pytest.mark.parametrize("config", ["particle", "acrobot", "car", "car_goal", "synth32"])
def test_stagewise_parity(pkg, oracle, config):
    """Each stage kernel against the oracle's function on IDENTICAL inputs (state copied from the
    oracle before every stage), over three inner iterations — the later ones exercise Hessian
    accumulation (Q1), active sets and non-zero duals after an AL update."""
    B = 5 if config != "synth32" else 2
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    if config == "synth32":   # push the controls into the action box so that the inequality set is exercised
        ub = ub + 1.2 * np.sin(np.arange(ub.size).reshape(ub.shape))
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub)
    triples = [_oracle_solver(oracle, model, T, x1[b], ub[b]) for b in range(B)]
    refs = [t[1] for t in triples]
    xb = sol.buffer("nominal_states")
    for b in range(B):
        assert _rel(xb[b], triples[b][2].ravel()) < 1e-12                 # rollout()
    n, m = sol.nx, sol.nu
    tol = 2e-11
    grads = ["jacobian_state", "jacobian_action", "gradient_state", "gradient_action",
             "hessian_state_state", "hessian_action_action", "hessian_action_state"]

    def compare(names, where, t=tol):
        for name in names:
            gb = sol.buffer(name)
            for b in range(B):
                assert _rel(gb[b], refs[b].buffer(name)) < t, (where, name, b, _rel(gb[b], refs[b].buffer(name)))

    for r in refs:
        r.call("reset_model_objective")
    for it in range(3):
        if it == 2:
            for r in refs:                       # non-trivial duals / penalties for the last round
                r.call("augmented_lagrangian_update") if r.problem.c.constraints else None
        _sync_from_oracle(sol, refs, T)
        sol.run_stage_("cost_nominal")
        for r in refs: r.call("cost_bang", 0)
        st = sol.stats()
        for b in range(B):
            assert st["objective"][b] == pytest.approx(refs[b].stats().objective, rel=1e-12), (it, b)
            assert st["max_violation"][b] == pytest.approx(refs[b].stats().max_violation, rel=1e-12, abs=1e-14)
        compare(["violations", "active_set"], (it, "cost"))
        _sync_from_oracle(sol, refs, T)
        sol.run_stage_("gradients")
        for r in refs: r.call("gradients")
        compare(grads, (it, "gradients"))
        _sync_from_oracle(sol, refs, T)
        sol.run_stage_("backward_pass")
        for r in refs:
            r.call("backward_pass"); r.call("lagrangian_gradient")
        compare(["K", "k", "P", "p"], (it, "backward"), 1e-8)   # Riccati recursion amplifies rounding over the horizon
        Lx = sol.buffer("gradient_state_lagrangian"); Lu = sol.buffer("gradient_action_lagrangian")
        for b in range(B):
            g = refs[b].buffer("gradient")
            assert _rel(Lx[b], g[:(T - 1) * n]) < 1e-8 and _rel(Lu[b], g[T * n:]) < 1e-8
        _sync_from_oracle(sol, refs, T)
        sol.run_stage_("forward_pass")
        for r in refs: r.call("forward_pass")
        st = sol.stats()
        for b in range(B):
            o = refs[b].stats()
            assert st["step_size"][b] == o.step_size and st["status"][b] == o.status, (it, b)
            assert st["objective"][b] == pytest.approx(o.objective, rel=1e-11)
        compare(["states", "actions", "nominal_states", "nominal_actions", "violations"], (it, "forward"), 1e-10)
    sol.close()


GENERATORS = ("pcg64", "splitmix64")        # workloads.make_inputs: the profiles' inputs, and the library's own that bench.py times
ORACLE_THREADS = 16
# |Δk| / max(max |k|, 1) per instance: ~10x what is observed, never looser than |ΔK|'s bound (observed: acrobot, car at BASELINE sizes on
# either generator 1.1e-9 at most; synth32, synth12 1e-14 at most)
TOL_K_SMALL = 1e-8
TOL_K_LARGE = 1e-13


def _num_simds():
    """4 x the device's CUs: the batch size up to which auto puts one instance on every SIMD (csrc/ilqr_launch_plan.hpp)."""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


_ORACLE_SOLVES = {}      # (config, B, offset, generator) -> the oracle's solve, for callers that ask for the same batch (reuse_oracle)


def _whole_solve(pkg, oracle, config, B, min_match, generator="pcg64", offset=0, expect_kernel=None, tol=2e-8, tol_K=1e-7,
                 tol_k=TOL_K_SMALL, chaotic=False, reuse_oracle=False):
    """Solve config's B instances (make_inputs(config, B, offset, generator), options CONFIG_OPTIONS[config]) on the device and on the
    oracle and compare them (parity_check.compare). expect_kernel: what auto must pick for this handle. chaotic: allow the
    self-perturbation rule (parity_check.chaotic) — only where it holds, the long acrobot shards. reuse_oracle: keep the oracle's
    solve for (and take it from) another test of the same batch — the device solve is run and compared in every test."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B, offset=offset, generator=generator)
    kw = pkg.workloads.CONFIG_OPTIONS.get(config, {})
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, **kw))
    if expect_kernel is not None:
        assert sol.resolved_kernel_variant() == expect_kernel, (config, B, sol.resolved_kernel_variant(), expect_kernel)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    sol.close()
    opts = oracle.default_options(**kw)
    key = (config, B, offset, generator)
    ref = _ORACLE_SOLVES.get(key) if reuse_oracle else None
    if ref is None:
        ref = oracle.solve_batch(model, T, x1, ub, options=opts, nthreads=ORACLE_THREADS)
        if reuse_oracle:
            _ORACLE_SOLVES[key] = ref

    def spread(idx):          # the oracle against itself with ū perturbed by one part in 1e15
        pert = oracle.solve_batch(model, T, x1[idx], ub[idx] * (1.0 + 1e-15), options=opts, nthreads=ORACLE_THREADS)
        return parity_check.errors(pert, {f: ref[f][idx] for f in ("x", "u", "K", "k")})
    one = oracle.Problem(model, 2)          # one step of the dynamics: x_t+1 = f(x_t, u_t)
    # tolerances ~10x what is observed on every BASELINE-size workload (profiles/r04_parity.txt, r05_parity.txt: control flow
    # identical on 100 % of the instances, max |dx|, |du| 1.6e-9, max |dK| / max |K| 2.2e-8)
    r = parity_check.compare(dict(x=x, u=u, K=K, k=k, stats=st), ref, min_match=min_match, tol=tol, tol_K=tol_K, tol_k=tol_k,
                             constraint_tolerance=opts.constraint_tolerance, max_dual_updates=opts.max_dual_updates,
                             spread=spread if chaotic else None, step=lambda x, u: one.rollout(x, u[None])[1], x1=x1)
    print("\n%s B=%d offset=%d %s (%s): control flow identical on %.2f%%, %d other paths, %d chaotic; max |dx| %.2e |du| %.2e "
          "|dK| %.2e |dk| %.2e (bounds %.0e %.0e %.0e %.0e)" % (config, B, offset, generator, expect_kernel, 100 * r["frac"],
          len(r["differ"]), len(r["loose"]), r["dx"], r["du"], r["dK"], r["dk"], tol, tol, tol_K, tol_k))
    r.update(x=x, u=u, K=K, k=k, st=st, ref=ref, x1=x1, ub=ub)
    return r


def test_particle_whole_solve(pkg, oracle):
    _whole_solve(pkg, oracle, "particle", 64, 0.999)


def test_acrobot_whole_solve_t51(pkg, oracle):
    r = _whole_solve(pkg, oracle, "acrobot51", 64, 0.999)
    assert (np.abs(r["x"][:, -1, :] - [np.pi, 0, 0, 0]).max(1) < 5e-3).all()      # test/acrobot.jl:114


@pytest.mark.parametrize("generator", GENERATORS)
def test_acrobot_whole_solve_headline(pkg, oracle, generator):
    """BASELINE configs[1]: acrobot T=101, batch=1024 — on splitmix64, the very instances bench.py times (one instance per SIMD)."""
    r = _whole_solve(pkg, oracle, "acrobot", 1024, 0.999, generator=generator, expect_kernel="latency")
    assert (np.abs(r["x"][:, -1, :] - [np.pi, 0, 0, 0]).max(1) < 5e-3).mean() > 0.99


def _car_instance_0(r):
    """test/car.jl:74-79 on instance 0 (the reference's deterministic initialisation, test/car.jl:24-29, under either generator)."""
    x, u = r["x"], r["u"]
    e = x[0, :-1, :2] - 0.5
    ct = np.c_[-5.0 - u[0], u[0] - 5.0, 0.01 - (e * e).sum(1)]
    assert (ct <= 5e-3).all()
    assert (np.abs(x[0, -1] - [1.0, 1.0, 0.0]) <= 5e-3).all()
    assert r["st"]["iterations"][0] == 92 and r["st"]["outer_iterations"][0] == 2


def test_car_whole_solve(pkg, oracle):
    r = _whole_solve(pkg, oracle, "car", 256, 0.999)
    _car_instance_0(r)


def test_car_goal_whole_solve(pkg, oracle):
    _whole_solve(pkg, oracle, "car_goal", 256, 0.999)


def test_resolve_is_deterministic(pkg):
    """reset + initialise + solve twice gives bitwise identical results."""
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot51", 32)
    sol = pkg.Solver(model=model, horizon=T, batch=32, options=pkg.Options(verbose=0))
    outs = []
    for _ in range(2):
        sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()
        outs.append(sol.get_trajectory() + sol.get_policy())
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    sol.close()


@pytest.mark.parametrize("generator", GENERATORS)
def test_car_full_config_batch_4096(pkg, oracle, generator):
    """BASELINE configs[2]: car T=51 with the full constraint set, batch=4096 on one GPU: the packed kernel, two waves per pack,
    whose last survivors the latency kernel finishes in a resume launch (hand-over by head count)."""
    r = _whole_solve(pkg, oracle, "car", 4096, 0.999, generator=generator, expect_kernel="packed2", reuse_oracle=True)
    st = r["st"]
    assert (st["max_violation"] <= 5e-3).mean() > 0.999
    _car_instance_0(r)


@pytest.mark.parametrize("generator", GENERATORS)
def test_acrobot_shard_of_65536_properties(pkg, oracle, generator):
    """BASELINE configs[3]: one 8192-instance shard of the 65536 batch (rank 3 of 8) on the one-wave packed kernel — every instance
    against the oracle (x, u, K, k, control flow; chaotic instances by the self-perturbation rule), and size-independent
    properties: the reference's terminal-goal test, determinism, and batch-size independence (an instance's result does not
    depend on which batch it is solved in)."""
    B = 8192
    lo, hi = pkg.distributed.shard_range(3, B)
    r = _whole_solve(pkg, oracle, "acrobot", B, 0.995, generator=generator, offset=lo, expect_kernel="packed1", chaotic=True)
    model, T, x1, ub = "acrobot", 101, r["x1"], r["ub"]
    x, u, st, full = r["x"], r["u"], r["st"], r["ref"]
    ok = np.abs(x[:, -1, :] - [np.pi, 0, 0, 0]).max(1) < 5e-3          # test/acrobot.jl:114
    assert ok.mean() > 0.995, ok.mean()
    # a few random ū make the open-loop acrobot rollout itself overflow; those instances are NaN
    # from the start in the reference too, everything else must stay finite
    x0 = oracle.Problem(model, T)
    diverged = np.array([not np.isfinite(x0.rollout(x1[b], ub[b])).all() for b in range(B)])
    assert diverged.mean() < 0.005
    assert np.isfinite(x[~diverged]).all() and np.isfinite(u[~diverged]).all()
    assert r["same"][diverged].all()                                  # NaN instances: identical control flow
    # Quu may lose positive definiteness on rare instances (the reference ignores potrf's info,
    # src/backward_pass.jl:69): the oracle must report the same on those instances
    bad = np.nonzero((st["potrf_info"] != 0) | diverged)[0][:16]
    assert bad.size < 0.01 * B
    if generator == "pcg64":
        _shard_sample_checks(oracle, model, T, x1, ub, x, st, full, bad, diverged)
    sub = slice(100, 164)
    small = pkg.Solver(model=model, horizon=T, batch=64, options=pkg.Options(verbose=0))
    small.initialize_rollout_(x1[sub], ub[sub]); small.solve_()
    xs, us = small.get_trajectory()
    assert np.array_equal(xs, x[sub]) and np.array_equal(us, u[sub])
    small.close()


def _shard_sample_checks(oracle, model, T, x1, ub, x, st, full, bad, diverged):
    """The config-4 shard's checks on a sample of its instances (every 257th and the first 16 with a failed pivot or an overflowing
    rollout), which the comparison of the whole shard supersedes: kept for the pcg64 shard as they were. (A sample that rich in
    failed pivots — where the chaotic instances are — is no sample of the control flow: on the splitmix64 shard one of its 36
    instances, instance 735, takes another path, as the oracle does itself when ū moves by one part in 1e15.)"""
    B = len(x)
    idx = np.unique(np.r_[bad, np.arange(0, B, 257)])
    ref = {f: full[f][idx] for f in ("x", "u", "K", "k")}
    ref["stats"] = {f: v[idx] for f, v in full["stats"].items()}
    same = (st["iterations"][idx] == ref["stats"]["iterations"]) & (st["rollouts"][idx] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.995, same.mean()
    assert same[np.isin(idx, np.nonzero(diverged)[0])].all()          # NaN instances: identical control flow
    assert ((st["potrf_info"][idx] != 0) == (ref["stats"]["potrf_info"] != 0))[same].all()
    fin = same & ~diverged[idx]
    ex = np.abs(x[idx] - ref["x"]).reshape(len(idx), -1).max(1)
    # 2e-8 like every whole-solve test — except on CHAOTIC instances (hundreds of iterations on the iteration cap), recognised by the
    # criterion tools/all_shards.py prints: the oracle differs from ITSELF by more than a tenth of that when ū is perturbed by one
    # part in 1e15 (profiles/r05_all_shards.txt: 3e-6 on the slowest instances of a shard)
    loose = np.nonzero(fin & (ex > 2e-8))[0]
    assert loose.size <= 0.02 * len(idx), loose.size
    if loose.size:
        pert = oracle.solve_batch(model, T, x1[idx[loose]], ub[idx[loose]] * (1.0 + 1e-15), nthreads=8)
        own = np.abs(pert["x"] - ref["x"][loose]).reshape(loose.size, -1).max(1)
        assert (ex[loose] <= 10.0 * own).all(), (ex[loose], own)


def test_unconstrained_solver_path(pkg, oracle):
    """Solver(dynamics, costs) without constraints → plain ilqr_solve! (src/solve.jl:137-139)."""
    B, T = 16, 31
    rng = np.random.default_rng(5)
    x1 = 0.3 * rng.standard_normal((B, 2)); ub = 0.1 * rng.standard_normal((B, T - 1, 1))
    sol = pkg.Solver(model="pendulum_euler", horizon=T, batch=B, constraints=False, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    pk = pkg.Solver(model="pendulum_euler", horizon=T, batch=B, constraints=False, options=pkg.Options(verbose=0))
    pk.set_kernel_variant_("packed")
    pk.initialize_rollout_(x1, ub); pk.solve_()
    assert np.abs(pk.get_trajectory()[0] - x).max() < 1e-9 and (pk.stats()["iterations"] == st["iterations"]).all()
    assert (pk.stats()["outer_iterations"] == 0).all()
    pk.close()
    ref = oracle.solve_batch("pendulum_euler", T, x1, ub, nthreads=4)
    assert (st["iterations"] == ref["stats"]["iterations"]).all()
    assert np.abs(x - ref["x"]).max() < 1e-8 and np.abs(u - ref["u"]).max() < 1e-8
    assert (st["outer_iterations"] == 0).all()
    sol.close()


OPTION_SETS = [
    dict(max_iterations=3),
    dict(max_dual_updates=2),
    dict(min_step_size=0.3),
    dict(constraint_tolerance=1.0e-6),
    dict(initial_constraint_penalty=10.0, scaling_penalty=2.0, max_penalty=50.0),
    dict(objective_tolerance=1.0e-9, lagrangian_gradient_tolerance=1.0e-9, max_iterations=20),
    dict(line_search=0, max_iterations=4),
    dict(reset_cache=1),
]


@pytest.mark.parametrize("variant", ["auto", "packed"])
@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_options_control_flow(pkg, oracle, opts, variant):
    """Every Options field that steers the solve loops (src/options.jl:1-15, src/solve.jl) must steer
    the device loops identically: same iteration / rollout / outer counts and the same trajectories."""
    B, T = 12, 21
    rng = np.random.default_rng(17)
    x1 = np.zeros((B, 3)); x1[:, :2] = 0.05 * rng.standard_normal((B, 2))
    ub = 1.0e-2 * np.array([1.0, 0.1]) * (1.0 + 0.5 * rng.uniform(-1, 1, (B, T - 1, 1)))
    sol = pkg.Solver(model="car", horizon=T, batch=B, options=pkg.Options(verbose=0, **opts))
    sol.set_kernel_variant_(variant)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch("car", T, x1, ub, options=oracle.default_options(**opts), nthreads=4)
    rs = ref["stats"]
    for f in ("iterations", "outer_iterations", "rollouts", "status"):
        assert (st[f] == rs[f]).all(), (f, st[f], rs[f])
    assert np.abs(x - ref["x"]).max() < 1e-7 and np.abs(u - ref["u"]).max() < 1e-7
    assert np.allclose(st["step_size"], rs["step_size"])
    # J = Σℓ + λᵀc + ½ρc² cancels heavily once the duals are large (line_search = :none case): 1e-6 relative
    assert np.allclose(st["objective"], rs["objective"], rtol=1e-6)
    sol.close()


def test_warm_start_resolve_and_minimal_horizon(pkg, oracle):
    """solve!(solver) twice on the same solver (the second call starts from the first solution and
    keeps the `states` buffer, Appendix A Q2), and the smallest legal horizon T = 2."""
    B, T = 6, 31
    model, _, x1, ub = pkg.workloads.make_inputs("particle", B)
    ub = np.concatenate([ub, ub, ub], axis=1)[:, :T - 1]
    sol = pkg.Solver(model="particle", horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub); sol.solve_(); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    pk = pkg.Solver(model="particle", horizon=T, batch=B, options=pkg.Options(verbose=0))      # the same on the packed kernel
    pk.set_kernel_variant_("packed")
    pk.initialize_rollout_(x1, ub); pk.solve_(); pk.solve_()
    xp, up = pk.get_trajectory()
    assert np.abs(xp - x).max() < 1e-9 and (pk.stats()["iterations"] == st["iterations"]).all()
    pk.close()
    pr = oracle.Problem("particle", T)
    for b in range(B):
        s = oracle.Solver(pr); s.initialize_controls(ub[b]); s.initialize_states(pr.rollout(x1[b], ub[b]))
        s.solve(); s.solve()
        xo, uo = s.get_trajectory(); so = s.stats()
        assert (st["iterations"][b], st["outer_iterations"][b]) == (so.iterations, so.outer_iterations)
        assert np.abs(x[b] - xo).max() < 1e-9 and np.abs(u[b] - uo).max() < 1e-9
    sol.close()
    sol = pkg.Solver(model="car", horizon=2, batch=3, options=pkg.Options(verbose=0))
    x1 = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.2], [0.9, 0.9, 0.0]]); ub = np.full((3, 1, 2), 0.05)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch("car", 2, x1, ub, nthreads=1)
    assert (st["iterations"] == ref["stats"]["iterations"]).all()
    assert np.abs(x - ref["x"]).max() < 1e-8 and np.abs(u - ref["u"]).max() < 1e-8
    sol.close()


def test_lds_budget_error(pkg):
    """A horizon whose working set exceeds the 160 KiB LDS is served by the streaming packed kernel only: the
    LDS-resident stage kernels refuse it loudly (no silent fallback)."""
    sol = pkg.Solver(model="acrobot", horizon=600, batch=2)
    with pytest.raises(pkg._ffi.IlqrError, match="LDS"):
        sol.run_stage_("gradients")
    sol.close()


def test_parameters_car_obs(pkg, oracle):
    """Solver(...; parameters = θ) (src/solver.jl:12,29): per-instance, per-timestep obstacle centres."""
    B = 128
    model, T, x1, ub = pkg.workloads.make_inputs("car_obs", B)
    w = pkg.workloads.make_parameters("car_obs", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    assert sol.nw == 2
    sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch(model, T, x1, ub, w=w, nthreads=8)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.99
    assert np.abs(x - ref["x"])[same].max() < 1e-7 and np.abs(u - ref["u"])[same].max() < 1e-7
    far = oracle.solve_batch(model, T, x1, ub, w=np.full_like(w, 9.0), nthreads=8)
    assert (np.abs(far["x"] - ref["x"]).reshape(B, -1).max(1) > 1e-6).mean() > 0.5   # the parameters matter
    # the obstacle constraint is met w.r.t. each instance's own (moving) obstacle
    e = x[:, :-1, :2] - w[:, :-1, :]
    assert ((0.01 - (e * e).sum(-1)) <= 5e-3)[st["max_violation"] <= 5e-3].all()
    # parameters survive a fresh-solver reset; a second solve reproduces the first bit for bit
    sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()
    x2, _ = sol.get_trajectory()
    assert np.array_equal(x, x2)
    with pytest.raises(pkg._ffi.IlqrError, match="no parameters"):
        s2 = pkg.Solver(model="car", horizon=T, batch=2); s2.set_parameters_(np.zeros((2, T, 0)))
    sol.close()


def test_stage_selectors_leave_the_users_parameter_columns_alone(pkg):
    """ilqr_set_stage_selectors writes the LAST n_selectors parameter columns of every timestep; the user's columns (the first
    nw - n_selectors) keep what ilqr_set_parameters put there before (advisor finding, round 5: they were zeroed). Then
    ilqr_set_parameters takes the user's columns only and the selector column survives it."""
    import ctypes as C
    B = 4
    model, T, x1, ub = pkg.workloads.make_inputs("car_obs", B)
    w = pkg.workloads.make_parameters("car_obs", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.set_parameters_(w)
    sel = np.linspace(1.0, 2.0, T).reshape(T, 1)
    L = pkg._ffi.lib()
    pkg._ffi.check(L.ilqr_set_stage_selectors(sol._h, sel.ctypes.data_as(pkg._ffi.c_double_p), 1))
    got = sol.buffer("parameters").reshape(B, T, 2)
    assert np.array_equal(got[:, :, 0], w[:, :, 0]) and np.array_equal(got[:, :, 1], np.broadcast_to(sel[:, 0], (B, T)))
    w1 = np.ascontiguousarray(3.0 + w[:, :, :1])
    pkg._ffi.check(L.ilqr_set_parameters(sol._h, w1.ctypes.data_as(pkg._ffi.c_double_p)))
    got = sol.buffer("parameters").reshape(B, T, 2)
    assert np.array_equal(got[:, :, 0], w1[:, :, 0]) and np.array_equal(got[:, :, 1], np.broadcast_to(sel[:, 0], (B, T)))
    sol.close()


def test_user_defined_model_plugin_path(pkg, oracle):
    """The reference's user flow (examples/particle.jl:17-51): write f, ℓ, c as plain functions, build
    Dynamics/Cost/Constraint objects, hand lists of them to Solver. Here that goes through the code
    generator, hipcc and the model-module registry; results must equal the oracle's particle solve
    (and the built-in particle model bit for bit, since the generated code is the same)."""
    T, B = 11, 32
    xT = [1.0, 0.0]
    dyn = pkg.Dynamics(lambda x, u: [x[0] + x[1], x[1] + u[0]], 2, 1)
    stage = pkg.Cost(lambda x, u: 0.1 * (x[0] * x[0] + x[1] * x[1]) + 0.1 * u[0] * u[0], 2, 1)
    term = pkg.Cost(lambda x, u: 0.1 * (x[0] * x[0] + x[1] * x[1]), 2, 0)
    goal = pkg.Constraint(lambda x, u: [x[0] - xT[0], x[1] - xT[1]], 2, 0)
    none = pkg.Constraint()
    model, _, x1, ub = pkg.workloads.make_inputs("particle", B)
    sol = pkg.Solver([dyn] * (T - 1), [stage] * (T - 1) + [term], [none] * (T - 1) + [goal],
                     batch=B, options=pkg.Options(verbose=0), name="user_particle")
    assert (sol.nx, sol.nu, sol.nc_stage, sol.nc_term) == (2, 1, 0, 2)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch("particle", T, x1, ub, nthreads=4)
    assert (st["iterations"] == ref["stats"]["iterations"]).mean() >= 0.99
    same = st["iterations"] == ref["stats"]["iterations"]
    assert np.abs(x - ref["x"])[same].max() < 1e-8
    builtin = pkg.Solver(model="particle", horizon=T, batch=B, options=pkg.Options(verbose=0))
    builtin.initialize_rollout_(x1, ub); builtin.solve_()
    xb, ub_ = builtin.get_trajectory()
    assert np.abs(x - xb).max() < 1e-9
    sol.close(); builtin.close()


def test_synth32_whole_solve(pkg, oracle):
    """BASELINE configs[4]: synthetic nx=32, nu=8, T=101 with 16 stage inequalities (large-model path:
    HBM-resident workspace, 16x16x4 fp64 MFMA tiles in the Riccati step)."""
    B = 8
    model, T, x1, ub = pkg.workloads.make_inputs("synth32", B)
    ub = ub + 1.5 * np.sin(0.37 * np.arange(ub.size).reshape(ub.shape))     # start outside the action box
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    assert (sol.nx, sol.nu, sol.nc_stage, sol.nc_term) == (32, 8, 16, 0)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=8)
    rs = ref["stats"]
    same = (st["iterations"] == rs["iterations"]) & (st["outer_iterations"] == rs["outer_iterations"]) & (st["rollouts"] == rs["rollouts"])
    assert same.all(), (st["iterations"], rs["iterations"])
    dx_, du_, dK_ = np.abs(x - ref["x"]).max(), np.abs(u - ref["u"]).max(), np.abs(K - ref["K"]).max() / np.abs(ref["K"]).max()
    assert dx_ <= 1e-11 and du_ <= 1e-11 and dK_ <= 1e-11, (dx_, du_, dK_)
    assert (np.abs(u[same]) <= 1.0 + 5e-3).all()          # the action box holds at the solution
    sol.close()


def test_synth32_shard_of_4096(pkg, oracle):
    """BASELINE configs[4] at full per-GPU size: 4096 instances over 8 GPUs = a 512-instance shard
    (rank 5 here). Oracle comparison on every 8th instance, box feasibility on all of them."""
    B = 512
    lo, _ = pkg.distributed.shard_range(5, B)
    model, T, x1, ub = pkg.workloads.make_inputs("synth32", B, offset=lo)
    ub = ub + 1.5 * np.sin(0.37 * np.arange(ub[0].size).reshape(ub[0].shape))[None] * np.linspace(0.5, 1.5, B)[:, None, None]
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    assert np.isfinite(x).all() and (st["potrf_info"] == 0).all()
    assert (st["max_violation"] <= 5e-3).mean() > 0.99 and (np.abs(u) <= 1.0 + 5e-3)[st["max_violation"] <= 5e-3].all()
    idx = np.arange(0, B, 8)
    ref = oracle.solve_batch(model, T, x1[idx], ub[idx], nthreads=8)
    same = (st["iterations"][idx] == ref["stats"]["iterations"]) & (st["rollouts"][idx] == ref["stats"]["rollouts"])
    assert same.all(), same.mean()
    dx_ = np.abs(x[idx] - ref["x"]).max()
    assert dx_ <= 1e-11, dx_
    sol.close()


@pytest.mark.parametrize("config,B", [("particle", 4), ("car", 6), ("acrobot51", 6)])
def test_iteration_trace_matches_oracle(pkg, oracle, config, B):
    """The whole convergence history — what the reference prints per iteration when `verbose`
    (src/solve.jl:40-45): outer/inner index, cost, ‖∇L‖∞, max violation, step size — against the oracle."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    cap = 1100
    sol.enable_trace_(cap)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    tr = sol.trace(); st = sol.stats()
    pr = oracle.Problem(model, T)
    for b in range(B):
        s = oracle.Solver(pr); s.initialize_controls(ub[b]); s.initialize_states(pr.rollout(x1[b], ub[b]))
        s.enable_trace(cap); s.solve()
        ref = s.trace()
        if st["iterations"][b] != len(ref):
            continue        # control flow flipped at a rounding-level tie: covered by the whole-solve tests
        g = tr[b, :len(ref)]
        assert np.array_equal(g[:, 0], [r.outer for r in ref]) and np.array_equal(g[:, 1], [r.inner for r in ref])
        assert np.array_equal(g[:, 5], [r.step_size for r in ref]) and np.array_equal(g[:, 6], [r.status for r in ref])
        J = np.array([r.objective for r in ref]); gn = np.array([r.gradient_norm for r in ref]); mv = np.array([r.max_violation for r in ref])
        assert np.allclose(g[:, 2], J, rtol=1e-8, atol=1e-10)
        assert np.allclose(g[:, 3], gn, rtol=1e-5, atol=1e-9)
        assert np.allclose(g[:, 4], mv, rtol=1e-6, atol=1e-10)
    assert sum(st["iterations"][b] > 0 for b in range(B)) == B
    sol.close()


def test_long_horizon_above_64k_lds(pkg, oracle):
    """acrobot T = 301: a 107 KB LDS working set (above the 64 KiB default dynamic-LDS limit, below the
    160 KiB of a gfx950 CU) — one instance per CU."""
    B, T = 6, 301
    rng = np.random.default_rng(23)
    x1 = np.zeros((B, 4)); ub = 0.3 * rng.standard_normal((B, T - 1, 1))
    sol = pkg.Solver(model="acrobot", horizon=T, batch=B, options=pkg.Options(verbose=0, max_dual_updates=2, max_iterations=15))
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch("acrobot", T, x1, ub, options=oracle.default_options(max_dual_updates=2, max_iterations=15), nthreads=6)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.all(), same          # six instances, 300 steps: observed identical control flow on all of them
    assert np.abs(x - ref["x"])[same].max() < 1e-7 and np.abs(u - ref["u"])[same].max() < 1e-7
    sol.close()


@pytest.mark.parametrize("config,B", [("acrobot51", 96), ("car", 96), ("particle", 32), ("car_obs", 48)])
def test_throughput_kernel_variant(pkg, oracle, config, B):
    """The two-waves-per-SIMD kernel (Jacobians in HBM/L2, 20 KB of LDS per instance) against the oracle
    and against the latency kernel."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    w = pkg.workloads.make_parameters(config, B) if config == "car_obs" else None
    outs = []
    for variant in ("throughput", "latency"):
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.set_kernel_variant_(variant)
        if w is not None:
            sol.set_parameters_(w)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        outs.append(sol.get_trajectory() + sol.get_policy() + (sol.stats(),))
        sol.close()
    (x, u, K, k, st), (x2, u2, K2, k2, st2) = outs
    ref = oracle.solve_batch(model, T, x1, ub, w=w, nthreads=8)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    fin = same & np.isfinite(ref["x"]).reshape(B, -1).all(1)
    assert same.mean() >= 0.99
    assert np.abs(x - ref["x"])[fin].max() < 1e-7 and np.abs(u - ref["u"])[fin].max() < 1e-7
    agree = st["iterations"] == st2["iterations"]
    assert agree.mean() >= 0.99
    assert np.abs(x - x2)[agree & fin].max() < 1e-7


def test_throughput_variant_refused_for_large_models(pkg):
    sol = pkg.Solver(model="synth32", horizon=11, batch=2)
    with pytest.raises(pkg._ffi.IlqrError, match="small models"):
        sol.set_kernel_variant_("throughput")
    sol.close()


def test_host_stepped_al_loop_with_callback(pkg):
    """solve!(solver; augmented_lagrangian_callback! = cb) (src/solve.jl:88,125): the host-stepped outer loop
    with a no-op callback reproduces the fused single-launch solve, the callback is invoked once
    per dual update, and a callback that edits the parameters changes the result."""
    B = 24
    model, T, x1, ub = pkg.workloads.make_inputs("car_obs", B)
    w = pkg.workloads.make_parameters("car_obs", B)
    fused = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    fused.enable_trace_(128)
    fused.set_parameters_(w); fused.initialize_rollout_(x1, ub); fused.solve_()
    xf, uf = fused.get_trajectory(); sf = fused.stats()
    calls = []
    stepped = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    stepped.enable_trace_(128)
    stepped.set_parameters_(w); stepped.initialize_rollout_(x1, ub)
    stepped.solve_(augmented_lagrangian_callback_=lambda s: calls.append(1))
    xs, us = stepped.get_trajectory(); ss = stepped.stats()
    # the per-iteration record survives the launches of the stepped loop: as many rows as the fused solve wrote, same
    # (outer, inner, step size, status) columns
    tl_f, tl_s = fused.scalar("trace_len"), stepped.scalar("trace_len")
    assert (tl_f == sf["iterations"]).all() and (tl_s == ss["iterations"]).all()
    tf, ts = fused.trace(), stepped.trace()
    for b in range(B):
        if sf["iterations"][b] == ss["iterations"][b]:
            k = int(tl_f[b])
            assert np.array_equal(tf[b, :k][:, [0, 1, 5, 6]], ts[b, :k][:, [0, 1, 5, 6]]), b
    # the stepped loop runs the same device functions from another kernel: same results up to the
    # compiler's FMA-contraction choices in the two inlining contexts
    same = (sf["iterations"] == ss["iterations"]) & (sf["rollouts"] == ss["rollouts"])
    assert same.mean() >= 0.99 and (sf["outer_iterations"] == ss["outer_iterations"])[same].all()
    assert np.abs(xf - xs)[same].max() < 1e-7 and np.abs(uf - us)[same].max() < 1e-7
    assert len(calls) == ss["outer_iterations"].max() - 1        # no callback after the final (converged) pass
    moved = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    moved.set_parameters_(w); moved.initialize_rollout_(x1, ub)

    def shift_obstacle(s):                                        # continuation on the model parameters
        s.set_parameters_(s.buffer("parameters").reshape(B, T, 2) + 0.03)
    moved.solve_(augmented_lagrangian_callback_=shift_obstacle)
    xm, _ = moved.get_trajectory()
    assert np.abs(xm - xf).max() > 1e-6
    for s in (fused, stepped, moved):
        s.close()


def test_plain_c_caller_of_the_abi(pkg, tmp_path):
    """examples/acrobot_batch.c: the C-ABI used from plain C (no Python, no torch types)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "acrobot_batch")
    libdir = os.path.join(root, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "acrobot_batch.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run([exe, "192"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reached the goal" in out.stdout


def test_time_varying_stage_objects(pkg, oracle):
    """Vectors of DISTINCT per-step objects (README.md:26 of the reference): two dynamics, two stage costs and three
    stage constraints (5 inequalities / none / 1 equality) alternating along the horizon, lowered exactly onto
    the one-template kernel by selectors in θ_t (lowering.py). The oracle evaluates the genuinely per-step objects
    (oracle/models.cpp "car_tv")."""
    T, B = 51, 48
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    dynamics, costs, constraints = pkg.models.car_tv(T)
    sol = pkg.Solver(dynamics, costs, constraints, batch=B, options=pkg.Options(verbose=0), name="car_tv")
    assert (sol.nx, sol.nu, sol.nc_stage, sol.nc_term, sol.num_user_parameter) == (3, 2, 6, 4, 0)
    sol.initialize_rollout_(x1, ub)
    ref = oracle.solve_batch("car_tv", T, x1, ub, nthreads=4)
    xb0 = np.stack([oracle.Problem("car_tv", T).rollout(x1[b], ub[b]) for b in range(4)])
    assert np.abs(sol.buffer("nominal_states").reshape(B, T, 3)[:4] - xb0).max() < 1e-12     # time-varying dynamics
    sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.99, same.mean()
    assert np.abs(x - ref["x"])[same].max() < 1e-7 and np.abs(u - ref["u"])[same].max() < 1e-7
    assert np.abs(K - ref["K"])[same].max() <= 5e-7 * np.abs(ref["K"]).max()
    assert np.allclose(st["objective"][same], ref["stats"]["objective"][same], rtol=1e-8)
    assert np.allclose(st["max_violation"][same], ref["stats"]["max_violation"][same], atol=1e-8)
    # rows of the switched-off constraint kinds: zero violation, zero multiplier
    c = sol.buffer("violations").reshape(B, -1)[:, :(T - 1) * 6].reshape(B, T - 1, 6)
    lam = sol.buffer("constraint_dual").reshape(B, -1)[:, :(T - 1) * 6].reshape(B, T - 1, 6)
    for t in range(T - 1):
        off = [i for i in range(6) if i not in sol.constraint_rows[t]]
        assert (c[:, t, off] == 0).all() and (lam[:, t, off] == 0).all()
    sol.close()


def test_time_varying_stage_objects_from_c_sources_per_kind(pkg, oracle):
    """car_tv (two dynamics, two stage costs, three stage constraints: 5 inequalities / none / 1 equality) the way a Julia or C host
    hands it over: C callables per kind (here printed from the symbolic objects, as the Julia wrapper prints Symbolics' C target),
    lowered by the LIBRARY — selector branches for all three categories, constraint kinds stacked row-wise with shifted inequality
    masks (ilqr_compile_model_stages). Against the oracle's genuinely per-step problem, and close to the symbolic route's result."""
    T, B = 51, 48
    _, _, x1, ub = pkg.workloads.make_inputs("car", B)
    dynamics, costs, constraints = pkg.models.car_tv(T)
    sol = pkg.Solver(stage_sources=pkg.lowering.c_stage_sources(dynamics, costs, constraints), batch=B, options=pkg.Options(verbose=0),
                     name="car_tv_c")
    assert (sol.nx, sol.nu, sol.nc_stage, sol.nc_term, sol.num_user_parameter, sol.nw) == (3, 2, 6, 4, 0, 0)
    assert sol.constraint_rows[0] == [0, 1, 2, 3, 4] and sol.constraint_rows[1] == [] and sol.constraint_rows[2] == [5]
    sol.initialize_rollout_(x1, ub)
    xb0 = np.stack([oracle.Problem("car_tv", T).rollout(x1[b], ub[b]) for b in range(4)])
    assert np.abs(sol.buffer("nominal_states").reshape(B, T, 3)[:4] - xb0).max() < 1e-12
    sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    ref = oracle.solve_batch("car_tv", T, x1, ub, nthreads=4)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.97, same.mean()
    assert np.abs(x - ref["x"])[same].max() < 1e-7 and np.abs(u - ref["u"])[same].max() < 1e-7
    assert np.abs(K - ref["K"])[same].max() <= 5e-7 * np.abs(ref["K"]).max()
    assert np.allclose(st["max_violation"][same], ref["stats"]["max_violation"][same], atol=1e-8)
    c = sol.buffer("violations").reshape(B, -1)[:, :(T - 1) * 6].reshape(B, T - 1, 6)
    lam = sol.buffer("constraint_dual").reshape(B, -1)[:, :(T - 1) * 6].reshape(B, T - 1, 6)
    for t in range(T - 1):
        off = [i for i in range(6) if i not in sol.constraint_rows[t]]
        assert (c[:, t, off] == 0).all() and (lam[:, t, off] == 0).all()
    sol.close()


def test_large_path_odd_dimensions_and_terminal_constraint(pkg, oracle):
    """synth12: nx = 12, nu = 5 (not multiples of the 16x16 MFMA tile or of the k-step: the zero-padded
    tile paths), state-dependent fu entries (bilinear term), a terminal equality (al_t on the large path) and
    a binding action box. User-defined model through the plugin path; oracle twin in oracle/models.cpp."""
    T, B = 41, 64
    mdl = pkg.models.synth12()
    rng = np.random.default_rng(12)
    x1 = 0.5 * rng.standard_normal((B, 12)); ub = 0.1 * rng.standard_normal((B, T - 1, 5))
    kw = dict(max_iterations=15, max_dual_updates=3)      # the problem is hard for the reference's AL loop; parity, not convergence
    sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                     [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0, **kw),
                     name="synth12")
    assert (sol.nx, sol.nu, sol.nc_stage, sol.nc_term) == (12, 5, 10, 3)
    sol.initialize_rollout_(x1, ub)
    xb0 = np.stack([oracle.Problem("synth12", T).rollout(x1[b], ub[b]) for b in range(4)])
    assert np.abs(sol.buffer("nominal_states").reshape(B, T, 12)[:4] - xb0).max() < 1e-12
    # one linearisation + Riccati pass from identical inputs, stage level
    refs = []
    for b in range(4):
        pr, s, _ = _oracle_solver(oracle, "synth12", T, x1[b], ub[b])
        s.call("cost_bang", 0); s.call("gradients"); s.call("backward_pass")
        refs.append((pr, s))
    sol.run_stage_("cost_nominal"); sol.run_stage_("gradients"); sol.run_stage_("backward_pass")
    for name in ("jacobian_state", "jacobian_action", "hessian_state_state", "hessian_action_action", "K", "k", "P", "p"):
        got = sol.buffer(name)[:4]
        want = np.stack([r[1].buffer(name) for r in refs])
        assert _rel(got, want) < 1e-9, name
    # whole solve
    sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    ref = oracle.solve_batch("synth12", T, x1, ub, options=oracle.default_options(**kw), nthreads=4)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.99, same.mean()
    assert np.abs(x - ref["x"])[same].max() < 1e-7 and np.abs(u - ref["u"])[same].max() < 1e-7
    assert np.abs(K - ref["K"])[same].max() <= 5e-7 * np.abs(ref["K"]).max()
    assert np.allclose(st["max_violation"][same], ref["stats"]["max_violation"][same], atol=1e-7)
    sol.close()


def test_synth12_workload_builtin_equals_plugin_and_oracle(pkg, oracle):
    """The mid-size workload of bench.py (`--config synth12`: nx = 12, nu = 5, T = 101, iteration caps of CONFIG_OPTIONS): the
    builtin model (csrc/models/model_synth12.h, generated at build time) against the same functions passed as a user-defined model
    at run time (bitwise: same generator, same kernels), both kernel variants, and against the oracle's twin."""
    B = 48
    model, T, x1, ub = pkg.workloads.make_inputs("synth12", B)
    kw = pkg.workloads.CONFIG_OPTIONS["synth12"]
    assert (model, T) == ("synth12", 101)
    res = {}
    for variant in ("latency", "mid"):
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, **kw))
        sol.set_kernel_variant_(variant)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        res[variant] = dict(x=sol.get_trajectory()[0], u=sol.get_trajectory()[1], K=sol.get_policy()[0], st=sol.stats())
        sol.close()
    mdl = pkg.models.synth12()
    sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                     [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0, **kw), name="synth12_rt")
    sol.set_kernel_variant_("latency")
    sol.initialize_rollout_(x1, ub); sol.solve_()
    res["plugin"] = dict(x=sol.get_trajectory()[0], u=sol.get_trajectory()[1], K=sol.get_policy()[0], st=sol.stats())
    sol.close()
    for other in ("mid", "plugin"):
        for k in ("x", "u", "K"):
            assert np.array_equal(res["latency"][k], res[other][k], equal_nan=True), (other, k)
        for k in ("iterations", "outer_iterations", "rollouts", "status", "objective"):
            assert np.array_equal(res["latency"]["st"][k], res[other]["st"][k], equal_nan=True), (other, k)
    ref = oracle.solve_batch(model, T, x1, ub, options=oracle.default_options(**kw), nthreads=8)
    st = res["mid"]["st"]
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.999, same.mean()
    assert np.abs(res["mid"]["x"] - ref["x"])[same].max() < 2e-8 and np.abs(res["mid"]["u"] - ref["u"])[same].max() < 2e-8


def _ragged_inputs(pr, B, seed=5):
    rng = np.random.default_rng(seed)
    T = pr.T
    x1 = np.zeros((B, pr.nx)); x1[:, :pr.state_dims[0]] = 0.5 * rng.standard_normal((B, pr.state_dims[0]))
    ub = np.zeros((B, T - 1, pr.nu))
    for t in range(T - 1):
        ub[:, t, :pr.action_dims[t]] = 0.2 * rng.standard_normal((B, pr.action_dims[t]))
    return x1, ub


def _check_ragged_against_the_oracle(pkg, oracle, sol, T, B):
    """Stage buffers of one linearisation + Riccati pass and the whole solve of the zero-padded template against the ORACLE's
    genuinely ragged problem (per-timestep blocks sized as src/data/{model,objective,policy}.jl size them)."""
    pr = oracle.Problem("ragged", T)
    n, m = sol.nx, sol.nu
    assert (n, m, sol.state_dims, sol.action_dims) == (4, 2, pr.state_dims, pr.action_dims)
    x1, ub = _ragged_inputs(pr, B)
    sol.initialize_rollout_(x1, ub)
    xb = sol.buffer("nominal_states").reshape(B, T, n)
    for b in range(3):
        assert np.abs(xb[b] - pr.rollout(x1[b], ub[b])).max() < 1e-13                # padding included: exactly zero in both
    # -- stages on identical inputs, twice (the second linearisation adds to the accumulated Hessians, Q1)
    refs = []
    for b in range(3):
        o = oracle.Solver(pr); o.initialize_controls(ub[b]); o.initialize_states(pr.rollout(x1[b], ub[b]))
        refs.append(o)
    for rep in range(2):
        sol.run_stage_("cost_nominal"); sol.run_stage_("gradients"); sol.run_stage_("backward_pass")
        for o in refs:
            o.call("cost_bang", 0); o.call("gradients"); o.call("backward_pass")
        shapes = {"jacobian_state": (T - 1, n, n), "jacobian_action": (T - 1, m, n), "gradient_state": (T, n), "gradient_action": (T - 1, m),
                  "hessian_state_state": (T, n, n), "hessian_action_action": (T - 1, m, m), "hessian_action_state": (T - 1, n, m),
                  "K": (T - 1, n, m), "k": (T - 1, m), "P": (T, n, n), "p": (T, n)}
        for name, shp in shapes.items():
            got = sol.buffer(name)[:3].reshape((3,) + shp)
            want = np.stack([o.padded(name) for o in refs])
            if name == "hessian_action_action":            # the template's padded actions carry u^2 / 2: 1 (x linearisations so far) on their diagonal
                for t in range(T - 1):
                    for j in range(pr.action_dims[t], m):
                        want[:, t, j, j] = rep + 1.0
            tol = 1e-12 if name.startswith(("jacobian", "gradient", "hessian")) else 1e-9
            assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), (name, rep)
            if name in ("K", "k", "P", "p", "jacobian_state", "jacobian_action"):
                assert (got[want == 0] == 0).all(), name                                 # the padding is EXACTLY zero
        sol.run_stage_("forward_pass")
        for o in refs:
            o.call("forward_pass")
        st = sol.stats()
        assert [st["step_size"][b] for b in range(3)] == [o.stats().step_size for o in refs]
    # -- whole solve
    sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    ref = oracle.solve_batch("ragged", T, x1, ub, nthreads=4)
    for f in ("iterations", "outer_iterations", "rollouts", "status"):
        assert (st[f] == ref["stats"][f]).all(), f                                      # control flow exact on every instance
    assert (st["step_size"] == ref["stats"]["step_size"]).all()
    assert np.abs(x - ref["x"]).max() <= 1e-7 and np.abs(u - ref["u"]).max() <= 1e-7
    assert np.abs(K - ref["K"]).max() <= 1e-7 * np.abs(ref["K"]).max() and np.abs(k - ref["k"]).max() <= 1e-7
    assert np.allclose(st["objective"], ref["stats"]["objective"], rtol=1e-9) and np.allclose(st["max_violation"], ref["stats"]["max_violation"], atol=1e-9)
    for t in range(T):
        assert (x[:, t, pr.state_dims[t]:] == 0).all()                                  # padding exactly zero
    for t in range(T - 1):
        n0, m0 = pr.state_dims[t], pr.action_dims[t]
        assert (u[:, t, m0:] == 0).all() and (k[:, t, m0:] == 0).all()
        assert (K[:, t, :, m0:] == 0).all() and (K[:, t, n0:, :] == 0).all()             # K[b][t] is [nx][nu]
    assert (st["max_violation"] <= 5e-3).all()
    return np.abs(x - ref["x"]).max(), np.abs(u - ref["u"]).max()


@pytest.mark.parametrize("T", [9, 41])
def test_time_varying_dimensions(pkg, oracle, T):
    """num_next_state != num_state along the horizon (src/dynamics.jl:5-7), lowered by zero padding (lowering.py, plan from
    ilqr_plan_stages) — against the oracle, which holds the genuinely ragged per-timestep buffers of the reference."""
    from test_codegen import _ragged_problem
    B = 24
    dynamics, costs, constraints, n_t, m_t = _ragged_problem(pkg, T)
    sol = pkg.Solver(dynamics, costs, constraints, batch=B, options=pkg.Options(verbose=0), name="ragged")
    _check_ragged_against_the_oracle(pkg, oracle, sol, T, B)
    sol.close()


def test_time_varying_dimensions_from_c_sources_per_kind(pkg, oracle):
    """The same problem the way a Julia or C host hands it over: C callables per kind, each in its own dimensions, lowered by the
    LIBRARY (ilqr_compile_model_stages + ilqr_set_stage_selectors) — no Python lowering, no symbolic generator."""
    T, B = 41, 24
    sol = pkg.Solver(stage_sources=pkg.models.ragged_c_stages(T), batch=B, options=pkg.Options(verbose=0), name="ragged_c")
    assert sol.num_user_parameter == 0 and sol.nw == 0             # ilqr_get_dims reports the USER's parameters: none
    with pytest.raises(pkg._ffi.IlqrError, match="no parameters"):
        sol.set_parameters_(np.zeros((B, T, 0)))
    _check_ragged_against_the_oracle(pkg, oracle, sol, T, B)
    # the selector columns are in the device's parameter block, behind nothing (no user parameters)
    w = sol.buffer("parameters").reshape(B, T, -1)
    assert w.shape[2] == sol._selectors.shape[1] and (w == sol._selectors[None]).all()
    sol.close()


def test_verbose_prints_the_reference_report(pkg, oracle, capsys):
    """options.verbose: the per-iteration report of src/solve.jl:39-44 (for instance 0), fed by the device trace."""
    model, T, x1, ub = pkg.workloads.make_inputs("particle", 4)
    sol = pkg.Solver(model=model, horizon=T, batch=4, options=pkg.Options(verbose=1))
    sol.initialize_rollout_(x1, ub); sol.solve_()
    out = capsys.readouterr().out
    pr, s, _ = _oracle_solver(oracle, model, T, x1[0], ub[0]); s.solve()
    assert out.count("iter:") == s.stats().iterations
    assert "gradient_norm:" in out and "max_violation:" in out and "step_size:" in out
    first_cost = float(out.split("cost:")[1].split()[0])
    s2 = oracle.Solver(pr, oracle.default_options()); s2.enable_trace(); s2.initialize_controls(ub[0])
    s2.initialize_states(pr.rollout(x1[0], ub[0])); s2.solve()
    assert abs(first_cost - s2.trace()[0].objective) <= 1e-9 * max(1.0, abs(first_cost))
    sol.close()


# ------------------------------------------------------------------ packed kernel (four instances per wave, no LDS)
@pytest.mark.parametrize("config,B", [("car", 7), ("acrobot51", 6), ("particle", 9), ("car_goal", 13)])
def test_packed_kernel_ragged_batches(pkg, oracle, config, B):
    """Batches that do not fill the last wave (B % 4 != 0) on the packed kernel, against the oracle."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.set_kernel_variant_("packed")
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=4)
    rs = ref["stats"]
    assert (st["iterations"] == rs["iterations"]).all() and (st["rollouts"] == rs["rollouts"]).all()
    assert (st["outer_iterations"] == rs["outer_iterations"]).all() and (st["status"] == rs["status"]).all()
    assert np.abs(x - ref["x"]).max() < 1e-7 and np.abs(u - ref["u"]).max() < 1e-7
    assert np.abs(K - ref["K"]).max() <= 5e-7 * max(1.0, np.abs(ref["K"]).max())
    assert np.allclose(st["objective"], rs["objective"], rtol=1e-8)
    sol.close()


@pytest.mark.parametrize("config,B", [("particle", 9), ("car", 37), ("acrobot51", 45), ("car_obs", 21), ("car_goal", 130)])
def test_packed_kernel_with_a_linearisation_server_equals_the_one_wave_form(pkg, oracle, config, B):
    """Two waves per pack: wave 1 linearises chunk ch - 1 into a second LDS buffer while wave 0 takes the Riccati steps of chunk ch
    (`packed2`; what `packed` / `auto` pick where the buffers fit the CU). Same functions on the same inputs in the same order per
    instance: trajectories, policies, duals, the workspace's last linearisation and every statistic BITWISE those of the one-wave
    form (`packed1`), with and without the straggler hand-over; against the oracle like any kernel."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    w = pkg.workloads.make_parameters(config, B) if config == "car_obs" else None
    out = {}
    for v, ho in (("packed1", 0), ("packed2", 0), ("packed2", -1)):
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.set_kernel_variant_(v); sol.set_handover_(ho)
        if w is not None:
            sol.set_parameters_(w)
        sol.enable_trace_(1100)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        st = sol.stats()
        out[(v, ho)] = dict(x=sol.get_trajectory()[0], u=sol.get_trajectory()[1], K=sol.get_policy()[0], k=sol.get_policy()[1],
                            lam=sol.buffer("constraint_dual"), fx=sol.buffer("jacobian_state"), gxx=sol.buffer("hessian_state_state"),
                            it=st["iterations"], ro=st["rollouts"], oi=st["outer_iterations"], viol=st["max_violation"], obj=st["objective"],
                            tr=sol.trace())
        sol.close()
    a = out[("packed1", 0)]
    for key in (("packed2", 0), ("packed2", -1)):
        b = out[key]
        for f in a:
            # every field BITWISE, the objective of every trace row included: all kernel families form J in one arithmetic
            # (ilqr_device.hpp: objective_term, ObjAcc; the generated cost / constraint functions are compiled without FMA contraction)
            assert np.array_equal(a[f], b[f], equal_nan=True), (key, f)
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=8, w=w)
    same = (a["it"] == ref["stats"]["iterations"]) & (a["ro"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.99 and np.abs(out[("packed2", 0)]["x"] - ref["x"])[same].max() < 1e-7


def test_packed_kernel_leaves_the_last_linearisation(pkg):
    """The packed kernel keeps fx, fu, gx, gu on chip while it iterates; when an instance leaves its inner loop they are
    written out, so the workspace reads like after the LDS-resident kernels (solver.problem.model.jacobian_state ...)."""
    B = 8
    model, T, x1, ub = pkg.workloads.make_inputs("car", B)
    out = {}
    for v in ("latency", "packed"):
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.set_kernel_variant_(v); sol.initialize_rollout_(x1, ub); sol.solve_()
        out[v] = {name: sol.buffer(name) for name in ("jacobian_state", "jacobian_action", "gradient_state", "gradient_action",
                                                     "hessian_state_state", "hessian_action_action", "hessian_action_state",
                                                     "K", "k", "gradient_state_lagrangian", "gradient_action_lagrangian",
                                                     "constraint_dual", "constraint_penalty", "violations", "active_set")}
        sol.close()
    for name, a in out["latency"].items():
        b = out["packed"][name]
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(a).max()), name


def test_long_horizon_runs_on_the_packed_kernel(pkg, oracle):
    """The reference has no horizon limit (src/data/problem.jl:25-46). acrobot T = 601 needs 236 KB per instance in the
    LDS-resident kernels (> 160 KiB of a CU): the solve goes to the streaming packed kernel, the LDS variants refuse."""
    B, T = 8, 601
    rng = np.random.default_rng(11)
    x1 = np.zeros((B, 4)); ub = 0.5 * rng.standard_normal((B, T - 1, 1))
    sol = pkg.Solver(model="acrobot", horizon=T, batch=B, options=pkg.Options(verbose=0))
    with pytest.raises(pkg._ffi.IlqrError, match="packed"):
        sol.set_kernel_variant_("latency")
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch("acrobot", T, x1, ub, nthreads=8)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.75, (st["iterations"], ref["stats"]["iterations"])     # 600 steps amplify rounding: a decision may flip
    assert np.abs(x - ref["x"])[same].max() < 1e-6 and np.abs(u - ref["u"])[same].max() < 1e-6
    assert (np.abs(x[:, -1, :] - [np.pi, 0, 0, 0]).max(1) < 5e-3)[st["max_violation"] <= 5e-3].all()
    sol.close()


def test_auto_variant_takes_the_packed_kernel_beyond_one_instance_per_simd(pkg):
    B = 1536
    model, T, x1, ub = pkg.workloads.make_inputs("car", B)
    res = []
    for v in ("auto", "packed"):
        sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.set_kernel_variant_(v); sol.initialize_rollout_(x1, ub); sol.solve_()
        res.append(sol.get_trajectory()[0]); sol.close()
    assert np.array_equal(res[0], res[1])


def test_c_host_defines_a_model_and_runs_two_handles_concurrently(pkg, tmp_path):
    """examples/particle_compile.c: ilqr_compile_model from plain C (the reference's callables as C source -> hipcc child
    process -> registered model), then the user model and the built-in twin on two handles from two host threads."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "particle_compile")
    libdir = os.path.join(root, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "particle_compile.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "user-defined model matches the built-in one" in out.stdout


@pytest.mark.parametrize("nm", [(3, 3), (4, 4), (2, 3)])
def test_packed_kernel_with_three_and_four_actions(pkg, nm):
    """nu = 3, 4 on the packed kernel (K and k take separate triangular solves, no spare rows in the 4x4 block), and
    nu > nx; user-defined models through the symbolic generator, compared with the latency kernel."""
    import sympy as sp
    n, m = nm
    h = 0.1
    A = [[(-0.5 if i == j else 0.0) + 0.2 * np.cos(1.0 + i + 2 * j) for j in range(n)] for i in range(n)]
    Bm = [[np.sin(1.0 + 3 * i + j) for j in range(m)] for i in range(n)]
    f = lambda x, u: [x[i] + h * (sum(A[i][j] * x[j] for j in range(n)) + sum(Bm[i][j] * u[j] for j in range(m)) + 0.3 * sp.sin(x[i]))
                      for i in range(n)]
    dyn = pkg.Dynamics(f, n, m)
    stage = pkg.Cost(lambda x, u: 0.5 * sum(xi * xi for xi in x) + 0.05 * sum((1 + j) * u[j] * u[j] for j in range(m)) + 0.01 * u[0] * u[m - 1], n, m)
    term = pkg.Cost(lambda x, u: 5.0 * sum(xi * xi for xi in x), n, 0)
    box = pkg.Constraint(lambda x, u: [u[0] - 0.8, -0.8 - u[0]], n, m, indices_inequality=[1, 2])
    goal = pkg.Constraint(lambda x, u: [x[0] - 0.3], n, 0)
    T, B = 31, 10
    rng = np.random.default_rng(23)
    x1 = rng.standard_normal((B, n)); ub = 0.3 * rng.standard_normal((B, T - 1, m))
    res = {}
    for v in ("latency", "packed"):
        sol = pkg.Solver([dyn] * (T - 1), [stage] * (T - 1) + [term], [box] * (T - 1) + [goal], batch=B,
                         options=pkg.Options(verbose=0), name="pk%d%d" % (n, m))
        sol.set_kernel_variant_(v)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        res[v] = (sol.get_trajectory(), sol.get_policy(), sol.stats())
        sol.close()
    a, b = res["latency"], res["packed"]
    assert (a[2]["iterations"] == b[2]["iterations"]).all() and (a[2]["rollouts"] == b[2]["rollouts"]).all()
    assert a[2]["iterations"].min() >= 2 and (b[2]["max_violation"] <= 5e-3).all()
    assert np.abs(a[0][0] - b[0][0]).max() < 1e-9 and np.abs(a[0][1] - b[0][1]).max() < 1e-9
    assert np.abs(a[1][0] - b[1][0]).max() <= 1e-8 * max(1.0, np.abs(a[1][0]).max())


# ------------------------------------------------------------------ shared step size (optional mode, not a reference behaviour)
@pytest.mark.parametrize("config", ["particle", "car", "acrobot51"])
def test_shared_step_with_a_batch_of_one_is_the_reference_solve(pkg, config):
    """solve_shared_step_ decides the Armijo test on the summed merit; with one instance the sum is that instance's merit,
    so the host-stepped loop must reproduce the fused single-launch solve! (iterations, step sizes, trajectories)."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, 3)
    for b in range(3):
        fused = pkg.Solver(model=model, horizon=T, batch=1, options=pkg.Options(verbose=0))
        fused.set_kernel_variant_("latency"); fused.enable_trace_(600)
        fused.initialize_rollout_(x1[b:b + 1], ub[b:b + 1]); fused.solve_()
        ss = pkg.Solver(model=model, horizon=T, batch=1, options=pkg.Options(verbose=0))
        ss.initialize_rollout_(x1[b:b + 1], ub[b:b + 1])
        steps = ss.solve_shared_step_()
        tr = fused.trace()[0][:int(fused.scalar("trace_len")[0])]
        assert len(steps) == tr.shape[0] and np.array_equal(np.array(steps), np.where(tr[:, 6] != 0, tr[:, 5], 0.0)), (config, b)
        sf, s1 = fused.stats(), ss.stats()
        for f in ("iterations", "outer_iterations", "rollouts", "status"):
            assert sf[f][0] == s1[f][0], (config, b, f)
        assert np.abs(fused.get_trajectory()[0] - ss.get_trajectory()[0]).max() < 1e-11
        assert np.abs(fused.get_policy()[0] - ss.get_policy()[0]).max() <= 1e-10 * max(1.0, np.abs(fused.get_policy()[0]).max())
        fused.close(); ss.close()


def test_shared_step_over_two_ranks_matches_one_rank(pkg, tmp_path):
    """The data-path collective: two ranks (gloo, both on device 0 — one GPU in the test box; RCCL takes the same call with
    one GPU per rank) solve halves of a car batch with ONE step size per iteration for all 8 instances. The accepted steps
    must be those of a single process solving the 8 instances, on both ranks, and every instance must end feasible."""
    B = 8
    model, T, x1, ub = pkg.workloads.make_inputs("car", B)
    one = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    one.initialize_rollout_(x1, ub)
    steps = np.array(one.solve_shared_step_())
    x_one = one.get_trajectory()[0]; st = one.stats()
    assert (st["max_violation"] <= 5e-3).all() and np.isfinite(x_one).all() and steps.size > 20
    one.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "ss")
    rc, _ = pkg.distributed.launch_ranks(os.path.join(root, "tests", "ss_worker.py"), [out, str(B)], 2, share_device=True, timeout=600)
    assert rc == 0
    parts = [np.load(out + ".%d.npz" % r) for r in range(2)]
    assert np.array_equal(parts[0]["steps"], parts[1]["steps"])                      # one step size for everybody
    assert np.array_equal(parts[0]["steps"], steps)                                  # ... the same as on one rank
    x_two = np.concatenate([parts[0]["x"], parts[1]["x"]])
    assert np.abs(x_two - x_one).max() < 1e-9
    assert (np.concatenate([p["max_violation"] for p in parts]) <= 5e-3).all()


def test_lazy_reset_of_large_models_is_unobservable(pkg):
    """ilqr_reset of an HBM-resident model defers zeroing the megabyte-sized Jacobian / Hessian / value arrays to the solve
    kernel; a getter, setter or stage call that could see stale values first must trigger it."""
    B, T = 3, 11
    model, _, x1, ub = pkg.workloads.make_inputs("synth32", B)
    ub = ub[:, :T - 1] + 0.3
    sol = pkg.Solver(model="synth32", horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub); sol.solve_()
    first = sol.get_trajectory()[0].copy()
    assert np.abs(sol.buffer("jacobian_state")).max() > 0 and np.abs(sol.buffer("hessian_state_state")).max() > 0
    sol.run_stage_("backward_pass")                                   # writes P, p
    assert np.abs(sol.buffer("P")).max() > 0
    sol.reset_()
    for name in ("jacobian_state", "jacobian_action", "hessian_state_state", "hessian_action_action", "hessian_action_state", "P", "p",
                 "K", "nominal_states", "constraint_dual"):
        assert not sol.buffer(name).any(), name                       # a fresh solver: all zero (src/data/*.jl)
    assert (sol.stats()["objective"] == np.inf).all()
    sol.reset_(); sol.initialize_rollout_(x1, ub)
    sol.run_stage_("cost_nominal"); sol.run_stage_("gradients")        # the accumulating stage on a fresh solver must start from zero Hessians
    h1 = sol.buffer("hessian_state_state").copy()
    sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()        # and the solve after a reset reproduces the first one
    assert np.array_equal(sol.get_trajectory()[0], first)
    assert not sol.buffer("P").any()                                  # the fused solve does not store P: still the fresh zeros
    sol.reset_(); sol.initialize_rollout_(x1, ub)
    sol.run_stage_("cost_nominal"); sol.run_stage_("gradients")
    assert np.array_equal(sol.buffer("hessian_state_state"), h1)
    sol.close()


def test_packed_kernel_edge_shapes(pkg):
    """Minimal horizons (one and two dynamics steps), horizons around the 16-step chunk of the fused linearise + Riccati
    sweep, batches that leave one to three rows of a wave empty: packed against latency kernel."""
    rng = np.random.default_rng(3)
    for model, n, m in (("particle", 2, 1), ("car", 3, 2)):
        for T in (2, 3, 16, 17, 18, 33, 34):
            for B in (1, 3, 5):
                x1 = 0.1 * rng.standard_normal((B, n)); ub = 0.05 * rng.standard_normal((B, T - 1, m))
                res = []
                for v in ("latency", "packed"):
                    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
                    sol.set_kernel_variant_(v); sol.initialize_rollout_(x1, ub); sol.solve_()
                    res.append((sol.get_trajectory()[0], sol.get_policy()[0], sol.stats())); sol.close()
                a, b = res
                assert (a[2]["iterations"] == b[2]["iterations"]).all() and (a[2]["rollouts"] == b[2]["rollouts"]).all(), (model, T, B)
                assert np.isfinite(b[0]).all() and np.abs(a[0] - b[0]).max() < 1e-9, (model, T, B)
                assert np.abs(a[1] - b[1]).max() <= 1e-8 * max(1.0, np.abs(a[1]).max()), (model, T, B)


@pytest.mark.parametrize("model,variant", [("acrobot", "latency"), ("car", "latency"), ("car", "throughput"), ("acrobot", "packed"),
                                           ("car", "packed"), ("particle", "latency")])
def test_fused_backward_pass_equals_staged_for_even_and_odd_horizons(pkg, model, variant):
    """The Riccati recursion of the FUSED solve kernel (its own template instantiation: no value-function stores) against the
    stage kernels, for horizons whose last pair / odd tail / single step enter a step through every branch of the unrolled
    loop. (An f64 MFMA that reads P one branch after the MFMA that wrote it got no wait states from hipcc: the first step of
    even horizons was wrong for nu = 3 until the rare paths carried their own, ilqr_device.hpp mfma_block_boundary_guard.)"""
    n, m = {"acrobot": (4, 1), "car": (3, 2), "particle": (2, 1)}[model]
    B = 5
    for T in (2, 3, 4, 5, 6, 7, 9, 10, 13, 14):
        rng = np.random.default_rng(100 + T)
        x1 = 0.1 * rng.standard_normal((B, n)); ub = 0.3 * rng.standard_normal((B, T - 1, m))
        out = {}
        for mode in ("fused", "staged"):
            sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, max_iterations=0, max_dual_updates=1))
            sol.set_kernel_variant_(variant)
            sol.initialize_rollout_(x1, ub)
            if mode == "fused":
                sol.solve_()
            else:
                for st in ("al_begin", "cost_nominal", "gradients", "backward_pass"):
                    sol.run_stage_(st)
            out[mode] = [sol.buffer(nm) for nm in ("K", "k", "gradient_state_lagrangian", "gradient_action_lagrangian")] + [sol.stats()["gradient_norm"]]
            sol.close()
        for a, b in zip(out["fused"], out["staged"]):
            assert np.array_equal(a, b), (model, variant, T, np.abs(a - b).max())


@pytest.mark.parametrize("nm", [(40, 6), (48, 16), (64, 8)])
def test_large_path_beyond_32_states_against_the_independent_restatement(pkg, nm):
    """nx = 40, nu = 6 and nx = 48, nu = 16 (the limits; three 16x16 MFMA tiles per side, the generic tile loops of ilqr_device_large.hpp; the reference sizes
    everything dynamically, src/data/policy.jl:44-78). No oracle twin exists for this size: the check is the second,
    independent restatement (numpy + sympy + scipy LAPACK, tests/golden/reference_restatement.py) run live."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    (n, m), T, B = nm, 21, 3
    rng = np.random.default_rng(40)
    x1 = 0.5 * rng.standard_normal((B, n)); ub = 0.4 * rng.standard_normal((B, T - 1, m))
    mdl = pkg.models.synth_nm(n, m)
    sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                     [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0), name="synth%d" % n)
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 2 * m)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    dyn, costs, cons = R.synth32_problem(T, n, m)
    for b in range(B):
        s = R.Solver(dyn, costs, cons)
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dyn, x1[b], ub[b]))
        s.solve()
        assert st["iterations"][b] == s.iterations and st["outer_iterations"][b] == s.outer_iterations, (b, st["iterations"][b], s.iterations)
        assert st["iterations"][b] >= 2
        assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 1e-8
        Kr = np.stack([Kt.T for Kt in s.K])                    # [t][n][m]: column-major m x n blocks
        assert np.abs(K[b] - Kr).max() <= 1e-7 * max(1.0, np.abs(Kr).max())
        assert abs(st["objective"][b] - s.objective) <= 1e-9 * max(1.0, abs(s.objective))
    sol.close()


@pytest.mark.parametrize("nm", [(1, 1), (2, 4), (4, 3), (3, 4), (5, 1), (9, 3), (16, 16), (17, 2)])
def test_dimension_sweep_against_the_independent_restatement(pkg, nm):
    """The reference sizes every buffer at run time (src/data/policy.jl:44-78, src/data/problem.jl:25-46); here the dimensions pick
    the kernel family and the tile shapes. The synth family at the corners between the families — nx = 1; nu > nx on the small path
    (latency, throughput and packed kernels); nx = 5 (first size of the large path), 9 x 3 and 16 x 16 (single 16x16 tiles: the
    four-wave kernel and its one-wave variant), 17 (first size with two tile rows) — every kernel variant that takes the size,
    against the second, independent restatement (numpy + sympy + scipy LAPACK) run live: control flow exact, x, u, K, J to rounding."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    (n, m), T, B = nm, 21, 5
    rng = np.random.default_rng(100 * n + m)
    x1 = 0.5 * rng.standard_normal((B, n)); ub = 0.4 * rng.standard_normal((B, T - 1, m)) + 0.9      # starts across the action box
    mdl = pkg.models.synth_nm(n, m)
    dyn, costs, cons = R.synth32_problem(T, n, m)
    refs = []
    for b in range(B):
        s = R.Solver(dyn, costs, cons)
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dyn, x1[b], ub[b]))
        s.solve()
        refs.append(s)
    variants = ("latency", "throughput", "packed") if (n <= 4 and m <= 4) else (("latency", "mid") if n <= 16 else ("latency",))
    for v in variants:
        sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                         [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0), name="sweep%d_%d" % (n, m))
        sol.set_kernel_variant_(v)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
        for b, s in enumerate(refs):
            assert st["iterations"][b] == s.iterations and st["outer_iterations"][b] == s.outer_iterations, (v, b, st["iterations"][b], s.iterations)
            assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 1e-8, (v, b)
            Kr = np.stack([Kt.T for Kt in s.K])
            assert np.abs(K[b] - Kr).max() <= 1e-7 * max(1.0, np.abs(Kr).max()), (v, b)
            assert abs(st["objective"][b] - s.objective) <= 1e-9 * max(1.0, abs(s.objective)), (v, b)
        assert st["iterations"].min() >= 2
        sol.close()


def test_more_than_64_constraint_rows_small_path(pkg):
    """70 stage rows on a (2, 1) model (tests/test_abi.py: 34 nested action boxes, an identically-zero equality, an identically -1
    inequality in the SECOND mask word): the C-source route (ilqr_compile_model_rows) and the symbolic route (codegen word arrays)
    against the independent restatement, on every small-path kernel. A lost inequality bit of row 69 would show as a violation of 1."""
    import ctypes as C
    import sympy as sp
    from test_abi import _ModelSource, _rows70_source, ROWS70_WORDS
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    T, B = 21, 6
    rng = np.random.default_rng(70)
    x1 = 0.3 * rng.standard_normal((B, 2)); ub = 0.8 * rng.standard_normal((B, T - 1, 1))
    f = lambda x, u: [x[0] + 0.1 * x[1], x[1] + 0.1 * (u[0] - sp.sin(x[0]))]
    lst = lambda x, u: x[0] * x[0] + x[1] * x[1] + 0.1 * u[0] * u[0]
    ltm = lambda x, u: 10.0 * ((x[0] - 1.0) * (x[0] - 1.0) + x[1] * x[1])
    rows = lambda x, u: sum([[u[0] - (0.5 + 0.01 * i), -(0.5 + 0.01 * i) - u[0]] for i in range(34)], []) + [0.0 * u[0], -1.0 + 0.0 * u[0]]
    ineq = list(range(1, 69)) + [70]
    refs = []
    dyn_r = R.Dynamics(f, 2, 1); con_r = R.Constraint(rows, 2, 1, indices_inequality=ineq)
    for b in range(B):
        s = R.Solver([dyn_r] * (T - 1), [R.Cost(lst, 2, 1)] * (T - 1) + [R.Cost(ltm, 2, 0)], [con_r] * (T - 1) + [R.Constraint()])
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout([dyn_r] * (T - 1), x1[b], ub[b]))
        s.solve()
        refs.append(s)
    L = pkg._ffi.lib()
    ms = _ModelSource(b"rows70", 2, 1, 0, 70, 0, 0, 0, _rows70_source().encode())
    name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
    assert L.ilqr_compile_model_rows(C.byref(ms), (C.c_uint64 * 2)(*ROWS70_WORDS), None, name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
    con = pkg.Constraint(rows, 2, 1, indices_inequality=ineq)
    for route in ("c", "symbolic"):
        for v in ("latency", "throughput", "packed"):
            if route == "c":
                sol = pkg.Solver(model=name.value.decode(), horizon=T, batch=B, options=pkg.Options(verbose=0))
            else:
                sol = pkg.Solver([pkg.Dynamics(f, 2, 1)] * (T - 1), [pkg.Cost(lst, 2, 1)] * (T - 1) + [pkg.Cost(ltm, 2, 0)],
                                 [con] * (T - 1) + [pkg.Constraint()], batch=B, options=pkg.Options(verbose=0), name="rows70s")
            assert sol.nc_stage == 70
            sol.set_kernel_variant_(v)
            sol.initialize_rollout_(x1, ub); sol.solve_()
            x, u = sol.get_trajectory(); st = sol.stats()
            assert (st["max_violation"] <= 5e-3).all(), (route, v, st["max_violation"])
            assert (np.abs(u) <= 0.5 + 5e-3).all()                 # the innermost of the nested boxes binds
            for b, s in enumerate(refs):
                assert st["iterations"][b] == s.iterations and st["outer_iterations"][b] == s.outer_iterations, (route, v, b)
                assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 1e-8, (route, v, b)
            sol.close()


def test_more_than_64_constraint_rows_large_path(pkg):
    """nx = 30, nu = 5 with an action box and a state box: 70 stage inequalities (synth_box) on the large path — four-wave kernel;
    cost pass, linearisation with Gauss-Newton AL terms over 70 rows — against the independent restatement."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    n, m, T, B = 30, 5, 21, 3
    rng = np.random.default_rng(3005)
    x1 = 0.9 * rng.standard_normal((B, n)); ub = 0.4 * rng.standard_normal((B, T - 1, m)) + 0.9       # across both boxes
    mdl = pkg.models.synth_box(n, m)
    sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                     [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0), name="box30")
    assert (sol.nx, sol.nu, sol.nc_stage) == (n, m, 70)
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    dyn, costs, cons = R.synth_box_problem(T, n, m)
    for b in range(B):
        s = R.Solver(dyn, costs, cons)
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dyn, x1[b], ub[b]))
        s.solve()
        assert st["iterations"][b] == s.iterations and st["outer_iterations"][b] == s.outer_iterations, (b, st["iterations"][b], s.iterations)
        assert st["iterations"][b] >= 2
        # (tolerance of the synth32 oracle tests: with dozens of active rows at penalties up to 1e4 one instance needs 330 iterations
        # and the last-bit differences between the two implementations' sums grow to a few 1e-8 in x; after ONE iteration and after
        # one dual update the same three instances agree to 1e-14)
        Kr = np.stack([Kt.T for Kt in s.K])
        assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 5e-7
        assert np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 5e-7 * max(1.0, np.abs(Kr).max())      # u = ū + K (x − x̄): |K| up to 1e2 here
        assert np.abs(K[b] - Kr).max() <= 5e-7 * max(1.0, np.abs(Kr).max())
        assert abs(st["max_violation"][b] - s.max_violation) <= 1e-7
    sol.close()


def test_cooperative_rollout_with_non_affine_trig_arguments(pkg):
    """The generated cooperative rollout code forms AFFINE trig arguments from per-lane coefficients and falls back to one select
    per angle otherwise (codegen.py). No built-in model takes the fallback: a user model with sin(x0 x1), cos(x0 + 2 x1^2)
    next to an affine sin(x0), on all three small-model kernels, against the independent restatement run live."""
    import sympy as sp
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    h, n, m, T, B = 0.1, 2, 1, 21, 4
    f = lambda x, u: [x[0] + h * (x[1] + 0.2 * sp.sin(x[0] * x[1])), x[1] + h * (u[0] - sp.sin(x[0]) + 0.1 * sp.cos(x[0] + 2.0 * x[1] * x[1]))]
    ls = lambda x, u: 0.1 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * u[0] * u[0]
    lt = lambda x, u: 2.0 * (x[0] * x[0] + x[1] * x[1])
    goal = lambda x, u: [x[0] - 0.5]
    rng = np.random.default_rng(77)
    x1 = 0.3 * rng.standard_normal((B, n)); ub = 0.5 * rng.standard_normal((B, T - 1, m))
    rdyn = R.Dynamics(f, n, m)
    rs = []
    for b in range(B):
        s = R.Solver([rdyn] * (T - 1), [R.Cost(ls, n, m)] * (T - 1) + [R.Cost(lt, n, 0)], [R.Constraint()] * (T - 1) + [R.Constraint(goal, n, 0)])
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout([rdyn] * (T - 1), x1[b], ub[b]))
        s.solve()
        rs.append(s)
    dyn = pkg.Dynamics(f, n, m)
    for variant in ("latency", "throughput", "packed"):
        sol = pkg.Solver([dyn] * (T - 1), [pkg.Cost(ls, n, m)] * (T - 1) + [pkg.Cost(lt, n, 0)],
                         [pkg.Constraint()] * (T - 1) + [pkg.Constraint(goal, n, 0)], batch=B, options=pkg.Options(verbose=0), name="nonaffine")
        sol.set_kernel_variant_(variant)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        x, u = sol.get_trajectory(); st = sol.stats()
        for b, s in enumerate(rs):
            assert st["iterations"][b] == s.iterations and st["rollouts"][b] == s.rollouts, (variant, b)
            assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 1e-8
        assert st["iterations"].min() >= 3
        sol.close()


def test_cooperative_rollout_with_many_angles_and_nested_trig(pkg):
    """Ten distinct angles on one dependency level (two batches of trig pairs: eight + two) and a nested sin(0.5 cos(x0)) on a
    second level, nx = 4, nu = 2, on all three small-model kernels, against the independent restatement run live."""
    import sympy as sp
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    h, n, m, T, B = 0.05, 4, 2, 17, 3

    def f(x, u):
        s = sp.sin
        a = [s(x[0]), sp.cos(x[1]), s(x[2]), sp.cos(x[3]), s(x[0] + x[1]), s(x[1] + x[2]), s(x[2] + x[3]), s(x[0] - x[3]), s(2.0 * x[0]), s(3.0 * x[1])]
        nest = s(0.5 * sp.cos(x[0]))
        return [x[0] + h * (x[2] + 0.1 * (a[0] + a[4] + a[8]) + 0.05 * nest),
                x[1] + h * (x[3] + 0.1 * (a[1] + a[5] + a[9])),
                x[2] + h * (u[0] - 0.3 * a[2] + 0.1 * a[6]),
                x[3] + h * (u[1] - 0.3 * a[3] + 0.1 * a[7])]
    ls = lambda x, u: 0.1 * sum(xi * xi for xi in x) + 0.05 * (u[0] * u[0] + u[1] * u[1])
    lt = lambda x, u: 2.0 * sum(xi * xi for xi in x)
    goal = lambda x, u: [x[0] - 0.4, x[1] + 0.2]
    rng = np.random.default_rng(78)
    x1 = 0.3 * rng.standard_normal((B, n)); ub = 0.5 * rng.standard_normal((B, T - 1, m))
    rdyn = R.Dynamics(f, n, m)
    rs = []
    for b in range(B):
        s_ = R.Solver([rdyn] * (T - 1), [R.Cost(ls, n, m)] * (T - 1) + [R.Cost(lt, n, 0)], [R.Constraint()] * (T - 1) + [R.Constraint(goal, n, 0)])
        s_.initialize_controls(ub[b]); s_.initialize_states(R.rollout([rdyn] * (T - 1), x1[b], ub[b]))
        s_.solve()
        rs.append(s_)
    dyn = pkg.Dynamics(f, n, m)
    for variant in ("latency", "throughput", "packed"):
        sol = pkg.Solver([dyn] * (T - 1), [pkg.Cost(ls, n, m)] * (T - 1) + [pkg.Cost(lt, n, 0)],
                         [pkg.Constraint()] * (T - 1) + [pkg.Constraint(goal, n, 0)], batch=B, options=pkg.Options(verbose=0), name="manyangles")
        sol.set_kernel_variant_(variant)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        x, u = sol.get_trajectory(); st = sol.stats()
        for b, s_ in enumerate(rs):
            assert st["iterations"][b] == s_.iterations and st["rollouts"][b] == s_.rollouts, (variant, b, st["iterations"][b], s_.iterations)
            assert np.abs(x[b] - np.stack(s_.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s_.nominal_actions[:-1])).max() < 1e-8
        sol.close()


def test_cooperative_rollout_with_a_parameter_inside_a_trig_argument(pkg):
    """θ_t (src/dynamics.jl:23: f(x, u, w)) inside an affine trig argument, sin(x0 + w0), per instance and timestep, on all three
    small-model kernels against the independent restatement run live."""
    import sympy as sp
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    h, n, m, T, B = 0.1, 2, 1, 19, 3
    f = lambda x, u, w: [x[0] + h * x[1], x[1] + h * (u[0] - sp.sin(x[0] + w[0]) + 0.2 * sp.cos(2.0 * x[0] - 0.5 * w[0]))]
    ls = lambda x, u, w: 0.1 * (x[0] * x[0] + x[1] * x[1]) + 0.05 * u[0] * u[0]
    lt = lambda x, u, w: 2.0 * (x[0] * x[0] + x[1] * x[1])
    goal = lambda x, u, w: [x[0] - 0.5]
    rng = np.random.default_rng(79)
    x1 = 0.3 * rng.standard_normal((B, n)); ub = 0.5 * rng.standard_normal((B, T - 1, m)); th = 0.4 * rng.standard_normal((B, T, 1))
    rdyn = R.Dynamics(f, n, m, 1)
    rs = []
    for b in range(B):
        par = [th[b, t] for t in range(T)]
        s_ = R.Solver([rdyn] * (T - 1), [R.Cost(ls, n, m, 1)] * (T - 1) + [R.Cost(lt, n, 0, 1)],
                      [R.Constraint()] * (T - 1) + [R.Constraint(goal, n, 0, num_parameter=1)], parameters=par)
        s_.initialize_controls(ub[b]); s_.initialize_states(R.rollout([rdyn] * (T - 1), x1[b], ub[b], par))
        s_.solve()
        rs.append(s_)
    dyn = pkg.Dynamics(f, n, m, 1)
    for variant in ("latency", "throughput", "packed"):
        sol = pkg.Solver([dyn] * (T - 1), [pkg.Cost(ls, n, m, 1)] * (T - 1) + [pkg.Cost(lt, n, 0, 1)],
                         [pkg.Constraint()] * (T - 1) + [pkg.Constraint(goal, n, 0, num_parameter=1)], batch=B, options=pkg.Options(verbose=0), name="thetatrig")
        sol.set_kernel_variant_(variant)
        sol.set_parameters_(th)
        sol.initialize_rollout_(x1, ub); sol.solve_()
        x, u = sol.get_trajectory(); st = sol.stats()
        for b, s_ in enumerate(rs):
            assert st["iterations"][b] == s_.iterations and st["rollouts"][b] == s_.rollouts, (variant, b, st["iterations"][b], s_.iterations)
            assert np.abs(x[b] - np.stack(s_.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s_.nominal_actions[:-1])).max() < 1e-8
        sol.close()


@pytest.mark.parametrize("config,B,devices", [("acrobot51", 64, [0, 0]), ("car", 96, [0, 0]), ("particle", 7, [0, 0, 0]), ("synth32", 5, [0, 0])])
def test_sharded_handle_equals_single_handle(pkg, config, B, devices):
    """ilqr_create_sharded (one Solver spanning several GPUs, as the reference's caller holds one Solver,
    src/solver.jl:28-46): the batch split into contiguous ranges over a device list — here sub-handles on the one GPU of the
    box — must reproduce the single handle BITWISE through every accessor (instances are independent; no data crosses ranges)."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    opt = dict(verbose=0, max_iterations=12) if config == "acrobot51" else dict(verbose=0)
    one = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(**opt))
    many = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(**opt), devices=devices)
    assert (many.nx, many.nu, many.B, many.T) == (one.nx, one.nu, B, T)
    for s in (one, many):
        s.enable_trace_(16)
        s.initialize_rollout_(x1, ub); s.solve_()
    for a, b in zip(one.get_trajectory() + one.get_policy(), many.get_trajectory() + many.get_policy()):
        assert np.array_equal(a, b, equal_nan=True)
    sa, sb = one.stats(), many.stats()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), k
    assert np.array_equal(one.trace(), many.trace(), equal_nan=True)
    for name in ("violations", "constraint_dual", "gradient_state", "K"):
        assert np.array_equal(one.buffer(name), many.buffer(name), equal_nan=True), name
    # setters scatter: a warm start through the sharded handle equals the same through the single one
    x, u = one.get_trajectory()
    for s in (one, many):
        s.reset_(); s.initialize_controls_(u * 0.9); s.initialize_states_(x); s.solve_()
    assert np.array_equal(one.get_trajectory()[0], many.get_trajectory()[0], equal_nan=True)
    # stage entry points and the host-stepped loop run on every range
    for s in (one, many):
        s.reset_(); s.initialize_rollout_(x1, ub); s.run_stage_("cost_nominal"); s.run_stage_("gradients"); s.run_stage_("backward_pass")
    assert np.array_equal(one.buffer("P"), many.buffer("P"), equal_nan=True)
    assert many.timing()[1] >= 1 and many.timing()[0] > 0.0
    one.close(); many.close()


@pytest.mark.parametrize("config,B,outer", [("acrobot51", 45, 2), ("acrobot51", 45, 4), ("car", 37, 2), ("particle", 9, 2)])
def test_straggler_handover_from_the_packed_to_the_latency_kernel(pkg, oracle, config, B, outer):
    """ilqr_set_handover: instances that enter outer iteration `outer` leave the packed kernel at that boundary and are finished
    by the latency kernel (here forced early, so that most instances change kernels mid-solve). The outcome must be the one of
    the packed kernel alone — same control flow, trace rows and results (the two kernels run the same arithmetic) — and it must
    not depend on which other instances share the batch."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)

    def run(handover, sel=slice(None), variant="packed"):
        nb = len(range(*sel.indices(B)))
        s = pkg.Solver(model=model, horizon=T, batch=nb, options=pkg.Options(verbose=0))
        s.set_kernel_variant_(variant); s.set_handover_(handover); s.enable_trace_(600)
        s.initialize_rollout_(x1[sel], ub[sel]); s.solve_()
        out = dict(x=s.get_trajectory()[0], u=s.get_trajectory()[1], K=s.get_policy()[0], st=s.stats(), tl=s.scalar("trace_len"),
                   tr=s.trace(), resume=s.scalar("resume"), lam=s.buffer("constraint_dual"))
        s.close()
        return out
    off, on = run(0), run(outer)
    moved = off["st"]["outer_iterations"] >= outer
    assert moved.any() and (on["resume"] == 0).all()
    for k in ("iterations", "outer_iterations", "rollouts", "status", "potrf_info"):
        assert np.array_equal(off["st"][k], on["st"][k]), k
    assert np.array_equal(off["tl"], on["tl"]) and (on["tl"] == on["st"]["iterations"]).all()       # one trace across both launches
    assert np.array_equal(off["tr"][:, :, [0, 1, 5, 6, 7]], on["tr"][:, :, [0, 1, 5, 6, 7]])
    for k in ("x", "u", "K", "lam"):
        assert np.abs(off[k] - on[k]).max() <= 1e-9 * max(1.0, np.abs(off[k]).max()), k
    assert np.array_equal(off["x"][~moved], on["x"][~moved])                                          # instances that never left: bitwise
    # batch independence: a sub-batch with the hand-over on gives bitwise what the instances got inside the larger batch
    sub = slice(3, 3 + min(B - 3, 7))
    part = run(outer, sub)
    assert np.array_equal(part["x"], on["x"][sub]) and np.array_equal(part["K"], on["K"][sub])
    # and the oracle agrees as with every other kernel
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=8)
    same = (on["st"]["iterations"] == ref["stats"]["iterations"]) & (on["st"]["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.95
    assert np.abs(on["x"] - ref["x"])[same].max() < 1e-7


@pytest.mark.parametrize("config,B,live", [("acrobot51", 45, 30), ("acrobot51", 45, 44), ("car", 37, 20), ("particle", 9, 8), ("acrobot", 300, 150)])
def test_straggler_handover_by_head_count_changes_no_result(pkg, config, B, live):
    """ilqr_set_handover_live: once no more than `live` instances of the batch are still running, each survivor leaves the packed
    kernel at the head of its next inner or outer iteration and the latency kernel finishes it in a launch behind it. WHICH
    instances leave, and where, depends on the timing of the run — so nothing may depend on it: counts, trace rows and every
    array must be those of the packed kernel alone, bitwise — the reported objective included: the two kernels do the same
    arithmetic, J in one canonical order (ilqr_device.hpp: objective_term) —, run after run."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)

    def run(on):
        s = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(config, {})))
        s.set_kernel_variant_("packed"); s.set_handover_(-1 if on else 0); s.set_handover_live_(live); s.enable_trace_(900)
        s.initialize_rollout_(x1, ub); s.solve_()
        out = dict(x=s.get_trajectory()[0], u=s.get_trajectory()[1], K=s.get_policy()[0], k=s.get_policy()[1], st=s.stats(),
                   tl=s.scalar("trace_len"), tr=s.trace(), resume=s.scalar("resume"), lam=s.buffer("constraint_dual"),
                   fx=s.buffer("jacobian_state"), gxx=s.buffer("hessian_state_state"), delta=s.scalar("delta_grad_product"),
                   gx=s.buffer("gradient_state"), gu=s.buffer("gradient_action"), xs=s.buffer("states"), us=s.buffer("actions"))
        s.close()
        return out
    off = run(False)
    for rep in range(3):
        on = run(True)
        assert (on["resume"] == 0).all()
        for k in ("iterations", "outer_iterations", "rollouts", "status", "potrf_info", "objective", "max_violation", "gradient_norm", "step_size"):
            assert np.array_equal(off["st"][k], on["st"][k], equal_nan=True), k
        assert np.array_equal(off["tl"], on["tl"])
        assert np.array_equal(off["tr"], on["tr"], equal_nan=True)            # every column, the objective included (one arithmetic for J in every kernel)
        # delta: the Armijo product of the LAST forward pass — the first one after a hand-over takes the number the packed kernel's
        # backward pass left in the block (S_DELTA_NEXT), not a sum of its own in another order
        for k in ("x", "u", "K", "k", "lam", "fx", "gxx", "delta", "gx", "gu", "xs", "us"):     # (fx, gx, gu, states: the resume launch's rounds of trials)
            assert np.array_equal(off[k], on[k], equal_nan=True), k


@pytest.mark.parametrize("config,B,offset,live,mark", [("acrobot", 61, 2 * 8192 + 2290, 40, 1), ("acrobot", 61, 2 * 8192 + 2290, 40, 8),
                                                       ("acrobot51", 45, 0, 30, 1), ("car", 37, 0, 20, 1), ("acrobot", 9, 6 * 8192 + 7605, 2, 8),
                                                       ("acrobot", 4104, 2 * 8192, 512, 6), ("acrobot51", 9000, 0, 1024, 2)])
def test_one_wave_packed_form_finishes_its_hand_overs_itself(pkg, config, B, offset, live, mark):
    """The one-wave form of the packed kernel (two packs per workgroup): a workgroup whose packs are through takes handed-over
    instances from the device-wide queue and finishes them with the latency kernel's code; an instance whose rejected line-search
    trials exceed the batch's mean by `mark` (ilqr_set_handover_mark) is marked, its workgroup's two packs leave at once and the
    workgroup finishes the marked instance first — and so do the other packs on its CU, whose workgroups keep quiet until no marked
    instance is on its way (4104 instances: 513 workgroups, two on every CU; 9000 instances: more workgroups than the chip holds at
    once — there nobody waits for anybody, a waiting workgroup would hold the next round's slots). Batches around the two stragglers of BASELINE config 4 (instance 2300 of shard 2,
    7609 of shard 6) and ordinary ones with the mark at one rejected trial (many marks). WHO leaves, and when, depends on the
    timing of the run: every count, trace row and array must be the latency kernel's, bitwise, run after run, and nothing may be
    left for the launch behind (resume = 0 everywhere)."""
    model, T, x1, ub = pkg.workloads.make_inputs(config, B, offset=offset)

    def run(variant, on=True):
        s = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(config, {})))
        s.set_kernel_variant_(variant); s.enable_trace_(1000)
        if variant != "latency":
            s.set_handover_(-1 if on else 0); s.set_handover_live_(live); s.set_handover_mark_(mark)
        s.initialize_rollout_(x1, ub); s.solve_()
        out = dict(x=s.get_trajectory()[0], u=s.get_trajectory()[1], K=s.get_policy()[0], k=s.get_policy()[1], st=s.stats(),
                   tl=s.scalar("trace_len"), tr=s.trace(), resume=s.scalar("resume"), lam=s.buffer("constraint_dual"),
                   fx=s.buffer("jacobian_state"), gxx=s.buffer("hessian_state_state"), delta=s.scalar("delta_grad_product"),
                   # the workers take their line-search trials in rounds of four (forward_pass<M, 2>): the extra trials live in the
                   # LDS of fx, fu, and problem.states / actions must be the LAST trial evaluated
                   gx=s.buffer("gradient_state"), gu=s.buffer("gradient_action"), xs=s.buffer("states"), us=s.buffer("actions"),
                   ho=s.handover_stats() if variant != "latency" else (0, 0))
        s.close()
        return out
    ref = run("latency")
    marked = 0
    for rep in range(3 if B < 1000 else 2):
        on = run("packed1")
        assert (on["resume"] == 0).all()
        marked += on["ho"][1]
        for k in ("iterations", "outer_iterations", "rollouts", "status", "potrf_info", "objective", "max_violation", "gradient_norm", "step_size"):
            assert np.array_equal(ref["st"][k], on["st"][k], equal_nan=True), k
        assert np.array_equal(ref["tl"], on["tl"])
        assert np.array_equal(ref["tr"], on["tr"], equal_nan=True)
        for k in ("x", "u", "K", "k", "lam", "fx", "gxx", "delta", "gx", "gu", "xs", "us"):
            assert np.array_equal(ref[k], on[k], equal_nan=True), k
    assert marked > 0 or config in ("car", "acrobot51")           # the straggler batches do mark
    off = run("packed1", on=False)
    for k in ("x", "u", "K", "lam"):
        assert np.array_equal(ref[k], off[k], equal_nan=True), k


@pytest.mark.parametrize("min_step", [1.0e-5, 0.125, 0.3])
def test_line_search_in_rounds_is_the_search_trial_by_trial(pkg, oracle, min_step):
    """forward_pass<M, SPEC> rolls out up to four step sizes of a line search at once (the rows of the rollout's wave) and then does,
    trial by trial, what src/forward_pass.jl:28-52 does. Against the oracle (one trial after the other): instances 880..891 of
    BASELINE config 4 — 885 fails EVERY search (17 trials down to min_step_size, then the inner solve ends: the trial buffers in the
    LDS of fx, fu must be brought back, problem.states must be the last trial) — and 2296..2303 (2300: two rollouts per iteration),
    with min_step_size at its default and at values that cut a round short (0.125: s, s/2, s/4, s/8 and no further; 0.3: two
    trials). Iterations, ROLLOUTS, status and step sizes exact; then the packed kernel's workers (rounds from the first trial) and
    the resume launch bitwise against the latency kernel, Jacobians and problem.states included."""
    model, T, x1a, uba = pkg.workloads.make_inputs("acrobot", 12, offset=880)
    _, _, x1b, ubb = pkg.workloads.make_inputs("acrobot", 8, offset=2 * 8192 + 2296)
    x1, ub = np.concatenate([x1a, x1b]), np.concatenate([uba, ubb])
    B = len(x1)
    opts = dict(min_step_size=min_step)
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=8, options=oracle.default_options(**opts))
    out = {}
    for variant in ("latency", "packed1"):
        s = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0, **opts))
        s.set_kernel_variant_(variant); s.enable_trace_(1100)
        if variant == "packed1":
            s.set_handover_(-1); s.set_handover_live_(B - 3); s.set_handover_mark_(1)
        s.initialize_rollout_(x1, ub); s.solve_()
        out[variant] = dict(x=s.get_trajectory()[0], u=s.get_trajectory()[1], K=s.get_policy()[0], st=s.stats(), tr=s.trace(),
                            fx=s.buffer("jacobian_state"), fu=s.buffer("jacobian_action"), xs=s.buffer("states"), us=s.buffer("actions"),
                            gx=s.buffer("gradient_state"))
        s.close()
    a = out["latency"]
    # instance 2300 itself is chaotic (the oracle against itself with ū·(1 + 1e-15) differs by 14 in x, profiles/r05_all_shards.txt):
    # it is in the batch for the bitwise comparison below, not for this one
    ok = np.arange(B) != 12 + 4
    for k in ("iterations", "rollouts", "outer_iterations", "status"):
        assert np.array_equal(a["st"][k][ok], ref["stats"][k][ok]), k
    assert (a["st"]["rollouts"] - a["st"]["iterations"]).max() >= 7             # searches that reject, and one instance whose searches fail
    fin = np.isfinite(ref["x"]).reshape(B, -1).all(1) & ok
    assert np.abs(a["x"] - ref["x"])[fin].max() < 1e-6 and np.abs(a["st"]["step_size"] - ref["stats"]["step_size"])[ok].max() == 0.0
    b = out["packed1"]
    for k in ("iterations", "rollouts", "status", "objective", "step_size"):
        assert np.array_equal(a["st"][k], b["st"][k], equal_nan=True), k
    assert np.array_equal(a["tr"], b["tr"], equal_nan=True)
    for k in ("x", "u", "K", "fx", "fu", "xs", "us", "gx"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_packed_kernel_extra_trials_for_an_instance_that_keeps_rejecting(pkg):
    """The packed kernel gives an instance with eight rejected line-search trials behind it up to three more trials within the
    cycle (ilqr_device_packed.hpp, ILQR_PK_TRIALS / ILQR_PK_REJECTS). Instance 2300 of shard 2 of BASELINE config 4 spends 1407
    rollouts on 725 iterations: with its three neighbours in one wave the path is taken hundreds of times, and every count, trace
    row and array must be what the latency kernel (one trial after the other, no cycles) gives — bitwise."""
    B = 4
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot", B, offset=2 * 8192 + 2300)
    out = {}
    for variant in ("packed", "latency"):
        s = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
        s.set_kernel_variant_(variant); s.set_handover_(0); s.enable_trace_(1000)
        s.initialize_rollout_(x1, ub); s.solve_()
        out[variant] = dict(x=s.get_trajectory()[0], u=s.get_trajectory()[1], K=s.get_policy()[0], st=s.stats(), tr=s.trace(),
                            lam=s.buffer("constraint_dual"))
        s.close()
    a, b = out["packed"], out["latency"]
    assert a["st"]["rollouts"][0] - a["st"]["iterations"][0] >= 500          # the rejecting kind
    for k in ("iterations", "outer_iterations", "rollouts", "status", "objective"):
        assert np.array_equal(a["st"][k], b["st"][k]), k
    assert np.array_equal(a["tr"], b["tr"], equal_nan=True)
    for k in ("x", "u", "K", "lam"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_c_callables_define_a_large_path_model(pkg, oracle, tmp_path):
    """ilqr_compile_model beyond nx, nu <= 4 (src/dynamics.jl:55-60, src/costs.jl:1-15, src/constraints.jl:54-64 accept any
    size): the synth12 callables of examples/synth12_model.c as C source -> AdaptedLargeModel (compact forms, every entry
    treated as state-dependent / non-zero) -> the four-wave large kernels; against the oracle's own synth12 and against the
    model the symbolic generator makes from the same functions. Then the plain-C host of examples/synth12_compile.c."""
    import ctypes as C
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "examples", "synth12_model.c"), "rb").read()

    class Src(C.Structure):
        _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                    ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]
    L = pkg._ffi.lib()
    ms = Src(b"synth12_t", 12, 5, 0, 10, 3, (1 << 10) - 1, 0, text)
    name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
    assert L.ilqr_compile_model(C.byref(ms), name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
    T, B = 41, 24
    rng = np.random.default_rng(12)
    x1 = 0.5 * rng.standard_normal((B, 12)); ub = 0.1 * rng.standard_normal((B, T - 1, 5))
    kw = dict(max_iterations=15, max_dual_updates=3)
    sol = pkg.Solver(model=name.value.decode(), horizon=T, batch=B, options=pkg.Options(verbose=0, **kw))
    assert (sol.nx, sol.nu, sol.nc_stage, sol.nc_term) == (12, 5, 10, 3)
    sol.initialize_rollout_(x1, ub)
    assert np.abs(sol.buffer("nominal_states").reshape(B, T, 12)[0] - oracle.Problem("synth12", T).rollout(x1[0], ub[0])).max() < 1e-12
    sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    ref = oracle.solve_batch("synth12", T, x1, ub, options=oracle.default_options(**kw), nthreads=4)
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.95, same.mean()
    assert np.abs(x - ref["x"])[same].max() < 1e-7 and np.abs(u - ref["u"])[same].max() < 1e-7
    assert np.abs(K - ref["K"])[same].max() <= 5e-7 * np.abs(ref["K"]).max()
    # the mirror of the compact rows: full Jacobians / Hessians read back like the reference's buffers
    fx = sol.buffer("jacobian_state").reshape(B, T - 1, 12, 12)
    assert np.abs(fx).max() > 0 and np.isfinite(sol.buffer("hessian_state_state")).all()
    sol.close()
    exe = str(tmp_path / "synth12_compile")
    lib = os.path.join(root, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "synth12_compile.c"),
                           "-o", exe, "-L" + lib, "-lilqr_hip", "-Wl,-rpath," + lib, "-lm"])
    out = subprocess.run([exe, os.path.join(root, "examples", "synth12_model.c")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0, out.stdout.decode()[-2000:]
    assert b"max |dx| = 0.000e+00" in out.stdout


@pytest.mark.parametrize("generator", GENERATORS)
def test_synth32_literal_config5_shard_against_the_oracle(pkg, oracle, generator):
    """BASELINE configs[4] exactly as SURVEY §8(d) states it and as `bench.py --config synth32` and profiles/r0x_synth32* measure
    it: x1 ~ 0.5 N(0,1), ū = 0 (NOT perturbed), default tolerances, the 512-instance shard of rank 5, on the four-wave latency
    kernel. Every instance against the oracle: control flow identical on all of them, |Δx|, |Δu| <= 1e-11, |ΔK| <= 1e-11 max|K|
    (over the shard and per instance), |Δk| <= 1e-13 max(max |k|, 1) per instance (TOL_K_LARGE) (src/solve.jl:88-129, whole solve)."""
    B = 512
    r = _whole_solve(pkg, oracle, "synth32", B, 1.0, generator=generator, offset=5 * B, expect_kernel="latency",
                     tol=1e-11, tol_K=1e-11, tol_k=TOL_K_LARGE)
    assert not r["ub"].any()
    x, u, K, st, ref = r["x"], r["u"], r["K"], r["st"], r["ref"]
    rs = ref["stats"]
    assert r["same"].all(), r["same"].mean()
    dx_, du_, dK_ = np.abs(x - ref["x"]).max(), np.abs(u - ref["u"]).max(), np.abs(K - ref["K"]).max() / np.abs(ref["K"]).max()
    assert dx_ <= 1e-11 and du_ <= 1e-11 and dK_ <= 1e-11, (dx_, du_, dK_)          # observed 1.8e-15 / 1.0e-14 / 3.1e-15
    assert (st["potrf_info"] == 0).all() and (rs["potrf_info"] == 0).all()


def test_synth32_tight11_against_the_oracle(pkg, oracle):
    """The large-path workload that is profiled (`bench.py --config synth32_tight11`: tolerances 1e-11, ~80 inner iterations of the
    four-wave latency kernel per instance) on the inputs bench.py times: 512 instances against the oracle with the literal config
    5's bar where the control flow is the oracle's. The objective test stops at |ΔJ| < 1e-11, the size of J's rounding: the last
    step lands on either side of it, so some instances stop one inner iteration earlier or later than the oracle (observed: 25 of
    512, J 1e-11 apart; the oracle itself changes path on 6 of the 512 when x1 moves by one part in 1e15:
    tools/oracle_self_flow.py, profiles/r07_parity.txt) — there the solutions still agree to what one more converged step changes
    (observed |Δx| 8e-8, |Δu| 8e-7)."""
    B = 512
    r = _whole_solve(pkg, oracle, "synth32_tight11", B, 0.9, generator="splitmix64", expect_kernel="latency",
                     tol=1e-11, tol_K=1e-11, tol_k=TOL_K_LARGE)
    st, rs = r["st"], r["ref"]["stats"]
    assert (st["iterations"] > 10).mean() > 0.9 and (st["potrf_info"] == 0).all()
    assert (st["outer_iterations"] == rs["outer_iterations"]).all() and (st["status"] == rs["status"]).all()
    assert (np.abs(st["iterations"] - rs["iterations"]) <= 1).all()
    d = ~r["same"]
    assert r["err"]["x"][d].max(initial=0.0) <= 1e-6 and r["err"]["u"][d].max(initial=0.0) <= 1e-5, (r["err"]["x"][d].max(), r["err"]["u"][d].max())


# auto's boundaries (csrc/ilqr_launch_plan.hpp, rows of tests/launch_plan_check.cpp at 256 CUs), in units of the device's CUs C:
# (config, B as (a, b) = a C + b, kernel auto picks). acrobot51: the latency kernel up to one instance per SIMD, the packed kernel
# beyond; car: the two-wave packed form up to 4 packs per CU, the one-wave form at 5; synth12: the four-wave latency kernel up to
# two instances per SIMD, one wave per instance (mid) beyond
BOUNDARIES = [("acrobot51", (4, 0), "latency"), ("acrobot51", (4, 1), "packed2"),
              ("car", (16, 0), "packed2"), ("car", (16, 4), "packed1"),
              ("synth12", (8, 0), "latency"), ("synth12", (8, 1), "mid")]


@pytest.mark.parametrize("config,size,kernel", BOUNDARIES, ids=["%s-%dC+%d-%s" % (c, a, b, k) for c, (a, b), k in BOUNDARIES])
def test_auto_boundary_kernels_against_the_oracle(pkg, oracle, config, size, kernel):
    """Both sides of each boundary of the auto variant on this device: the kernel auto picks, and that kernel's whole solve of the
    splitmix64 inputs against the oracle (the kernels on the two sides are all correct: only the kernel assert sees a boundary
    in the wrong place)."""
    C = _num_simds() // 4
    B = size[0] * C + size[1]
    big = pkg.workloads.CONFIGS[config][0] == "synth12"
    # (at 256 CUs car's 16 C is BASELINE config 2, test_car_full_config_batch_4096[splitmix64]: one oracle solve for both)
    r = _whole_solve(pkg, oracle, config, B, 1.0 if big else 0.999, generator="splitmix64", expect_kernel=kernel,
                     reuse_oracle=config == "car", **(dict(tol=1e-11, tol_K=1e-11, tol_k=TOL_K_LARGE) if big else {}))
    if config == "car":
        _car_instance_0(r)


@pytest.mark.parametrize("config,col", [("synth32", 0), ("synth32", 5)])
def test_large_path_backward_pass_with_a_failed_pivot(pkg, oracle, config, col):
    """The reference ignores potrf's return code (src/backward_pass.jl:68-69): when Quu is not positive definite, K and k are what
    potrs makes of the partly factored matrix dpotf2 leaves behind, and the recursion goes on with them. The large path takes
    that case on a branch of its own (ilqr_device_large.hpp: failed pivot -> the literal dpotf2 sequence and LDS-resident solves);
    here guu gets a negative diagonal entry at three timesteps (pivot `col` + 1 fails first), and potrf_info, K, k, P, p and the
    Lagrangian gradient must be the oracle's."""
    B = 3
    model, T, x1, ub = pkg.workloads.make_inputs(config, B)
    ub = ub + 1.2 * np.sin(np.arange(ub.size).reshape(ub.shape))
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub)
    refs = [_oracle_solver(oracle, model, T, x1[b], ub[b])[1] for b in range(B)]
    n, m = sol.nx, sol.nu
    for r in refs:
        r.call("reset_model_objective"); r.call("cost_bang", 0); r.call("gradients")
    for b, r in enumerate(refs):
        guu = r.buffer("hessian_action_action").reshape(T - 1, m, m).copy()
        for t in ((T - 2, T // 2, 3) if b < 2 else ()):              # the third instance stays positive definite
            guu[t, col, col] = -5.0 - b
        r.set_buffer("hessian_action_action", guu)
    _sync_from_oracle(sol, refs, T)
    sol.run_stage_("backward_pass")
    for r in refs:
        r.call("backward_pass"); r.call("lagrangian_gradient")
    st = sol.stats()
    want = np.array([r.stats().potrf_info for r in refs])
    assert (want[:2] == col + 1).all() and want[2] == 0
    assert np.array_equal(st["potrf_info"], want)
    for name in ("K", "k", "P", "p"):
        gb = sol.buffer(name)
        for b in range(B):
            assert _rel(gb[b], refs[b].buffer(name)) < 1e-8, (name, b, _rel(gb[b], refs[b].buffer(name)))
    Lx = sol.buffer("gradient_state_lagrangian"); Lu = sol.buffer("gradient_action_lagrangian")
    for b in range(B):
        g = refs[b].buffer("gradient")
        assert _rel(Lx[b], g[:(T - 1) * n]) < 1e-8 and _rel(Lu[b], g[T * n:]) < 1e-8
    sol.close()


def test_one_action_backward_pass_with_a_failed_pivot_is_repeated_literally(pkg, oracle):
    """Latency kernel, models with one action: the short form of the Riccati recursion (backward_pass_m1) assumes positive pivots
    and a pass that meets another kind is repeated by the literal code. Acrobot with guu < 0 at two timesteps: potrf_info, K, k,
    P, p against the oracle (src/backward_pass.jl:68-75: LAPACK leaves q on the diagonal, potrs divides by it twice); the
    healthy instance beside them takes the short form alone, and a whole solve counts no repeated pass."""
    B = 3
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot51", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.set_kernel_variant_("latency")
    sol.initialize_rollout_(x1, ub)
    refs = [_oracle_solver(oracle, model, T, x1[b], ub[b])[1] for b in range(B)]
    n, m = sol.nx, sol.nu
    for r in refs:
        r.call("reset_model_objective"); r.call("cost_bang", 0); r.call("gradients")
    for b, r in enumerate(refs[:2]):
        guu = r.buffer("hessian_action_action").copy()
        guu[[T - 3, 7]] = -50.0 - 10.0 * b
        r.set_buffer("hessian_action_action", guu)
    _sync_from_oracle(sol, refs, T)
    sol.run_stage_("backward_pass")
    for r in refs:
        r.call("backward_pass"); r.call("lagrangian_gradient")
    want = np.array([r.stats().potrf_info for r in refs])
    assert (want[:2] == 1).all() and want[2] == 0
    assert np.array_equal(sol.stats()["potrf_info"], want)
    for name in ("K", "k", "P", "p"):
        gb = sol.buffer(name)
        for b in range(B):
            assert _rel(gb[b], refs[b].buffer(name)) < 1e-8, (name, b)
    sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()
    assert (sol.scalar("literal_backward_passes") == 0).all() and (sol.stats()["potrf_info"] == 0).all()
    sol.close()


def test_device_reciprocal_and_rsqrt_at_special_values(pkg):
    """ilqr::recip_fast / rsqrt_fast / sqrt_rsqrt_fast (v_rcp_f64 / v_rsq_f64 + Newton steps) replace IEEE division and sqrt on
    the serial chains (src/rollout.jl:27-29 through the generated dynamics, src/backward_pass.jl:68-75). On ordinary arguments they
    are within 1.5 ulp of IEEE; this pins what they return where IEEE gives a special value, as documented in DESIGN.md §6."""
    import ctypes as C
    L = pkg._ffi.lib()

    def run(fn, xs):
        xs = np.ascontiguousarray(xs, dtype=np.float64); ys = np.empty_like(xs)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        pkg._ffi.check(L.ilqr_device_math(fn.encode(), p(xs), p(ys), len(xs)))
        return ys
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(1e-3, 1e3, 4000), -rng.uniform(1e-3, 1e3, 1000), 10.0 ** rng.uniform(-280, 280, 2000)])
    r = run("recip_fast", xs)
    assert (np.abs(r - 1.0 / xs) <= 1.5 * np.spacing(np.abs(1.0 / xs))).all()
    pos = np.abs(xs)
    assert (np.abs(run("rsqrt_fast", pos) - 1.0 / np.sqrt(pos)) <= 2.0 * np.spacing(1.0 / np.sqrt(pos))).all()
    assert (np.abs(run("sqrt_fast", pos) - np.sqrt(pos)) <= 1.0 * np.spacing(np.sqrt(pos))).all()
    tiny = np.nextafter(0.0, 1.0)
    sp = np.array([0.0, -0.0, tiny, -tiny, 1e-310, 1e308, -1e308, np.inf, -np.inf, np.nan])
    with np.errstate(all="ignore"):
        ieee = 1.0 / sp
    r = run("recip_fast", sp)
    # IEEE: +-Inf at +-0 and at subnormals whose reciprocal overflows, a subnormal at 1e308, +-0 at +-Inf. The Newton step turns the
    # infinite ones into NaN (0 * Inf) and flushes the subnormal result: a NaN where the reference would carry an Inf — an
    # instance that is diverged in the reference too (the Inf becomes a NaN one operation later: Inf - Inf, 0 * Inf, sin(Inf))
    assert np.isinf(ieee[:4]).all() and np.isnan(r[:4]).all()
    assert np.isnan(r[4]) or np.isinf(r[4])
    assert abs(r[5]) <= 1.0e-307 and abs(r[6]) <= 1.0e-307 and np.isnan(r[9])
    assert np.isnan(r[7:9]).all() or (r[7:9] == 0.0).all()
    rs = run("rsqrt_fast", np.array([0.0, tiny, 1e-310, np.inf, np.nan]))
    assert np.isnan(rs[[0, 4]]).all() or (np.isinf(rs[0]) and np.isnan(rs[4]))     # IEEE 1/sqrt(0) = Inf; callers test the pivot first
    sn, cs = run("sin_fast", np.array([0.0, np.inf, np.nan, 1e300])), run("cos_fast", np.array([0.0, np.inf, np.nan, 1e300]))
    assert sn[0] == 0.0 and cs[0] == 1.0 and np.isnan(sn[1:3]).all() and np.isnan(cs[1:3]).all() and abs(sn[3]) <= 1.0


def test_dynamics_with_a_pole_against_the_oracle(pkg, oracle):
    """A dynamics with a division whose denominator is exactly zero at the initial state of some instances, close to zero on the
    way of others (pendulum_pole, oracle/models.cpp): IEEE division in the oracle and in the per-lane model code, recip_fast on
    the cooperative rollout path. Instances that hit the pole exactly are diverged in both (NaN objective, same counts);
    every other instance must agree as any model does."""
    import sympy as sp
    T, B = 21, 24
    dyn = pkg.Dynamics(lambda x, u: [x[0] + 0.1 * x[1], x[1] + 0.1 * (u[0] - sp.sin(x[0]) - 0.1 * x[1] + 0.001 / (x[0] - 0.3))], 2, 1)
    stage = pkg.Cost(lambda x, u: x[0] * x[0] + x[1] * x[1] + 0.1 * u[0] * u[0], 2, 1)
    term = pkg.Cost(lambda x, u: 10.0 * (x[0] * x[0] + x[1] * x[1]), 2, 0)
    rng = np.random.default_rng(11)
    x1 = np.stack([rng.uniform(-0.2, 0.6, B), rng.uniform(-0.5, 0.5, B)], 1)
    x1[0] = [0.3, 0.0]; x1[1] = [0.3, 0.2]                         # denominator exactly zero at t = 1
    x1[2] = [0.25, 0.5]                                             # x0 reaches 0.3 exactly after one step: 0.25 + 0.1 * 0.5
    ub = 0.05 * rng.standard_normal((B, T - 1, 1))
    sol = pkg.Solver([dyn] * (T - 1), [stage] * (T - 1) + [term], batch=B, options=pkg.Options(verbose=0), name="user_pendulum_pole")
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); st = sol.stats()
    ref = oracle.solve_batch("pendulum_pole", T, x1, ub, nthreads=4)
    rs = ref["stats"]
    for k in ("iterations", "rollouts", "status"):
        assert np.array_equal(st[k], rs[k]), (k, st[k], rs[k])
    dead = ~np.isfinite(ref["x"]).all(axis=(1, 2))
    assert dead[:2].all() and not dead[3:].all()
    assert np.array_equal(np.isfinite(x).all(axis=(1, 2)), ~dead)
    assert np.abs(x[~dead] - ref["x"][~dead]).max() < 1e-8 and np.abs(u[~dead] - ref["u"][~dead]).max() < 1e-8
    sol.close()


def test_c_callables_synth32_with_probed_structure(pkg, oracle):
    """BASELINE config 5's model handed over as C callables (examples/synth32_model.c): ilqr_compile_model finds the 32
    state-dependent Jacobian entries of 1280 and the 40 structurally non-zero Hessian entries of 1344 by probing the callables on the
    host (the sizes of the generated Model_synth32's tables) and the large kernels run on them; against the oracle and against the
    generated model (the constants are the host libm's here and the device's there: last-bit differences only)."""
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "examples", "synth32_model.c"), "rb").read()

    class Src(C.Structure):
        _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                    ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]
    L = pkg._ffi.lib()
    ms = Src(b"synth32_c", 32, 8, 0, 16, 0, (1 << 16) - 1, 0, text)
    name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
    assert L.ilqr_compile_model(C.byref(ms), name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
    jv, hs = C.c_int32(), C.c_int32()
    assert L.ilqr_model_compact_sizes(name.value, C.byref(jv), C.byref(hs)) == 0 and (jv.value, hs.value) == (32, 40)
    B = 6
    model, T, x1, ub = pkg.workloads.make_inputs("synth32", B)
    ub = ub + 1.5 * np.sin(0.37 * np.arange(ub.size).reshape(ub.shape))     # start outside the action box
    out = {}
    for label, mdl in (("c", name.value.decode()), ("generated", model)):
        sol = pkg.Solver(model=mdl, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.initialize_rollout_(x1, ub); sol.solve_()
        out[label] = (sol.get_trajectory(), sol.get_policy(), sol.stats(), sol.buffer("jacobian_state"), sol.buffer("hessian_action_action"))
        sol.close()
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=6)
    (x, u), (K, _), st, fx, guu = out["c"]
    same = (st["iterations"] == ref["stats"]["iterations"]) & (st["rollouts"] == ref["stats"]["rollouts"]) & (st["outer_iterations"] == ref["stats"]["outer_iterations"])
    assert same.all()
    assert np.abs(x - ref["x"]).max() < 1e-7 and np.abs(u - ref["u"]).max() < 1e-7
    assert np.abs(K - ref["K"]).max() <= 5e-7 * np.abs(ref["K"]).max()
    (xg, ug), _, stg, fxg, guug = out["generated"]
    assert np.array_equal(st["iterations"], stg["iterations"]) and np.abs(x - xg).max() < 1e-9
    # the mirror of the compact rows reads like the reference's full buffers whichever way the tables were made
    assert np.abs(fx - fxg).max() < 1e-13 and np.abs(guu - guug).max() <= 1e-12 * np.abs(guug).max()


def test_c_callables_synth32_without_the_structure_probe(pkg, oracle, monkeypatch):
    """The same C source with ILQR_NO_STRUCTURE_PROBE (what a host without a C++ compiler gets): dense tables — all 1280 Jacobian
    entries state-dependent, all 1344 Hessian entries streamed. Slow, but the reference takes any callable (src/dynamics.jl:55-60),
    so it must run and agree: against the oracle and against the probed build of the same source."""
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "examples", "synth32_model.c"), "rb").read()

    class Src(C.Structure):
        _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                    ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]
    L = pkg._ffi.lib()
    names = {}
    for label in ("dense", "probed"):
        if label == "dense":
            monkeypatch.setenv("ILQR_NO_STRUCTURE_PROBE", "1")
        else:
            monkeypatch.delenv("ILQR_NO_STRUCTURE_PROBE")
        ms = Src(b"synth32_c", 32, 8, 0, 16, 0, (1 << 16) - 1, 0, text)
        name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
        assert L.ilqr_compile_model(C.byref(ms), name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
        jv, hs = C.c_int32(), C.c_int32()
        assert L.ilqr_model_compact_sizes(name.value, C.byref(jv), C.byref(hs)) == 0
        assert (jv.value, hs.value) == ((1280, 1344) if label == "dense" else (32, 40))
        names[label] = name.value.decode()
    B, T = 4, 21
    model, _, x1, ub = pkg.workloads.make_inputs("synth32", B)
    ub = ub[:, :T - 1] + 1.5 * np.sin(0.37 * np.arange(B * (T - 1) * 8).reshape(B, T - 1, 8))
    out = {}
    for label, mdl in names.items():
        sol = pkg.Solver(model=mdl, horizon=T, batch=B, options=pkg.Options(verbose=0))
        sol.initialize_rollout_(x1, ub); sol.solve_()
        out[label] = (sol.get_trajectory(), sol.get_policy(), sol.stats(), sol.buffer("jacobian_action"), sol.buffer("hessian_state_state"))
        sol.close()
    ref = oracle.solve_batch(model, T, x1, ub, nthreads=4)
    (x, u), (K, _), st, fu, gxx = out["dense"]
    assert (st["iterations"] == ref["stats"]["iterations"]).all() and (st["rollouts"] == ref["stats"]["rollouts"]).all() and st["iterations"].min() >= 2
    assert np.abs(x - ref["x"]).max() < 1e-7 and np.abs(u - ref["u"]).max() < 1e-7
    assert np.abs(K - ref["K"]).max() <= 5e-7 * np.abs(ref["K"]).max()
    (xp, up), (Kp, _), stp, fup, gxxp = out["probed"]
    assert np.array_equal(st["iterations"], stp["iterations"]) and np.abs(x - xp).max() < 1e-10 and np.abs(K - Kp).max() <= 1e-9 * np.abs(Kp).max()
    assert np.abs(fu - fup).max() < 1e-14 and np.abs(gxx - gxxp).max() <= 1e-12 * np.abs(gxxp).max()


@pytest.mark.parametrize("probe", [True, False])
def test_c_callables_at_the_size_limits(pkg, probe, monkeypatch):
    """ilqr_compile_model at nx = 64, nu = 16, 32 stage rows (the limits it advertises; advisor finding of round 3: only nx = 12 had
    ever run): the synth family's C source (models.synth_c_source, what examples/synth32_model.c is for 32 x 8), with the structure probe (64 of 5120 Jacobian entries
    state-dependent, 80 of 5376 Hessian entries) and without it (dense tables: every entry through per-thread arrays — tens of KB of
    scratch per thread, slow, but it must run), against the independent restatement of the same family."""
    import ctypes as C
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import reference_restatement as R
    text = pkg.models.synth_c_source(64, 16).encode()

    class Src(C.Structure):
        _fields_ = [("name", C.c_char_p), ("nx", C.c_int32), ("nu", C.c_int32), ("nw", C.c_int32), ("nc_stage", C.c_int32),
                    ("nc_term", C.c_int32), ("ineq_stage", C.c_uint64), ("ineq_term", C.c_uint64), ("source", C.c_char_p), ("flags", C.c_int32)]
    if not probe:
        monkeypatch.setenv("ILQR_NO_STRUCTURE_PROBE", "1")
    L = pkg._ffi.lib()
    ms = Src(b"synth64_c", 64, 16, 0, 32, 0, (1 << 32) - 1, 0, text)
    name = C.create_string_buffer(128); path = C.create_string_buffer(1024)
    assert L.ilqr_compile_model(C.byref(ms), name, 128, path, 1024) == 0, L.ilqr_last_error().decode()
    jv, hs = C.c_int32(), C.c_int32()
    assert L.ilqr_model_compact_sizes(name.value, C.byref(jv), C.byref(hs)) == 0
    assert (jv.value, hs.value) == ((64, 80) if probe else (64 * 80, 64 * 64 + 16 * 16 + 16 * 64))
    n, m, T, B = 64, 16, 11, 2
    rng = np.random.default_rng(64)
    x1 = 0.5 * rng.standard_normal((B, n)); ub = 0.4 * rng.standard_normal((B, T - 1, m)) + 0.8
    sol = pkg.Solver(model=name.value.decode(), horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub); sol.solve_()
    x, u = sol.get_trajectory(); K, k = sol.get_policy(); st = sol.stats()
    dyn, costs, cons = R.synth32_problem(T, n, m)
    for b in range(B):
        s = R.Solver(dyn, costs, cons)
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dyn, x1[b], ub[b]))
        s.solve()
        assert st["iterations"][b] == s.iterations and st["outer_iterations"][b] == s.outer_iterations and s.iterations >= 2
        assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 1e-8
        Kr = np.stack([Kt.T for Kt in s.K])
        assert np.abs(K[b] - Kr).max() <= 1e-7 * max(1.0, np.abs(Kr).max())
    sol.close()


def test_large_model_setter_shows_what_the_kernels_will_use(pkg):
    """Large path: the full jacobian_* / hessian_* arrays are a mirror of the compact rows the kernels stream. A host write at a
    CONSTANT Jacobian position, or outside the structural Hessian pattern, cannot be represented in the compact form: it is
    dropped, and a getter afterwards must return what the kernels will use — the generated constant, a zero — not the value
    written (advisor finding, round 3: the getter kept returning the host's values). Entries inside the pattern round-trip."""
    B = 2
    model, T, x1, ub = pkg.workloads.make_inputs("synth32", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    sol.initialize_rollout_(x1, ub); sol.run_stage_("cost_nominal"); sol.run_stage_("gradients")
    fx = sol.buffer("jacobian_state").reshape(B, T - 1, 32, 32).copy()        # [b][t][column][row]
    gxx = sol.buffer("hessian_state_state").reshape(B, T, 32, 32).copy()
    w = fx.copy()
    w[:, :, 3, 5] += 7.0            # (row 5, column 3): a constant entry of A
    w[:, :, 4, 4] += 0.25           # a diagonal entry: state-dependent, representable
    sol.set_buffer("jacobian_state", w)
    back = sol.buffer("jacobian_state").reshape(B, T - 1, 32, 32)
    assert np.array_equal(back[:, :, 3, 5], fx[:, :, 3, 5])                   # the constant stands
    assert np.array_equal(back[:, :, 4, 4], w[:, :, 4, 4])                    # the state-dependent entry took the write
    h = gxx.copy()
    h[:, :, 1, 2] = 3.0             # off the diagonal: outside the pattern of this model's Hessians
    h[:, :, 6, 6] += 1.5
    sol.set_buffer("hessian_state_state", h)
    back = sol.buffer("hessian_state_state").reshape(B, T, 32, 32)
    assert (back[:, :, 1, 2] == 0.0).all() and np.array_equal(back[:, :, 6, 6], h[:, :, 6, 6])
    sol.close()


def test_one_wave_variant_of_the_large_path_equals_the_four_wave_kernel(pkg, oracle):
    """Large models whose matrices are single 16x16 tiles (4 < nx <= 16, nu <= 16 — the sizes most models have, and for which the
    reference sizes its buffers at run time like for any other, /root/reference/src/data/policy.jl:44-78): `mid`, ONE wave per
    instance running the four wave roles of every phase in turn (eight instances per CU instead of two). Same phase functions,
    same arithmetic: stage results and whole solves BITWISE those of the four-wave kernel; against the oracle like it (`auto` takes
    the variant beyond 8 instances per CU: tools/mid_bench.py)."""
    T, B = 41, 96
    mdl = pkg.models.synth12()
    rng = np.random.default_rng(12)
    x1 = 0.5 * rng.standard_normal((B, 12)); ub = 0.1 * rng.standard_normal((B, T - 1, 5))
    kw = dict(max_iterations=15, max_dual_updates=3)
    out = {}
    for variant in ("latency", "mid"):
        sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                         [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=B, options=pkg.Options(verbose=0, **kw), name="synth12")
        sol.set_kernel_variant_(variant)
        sol.initialize_rollout_(x1, ub)
        sol.run_stage_("cost_nominal"); sol.run_stage_("gradients"); sol.run_stage_("backward_pass")
        stage = {k: sol.buffer(k) for k in ("jacobian_state", "hessian_action_action", "K", "k", "P", "p", "gradient_state_lagrangian")}
        sol.run_stage_("forward_pass")
        stage["x1"] = sol.buffer("nominal_states"); stage["delta"] = sol.scalar("delta_grad_product"); stage["alpha"] = sol.stats()["step_size"]
        sol.reset_(); sol.initialize_rollout_(x1, ub); sol.enable_trace_(80); sol.solve_()
        out[variant] = dict(stage=stage, x=sol.get_trajectory()[0], u=sol.get_trajectory()[1], K=sol.get_policy()[0], st=sol.stats(),
                            tr=sol.trace(), lam=sol.buffer("constraint_dual"))
        sol.close()
    a, b = out["latency"], out["mid"]
    for k in a["stage"]:
        assert np.array_equal(a["stage"][k], b["stage"][k], equal_nan=True), k
    for k in ("iterations", "outer_iterations", "rollouts", "status", "potrf_info", "objective", "max_violation"):
        assert np.array_equal(a["st"][k], b["st"][k], equal_nan=True), k
    for k in ("x", "u", "K", "lam", "tr"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    ref = oracle.solve_batch("synth12", T, x1, ub, options=oracle.default_options(**kw), nthreads=4)
    same = (b["st"]["iterations"] == ref["stats"]["iterations"]) & (b["st"]["rollouts"] == ref["stats"]["rollouts"])
    assert same.mean() >= 0.99 and np.abs(b["x"] - ref["x"])[same].max() < 1e-7
    # the variant does not exist where a matrix needs more than one tile
    big = pkg.Solver(model="synth32", horizon=11, batch=2, options=pkg.Options(verbose=0))
    with pytest.raises(pkg._ffi.IlqrError):
        big.set_kernel_variant_("mid")
    big.close()


def _placement(pkg, sol):
    """(SIMD of the critical wave, SIMD of wave 1) per instance from the stamps the latency kernel leaves in the scalar block"""
    L = pkg._ffi.lib()
    sc = sol.buffer("_scalars")
    def where(v):
        v = int(v)
        return (v >> 32, (v >> 13) & 7, (v >> 12) & 1, (v >> 8) & 15, (v >> 4) & 3)
    h0, h1 = L.ilqr_scalar_slot(b"hw_id_wave0"), L.ilqr_scalar_slot(b"hw_id_wave1")
    return [(where(sc[b, h0]), where(sc[b, h1])) for b in range(sc.shape[0])], sc


def test_a_full_chip_launch_puts_one_critical_wave_on_every_simd(pkg):
    """the workgroups of a CU agree on their critical waves (pick_roles). On a chip whose SIMDs the batch fills exactly
    (4 workgroups of two waves per CU) no SIMD may host two critical waves — as launched, 3 % of them do, and the instances on those
    run 1.4 x slower than the rest; the time stamps must be set. A property of scheduling, not of results: asked of two of five
    launches (a workgroup that arrives late decides alone; observed: every launch)."""
    from collections import Counter
    L = pkg._ffi.lib()
    model, T, x1, ub = pkg.workloads.make_inputs("acrobot51", 1024)
    sol = pkg.Solver(model=model, horizon=T, batch=1024, options=pkg.Options(verbose=0, max_iterations=6, max_dual_updates=2))
    assert sol.resolved_kernel_variant() == "latency"
    good = 0
    for rep in range(5):
        sol.reset_(); sol.initialize_rollout_(x1, ub); sol.solve_()
        W, sc = _placement(pkg, sol)
        t0, t1 = sc[:, L.ilqr_scalar_slot(b"t_start")], sc[:, L.ilqr_scalar_slot(b"t_end")]
        assert (t1 > t0).all() and (t0 > 0).all()
        crit = Counter(w[0] for w in W)
        simds = set(w[0] for w in W) | set(w[1] for w in W)
        if len(simds) < 1024:
            pytest.skip("the device has fewer than 1024 SIMDs: the batch does not fill it exactly")
        assert all(w[0] != w[1] for w in W)
        good += max(crit.values()) == 1
    assert good >= 2, good
    sol.close()


def test_roles_change_no_result(pkg, tmp_path):
    """Which wave of an instance is the critical one is decided per launch from where the hardware put them; the two
    waves run the same code on the same data either way. ILQR_ROLE_SLOTS=0 (roles as launched) must give the same bits — in a
    process of its own, the library reads the variable once."""
    import subprocess
    code = ("import sys, hashlib, numpy as np; sys.path.insert(0, %r); from ilqr_amd_loader import load_package; pkg = load_package();"
            "h = hashlib.sha256();\n"
            "for cfg, B, var in (('acrobot51', 300, 'latency'), ('car', 1100, 'packed2')):\n"
            "    model, T, x1, ub = pkg.workloads.make_inputs(cfg, B); s = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0));"
            " s.set_kernel_variant_(var); s.initialize_rollout_(x1, ub); s.solve_();\n"
            "    for a in s.get_trajectory() + s.get_policy() + (s.stats()['iterations'], s.stats()['objective'], s.buffer('constraint_dual')): h.update(np.ascontiguousarray(a).tobytes())\n"
            "    s.close()\n"
            "print(h.hexdigest())") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("1", "0"):
        env = dict(os.environ, ILQR_ROLE_SLOTS=flag)
        r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out[flag] = r.stdout.decode().split()[-1]
    assert out["1"] == out["0"]
