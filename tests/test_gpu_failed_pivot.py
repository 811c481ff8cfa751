"""The failed-pivot branches of every kernel family against real LAPACK.

The reference ignores potrf's return code (src/backward_pass.jl:68-69): when Quu is not positive definite, K and k are what potrs
makes of the half-factored matrix dpotf2 leaves behind, and the recursion goes on with them. Every kernel family repeats such a step
on a cold, wave-uniform branch in the literal dpotf2 order (potrf_U<m> behind __any(potrf_U_nofail<m>) in ilqr_device.hpp and
ilqr_device_packed.hpp; potrf_U_lanes + potrs_U_lds in ilqr_device_large.hpp, with a second right-hand side per lane at nx = 64).
Whole solves meet almost no failed pivot, so here the pivots are made to fail:

  stage kernels   guu gets a negative (or NaN) diagonal entry at the first step taken, a middle one and t = 0, in two of three
                  instances; K_STAGE (nu = 2, 3, 4), K_STAGE_SLIM, K_STAGE_MID and the four-wave large kernel (one tile row, two,
                  and nx = 64), first, middle and last pivots (tests/failed_pivot_inputs.py: STAGE_CASES)
  fused kernels   a model whose stage cost carries w0 u_j^2 with a per-instance w0: the failure comes from the model, on the
                  latency, throughput and packed solve kernels, and in a short whole solve

The yardstick is tests/riccati_ref.py (the independent restatement's recursion with scipy's dpotrf / dpotrs) on the handle's own
buffers, and the oracle as well where it has the model. Bars: the project's Riccati bar, _rel < 1e-8 (the inputs keep two
differently rounded CPU passes within 1e-10 of each other — the oracle's pass and riccati_ref for car, synth12 and synth32, riccati_ref
with LAPACK's and with the oracle's factorisation and solves for the other sizes: tests/test_failed_pivot_inputs.py); potrf_info equal; a healthy
instance BITWISE what it is in a batch where nobody fails (on the packed kernel: the wave-mates of a failing instance go through
potrf_U instead of potrf_U_nofail); fused BITWISE staged. Generating a model's code is host work per handle (8 s at 64 x 8): the stage
cases share one handle per (model, variant, horizon), reset between uses.
Measured on an MI355X with the model modules in the library's cache: 37 tests in 34 s, each under 2.5 s except the first 64 x 8 case
(21 s: the symbolic derivatives of that model once per session and its code twice, one handle per horizon — host work, which
tests/test_gpu_parity.py's 64 x 8 case pays as well); the other two 64 x 8 cases reuse its handles and take under a second.

Worst observed |device - riccati_ref| / max(1, |riccati_ref|) per kernel family (MI355X), bar 1e-8; bitwise bars: no difference:
    K_STAGE (latency, nu = 2, 3, 4)        2.2e-11 (car, pivot 1)
    K_STAGE_SLIM (throughput)              5.9e-12 (synth 4 x 4, pivot 1)
    K_STAGE_MID (one-wave large)           5.6e-11 (synth 16 x 16, pivot 1)
    four-wave large (nx = 17, 32, 64)      5.0e-12 (synth 64 x 8, pivot 1)
    solve kernels, model-made failure      latency 1.1e-14, throughput 1.1e-14, packed 1.1e-14
"""
import numpy as np
import pytest

import failed_pivot_inputs as FP
import riccati_ref
from oracle_sync import sync_from_oracle
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu

R = riccati_ref.R
OUT = ("K", "k", "P", "p", "gradient_state_lagrangian", "gradient_action_lagrangian")


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
    s = oracle.Solver(pr, oracle.default_options())
    s.initialize_controls(ub); s.initialize_states(pr.rollout(x1, ub))
    return s


SYMBOLIC = {}           # the symbolic derivatives of a size once per session (20 s at 64 x 8)


@pytest.fixture(scope="module")
def handles():
    """(model, variant, horizon) -> the handle the stage cases of that shape share"""
    cache = {}
    yield cache
    for sol in cache.values():
        sol.close()


def _stage_handle(pkg, handles, model, variant, T, x1, ub):
    if (model, variant, T) in handles:
        sol = handles[(model, variant, T)]
        sol.reset_()                                    # a fresh solver: zero Hessians, potrf_info = 0
        sol.set_kernel_variant_(variant)
        sol.initialize_rollout_(x1, ub)
        return sol
    if isinstance(model, str) and model != "synth12":
        sol = pkg.Solver(model=model, horizon=T, batch=FP.B, options=pkg.Options(verbose=0))
    else:
        if model not in SYMBOLIC:
            SYMBOLIC[model] = pkg.models.synth12() if model == "synth12" else pkg.models.synth_nm(*model)
        mdl = SYMBOLIC[model]
        # the names test_gpu_parity.py gives the same models: one module in the library's cache for both
        name = "synth12" if model == "synth12" else ("synth%d" % model[0] if model[0] > 32 else "sweep%d_%d" % model)
        sol = pkg.Solver([mdl["dynamics"]] * (T - 1), [mdl["cost_stage"]] * (T - 1) + [mdl["cost_term"]],
                         [mdl["con_stage"]] * (T - 1) + [mdl["con_term"]], batch=FP.B, options=pkg.Options(verbose=0), name=name)
    sol.set_kernel_variant_(variant)
    sol.initialize_rollout_(x1, ub)
    handles[(model, variant, T)] = sol
    return sol


def _stage_run(pkg, handles, oracle, case, T, value=None):
    """One backward_pass stage with the case's pivot made to fail (value = None: negative; else that value at the middle step), and
    one with nobody failing. Returns (failing run, healthy run, oracle solvers or None); a run = dict(buffers, info, ref)."""
    _, variant, model, pivot = case
    n, m = FP.dims(model)
    x1, ub = FP.start(model, T)
    refs = None
    if isinstance(model, str):
        refs = [_oracle_solver(oracle, model, T, x1[b], ub[b]) for b in range(FP.B)]
        for r in refs:
            r.call("reset_model_objective"); r.call("cost_bang", 0); r.call("gradients")
    sol = _stage_handle(pkg, handles, model, variant, T, x1, ub)
    assert (sol.nx, sol.nu) == (n, m)
    if refs is not None:
        sync_from_oracle(sol, refs, T)                 # the oracle's linearisation: all three run the pass on identical arrays
    else:
        sol.run_stage_("cost_nominal"); sol.run_stage_("gradients")
    runs = []
    for fail in (False, True):                          # on one handle: nobody fails, then the case
        if fail:
            guu = FP.inject(sol.buffer("hessian_action_action"), T, m, pivot, value)
            sol.set_buffer("hessian_action_action", guu)
            if refs is not None:
                for b, r in enumerate(refs):
                    r.set_buffer("hessian_action_action", guu[b])
        inputs = {name: sol.buffer(name) for name in riccati_ref.INPUTS}         # as the kernels will read them
        if fail:
            assert np.array_equal(inputs["hessian_action_action"], guu, equal_nan=True)
        sol.run_stage_("backward_pass")
        runs.append(dict(buf={name: sol.buffer(name) for name in OUT}, info=sol.stats()["potrf_info"],
                         ref=riccati_ref.of_handle(sol, inputs) if fail else None))
    if refs is not None:
        for r in refs:
            r.call("backward_pass"); r.call("lagrangian_gradient")
    return runs[1], runs[0], refs


def _oracle_buffers(r, T, n):
    g = r.buffer("gradient")
    return dict(K=r.buffer("K"), k=r.buffer("k"), P=r.buffer("P"), p=r.buffer("p"),
                gradient_state_lagrangian=g[:(T - 1) * n], gradient_action_lagrangian=g[T * n:])


@pytest.mark.parametrize("case", FP.STAGE_CASES, ids=FP.case_id)
def test_stage_backward_pass_with_a_failed_pivot_is_lapacks(pkg, handles, oracle, case):
    _, _, model, pivot = case
    n, m = FP.dims(model)
    worst = 0.0
    for T in FP.HORIZONS:
        bad, healthy, refs = _stage_run(pkg, handles, oracle, case, T)
        want_info = np.array([info for _, info in bad["ref"]])
        assert (want_info == [pivot, pivot, 0]).all()
        assert np.array_equal(bad["info"], want_info), (T, bad["info"])
        assert (healthy["info"] == 0).all()
        for b in range(FP.B):
            for name in OUT:
                e = _rel(bad["buf"][name][b], bad["ref"][b][0][name])
                worst = max(worst, e)
                assert e < 1e-8, (T, b, name, e)
                if refs is not None:
                    eo = _rel(bad["buf"][name][b], _oracle_buffers(refs[b], T, n)[name])
                    assert eo < 1e-8, (T, b, name, "oracle", eo)
            if refs is not None:
                assert refs[b].stats().potrf_info == want_info[b]
        for name in OUT:                                # the instance beside the failing ones: as if nobody had failed
            assert np.array_equal(bad["buf"][name][2], healthy["buf"][name][2]), (T, name)
    print("%s: worst %.2e" % (FP.case_id(case), worst))


@pytest.mark.parametrize("case", FP.NAN_CASES, ids=FP.case_id)
def test_stage_backward_pass_with_a_nan_pivot(pkg, handles, oracle, case):
    """guu[t, j, j] = NaN at a middle step: K, k at that step and P, p from it backwards are NaN exactly where LAPACK's are, the rest is
    within the bar, and potrf_info = j + 1 — this project's diagnostic (the LAPACK here returns 0 on a NaN pivot)."""
    _, _, model, pivot = case
    n, m = FP.dims(model)
    for T in FP.HORIZONS:
        tm = FP.failing_steps(T)[1]
        bad, healthy, refs = _stage_run(pkg, handles, oracle, case, T, value=np.nan)
        assert np.array_equal(bad["info"], [pivot, pivot, 0]), (T, bad["info"])
        assert (healthy["info"] == 0).all()
        for b in range(FP.B):
            for name in OUT:
                got, want = bad["buf"][name][b], bad["ref"][b][0][name]
                assert np.array_equal(np.isnan(got), np.isnan(want)), (T, b, name)
                ok = ~np.isnan(want)
                assert not ok.any() or _rel(got[ok], want[ok]) < 1e-8, (T, b, name)
            K = bad["buf"]["K"][b].reshape(T - 1, n * m); P = bad["buf"]["P"][b].reshape(T, n * n)
            assert np.isnan(K[:tm + 1]).all() == (b < 2) and not np.isnan(K[tm + 1:]).any()
            assert np.isnan(P[:tm + 1]).all() == (b < 2) and not np.isnan(P[tm + 1:]).any()
            if refs is not None and b < 2:
                assert refs[b].stats().potrf_info == pivot
        for name in OUT:
            assert np.array_equal(bad["buf"][name][2], healthy["buf"][name][2]), (T, name)


# ------------------------------------------------------------------ fused kernels and the packed kernel: the failure comes from the model
def _w0_handle(pkg, n, m, T, variant, x1, ub, w, **options):
    dyn, costs, cons = FP.w0_problem(pkg, n, m, T)
    sol = pkg.Solver(dyn, costs, cons, batch=FP.FUSED_B, options=pkg.Options(verbose=0, **options), name="fpw%d%d" % (n, m))
    sol.set_kernel_variant_(variant)
    sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    return sol


FUSED_OUT = ("K", "k", "gradient_state_lagrangian", "gradient_action_lagrangian")


@pytest.mark.parametrize("variant", ["latency", "throughput", "packed"])
@pytest.mark.parametrize("nm", sorted(FP.FUSED_SIZES), ids=lambda nm: "%dx%d" % nm)
def test_fused_backward_pass_with_failed_pivots_from_the_model(pkg, nm, variant):
    """The Riccati recursion inside the solve kernels (max_iterations = 0: one linearisation, one backward pass) on instances whose
    every step fails at pivot j + 1: bitwise the stage kernels, LAPACK's within the bar, and the healthy instances bitwise what they
    are when nobody fails — on the packed kernel they share a wave with a failing one and take its branch."""
    n, m = nm
    pivot = FP.FUSED_SIZES[nm] + 1
    worst = 0.0
    for T in FP.FUSED_HORIZONS:
        out = {}
        for failing in ((),) + FP.FUSED_FAILING:
            x1, ub, w = FP.w0_inputs(n, m, T, failing)
            for mode in ("fused", "staged"):
                sol = _w0_handle(pkg, n, m, T, variant, x1, ub, w, max_iterations=0, max_dual_updates=1)
                if mode == "fused":
                    sol.solve_()
                else:
                    for st in ("al_begin", "cost_nominal", "gradients", "backward_pass"):
                        sol.run_stage_(st)
                res = {name: sol.buffer(name) for name in FUSED_OUT}
                res["gradient_norm"] = sol.stats()["gradient_norm"]; res["potrf_info"] = sol.stats()["potrf_info"]
                if mode == "staged":
                    res["ref"] = riccati_ref.of_handle(sol)
                out[(failing, mode)] = res
                sol.close()
            fused, staged = out[(failing, "fused")], out[(failing, "staged")]
            for name in FUSED_OUT + ("gradient_norm", "potrf_info"):
                assert np.array_equal(fused[name], staged[name]), (T, failing, name)
            want_info = np.array([pivot if b in failing else 0 for b in range(FP.FUSED_B)])
            assert np.array_equal(fused["potrf_info"], want_info), (T, failing, fused["potrf_info"])
            for b in range(FP.FUSED_B):
                ref, info = staged["ref"][b]
                assert info == want_info[b]
                for name in FUSED_OUT:
                    e = _rel(fused[name][b], ref[name])
                    worst = max(worst, e)
                    assert e < 1e-8, (T, failing, b, name, e)
                if b not in failing:
                    for name in FUSED_OUT + ("gradient_norm",):
                        assert np.array_equal(fused[name][b], out[((), "fused")][name][b]), (T, failing, b, name)
    print("fused %s %dx%d: worst %.2e" % (variant, n, m, worst))


@pytest.mark.parametrize("nm", sorted(FP.FUSED_SIZES), ids=lambda nm: "%dx%d" % nm)
def test_short_whole_solve_goes_on_with_the_garbage_gains_like_the_reference(pkg, nm):
    """max_iterations = 3 on the same model: the solve carries on with what potrs made of the half-factored matrices, as the reference
    does — iterations, rollouts, status and potrf_info identical to the restatement run live, x and u within the dimension sweep's
    1e-8, on every variant."""
    n, m = nm
    T, failing = 7, FP.FUSED_FAILING[1]
    pivot = FP.FUSED_SIZES[nm] + 1
    x1, ub, w = FP.w0_inputs(n, m, T, failing)
    dyn, costs, cons = FP.w0_problem(R, n, m, T)
    refs = []
    for b in range(FP.FUSED_B):
        par = [w[b, t] for t in range(T)]
        s = R.Solver(dyn, costs, cons, parameters=par, options=R.Options(max_iterations=3))
        s.initialize_controls(ub[b]); s.initialize_states(R.rollout(dyn, x1[b], ub[b], par))
        with np.errstate(all="ignore"):
            s.solve()
        assert s.potrf_info == (pivot if b in failing else 0)
        refs.append(s)
    for variant in ("latency", "throughput", "packed"):
        sol = _w0_handle(pkg, n, m, T, variant, x1, ub, w, max_iterations=3)
        sol.solve_()
        x, u = sol.get_trajectory(); st = sol.stats()
        for b, s in enumerate(refs):
            got = (st["iterations"][b], st["outer_iterations"][b], st["rollouts"][b], bool(st["status"][b]), st["potrf_info"][b])
            want = (s.iterations, s.outer_iterations, s.rollouts, bool(s.status), s.potrf_info)
            assert got == want, (variant, b, got, want)
            assert np.abs(x[b] - np.stack(s.nominal_states)).max() < 1e-8 and np.abs(u[b] - np.stack(s.nominal_actions[:-1])).max() < 1e-8, (variant, b)
        sol.close()
