"""The inputs of tests/test_gpu_failed_pivot.py are well conditioned: checked on the CPU, before the GPU test relies on the project's
Riccati bar (1e-8) for them.

Where the oracle has the model (car, synth12, synth32): the oracle's linearisation with the bad pivots injected, then the oracle's
backward pass (its own dpotf2 order) against tests/riccati_ref.py (real LAPACK, BLAS order) — two differently rounded passes over
the same arrays must agree to 1e-10, K, k, P, p, the Lagrangian gradient and the return code. The synth family at other sizes has no
oracle twin and the oracle no entry that takes arrays: there the linearisation is the restatement's, and riccati_ref is held
against the same recursion run with the ORACLE's factorisation and solves (orc_potrf_U / orc_potrs_U, dpotf2 order, in place of
scipy's dpotrf / dpotrs) — the two differ where the failed pivot is handled, and must agree to 1e-10 too. Beside it, the change of
riccati_ref's result when every input entry moves by one rounding (relative 2^-52, random signs) is bounded by the same 1e-10.
The model that fails by itself (fused and packed kernels) is checked like the synth family, and for the pivot it is meant to fail
at every step.
Observed: oracle's pass against riccati_ref 8.7e-12 at worst (synth12, pivot 1); the oracle's factorisation and solves inside the
restatement's recursion 3.2e-11 at worst (synth 16 x 16, pivot 1); one rounding of the inputs 3.6e-11 at worst (synth 16 x 16, pivot 1; a failing FIRST pivot amplifies
most: every later row of the solve goes through the division by it).
"""
import numpy as np
import pytest
from scipy.linalg import lapack

import failed_pivot_inputs as FP
import riccati_ref

R = riccati_ref.R
OUT = ("K", "k", "P", "p", "gradient_state_lagrangian", "gradient_action_lagrangian")


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def _restatement_linearisation(problem, x1, ub, w=None):
    dyn, costs, cons = problem
    T = len(costs)
    par = None if w is None else [w[t] for t in range(T)]
    s = R.Solver(dyn, costs, cons, parameters=par)
    s.initialize_controls(ub); s.initialize_states(R.rollout(dyn, x1, ub, par))
    s.cost_bang("nominal"); s.gradients_bang("nominal")
    return [np.stack(a) for a in (s.fx, s.fu, s.gx, s.gu, s.gxx, s.guu, s.gux)]


def _one_rounding(args, seed):
    """riccati_ref on `args` and on a copy moved by one rounding per entry: the worst relative change over the outputs"""
    rng = np.random.default_rng(seed)
    a = riccati_ref.to_buffers(riccati_ref.backward_pass(*args))
    moved = [v * (1.0 + 2.0 ** -52 * rng.choice([-1.0, 1.0], size=v.shape)) for v in args]
    b = riccati_ref.to_buffers(riccati_ref.backward_pass(*moved))
    return max(_rel(a[k], b[k]) for k in OUT)


class OracleLapack:
    """scipy.linalg.lapack's dpotrf / dpotrs, computed by the oracle's potrf_U / potrs_U"""

    def __init__(self, oracle):
        self.o = oracle

    def dpotrf(self, a, lower=0, clean=0, overwrite_a=0):
        a = np.asfortranarray(np.array(a, dtype=np.float64))
        return a, self.o.lib().orc_potrf_U(a.ctypes.data_as(self.o.c_double_p), a.shape[0])

    def dpotrs(self, U, b, lower=0):
        U = np.asfortranarray(U); b = np.asfortranarray(np.array(b, dtype=np.float64))
        self.o.lib().orc_potrs_U(U.ctypes.data_as(self.o.c_double_p), U.shape[0], b.ctypes.data_as(self.o.c_double_p), b.shape[1])
        return b, 0


def _oracle_factorisation(oracle, args):
    """riccati_ref against the same recursion with the oracle's factorisation and solves: the worst relative difference"""
    a = riccati_ref.backward_pass(*args)
    b = riccati_ref.backward_pass(*args, lapack=OracleLapack(oracle))
    assert a["info"] == b["info"]
    a, b = riccati_ref.to_buffers(a), riccati_ref.to_buffers(b)
    return max(_rel(b[k], a[k]) for k in OUT)


PROBLEMS = {}


def _synth(nm, T):
    if nm not in PROBLEMS:                       # the symbolic derivatives of a size once (a minute at 64 x 8), whatever the horizon
        PROBLEMS[nm] = R.synth32_problem(2, *nm)
    dyn, costs, cons = PROBLEMS[nm]
    return dyn * (T - 1), costs[:1] * (T - 1) + costs[1:], cons[:1] * (T - 1) + cons[1:]


@pytest.mark.parametrize("case", FP.STAGE_CASES, ids=FP.case_id)
def test_injected_pivots_leave_a_well_conditioned_pass(oracle, case):
    _, _, model, pivot = case
    n, m = FP.dims(model)
    worst, swap = 0.0, 0.0
    for T in FP.HORIZONS:
        x1, ub = FP.start(model, T)
        if isinstance(model, str):
            refs = []
            for b in range(FP.B):
                pr = oracle.Problem(model, T)
                s = oracle.Solver(pr, oracle.default_options())
                s.initialize_controls(ub[b]); s.initialize_states(pr.rollout(x1[b], ub[b]))
                s.call("reset_model_objective"); s.call("cost_bang", 0); s.call("gradients")
                refs.append(s)
            guu = FP.inject(np.stack([s.buffer("hessian_action_action") for s in refs]), T, m, pivot)
            for b, s in enumerate(refs):
                s.set_buffer("hessian_action_action", guu[b])
                out = riccati_ref.backward_pass(*riccati_ref.from_buffers({k: s.buffer(k) for k in riccati_ref.INPUTS}, T, n, m))
                s.call("backward_pass"); s.call("lagrangian_gradient")
                assert s.stats().potrf_info == out["info"] == (pivot if b < 2 else 0)
                want = riccati_ref.to_buffers(out)
                g = s.buffer("gradient")
                got = dict(K=s.buffer("K"), k=s.buffer("k"), P=s.buffer("P"), p=s.buffer("p"),
                           gradient_state_lagrangian=g[:(T - 1) * n], gradient_action_lagrangian=g[T * n:])
                worst = max(worst, max(_rel(got[k], want[k]) for k in OUT))
        else:
            for b in range(FP.B):
                args = _restatement_linearisation(_synth(model, T), x1[b], ub[b])
                guu = np.stack([args[5].transpose(0, 2, 1).reshape(-1)] * FP.B)     # inject() speaks the handle's layout
                args[5] = FP.inject(guu, T, m, pivot)[b].reshape(T - 1, m, m).transpose(0, 2, 1)
                assert riccati_ref.backward_pass(*args)["info"] == (pivot if b < 2 else 0)
                worst = max(worst, _one_rounding(args, 100 * T + b))
                swap = max(swap, _oracle_factorisation(oracle, args))
    print("%s: %.2e, oracle's factorisation %.2e" % (FP.case_id(case), worst, swap))
    assert swap <= 1e-10, swap
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("nm", sorted(FP.FUSED_SIZES))
def test_the_model_that_fails_by_itself_fails_where_it_should(oracle, nm):
    n, m = nm
    worst, swap = 0.0, 0.0
    for T in FP.FUSED_HORIZONS:
        x1, ub, w = FP.w0_inputs(n, m, T, FP.FUSED_FAILING[1])
        problem = FP.w0_problem(R, n, m, T)
        for b in range(FP.FUSED_B):
            args = _restatement_linearisation(problem, x1[b], ub[b], w[b])
            fails = b in FP.FUSED_FAILING[1]
            # step by step: the pivot that fails is j + 1 (with the garbage value function behind it too)
            out = riccati_ref.backward_pass(*args)
            for t in range(T - 1):
                Quu = args[1][t].T @ out["P"][t + 1] @ args[1][t] + args[5][t]
                assert lapack.dpotrf(np.asfortranarray(Quu), lower=0)[1] == (FP.FUSED_SIZES[nm] + 1 if fails else 0), (T, b, t)
            worst = max(worst, _one_rounding(args, 100 * T + b))
            swap = max(swap, _oracle_factorisation(oracle, args))
    print("w0 model %dx%d: %.2e, oracle's factorisation %.2e" % (n, m, worst, swap))
    assert swap <= 1e-10, swap
    assert worst <= 1e-10, worst
