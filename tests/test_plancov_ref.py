"""The yardstick of the plan covariance (tests/plancov_ref.py) without a GPU, on the inputs of tests/test_gpu_plancov.py:

  1. the complex-step action Jacobian agrees with a central difference of the real callables on car_obs, acrobot, synth12 and the
     coupled-dynamics family (whose ∂f/∂u depends on the state);
  2. form (a), the recursion, and form (b), transition matrices with the action variances through scipy's eigenpairs of Σ_t, agree
     within a tenth of TOL_XU = 1e-10 relative to max(1, max |reference|) — so the GPU bound TOL_XU is an honest one — with and without
     feedback and process noise; every Σ_t is symmetric and positive semi-definite;
  3. the sampled covariance of 2 n nonlinear closed-loop rollouts at ε = FD_EPS agrees with form (a) within FD_MEASURED <= 1e-6: the
     measurement the bound of the GPU test (FD_BOUND = 10 · FD_MEASURED) comes from;
  4. the header declares both entry points, _ffi.SYMBOLS carries them with the header's types, Julia binds them, the Solver has the
     two methods and the kernels are instantiated per model module.

The plans have no solve behind them: x̄ is the open-loop rollout of the workload's ū, K the LQR gains of its own linearisation."""
import importlib.util
import os
import re

import numpy as np
import pytest

import coupled_dynamics as CD
import estimator_ref as E
import plancov_ref as PC
import plant_ref as R
import policy_ref as P
import test_julia_binding_static as S
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_XU = 1e-10
FNS = ["ilqr_plan_covariance", "ilqr_plan_covariance_device"]
MODELS = ["car_obs", "acrobot", "synth12"]
_PLANS = {}


def _plans(name, B=3):
    """(x̄ [B, T, n], ū, K, θ or None) of a built-in model; computed once and left unchanged"""
    if name not in _PLANS:
        x1, ub, w = R.inputs(load_package().workloads, name, B)
        xb = np.stack([PC.nominal(name, x1[b], ub[b], None if w is None else w[b]) for b in range(B)])
        K = np.stack([PC.lqr_gains(name, xb[b], ub[b], None if w is None else w[b]) for b in range(B)])
        _PLANS[name] = (xb, ub, K, w)
    return _PLANS[name]


def _central(f, x, u, w, h=1e-6):
    return np.stack([(np.asarray(f(x, u + h * e, w, 0)) - np.asarray(f(x, u - h * e, w, 0))) / (2 * h) for e in np.eye(len(u))], axis=1)


@pytest.mark.parametrize("name", MODELS)
def test_action_jacobian_against_a_central_difference(name):
    xb, ub, _, w = _plans(name)
    f = R.dynamics(name)
    for b in range(xb.shape[0]):
        wi = np.zeros(0) if w is None else w[b, 0]
        Bm = PC.action_jacobian(name, xb[b, 1], ub[b, 1], wi)
        D = _central(f, xb[b, 1], ub[b, 1], wi)
        assert Bm.shape == D.shape and np.abs(Bm).max() > 0 and np.abs(Bm - D).max() < 1e-8, (name, b, np.abs(Bm - D).max())


@pytest.mark.parametrize("nm", CD.MPC_SIZES, ids=["%dx%d" % nm for nm in CD.MPC_SIZES])
def test_action_jacobian_of_the_coupled_family(nm):
    n, m = nm
    name = CD.register_yardstick(n, m)
    x1, ub = CD.inputs(n, m, CD.BATCH_MPC)
    f = R.dynamics(name)
    for b in range(CD.BATCH_MPC):
        Bm, D = PC.action_jacobian(name, x1[b], ub[b, 0], np.zeros(0)), _central(f, x1[b], ub[b, 0], np.zeros(0))
        assert np.abs(Bm - D).max() < 1e-8, (nm, b)
        other = PC.action_jacobian(name, x1[b] + 0.1, ub[b, 0], np.zeros(0))
        moved = {(i, j) for i, j in zip(*np.nonzero(other != Bm))}
        assert moved == CD.structure(n, m)[1], nm              # the state-dependent entries of ∂f/∂u are the family's


@pytest.mark.parametrize("name", MODELS)
def test_the_two_forms_agree_and_sigma_stays_psd(name):
    xb, ub, K, w = _plans(name)
    B, n = xb.shape[0], xb.shape[2]
    Ps = E.p_start(B, n)
    worst = 0.0
    for fb in (True, False):
        for q in (E.q(n), None):
            for b in range(B):
                wb = None if w is None else w[b]
                a = PC.recursion(name, xb[b], ub[b], K[b], wb, Ps[b], R.T - 1, fb, q)
                c = PC.transition_form(name, xb[b], ub[b], K[b], wb, Ps[b], R.T - 1, fb, q)
                assert a["first_nonfinite"] == -1 and np.array_equal(a["sdiag"][0], np.diag(Ps[b])) and np.array_equal(a["P"], a["sigma"][-1])
                d = max(P.rel(a[key], c[key]) for key in ("sigma", "sdiag", "udiag"))
                worst = max(worst, d)
                assert d <= 0.1 * TOL_XU, (name, fb, b, d)
                assert (a["udiag"] > 0.0).all() if fb else (a["udiag"] == 0.0).all()
                for St in a["sigma"]:
                    ev = np.linalg.eigvalsh(St)
                    assert np.array_equal(St, St.T) and ev[0] >= -1e-12 * ev[-1], (name, fb, b)
    print("plan covariance %s: the two forms differ by %.2e at most (bound %.1e)" % (name, worst, 0.1 * TOL_XU))


def test_only_the_lower_triangle_of_p0_is_read():
    xb, ub, K, w = _plans("acrobot")
    P0 = E.p_start(3, 4)[0]
    junk = P0 + np.triu(np.full((4, 4), np.nan), 1)
    a, c = (PC.recursion("acrobot", xb[0], ub[0], K[0], None, p, 3) for p in (P0, junk))
    assert np.array_equal(a["sigma"], c["sigma"])
    bad = P0.copy(); bad[2, 2] = np.nan
    assert PC.recursion("acrobot", xb[0], ub[0], K[0], None, bad, 3)["first_nonfinite"] == 0


@pytest.mark.parametrize("name", MODELS)
def test_sampled_covariance_against_the_recursion(name):
    """the measurement behind FD_BOUND: nonlinear closed-loop rollouts of x̄_0 ± ε L e_j against form (a), q = 0"""
    xb, ub, K, w = _plans(name)
    B, n = xb.shape[0], xb.shape[2]
    Ps = E.p_start(B, n)
    worst = 0.0
    for b in range(B):
        es, eu = PC.sampled_against_recursion(name, xb[b], ub[b], K[b], None if w is None else w[b], Ps[b])
        worst = max(worst, es, eu)
    print("plan covariance %s: sampled against propagated at eps = %.0e: %.2e (FD_MEASURED %.1e, FD_BOUND %.1e)" % (name, PC.FD_EPS, worst, PC.FD_MEASURED, PC.FD_BOUND))
    assert worst <= PC.FD_MEASURED <= 1e-6 and PC.FD_BOUND == 10.0 * PC.FD_MEASURED, (name, worst)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_symbols_are_declared_mirrored_and_bound():
    hdr = S.strip_comments(open(os.path.join(ROOT, "include", "ilqr_hip.h")).read())
    spec = importlib.util.spec_from_file_location("ilqr_ffi_plancov", os.path.join(ROOT, "iterativelqr.jl_amd", "_ffi.py"))
    ffi = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ffi)
    protos = S.parse_header()[1]
    jl = open(S.JULIA).read()
    for name in FNS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in ffi.SYMBOLS and len(ffi.SYMBOLS[name][1]) == len(protos[name][1]), name
        assert ":" + name in jl, name
    assert protos["ilqr_plan_covariance"] == ("i32", ["ptr:void", "i32", "i32"] + ["ptr:f64"] * 6 + ["ptr:i32"])
    assert protos["ilqr_plan_covariance_device"] == protos["ilqr_plan_covariance"]
    full = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for said in ("actuator limits", "non-diagonal Q", "measurement updates along the horizon", "back-offs", "ilqr_mpc_run_*"):
        assert said in full, said
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    pcv = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device_plancov.hpp")).read()
    assert "&launch_plan_covariance<M>" in dev and '#include "ilqr_device_plancov.hpp"' in dev
    assert "static_assert(sizeof(PlanCovArgs) <= 4096" in pcv and "__launch_bounds__(64) void plan_covariance_large_kernel" in pcv
    api = open(os.path.join(ROOT, "iterativelqr.jl_amd", "api.py")).read()
    assert "def plan_covariance_(self, P0, steps=None, feedback=True, q=None, full=False)" in api and "def plan_covariance_device_(" in api
