"""ilqr_plan_covariance at model sizes its own GPU test (tests/test_gpu_plancov.py: nx in {3, 4, 12, 32}) does not reach, feedback on,
S = T − 1, against the yardstick tests/plancov_ref.py. Bound: TOL_XU = 1e-10 relative to max(1, max |reference|).

The synth family of the MPC sweep, obtained as tests/test_gpu_closed_loop_sizes.py obtains it (the same modules under the same names,
nothing new to compile), T = 21:

    (1, 1)    the smallest small-form model                       (4, 3)   the largest; B = 70: two waves, the second ragged
    (5, 1)    the first large size, one padded tile               (17, 2)  odd, two tiles (NT = 2, NP = 32, ld = 48)
    (33, 2)   three tiles                                          (64, 8)  NT = 4 and the ld = NP + 16 padding: 141 KB of LDS, the
                                                                            function-attribute branch of the launch

The coupled-dynamics family (tests/coupled_dynamics.py) at its MPC_SIZES (5, 2), (17, 3), (33, 2), T = 11, built as
tests/test_gpu_coupled_dynamics.py builds it: its ∂f/∂u has the state-dependent entries (i, i mod m), so the JAC_VAR_IDX >= nx·nx
range of the patch is at work; and (17, 3) once more through the C-callable route with dense tables, JAC_NVAR = 340 > 256: the
run-time loop of the patch, most of whose entries are ∂f/∂u's. This family is the only cover of the ∂f/∂u patch on the large form.

B = 3 on the large form. P0 = estimator_ref.p_start, q = estimator_ref.q(n)."""
import numpy as np
import pytest

import coupled_dynamics as CD
import estimator_ref as E
import plancov_ref as PC
import policy_ref as P
import test_gpu_closed_loop_sizes as CL
import test_gpu_coupled_dynamics as GC
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU = 1e-10


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in ("ilqr_plan_covariance", "ilqr_plan_covariance_device"):
        assert hasattr(p._ffi.lib(), fn), fn
    return p


def _check(sol, name, xb, ub, K, label):
    B, n = sol.B, sol.nx
    S = sol.T - 1
    Ps, q = E.p_start(B, n), E.q(n)
    out = sol.plan_covariance_(Ps, feedback=True, q=q, full=True)
    sg = out["sigma"]
    assert (out["first_nonfinite"] == -1).all() and np.array_equal(sg, sg.transpose(0, 1, 3, 2))
    assert np.array_equal(out["sdiag"], np.diagonal(sg, axis1=2, axis2=3)) and np.array_equal(out["P"], sg[:, S]) and (out["udiag"] > 0.0).all()
    worst = 0.0
    for b in CL._some(B):
        ref = PC.recursion(name, xb[b], ub[b], K[b], None, Ps[b], S, True, q)
        assert np.isfinite(ref["sigma"]).all()
        worst = max(worst, P.rel(sg[b], ref["sigma"]), P.rel(out["sdiag"][b], ref["sdiag"]), P.rel(out["udiag"][b], ref["udiag"]), P.rel(out["P"][b], ref["P"]))
    # without feedback K is not read and the actions have no variance
    quiet = sol.plan_covariance_(Ps, feedback=False, q=q)
    b = list(CL._some(B))[-1]
    ref = PC.recursion(name, xb[b], ub[b], None, None, Ps[b], S, False, q)
    worst = max(worst, P.rel(quiet["sdiag"][b], ref["sdiag"]), P.rel(quiet["P"][b], ref["P"]))
    assert (quiet["udiag"] == 0.0).all()
    print("plan covariance %s: worst relative error %.2e (bound %.0e)" % (label, worst, TOL_XU))
    assert worst < TOL_XU, (label, worst)


@pytest.mark.parametrize("nm", CL.SIZES, ids=CL.IDS)
def test_plan_covariance_over_the_sizes(pkg, nm):
    n, m = nm
    sol, xb, ub, K = CL._solved(pkg, n, m)
    _check(sol, CL._name(n, m), xb, ub, K, "synth %dx%d" % nm)
    sol.close()


@pytest.mark.parametrize("nm", CD.MPC_SIZES, ids=GC.MPC_IDS)
def test_plan_covariance_on_coupled_dynamics(pkg, nm):
    sol, xb, ub, K, _ = GC._solved_mpc(pkg, nm)
    _check(sol, CD.register_yardstick(*nm), xb, ub, K, "coupled %dx%d" % nm)
    sol.close()


def test_plan_covariance_on_the_dense_c_route(pkg, monkeypatch):
    """(17, 3) through the adapter with dense tables: JAC_NVAR = 340 > 256, the run-time loop of the patch"""
    nm = (17, 3)
    sol, xb, ub, K, _ = GC._solved_mpc(pkg, nm, make=lambda: GC._c_solver(pkg, nm, False, monkeypatch, B=CD.BATCH_MPC))
    _check(sol, CD.register_yardstick(*nm), xb, ub, K, "coupled c-17x3-dense")
    sol.close()
