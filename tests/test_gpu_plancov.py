"""ilqr_plan_covariance on the GPU. T = 11, built-in models car_obs (3 x 2, user parameters), acrobot (4 x 1), synth12 (large form)
and synth32 (32 x 8); B = 3 and 70 (synth32: 3), handles solved as in tests/test_gpu_estimator.py. Yardstick: tests/plancov_ref.py
(complex-step Jacobians in x and u, plain numpy); P0 = estimator_ref.p_start, q = estimator_ref.q(n) or none. The bound TOL_XU = 1e-10
relative to max(1, max |reference|) is the project's own for these kernels (tests/test_plancov_ref.py: the yardstick's two forms agree
within a tenth of it).

1. Against the yardstick: feedback 0 and 1, S in {1, 3, T−1}, q given and NULL; instances (0, 1, 63, 64, 69) at B = 70.
2. Bitwise structure: every Σ_t symmetric, sdiag the diagonal of sigma, P_out == sigma[S]; fewer outputs change no bit of the rest;
   P_out aliased to P0 gives the same bits; without feedback udiag is exactly 0 and a NaN written into K changes nothing.
3. Without feedback and S = k, P agrees within TOL_XU with estimate_predict_(x̂ = x̄_0, P0, steps=k, feedback=False, q).
4. An instance's bits are the same at B = 3 and inside B = 70, and through the host and device forms.
5. It agrees with what the device already does: the sampled covariance of 2 nx closed-loop rollouts per instance
   (rollout_policy(step_size=0, trajectories=True) from x̄_0 ± ε L e_j, P0 = L Lᵀ, q = 0) against sigma and udiag, within
   plancov_ref.FD_BOUND — ten times what the same comparison gives entirely in numpy (plancov_ref's docstring; ε, the measured value
   and the bound are printed).
6. A NaN on one instance's P0 diagonal: first_nonfinite == 0 there, every other instance bit for bit.
7. get_trajectory, get_policy and a following solve_ are bit for bit what they are without the call.
8. A sharded handle [0, 0] equals the single one (host form); the device form is refused there.
9. Each refusal of the contract is refused, and the output arrays are untouched."""
import ctypes as C

import numpy as np
import pytest

import estimator_ref as E
import plancov_ref as PC
import plant_ref as R
import policy_ref as P
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
TOL_XU = 1e-10
T = R.T
MODELS = ["car_obs", "acrobot", "synth12", "synth32"]
FNS = ("ilqr_plan_covariance", "ilqr_plan_covariance_device")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    for fn in FNS:
        assert hasattr(p._ffi.lib(), fn), fn
    return p


def _solved(pkg, name, B, **kw):
    sol = pkg.Solver(model=name, horizon=T, batch=B, options=pkg.Options(verbose=0, **R.SOLVE), **kw)
    x1, ub, w = R.inputs(pkg.workloads, name, B)
    if w is not None:
        sol.set_parameters_(w)
    sol.initialize_rollout_(x1, ub)
    sol.solve_()
    return sol, w


def _some(B):
    return range(B) if B <= 3 else (0, 1, 63, 64, 69)


def _same(a, b, keys=None):
    for key in (keys or a):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


# ----------------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("name", MODELS)
def test_against_the_yardstick(pkg, name):
    worst = 0.0
    for B in R.BATCHES[name]:
        sol, w = _solved(pkg, name, B)
        (xb, ub), (K, _) = sol.get_trajectory(), sol.get_policy()
        n = sol.nx
        Ps = E.p_start(B, n)
        for fb in (True, False):
            for q in (E.q(n), None):
                refs = {b: PC.recursion(name, xb[b], ub[b], K[b], None if w is None else w[b], Ps[b], T - 1, fb, q) for b in _some(B)}
                for S in (1, 3, T - 1):
                    out = sol.plan_covariance_(Ps, steps=S, feedback=fb, q=q, full=True)
                    sg = out["sigma"]
                    assert (out["first_nonfinite"] == -1).all()
                    assert np.array_equal(sg, sg.transpose(0, 1, 3, 2))                                       # 2: symmetric, bit for bit
                    assert np.array_equal(out["sdiag"], np.diagonal(sg, axis1=2, axis2=3)) and np.array_equal(out["P"], sg[:, S])
                    assert np.array_equal(sg[:, 0], np.stack([E.mirror(p) for p in Ps]))
                    assert (out["udiag"] > 0.0).all() if fb else (out["udiag"] == 0.0).all()
                    for b, ref in refs.items():
                        errs = [P.rel(sg[b], ref["sigma"][:S + 1]), P.rel(out["sdiag"][b], ref["sdiag"][:S + 1]), P.rel(out["udiag"][b], ref["udiag"][:S]),
                                P.rel(out["P"][b], ref["sigma"][S])]
                        worst = max(worst, max(errs))
                        assert max(errs) < TOL_XU, (name, B, fb, q is None, S, b, errs)
        sol.close()
    print("plan covariance %s: worst relative error %.2e (bound %.0e)" % (name, worst, TOL_XU))


def _raw(pkg, sol, P0, S, fb, q, want, P_out=None):
    """ilqr_plan_covariance with the outputs named in `want` only -> dict of them (P_out: the caller's array, e.g. P0 itself)"""
    F64, I32 = pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    B, n, m = sol.B, sol.nx, sol.nu
    arr = dict(sdiag=np.empty((B, S + 1, n)), udiag=np.empty((B, S, m)), sigma=np.empty((B, S + 1, n, n)),
               P=np.empty((B, n, n)) if P_out is None else P_out, first_nonfinite=np.empty(B, dtype=np.int32))
    p = lambda key: arr[key].ctypes.data_as(I32 if key == "first_nonfinite" else F64) if key in want else None
    pkg._ffi.check(pkg._ffi.lib().ilqr_plan_covariance(sol._h, S, 1 if fb else 0, None if q is None else q.ctypes.data_as(F64), P0.ctypes.data_as(F64),
                                                       p("sdiag"), p("udiag"), p("sigma"), p("P"), p("first_nonfinite")))
    return {key: arr[key] for key in want}


@pytest.mark.parametrize("name,B", [("car_obs", 70), ("acrobot", 3), ("synth12", 3), ("synth32", 3)])
def test_bitwise_structure(pkg, name, B):
    sol, w = _solved(pkg, name, B)
    n, S = sol.nx, 3
    Ps, q = E.p_start(B, n), E.q(n)
    every = ("sdiag", "udiag", "sigma", "P", "first_nonfinite")
    full = _raw(pkg, sol, Ps, S, True, q, every)
    _same(full, sol.plan_covariance_(Ps, steps=S, feedback=True, q=q, full=True))
    for want in (("sdiag",), ("udiag",), ("sigma",), ("P",), ("first_nonfinite",), ("sdiag", "P"), ("udiag", "sigma", "first_nonfinite")):
        _same(_raw(pkg, sol, Ps, S, True, q, want), full, want)                                               # fewer outputs: no bit of the rest changes
    alias = Ps.copy()
    out = _raw(pkg, sol, alias, S, True, q, ("P", "sdiag"), P_out=alias)                                      # P_out aliased to P0
    assert out["P"] is alias and np.array_equal(alias, full["P"]) and np.array_equal(out["sdiag"], full["sdiag"])
    junk = Ps + np.triu(np.full((n, n), np.nan), 1)[None]                                                     # the upper triangle of P0 is not read
    _same(_raw(pkg, sol, junk, S, True, q, every), full)
    # without feedback: udiag is exactly 0, and K is not read
    quiet = sol.plan_covariance_(Ps, steps=S, feedback=False, q=q, full=True)
    assert (quiet["udiag"] == 0.0).all() and not np.array_equal(quiet["P"], full["P"])
    K = sol.buffer("K").copy()
    sol.set_buffer("K", np.full_like(K, np.nan))
    _same(sol.plan_covariance_(Ps, steps=S, feedback=False, q=q, full=True), quiet)
    loud = sol.plan_covariance_(Ps, steps=S, feedback=True, q=q)
    assert (loud["first_nonfinite"] == 1).all() and np.array_equal(loud["sdiag"][:, 0], full["sdiag"][:, 0])  # with feedback the NaN arrives at Σ_1
    sol.set_buffer("K", K)
    _same(sol.plan_covariance_(Ps, steps=S, feedback=True, q=q, full=True), full)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name,B", [("car_obs", 70), ("acrobot", 70), ("synth12", 3), ("synth32", 3)])
def test_without_feedback_it_is_the_filters_time_update_at_the_nominal_state(pkg, name, B):
    sol, w = _solved(pkg, name, B)
    n = sol.nx
    xb = sol.get_trajectory()[0]
    Ps, q = E.p_start(B, n), E.q(n)
    for k in (1, 3):
        out = sol.plan_covariance_(Ps, steps=k, feedback=False, q=q)
        _, P1 = sol.estimate_predict_(xb[:, 0], Ps, steps=k, feedback=False, q=q)
        err = max(P.rel(out["P"][b], P1[b]) for b in range(B))
        print("plan covariance %s k=%d against estimate_predict_: %.2e" % (name, k, err))
        assert err < TOL_XU, (name, k, err)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["car_obs", "acrobot", "synth12"])
def test_an_instance_does_not_depend_on_its_batch_or_on_the_form(pkg, name):
    import torch
    big, w = _solved(pkg, name, 70)
    small, _ = _solved(pkg, name, 3)
    n, m, S = big.nx, big.nu, T - 1
    for b in range(3):                             # the two handles hold the same plans for the first three instances
        assert np.array_equal(big.get_trajectory()[1][b], small.get_trajectory()[1][b])
    Ps, q = E.p_start(70, n), E.q(n)
    o70 = big.plan_covariance_(Ps, feedback=True, q=q, full=True)
    o3 = small.plan_covariance_(Ps[:3], feedback=True, q=q, full=True)
    for key in o3:
        assert np.array_equal(o70[key][:3], o3[key]), key
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    with torch.cuda.stream(torch.cuda.ExternalStream(big.stream_ptr())):
        dP = torch.from_numpy(Ps.copy()).to(dev)
        dsd, dud, dsg = torch.zeros(70, S + 1, n, **f64), torch.zeros(70, S, m, **f64), torch.zeros(70, S + 1, n, n, **f64)
        dnf = torch.zeros(70, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    big.plan_covariance_device_(dP.data_ptr(), feedback=True, q=q, d_sdiag_ptr=dsd.data_ptr(), d_udiag_ptr=dud.data_ptr(), d_sigma_ptr=dsg.data_ptr(),
                                d_P_out_ptr=dP.data_ptr(), d_first_nonfinite_ptr=dnf.data_ptr())                # P_out aliased to P0 on the device
    big.synchronize()
    for key, t in (("sdiag", dsd), ("udiag", dud), ("sigma", dsg), ("P", dP), ("first_nonfinite", dnf)):
        assert np.array_equal(t.cpu().numpy(), o70[key]), key
    big.close(); small.close()


# ----------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", ["car_obs", "acrobot", "synth12"])
def test_it_agrees_with_sampled_closed_loop_rollouts(pkg, name):
    B = 3
    sol, w = _solved(pkg, name, B)
    n = sol.nx
    xb = sol.get_trajectory()[0]
    Ps = E.p_start(B, n)
    out = sol.plan_covariance_(Ps, feedback=True, q=None, full=True)
    x1 = np.stack([PC.sample_starts(xb[b, 0], Ps[b]) for b in range(B)])
    roll = sol.rollout_policy(x1, step_size=0.0, trajectories=True)                   # (under the handle's own θ)
    assert (roll["first_nonfinite"] == -1).all()
    worst = 0.0
    for b in range(B):
        Sh, Uh = PC.sampled(roll["x"][b], roll["u"][b])
        worst = max(worst, PC.rel_cov(Sh, out["sigma"][b]), PC.rel_cov(Uh, out["udiag"][b]))
    print("plan covariance %s: sampled on the device against propagated: eps %.0e, %.2e (in numpy %.1e, bound %.1e)"
          % (name, PC.FD_EPS, worst, PC.FD_MEASURED, PC.FD_BOUND))
    assert worst <= PC.FD_BOUND, (name, worst)
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("name,B", [("car_obs", 70), ("acrobot", 70), ("synth12", 3), ("synth32", 3)])
def test_a_nan_in_one_instance(pkg, name, B):
    sol, w = _solved(pkg, name, B)
    n = sol.nx
    Ps, q = E.p_start(B, n), E.q(n)
    clean = sol.plan_covariance_(Ps, steps=3, feedback=True, q=q, full=True)
    bad_b = B - 2
    Pn = Ps.copy(); Pn[bad_b, n - 1, n - 1] = np.nan
    out = sol.plan_covariance_(Pn, steps=3, feedback=True, q=q, full=True)
    others = np.arange(B) != bad_b
    assert out["first_nonfinite"][bad_b] == 0 and (out["first_nonfinite"][others] == -1).all()
    for key in clean:
        assert np.array_equal(out[key][others], clean[key][others]), key
    sol.close()


# ----------------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["acrobot", "synth12"])
def test_the_call_reads_the_handle(pkg, name):
    B = 3
    a, w = _solved(pkg, name, B)
    b, _ = _solved(pkg, name, B)
    # the handle's own arrays before and after the call (the scalars too: they hold clock readings, which differ between two handles)
    state = lambda s: s.get_trajectory() + s.get_policy() + (s.buffer("_scalars"),)
    before = state(a)
    a.plan_covariance_(E.p_start(B, a.nx), feedback=True, q=E.q(a.nx), full=True)
    a.plan_covariance_(E.p_start(B, a.nx), steps=2, feedback=False)
    for u, v in zip(state(a), before):
        assert np.array_equal(u, v, equal_nan=True)
    # and against a handle that never made the call, now and after a following solve
    plan = lambda s: s.get_trajectory() + s.get_policy()
    for again in (False, True):
        if again:
            a.solve_(); b.solve_()
        for u, v in zip(plan(a), plan(b)):
            assert np.array_equal(u, v, equal_nan=True)
        sa, sb = a.stats(), b.stats()
        for key in sa:
            assert np.array_equal(sa[key], sb[key], equal_nan=True), key
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------- 8
def test_sharded_handle_equals_the_single_one(pkg):
    B = 7
    one, w = _solved(pkg, "car_obs", B)
    two, _ = _solved(pkg, "car_obs", B, devices=[0, 0])
    Ps, q = E.p_start(B, one.nx), E.q(one.nx)
    o1, o2 = (s.plan_covariance_(Ps, steps=5, feedback=True, q=q, full=True) for s in (one, two))
    _same(o1, o2)
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        two.plan_covariance_device_(1, steps=1, d_P_out_ptr=1)
    one.close(); two.close()


# ----------------------------------------------------------------------------------------------------------------------- 9
def test_refusals(pkg):
    L, F64, I32 = pkg._ffi.lib(), pkg._ffi.c_double_p, C.POINTER(C.c_int32)
    B = 3
    sol, _ = _solved(pkg, "acrobot", B)
    fresh = pkg.Solver(model="acrobot", horizon=T, batch=B, options=pkg.Options(verbose=0))        # holds no policy yet
    n, m = sol.nx, sol.nu
    Ps = E.p_start(B, n)
    MARK = -12345.0
    sd, ud, Po, nf = np.full((B, T, n), MARK), np.full((B, T - 1, m), MARK), np.full((B, n, n), MARK), np.full(B, -77, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(I32 if a.dtype == np.int32 else F64)
    q_ok = E.q(n)

    def call(fn, h=None, steps=3, fb=1, q=q_ok, P0=Ps, outs=True):
        h = sol._h if h is None else h
        o = (p(sd), p(ud), None, p(Po), p(nf)) if outs else (None,) * 5
        if fn.endswith("_device"):             # refused before anything is dereferenced: the host arrays stand in for device arrays
            o = tuple(None if v is None else C.cast(v, C.c_void_p) for v in o)
            return getattr(L, fn)(h, steps, fb, p(q), None if P0 is None else C.c_void_p(P0.ctypes.data), *o)
        return getattr(L, fn)(h, steps, fb, p(q), p(P0), *o)

    neg, nan, inf = q_ok.copy(), q_ok.copy(), q_ok.copy()
    neg[n - 1], nan[1], inf[0] = -1.0e-9, np.nan, np.inf
    INVALID = -1
    for fn in FNS:
        cases = dict(steps_0=dict(steps=0), steps_T=dict(steps=T), steps_neg=dict(steps=-1), feedback_2=dict(fb=2), feedback_neg=dict(fb=-1),
                     null_P0=dict(P0=None), no_output=dict(outs=False), q_negative=dict(q=neg), q_nan=dict(q=nan), q_inf=dict(q=inf),
                     no_policy=dict(h=fresh._h), null_handle=dict(h=C.c_void_p(0)))
        for label, kw in cases.items():
            rc = call(fn, **kw)
            assert rc == INVALID and L.ilqr_last_error(), (fn, label, rc)
    assert call(FNS[0], h=fresh._h, fb=0) == 0                                                     # without feedback no policy is needed
    sd[:], ud[:], Po[:], nf[:] = MARK, MARK, MARK, -77
    for label, kw in dict(steps_0=dict(steps=0), feedback_2=dict(fb=2), q_negative=dict(q=neg), no_policy=dict(h=fresh._h)).items():
        assert call(FNS[0], **kw) == INVALID, label
        sol.synchronize()
        assert (sd == MARK).all() and (ud == MARK).all() and (Po == MARK).all() and (nf == -77).all(), label      # nothing was launched
    with pytest.raises(pkg._ffi.IlqrError, match="no policy"):
        fresh.plan_covariance_(Ps)
    with pytest.raises(pkg._ffi.IlqrError, match="steps"):
        sol.plan_covariance_(Ps, steps=T)
    assert (sol.plan_covariance_(Ps)["first_nonfinite"] == -1).all()
    sol.close(); fresh.close()
