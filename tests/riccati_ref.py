"""The yardstick of tests/test_gpu_failed_pivot.py (TEST INFRASTRUCTURE): backward_pass! (src/backward_pass.jl:1-91) and
lagrangian_gradient! (src/solve.jl:67-83) over plain arrays, with the REAL LAPACK (scipy's dpotrf / dpotrs, return code ignored as in
the reference). The recursion is not restated here: it is tests/golden/reference_restatement.py's Solver.backward_pass_bang /
lagrangian_gradient_bang, run on a solver whose linearisation lists have been overwritten — so the check needs no twin of the
model, only the arrays a handle holds after its `gradients` stage.

Arrays here are numpy row-major [t][row][col]; the handle's (and the oracle's) buffers are column-major blocks, i.e. the transposes:
from_buffers / to_buffers convert (K[t] is nu x nx here, [t][nx][nu] on the device).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import reference_restatement as R  # noqa: E402

INPUTS = ("jacobian_state", "jacobian_action", "gradient_state", "gradient_action",
          "hessian_state_state", "hessian_action_action", "hessian_action_state")


def backward_pass(fx, fu, gx, gu, gxx, guu, gux, lapack=None):
    """fx [T-1, n, n], fu [T-1, n, m], gx [T, n], gu [T-1, m], gxx [T, n, n], guu [T-1, m, m], gux [T-1, m, n] ->
    dict(K [T-1, m, n], k [T-1, m], P [T, n, n], p [T, n], info (the first non-zero potrf return code of the pass, taken backwards),
    Lx [T-1, n], Lu [T-1, m] (the Lagrangian gradient's state and action parts)).
    lapack: an object with scipy.linalg.lapack's dpotrf / dpotrs to run the same recursion with, in place of the real one."""
    fx, fu, gx, gu, gxx, guu, gux = [np.asarray(a, dtype=np.float64) for a in (fx, fu, gx, gu, gxx, guu, gux)]
    H, n, m = gx.shape[0], gx.shape[1], gu.shape[1]
    assert fx.shape == (H - 1, n, n) and fu.shape == (H - 1, n, m) and gu.shape == (H - 1, m) and gxx.shape == (H, n, n)
    assert guu.shape == (H - 1, m, m) and gux.shape == (H - 1, m, n)
    stub = SimpleNamespace(num_state=n, num_next_state=n, num_action=m, num_parameter=0)
    s = R.Solver([stub] * (H - 1), [None] * H)
    for name, src in (("fx", fx), ("fu", fu), ("gx", gx), ("gu", gu), ("gxx", gxx), ("guu", guu), ("gux", gux)):
        for dst, a in zip(getattr(s, name), src):
            dst[...] = a
    real = R.lapack
    try:
        if lapack is not None:
            R.lapack = lapack
        with np.errstate(all="ignore"):                 # NaN / Inf inputs are cases, not errors
            s.backward_pass_bang()
            s.lagrangian_gradient_bang()
    finally:
        R.lapack = real
    g = s.gradient
    return dict(K=np.stack(s.K), k=np.stack(s.k), P=np.stack(s.P), p=np.stack(s.p), info=s.potrf_info,
                Lx=np.stack([g[i] for i in s.indices_state[:H - 1]]), Lu=np.stack([g[i] for i in s.indices_action]))


def from_buffers(buf, T, n, m):
    """One instance's flat buffers (name -> array, names as INPUTS) -> the arguments of backward_pass."""
    mat = lambda name, steps, cols, rows: np.asarray(buf[name], dtype=np.float64).reshape(steps, cols, rows).transpose(0, 2, 1)
    vec = lambda name, steps, rows: np.asarray(buf[name], dtype=np.float64).reshape(steps, rows)
    return (mat("jacobian_state", T - 1, n, n), mat("jacobian_action", T - 1, m, n), vec("gradient_state", T, n),
            vec("gradient_action", T - 1, m), mat("hessian_state_state", T, n, n), mat("hessian_action_action", T - 1, m, m),
            mat("hessian_action_state", T - 1, n, m))


def to_buffers(out):
    """backward_pass's result in the layout of the handle's buffers: K [T-1][n][m], P [T][n][n] column-major blocks, flat."""
    return dict(K=out["K"].transpose(0, 2, 1).ravel(), k=out["k"].ravel(), P=out["P"].transpose(0, 2, 1).ravel(), p=out["p"].ravel(),
                gradient_state_lagrangian=out["Lx"].ravel(), gradient_action_lagrangian=out["Lu"].ravel())


def of_handle(sol, buffers=None):
    """riccati_ref on every instance of a handle, from the handle's own buffers as they stand: a list of (to_buffers dict, info)."""
    buffers = buffers if buffers is not None else {name: sol.buffer(name) for name in INPUTS}
    res = []
    for b in range(sol.B):
        out = backward_pass(*from_buffers({k: v[b] for k, v in buffers.items()}, sol.T, sol.nx, sol.nu))
        res.append((to_buffers(out), out["info"]))
    return res
