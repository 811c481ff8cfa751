"""The whole-solve comparison of a device solve with the CPU oracle's, as a function of arrays: it opens no GPU and calls no
solver of its own (what it needs beyond the arrays — the oracle's own spread under a perturbed ū, a rollout — comes in as
callables). tests/test_gpu_parity.py (_whole_solve and the shard tests) asserts through it; tests/test_parity_check.py feeds it
planted faults.

Both sides are dicts of the oracle's solve_batch shape: x [B,T,n], u [B,T-1,m], K [B,T-1,n,m], k [B,T-1,m] and "stats", a dict of
per-instance arrays (iterations, outer_iterations, rollouts, status, objective, max_violation, potrf_info)."""
import numpy as np

FLOW = ("iterations", "outer_iterations", "rollouts", "status")
# at most this fraction of a batch may exceed the bounds as CHAOTIC instances (compare(..., spread=...))
CHAOTIC_ALLOWANCE = 0.02


def same_control_flow(st, rs):
    """Per instance: the device took the oracle's path (iteration, outer-iteration and rollout counts, exit status)."""
    return np.logical_and.reduce([np.asarray(st[f]) == np.asarray(rs[f]) for f in FLOW])


def errors(dev, ref):
    """Per-instance max |Δx|, |Δu| (absolute) and |ΔK|, |Δk| relative to max(max |K|, 1), max(max |k|, 1) of the oracle's instance."""
    B = len(ref["x"])

    def d(f, rel):
        with np.errstate(invalid="ignore"):           # inf - inf where both sides overflowed: NaN, counted as an error
            e = np.abs(np.asarray(dev[f]) - ref[f]).reshape(B, -1).max(1)
        return e / np.maximum(np.abs(ref[f]).reshape(B, -1).max(1), 1.0) if rel else e
    return dict(x=d("x", False), u=d("u", False), K=d("K", True), k=d("k", True))


def chaotic(err, tol, idx, spread, allowance=CHAOTIC_ALLOWANCE, batch=None):
    """The self-perturbation rule for instances `idx` that break a bound (err, tol: per field, err indexed by instance): there may be
    at most allowance x batch of them, and each must be CHAOTIC — the oracle differs from ITSELF, when ū is perturbed by one part in
    1e15, by at least a tenth of what the device differs from it, in every field that breaks its bound. spread(idx) returns that
    self-difference per field (dict of arrays over idx). Returns the per-field spreads for reporting."""
    idx = np.asarray(idx)
    batch = len(next(iter(err.values()))) if batch is None else batch
    assert idx.size <= allowance * batch, "%d instances beyond the bounds, %d allowed as chaotic" % (idx.size, int(allowance * batch))
    if not idx.size:
        return {}
    own = spread(idx)
    for f in tol:
        e = err[f][idx]
        with np.errstate(invalid="ignore"):
            bad = ~(e <= tol[f]) & ~(e <= 10.0 * own[f])      # a NaN is never within a bound, nor chaotic
        assert not bad.any(), ("not chaotic", f, idx[bad], e[bad], own[f][bad])
    return own


def compare(dev, ref, *, min_match, tol, tol_K, tol_k, constraint_tolerance, max_dual_updates, spread=None, step=None, x1=None):
    """Asserts that the device solve `dev` is the oracle's `ref`:
    - control flow identical on >= min_match of the instances;
    - > 99 % of the instances finite in the oracle; where the oracle is not and the control flow is the same, the device is non-finite
      in the same places;
    - on the finite instances with the oracle's control flow: |Δx|, |Δu| <= tol, |ΔK| <= tol_K, |Δk| <= tol_k (errors()), objective
      to 1e-8 and max_violation to 1e-6 relative, the same potrf info — except, with `spread`, chaotic instances (chaotic());
    - on the finite instances whose control flow differs, the reference's own end-to-end property (src/solve.jl:88-129: the outer
      loop stops when max_violation <= constraint_tolerance or after max_dual_updates), x, u, K and k finite wherever the oracle's
      are, and — with `step`, a
      callable (x_t, u_t) -> x_t+1 of the model's dynamics — x the trajectory its own u gives from x1, step by step (one step at a
      time: a whole open-loop rollout of a chaotic instance moves by 1e-4 when ū moves by one part in 1e15).
    Returns dict(frac, differ, loose, dx, du, dK, dk) with the maxima over the instances compared within the bounds."""
    st, rs = dev["stats"], ref["stats"]
    B = len(ref["x"])
    same = same_control_flow(st, rs)
    frac = same.mean()
    assert frac >= min_match, "control flow matched on only %.1f%% of instances" % (100 * frac)
    # instances whose initial open-loop rollout already overflows are NaN in the reference as well:
    # there the two sides must be non-finite in the same places; they are left out of the numeric diffs
    finite = np.isfinite(ref["x"]).reshape(B, -1).all(1) & np.isfinite(ref["u"]).reshape(B, -1).all(1)
    assert finite.mean() > 0.99
    for b in np.nonzero(same & ~finite)[0]:
        assert np.array_equal(np.isfinite(dev["x"][b]), np.isfinite(ref["x"][b])), b
    same_f = same & finite
    err = errors(dev, ref)
    tols = dict(x=tol, u=tol, K=tol_K, k=tol_k)
    over = np.zeros(B, bool)
    for f in tols:
        with np.errstate(invalid="ignore"):
            over |= ~(err[f] <= tols[f])          # NaN where the oracle is finite counts as over
    loose = np.nonzero(same_f & over)[0]
    if spread is None:
        for f in tols:
            assert err[f][same_f].max(initial=0.0) <= tols[f] and not over[same_f].any(), \
                (f, err[f][same_f].max(initial=0.0), tols[f], np.nonzero(same_f & over)[0][:8])
    else:
        chaotic(err, tols, loose, spread, batch=B)
    reg = same_f.copy()
    reg[loose] = False
    assert np.allclose(st["objective"][reg], rs["objective"][reg], rtol=1e-8)
    assert np.allclose(st["max_violation"][reg], rs["max_violation"][reg], rtol=1e-6, atol=1e-10)
    assert (np.asarray(st["potrf_info"]) == rs["potrf_info"])[same].all()
    # instances whose control flow differs still have to satisfy the reference's own end-to-end property
    differ = np.nonzero(~same & finite)[0]
    for b in differ:
        for f in ("x", "u", "K", "k"):
            assert np.isfinite(dev[f][b])[np.isfinite(ref[f][b])].all(), ("non-finite where the oracle is finite", b, f)
        assert st["max_violation"][b] <= constraint_tolerance or st["outer_iterations"][b] == max_dual_updates, \
            ("neither feasible nor out of dual updates", b, st["max_violation"][b], st["outer_iterations"][b])
        if step is not None:
            x, u = np.asarray(dev["x"][b]), np.asarray(dev["u"][b])
            assert np.array_equal(x[0], x1[b]), ("initial state", b)
            for t in range(len(u)):
                xn = np.asarray(step(x[t], u[t]))
                assert np.abs(x[t + 1] - xn).max() <= 1e-9 * max(1.0, np.abs(xn).max()), ("x is not the rollout of u", b, t, x[t + 1], xn)
    mx = {f: err[f][reg].max(initial=0.0) for f in tols}
    return dict(frac=frac, differ=differ, loose=loose, dx=mx["x"], du=mx["u"], dK=mx["K"], dk=mx["k"], err=err, same=same)
