"""The yardstick of the warm-start tests (tests/test_duals_ref.py, tests/test_gpu_warm_duals.py): what ilqr_shift_duals leaves in
constraint_dual / constraint_penalty, in numpy, and what ilqr_solve_warm computes, composed from the CPU oracle's exported steps.

With k = steps, N = T − 1, ncs / nct stage / terminal rows and C = N·ncs + nct doubles per instance (stage row t at t·ncs, the
terminal rows at N·ncs):

    λ'_t = λ_{t+k}  (t < N−k),  then λ_{N−1} ("hold") or 0 ("zero");  terminal rows stay
    ρ'   "keep":  as λ, the tail under "zero" gets ρ0;   "reset":  ρ0 everywhere

A warm solve is constrained_ilqr_solve! (src/solve.jl:88-129) with lines :95-103 (λ ← 0, ρ ← ρ0) skipped: not a reference behaviour.
"""
import numpy as np

SMALL = dict(model="car_obs", config="car_obs", B=5)          # the inputs tests/test_duals_ref.py qualifies (see there)


def shift_duals(lam, rho, ncs, nct, k, tail="hold", penalty="keep", rho0=1.0):
    """(λ', ρ') of one instance or of a batch ([..., C]); pure copies, so signs and bits are kept."""
    lam, rho = np.asarray(lam, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    C = lam.shape[-1]
    N = (C - nct) // ncs if ncs > 0 else None
    assert tail in ("hold", "zero") and penalty in ("keep", "reset") and k >= 0
    out = []
    for v, fill in ((lam, 0.0), (rho, rho0)):
        o = v.copy()
        if ncs > 0 and k > 0:
            assert k <= N
            s = v[..., :N * ncs].reshape(v.shape[:-1] + (N, ncs))
            d = np.empty_like(s)
            d[..., :N - k, :] = s[..., k:, :]
            d[..., N - k:, :] = s[..., N - 1:N, :] if tail == "hold" else fill
            o[..., :N * ncs] = d.reshape(v.shape[:-1] + (N * ncs,))
        out.append(o)
    if penalty == "reset":
        out[1] = np.full_like(rho, rho0)
    return out[0], out[1]


def shift_trajectory(xb, ub, w, k=1):
    """what shift_horizon_(k) (open loop, hold, no w_tail) installs: x1' = x̄_k, u' = ū_{t+k} then ū_{N−1}, w' = w_{t+k} then w_{T−1}"""
    import shift_ref
    return shift_ref.shifted_inputs(xb, ub, w, k)


def composed_solve(O, model, T, x1, ub, lam=None, rho=None, w=None, options=None):
    """One instance on a fresh oracle.Solver (whose scalars are what reset!(data), src/solve.jl:93, leaves): initialize, write λ / ρ
    (None: λ = 0, ρ = ρ0 — the cold values), then the loop of src/solve.jl:105-122 from the oracle's exported steps with the outer
    iterations counted here. Returns x, u, K (as get_policy lays it out), k, lam, rho and the statistics."""
    opt = options if options is not None else O.default_options(verbose=0)
    pr = O.Problem(model, T)
    xb = pr.rollout(x1, ub, w)
    s = O.Solver(pr, opt, w=w)
    s.initialize_controls(ub); s.initialize_states(xb)
    C = s.buffer("constraint_dual").size
    s.set_buffer("constraint_dual", np.zeros(C) if lam is None else lam)
    s.set_buffer("constraint_penalty", np.full(C, opt.initial_constraint_penalty) if rho is None else rho)
    outer = 0
    for i in range(1, opt.max_dual_updates + 1):                      # (:105)
        outer = i
        s.call("ilqr_solve")                                          # (:109)
        s.call("cost_bang", 0)                                        # (:113)
        if s.stats().max_violation <= opt.constraint_tolerance:       # (:117)
            break
        s.call("augmented_lagrangian_update")                         # (:120-122)
    st = s.stats()
    stats = {f: getattr(st, f) for f, _ in O.OrcStats._fields_}
    stats["outer_iterations"] = outer
    n, m = pr.nx, pr.nu
    x, u = s.get_trajectory()
    return dict(x=x, u=u, K=s.buffer("K").reshape(T - 1, n, m), k=s.buffer("k").reshape(T - 1, m),
                lam=s.buffer("constraint_dual"), rho=s.buffer("constraint_penalty"), stats=stats)


def composed_batch(O, model, T, x1, ub, lam=None, rho=None, w=None, options=None):
    """composed_solve over a batch, stacked as oracle.solve_batch stacks its results"""
    B = len(x1)
    rs = [composed_solve(O, model, T, x1[b], ub[b], None if lam is None else lam[b], None if rho is None else rho[b],
                         None if w is None else w[b], options) for b in range(B)]
    out = {f: np.stack([r[f] for r in rs]) for f in ("x", "u", "K", "k", "lam", "rho")}
    out["stats"] = {f: np.array([r["stats"][f] for r in rs]) for f in rs[0]["stats"]}
    return out


_CASE = {}


def small_case(pkg, O):
    """The shared inputs of the warm-solve tests, computed once: SMALL's batch solved cold on the oracle (composed loop), its
    trajectory and parameters shifted by one period, its duals shifted with hold / keep; then the cold and the warm re-solve from
    the shifted trajectory. Nothing in the returned dict may be modified."""
    if _CASE:
        return _CASE
    cfg, B = SMALL["config"], SMALL["B"]
    model, T, x1, ub = pkg.workloads.make_inputs(cfg, B)
    w = pkg.workloads.make_parameters(cfg, B)
    opt = O.default_options(verbose=0)
    first = composed_batch(O, model, T, x1, ub, w=w, options=opt)
    ncs, nct = 5, 4                                                    # car_obs: 5 stage rows, 4 terminal rows
    assert first["lam"].shape[1] == (T - 1) * ncs + nct
    sh = [shift_trajectory(first["x"][b], first["u"][b], w[b], 1) for b in range(B)]
    x1s, ubs, ws = (np.stack([s[i] for s in sh]) for i in range(3))
    lam, rho = shift_duals(first["lam"], first["rho"], ncs, nct, 1, "hold", "keep", opt.initial_constraint_penalty)
    _CASE.update(model=model, T=T, B=B, x1=x1, ub=ub, w=w, ncs=ncs, nct=nct, options=opt, first=first, x1s=x1s, ubs=ubs, ws=ws,
                 lam=lam, rho=rho,
                 cold=composed_batch(O, model, T, x1s, ubs, w=ws, options=opt),
                 warm=composed_batch(O, model, T, x1s, ubs, lam, rho, w=ws, options=opt))
    return _CASE
