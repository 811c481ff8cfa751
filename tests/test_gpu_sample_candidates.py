"""ilqr_sample_rollout_candidates on the GPU. The yardstick of the scores and of the installation is the library's own path over
materialised candidates (ilqr_initialize_rollout_candidates, itself checked against the CPU oracle in tests/test_gpu_candidates.py):
the candidates as drawn are exported, fed to that path on a second handle, and everything must be equal BIT FOR BIT. The noise is
checked against the host twin ilqr_candidate_noise (itself against numpy in tests/test_sample_candidates_abi.py), the blend against
numpy on the device's own scores (tests/sample_ref.py).

Bounds, fixed before the kernels ran. Noise: |(u_out − base) / sigma_j − candidate_noise| <= 1e-13 with a base of zeros (no
base-rounding term): |z| <= 8.7, the integers and the cosine's argument are the same IEEE operations on both sides, a few ulp each for
log, sqrt and cos make at most about 16 ulp of 8.7 = 3e-14. Blend: weights against numpy exp on the device's scores <= 1e-11, the
installed ū against the numpy sum in ascending s over u_out and those weights <= 1e-11 · max(1, |u|): about S · 4 ulp = 1e-13 at
S = 70, with a margin of 100."""
import os
import subprocess

import numpy as np
import pytest

import candidates_ref as R
import sample_ref as SR
from ilqr_amd_loader import load_package

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261019
TOL_NOISE, TOL_BLEND = 1e-13, 1e-11
SCORES = ("cost", "max_violation", "first_nonfinite", "chosen")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if p._ffi.lib().ilqr_device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on a GPU box")
    assert hasattr(p._ffi.lib(), "ilqr_sample_rollout_candidates"), "the library has no ilqr_sample_rollout_candidates"
    return p


def _inputs(pkg, name, B, T=None):
    """(model, T, x1 [B, n], base [B, T-1, m], w or None, sigma [m]) of the case; T: a shorter horizon of the same workload"""
    cfg, T_, size = R.CASES[name]
    model, T0, x1, ub = pkg.workloads.make_inputs(cfg, B)
    assert T0 == T_
    w = pkg.workloads.make_parameters(cfg, B) if name == "car_obs" else None
    if T is not None:
        ub, T_ = np.ascontiguousarray(ub[:, :T - 1]), T
        w = None if w is None else np.ascontiguousarray(w[:, :T])
    return model, T_, x1, ub, w, np.full(ub.shape[2], size)


def _handle(pkg, name, model, T, B, w=None, **kw):
    opts = pkg.Options(verbose=0, **pkg.workloads.CONFIG_OPTIONS.get(R.CASES[name][0], {}))
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=opts, **kw)
    if w is not None:
        sol.set_parameters_(w)
    return sol


def _state(sol):
    return sol.buffer("nominal_states"), sol.buffer("nominal_actions"), sol.buffer("_scalars")


def _solved(sol):
    st = sol.stats()
    return sol.get_trajectory() + sol.get_policy() + tuple(st[k] for k in sorted(st))


def _eq(p, q):
    return len(p) == len(q) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(p, q))


def _same(a, b, keys=None):
    keys = sorted(a) if keys is None else keys
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_equals_the_path_over_materialised_candidates_bitwise(pkg, name):
    """S = 70: two waves, the second ragged; T − 1 is no multiple of 8: the last tile is ragged; synth12: the large path."""
    B, S = (3, 70) if name != "synth12" else (2, 9)
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    assert (T - 1) % 8 != 0
    a, b = _handle(pkg, name, model, T, B, w), _handle(pkg, name, model, T, B, w)
    out = a.sample_rollout_candidates_(sigma, S, seed=SEED, x1=x1, base_u=base, return_candidates=True)
    u = out["u"]
    assert np.array_equal(u[:, 0], base) and (u[:, 1:] != base[:, None]).any()
    ref = b.initialize_rollout_candidates_(x1, u)
    assert _same(out, ref, SCORES), {k: np.abs(out[k].astype(float) - ref[k]).max() for k in SCORES}
    assert (out["chosen"] >= 0).all() and np.isfinite(out["cost"]).any()
    pick = np.zeros((B, S))
    pick[np.arange(B), out["chosen"]] = 1.0
    assert np.array_equal(out["weights"], pick)
    assert _eq(_state(a), _state(b))
    assert np.array_equal(a.buffer("nominal_actions").reshape(B, T - 1, -1), u[np.arange(B), out["chosen"]])
    a.solve_(); b.solve_()
    first = _solved(a)
    assert _eq(first, _solved(b))
    a.reset_(); a.initialize_rollout_resident_(); a.solve_()          # the resident inputs replay the installed guess
    assert _eq(first, _solved(a))
    a.close(); b.close()


@pytest.mark.parametrize("name", ["car_obs", "synth12"])
def test_the_noise_is_the_host_twins(pkg, name):
    B, S = (3, 70) if name != "synth12" else (2, 9)
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    sigma = sigma * (1.0 + np.arange(sigma.size))                     # a different size per component
    sol = _handle(pkg, name, model, T, B, w)
    zero = np.zeros_like(base)
    u = sol.sample_rollout_candidates_(sigma, S, seed=SEED, x1=x1, base_u=zero, return_candidates=True)["u"]
    assert np.array_equal(u[:, 0], zero)
    z = pkg.candidate_noise(SEED, B, S, T - 1, sigma.size)
    err = np.abs(u[:, 1:] / sigma - z[:, 1:]).max()
    print("device noise against the host twin (%s): %.2e" % (name, err))
    assert err <= TOL_NOISE, err
    sol.close()


@pytest.mark.parametrize("name", ["acrobot", "car_obs", "synth12"])
def test_candidates_are_independent_and_calls_repeat(pkg, name):
    """S = 257 crosses the 256-candidate workgroup of the scoring kernel and makes the weights kernel combine several waves; the
    candidates it shares with the S = 70 call (synth12: 9 against 5) and their scores are bit for bit the same."""
    B = 2
    S, Sp = (257, 70) if name != "synth12" else (9, 5)
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    sol = _handle(pkg, name, model, T, B, w)
    call = lambda S_, **kw: sol.sample_rollout_candidates_(sigma, S_, x1=x1, base_u=base, return_candidates=True, **dict(dict(seed=SEED), **kw))
    full, again, part = call(S), call(S), call(Sp)
    assert _same(full, again)
    for k in ("cost", "max_violation", "first_nonfinite", "u"):
        assert np.array_equal(part[k], full[k][:, :Sp], equal_nan=True), k
    for b in range(B):          # the device's choice is the rule applied to the device's own scores
        assert full["chosen"][b] == R.select(full["cost"][b], full["max_violation"][b], full["first_nonfinite"][b])
        assert part["chosen"][b] == R.select(part["cost"][b], part["max_violation"][b], part["first_nonfinite"][b])
    other = call(Sp, seed=SEED + 1)
    assert np.array_equal(other["u"][:, 0], base) and (other["u"][:, 1:] != part["u"][:, 1:]).all()
    one = call(1)
    assert (one["chosen"] == 0).all() and np.array_equal(one["cost"], full["cost"][:, :1], equal_nan=True) and np.array_equal(one["u"][:, 0], base)
    ref = _handle(pkg, name, model, T, B, w)
    ref.initialize_rollout_(x1, base)
    assert _eq(_state(sol), _state(ref))                             # S = 1 installs the base
    flat = sol.sample_rollout_candidates_(np.zeros_like(sigma), Sp, seed=SEED, x1=x1, base_u=base, return_candidates=True)
    assert (flat["u"] == base[:, None]).all() and (flat["chosen"] == 0).all()          # sigma = 0: every candidate is the base, ties to 0
    assert _eq(_state(sol), _state(ref))
    sol.close(); ref.close()


def test_sharded_handle_first_instance_and_device_form(pkg):
    import torch
    name, B, S = "car_obs", 5, 70
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    sol = _handle(pkg, name, model, T, B, w)
    kw = dict(seed=SEED, violation_weight=2.0, return_candidates=True)
    host = sol.sample_rollout_candidates_(sigma, S, x1=x1, base_u=base, **kw)
    host_state = _state(sol)
    sh = _handle(pkg, name, model, T, B, w, devices=[0, 0])
    assert _same(host, sh.sample_rollout_candidates_(sigma, S, x1=x1, base_u=base, **kw))
    assert _eq(host_state, _state(sh))
    sh.initialize_rollout_(x1, base)
    assert _same(host, sh.sample_rollout_candidates_(sigma, S, **kw))                 # every shard's own resident inputs
    assert _eq(host_state, _state(sh))
    with pytest.raises(pkg._ffi.IlqrError, match="sharded"):
        sh.sample_rollout_candidates_device_(sigma, S)
    two = _handle(pkg, name, model, T, 2, w[3:])
    tail = two.sample_rollout_candidates_(sigma, S, x1=x1[3:], base_u=base[3:], first_instance=3, **kw)
    assert all(np.array_equal(tail[k], host[k][3:], equal_nan=True) for k in host)
    with pytest.raises(pkg._ffi.IlqrError, match="2\\^23"):
        two.sample_rollout_candidates_(sigma, S, x1=x1[3:], base_u=base[3:], first_instance=(1 << 23) - 1)
    dv = _handle(pkg, name, model, T, B, w)
    with pytest.raises(pkg._ffi.IlqrError, match="resident"):
        dv.sample_rollout_candidates_(sigma, S)                                       # no resident inputs yet
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.ExternalStream(dv.stream_ptr())):
        d_x1, d_base = torch.from_numpy(x1).to(dev), torch.from_numpy(base).to(dev)
        d = dict(chosen=torch.zeros(B, dtype=torch.int32, device=dev), cost=torch.zeros(B, S, dtype=torch.float64, device=dev),
                 max_violation=torch.zeros(B, S, dtype=torch.float64, device=dev), first_nonfinite=torch.zeros(B, S, dtype=torch.int32, device=dev),
                 weights=torch.zeros(B, S, dtype=torch.float64, device=dev), u=torch.zeros(B, S, T - 1, sigma.size, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    dv.sample_rollout_candidates_device_(sigma, S, seed=SEED, violation_weight=2.0, d_x1_ptr=d_x1.data_ptr(), d_base_u_ptr=d_base.data_ptr(),
                                         d_chosen_ptr=d["chosen"].data_ptr(), d_cost_ptr=d["cost"].data_ptr(),
                                         d_max_violation_ptr=d["max_violation"].data_ptr(), d_first_nonfinite_ptr=d["first_nonfinite"].data_ptr(),
                                         d_weights_ptr=d["weights"].data_ptr(), d_u_out_ptr=d["u"].data_ptr())
    dv.synchronize()
    assert _same(host, {k: v.cpu().numpy() for k, v in d.items()})
    assert _eq(host_state, _state(dv))
    dv.sample_rollout_candidates_device_(sigma, S, seed=SEED, violation_weight=2.0, d_x1_ptr=d_x1.data_ptr(), d_base_u_ptr=d_base.data_ptr())    # no outputs wanted
    dv.synchronize()
    assert _eq(host_state, _state(dv))
    sol.close(); sh.close(); two.close(); dv.close()


def test_blend(pkg):
    name, B, S = "car_obs", 3, 70
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    sol, other = _handle(pkg, name, model, T, B, w), _handle(pkg, name, model, T, B, w)
    pick = sol.sample_rollout_candidates_(sigma, S, seed=SEED, x1=x1, base_u=base, return_candidates=True)
    u_pick = sol.buffer("nominal_actions").reshape(B, T - 1, -1)
    fin = np.where(pick["first_nonfinite"] == -1, pick["cost"], np.nan)
    spread = float(np.nanmax(np.nanmax(fin, axis=1) - np.nanmin(fin, axis=1)))
    assert spread > 0.0
    for temperature in (spread, 1e-6 * spread):
        out = sol.sample_rollout_candidates_(sigma, S, seed=SEED, mode="blend", temperature=temperature, x1=x1, base_u=base, return_candidates=True)
        assert _same(out, pick, SCORES + ("u",))
        got = sol.buffer("nominal_actions").reshape(B, T - 1, -1)
        worst = dict(w=0.0, u=0.0)
        for b in range(B):
            chosen, wt = SR.blend_weights(out["cost"][b], out["max_violation"][b], out["first_nonfinite"][b], 0.0, temperature)
            assert chosen == out["chosen"][b]
            worst["w"] = max(worst["w"], np.abs(out["weights"][b] - wt).max())
            assert abs(out["weights"][b].sum() - 1.0) < TOL_BLEND and (out["weights"][b][out["first_nonfinite"][b] != -1] == 0.0).all()
            want = SR.blend_actions(out["u"][b], out["weights"][b])
            worst["u"] = max(worst["u"], (np.abs(got[b] - want) / np.maximum(1.0, np.abs(want))).max())
        print("blend at temperature %.3e: %s" % (temperature, worst))
        assert worst["w"] <= TOL_BLEND and worst["u"] <= TOL_BLEND, worst
        other.initialize_rollout_(x1, got)
        assert _eq(_state(sol), _state(other))
        if temperature == spread:
            assert (np.count_nonzero(out["weights"] > 1e-3, axis=1) > 1).all() and np.abs(got - u_pick).max() > 1e-6     # a real blend
        else:
            assert np.abs(got - u_pick).max() <= TOL_BLEND                   # the tiny temperature: the pick
    sol.close(); other.close()


def test_blend_with_a_poisoned_instance(pkg):
    """A NaN in the base of instance 1 at step 3 reaches every candidate of it: first_nonfinite == 4, chosen == −1, weights 0, the base
    installed (NaN and all); the neighbours are bitwise what they are without the poison."""
    name, B, S = "acrobot", 3, 70
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    sol, other = _handle(pkg, name, model, T, B), _handle(pkg, name, model, T, B)
    kw = dict(seed=SEED, mode="blend", temperature=50.0, x1=x1, return_candidates=True)
    clean = sol.sample_rollout_candidates_(sigma, S, base_u=base, **kw)
    clean_u = sol.buffer("nominal_actions").reshape(B, T - 1, -1)
    bad = base.copy()
    bad[1, 3] = np.nan
    out = sol.sample_rollout_candidates_(sigma, S, base_u=bad, **kw)
    assert (out["first_nonfinite"][1] == 4).all() and out["chosen"][1] == -1 and (out["weights"][1] == 0.0).all()
    keep = [0, 2]
    assert all(np.array_equal(out[k][keep], clean[k][keep], equal_nan=True) for k in out)
    got = sol.buffer("nominal_actions").reshape(B, T - 1, -1)
    assert np.array_equal(got[keep], clean_u[keep]) and np.array_equal(got[1], bad[1], equal_nan=True)
    other.initialize_rollout_(x1, got)
    assert _eq(_state(sol), _state(other))
    sol.close(); other.close()


def test_composition_with_the_shift(pkg):
    """solve, shift_horizon_(1), sample with x1 = None, base_u = None: the call given the shifted (x1', u') explicitly, bit for bit;
    K, k, duals, penalties and the trace are what they were."""
    name, B, S = "acrobot", 2, 70
    model, T, x1, base, w, sigma = _inputs(pkg, name, B)
    a, b = _handle(pkg, name, model, T, B), _handle(pkg, name, model, T, B)
    a.enable_trace_(64)
    a.initialize_rollout_(x1, base)
    a.solve_()
    a.shift_horizon_(1)
    x1p = a.buffer("nominal_states").reshape(B, T, -1)[:, 0].copy()
    up = a.buffer("nominal_actions").reshape(B, T - 1, -1).copy()
    snap = lambda: a.get_policy() + (a.buffer("constraint_dual"), a.buffer("constraint_penalty"), a.trace())
    before = snap()
    out = a.sample_rollout_candidates_(0.25 * sigma, S, seed=SEED, return_candidates=True)
    assert _eq(before, snap())
    assert np.array_equal(out["u"][:, 0], up)
    ref = b.sample_rollout_candidates_(0.25 * sigma, S, seed=SEED, x1=x1p, base_u=up, return_candidates=True)
    assert _same(out, ref)
    assert _eq(_state(a)[:2], _state(b)[:2])
    assert np.array_equal(a.buffer("nominal_actions").reshape(B, T - 1, -1), out["u"][np.arange(B), np.maximum(out["chosen"], 0)])
    a.close(); b.close()


def test_minimal_horizon(pkg):
    """T = 2: one action, one (ragged) tile"""
    B, S, T = 3, 70, 2
    model, T, x1, base, w, sigma = _inputs(pkg, "particle", B, T=T)
    a, b = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0)), pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0))
    out = a.sample_rollout_candidates_(sigma, S, seed=SEED, x1=x1, base_u=base, return_candidates=True)
    assert _same(out, b.initialize_rollout_candidates_(x1, out["u"]), SCORES)
    assert _eq(_state(a), _state(b))
    assert np.abs(out["u"][:, 1:, 0] - base[:, None, 0] - sigma * pkg.candidate_noise(SEED, B, S, 1, 1)[:, 1:, 0]).max() <= TOL_NOISE
    a.close(); b.close()


def test_unconstrained_handle_reports_zero_violation(pkg):
    B, S = 2, 5
    model, T, x1, base, w, sigma = _inputs(pkg, "car", B)
    sol = pkg.Solver(model=model, horizon=T, batch=B, options=pkg.Options(verbose=0), constraints=False)
    out = sol.sample_rollout_candidates_(sigma, S, seed=SEED, violation_weight=3.0, x1=x1, base_u=base)
    assert (out["max_violation"] == 0.0).all() and np.isfinite(out["cost"]).all() and (out["chosen"] >= 0).all()
    sol.close()


def test_plain_c_example(pkg, tmp_path):
    """examples/sample_candidates.c: solve, shift, sample around the shifted guess, solve again — from plain C"""
    exe = str(tmp_path / "sample_candidates")
    libdir = os.path.join(ROOT, "iterativelqr.jl_amd", "lib")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sample_candidates.c"),
                           "-o", exe, "-L" + libdir, "-lilqr_hip", "-Wl,-rpath," + libdir, "-lm"])
    out = subprocess.run(["timeout", "-k", "10", "120", exe, "16", "32"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    first = out.stdout.splitlines()[0]
    assert first.startswith("chosen candidate of instance 0: ") and 0 <= int(first.split(": ")[1].split()[0]) < 32, first
    assert "sample candidates check passed" in out.stdout
