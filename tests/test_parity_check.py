"""The whole-solve comparison (tests/parity_check.py) that the GPU parity tests assert through, fed planted faults on CPU arrays:
each must make it fail, and the unchanged arrays must pass."""
import numpy as np
import pytest

import parity_check as P

B, T, N, M = 200, 12, 2, 1
A = np.array([[1.0, 0.1], [-0.05, 0.98]])
BU = np.array([[0.0], [0.1]])
OPTS = dict(min_match=0.99, tol=2e-8, tol_K=1e-7, tol_k=1e-7, constraint_tolerance=5e-3, max_dual_updates=10)
DIFFER = 7          # an instance whose control flow differs from the oracle's (a legitimate other path)


def step(x, u):
    return A @ x + BU @ u


def rollout(x1, u):
    x = np.zeros((T, N))
    x[0] = x1
    for t in range(T - 1):
        x[t + 1] = step(x[t], u[t])
    return x


def pair():
    """An oracle solve and a device solve that agrees with it to rounding, one instance on another path."""
    rng = np.random.default_rng(3)
    x1 = rng.standard_normal((B, N))
    u = rng.standard_normal((B, T - 1, M))
    ref = dict(x=np.stack([rollout(x1[b], u[b]) for b in range(B)]), u=u, K=3.0 * rng.standard_normal((B, T - 1, N, M)),
               k=rng.standard_normal((B, T - 1, M)))
    ref["stats"] = dict(iterations=rng.integers(20, 400, B), outer_iterations=rng.integers(1, 4, B), rollouts=rng.integers(20, 900, B),
                        status=np.zeros(B, int), objective=rng.uniform(1.0, 10.0, B), max_violation=rng.uniform(0.0, 4e-3, B),
                        potrf_info=np.zeros(B, int))
    dev = {f: ref[f] * (1.0 + 1e-13) for f in ("u", "K", "k")}
    dev["x"] = np.stack([rollout(x1[b], dev["u"][b]) for b in range(B)])
    dev["stats"] = {f: v.copy() for f, v in ref["stats"].items()}
    st = dev["stats"]
    st["iterations"][DIFFER] += 3; st["rollouts"][DIFFER] += 5; st["outer_iterations"][DIFFER] = 10; st["max_violation"][DIFFER] = 0.2
    dev["u"][DIFFER] = u[DIFFER] + 0.3 * rng.standard_normal((T - 1, M))
    dev["x"][DIFFER] = rollout(x1[DIFFER], dev["u"][DIFFER])
    return dev, ref, x1


def run(dev, ref, x1, **kw):
    return P.compare(dev, ref, step=step, x1=x1, **dict(OPTS, **kw))


def test_unchanged_arrays_pass():
    dev, ref, x1 = pair()
    r = run(dev, ref, x1)
    assert list(r["differ"]) == [DIFFER] and r["frac"] == pytest.approx(1 - 1 / B)
    assert 0 < r["dx"] < 1e-11 and 0 < r["dk"] < 1e-11


def test_k_off_by_one_part_in_a_million_fails():
    dev, ref, x1 = pair()
    dev["k"] = dev["k"] * (1.0 + 1e-6)
    with pytest.raises(AssertionError):
        run(dev, ref, x1)


def test_garbage_trajectory_on_an_instance_with_other_control_flow_fails():
    dev, ref, x1 = pair()
    dev["x"][DIFFER, 1:] = np.random.default_rng(5).standard_normal((T - 1, N))
    with pytest.raises(AssertionError):
        run(dev, ref, x1)


def test_other_control_flow_must_end_the_reference_way():
    dev, ref, x1 = pair()
    dev["stats"]["outer_iterations"][DIFFER] = 4          # infeasible and dual updates left: the outer loop would not have stopped
    with pytest.raises(AssertionError):
        run(dev, ref, x1)


@pytest.mark.parametrize("field", ["x", "u", "K", "k"])
@pytest.mark.parametrize("b", [DIFFER, 0])
def test_nan_where_the_oracle_is_finite_fails(b, field):
    dev, ref, x1 = pair()
    dev[field][b, 4] = np.nan
    with pytest.raises(AssertionError):
        run(dev, ref, x1)


@pytest.mark.parametrize("field", ["x", "u", "K", "k"])
def test_nan_is_never_excused_as_chaotic(field):
    dev, ref, x1 = pair()
    dev[field][0, 3] = np.nan
    with pytest.raises(AssertionError):
        run(dev, ref, x1, spread=_spread(ref, 0.2))


def test_non_finite_instances_must_match_the_oracle_there():
    dev, ref, x1 = pair()
    ref["x"][11, 5:] = np.inf
    dev["x"][11, 5:] = np.inf
    run(dev, ref, x1)
    dev["x"][11, 6] = 0.0
    with pytest.raises(AssertionError):
        run(dev, ref, x1)


def test_one_mismatching_instance_fails_without_the_chaotic_rule():
    dev, ref, x1 = pair()
    dev["x"][20, -1] += 1e-7
    with pytest.raises(AssertionError):
        run(dev, ref, x1)


def _spread(ref, scale):
    """The oracle against itself under a perturbed ū: `scale` times the planted error on the planted instances."""
    def spread(idx):
        return {f: np.full(len(idx), scale * 1e-6) for f in ("x", "u", "K", "k")}
    return spread


def test_chaotic_allowance():
    dev, ref, x1 = pair()
    n = int(P.CHAOTIC_ALLOWANCE * B)
    for b in range(30, 30 + n):
        dev["x"][b, -1] += 1e-6
    r = run(dev, ref, x1, spread=_spread(ref, 0.2))              # within 10x the oracle's own spread: chaotic
    assert len(r["loose"]) == n
    with pytest.raises(AssertionError):
        run(dev, ref, x1, spread=_spread(ref, 0.05))             # beyond it: not chaotic
    dev["x"][30 + n, -1] += 1e-6                                  # one more than the allowance
    with pytest.raises(AssertionError):
        run(dev, ref, x1, spread=_spread(ref, 0.2))


def test_min_match():
    dev, ref, x1 = pair()
    with pytest.raises(AssertionError):
        run(dev, ref, x1, min_match=1.0)
