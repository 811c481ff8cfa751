"""The yardstick of the candidate-sampling tests (tests/test_sample_candidates_abi.py, tests/test_gpu_sample_candidates.py) in numpy:
the noise z(seed, b, s, t, j) of include/ilqr_hip.h restated with uint64 arithmetic, np.log and np.cos, and the blend rule
(softmin weights over the eligible candidates, the weighted sum in ascending s). The selection rule is candidates_ref.select."""
import math

import numpy as np

import candidates_ref as R

M64 = (1 << 64) - 1


def mix(z):
    """splitmix64 on a uint64 array (wrap-around arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys(seed, B, S, steps, nu, first_instance=0):
    """key[b, s, t, j] = seed ^ (b·2^40 + s·2^24 + t·2^4 + j), b counted from first_instance"""
    b = (np.arange(B, dtype=np.uint64) + np.uint64(first_instance)).reshape(B, 1, 1, 1)
    s = np.arange(S, dtype=np.uint64).reshape(1, S, 1, 1)
    t = np.arange(steps, dtype=np.uint64).reshape(1, 1, steps, 1)
    j = np.arange(nu, dtype=np.uint64).reshape(1, 1, 1, nu)
    packed = b * np.uint64(1 << 40) + s * np.uint64(1 << 24) + t * np.uint64(1 << 4) + j
    return np.uint64(seed & M64) ^ packed


def unif(h):
    return ((h >> np.uint64(11)).astype(np.float64) + 0.5) / 9007199254740992.0


def noise(seed, B, S, steps, nu, first_instance=0):
    """z [B, S, steps, nu]; row s = 0 is zero"""
    h1 = mix(keys(seed, B, S, steps, nu, first_instance))
    h2 = mix(h1)
    z = np.sqrt(-2.0 * np.log(unif(h1))) * np.cos(6.283185307179586 * unif(h2))
    z[:, 0] = 0.0
    return z


def blend_weights(cost, max_violation, nonfinite, weight, temperature):
    """(chosen, w [S]) of one instance: w_s = exp(−(score_s − score_min) / temperature) over the eligible candidates (finite score,
    first_nonfinite == −1), 0 for the others, divided by their sum; nobody eligible: chosen −1, all weights 0."""
    sc = R.scores(cost, max_violation, weight)
    chosen = R.select(cost, max_violation, nonfinite, weight)
    w = np.zeros(len(sc))
    if chosen < 0:
        return chosen, w
    for s, v in enumerate(sc):
        if math.isfinite(v) and int(nonfinite[s]) == -1:
            w[s] = np.exp(-(v - sc[chosen]) / temperature)
    total = 0.0
    for v in w:                                   # ascending s
        total += v
    return chosen, w / total


def blend_actions(u, w):
    """Σ_s w_s · u[s] of one instance, summed in ascending s: u [S, T-1, nu], w [S]"""
    acc = np.zeros(u.shape[1:])
    for s in range(u.shape[0]):
        if w[s] != 0.0:
            acc = acc + w[s] * u[s]
    return acc
