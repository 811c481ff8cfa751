"""The yardstick of the horizon-shift tests (tests/test_shift_abi.py, tests/test_gpu_shift.py): what ilqr_shift_horizon installs,
in numpy and on the CPU oracle. With k = steps, N = T − 1:

    x1' = x1  or  x̄_k          w'_t = w_{t+k}  (t + k <= T−1),  then w_tail[t − (T−k)]  or  w_{T−1}
    open loop:    u'_t = ū_{t+k}  (t < N−k),  then ū_{N−1} ("hold") or 0 ("zero")
    closed loop:  u'_t = ū_{t+k} + K_{t+k} (x'_t − x̄_{t+k}),  x'_{t+1} = f(x'_t, u'_t, w'_t),  x'_0 = x1'   (t < N−k), tail as above

Arrays are one instance's: xb [T, n], ub [T-1, m], K [T-1, n, m] (as get_policy returns it), w None or [T, nw].
"""
import numpy as np

import policy_ref


def shifted_inputs(xb, ub, w, k, tail="hold", x1=None, w_tail=None):
    """The open-loop (x1', u', w') by slicing; w' is None when w is. Row T−1 of w is the terminal row: it is what "hold" repeats."""
    xb, ub = np.asarray(xb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    N = ub.shape[0]
    assert 0 <= k <= N and tail in ("hold", "zero")
    x1p = xb[k].copy() if x1 is None else np.array(x1, dtype=np.float64)
    up = np.empty_like(ub)
    up[:N - k] = ub[k:]
    up[N - k:] = ub[N - 1] if tail == "hold" else 0.0
    wp = None
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        T = w.shape[0]
        assert T == N + 1
        wp = np.empty_like(w)
        wp[:T - k] = w[k:]
        if k > 0:
            wp[T - k:] = w[T - 1] if w_tail is None else np.asarray(w_tail, dtype=np.float64).reshape(k, w.shape[1])
    else:
        assert w_tail is None
    return x1p, up, wp


def _head_slices(T, xb, ub, K, wp, k):
    """the arrays of the closed-loop head as a problem of horizon T − k"""
    n, m = np.asarray(xb).shape[-1], np.asarray(ub).shape[-1]
    xs, us, Ks = np.asarray(xb).reshape(T, n)[k:], np.asarray(ub).reshape(T - 1, m)[k:], np.asarray(K).reshape(T - 1, n, m)[k:]
    ws = None if wp is None else np.ascontiguousarray(np.asarray(wp)[:T - k])
    return np.ascontiguousarray(xs), np.ascontiguousarray(us), np.ascontiguousarray(Ks), ws


def feedback_head(O, model, T, xb, ub, K, wp, k, x1):
    """The closed-loop head on the oracle: policy_ref.oracle_reading on the slices xb[k:], ub[k:], K[k:], w'[:T−k] with horizon
    T − k, from x1. Returns dict(x [T−k, n], u [T−k−1, m], first_nonfinite)."""
    assert 0 <= k < T - 1
    xs, us, Ks, ws = _head_slices(T, xb, ub, K, wp, k)
    r = policy_ref.oracle_reading(O, model, T - k, xs, us, Ks, x1, ws)
    return dict(x=r["x"], u=r["u"], first_nonfinite=r["first_nonfinite"])


def feedback_head_numpy(O, model, T, xb, ub, K, wp, k, x1):
    """the second reading: policy_ref.numpy_reading (the plain loop, α = 0) on the same slices"""
    xs, us, Ks, ws = _head_slices(T, xb, ub, K, wp, k)
    return policy_ref.numpy_reading(O, model, T - k, xs, us, Ks, np.zeros_like(us), x1, 0.0, ws)


def head_spread(O, model, T, xb, ub, K, wp, k, x1s):
    """policy_ref.spread on the sliced arrays: how far the oracle's own closed-loop head moves under a 1e-15 move of x1"""
    xs, us, Ks, ws = _head_slices(T, xb, ub, K, wp, k)
    return policy_ref.spread(O, model, T - k, xs, us, Ks, x1s, None if ws is None else [ws] * len(x1s))


def measured_starts(xbk, count, size, seed):
    """x1[i] = x̄_k + size · N(0, 1); a fixed seed"""
    rng = np.random.default_rng(seed)
    return np.asarray(xbk, dtype=np.float64)[None, :] + size * rng.standard_normal((count, len(xbk)))


def measured_start(xbk, size, b, k):
    """the start of instance b for a shift by k in the tests: one draw, seeded by (b, k)"""
    return measured_starts(xbk, 1, size, seed=policy_ref.SEED + 1000 * k + b)[0]


def time_varying(w):
    """the workload's parameters made to differ from row to row: + 0.01 · t"""
    w = np.asarray(w, dtype=np.float64)
    return w + 0.01 * np.arange(w.shape[-2], dtype=np.float64)[:, None]
