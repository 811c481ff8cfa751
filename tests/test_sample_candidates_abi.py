"""ilqr_sample_rollout_candidates / ilqr_candidate_noise without a GPU: the symbols are exported, declared and mirrored, every refusal
that needs no handle holds, the host twin of the device's generator agrees with a numpy restatement (tests/sample_ref.py), is a pure
function of (seed, b, s, t, j) and has the first two moments of a standard normal, and the blend rule of the yardstick does what the
header says on hand-made score tables.

Bounds. |Δz| <= 1e-14 between the library (libm) and numpy: both evaluate log, sqrt and cos to about an ulp, the integers and
the cosine's argument are the same IEEE operations, |z| <= 8.7: a few ulp of 8.7 is below 1e-14. Moments over 2^16 values:
|mean| < 0.02, |var − 1| < 0.03 — five standard errors (1 / 256 and sqrt(2 / 65536))."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sample_ref as R
from ilqr_amd_loader import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ["ilqr_sample_rollout_candidates", "ilqr_sample_rollout_candidates_device"]
SEED = 20261019


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    p = load_package()
    assert hasattr(p._ffi.lib(), FNS[0]), "the library has no %s: nothing here has a subject" % FNS[0]
    return p


def test_symbols_are_exported_declared_and_mirrored(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_hip.h")).read(), flags=re.S)
    L = pkg._ffi.lib()
    for name in FNS + ["ilqr_candidate_noise"]:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
    for name in FNS:
        res, args = pkg._ffi.SYMBOLS[name]
        assert res is C.c_int and len(args) == 16 and args[1] is C.c_int32 and args[2] is C.c_int32 and args[3] is C.c_uint64 and args[4] is C.c_int64
        assert args[5] is pkg._ffi.c_double_p and args[6] is C.c_double and args[7] is C.c_double            # sigma: a host pointer in both forms
    res, args = pkg._ffi.SYMBOLS["ilqr_candidate_noise"]
    assert res is C.c_int and args == [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, pkg._ffi.c_double_p]
    assert re.search(r"#define\s+ILQR_SAMPLE_PICK\s+0\b", hdr) and re.search(r"#define\s+ILQR_SAMPLE_BLEND\s+1\b", hdr)
    assert callable(pkg.Solver.sample_rollout_candidates_) and callable(pkg.Solver.sample_rollout_candidates_device_) and callable(pkg.candidate_noise)
    assert pkg.Solver._SAMPLE_MODES == {"pick": 0, "blend": 1}
    jl = open(os.path.join(ROOT, "iterativelqr.jl_amd", "julia", "IterativeLQRAMD.jl")).read()
    assert "function sample_rollout_candidates!(" in jl and ":ilqr_sample_rollout_candidates, LIB[]" in jl and ":ilqr_candidate_noise, LIB[]" in jl
    assert "sample_rollout_candidates!," in jl.split("const LIB")[0]
    assert os.path.exists(os.path.join(ROOT, "examples", "sample_candidates.c"))
    dev = open(os.path.join(ROOT, "iterativelqr.jl_amd", "csrc", "ilqr_device.hpp")).read()
    assert '#include "ilqr_device_sample.hpp"' in dev and "launch_sample_candidates" in dev


@pytest.mark.parametrize("fn", FNS)
def test_argument_refusals_need_no_device(pkg, fn):
    """candidates outside 1 .. 65536, an unknown mode, a null sigma or a negative or non-finite entry, a bad violation_weight, a blend
    whose temperature is not finite and > 0, a first_instance outside 0 .. 2^23 − 1 and a null handle are refused before the handle is
    looked at (so: on a machine with no device, where no handle can exist), each with the function's name in the message. The
    refusals that need a handle — first_instance + batch beyond 2^23, NULL x1 / base_u without resident inputs, the device form on a
    sharded handle — are in the GPU file."""
    L = pkg._ffi.lib()
    f = getattr(L, fn)

    def sig(v):
        arr = np.array([v, 0.0, 0.0, 0.0])
        return arr.ctypes.data_as(pkg._ffi.c_double_p), arr

    good, nan, inf = 0.1, math.nan, math.inf
    cases = [(0, 0, 0, good, 0.0, 1.0, b"candidates must lie in 1 .. 65536"), (-2, 0, 0, good, 0.0, 1.0, b"candidates must lie in 1 .. 65536"),
             (65537, 1, 0, good, 0.0, 1.0, b"candidates must lie in 1 .. 65536"),
             (4, 2, 0, good, 0.0, 1.0, b"unknown mode"), (4, -1, 0, good, 0.0, 1.0, b"unknown mode"),
             (4, 0, 0, None, 0.0, 1.0, b"null sigma"), (4, 0, 0, -0.5, 0.0, 1.0, b"sigma must be finite and >= 0"),
             (4, 1, 0, nan, 0.0, 1.0, b"sigma must be finite and >= 0"), (4, 0, 0, inf, 0.0, 1.0, b"sigma must be finite and >= 0"),
             (4, 0, 0, good, -1.0, 1.0, b"violation_weight"), (4, 0, 0, good, nan, 1.0, b"violation_weight"), (4, 1, 0, good, inf, 1.0, b"violation_weight"),
             (4, 1, 0, good, 0.0, 0.0, b"temperature"), (4, 1, 0, good, 0.0, -2.0, b"temperature"), (4, 1, 0, good, 0.0, nan, b"temperature"),
             (4, 1, 0, good, 0.0, inf, b"temperature"),
             (4, 0, -1, good, 0.0, 1.0, b"first_instance"), (4, 0, 1 << 23, good, 0.0, 1.0, b"first_instance"),
             (4, 0, 0, good, 0.0, -5.0, b"null handle"),                      # pick does not read the temperature
             (65536, 1, (1 << 23) - 1, 0.0, 2.5, 1e-300, b"null handle")]
    for cand, mode, first, sigma, weight, temp, msg in cases:
        sp, keep = sig(sigma) if sigma is not None else (None, None)
        assert f(None, cand, mode, 7, first, sp, weight, temp, None, None, None, None, None, None, None, None) == -1, msg
        err = L.ilqr_last_error()
        assert msg in err and fn.encode() in err, err


def test_candidate_noise_refusals(pkg):
    L = pkg._ffi.lib()
    z = np.zeros(64)
    p = z.ctypes.data_as(pkg._ffi.c_double_p)
    for first, B, S, steps, nu, ptr in [(0, 1, 1, 1, 1, None), (-1, 1, 1, 1, 1, p), ((1 << 23), 1, 1, 1, 1, p), ((1 << 23) - 1, 2, 1, 1, 1, p),
                                        (0, -1, 1, 1, 1, p), (0, 1, 65537, 0, 1, p), (0, 1, 1, (1 << 20) + 1, 0, p), (0, 1, 1, 1, 17, p),
                                        (0, 1, -1, 1, 1, p), (0, 1, 1, -1, 1, p), (0, 1, 1, 1, -1, p)]:
        assert L.ilqr_candidate_noise(SEED, first, B, S, steps, nu, ptr) == -1, (first, B, S, steps, nu)
        assert b"ilqr_candidate_noise" in L.ilqr_last_error()
    assert L.ilqr_candidate_noise(SEED, (1 << 23) - 1, 1, 2, 2, 16, p) == 0          # the last instance, the widest action
    assert (z[:32] == 0.0).all() and (z[32:] != 0.0).all()
    assert L.ilqr_candidate_noise(SEED, 0, 0, 5, 5, 5, p) == 0                       # an empty batch writes nothing


def test_candidate_noise_is_the_numpy_restatement(pkg):
    B, S, steps, nu = 3, 70, 13, 2
    z = pkg.candidate_noise(SEED, B, S, steps, nu)
    ref = R.noise(SEED, B, S, steps, nu)
    assert z.shape == ref.shape == (B, S, steps, nu)
    assert (z[:, 0] == 0.0).all() and not np.signbit(z[:, 0]).any()
    err = np.abs(z - ref).max()
    print("candidate_noise against numpy: max |dz| = %.2e, max |z| = %.3f" % (err, np.abs(z).max()))
    assert err <= 1e-14 and np.abs(z).max() <= 8.7
    # a seed with the top bit set, and the top of every index range: the packing is the header's
    big = (1 << 63) + 12345
    z = pkg.candidate_noise(big, 1, 3, 2, 16, first_instance=(1 << 23) - 1)
    assert np.abs(z - R.noise(big, 1, 3, 2, 16, first_instance=(1 << 23) - 1)).max() <= 1e-14
    L = pkg._ffi.lib()
    steps = 1 << 20
    tail = np.empty((1, 2, steps, 1))
    assert L.ilqr_candidate_noise(SEED, 5, 1, 2, steps, 1, tail.ctypes.data_as(pkg._ffi.c_double_p)) == 0
    h1 = R.mix(np.uint64(SEED) ^ np.uint64((5 << 40) + (1 << 24) + ((steps - 1) << 4)))
    want = math.sqrt(-2.0 * math.log(float(R.unif(h1)))) * math.cos(6.283185307179586 * float(R.unif(R.mix(h1))))
    assert abs(tail[0, 1, steps - 1, 0] - want) <= 1e-14


def test_candidate_noise_is_a_pure_function_of_its_indices(pkg):
    """The value at (b, s, t, j) does not depend on B, S or steps: slices of a larger call are the smaller call bit for bit, and
    first_instance = k gives rows k.. of first_instance = 0. (nu is part of the layout only: component j keeps its value too.)"""
    big = pkg.candidate_noise(SEED, 5, 70, 13, 3)
    assert np.array_equal(pkg.candidate_noise(SEED, 2, 9, 7, 3), big[:2, :9, :7])
    assert np.array_equal(pkg.candidate_noise(SEED, 5, 70, 13, 2), big[..., :2])
    assert np.array_equal(pkg.candidate_noise(SEED, 2, 70, 13, 3, first_instance=3), big[3:])
    assert np.array_equal(pkg.candidate_noise(SEED, 5, 70, 13, 3), big)
    other = pkg.candidate_noise(SEED + 1, 5, 70, 13, 3)
    assert (other[:, 1:] != big[:, 1:]).all()


def test_candidate_noise_moments_and_keys(pkg):
    z = pkg.candidate_noise(SEED, 4, 65, 64, 4)[:, 1:]            # 4 · 64 · 64 · 4 = 2^16 values
    assert z.size == 1 << 16
    mean, var = z.mean(), z.var()
    print("candidate_noise over 2^16 values: mean %.4f, var %.4f" % (mean, var))
    assert abs(mean) < 0.02 and abs(var - 1.0) < 0.03
    k = R.keys(SEED, 4, 4, 16, 16).ravel()                        # the first 4096 keys in layout order
    assert k.size == 4096 and np.unique(k).size == 4096
    k = R.keys(SEED, 2, 2, 2, 2, first_instance=(1 << 23) - 2) ^ np.uint64(SEED)
    assert int(k[1, 1, 1, 1]) == (((1 << 23) - 1) << 40) + (1 << 24) + (1 << 4) + 1


def test_the_blend_rule_on_hand_made_tables():
    nan, inf = math.nan, math.inf
    ok = [-1] * 4
    c, w = R.blend_weights([3.0, 1.0, 2.0, 1.5], [0.0] * 4, ok, 0.0, 1.0)
    assert c == 1 and abs(w.sum() - 1.0) < 1e-15 and w[1] == w.max()
    assert np.allclose(w, np.exp(-np.array([2.0, 0.0, 1.0, 0.5])) / np.exp(-np.array([2.0, 0.0, 1.0, 0.5])).sum(), rtol=0, atol=1e-16)
    # ineligible candidates (a NaN or infinite score, a non-finite state) get 0; the others still sum to 1
    c, w = R.blend_weights([nan, 5.0, -inf, 4.0], [0.0] * 4, [-1, -1, -1, 2], 0.0, 0.5)
    assert c == 1 and list(w) == [0.0, 1.0, 0.0, 0.0]
    c, w = R.blend_weights([1.0, 5.0, 2.0, 3.0], [0.0] * 4, [7, -1, 0, -1], 0.0, 2.0)
    assert c == 3 and w[0] == 0.0 and w[2] == 0.0 and abs(w.sum() - 1.0) < 1e-15 and abs(w[1] / w[3] - math.exp(-1.0)) < 1e-15
    # nobody eligible: all weights 0 and chosen −1
    c, w = R.blend_weights([nan, inf, 1.0, -inf], [0.0] * 4, [-1, -1, 4, -1], 0.0, 1.0)
    assert c == -1 and (w == 0.0).all()
    # the violation weight enters the score
    c, w = R.blend_weights([1.0, 2.0, 3.0], [0.5, 0.1, 0.0], [-1] * 3, 5.0, 1.0)               # 3.5, 2.5, 3.0
    assert c == 1 and np.allclose(w * np.exp(-np.array([1.0, 0.0, 0.5])).sum(), np.exp(-np.array([1.0, 0.0, 0.5])), rtol=0, atol=1e-15)
    # a very small temperature: the weights are the pick (ties included: every minimiser keeps its share)
    c, w = R.blend_weights([3.0, 1.0, 2.0, 1.5], [0.0] * 4, ok, 0.0, 1e-9)
    assert c == 1 and list(w) == [0.0, 1.0, 0.0, 0.0]
    c, w = R.blend_weights([3.0, 1.0, 1.0, 1.5], [0.0] * 4, ok, 0.0, 1e-9)
    assert c == 1 and list(w) == [0.0, 0.5, 0.5, 0.0]
    # the blended actions: the weighted sum in ascending s
    u = np.arange(24, dtype=np.float64).reshape(4, 3, 2)
    assert np.array_equal(R.blend_actions(u, np.array([0.0, 1.0, 0.0, 0.0])), u[1])
    assert np.array_equal(R.blend_actions(u, np.array([0.5, 0.0, 0.0, 0.5])), 0.5 * u[0] + 0.5 * u[3])
