"""Host-side mirror of IterativeLQR.jl's user API over the C-ABI.

Names follow src/IterativeLQR.jl:30-45: Dynamics, Cost, Constraint (codegen.py),
Solver, Options, initialize_controls!, initialize_states!, solve!, get_trajectory,
rollout. Julia's `f!` becomes `f_`. One Solver here owns a BATCH of B independent
instances; every array gains a leading batch axis.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _ffi, lowering, codegen
from ._ffi import Options as _COptions


def Options(**kw):
    """Options(; kwargs...) — src/options.jl:1-15. line_search: "armijo" | "none"."""
    o = _COptions()
    _ffi.check(_ffi.lib().ilqr_default_options(C.byref(o)))
    for k, v in kw.items():
        if k == "line_search" and isinstance(v, str):
            v = {"armijo": 1, "none": 0}[v]
        if not hasattr(o, k):
            raise TypeError("Options has no field %r" % k)
        setattr(o, k, v)
    return o


def _p(a):
    return a.ctypes.data_as(_ffi.c_double_p)


def _nul(a):
    """a float64 array as a pointer, None as a null pointer"""
    return _p(a) if a is not None else None


def _vp(p):
    """a raw device pointer, None (or 0) as a null pointer"""
    return C.c_void_p(p) if p else None


def _limits(nu, u_min, u_max):
    """the actuator's limits as contiguous float64 vectors of nu entries (None stays None)"""
    out = []
    for name, v in (("u_min", u_min), ("u_max", u_max)):
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.shape != (nu,):
                raise ValueError("%s must have nu entries" % name)
        out.append(v)
    return out


def _sigma_y(nx, sigma_y):
    if sigma_y is None:
        return None
    sigma_y = np.ascontiguousarray(sigma_y, dtype=np.float64)
    if sigma_y.shape != (nx,):
        raise ValueError("sigma_y must have nx entries")
    return sigma_y


def _variances(nx, measured, q, r):
    """the filter's mask (int32) and variance vectors (float64) of nx entries each (None stays None)"""
    if measured is not None:
        measured = np.ascontiguousarray(measured, dtype=np.int32)
        if measured.shape != (nx,):
            raise ValueError("measured must have nx entries")
    out = [measured]
    for name, v in (("q", q), ("r", r)):
        if v is not None:
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (nx,)))
        out.append(v)
    return out


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


class MpcResult:
    """What Solver.mpc_run_ returns: the closed-loop states x and actions u, the per-period log and first_nonfinite; with score=True
    the realised stage cost and violation of every plant step, cl_cost and cl_violation [B, periods · steps] (None otherwise); with
    limits, measurement noise or a delay what the controller was given per period, y_cl [B, periods, nx], and the number of (step,
    component) pairs the actuator's limits changed, saturated [B] (None otherwise); with an estimator the estimate the controller
    was anchored at per period, xhat [B, periods, nx], the diagonal of its covariance at that moment, pdiag [B, periods, nx], the
    period's normalised innovation squared, nis [B, periods], and the last covariance P [B, nx, nx] (None otherwise)."""
    __slots__ = ("x", "u", "log", "first_nonfinite", "cl_cost", "cl_violation", "y_cl", "saturated", "xhat", "pdiag", "nis", "P")

    def __init__(self, x, u, log, first_nonfinite, cl_cost=None, cl_violation=None, y_cl=None, saturated=None, xhat=None, pdiag=None, nis=None,
                 P=None):
        self.x, self.u, self.log, self.first_nonfinite = x, u, log, first_nonfinite
        self.cl_cost, self.cl_violation = cl_cost, cl_violation
        self.y_cl, self.saturated = y_cl, saturated
        self.xhat, self.pdiag, self.nis, self.P = xhat, pdiag, nis, P


MODEL_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-mllvm", "-amdgpu-mfma-vgpr-form",   # MFMA results straight into VGPRs (no AGPR copies)
               "-Wno-unused-parameter"]


def _toolchain_hash():
    """Everything besides the model source that ends up in a model module: the kernel templates it instantiates
    (csrc/*.hpp), the C-ABI header and the compile flags. A cached module built against other headers would be
    launched with a KArgs / Layout it misreads."""
    import hashlib
    h = hashlib.sha256(" ".join(MODEL_FLAGS).encode())
    for d, pat in ((_ffi.CSRC, ".hpp"), (_ffi.INCLUDE, ".h")):
        for f in sorted(os.listdir(d)):
            if f.endswith(pat):
                h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def compile_model(name, dynamics, cost_stage, cost_term, con_stage=None, con_term=None):
    """Symbolic model objects -> generated device code -> model module (.so).

    Returns (registered_name, path). The registered name carries a hash of the generated source AND of the kernel
    headers / flags, so two different problems traced under the same user name never share a registry entry or a
    cached module, and a header change invalidates every cached module."""
    import hashlib
    sname, src = codegen.generate_model_source(name, dynamics, cost_stage, cost_term, con_stage, con_term)
    tag = hashlib.sha256((src + _toolchain_hash()).encode()).hexdigest()[:16]
    uname = "%s_%s" % (name, tag)
    src = src.replace("struct %s {" % sname, "struct %s_%s {" % (sname, tag), 1)
    src = src.replace('NAME = "%s";' % name, 'NAME = "%s";' % uname, 1)
    cache = os.path.join(_ffi.LIB_DIR, "models")
    os.makedirs(cache, exist_ok=True)
    so = os.path.join(cache, "libilqr_model_%s.so" % uname)
    if not os.path.exists(so):
        hip = os.path.join(cache, "model_%s.hip" % uname)
        with open(hip, "w") as f:
            f.write('#include "ilqr_device.hpp"\n' + src + "ILQR_DEFINE_MODEL(%s_%s)\n" % (sname, tag))
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + MODEL_FLAGS + ["-I", _ffi.CSRC, hip, "-o", tmp,
                               "-L", _ffi.LIB_DIR, "-lilqr_hip", "-Wl,-rpath," + _ffi.LIB_DIR])
        os.replace(tmp, so)
    return uname, so


def compile_sensor_source(name, nx, ny, ns, source):
    """C source of a sensor's `sensor_row` (written by hand, or generate_sensor_source's) -> sensor module (ilqr_compile_sensor:
    hipcc as a child process, cached in lib/models). Returns (registered_name, path)."""
    reg, path = C.create_string_buffer(256), C.create_string_buffer(4096)
    src = _ffi.SensorSource(name.encode(), int(nx), int(ny), int(ns), source.encode(), 0)
    _ffi.check(_ffi.lib().ilqr_compile_sensor(C.byref(src), reg, len(reg), path, len(path)))
    return reg.value.decode(), path.value.decode()


def compile_sensor(name, h, nx, ns=0):
    """A nonlinear sensor y = h(x, s) from a Python function on sympy symbols (x: nx states, s: ns sensor parameters; returns the ny
    outputs): traced, differentiated and emitted row-wise by codegen.generate_sensor_source, compiled by ilqr_compile_sensor.
    Returns (registered_name, path); the name is what the Solver's sensor methods and mpc_run_(estimator=dict(sensor=...)) take."""
    ny, src = codegen.generate_sensor_source(name, h, nx, ns)
    return compile_sensor_source(name, nx, ny, ns, src)


def sensor_dims(sensor):
    """(nx, ny, ns) of a registered sensor"""
    d = [C.c_int32() for _ in range(3)]
    _ffi.check(_ffi.lib().ilqr_sensor_dims(sensor.encode(), *[C.byref(v) for v in d]))
    return tuple(v.value for v in d)


class Solver:
    """Solver(dynamics, costs[, constraints]; options) — src/solver.jl:11-46 — for a batch.

    `dynamics` / `costs` / `constraints` are either lists of codegen objects laid
    out like the reference's (T-1 dynamics, T costs, T constraints; stage objects
    identical, terminal object last) or omitted when `model` names a built-in.
    """

    def __init__(self, dynamics=None, costs=None, constraints=None, *, model=None, horizon=None, batch=1,
                 options=None, device=0, devices=None, name="user", stage_sources=None):
        """devices: list of HIP ordinals — the batch is split into contiguous ranges over them (ilqr_create_sharded: one handle,
        every GPU of the node); device: a single ordinal (ilqr_create).
        stage_sources = (StageKinds, C source): distinct per-step objects given as C callables per kind — the route of a host
        without the symbolic generator (ilqr_compile_model_stages; the Julia wrapper's Solver(dynamics, costs, constraints) with
        differing objects); dynamics / costs / constraints stay None."""
        L = _ffi.lib()
        model_library = None
        self._selectors = None
        if stage_sources is not None:
            kinds, source = stage_sources
            T = kinds.horizon
            cap = T * (kinds.n_dynamics + kinds.n_costs + kinds.n_constraints)
            plan, sel = _ffi.StagePlan(), (C.c_double * max(cap, 1))()
            sd, ad = (C.c_int32 * T)(), (C.c_int32 * max(T - 1, 1))()
            reg, path = C.create_string_buffer(160), C.create_string_buffer(1024)
            _ffi.check(L.ilqr_compile_model_stages(name.encode(), C.byref(kinds), source if isinstance(source, bytes) else source.encode(),
                                                   C.byref(plan), sel, cap, sd, ad, reg, 160, path, 1024))
            S = plan.n_selectors
            self._selectors = np.array([sel[i] for i in range(T * S)], dtype=np.float64).reshape(T, S)
            self.num_user_parameter = kinds.num_parameter
            self.state_dims, self.action_dims = list(sd), list(ad)[:T - 1]
            self.constraint_rows = [[plan.constraint_row0[kinds.constraint_of_step[t]] + i
                                     for i in range(kinds.constraint_nc[kinds.constraint_of_step[t]])] if kinds.n_constraints else []
                                    for t in range(T - 1)]
            model, model_library = reg.value.decode(), path.value.decode()
            horizon = T
            constrained = True if constraints is None else bool(constraints)
        elif model is None:
            T = len(costs)
            low = lowering.lower(dynamics, costs, constraints)       # distinct per-step objects -> one stage template
            self._selectors = low["selectors"]
            self.num_user_parameter = low["num_user_parameter"]
            self.constraint_rows = low["constraint_rows"]
            self.state_dims, self.action_dims = low["state_dims"], low["action_dims"]
            model, model_library = compile_model(name, low["dynamics"], low["cost_stage"], low["cost_term"],
                                                 low["con_stage"], low["con_term"])
            horizon = T
            constrained = constraints is not None
        else:
            constrained = True if constraints is None else bool(constraints)
        self.model, self.T, self.B = model, int(horizon), int(batch)
        desc = _ffi.ProblemDesc(model.encode(), model_library.encode() if model_library else None,
                                self.T, self.B, device, 1 if constrained else 0)
        h = C.c_void_p()
        self.devices = None if devices is None else [int(d) for d in devices]
        if self.devices is None:
            _ffi.check(L.ilqr_create(C.byref(desc), C.byref(h)))
        else:
            arr = (C.c_int32 * len(self.devices))(*self.devices)
            _ffi.check(L.ilqr_create_sharded(C.byref(desc), arr, len(self.devices), C.byref(h)))
        self._h = h
        d = [C.c_int32() for _ in range(7)]
        _ffi.check(L.ilqr_get_dims(self._h, *[C.byref(v) for v in d]))
        self.nx, self.nu, self.nw, self.nc_stage, self.nc_term = [v.value for v in d[:5]]
        self.options = options if options is not None else Options()
        _ffi.check(L.ilqr_set_options(self._h, C.byref(self.options)))
        if self._selectors is None or self._selectors.shape[1] == 0:
            self._selectors, self.num_user_parameter = None, self.nw
        else:      # time-varying stage objects: the handle keeps the selector table and writes it behind the user's parameters in θ_t
            sel = np.ascontiguousarray(self._selectors, dtype=np.float64)
            _ffi.check(L.ilqr_set_stage_selectors(self._h, _p(sel), sel.shape[1]))
            self.nw -= sel.shape[1]             # what ilqr_get_dims reports from here on: the user's parameters per timestep

    # -- src/solver.jl:56-66
    def initialize_controls_(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.B, self.T - 1, self.nu)
        _ffi.check(_ffi.lib().ilqr_initialize_controls(self._h, _p(u)))

    def initialize_states_(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.B, self.T, self.nx)
        _ffi.check(_ffi.lib().ilqr_initialize_states(self._h, _p(x)))

    def initialize_rollout_(self, x1, u):
        """x̄ = rollout(dynamics, x1, ū); initialize_controls!; initialize_states! on the device."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(self.B, self.nx)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(self.B, self.T - 1, self.nu)
        _ffi.check(_ffi.lib().ilqr_initialize_rollout(self._h, _p(x1), _p(u)))

    def initialize_rollout_device_(self, d_x1_ptr, d_u_ptr):
        _ffi.check(_ffi.lib().ilqr_initialize_rollout_device(self._h, C.c_void_p(d_x1_ptr), C.c_void_p(d_u_ptr)))

    def initialize_rollout_resident_(self):
        """initialize_rollout_ again from the inputs the handle keeps in HBM since the last call with host arrays (works on a
        handle that spans several devices, where device pointers of one device make no sense)."""
        _ffi.check(_ffi.lib().ilqr_initialize_rollout_resident(self._h))

    def initialize_rollout_candidates_(self, x1, u, violation_weight=0.0):
        """initialize_rollout_ from the best of S candidate action sequences per instance (ilqr_initialize_rollout_candidates):
        x1 [B, nx], u [B, S, T-1, nu]. Every candidate is rolled out and scored on the device, score = cost (+ violation_weight ·
        max_violation); the eligible candidate (finite score, no non-finite state) with the lowest score, ties to the lowest
        index, is installed exactly as initialize_rollout_(x1, u[:, chosen]) would install it. Returns a dict with chosen [B]
        (−1: nobody eligible, candidate 0 installed), cost, max_violation and first_nonfinite [B, S]."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(self.B, self.nx)
        u = np.ascontiguousarray(u, dtype=np.float64)
        per = (self.T - 1) * self.nu
        if u.ndim < 2 or u.shape[0] != self.B or u.size == 0 or u.size % (self.B * per) != 0:
            raise ValueError("u must have shape [B, S, T-1, nu]")
        S = u.size // (self.B * per)
        u = u.reshape(self.B, S, self.T - 1, self.nu)
        i32 = C.POINTER(C.c_int32)
        out = dict(chosen=np.empty(self.B, dtype=np.int32), cost=np.empty((self.B, S)), max_violation=np.empty((self.B, S)),
                   first_nonfinite=np.empty((self.B, S), dtype=np.int32))
        _ffi.check(_ffi.lib().ilqr_initialize_rollout_candidates(self._h, S, float(violation_weight), _p(x1), _p(u), out["chosen"].ctypes.data_as(i32),
                                                                 _p(out["cost"]), _p(out["max_violation"]), out["first_nonfinite"].ctypes.data_as(i32)))
        return out

    def initialize_rollout_candidates_device_(self, candidates, d_x1_ptr, d_u_ptr, violation_weight=0.0, d_chosen_ptr=None, d_cost_ptr=None,
                                              d_max_violation_ptr=None, d_first_nonfinite_ptr=None):
        """The same with raw device pointers on the handle's device (None = not wanted); asynchronous on the handle's stream."""
        _ffi.check(_ffi.lib().ilqr_initialize_rollout_candidates_device(self._h, int(candidates), float(violation_weight), _vp(d_x1_ptr), _vp(d_u_ptr),
                                                                        _vp(d_chosen_ptr), _vp(d_cost_ptr), _vp(d_max_violation_ptr), _vp(d_first_nonfinite_ptr)))

    _SAMPLE_MODES = {"pick": 0, "blend": 1}

    def _sample_arguments(self, sigma, candidates, mode):
        if mode not in self._SAMPLE_MODES:
            raise ValueError('mode must be "pick" or "blend"')
        sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (self.nu,)))
        return sigma, int(candidates), self._SAMPLE_MODES[mode]

    def sample_rollout_candidates_(self, sigma, candidates, seed=0, mode="pick", temperature=1.0, violation_weight=0.0, x1=None, base_u=None,
                                   first_instance=0, return_candidates=False):
        """initialize_rollout_ from candidates drawn on the device around a base sequence (ilqr_sample_rollout_candidates): candidate 0
        is base_u [B, T-1, nu] itself, candidate s >= 1 is base_u + sigma[j] · z with z = candidate_noise(seed, first_instance + b, s, t, j).
        x1 / base_u = None: the handle's resident inputs (after shift_horizon_: the shifted start and guess). Scores and choice as
        initialize_rollout_candidates_; mode="pick" installs the winner, mode="blend" base_u + sigma · Σ_s w_s z_s with the softmin
        weights w_s ∝ exp(−(score_s − score_min) / temperature) over the eligible candidates. Returns a dict with chosen [B], cost,
        max_violation, first_nonfinite, weights [B, S] and, with return_candidates, u [B, S, T-1, nu]: the candidates as drawn."""
        sigma, S, mode = self._sample_arguments(sigma, candidates, mode)
        if x1 is not None:
            x1 = np.ascontiguousarray(x1, dtype=np.float64)
            if x1.shape != (self.B, self.nx):
                raise ValueError("x1 must have shape [B, nx]")
        if base_u is not None:
            base_u = np.ascontiguousarray(base_u, dtype=np.float64)
            if base_u.shape != (self.B, self.T - 1, self.nu):
                raise ValueError("base_u must have shape [B, T-1, nu]")
        if S < 1:
            raise ValueError("candidates must be >= 1")
        i32 = C.POINTER(C.c_int32)
        out = dict(chosen=np.empty(self.B, dtype=np.int32), cost=np.empty((self.B, S)), max_violation=np.empty((self.B, S)),
                   first_nonfinite=np.empty((self.B, S), dtype=np.int32), weights=np.empty((self.B, S)))
        if return_candidates:
            out["u"] = np.empty((self.B, S, self.T - 1, self.nu))
        _ffi.check(_ffi.lib().ilqr_sample_rollout_candidates(
            self._h, S, mode, int(seed), int(first_instance), _p(sigma), float(violation_weight), float(temperature),
            _nul(x1), _nul(base_u), out["chosen"].ctypes.data_as(i32), _p(out["cost"]),
            _p(out["max_violation"]), out["first_nonfinite"].ctypes.data_as(i32), _p(out["weights"]), _p(out["u"]) if return_candidates else None))
        return out

    def sample_rollout_candidates_device_(self, sigma, candidates, seed=0, mode="pick", temperature=1.0, violation_weight=0.0, d_x1_ptr=None,
                                          d_base_u_ptr=None, first_instance=0, d_chosen_ptr=None, d_cost_ptr=None, d_max_violation_ptr=None,
                                          d_first_nonfinite_ptr=None, d_weights_ptr=None, d_u_out_ptr=None):
        """The same with raw device pointers on the handle's device (None = the resident input / not wanted); sigma stays a host
        array; asynchronous on the handle's stream."""
        sigma, S, mode = self._sample_arguments(sigma, candidates, mode)
        _ffi.check(_ffi.lib().ilqr_sample_rollout_candidates_device(
            self._h, S, mode, int(seed), int(first_instance), _p(sigma), float(violation_weight), float(temperature), _vp(d_x1_ptr), _vp(d_base_u_ptr),
            _vp(d_chosen_ptr), _vp(d_cost_ptr), _vp(d_max_violation_ptr), _vp(d_first_nonfinite_ptr), _vp(d_weights_ptr), _vp(d_u_out_ptr)))

    _TAILS = {"hold": 0, "zero": 1}

    def _shift_arguments(self, steps, tail):
        steps = int(steps)
        if not 0 <= steps <= self.T - 1:
            raise ValueError("steps must lie in 0 .. T-1")
        if tail not in self._TAILS:
            raise ValueError('tail must be "hold" or "zero"')
        return steps, self._TAILS[tail]

    def shift_horizon_(self, steps=1, x1=None, feedback=False, tail="hold", w_tail=None):
        """Receding-horizon shift on the device (ilqr_shift_horizon): the solved trajectory moves forward by `steps` control periods
        and is installed as initialize_rollout_ would install it. x1 [B, nx]: the measured states (None: x̄_steps). The actions are
        ū_{t+steps}, then the last action held (tail="hold") or 0 ("zero"); with feedback=True the head is the shifted policy run
        closed-loop from x1, u'_t = ū_{t+steps} + K_{t+steps} (x'_t − x̄_{t+steps}). The parameters move with the horizon; their last
        `steps` rows are w_tail [B, steps, num_parameter] or, without it, the last row held. The policy, duals and scalars stay."""
        steps, tail = self._shift_arguments(steps, tail)
        if x1 is not None:
            x1 = np.ascontiguousarray(x1, dtype=np.float64)
            if x1.shape != (self.B, self.nx):
                raise ValueError("x1 must have shape [B, nx]")
        if w_tail is not None:
            w_tail = np.ascontiguousarray(w_tail, dtype=np.float64)
            if self.num_user_parameter > 0 and steps > 0 and w_tail.shape != (self.B, steps, self.num_user_parameter):
                raise ValueError("w_tail must have shape [B, steps, num_parameter]")
        _ffi.check(_ffi.lib().ilqr_shift_horizon(self._h, steps, tail, 1 if feedback else 0, _nul(x1),
                                                 _nul(w_tail)))

    def shift_horizon_device_(self, steps=1, d_x1_ptr=None, feedback=False, tail="hold", d_w_tail_ptr=None):
        """The same with raw device pointers on the handle's device (None = not given); asynchronous on the handle's stream."""
        steps, tail = self._shift_arguments(steps, tail)
        _ffi.check(_ffi.lib().ilqr_shift_horizon_device(self._h, steps, tail, 1 if feedback else 0, _vp(d_x1_ptr), _vp(d_w_tail_ptr)))

    _PENALTIES = {"keep": 0, "reset": 1}

    def _duals_arguments(self, steps, tail, penalty):
        steps, tail = self._shift_arguments(steps, tail)
        if penalty not in self._PENALTIES:
            raise ValueError('penalty must be "keep" or "reset"')
        _ffi.check(_ffi.lib().ilqr_set_options(self._h, C.byref(self.options)))     # ρ0 = options.initial_constraint_penalty
        return steps, tail, self._PENALTIES[penalty]

    def shift_duals_(self, steps=1, tail="hold", penalty="keep"):
        """Receding-horizon shift of the duals and penalties on the device (ilqr_shift_duals), the companion of shift_horizon_:
        λ'_t = λ_{t+steps} for the stage rows that have a source, the last `steps` stage rows get the old last stage row
        (tail="hold") or 0 ("zero"), the terminal rows stay. penalty="keep": ρ moves as λ does (a "zero" tail gets
        options.initial_constraint_penalty); "reset": every entry of ρ becomes options.initial_constraint_penalty. Nothing else of
        the handle changes. Refused on an unconstrained handle and on one that holds no duals yet."""
        _ffi.check(_ffi.lib().ilqr_shift_duals(self._h, *self._duals_arguments(steps, tail, penalty)))

    def shift_duals_device_(self, steps=1, tail="hold", penalty="keep"):
        """The same, asynchronous on the handle's stream; not on a handle that spans several devices."""
        _ffi.check(_ffi.lib().ilqr_shift_duals_device(self._h, *self._duals_arguments(steps, tail, penalty)))

    def solve_warm_(self, sync=True):
        """solve_ with src/solve.jl:95-103 (λ ← 0, ρ ← ρ0) skipped (ilqr_solve_warm): the solve keeps the duals and penalties the
        handle holds — those of the last solve, moved along by shift_duals_, or the caller's own written with set_buffer. Everything
        else is solve_'s: one launch, every kernel variant, outer_iterations counted from 1. Not a reference behaviour. Refused on
        an unconstrained handle and on one that holds no duals yet (after reset_ ρ is not a solve's)."""
        _ffi.check(_ffi.lib().ilqr_set_options(self._h, C.byref(self.options)))
        _ffi.check(_ffi.lib().ilqr_solve_warm(self._h))
        if sync:
            self.synchronize()

    def _plant_arguments(self, steps, sigma_x, w_plant, rows):
        steps = int(steps)
        if not 1 <= steps <= self.T - 1:
            raise ValueError("steps must lie in 1 .. T-1")
        if sigma_x is not None:
            sigma_x = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_x, dtype=np.float64), (self.nx,)))
        if w_plant is not None:
            w_plant = np.ascontiguousarray(w_plant, dtype=np.float64)
            if self.num_user_parameter > 0 and w_plant.shape != (self.B, rows, self.num_user_parameter):
                raise ValueError("w_plant must have shape [B, %d, num_parameter]" % rows)
        return steps, sigma_x, w_plant

    def plant_step_(self, x, steps=1, feedback=False, sigma_x=None, seed=0, first_instance=0, step0=0, w_plant=None, u_min=None, u_max=None):
        """The plant of a closed MPC loop on the device (ilqr_plant_step): the plant states x [B, nx] move on by `steps` control
        periods under the head of the handle's plan, u_i = ū_i, or with feedback=True ū_i + K_i (x − x̄_i); x ← f(x, u_i, w_i), then
        x_j += sigma_x[j] · z with z = candidate_noise(seed, first_instance + b, 1 + j // 16, step0 + i, j % 16). w_plant [B, steps,
        num_parameter]: the plant's own parameters (None: the handle's). Reads the handle; changes none of its state. Returns a dict
        with x [B, steps + 1, nx] (row 0 the input states, the last row the new plant states), u [B, steps, nu] and first_nonfinite [B]
        (−1, or the first step after which a state component is not finite). u_min, u_max [nu] (either may be None): the actuator's
        limits (ilqr_plant_step_limited) — the action, feedback included, is clamped into them before it is applied and recorded in
        u, and the dict gains saturated [B], the number of (step, component) pairs the clamp changed."""
        steps, sigma_x, w_plant = self._plant_arguments(steps, sigma_x, w_plant, int(steps))
        u_min, u_max = _limits(self.nu, u_min, u_max)
        x = np.array(x, dtype=np.float64, order="C")
        if x.shape != (self.B, self.nx):
            raise ValueError("x must have shape [B, nx]")
        out = dict(x=np.empty((self.B, steps + 1, self.nx)), u=np.empty((self.B, steps, self.nu)), first_nonfinite=np.empty(self.B, dtype=np.int32))
        if u_min is not None or u_max is not None:
            out["saturated"] = np.empty(self.B, dtype=np.int32)
            _ffi.check(_ffi.lib().ilqr_plant_step_limited(self._h, steps, 1 if feedback else 0, int(seed), int(first_instance), int(step0),
                                                          _nul(sigma_x), _nul(u_min),
                                                          _nul(u_max), _nul(w_plant),
                                                          _p(x), _p(out["x"]), _p(out["u"]), out["first_nonfinite"].ctypes.data_as(C.POINTER(C.c_int32)),
                                                          out["saturated"].ctypes.data_as(C.POINTER(C.c_int32))))
            return out
        _ffi.check(_ffi.lib().ilqr_plant_step(self._h, steps, 1 if feedback else 0, int(seed), int(first_instance), int(step0),
                                              _nul(sigma_x), _nul(w_plant), _p(x),
                                              _p(out["x"]), _p(out["u"]), out["first_nonfinite"].ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def plant_step_device_(self, d_x_ptr, steps=1, feedback=False, sigma_x=None, seed=0, first_instance=0, step0=0, d_w_plant_ptr=None,
                           d_x_out_ptr=None, d_u_out_ptr=None, d_first_nonfinite_ptr=None, u_min=None, u_max=None, d_saturated_ptr=None):
        """The same with raw device pointers on the handle's device (None = not given / not wanted); d_x_ptr [B, nx] is updated in
        place; sigma_x, u_min and u_max stay host arrays; asynchronous on the handle's stream."""
        steps, sigma_x, _ = self._plant_arguments(steps, sigma_x, None, int(steps))
        u_min, u_max = _limits(self.nu, u_min, u_max)
        if u_min is not None or u_max is not None or d_saturated_ptr:
            _ffi.check(_ffi.lib().ilqr_plant_step_limited_device(self._h, steps, 1 if feedback else 0, int(seed), int(first_instance), int(step0),
                                                                 _nul(sigma_x),
                                                                 _nul(u_min), _nul(u_max),
                                                                 _vp(d_w_plant_ptr), _vp(d_x_ptr), _vp(d_x_out_ptr), _vp(d_u_out_ptr),
                                                                 _vp(d_first_nonfinite_ptr), _vp(d_saturated_ptr)))
            return
        _ffi.check(_ffi.lib().ilqr_plant_step_device(self._h, steps, 1 if feedback else 0, int(seed), int(first_instance), int(step0),
                                                     _nul(sigma_x), _vp(d_w_plant_ptr), _vp(d_x_ptr), _vp(d_x_out_ptr),
                                                     _vp(d_u_out_ptr), _vp(d_first_nonfinite_ptr)))

    def plant_measure_(self, x, step=0, sigma_y=None, seed=0, first_instance=0):
        """What a controller is given of the plant states x [B, nx] (ilqr_plant_measure): y = x where sigma_y is None or zero, else
        y_j = x_j + sigma_y[j] · z with z = candidate_noise(seed, first_instance + b, 5 + j // 16, step, j % 16) — `step` the number of
        plant steps taken when the measurement is made. Reads nothing of the handle's state. Returns y [B, nx]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.B, self.nx):
            raise ValueError("x must have shape [B, nx]")
        sigma_y = _sigma_y(self.nx, sigma_y)
        y = np.empty((self.B, self.nx))
        _ffi.check(_ffi.lib().ilqr_plant_measure(self._h, int(seed), int(first_instance), int(step), _nul(sigma_y),
                                                 _p(x), _p(y)))
        return y

    def plant_measure_device_(self, d_x_ptr, d_y_ptr, step=0, sigma_y=None, seed=0, first_instance=0):
        """The same with raw device pointers on the handle's device (they may be the same array); sigma_y stays a host array;
        asynchronous on the handle's stream."""
        sigma_y = _sigma_y(self.nx, sigma_y)
        _ffi.check(_ffi.lib().ilqr_plant_measure_device(self._h, int(seed), int(first_instance), int(step),
                                                        _nul(sigma_y), C.c_void_p(d_x_ptr), C.c_void_p(d_y_ptr)))

    def _sensor(self, H, r=None, sigma_y=None, per_instance=True):
        """the linear sensor's arrays: H [ny, nx] (or, where allowed, [B, ny, nx]: one per instance), r and sigma_y [ny] (or scalars)"""
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.ndim == 3 and not per_instance:
            raise ValueError("H must have shape [ny, nx] here: one sensor for the batch")
        if H.ndim not in (2, 3) or H.shape[-1] != self.nx or (H.ndim == 3 and H.shape[0] != self.B):
            raise ValueError("H must have shape [ny, nx] or [B, ny, nx]")
        ny = H.shape[-2]
        vec = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (ny,)))
        return H, ny, vec(r), vec(sigma_y)

    def estimate_update_linear_(self, xhat, P, y, H, r, yhat=None):
        """The measurement update of the filter with a linear sensor y = H x + v, v ~ N(0, diag(r)) (ilqr_estimate_update_linear):
        H [ny, nx] shared by the batch or [B, ny, nx] one per instance, ny smaller or larger than nx (<= 64); the rows are taken in one
        after the other, d = P h_jᵀ, s = h_j·d + r[j], ν = y_j − h_j·x̂, x̂ += d ν / s, P −= d dᵀ / s. yhat [B, ny]: the caller's h(x̂) of a
        nonlinear sensor whose Jacobian at x̂ is H — ν is then y_j − ŷ_j − h_j·(x̂ − x̂₀). Returns the dict of estimate_update_:
        xhat, P (new arrays), innovation [B, ny], nis [B], first_bad [B]."""
        H, ny, r, _ = self._sensor(H, r)
        if r is None:
            raise ValueError("r must be given")
        xhat, P = self._estimate_arrays(xhat, P)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.B, ny):
            raise ValueError("y must have shape [B, ny]")
        if yhat is not None:
            yhat = np.ascontiguousarray(yhat, dtype=np.float64)
            if yhat.shape != (self.B, ny):
                raise ValueError("yhat must have shape [B, ny]")
        out = dict(xhat=xhat, P=P, innovation=np.empty((self.B, ny)), nis=np.empty(self.B), first_bad=np.empty(self.B, dtype=np.int32))
        _ffi.check(_ffi.lib().ilqr_estimate_update_linear(self._h, ny, 1 if H.ndim == 3 else 0, _p(H), _p(r), _p(y),
                                                          _nul(yhat), _p(xhat), _p(P), _p(out["innovation"]),
                                                          _p(out["nis"]), _i32p(out["first_bad"])))
        return out

    def estimate_update_linear_device_(self, d_xhat_ptr, d_P_ptr, d_y_ptr, d_H_ptr, ny, r, per_instance_H=False, d_yhat_ptr=None,
                                       d_innovation_ptr=None, d_nis_ptr=None, d_first_bad_ptr=None):
        """The same with raw device pointers on the handle's device (None = not wanted), H among them; r stays a host array;
        asynchronous on the handle's stream."""
        ny = int(ny)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64), (max(ny, 0),)))
        _ffi.check(_ffi.lib().ilqr_estimate_update_linear_device(self._h, ny, 1 if per_instance_H else 0, _vp(d_H_ptr), _p(r), _vp(d_y_ptr),
                                                                 _vp(d_yhat_ptr), _vp(d_xhat_ptr), _vp(d_P_ptr), _vp(d_innovation_ptr), _vp(d_nis_ptr),
                                                                 _vp(d_first_bad_ptr)))

    def plant_measure_linear_(self, x, H, step=0, sigma_y=None, seed=0, first_instance=0):
        """What a linear sensor reads of the plant states x [B, nx] (ilqr_plant_measure_linear): y = H x with H [ny, nx], plus
        sigma_y[j] · z where sigma_y[j] != 0, z = candidate_noise(seed, first_instance + b, 5 + j // 16, step, j % 16) — plant_measure_'s
        stream. Returns y [B, ny]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.B, self.nx):
            raise ValueError("x must have shape [B, nx]")
        H, ny, _, sigma_y = self._sensor(H, None, sigma_y, per_instance=False)
        y = np.empty((self.B, ny))
        _ffi.check(_ffi.lib().ilqr_plant_measure_linear(self._h, int(seed), int(first_instance), int(step), ny, _p(H),
                                                        _nul(sigma_y), _p(x), _p(y)))
        return y

    def plant_measure_linear_device_(self, d_x_ptr, d_y_ptr, d_H_ptr, ny, step=0, sigma_y=None, seed=0, first_instance=0):
        """The same with raw device pointers on the handle's device for x, y and H [ny, nx]; sigma_y stays a host array;
        asynchronous on the handle's stream."""
        ny = int(ny)
        if sigma_y is not None:
            sigma_y = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_y, dtype=np.float64), (max(ny, 0),)))
        _ffi.check(_ffi.lib().ilqr_plant_measure_linear_device(self._h, int(seed), int(first_instance), int(step), ny,
                                                               C.c_void_p(d_H_ptr) if d_H_ptr else None,
                                                               _nul(sigma_y), C.c_void_p(d_x_ptr),
                                                               C.c_void_p(d_y_ptr)))

    def _nl_sensor(self, sensor, s, r=None, sigma_y=None):
        """a compiled sensor's arguments: (name bytes, ny, per_instance_s, s or None, r, sigma_y) — s [ns] shared or [B, ns]"""
        _, ny, ns = sensor_dims(sensor)
        per = 0
        if s is not None:
            s = np.ascontiguousarray(s, dtype=np.float64)
            if s.shape == (self.B, ns) and s.ndim == 2:
                per = 1
            elif s.shape != (ns,):
                raise ValueError("s must have shape [ns] or [B, ns]")
            if ns == 0:
                s = None
        vec = lambda v: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (ny,)))
        return sensor.encode(), ny, per, s, vec(r), vec(sigma_y)

    def sensor_linearise_(self, sensor, x_lin, s=None, x_prior=None):
        """A compiled nonlinear sensor y = h(x, s) (compile_sensor) linearised on the device (ilqr_sensor_linearise) at x_lin [B, nx]:
        returns (H [B, ny, nx] = ∂h/∂x there, yhat [B, ny] = h(x_lin, s)); with x_prior [B, nx], yhat = h + H (x_prior − x_lin), the
        reference output of an iterated filter. s [ns] shared by the batch or [B, ns]."""
        name, ny, per, s, _, _ = self._nl_sensor(sensor, s)
        x_lin = np.ascontiguousarray(x_lin, dtype=np.float64)
        if x_lin.shape != (self.B, self.nx):
            raise ValueError("x_lin must have shape [B, nx]")
        if x_prior is not None:
            x_prior = np.ascontiguousarray(x_prior, dtype=np.float64)
            if x_prior.shape != (self.B, self.nx):
                raise ValueError("x_prior must have shape [B, nx]")
        H, yhat = np.empty((self.B, ny, self.nx)), np.empty((self.B, ny))
        _ffi.check(_ffi.lib().ilqr_sensor_linearise(self._h, name, per, _nul(s), _p(x_lin), _nul(x_prior), _p(H), _p(yhat)))
        return H, yhat

    def sensor_linearise_device_(self, sensor, d_x_lin_ptr, d_H_ptr, d_yhat_ptr, d_s_ptr=None, per_instance_s=False, d_x_prior_ptr=None):
        """The same with raw device pointers on the handle's device, s among them; asynchronous on the handle's stream."""
        _ffi.check(_ffi.lib().ilqr_sensor_linearise_device(self._h, sensor.encode(), 1 if per_instance_s else 0, _vp(d_s_ptr), _vp(d_x_lin_ptr),
                                                           _vp(d_x_prior_ptr), _vp(d_H_ptr), _vp(d_yhat_ptr)))

    def plant_measure_sensor_(self, sensor, x, s=None, step=0, sigma_y=None, seed=0, first_instance=0):
        """What a compiled nonlinear sensor reads of the plant states x [B, nx] (ilqr_plant_measure_sensor): y = h(x, s), plus
        sigma_y[j] · z where sigma_y[j] != 0 — plant_measure_'s stream. Returns y [B, ny]."""
        name, ny, per, s, _, sigma_y = self._nl_sensor(sensor, s, None, sigma_y)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.B, self.nx):
            raise ValueError("x must have shape [B, nx]")
        y = np.empty((self.B, ny))
        _ffi.check(_ffi.lib().ilqr_plant_measure_sensor(self._h, name, per, _nul(s), int(seed), int(first_instance), int(step), _nul(sigma_y),
                                                        _p(x), _p(y)))
        return y

    def plant_measure_sensor_device_(self, sensor, d_x_ptr, d_y_ptr, d_s_ptr=None, per_instance_s=False, step=0, sigma_y=None, seed=0,
                                     first_instance=0):
        """The same with raw device pointers on the handle's device for x, y and s; sigma_y stays a host array; asynchronous on the
        handle's stream."""
        _, ny, _ = sensor_dims(sensor)
        if sigma_y is not None:
            sigma_y = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_y, dtype=np.float64), (ny,)))
        _ffi.check(_ffi.lib().ilqr_plant_measure_sensor_device(self._h, sensor.encode(), 1 if per_instance_s else 0, _vp(d_s_ptr), int(seed),
                                                               int(first_instance), int(step), _nul(sigma_y), _vp(d_x_ptr), _vp(d_y_ptr)))

    def estimate_update_sensor_(self, xhat, P, y, sensor, r, s=None, iterations=1):
        """The measurement update of the extended Kalman filter with a compiled nonlinear sensor (ilqr_estimate_update_sensor): the
        sensor is linearised on the device at the estimate and estimate_update_linear_'s update runs on the result; iterations > 1
        (up to 8): the iterated filter, relinearised at each iteration's estimate and updated from the prior again. Returns the dict of
        estimate_update_: xhat, P (new arrays), innovation [B, ny], nis [B], first_bad [B]."""
        name, ny, per, s, r, _ = self._nl_sensor(sensor, s, r)
        if r is None:
            raise ValueError("r must be given")
        xhat, P = self._estimate_arrays(xhat, P)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.B, ny):
            raise ValueError("y must have shape [B, ny]")
        out = dict(xhat=xhat, P=P, innovation=np.empty((self.B, ny)), nis=np.empty(self.B), first_bad=np.empty(self.B, dtype=np.int32))
        _ffi.check(_ffi.lib().ilqr_estimate_update_sensor(self._h, name, per, _nul(s), int(iterations), _p(r), _p(y), _p(xhat), _p(P),
                                                          _p(out["innovation"]), _p(out["nis"]), _i32p(out["first_bad"])))
        return out

    def estimate_update_sensor_device_(self, d_xhat_ptr, d_P_ptr, d_y_ptr, sensor, r, d_s_ptr=None, per_instance_s=False, iterations=1,
                                       d_innovation_ptr=None, d_nis_ptr=None, d_first_bad_ptr=None):
        """The same with raw device pointers on the handle's device (None = not wanted), s among them; r stays a host array;
        asynchronous on the handle's stream."""
        _, ny, _ = sensor_dims(sensor)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.float64), (ny,)))
        _ffi.check(_ffi.lib().ilqr_estimate_update_sensor_device(self._h, sensor.encode(), 1 if per_instance_s else 0, _vp(d_s_ptr), int(iterations),
                                                                 _p(r), _vp(d_y_ptr), _vp(d_xhat_ptr), _vp(d_P_ptr), _vp(d_innovation_ptr),
                                                                 _vp(d_nis_ptr), _vp(d_first_bad_ptr)))

    def _estimate_arrays(self, xhat, P):
        xhat, P = np.array(xhat, dtype=np.float64, order="C"), np.array(P, dtype=np.float64, order="C")
        if xhat.shape != (self.B, self.nx):
            raise ValueError("xhat must have shape [B, nx]")
        if P.shape != (self.B, self.nx, self.nx):
            raise ValueError("P must have shape [B, nx, nx]")
        return xhat, P

    def estimate_predict_(self, xhat, P, steps=1, feedback=False, u_min=None, u_max=None, q=None):
        """The time update of the extended Kalman filter on the device (ilqr_estimate_predict): the estimates xhat [B, nx] move on by
        `steps` control periods under the head of the handle's plan exactly as plant_step_ moves a state without noise (feedback,
        u_min, u_max as there), and per step P ← F P Fᵀ + diag(q) with F the model's dynamics state Jacobian at the estimate before it
        moves. P [B, nx, nx] symmetric; q [nx] (or a scalar, None = 0). Reads the handle; changes none of its state. Returns (xhat, P),
        new arrays."""
        steps, _, _ = self._plant_arguments(steps, None, None, int(steps))
        u_min, u_max = _limits(self.nu, u_min, u_max)
        _, q, _ = _variances(self.nx, None, q, None)
        xhat, P = self._estimate_arrays(xhat, P)
        _ffi.check(_ffi.lib().ilqr_estimate_predict(self._h, steps, 1 if feedback else 0, _nul(u_min), _nul(u_max), _nul(q), _p(xhat), _p(P)))
        return xhat, P

    def estimate_predict_device_(self, d_xhat_ptr, d_P_ptr, steps=1, feedback=False, u_min=None, u_max=None, q=None):
        """The same with raw device pointers on the handle's device, updated in place; u_min, u_max and q stay host arrays;
        asynchronous on the handle's stream."""
        steps, _, _ = self._plant_arguments(steps, None, None, int(steps))
        u_min, u_max = _limits(self.nu, u_min, u_max)
        _, q, _ = _variances(self.nx, None, q, None)
        _ffi.check(_ffi.lib().ilqr_estimate_predict_device(self._h, steps, 1 if feedback else 0, _nul(u_min), _nul(u_max), _nul(q),
                                                           C.c_void_p(d_xhat_ptr), C.c_void_p(d_P_ptr)))

    def estimate_update_(self, xhat, P, y, r, measured=None):
        """The measurement update of the filter on the device (ilqr_estimate_update): the components j of y [B, nx] with measured[j]
        (None: all) are taken in one after the other, ν = y_j − x̂_j, s = P_jj + r[j], g = P[:, j] / s, x̂ += g ν, P −= g P[j, :]. r [nx]
        (or a scalar): the measurement noise variances. Returns a dict with xhat, P (new arrays), innovation [B, nx], nis [B] and
        first_bad [B] (−1, or the first component whose s was not a finite number > 0 and which was skipped)."""
        measured, _, r = _variances(self.nx, measured, None, r)
        if r is None:
            raise ValueError("r must be given")
        xhat, P = self._estimate_arrays(xhat, P)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (self.B, self.nx):
            raise ValueError("y must have shape [B, nx]")
        out = dict(xhat=xhat, P=P, innovation=np.empty((self.B, self.nx)), nis=np.empty(self.B), first_bad=np.empty(self.B, dtype=np.int32))
        _ffi.check(_ffi.lib().ilqr_estimate_update(self._h, _i32p(measured), _p(r), _p(y), _p(xhat), _p(P), _p(out["innovation"]), _p(out["nis"]),
                                                   _i32p(out["first_bad"])))
        return out

    def estimate_update_device_(self, d_xhat_ptr, d_P_ptr, d_y_ptr, r, measured=None, d_innovation_ptr=None, d_nis_ptr=None, d_first_bad_ptr=None):
        """The same with raw device pointers on the handle's device (None = not wanted); r and measured stay host arrays;
        asynchronous on the handle's stream."""
        measured, _, r = _variances(self.nx, measured, None, r)
        if r is None:
            raise ValueError("r must be given")
        _ffi.check(_ffi.lib().ilqr_estimate_update_device(self._h, _i32p(measured), _p(r), _vp(d_y_ptr), _vp(d_xhat_ptr), _vp(d_P_ptr),
                                                          _vp(d_innovation_ptr), _vp(d_nis_ptr), _vp(d_first_bad_ptr)))

    def plan_covariance_(self, P0, steps=None, feedback=True, q=None, full=False):
        """A state covariance propagated down the handle's plan under its feedback policy (ilqr_plan_covariance): Σ_0 = P0 [B, nx, nx]
        (the lower triangle is read and mirrored), Σ_{t+1} = Φ Σ_t Φᵀ + diag(q) for t = 0 .. steps − 1 with Φ = A + Bm K_t (feedback) or
        A, the model's dynamics Jacobians at the nominal point (x̄_t, ū_t, θ_t). steps=None: T − 1. q [nx] (or a scalar, None = 0).
        Reads the handle; changes none of its state. Returns a dict with sdiag [B, steps + 1, nx] (the diagonals of Σ_0 .. Σ_steps),
        udiag [B, steps, nu] (the variances of the actions, 0 without feedback), P [B, nx, nx] (= Σ_steps), first_nonfinite [B] (−1,
        or the first t with a non-finite entry on the diagonal of Σ_t) and, with full, sigma [B, steps + 1, nx, nx]."""
        S = self.T - 1 if steps is None else int(steps)
        _, q, _ = _variances(self.nx, None, q, None)
        P0 = np.ascontiguousarray(P0, dtype=np.float64)
        if P0.shape != (self.B, self.nx, self.nx):
            raise ValueError("P0 must have shape [B, nx, nx]")
        rows = max(S, 0)
        out = dict(sdiag=np.empty((self.B, rows + 1, self.nx)), udiag=np.empty((self.B, rows, self.nu)), P=np.empty((self.B, self.nx, self.nx)),
                   first_nonfinite=np.empty(self.B, dtype=np.int32))
        if full:
            out["sigma"] = np.empty((self.B, rows + 1, self.nx, self.nx))
        _ffi.check(_ffi.lib().ilqr_plan_covariance(self._h, S, 1 if feedback else 0, _nul(q), _p(P0), _p(out["sdiag"]), _p(out["udiag"]),
                                                   _nul(out.get("sigma")), _p(out["P"]), _i32p(out["first_nonfinite"])))
        return out

    def plan_covariance_device_(self, d_P0_ptr, steps=None, feedback=True, q=None, d_sdiag_ptr=None, d_udiag_ptr=None, d_sigma_ptr=None,
                                d_P_out_ptr=None, d_first_nonfinite_ptr=None):
        """The same with raw device pointers on the handle's device (None = not wanted; d_P_out_ptr may be d_P0_ptr); q stays a host
        array; asynchronous on the handle's stream."""
        S = self.T - 1 if steps is None else int(steps)
        _, q, _ = _variances(self.nx, None, q, None)
        _ffi.check(_ffi.lib().ilqr_plan_covariance_device(self._h, S, 1 if feedback else 0, _nul(q), _vp(d_P0_ptr), _vp(d_sdiag_ptr), _vp(d_udiag_ptr),
                                                          _vp(d_sigma_ptr), _vp(d_P_out_ptr), _vp(d_first_nonfinite_ptr)))

    def plant_score_(self, x, u, w_plant=None):
        """The score of plant steps on the device (ilqr_plant_score): the realised stage cost and constraint violation of the states a
        plant visited and the actions it applied, x [B, steps + 1, nx] and u [B, steps, nu] as plant_step_ returns them (the last row
        of x is not read), under w_plant [B, steps, num_parameter] or, without it, the handle's θ at horizon positions 0 .. steps − 1.
        To be called while the handle still holds the plan the steps were taken under. Reads the handle; changes none of its state.
        Returns a dict with cost and violation, each [B, steps]; nothing is summed."""
        x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        if u.ndim != 3 or u.shape[0] != self.B or u.shape[2] != self.nu:
            raise ValueError("u must have shape [B, steps, nu]")
        steps, _, w_plant = self._plant_arguments(u.shape[1], None, w_plant, u.shape[1])
        if x.shape != (self.B, steps + 1, self.nx):
            raise ValueError("x must have shape [B, steps + 1, nx]")
        out = dict(cost=np.empty((self.B, steps)), violation=np.empty((self.B, steps)))
        _ffi.check(_ffi.lib().ilqr_plant_score(self._h, steps, _nul(w_plant), _p(x), _p(u), _p(out["cost"]),
                                               _p(out["violation"])))
        return out

    def plant_score_device_(self, steps, d_x_ptr, d_u_ptr, d_cost_ptr, d_violation_ptr=None, d_w_plant_ptr=None):
        """The same with raw device pointers on the handle's device (None = not given / not wanted); asynchronous on the handle's
        stream."""
        _ffi.check(_ffi.lib().ilqr_plant_score_device(self._h, int(steps), _vp(d_w_plant_ptr), _vp(d_x_ptr), _vp(d_u_ptr), _vp(d_cost_ptr),
                                                      _vp(d_violation_ptr)))

    def mpc_run_(self, periods, steps=1, x0=None, plant_feedback=False, shift_feedback=False, shift_tail="hold", warm=True, duals_tail="hold",
                 duals_penalty="keep", sigma_x=None, seed=0, first_instance=0, w_plant=None, w_preview=None, score=False, u_min=None, u_max=None,
                 sigma_y=None, delay=0, estimator=None):
        """The closed MPC loop, enqueued once and synchronised once (ilqr_mpc_run): for each of `periods` re-solves plant_step_(steps)
        on a plant state that stays on the device, shift_horizon_(steps, x1 = the plant state), and shift_duals_ + solve_warm_ (warm)
        or solve_. x0 [B, nx]: the first plant state (None: x̄_0 of the handle); w_plant [B, periods · steps, num_parameter]. Returns an
        MpcResult with x [B, periods · steps + 1, nx], u [B, periods · steps, nu], log (a dict of [B, periods] arrays with the fields of
        stats(), per re-solve) and first_nonfinite [B] (−1, or the global plant step after which a state was not finite).
        w_preview [B, periods · steps, num_parameter]: the parameter rows that enter the horizon, `steps` of them per period, as
        shift_horizon_'s w_tail (None: the last row held). score=True: plant_score_ of every period's steps, taken before the shift,
        as cl_cost and cl_violation [B, periods · steps] of the result. Either goes through ilqr_mpc_run_preview.
        u_min, u_max [nu]: the actuator's limits, as plant_step_'s; sigma_y [nx]: measurement noise, as plant_measure_'s, on the plant
        state the shift is handed; delay=1: the re-solve is anchored at a one-period model prediction from a measurement one period
        old (the solve takes a period), instead of at a measurement of the state it is applied from. Any of them goes through
        ilqr_mpc_run_io, and the result carries y_cl [B, periods, nx], what the controller was given, and saturated [B].
        estimator = dict(r=, q=None, measured=None, xhat0=None, P0=): an extended Kalman filter between the measurement and the
        controller (ilqr_mpc_run_est) — estimate_predict_ under the plan in flight and estimate_update_ with the period's measurement, in
        the order `delay` sets; the re-solve is anchored at the estimate. xhat0 [B, nx] (None: the first plant state), P0 [B, nx, nx].
        The result carries xhat, pdiag, nis and the last covariance P; y_cl is then the measurement taken.
        estimator = dict(H=, r=, q=None, xhat0=None, P0=, sigma_y=None): the same loop with the linear sensor y = H x + v of
        plant_measure_linear_ / estimate_update_linear_ (ilqr_mpc_run_sensor), selected by the key H [ny, nx]; r and sigma_y have ny
        entries, y_cl is [B, periods, ny]. Not together with `measured` or with the loop's own sigma_y.
        estimator = dict(sensor=, r=, s=None, q=None, xhat0=None, P0=, sigma_y=None, iterations=1): the same loop with a compiled
        nonlinear sensor y = h(x, s) (compile_sensor; ilqr_mpc_run_nlsensor), selected by the key sensor: plant_measure_sensor_ and
        estimate_update_sensor_ in the places of the linear ones; s [ns] or [B, ns]. Not together with H or `measured`."""
        periods = int(periods)
        if periods < 1:
            raise ValueError("periods must be >= 1")
        if delay not in (0, 1):
            raise ValueError("delay must be 0 or 1")
        u_min, u_max = _limits(self.nu, u_min, u_max)
        sigma_y = _sigma_y(self.nx, sigma_y)
        io = u_min is not None or u_max is not None or sigma_y is not None or delay == 1
        # the kind of estimator is named by one key: sensor (compiled nonlinear), H (linear), else the selection of state components
        nonlinear = estimator is not None and "sensor" in estimator
        linear = estimator is not None and not nonlinear and "H" in estimator
        if estimator is not None:
            common = {"q", "r", "xhat0", "P0"}
            allowed = common | ({"sensor", "s", "sigma_y", "iterations"} if nonlinear else {"H", "sigma_y"} if linear else {"measured"})
            if nonlinear and ("H" in estimator or "measured" in estimator):
                raise ValueError("estimator: sensor excludes H and measured")
            if linear and "measured" in estimator:
                raise ValueError("estimator: H and measured exclude each other")
            unknown = set(estimator) - allowed
            if unknown:
                raise ValueError("estimator: unknown keys %s" % sorted(unknown))
            if (linear or nonlinear) and sigma_y is not None:
                raise ValueError("estimator: with a sensor (H or sensor) the sensor's own sigma_y [ny] replaces the loop's")
            if estimator.get("r") is None or estimator.get("P0") is None:
                raise ValueError("estimator needs r and P0")
            if nonlinear:
                e_name, e_ny, e_per, e_s, e_r, e_sigma = self._nl_sensor(estimator["sensor"], estimator.get("s"), estimator["r"], estimator.get("sigma_y"))
                _, e_q, _ = _variances(self.nx, None, estimator.get("q"), None)
            elif linear:
                e_H, e_ny, e_r, e_sigma = self._sensor(estimator["H"], estimator["r"], estimator.get("sigma_y"), per_instance=False)
                _, e_q, _ = _variances(self.nx, None, estimator.get("q"), None)
            else:
                e_measured, e_q, e_r = _variances(self.nx, estimator.get("measured"), estimator.get("q"), estimator["r"])
            e_P = np.array(estimator["P0"], dtype=np.float64, order="C")
            if e_P.shape != (self.B, self.nx, self.nx):
                raise ValueError("P0 must have shape [B, nx, nx]")
            e_xhat0 = estimator.get("xhat0")
            if e_xhat0 is not None:
                e_xhat0 = np.ascontiguousarray(e_xhat0, dtype=np.float64)
                if e_xhat0.shape != (self.B, self.nx):
                    raise ValueError("xhat0 must have shape [B, nx]")
        steps, sigma_x, w_plant = self._plant_arguments(steps, sigma_x, w_plant, periods * int(steps))
        if w_preview is not None:
            w_preview = np.ascontiguousarray(w_preview, dtype=np.float64)
            if self.num_user_parameter > 0 and w_preview.shape != (self.B, periods * steps, self.num_user_parameter):
                raise ValueError("w_preview must have shape [B, %d, num_parameter]" % (periods * steps))
        for name, val, table in (("shift_tail", shift_tail, self._TAILS), ("duals_tail", duals_tail, self._TAILS), ("duals_penalty", duals_penalty, self._PENALTIES)):
            if val not in table:
                raise ValueError("%s must be one of %s" % (name, sorted(table)))
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            if x0.shape != (self.B, self.nx):
                raise ValueError("x0 must have shape [B, nx]")
        _ffi.check(_ffi.lib().ilqr_set_options(self._h, C.byref(self.options)))
        d = _ffi.MpcDesc(periods, steps, 1 if plant_feedback else 0, 1 if shift_feedback else 0, self._TAILS[shift_tail], 1 if warm else 0,
                         self._TAILS[duals_tail], self._PENALTIES[duals_penalty], int(seed), int(first_instance),
                         _nul(sigma_x))
        R = periods * steps
        x, u = np.empty((self.B, R + 1, self.nx)), np.empty((self.B, R, self.nu))
        log, nf = np.empty((self.B, periods, _ffi.MPC_LOG_W)), np.empty(self.B, dtype=np.int32)
        cl_cost, cl_violation = (np.empty((self.B, R)), np.empty((self.B, R))) if score else (None, None)
        y_cl = saturated = xhat = pdiag = nis = None
        plant, preview = (_nul(x0), _nul(w_plant)), (_nul(w_preview),)
        out, scores = (_p(x), _p(u), _p(log), _i32p(nf)), (_nul(cl_cost), _nul(cl_violation))
        if estimator is not None or io:
            pio = _ffi.PlantIO(_nul(u_min), _nul(u_max), _nul(sigma_y), int(delay), 0)
            y_cl, saturated = np.empty((self.B, periods, e_ny if (linear or nonlinear) else self.nx)), np.empty(self.B, dtype=np.int32)
            seam = (_p(y_cl), _i32p(saturated))
        # the plainest entry point that offers what was asked for, and its arguments behind the handle and the descriptor
        if estimator is not None:
            xhat, pdiag, nis = np.empty((self.B, periods, self.nx)), np.empty((self.B, periods, self.nx)), np.empty((self.B, periods))
            if nonlinear:
                run, est = _ffi.lib().ilqr_mpc_run_nlsensor, _ffi.NlSensor(e_name, e_per, _nul(e_s), _p(e_r), _nul(e_q), _nul(e_sigma),
                                                                             int(estimator.get("iterations", 1)))
            elif linear:
                run, est = _ffi.lib().ilqr_mpc_run_sensor, _ffi.Sensor(e_ny, 0, _p(e_H), _p(e_r), _nul(e_q), _nul(e_sigma))
            else:
                run, est = _ffi.lib().ilqr_mpc_run_est, _ffi.Estimator(_i32p(e_measured), _nul(e_q), _p(e_r))
            args = ((C.byref(pio), C.byref(est), _nul(x0), _nul(e_xhat0), _p(e_P), _nul(w_plant)) + preview + out + scores + seam
                    + (_p(xhat), _p(pdiag), _p(nis)))
        elif io:
            run, args = _ffi.lib().ilqr_mpc_run_io, (C.byref(pio),) + plant + preview + out + scores + seam
        elif w_preview is not None or score:
            run, args = _ffi.lib().ilqr_mpc_run_preview, plant + preview + out + scores
        else:
            run, args = _ffi.lib().ilqr_mpc_run, plant + out
        _ffi.check(run(self._h, C.byref(d), *args))
        ints = ("iterations", "outer_iterations", "status", "potrf_info", "rollouts")
        return MpcResult(x, u, {f: (log[:, :, c].astype(np.int32) if f in ints else log[:, :, c].copy()) for c, f in enumerate(_ffi.MPC_LOG_COLUMNS)},
                         nf, cl_cost, cl_violation, y_cl, saturated, xhat, pdiag, nis, e_P if estimator is not None else None)

    def set_parameters_(self, w):
        """Solver(...; parameters=θ): w[b, t] is the parameter vector of timestep t of instance b."""
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(self.B, self.T, self.num_user_parameter)
        _ffi.check(_ffi.lib().ilqr_set_parameters(self._h, _p(w)))      # (selector columns of a lowered problem are the library's)

    def reset_(self):
        _ffi.check(_ffi.lib().ilqr_reset(self._h))

    # -- src/solve.jl:137-143
    def solve_(self, sync=True, augmented_lagrangian_callback_=None):
        """solve!(solver; augmented_lagrangian_callback!) — src/solve.jl:88-129,137-143.

        Without a callback the whole AL/iLQR solve is ONE kernel launch. With a callback the outer AL
        loop is stepped from the host (one launch per outer iteration) and `callback(solver)` runs after
        each dual update exactly where the reference calls it (src/solve.jl:125), e.g. for continuation
        on the parameters."""
        _ffi.check(_ffi.lib().ilqr_set_options(self._h, C.byref(self.options)))
        verbose = bool(self.options.verbose) and augmented_lagrangian_callback_ is None
        if verbose and not getattr(self, "_trace_cap", 0):     # options.verbose: the per-iteration report of src/solve.jl:39-44
            self.enable_trace_(int(self.options.max_iterations) * max(1, int(self.options.max_dual_updates)))
        if augmented_lagrangian_callback_ is None:
            _ffi.check(_ffi.lib().ilqr_solve(self._h))
            if sync or verbose:
                self.synchronize()
            if verbose:
                self.print_trace()
            return
        self.run_stage_("al_begin")
        for _ in range(int(self.options.max_dual_updates)):
            self.run_stage_("al_outer")
            if bool((self.buffer("_scalars")[:, _ffi.lib().ilqr_scalar_slot(b"done")] != 0.0).all()):   # every instance met the tolerance
                break
            augmented_lagrangian_callback_(self)

    def run_stage_param_(self, stage, param, flag):
        _ffi.check(_ffi.lib().ilqr_set_options(self._h, C.byref(self.options)))
        _ffi.check(_ffi.lib().ilqr_run_stage_param(self._h, _ffi.STAGES[stage], float(param), int(flag)))

    def solve_shared_step_(self, allreduce_sum=None):
        """solve! with ONE step size per inner iteration for the whole batch (all ranks): the optional mode of the north
        star, not a reference behaviour — the reference line-searches every Solver on its own. forward_pass!'s Armijo loop
        (src/forward_pass.jl:26-52) runs on the host over the SUMMED merit: per trial one all-reduce of three doubles
        (Σ J(α), Σ J_prev, Σ ∇Lᵀ·Δz over the instances still in their inner loop) — `allreduce_sum(np.ndarray) -> np.ndarray`,
        e.g. distributed.torch_allreduce_sum(dist, device) for RCCL; identity on one rank. Everything else (linearisation,
        Riccati pass, convergence tests, dual updates) stays per instance on the device. With a batch of one instance it
        reproduces solve_ exactly. Constrained solvers only. Returns the list of accepted step sizes.
        The loop itself lives in the library (ilqr_solve_shared_step: a Julia or C host passes its RCCL / MPI reducer as a C
        callback); this method only wraps `allreduce_sum` into that callback."""
        L = _ffi.lib()
        _ffi.check(L.ilqr_set_options(self._h, C.byref(self.options)))
        cb = None
        if allreduce_sum is not None:
            def reduce(values, n, _ctx):
                try:
                    v = np.ctypeslib.as_array(values, shape=(n,))
                    v[:] = np.asarray(allreduce_sum(v.copy()), dtype=np.float64)
                    return 0
                except Exception:                  # nothing may propagate through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = _ffi.ALLREDUCE_SUM_FN(reduce)
        cap = int(self.options.max_dual_updates) * int(self.options.max_iterations)
        steps = np.zeros(max(cap, 1)); n = C.c_int32(0)
        _ffi.check(L.ilqr_solve_shared_step(self._h, C.cast(cb, C.c_void_p) if cb is not None else None, None, _p(steps), cap, C.byref(n)))
        return [float(a) for a in steps[:n.value]]

    def synchronize(self):
        _ffi.check(_ffi.lib().ilqr_synchronize(self._h))

    def run_stage_(self, stage):
        _ffi.check(_ffi.lib().ilqr_set_options(self._h, C.byref(self.options)))
        _ffi.check(_ffi.lib().ilqr_run_stage(self._h, _ffi.STAGES[stage]))

    # -- src/solver.jl:48-50
    def get_trajectory(self):
        x = np.empty((self.B, self.T, self.nx)); u = np.empty((self.B, self.T - 1, self.nu))
        _ffi.check(_ffi.lib().ilqr_get_trajectory(self._h, _p(x), _p(u)))
        return x, u

    def get_policy(self):
        """(K, k): K[b, t] is the nu×nx gain as a [nx][nu] column-major block."""
        K = np.empty((self.B, self.T - 1, self.nx, self.nu)); k = np.empty((self.B, self.T - 1, self.nu))
        _ffi.check(_ffi.lib().ilqr_get_policy(self._h, _p(K), _p(k)))
        return K, k

    def rollout_policy(self, x1, w=None, step_size=0.0, trajectories=False):
        """Closed-loop rollouts of the current policy from x1[b, s] (ilqr_rollout_policy): u_t = ū_t + K_t (x_t − x̄_t) + step_size k_t,
        S samples per instance, optionally under the samples' own parameters w[b, s, t]. Returns a dict with cost [B, S] (the plain
        objective), max_violation [B, S], first_nonfinite [B, S] (−1, or the first 0-based t with a non-finite state) and, with
        trajectories=True, x [B, S, T, nx] and u [B, S, T-1, nu]. Reads the handle; changes none of its state."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        if x1.ndim < 2 or x1.shape[0] != self.B or x1.size % (self.B * self.nx) != 0:
            raise ValueError("x1 must have shape [B, S, nx]")
        S = x1.size // (self.B * self.nx)
        x1 = x1.reshape(self.B, S, self.nx)
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if self.nw > 0:
                w = w.reshape(self.B, S, self.T, self.nw)
        out = dict(cost=np.empty((self.B, S)), max_violation=np.empty((self.B, S)), first_nonfinite=np.empty((self.B, S), dtype=np.int32))
        if trajectories:
            out["x"] = np.empty((self.B, S, self.T, self.nx)); out["u"] = np.empty((self.B, S, self.T - 1, self.nu))
        _ffi.check(_ffi.lib().ilqr_rollout_policy(self._h, S, float(step_size), _p(x1), _nul(w), _p(out["cost"]),
                                                  _p(out["max_violation"]), out["first_nonfinite"].ctypes.data_as(C.POINTER(C.c_int32)),
                                                  _p(out["x"]) if trajectories else None, _p(out["u"]) if trajectories else None))
        return out

    def rollout_policy_device(self, samples, d_x1_ptr, d_cost_ptr, d_w_ptr=None, step_size=0.0, d_max_violation_ptr=None,
                              d_first_nonfinite_ptr=None, d_x_ptr=None, d_u_ptr=None):
        """The same with raw device pointers on the handle's device (None = not wanted); asynchronous on the handle's stream."""
        _ffi.check(_ffi.lib().ilqr_rollout_policy_device(self._h, int(samples), float(step_size), _vp(d_x1_ptr), _vp(d_w_ptr), _vp(d_cost_ptr),
                                                         _vp(d_max_violation_ptr), _vp(d_first_nonfinite_ptr), _vp(d_x_ptr), _vp(d_u_ptr)))

    def stream_ptr(self):
        """The handle's HIP stream as an integer (ilqr_get_stream), e.g. for torch.cuda.ExternalStream; not on a sharded handle."""
        s = C.c_void_p()
        _ffi.check(_ffi.lib().ilqr_get_stream(self._h, C.byref(s)))
        return s.value or 0

    def stats(self):
        st = (_ffi.Stats * self.B)()
        _ffi.check(_ffi.lib().ilqr_get_stats(self._h, st))
        return {f: np.array([getattr(s, f) for s in st]) for f, _ in _ffi.Stats._fields_ if f != "reserved"}

    def enable_action_value_buffers_(self):
        """Have the backward-pass stage also store policy.action_value.* (Qx, Qu, Qxx, Quu, Qux) to HBM."""
        _ffi.check(_ffi.lib().ilqr_enable_action_value_buffers(self._h))

    def scalar(self, name):
        """One named SolverData scalar per instance (see ilqr_scalar_slot), e.g. "delta_grad_product"."""
        i = _ffi.lib().ilqr_scalar_slot(name.encode())
        if i < 0:
            raise KeyError(name)
        return self.buffer("_scalars")[:, i]

    def buffer(self, name):
        n = C.c_size_t(0)
        _ffi.check(_ffi.lib().ilqr_buffer_len(self._h, name.encode(), C.byref(n)))
        out = np.empty((self.B, n.value))
        if n.value:
            _ffi.check(_ffi.lib().ilqr_get_buffer(self._h, name.encode(), _p(out)))
        return out

    def set_buffer(self, name, values):
        n = C.c_size_t(0)
        _ffi.check(_ffi.lib().ilqr_buffer_len(self._h, name.encode(), C.byref(n)))
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(self.B, n.value)
        if n.value:
            _ffi.check(_ffi.lib().ilqr_set_buffer(self._h, name.encode(), _p(v)))

    def set_kernel_variant_(self, variant):
        """"auto" | "latency" | "throughput" | "packed" | "mid" | "packed1" | "packed2" (see ilqr_set_kernel_variant)."""
        v = {"auto": 0, "latency": 1, "throughput": 2, "packed": 3, "mid": 4, "packed1": 5, "packed2": 6}.get(variant, variant)
        _ffi.check(_ffi.lib().ilqr_set_kernel_variant(self._h, int(v)))

    def resolved_kernel_variant(self):
        """The kernel solve_ launches for this handle as it stands: "latency" | "throughput" | "mid" | "packed1" | "packed2"."""
        v = C.c_int32(0)
        _ffi.check(_ffi.lib().ilqr_resolved_kernel_variant(self._h, C.byref(v)))
        return {1: "latency", 2: "throughput", 4: "mid", 5: "packed1", 6: "packed2"}[v.value]

    def set_handover_(self, outer):
        """Straggler hand-over of the packed kernel (see ilqr_set_handover): -1 auto (by head count), 0 off, k >= 2 = instances entering outer iteration k."""
        _ffi.check(_ffi.lib().ilqr_set_handover(self._h, int(outer)))

    def set_handover_live_(self, live):
        """Hand-over by head count (see ilqr_set_handover_live): -1 auto, 0 off, n = survivors of the batch at which they all leave."""
        _ffi.check(_ffi.lib().ilqr_set_handover_live(self._h, int(live)))

    def set_handover_mark_(self, rejected):
        """Early leave of stragglers (see ilqr_set_handover_mark): -1 auto, 0 never, n = rejected line-search trials above the batch's mean."""
        _ffi.check(_ffi.lib().ilqr_set_handover_mark(self._h, int(rejected)))

    def handover_stats(self):
        """(instances the packed kernel's workgroups took from their queue, instances marked as stragglers) of the last solve_."""
        q = C.c_int32(0); m = C.c_int32(0)
        _ffi.check(_ffi.lib().ilqr_get_handover_stats(self._h, C.byref(q), C.byref(m)))
        return q.value, m.value

    def enable_trace_(self, capacity):
        """Record per-iteration rows (what `verbose` prints in the reference) during solve_."""
        self._trace_cap = int(capacity)
        _ffi.check(_ffi.lib().ilqr_enable_trace(self._h, self._trace_cap))

    def trace(self):
        """[B, capacity, 8]: outer, inner, objective, gradient_norm, max_violation, step_size, status, rollouts."""
        out = np.zeros((self.B, self._trace_cap, 8))
        _ffi.check(_ffi.lib().ilqr_get_trace(self._h, _p(out)))
        return out

    def print_trace(self, instance=0):
        """What the reference prints per inner iteration when options.verbose (src/solve.jl:39-44), for one instance."""
        rows = self.trace()[instance][:int(self.scalar("trace_len")[instance])]
        for outer, inner, J, g, v, a, status, _ in rows:
            print("iter:                  %d\n"
                  "             cost:                  %r\n"
                  "\t\t\t gradient_norm:         %r\n"
                  "\t\t\t max_violation:         %r\n"
                  "\t\t\t step_size:             %r" % (int(inner), float(J), float(g), float(v), float(a)))

    def timing(self):
        ms = C.c_double(0); nl = C.c_int32(0)
        _ffi.check(_ffi.lib().ilqr_timing_get(self._h, C.byref(ms), C.byref(nl)))
        return ms.value, nl.value

    def timing_reset(self):
        _ffi.check(_ffi.lib().ilqr_timing_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().ilqr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# free-function spellings of the reference's exports (src/IterativeLQR.jl:40-45)
def candidate_noise(seed, batch, candidates, steps, nu, first_instance=0):
    """z [batch, candidates, steps, nu] of the candidates Solver.sample_rollout_candidates_ draws (ilqr_candidate_noise): the host twin
    of the device's generator, a pure function of (seed, first_instance + b, s, t, j); row s = 0 is zero. Needs no device."""
    z = np.empty((int(batch), int(candidates), int(steps), int(nu)))
    _ffi.check(_ffi.lib().ilqr_candidate_noise(int(seed), int(first_instance), int(batch), int(candidates), int(steps), int(nu), _p(z)))
    return z


def initialize_controls_(solver, u):
    solver.initialize_controls_(u)


def initialize_states_(solver, x):
    solver.initialize_states_(x)


def solve_(solver, *args, augmented_lagrangian_callback_=None):
    """solve!(solver[, states, actions]; augmented_lagrangian_callback!) — src/solve.jl:56-60,88,131-135."""
    if args:
        states, actions = args
        solver.initialize_controls_(actions)
        solver.initialize_states_(states)
    solver.solve_(augmented_lagrangian_callback_=augmented_lagrangian_callback_)


def get_trajectory(solver):
    return solver.get_trajectory()
