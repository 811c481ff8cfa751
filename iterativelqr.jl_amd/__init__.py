"""MI355X-native batched iLQR: host-side mirror of IterativeLQR.jl's API over a
C-ABI (include/ilqr_hip.h) into hand-written HIP kernels (csrc/)."""
from . import _ffi, codegen, distributed, lowering, models, workloads  # noqa: F401
from .api import (MpcResult, Options, Solver, candidate_noise, compile_model, compile_sensor, compile_sensor_source,  # noqa: F401
                  get_trajectory, initialize_controls_, initialize_states_, sensor_dims, solve_)
from .codegen import Constraint, Cost, Dynamics  # noqa: F401
