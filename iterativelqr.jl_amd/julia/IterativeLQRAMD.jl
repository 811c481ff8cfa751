# IterativeLQRAMD.jl — Julia host side of the MI355X-native batched iLQR solver.
#
# THIS FILE HAS NEVER RUN. The build image has no Julia (SURVEY.md §0), so nothing below has been parsed, let alone
# executed: the `ccall` signatures are written against include/ilqr_hip.h by hand, and the Symbolics calls
# (`build_function(...; target = CTarget(), fname, lhsname, rhsnames)`) from memory of its documentation. Treat it as the
# sketch of the binding a maintainer of IterativeLQR.jl would add — the same exported names (src/IterativeLQR.jl:30-45) over
# `ccall`s into libilqr_hip.so — not as a tested component. What IS tested is the C-ABI it binds (tests/test_abi.py, the C
# programs under examples/) and the Python twin of this file, iterativelqr.jl_amd/api.py, which drives every entry point
# used here (including ilqr_compile_model_stages / ilqr_set_stage_selectors, through Solver(stage_sources = ...)).
#
# One `Solver` here owns a BATCH of B independent problem instances of one model;
# states are B×T×nx, actions B×(T-1)×nu (row-major on the C side, so Julia arrays
# are passed as (nx, T, B) / (nu, T-1, B) column-major views of the same memory).
module IterativeLQRAMD

export Options, Solver, Dynamics, Cost, Constraint, initialize_controls!, initialize_states!, initialize_rollout!, initialize_rollout_candidates!, sample_rollout_candidates!, candidate_noise, shift_horizon!, shift_duals!, solve_warm!, plant_step!, mpc_run!, MpcDesc, plant_score!, plant_score_device!, mpc_run_preview!, plant_step_limited!, plant_measure!, mpc_run_io!, PlantIO, estimate_predict!, plan_covariance!, plan_covariance_device!, estimate_update!, mpc_run_est!, Estimator, estimate_update_linear!, plant_measure_linear!, mpc_run_sensor!, Sensor,
       set_parameters!, solve!, solve_shared_step!, get_trajectory, get_policy, rollout_policy, stats, set_kernel_variant!, set_handover!, set_handover_live!, set_handover_mark!, enable_trace!, trace,
       compile_sensor, load_sensor_library, sensor_dims, sensor_linearise!, plant_measure_sensor!, estimate_update_sensor!, mpc_run_nlsensor!

import Libdl

const LIB = Ref{String}(joinpath(@__DIR__, "..", "lib", "libilqr_hip.so"))

# Options{T} — src/options.jl:1-15, field for field (C layout of ilqr_options)
Base.@kwdef mutable struct Options
    line_search::Int32 = 1                      # 1 = :armijo, 0 = :none
    max_iterations::Int32 = 100
    max_dual_updates::Int32 = 10
    min_step_size::Float64 = 1.0e-5
    objective_tolerance::Float64 = 1.0e-3
    lagrangian_gradient_tolerance::Float64 = 1.0e-3
    constraint_tolerance::Float64 = 5.0e-3
    constraint_norm::Float64 = Inf
    initial_constraint_penalty::Float64 = 1.0
    scaling_penalty::Float64 = 10.0
    max_penalty::Float64 = 1.0e8
    reset_cache::Int32 = 0
    verbose::Int32 = 0
end

struct ProblemDesc
    model::Cstring
    model_library::Cstring
    horizon::Int32
    batch::Int32
    device::Int32
    constrained::Int32
end

struct Stats
    objective::Float64
    gradient_norm::Float64
    max_violation::Float64
    step_size::Float64
    iterations::Int32
    outer_iterations::Int32
    status::Int32
    potrf_info::Int32
    rollouts::Int32
    reserved::Int32
end

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:ilqr_last_error, LIB[]), Cstring, ()))
    error("ilqr error $rc: $msg")
end

mutable struct Solver
    handle::Ptr{Cvoid}
    nx::Int; nu::Int; T::Int; B::Int
    options::Options
    state_dims::Vector{Int}; action_dims::Vector{Int}     # real entries per step (all nx / nu unless the problem's dimensions vary)
end

"""
    Solver(model; horizon, batch, constrained=true, options=Options(), device=0, devices=Int[], model_library="")

Batched counterpart of `Solver(dynamics, costs, constraints)` (src/solver.jl:28-46).
`model` names a built-in ("acrobot", "car", "particle", ...) or a model compiled by
the code generator (iterativelqr.jl_amd/codegen.py) whose module is `model_library`.
`devices = [0, 1, ..., 7]` spreads the batch over the GPUs of the node (contiguous ranges of
ceil(batch / length(devices)) instances, `ilqr_create_sharded`); every other call is unchanged.
"""
function Solver(model::AbstractString; horizon::Integer, batch::Integer, constrained::Bool=true,
                options::Options=Options(), device::Integer=0, devices::AbstractVector{<:Integer}=Int[],
                model_library::AbstractString="")
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve model model_library begin
        desc = ProblemDesc(Base.unsafe_convert(Cstring, model),
                           isempty(model_library) ? Cstring(C_NULL) : Base.unsafe_convert(Cstring, model_library),
                           Int32(horizon), Int32(batch), Int32(device), Int32(constrained))
        if isempty(devices)
            check(ccall((:ilqr_create, LIB[]), Cint, (Ref{ProblemDesc}, Ref{Ptr{Cvoid}}), desc, h))
        else
            devs = Int32.(collect(devices))
            check(ccall((:ilqr_create_sharded, LIB[]), Cint, (Ref{ProblemDesc}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
                        desc, devs, Int32(length(devs)), h))
        end
    end
    d = [Ref{Int32}(0) for _ in 1:7]
    check(ccall((:ilqr_get_dims, LIB[]), Cint,
                (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}),
                h[], d...))
    s = Solver(h[], d[1][], d[2][], d[6][], d[7][], options, fill(Int(d[1][]), d[6][]), fill(Int(d[2][]), d[6][] - 1))
    finalizer(x -> ccall((:ilqr_destroy, LIB[]), Cint, (Ptr{Cvoid},), x.handle), s)
    return s
end

# initialize_controls!(solver, ū) — src/solver.jl:56-60; ū :: Array{Float64,3} of size (nu, T-1, B)
function initialize_controls!(s::Solver, u::Array{Float64,3})
    @assert size(u) == (s.nu, s.T - 1, s.B)
    check(ccall((:ilqr_initialize_controls, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), s.handle, u))
end

# initialize_states!(solver, x̄) — src/solver.jl:62-66; x̄ :: (nx, T, B)
function initialize_states!(s::Solver, x::Array{Float64,3})
    @assert size(x) == (s.nx, s.T, s.B)
    check(ccall((:ilqr_initialize_states, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), s.handle, x))
end

# x̄ = rollout(dynamics, x1, ū) on the device (src/rollout.jl:33-42) + both initialisers
function initialize_rollout!(s::Solver, x1::Matrix{Float64}, u::Array{Float64,3})
    @assert size(x1) == (s.nx, s.B) && size(u) == (s.nu, s.T - 1, s.B)
    check(ccall((:ilqr_initialize_rollout, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.handle, x1, u))
end

# initialize_rollout! from the best of S candidate action sequences per instance (ilqr_initialize_rollout_candidates):
# u :: (nu, T-1, S, B). Every candidate is rolled out and scored on the device, score = cost (+ violation_weight · max_violation);
# the eligible candidate with the lowest score (ties: lowest index) is installed as initialize_rollout! would install it.
# Returns (chosen, cost, max_violation, first_nonfinite): chosen is 1-based per instance, 0 when no candidate was eligible
# (candidate 1 is installed then); the others are S×B.
function initialize_rollout_candidates!(s::Solver, x1::Matrix{Float64}, u::Array{Float64,4}; violation_weight::Float64 = 0.0)
    @assert size(x1) == (s.nx, s.B) && size(u, 1) == s.nu && size(u, 2) == s.T - 1 && size(u, 4) == s.B
    S = size(u, 3)
    chosen = Vector{Int32}(undef, s.B)
    cost = Array{Float64,2}(undef, S, s.B); viol = Array{Float64,2}(undef, S, s.B); nonfinite = Array{Int32,2}(undef, S, s.B)
    check(ccall((:ilqr_initialize_rollout_candidates, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                s.handle, Int32(S), violation_weight, x1, u, chosen, cost, viol, nonfinite))
    return chosen .+ Int32(1), cost, viol, nonfinite
end

# initialize_rollout! from candidates DRAWN ON THE DEVICE around a base sequence (ilqr_sample_rollout_candidates): candidate 1 is
# base_u :: (nu, T-1, B) itself, candidate s >= 2 is base_u + sigma[j] · z with z = candidate_noise(...) (0-based indices in the key).
# x1 / base_u = nothing: the handle's resident inputs (after shift_horizon!: the shifted start and guess). mode = :pick installs the
# winner, :blend base_u + sigma · Σ_s w_s z_s with the softmin weights w_s ∝ exp(−(score_s − score_min) / temperature). Returns
# (chosen, cost, max_violation, first_nonfinite, weights, u): chosen 1-based, 0 when no candidate was eligible; u :: (nu, T-1, S, B) or
# nothing without return_candidates.
function sample_rollout_candidates!(s::Solver, sigma::Vector{Float64}, candidates::Integer; seed::Integer = 0, mode::Symbol = :pick,
                                    temperature::Float64 = 1.0, violation_weight::Float64 = 0.0, x1::Union{Nothing,Matrix{Float64}} = nothing,
                                    base_u::Union{Nothing,Array{Float64,3}} = nothing, first_instance::Integer = 0, return_candidates::Bool = false)
    @assert length(sigma) == s.nu && candidates >= 1 && (mode === :pick || mode === :blend)
    @assert x1 === nothing || size(x1) == (s.nx, s.B)
    @assert base_u === nothing || size(base_u) == (s.nu, s.T - 1, s.B)
    S = Int(candidates)
    chosen = Vector{Int32}(undef, s.B)
    cost = Array{Float64,2}(undef, S, s.B); viol = Array{Float64,2}(undef, S, s.B); nonfinite = Array{Int32,2}(undef, S, s.B)
    weights = Array{Float64,2}(undef, S, s.B)
    u = return_candidates ? Array{Float64,4}(undef, s.nu, s.T - 1, S, s.B) : nothing
    nul = Ptr{Float64}(C_NULL)
    check(ccall((:ilqr_sample_rollout_candidates, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, UInt64, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                s.handle, Int32(S), Int32(mode === :pick ? 0 : 1), UInt64(seed), Int64(first_instance), sigma, violation_weight, temperature,
                x1 === nothing ? nul : x1, base_u === nothing ? nul : base_u, chosen, cost, viol, nonfinite, weights, u === nothing ? nul : u))
    return chosen .+ Int32(1), cost, viol, nonfinite, weights, u
end

# z of the candidates the device draws, on the host (ilqr_candidate_noise; needs no device): (nu, steps, candidates, batch), the
# first candidate's slice is zero
function candidate_noise(seed::Integer, batch::Integer, candidates::Integer, steps::Integer, nu::Integer; first_instance::Integer = 0)
    z = Array{Float64,4}(undef, nu, steps, candidates, batch)
    check(ccall((:ilqr_candidate_noise, LIB[]), Cint, (UInt64, Int64, Int32, Int32, Int32, Int32, Ptr{Float64}),
                UInt64(seed), Int64(first_instance), Int32(batch), Int32(candidates), Int32(steps), Int32(nu), z))
    return z
end

# Receding-horizon shift on the device (ilqr_shift_horizon): the solved trajectory moves forward by `steps` control periods and is
# installed as initialize_rollout! would install it. x1 :: (nx, B), the measured states (nothing: x̄ at step `steps`); tail = :hold
# keeps the last action over the new steps, :zero writes 0; feedback = true runs the shifted policy closed-loop from x1 over the
# head of the horizon. The parameters move with the horizon: their last `steps` columns are w_tail :: (nw, steps, B) or the last
# column held. Policy, duals and scalars stay.
function shift_horizon!(s::Solver; steps::Integer = 1, x1::Union{Nothing,Matrix{Float64}} = nothing, feedback::Bool = false,
                        tail::Symbol = :hold, w_tail::Union{Nothing,Array{Float64,3}} = nothing)
    @assert 0 <= steps <= s.T - 1 && (tail === :hold || tail === :zero)
    @assert x1 === nothing || size(x1) == (s.nx, s.B)
    @assert w_tail === nothing || (size(w_tail, 2) == steps && size(w_tail, 3) == s.B)
    nul = Ptr{Float64}(C_NULL)
    check(ccall((:ilqr_shift_horizon, LIB[]), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                s.handle, Int32(steps), Int32(tail === :hold ? 0 : 1), Int32(feedback ? 1 : 0), x1 === nothing ? nul : x1,
                w_tail === nothing ? nul : w_tail))
end

# Receding-horizon shift of the duals and penalties on the device (ilqr_shift_duals), the companion of shift_horizon!: λ'_t = λ_{t+steps},
# the last `steps` stage rows the old last stage row (tail = :hold) or 0 (:zero), the terminal rows stay; penalty = :keep moves ρ as λ
# (a :zero tail gets initial_constraint_penalty), :reset writes initial_constraint_penalty everywhere. Nothing else changes.
function shift_duals!(s::Solver; steps::Integer = 1, tail::Symbol = :hold, penalty::Symbol = :keep)
    @assert 0 <= steps <= s.T - 1 && (tail === :hold || tail === :zero) && (penalty === :keep || penalty === :reset)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    check(ccall((:ilqr_shift_duals, LIB[]), Cint, (Ptr{Cvoid}, Int32, Int32, Int32),
                s.handle, Int32(steps), Int32(tail === :hold ? 0 : 1), Int32(penalty === :keep ? 0 : 1)))
end

# The same, asynchronous on the handle's stream (not on a handle that spans several devices)
function shift_duals_device!(s::Solver; steps::Integer = 1, tail::Symbol = :hold, penalty::Symbol = :keep)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    check(ccall((:ilqr_shift_duals_device, LIB[]), Cint, (Ptr{Cvoid}, Int32, Int32, Int32),
                s.handle, Int32(steps), Int32(tail === :hold ? 0 : 1), Int32(penalty === :keep ? 0 : 1)))
end

# solve! with src/solve.jl:95-103 (λ ← 0, ρ ← ρ0) skipped: the duals and penalties the handle holds are kept (ilqr_solve_warm).
# Not a reference behaviour: the reference opens every constrained solve cold.
function solve_warm!(s::Solver)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    check(ccall((:ilqr_solve_warm, LIB[]), Cint, (Ptr{Cvoid},), s.handle))
    check(ccall((:ilqr_synchronize, LIB[]), Cint, (Ptr{Cvoid},), s.handle))
    return nothing
end

# The plant of a closed MPC loop on the device (ilqr_plant_step): the plant states x :: (nx, B) move on by `steps` control periods
# under the head of the handle's plan, u_i = ū_i or (feedback) ū_i + K_i (x − x̄_i), x ← f(x, u_i, w_i) + sigma_x .* z with z the noise
# of candidate_noise at candidate 1 + j ÷ 16, step step0 + i, component j % 16. w_plant :: (nw, steps, B): the plant's own parameters.
# Reads the handle. Returns (x_out :: (nx, steps + 1, B), u_out :: (nu, steps, B), first_nonfinite :: B); x is updated in place.
function plant_step!(s::Solver, x::Matrix{Float64}; steps::Integer = 1, feedback::Bool = false, seed::Integer = 0,
                     first_instance::Integer = 0, step0::Integer = 0, sigma_x::Union{Nothing,Vector{Float64}} = nothing,
                     w_plant::Union{Nothing,Array{Float64,3}} = nothing)
    @assert 1 <= steps <= s.T - 1 && size(x) == (s.nx, s.B)
    @assert sigma_x === nothing || length(sigma_x) == s.nx
    @assert w_plant === nothing || (size(w_plant, 2) == steps && size(w_plant, 3) == s.B)
    nul = Ptr{Float64}(C_NULL)
    x_out = Array{Float64,3}(undef, s.nx, steps + 1, s.B)
    u_out = Array{Float64,3}(undef, s.nu, steps, s.B)
    nf = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_plant_step, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                s.handle, Int32(steps), Int32(feedback ? 1 : 0), UInt64(seed), Int64(first_instance), Int32(step0),
                sigma_x === nothing ? nul : sigma_x, w_plant === nothing ? nul : w_plant, x, x_out, u_out, nf))
    return x_out, u_out, nf
end

# ilqr_mpc_desc, field for field
struct MpcDesc
    periods::Int32
    steps::Int32
    plant_feedback::Int32
    shift_feedback::Int32
    shift_tail::Int32
    warm::Int32
    duals_tail::Int32
    duals_penalty::Int32
    seed::UInt64
    first_instance::Int64
    sigma_x::Ptr{Float64}
end

# The closed MPC loop, enqueued once (ilqr_mpc_run): per period plant_step!, shift_horizon! from the plant state, (warm) shift_duals!
# and solve_warm!, else solve!, and a log row with the fields of Stats as Float64. x0 :: (nx, B) (nothing: x̄ at step 1 of the handle).
# Returns (x :: (nx, periods·steps + 1, B), u :: (nu, periods·steps, B), log :: (9, periods, B), first_nonfinite :: B).
# (The symbol is looked up by hand: the descriptor travels as Ref{MpcDesc}.)
function mpc_run!(s::Solver; periods::Integer, steps::Integer = 1, plant_feedback::Bool = false, shift_feedback::Bool = false,
                  shift_tail::Symbol = :hold, warm::Bool = true, duals_tail::Symbol = :hold, duals_penalty::Symbol = :keep,
                  seed::Integer = 0, first_instance::Integer = 0, sigma_x::Union{Nothing,Vector{Float64}} = nothing,
                  x0::Union{Nothing,Matrix{Float64}} = nothing, w_plant::Union{Nothing,Array{Float64,3}} = nothing)
    @assert periods >= 1 && 1 <= steps <= s.T - 1
    @assert sigma_x === nothing || length(sigma_x) == s.nx
    @assert x0 === nothing || size(x0) == (s.nx, s.B)
    R = periods * steps
    @assert w_plant === nothing || (size(w_plant, 2) == R && size(w_plant, 3) == s.B)
    nul = Ptr{Float64}(C_NULL)
    x = Array{Float64,3}(undef, s.nx, R + 1, s.B)
    u = Array{Float64,3}(undef, s.nu, R, s.B)
    log = Array{Float64,3}(undef, 9, periods, s.B)
    nf = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    sig = sigma_x === nothing ? Float64[] : sigma_x
    GC.@preserve sig begin
        d = MpcDesc(Int32(periods), Int32(steps), Int32(plant_feedback ? 1 : 0), Int32(shift_feedback ? 1 : 0),
                    Int32(shift_tail === :hold ? 0 : 1), Int32(warm ? 1 : 0), Int32(duals_tail === :hold ? 0 : 1),
                    Int32(duals_penalty === :keep ? 0 : 1), UInt64(seed), Int64(first_instance),
                    sigma_x === nothing ? nul : pointer(sig))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_mpc_run)
        check(ccall(fn, Cint, (Ptr{Cvoid}, Ref{MpcDesc}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    s.handle, d, x0 === nothing ? nul : x0, w_plant === nothing ? nul : w_plant, x, u, log, nf))
    end
    return x, u, log, nf
end

# The score of plant steps on the device (ilqr_plant_score): the realised stage cost and constraint violation of the states a plant
# visited and the actions it applied, x :: (nx, steps + 1, B) and u :: (nu, steps, B) as plant_step! returns them, under w_plant or
# the handle's θ at horizon positions 1 .. steps. To be called while the handle still holds the plan the steps were taken under.
# Reads the handle. Returns (cost :: (steps, B), violation :: (steps, B)); nothing is summed.
function plant_score!(s::Solver, x::Array{Float64,3}, u::Array{Float64,3}; w_plant::Union{Nothing,Array{Float64,3}} = nothing)
    steps = size(u, 2)
    @assert 1 <= steps <= s.T - 1 && size(x) == (s.nx, steps + 1, s.B) && size(u) == (s.nu, steps, s.B)
    @assert w_plant === nothing || (size(w_plant, 2) == steps && size(w_plant, 3) == s.B)
    cost = Matrix{Float64}(undef, steps, s.B)
    violation = Matrix{Float64}(undef, steps, s.B)
    check(ccall((:ilqr_plant_score, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                s.handle, Int32(steps), w_plant === nothing ? Ptr{Float64}(C_NULL) : w_plant, x, u, cost, violation))
    return cost, violation
end

# The same with raw device pointers on the handle's device (C_NULL: not given / not wanted); asynchronous on the handle's stream.
function plant_score_device!(s::Solver, steps::Integer, d_x::Ptr{Float64}, d_u::Ptr{Float64}, d_cost::Ptr{Float64};
                             d_violation::Ptr{Float64} = Ptr{Float64}(C_NULL), d_w_plant::Ptr{Float64} = Ptr{Float64}(C_NULL))
    check(ccall((:ilqr_plant_score_device, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                s.handle, Int32(steps), d_w_plant, d_x, d_u, d_cost, d_violation))
    return nothing
end

# mpc_run! following a previewed parameter stream, and scored (ilqr_mpc_run_preview): w_preview :: (nw, periods·steps, B) are the
# parameter rows that enter the horizon, `steps` of them per period; score = true adds the realised stage cost and violation of every
# plant step, each :: (periods·steps, B). Returns (x, u, log, first_nonfinite, cl_cost, cl_violation), the last two `nothing` without
# score. (The symbol is looked up by hand: the descriptor travels as Ref{MpcDesc}.)
function mpc_run_preview!(s::Solver; periods::Integer, steps::Integer = 1, plant_feedback::Bool = false, shift_feedback::Bool = false,
                          shift_tail::Symbol = :hold, warm::Bool = true, duals_tail::Symbol = :hold, duals_penalty::Symbol = :keep,
                          seed::Integer = 0, first_instance::Integer = 0, sigma_x::Union{Nothing,Vector{Float64}} = nothing,
                          x0::Union{Nothing,Matrix{Float64}} = nothing, w_plant::Union{Nothing,Array{Float64,3}} = nothing,
                          w_preview::Union{Nothing,Array{Float64,3}} = nothing, score::Bool = false)
    @assert periods >= 1 && 1 <= steps <= s.T - 1
    @assert sigma_x === nothing || length(sigma_x) == s.nx
    @assert x0 === nothing || size(x0) == (s.nx, s.B)
    R = periods * steps
    @assert w_plant === nothing || (size(w_plant, 2) == R && size(w_plant, 3) == s.B)
    @assert w_preview === nothing || (size(w_preview, 2) == R && size(w_preview, 3) == s.B)
    nul = Ptr{Float64}(C_NULL)
    x = Array{Float64,3}(undef, s.nx, R + 1, s.B)
    u = Array{Float64,3}(undef, s.nu, R, s.B)
    log = Array{Float64,3}(undef, 9, periods, s.B)
    nf = Vector{Int32}(undef, s.B)
    cl_cost = score ? Matrix{Float64}(undef, R, s.B) : nothing
    cl_violation = score ? Matrix{Float64}(undef, R, s.B) : nothing
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    sig = sigma_x === nothing ? Float64[] : sigma_x
    GC.@preserve sig begin
        d = MpcDesc(Int32(periods), Int32(steps), Int32(plant_feedback ? 1 : 0), Int32(shift_feedback ? 1 : 0),
                    Int32(shift_tail === :hold ? 0 : 1), Int32(warm ? 1 : 0), Int32(duals_tail === :hold ? 0 : 1),
                    Int32(duals_penalty === :keep ? 0 : 1), UInt64(seed), Int64(first_instance),
                    sigma_x === nothing ? nul : pointer(sig))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_mpc_run_preview)
        check(ccall(fn, Cint, (Ptr{Cvoid}, Ref{MpcDesc}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                    s.handle, d, x0 === nothing ? nul : x0, w_plant === nothing ? nul : w_plant, w_preview === nothing ? nul : w_preview,
                    x, u, log, nf, score ? cl_cost : nul, score ? cl_violation : nul))
    end
    return x, u, log, nf, cl_cost, cl_violation
end

# plant_step! with an actuator that saturates (ilqr_plant_step_limited): the action, feedback included, is clamped into
# [u_min, u_max] (either may be nothing: no limit on that side) before it is applied and recorded. Returns (x_out, u_out,
# first_nonfinite, saturated :: B — the (step, component) pairs the clamp changed); x is updated in place.
function plant_step_limited!(s::Solver, x::Matrix{Float64}; steps::Integer = 1, feedback::Bool = false, seed::Integer = 0,
                             first_instance::Integer = 0, step0::Integer = 0, sigma_x::Union{Nothing,Vector{Float64}} = nothing,
                             u_min::Union{Nothing,Vector{Float64}} = nothing, u_max::Union{Nothing,Vector{Float64}} = nothing,
                             w_plant::Union{Nothing,Array{Float64,3}} = nothing)
    @assert 1 <= steps <= s.T - 1 && size(x) == (s.nx, s.B)
    @assert sigma_x === nothing || length(sigma_x) == s.nx
    @assert (u_min === nothing || length(u_min) == s.nu) && (u_max === nothing || length(u_max) == s.nu)
    @assert w_plant === nothing || (size(w_plant, 2) == steps && size(w_plant, 3) == s.B)
    nul = Ptr{Float64}(C_NULL)
    x_out = Array{Float64,3}(undef, s.nx, steps + 1, s.B)
    u_out = Array{Float64,3}(undef, s.nu, steps, s.B)
    nf = Vector{Int32}(undef, s.B)
    saturated = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_plant_step_limited, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                s.handle, Int32(steps), Int32(feedback ? 1 : 0), UInt64(seed), Int64(first_instance), Int32(step0),
                sigma_x === nothing ? nul : sigma_x, u_min === nothing ? nul : u_min, u_max === nothing ? nul : u_max,
                w_plant === nothing ? nul : w_plant, x, x_out, u_out, nf, saturated))
    return x_out, u_out, nf, saturated
end

# What a controller is given of the plant states x :: (nx, B) (ilqr_plant_measure): y = x where sigma_y is nothing or zero, else
# y_j = x_j + sigma_y[j] · z with z the noise of candidate_noise at candidate 5 + j ÷ 16, step `step`, component j % 16; `step` is
# the number of plant steps taken when the measurement is made. Returns y :: (nx, B).
function plant_measure!(s::Solver, x::Matrix{Float64}; step::Integer = 0, seed::Integer = 0, first_instance::Integer = 0,
                        sigma_y::Union{Nothing,Vector{Float64}} = nothing)
    @assert size(x) == (s.nx, s.B) && (sigma_y === nothing || length(sigma_y) == s.nx)
    y = Matrix{Float64}(undef, s.nx, s.B)
    check(ccall((:ilqr_plant_measure, LIB[]), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                s.handle, UInt64(seed), Int64(first_instance), Int32(step), sigma_y === nothing ? Ptr{Float64}(C_NULL) : sigma_y, x, y))
    return y
end

# ilqr_plant_io, field for field
struct PlantIO
    u_min::Ptr{Float64}
    u_max::Ptr{Float64}
    sigma_y::Ptr{Float64}
    delay::Int32
    reserved::Int32
end

# mpc_run_preview! with the seam between plant and controller in the loop (ilqr_mpc_run_io): actuator limits u_min, u_max,
# measurement noise sigma_y on the state the shift is handed, and delay = 1 — the re-solve is anchored at a one-period model
# prediction from a measurement one period old. Returns (x, u, log, first_nonfinite, cl_cost, cl_violation, y_cl :: (nx, periods, B),
# saturated :: B). (The symbol is looked up by hand: the descriptors travel as Ref{MpcDesc}, Ref{PlantIO}.)
function mpc_run_io!(s::Solver; periods::Integer, steps::Integer = 1, plant_feedback::Bool = false, shift_feedback::Bool = false,
                     shift_tail::Symbol = :hold, warm::Bool = true, duals_tail::Symbol = :hold, duals_penalty::Symbol = :keep,
                     seed::Integer = 0, first_instance::Integer = 0, sigma_x::Union{Nothing,Vector{Float64}} = nothing,
                     x0::Union{Nothing,Matrix{Float64}} = nothing, w_plant::Union{Nothing,Array{Float64,3}} = nothing,
                     w_preview::Union{Nothing,Array{Float64,3}} = nothing, score::Bool = false,
                     u_min::Union{Nothing,Vector{Float64}} = nothing, u_max::Union{Nothing,Vector{Float64}} = nothing,
                     sigma_y::Union{Nothing,Vector{Float64}} = nothing, delay::Integer = 0)
    @assert periods >= 1 && 1 <= steps <= s.T - 1 && (delay == 0 || delay == 1)
    @assert sigma_x === nothing || length(sigma_x) == s.nx
    @assert sigma_y === nothing || length(sigma_y) == s.nx
    @assert (u_min === nothing || length(u_min) == s.nu) && (u_max === nothing || length(u_max) == s.nu)
    @assert x0 === nothing || size(x0) == (s.nx, s.B)
    R = periods * steps
    @assert w_plant === nothing || (size(w_plant, 2) == R && size(w_plant, 3) == s.B)
    @assert w_preview === nothing || (size(w_preview, 2) == R && size(w_preview, 3) == s.B)
    nul = Ptr{Float64}(C_NULL)
    x = Array{Float64,3}(undef, s.nx, R + 1, s.B)
    u = Array{Float64,3}(undef, s.nu, R, s.B)
    log = Array{Float64,3}(undef, 9, periods, s.B)
    nf = Vector{Int32}(undef, s.B)
    cl_cost = score ? Matrix{Float64}(undef, R, s.B) : nothing
    cl_violation = score ? Matrix{Float64}(undef, R, s.B) : nothing
    y_cl = Array{Float64,3}(undef, s.nx, periods, s.B)
    saturated = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    sig = sigma_x === nothing ? Float64[] : sigma_x
    lo = u_min === nothing ? Float64[] : u_min
    hi = u_max === nothing ? Float64[] : u_max
    sy = sigma_y === nothing ? Float64[] : sigma_y
    GC.@preserve sig lo hi sy begin
        d = MpcDesc(Int32(periods), Int32(steps), Int32(plant_feedback ? 1 : 0), Int32(shift_feedback ? 1 : 0),
                    Int32(shift_tail === :hold ? 0 : 1), Int32(warm ? 1 : 0), Int32(duals_tail === :hold ? 0 : 1),
                    Int32(duals_penalty === :keep ? 0 : 1), UInt64(seed), Int64(first_instance),
                    sigma_x === nothing ? nul : pointer(sig))
        io = PlantIO(u_min === nothing ? nul : pointer(lo), u_max === nothing ? nul : pointer(hi),
                     sigma_y === nothing ? nul : pointer(sy), Int32(delay), Int32(0))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_mpc_run_io)
        check(ccall(fn, Cint, (Ptr{Cvoid}, Ref{MpcDesc}, Ref{PlantIO}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                    s.handle, d, io, x0 === nothing ? nul : x0, w_plant === nothing ? nul : w_plant, w_preview === nothing ? nul : w_preview,
                    x, u, log, nf, score ? cl_cost : nul, score ? cl_violation : nul, y_cl, saturated))
    end
    return x, u, log, nf, cl_cost, cl_violation, y_cl, saturated
end

# The time update of the extended Kalman filter on the device (ilqr_estimate_predict): the estimates xhat :: (nx, B) move on by
# `steps` control periods under the head of the handle's plan as plant_step_limited! moves a state without noise, and per step
# P ← F P Fᵀ + diag(q), F the model's dynamics state Jacobian at the estimate before it moves. P :: (nx, nx, B), symmetric. Both
# arrays are updated in place.
function estimate_predict!(s::Solver, xhat::Matrix{Float64}, P::Array{Float64,3}; steps::Integer = 1, feedback::Bool = false,
                           u_min::Union{Nothing,Vector{Float64}} = nothing, u_max::Union{Nothing,Vector{Float64}} = nothing,
                           q::Union{Nothing,Vector{Float64}} = nothing)
    @assert size(xhat) == (s.nx, s.B) && size(P) == (s.nx, s.nx, s.B) && 1 <= steps <= s.T - 1
    @assert (u_min === nothing || length(u_min) == s.nu) && (u_max === nothing || length(u_max) == s.nu) && (q === nothing || length(q) == s.nx)
    nul = Ptr{Float64}(C_NULL)
    check(ccall((:ilqr_estimate_predict, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                s.handle, Int32(steps), Int32(feedback ? 1 : 0), u_min === nothing ? nul : u_min, u_max === nothing ? nul : u_max,
                q === nothing ? nul : q, xhat, P))
    return xhat, P
end

# A state covariance propagated down the handle's plan under its feedback policy (ilqr_plan_covariance): Σ_0 = P0 :: (nx, nx, B)
# (one triangle is read and mirrored), Σ_{t+1} = Φ Σ_t Φᵀ + diag(q) with Φ = A + Bm K_t (feedback) or A at the nominal point of the
# plan. Reads the handle. Returns (sdiag :: (nx, steps + 1, B), udiag :: (nu, steps, B), P :: (nx, nx, B) = Σ_steps,
# first_nonfinite :: B, sigma :: (nx, nx, steps + 1, B) or nothing).
function plan_covariance!(s::Solver, P0::Array{Float64,3}; steps::Integer = s.T - 1, feedback::Bool = true,
                          q::Union{Nothing,Vector{Float64}} = nothing, full::Bool = false)
    @assert size(P0) == (s.nx, s.nx, s.B) && 1 <= steps <= s.T - 1 && (q === nothing || length(q) == s.nx)
    nul = Ptr{Float64}(C_NULL)
    sdiag = Array{Float64,3}(undef, s.nx, steps + 1, s.B)
    udiag = Array{Float64,3}(undef, s.nu, steps, s.B)
    sigma = full ? Array{Float64,4}(undef, s.nx, s.nx, steps + 1, s.B) : nothing
    P = Array{Float64,3}(undef, s.nx, s.nx, s.B)
    nf = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_plan_covariance, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                s.handle, Int32(steps), Int32(feedback ? 1 : 0), q === nothing ? nul : q, P0, sdiag, udiag, full ? sigma : nul, P, nf))
    return sdiag, udiag, P, nf, sigma
end

# The same on device arrays of the handle's device (C_NULL: not wanted; d_P_out may be d_P0), asynchronous on the handle's stream;
# q stays a host vector.
function plan_covariance_device!(s::Solver, d_P0::Ptr{Float64}; steps::Integer = s.T - 1, feedback::Bool = true,
                                 q::Union{Nothing,Vector{Float64}} = nothing, d_sdiag::Ptr{Float64} = Ptr{Float64}(C_NULL),
                                 d_udiag::Ptr{Float64} = Ptr{Float64}(C_NULL), d_sigma::Ptr{Float64} = Ptr{Float64}(C_NULL),
                                 d_P_out::Ptr{Float64} = Ptr{Float64}(C_NULL), d_first_nonfinite::Ptr{Int32} = Ptr{Int32}(C_NULL))
    @assert 1 <= steps <= s.T - 1 && (q === nothing || length(q) == s.nx)
    check(ccall((:ilqr_plan_covariance_device, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                s.handle, Int32(steps), Int32(feedback ? 1 : 0), q === nothing ? Ptr{Float64}(C_NULL) : q, d_P0, d_sdiag, d_udiag, d_sigma,
                d_P_out, d_first_nonfinite))
    return nothing
end

# The measurement update (ilqr_estimate_update): the components j of y :: (nx, B) with measured[j] == 1 (nothing: all) are taken in
# one after the other with the variances r. xhat and P are updated in place. Returns (innovation :: (nx, B), nis :: B, first_bad :: B).
function estimate_update!(s::Solver, xhat::Matrix{Float64}, P::Array{Float64,3}, y::Matrix{Float64}, r::Vector{Float64};
                          measured::Union{Nothing,Vector{Int32}} = nothing)
    @assert size(xhat) == (s.nx, s.B) && size(P) == (s.nx, s.nx, s.B) && size(y) == (s.nx, s.B) && length(r) == s.nx
    @assert measured === nothing || length(measured) == s.nx
    innovation = Matrix{Float64}(undef, s.nx, s.B)
    nis = Vector{Float64}(undef, s.B)
    first_bad = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_estimate_update, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                s.handle, measured === nothing ? Ptr{Int32}(C_NULL) : measured, r, y, xhat, P, innovation, nis, first_bad))
    return innovation, nis, first_bad
end

# ilqr_estimator, field for field
struct Estimator
    measured::Ptr{Int32}
    q::Ptr{Float64}
    r::Ptr{Float64}
end

# mpc_run_io! with the filter between sensor and controller (ilqr_mpc_run_est): the re-solve is anchored at the estimate. P0 ::
# (nx, nx, B) holds the last covariance on return. Returns (x, u, log, first_nonfinite, y_cl, saturated, xhat :: (nx, periods, B),
# pdiag :: (nx, periods, B), nis :: (periods, B), P0). (The symbol is looked up by hand, as mpc_run_io!'s.)
function mpc_run_est!(s::Solver, r::Vector{Float64}, P0::Array{Float64,3}; periods::Integer, steps::Integer = 1, plant_feedback::Bool = false,
                      shift_feedback::Bool = false, shift_tail::Symbol = :hold, warm::Bool = true, duals_tail::Symbol = :hold,
                      duals_penalty::Symbol = :keep, seed::Integer = 0, first_instance::Integer = 0,
                      sigma_x::Union{Nothing,Vector{Float64}} = nothing, x0::Union{Nothing,Matrix{Float64}} = nothing,
                      xhat0::Union{Nothing,Matrix{Float64}} = nothing, u_min::Union{Nothing,Vector{Float64}} = nothing,
                      u_max::Union{Nothing,Vector{Float64}} = nothing, sigma_y::Union{Nothing,Vector{Float64}} = nothing, delay::Integer = 0,
                      measured::Union{Nothing,Vector{Int32}} = nothing, q::Union{Nothing,Vector{Float64}} = nothing)
    @assert periods >= 1 && 1 <= steps <= s.T - 1 && (delay == 0 || delay == 1)
    @assert length(r) == s.nx && size(P0) == (s.nx, s.nx, s.B) && (q === nothing || length(q) == s.nx) && (measured === nothing || length(measured) == s.nx)
    @assert (x0 === nothing || size(x0) == (s.nx, s.B)) && (xhat0 === nothing || size(xhat0) == (s.nx, s.B))
    R = periods * steps
    nul = Ptr{Float64}(C_NULL)
    x = Array{Float64,3}(undef, s.nx, R + 1, s.B)
    u = Array{Float64,3}(undef, s.nu, R, s.B)
    log = Array{Float64,3}(undef, 9, periods, s.B)
    nf = Vector{Int32}(undef, s.B)
    y_cl = Array{Float64,3}(undef, s.nx, periods, s.B)
    saturated = Vector{Int32}(undef, s.B)
    xhat = Array{Float64,3}(undef, s.nx, periods, s.B)
    pdiag = Array{Float64,3}(undef, s.nx, periods, s.B)
    nis = Matrix{Float64}(undef, periods, s.B)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    sig = sigma_x === nothing ? Float64[] : sigma_x
    lo = u_min === nothing ? Float64[] : u_min
    hi = u_max === nothing ? Float64[] : u_max
    sy = sigma_y === nothing ? Float64[] : sigma_y
    mk = measured === nothing ? Int32[] : measured
    qq = q === nothing ? Float64[] : q
    GC.@preserve sig lo hi sy mk qq r begin
        d = MpcDesc(Int32(periods), Int32(steps), Int32(plant_feedback ? 1 : 0), Int32(shift_feedback ? 1 : 0),
                    Int32(shift_tail === :hold ? 0 : 1), Int32(warm ? 1 : 0), Int32(duals_tail === :hold ? 0 : 1),
                    Int32(duals_penalty === :keep ? 0 : 1), UInt64(seed), Int64(first_instance),
                    sigma_x === nothing ? nul : pointer(sig))
        io = PlantIO(u_min === nothing ? nul : pointer(lo), u_max === nothing ? nul : pointer(hi),
                     sigma_y === nothing ? nul : pointer(sy), Int32(delay), Int32(0))
        est = Estimator(measured === nothing ? Ptr{Int32}(C_NULL) : pointer(mk), q === nothing ? nul : pointer(qq), pointer(r))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_mpc_run_est)
        check(ccall(fn, Cint, (Ptr{Cvoid}, Ref{MpcDesc}, Ref{PlantIO}, Ref{Estimator}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    s.handle, d, io, est, x0 === nothing ? nul : x0, xhat0 === nothing ? nul : xhat0, P0, nul, nul, x, u, log, nf, nul, nul, y_cl,
                    saturated, xhat, pdiag, nis))
    end
    return x, u, log, nf, y_cl, saturated, xhat, pdiag, nis, P0
end

# The measurement update with a linear sensor y = H x + v, v ~ N(0, diag(r)) (ilqr_estimate_update_linear): H :: (nx, ny) shared by the
# batch or (nx, ny, B) one per instance (column-major here is the header's row-major [ny][nx]), y :: (ny, B), r :: ny, yhat :: (ny, B)
# the caller's h(x̂) of a nonlinear sensor linearised at x̂. xhat and P are updated in place. Returns (innovation :: (ny, B), nis :: B,
# first_bad :: B).
function estimate_update_linear!(s::Solver, xhat::Matrix{Float64}, P::Array{Float64,3}, y::Matrix{Float64}, H::Array{Float64}, r::Vector{Float64};
                                 yhat::Union{Nothing,Matrix{Float64}} = nothing)
    ny = size(H, 2)
    @assert size(xhat) == (s.nx, s.B) && size(P) == (s.nx, s.nx, s.B) && size(y) == (ny, s.B) && length(r) == ny
    @assert size(H) == (s.nx, ny) || size(H) == (s.nx, ny, s.B)
    @assert yhat === nothing || size(yhat) == (ny, s.B)
    innovation = Matrix{Float64}(undef, ny, s.B)
    nis = Vector{Float64}(undef, s.B)
    first_bad = Vector{Int32}(undef, s.B)
    check(ccall((:ilqr_estimate_update_linear, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}),
                s.handle, Int32(ny), Int32(ndims(H) == 3 ? 1 : 0), H, r, y, yhat === nothing ? Ptr{Float64}(C_NULL) : yhat, xhat, P, innovation, nis,
                first_bad))
    return innovation, nis, first_bad
end

# What a linear sensor reads of the plant states x :: (nx, B) (ilqr_plant_measure_linear): y = H x with H :: (nx, ny), plus sigma_y[j] · z
# from plant_measure!'s stream. Returns y :: (ny, B).
function plant_measure_linear!(s::Solver, x::Matrix{Float64}, H::Matrix{Float64}; step::Integer = 0,
                               sigma_y::Union{Nothing,Vector{Float64}} = nothing, seed::Integer = 0, first_instance::Integer = 0)
    ny = size(H, 2)
    @assert size(x) == (s.nx, s.B) && size(H, 1) == s.nx && (sigma_y === nothing || length(sigma_y) == ny)
    y = Matrix{Float64}(undef, ny, s.B)
    check(ccall((:ilqr_plant_measure_linear, LIB[]), Cint,
                (Ptr{Cvoid}, UInt64, Int64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                s.handle, UInt64(seed), Int64(first_instance), Int32(step), Int32(ny), H, sigma_y === nothing ? Ptr{Float64}(C_NULL) : sigma_y, x, y))
    return y
end

# ilqr_sensor, field for field
struct Sensor
    ny::Int32
    reserved::Int32
    H::Ptr{Float64}
    r::Ptr{Float64}
    q::Ptr{Float64}
    sigma_y::Ptr{Float64}
end

# mpc_run_est! with the linear sensor in the place of the selection of state components (ilqr_mpc_run_sensor): H :: (nx, ny), r and
# sigma_y :: ny. Returns (x, u, log, first_nonfinite, y_cl :: (ny, periods, B), saturated, xhat, pdiag, nis, P0). (The symbol is looked
# up by hand, as mpc_run_io!'s.)
function mpc_run_sensor!(s::Solver, H::Matrix{Float64}, r::Vector{Float64}, P0::Array{Float64,3}; periods::Integer, steps::Integer = 1,
                         plant_feedback::Bool = false, shift_feedback::Bool = false, shift_tail::Symbol = :hold, warm::Bool = true,
                         duals_tail::Symbol = :hold, duals_penalty::Symbol = :keep, seed::Integer = 0, first_instance::Integer = 0,
                         sigma_x::Union{Nothing,Vector{Float64}} = nothing, x0::Union{Nothing,Matrix{Float64}} = nothing,
                         xhat0::Union{Nothing,Matrix{Float64}} = nothing, u_min::Union{Nothing,Vector{Float64}} = nothing,
                         u_max::Union{Nothing,Vector{Float64}} = nothing, sigma_y::Union{Nothing,Vector{Float64}} = nothing, delay::Integer = 0,
                         q::Union{Nothing,Vector{Float64}} = nothing)
    ny = size(H, 2)
    @assert periods >= 1 && 1 <= steps <= s.T - 1 && (delay == 0 || delay == 1)
    @assert size(H, 1) == s.nx && length(r) == ny && size(P0) == (s.nx, s.nx, s.B) && (q === nothing || length(q) == s.nx)
    @assert sigma_y === nothing || length(sigma_y) == ny
    @assert (x0 === nothing || size(x0) == (s.nx, s.B)) && (xhat0 === nothing || size(xhat0) == (s.nx, s.B))
    R = periods * steps
    nul = Ptr{Float64}(C_NULL)
    x = Array{Float64,3}(undef, s.nx, R + 1, s.B)
    u = Array{Float64,3}(undef, s.nu, R, s.B)
    log = Array{Float64,3}(undef, 9, periods, s.B)
    nf = Vector{Int32}(undef, s.B)
    y_cl = Array{Float64,3}(undef, ny, periods, s.B)
    saturated = Vector{Int32}(undef, s.B)
    xhat = Array{Float64,3}(undef, s.nx, periods, s.B)
    pdiag = Array{Float64,3}(undef, s.nx, periods, s.B)
    nis = Matrix{Float64}(undef, periods, s.B)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    sig = sigma_x === nothing ? Float64[] : sigma_x
    lo = u_min === nothing ? Float64[] : u_min
    hi = u_max === nothing ? Float64[] : u_max
    sy = sigma_y === nothing ? Float64[] : sigma_y
    qq = q === nothing ? Float64[] : q
    GC.@preserve sig lo hi sy qq r H begin
        d = MpcDesc(Int32(periods), Int32(steps), Int32(plant_feedback ? 1 : 0), Int32(shift_feedback ? 1 : 0),
                    Int32(shift_tail === :hold ? 0 : 1), Int32(warm ? 1 : 0), Int32(duals_tail === :hold ? 0 : 1),
                    Int32(duals_penalty === :keep ? 0 : 1), UInt64(seed), Int64(first_instance),
                    sigma_x === nothing ? nul : pointer(sig))
        io = PlantIO(u_min === nothing ? nul : pointer(lo), u_max === nothing ? nul : pointer(hi), nul, Int32(delay), Int32(0))
        sensor = Sensor(Int32(ny), Int32(0), pointer(H), pointer(r), q === nothing ? nul : pointer(qq), sigma_y === nothing ? nul : pointer(sy))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_mpc_run_sensor)
        check(ccall(fn, Cint, (Ptr{Cvoid}, Ref{MpcDesc}, Ref{PlantIO}, Ref{Sensor}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    s.handle, d, io, sensor, x0 === nothing ? nul : x0, xhat0 === nothing ? nul : xhat0, P0, nul, nul, x, u, log, nf, nul, nul, y_cl,
                    saturated, xhat, pdiag, nis))
    end
    return x, u, log, nf, y_cl, saturated, xhat, pdiag, nis, P0
end

# Solver(...; parameters = θ) — src/solver.jl:12,29; θ :: (nw, T, B)
function set_parameters!(s::Solver, w::Array{Float64,3})
    check(ccall((:ilqr_set_parameters, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), s.handle, w))
end

# solve!(solver[, states, actions]) — src/solve.jl:137-143, 131-135
function solve!(s::Solver, args...)
    if length(args) == 2
        initialize_controls!(s, args[2]); initialize_states!(s, args[1])
    end
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    check(ccall((:ilqr_solve, LIB[]), Cint, (Ptr{Cvoid},), s.handle))
    check(ccall((:ilqr_synchronize, LIB[]), Cint, (Ptr{Cvoid},), s.handle))
    return nothing
end

# get_trajectory(solver) — src/solver.jl:48-50
function get_trajectory(s::Solver)
    x = Array{Float64,3}(undef, s.nx, s.T, s.B); u = Array{Float64,3}(undef, s.nu, s.T - 1, s.B)
    check(ccall((:ilqr_get_trajectory, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.handle, x, u))
    return x, u
end

# solver.policy.K / .k — K[:, :, t, b] is the nu×nx gain (column-major, as in the reference)
function get_policy(s::Solver)
    K = Array{Float64,4}(undef, s.nu, s.nx, s.T - 1, s.B); k = Array{Float64,3}(undef, s.nu, s.T - 1, s.B)
    check(ccall((:ilqr_get_policy, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), s.handle, K, k))
    return K, k
end

# Closed-loop rollouts of the current policy from x1[:, s, b] (ilqr_rollout_policy): rollout!(policy, problem; step_size) of
# src/rollout.jl:1-31 started at the caller's states, S samples per instance, optionally under the samples' own parameters
# w[:, t, s, b]. Returns (cost, max_violation, first_nonfinite) as S×B arrays and, with trajectories = true, x (nx×T×S×B) and
# u (nu×(T-1)×S×B) as well. The handle's state is not changed.
function rollout_policy(s::Solver, x1::Array{Float64,3}; w::Union{Nothing,Array{Float64,4}} = nothing, step_size::Float64 = 0.0,
                        trajectories::Bool = false)
    S = size(x1, 2)
    cost = Array{Float64,2}(undef, S, s.B); viol = Array{Float64,2}(undef, S, s.B); nonfinite = Array{Int32,2}(undef, S, s.B)
    x = trajectories ? Array{Float64,4}(undef, s.nx, s.T, S, s.B) : nothing
    u = trajectories ? Array{Float64,4}(undef, s.nu, s.T - 1, S, s.B) : nothing
    nul = Ptr{Float64}(C_NULL)
    check(ccall((:ilqr_rollout_policy, LIB[]), Cint,
                (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                s.handle, Int32(S), step_size, x1, w === nothing ? nul : w, cost, viol, nonfinite,
                trajectories ? x : nul, trajectories ? u : nul))
    return trajectories ? (cost, viol, nonfinite, x, u) : (cost, viol, nonfinite)
end

# solver.data.* per instance
function stats(s::Solver)
    st = Vector{Stats}(undef, s.B)
    check(ccall((:ilqr_get_stats, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Stats}), s.handle, st))
    return st
end

# ------------------------------------------------------------------------------------------------------------
# Dynamics / Cost / Constraint with the reference's constructors (src/dynamics.jl:16-34, src/costs.jl:17-44,
# src/constraints.jl:17-43): the user function is traced on Symbolics variables exactly as the reference does, but
# instead of `eval(build_function(...)[2])` (a Julia closure) the expressions are emitted as C
# (`Symbolics.build_function(expr, x, u, w; target = Symbolics.CTarget())` — from memory of the Symbolics docs; the
# image has no Julia, so this half has never run) and handed to `ilqr_compile_model`, which wraps them for the kernels
# (csrc/ilqr_model_adapter.hpp) and compiles them with hipcc. Requires `using Symbolics` in the caller's environment.
# `body` is C source whose function names start with the placeholder @P@ (e.g. @P@_jacobian_state): Solver(...) gives every
# distinct object of a problem its own prefix — dynamics_<k>, cost_stage_<k>, constraint_stage_<k>, cost_terminal,
# constraint_terminal — as ilqr_compile_model_stages expects them (include/ilqr_hip.h).
struct Dynamics;  body::String; num_next_state::Int; num_state::Int; num_action::Int; num_parameter::Int; end
struct Cost;      body::String; num_state::Int; num_action::Int; num_parameter::Int; end
struct Constraint; body::String; num_constraint::Int; num_state::Int; num_action::Int; num_parameter::Int
                   indices_inequality::Vector{Int}; end
Constraint() = Constraint("", 0, 0, 0, 0, Int[])

# one `ILQR_MODEL_FN void name(double* out, const double* x, const double* u, const double* w)` per expression array
function c_function(Symbolics, name::String, exprs, x, u, w)
    src = Symbolics.build_function(exprs, x, u, w; target = Symbolics.CTarget(), fname = name * "_raw",
                                   lhsname = :out, rhsnames = [:x, :u, :w])
    return string(src, "\nILQR_MODEL_FN void ", name,
                  "(double* out, const double* x, const double* u, const double* w) { ", name, "_raw(out, x, u, w); }\n")
    # (name carries the @P@ placeholder; it is substituted in the whole body, raw function included, before compilation)
end

function Dynamics(Symbolics, f::Function, num_state::Int, num_action::Int; num_parameter::Int = 0)
    x = Symbolics.variables(:x, 1:num_state); u = Symbolics.variables(:u, 1:num_action); w = Symbolics.variables(:w, 1:num_parameter)
    y = num_parameter > 0 ? f(x, u, w) : f(x, u)
    body = c_function(Symbolics, "@P@", y, x, u, w) *
           c_function(Symbolics, "@P@_jacobian_state", vec(Symbolics.jacobian(y, x)), x, u, w) *
           c_function(Symbolics, "@P@_jacobian_action", vec(Symbolics.jacobian(y, u)), x, u, w)
    Dynamics(body, length(y), num_state, num_action, num_parameter)      # num_next_state = length(f(x, u)), src/dynamics.jl:22-29
end

function Cost(Symbolics, f::Function, num_state::Int, num_action::Int; num_parameter::Int = 0, terminal::Bool = num_action == 0)
    x = Symbolics.variables(:x, 1:num_state); u = Symbolics.variables(:u, 1:num_action); w = Symbolics.variables(:w, 1:num_parameter)
    l = num_parameter > 0 ? f(x, u, w) : f(x, u)
    gx = Symbolics.gradient(l, x); gu = Symbolics.gradient(l, u)
    p = "@P@"
    body = c_function(Symbolics, p, [l], x, u, w) * c_function(Symbolics, p * "_gradient_state", gx, x, u, w) *
           c_function(Symbolics, p * "_hessian_state_state", vec(Symbolics.jacobian(gx, x)), x, u, w)
    if !terminal
        body *= c_function(Symbolics, p * "_gradient_action", gu, x, u, w) *
                c_function(Symbolics, p * "_hessian_action_action", vec(Symbolics.jacobian(gu, u)), x, u, w) *
                c_function(Symbolics, p * "_hessian_action_state", vec(Symbolics.jacobian(gu, x)), x, u, w)
    end
    Cost(body, num_state, num_action, num_parameter)
end

function Constraint(Symbolics, f::Function, num_state::Int, num_action::Int; indices_inequality::Vector{Int} = Int[],
                    num_parameter::Int = 0, terminal::Bool = num_action == 0)
    x = Symbolics.variables(:x, 1:num_state); u = Symbolics.variables(:u, 1:num_action); w = Symbolics.variables(:w, 1:num_parameter)
    c = num_parameter > 0 ? f(x, u, w) : f(x, u)
    p = "@P@"
    body = c_function(Symbolics, p, c, x, u, w) * c_function(Symbolics, p * "_jacobian_state", vec(Symbolics.jacobian(c, x)), x, u, w)
    terminal || (body *= c_function(Symbolics, p * "_jacobian_action", vec(Symbolics.jacobian(c, u)), x, u, w))
    Constraint(body, length(c), num_state, num_action, num_parameter, indices_inequality)
end

# The reference's own signatures — Dynamics(f, nx, nu; num_parameter), Cost(f, nx, nu; num_parameter),
# Constraint(f, nx, nu; indices_inequality, num_parameter) (src/dynamics.jl:16, src/costs.jl:17, src/constraints.jl:17) —
# with Symbolics taken from the session (`using Symbolics` before the first call, as a user of the reference has anyway)
function symbolics_module()
    isdefined(Main, :Symbolics) || error("IterativeLQRAMD: `using Symbolics` first (the constructors trace the user function symbolically, as the reference does)")
    return getfield(Main, :Symbolics)
end
Dynamics(f::Function, num_state::Int, num_action::Int; kwargs...) = Dynamics(symbolics_module(), f, num_state, num_action; kwargs...)
Cost(f::Function, num_state::Int, num_action::Int; kwargs...) = Cost(symbolics_module(), f, num_state, num_action; kwargs...)
Constraint(f::Function, num_state::Int, num_action::Int; kwargs...) = Constraint(symbolics_module(), f, num_state, num_action; kwargs...)

# ilqr_stage_kinds / ilqr_stage_plan (include/ilqr_hip.h), field for field
struct StageKinds
    horizon::Int32; num_parameter::Int32
    n_dynamics::Int32; dynamics_nx::Ptr{Int32}; dynamics_nu::Ptr{Int32}; dynamics_nx_next::Ptr{Int32}; dynamics_of_step::Ptr{Int32}
    n_costs::Int32; cost_nx::Ptr{Int32}; cost_nu::Ptr{Int32}; cost_of_step::Ptr{Int32}
    n_constraints::Int32; constraint_nc::Ptr{Int32}; constraint_nx::Ptr{Int32}; constraint_nu::Ptr{Int32}
    constraint_ineq::Ptr{UInt64}; constraint_of_step::Ptr{Int32}
    nx_term::Int32; nc_term::Int32; ineq_term::NTuple{4,UInt64}
end
struct StagePlan
    nx::Int32; nu::Int32; nw::Int32; nc_stage::Int32; nc_term::Int32; n_selectors::Int32
    sel_dynamics::Int32; sel_cost::Int32; sel_constraint::Int32
    constraint_row0::NTuple{16,Int32}; ineq_stage_words::NTuple{4,UInt64}
end
# inequality rows as four 64-bit words: row i (1-based, as indices_inequality is) = bit (i - 1) % 64 of word (i - 1) ÷ 64
function ineq_words(idx)
    w = zeros(UInt64, 4)
    for i in idx
        w[(i - 1) ÷ 64 + 1] |= UInt64(1) << ((i - 1) % 64)
    end
    return w
end

# distinct objects of a vector in order of first appearance, and the (0-based) kind of every element
function kinds_of(objs)
    kinds = eltype(objs)[]; index = Int32[]
    for o in objs
        k = findfirst(q -> q == o, kinds)
        if k === nothing
            push!(kinds, o); k = length(kinds)
        end
        push!(index, Int32(k - 1))
    end
    return kinds, index
end
Base.:(==)(a::Dynamics, b::Dynamics) = a.body == b.body && (a.num_next_state, a.num_state, a.num_action) == (b.num_next_state, b.num_state, b.num_action)
Base.:(==)(a::Cost, b::Cost) = a.body == b.body && (a.num_state, a.num_action) == (b.num_state, b.num_action)
Base.:(==)(a::Constraint, b::Constraint) = a.body == b.body && a.indices_inequality == b.indices_inequality &&
                                           (a.num_constraint, a.num_state, a.num_action) == (b.num_constraint, b.num_state, b.num_action)

"""
    Solver(dynamics, costs, constraints; batch, options, name)

`Solver(dynamics, costs, constraints)` of the reference (src/solver.jl:28-46) for a batch: T-1 Dynamics, T Costs, T Constraints,
the last Cost / Constraint being the terminal objects (they are evaluated with `u = zeros(0)`, src/costs.jl:52, src/constraints.jl:69).
The objects MAY DIFFER from step to step and so may their dimensions (README.md:26, src/dynamics.jl:5-7): the distinct ones are
handed to the library kind by kind (`ilqr_compile_model_stages`), which lowers them onto its one-stage template — selectors in θ_t,
stacked constraint rows, zero padding to the largest dimensions — and the handle is given the selector table
(`ilqr_set_stage_selectors`). Arrays passed to / returned by the solver are the PADDED ones: (solver.nx, T, B) with
`solver.state_dims[t]` real entries at step t, likewise `solver.action_dims`.
"""
function Solver(dynamics::Vector{Dynamics}, costs::Vector{Cost}, constraints::Vector{Constraint};
                batch::Integer, options::Options = Options(), name::AbstractString = "user", device::Integer = 0,
                devices::AbstractVector{<:Integer} = Int[], constrained::Bool = true)
    T = length(costs)
    length(dynamics) == T - 1 && length(constraints) == T ||
        error("Solver: expected T-1 dynamics, T costs and T constraints (src/solver.jl:28-46)")
    dk, di = kinds_of(dynamics)
    ck, ci = kinds_of(costs[1:end-1])
    kk, ki = kinds_of(constraints[1:end-1])
    ct, kt = costs[end], constraints[end]
    nwu = maximum(o.num_parameter for o in vcat(dk, ck, kk, [ct], [kt]))
    prefix(body, p) = replace(body, "@P@" => p)
    source = join([prefix(d.body, "dynamics_$(k - 1)") for (k, d) in enumerate(dk)]) *
             join([prefix(c.body, "cost_stage_$(k - 1)") for (k, c) in enumerate(ck)]) *
             join([prefix(c.body, "constraint_stage_$(k - 1)") for (k, c) in enumerate(kk) if c.num_constraint > 0]) *
             prefix(ct.body, "cost_terminal") * (kt.num_constraint > 0 ? prefix(kt.body, "constraint_terminal") : "")
    i32(v) = Int32.(collect(v))
    dnx, dnu, dnn = i32(d.num_state for d in dk), i32(d.num_action for d in dk), i32(d.num_next_state for d in dk)
    cnx, cnu = i32(c.num_state for c in ck), i32(c.num_action for c in ck)
    knc, knx, knu = i32(c.num_constraint for c in kk), i32(c.num_state for c in kk), i32(c.num_action for c in kk)
    kin = reduce(vcat, [ineq_words(c.indices_inequality) for c in kk]; init = UInt64[])
    cap = T * (length(dk) + length(ck) + length(kk))
    selectors = zeros(Float64, max(cap, 1)); state_dims = zeros(Int32, T); action_dims = zeros(Int32, T - 1)
    plan = Ref(StagePlan(0, 0, 0, 0, 0, 0, 0, 0, 0, ntuple(_ -> Int32(0), 16), ntuple(_ -> UInt64(0), 4)))
    regname = Vector{UInt8}(undef, 160); path = Vector{UInt8}(undef, 1024)
    GC.@preserve name source dnx dnu dnn di cnx cnu ci knc knx knu kin ki begin
        kinds = StageKinds(Int32(T), Int32(nwu),
                           Int32(length(dk)), pointer(dnx), pointer(dnu), pointer(dnn), pointer(di),
                           Int32(length(ck)), pointer(cnx), pointer(cnu), pointer(ci),
                           Int32(length(kk)), pointer(knc), pointer(knx), pointer(knu), pointer(kin), pointer(ki),
                           Int32(ct.num_state), Int32(kt.num_constraint), Tuple(ineq_words(kt.indices_inequality)))
        check(ccall((:ilqr_compile_model_stages, LIB[]), Cint,
                    (Cstring, Ref{StageKinds}, Cstring, Ref{StagePlan}, Ptr{Float64}, Csize_t, Ptr{Int32}, Ptr{Int32},
                     Ptr{UInt8}, Csize_t, Ptr{UInt8}, Csize_t),
                    name, kinds, source, plan, selectors, cap, state_dims, action_dims, regname, length(regname), path, length(path)))
    end
    s = Solver(unsafe_string(pointer(regname)); horizon = T, batch = batch, constrained = constrained, options = options,
               device = device, devices = devices, model_library = unsafe_string(pointer(path)))
    S = plan[].n_selectors
    S > 0 && check(ccall((:ilqr_set_stage_selectors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32), s.handle, selectors, S))
    s.state_dims = Int.(state_dims); s.action_dims = Int.(action_dims)
    return s
end

# Solver(dynamics, costs) — src/solver.jl:11-26: no constraints, plain iLQR
function Solver(dynamics::Vector{Dynamics}, costs::Vector{Cost}; kwargs...)
    T = length(costs)
    return Solver(dynamics, costs, [Constraint() for _ in 1:T]; constrained = false, kwargs...)
end

# solve!(solver; augmented_lagrangian_callback! = cb) — src/solve.jl:88,125: the outer AL loop stepped from the host, one launch
# per outer iteration (ILQR_STAGE_AL_BEGIN = 7, ILQR_STAGE_AL_OUTER = 8), cb(solver) after every dual update
function solve!(s::Solver, augmented_lagrangian_callback!::Function)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    check(ccall((:ilqr_run_stage, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, 7))
    done = ccall((:ilqr_scalar_slot, LIB[]), Cint, (Cstring,), "done")
    nsc = ccall((:ilqr_scalar_slot, LIB[]), Cint, (Cstring,), "count")
    sc = Matrix{Float64}(undef, nsc, s.B)
    for _ in 1:s.options.max_dual_updates
        check(ccall((:ilqr_run_stage, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, 8))
        check(ccall((:ilqr_get_buffer, LIB[]), Cint, (Ptr{Cvoid}, Cstring, Ptr{Float64}), s.handle, "_scalars", sc))
        all(sc[done + 1, :] .!= 0.0) && break
        augmented_lagrangian_callback!(s)
    end
    return nothing
end

# solve! with ONE step size per inner iteration for the whole batch, over every process of a multi-GPU job (not a reference behaviour:
# the optional mode of include/ilqr_hip.h, ilqr_solve_shared_step). `reduce!(v::Vector{Float64})` sums v in place over all processes
# (MPI.Allreduce!(v, +, comm), an RCCL binding, ...); without it the batch of this handle shares its step size alone.
function solve_shared_step!(s::Solver, reduce!::Union{Function,Nothing} = nothing)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    cap = Int(s.options.max_dual_updates) * Int(s.options.max_iterations)
    steps = zeros(Float64, max(cap, 1)); n = Ref{Int32}(0)
    if reduce! === nothing
        check(ccall((:ilqr_solve_shared_step, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{Int32}),
                    s.handle, C_NULL, C_NULL, steps, cap, n))
    else
        cb = function (values::Ptr{Float64}, len::Int32, ::Ptr{Cvoid})::Cint
            v = unsafe_wrap(Array, values, Int(len)); reduce!(v); return Cint(0)
        end
        cfn = @cfunction($cb, Cint, (Ptr{Float64}, Int32, Ptr{Cvoid}))
        GC.@preserve cfn check(ccall((:ilqr_solve_shared_step, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int32, Ref{Int32}),
                                     s.handle, cfn, C_NULL, steps, cap, n))
    end
    return steps[1:min(Int(n[]), cap)]      # n = inner iterations taken; at most `cap` entries were written
end

# 0 = auto, 1 = latency, 2 = throughput, 3 = packed (four instances per wave, no horizon limit)
set_kernel_variant!(s::Solver, v::Integer) = check(ccall((:ilqr_set_kernel_variant, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, v))
# straggler hand-over of the packed kernel (include/ilqr_hip.h): outer = -1 by head count (default), 0 off, k >= 2 by outer iteration;
# live = survivors of the batch at which they all leave (-1 auto)
set_handover!(s::Solver, outer::Integer) = check(ccall((:ilqr_set_handover, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, outer))
set_handover_live!(s::Solver, live::Integer) = check(ccall((:ilqr_set_handover_live, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, live))
set_handover_mark!(s::Solver, rejected::Integer) = check(ccall((:ilqr_set_handover_mark, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, rejected))
function handover_stats(s::Solver)      # (instances through the workgroups' queue, instances marked as stragglers) of the last solve!
    q = Ref{Int32}(0); m = Ref{Int32}(0)
    check(ccall((:ilqr_get_handover_stats, LIB[]), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), s.handle, q, m))
    return (queued = Int(q[]), marked = Int(m[]))
end

# what `verbose` prints per inner iteration (src/solve.jl:40-45), recorded on the device: rows of
# (outer, inner, objective, gradient_norm, max_violation, step_size, status, rollouts) per instance
enable_trace!(s::Solver, capacity::Integer) = check(ccall((:ilqr_enable_trace, LIB[]), Cint, (Ptr{Cvoid}, Int32), s.handle, capacity))
function trace(s::Solver, capacity::Integer)
    out = Array{Float64,3}(undef, 8, capacity, s.B)
    check(ccall((:ilqr_get_trace, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), s.handle, out))
    return out
end

# ---- a nonlinear sensor y = h(x, s) + v compiled as a module of its own (ilqr_compile_sensor). `source` defines
# `ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s)` (include/ilqr_hip.h): what
# Symbolics.build_function(..., target = CTarget()) emits per row of h and of its Jacobian, one case of a switch each.
# ilqr_sensor_source, field for field
struct SensorSource
    name::Cstring
    nx::Int32
    ny::Int32
    ns::Int32
    source::Cstring
    flags::Int32
end

# Returns (registered name, module path). (The symbol is looked up by hand, as mpc_run_io!'s: the struct goes by reference.)
function compile_sensor(name::String, nx::Integer, ny::Integer, ns::Integer, source::String)
    reg = zeros(UInt8, 256); path = zeros(UInt8, 4096)
    GC.@preserve name source begin
        src = SensorSource(Base.unsafe_convert(Cstring, name), Int32(nx), Int32(ny), Int32(ns), Base.unsafe_convert(Cstring, source), Int32(0))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_compile_sensor)
        check(ccall(fn, Cint, (Ref{SensorSource}, Ptr{UInt8}, Csize_t, Ptr{UInt8}, Csize_t), src, reg, length(reg), path, length(path)))
    end
    return unsafe_string(pointer(reg)), unsafe_string(pointer(path))
end
load_sensor_library(path::String) = check(ccall((:ilqr_load_sensor_library, LIB[]), Cint, (Cstring,), path))
register_sensor(vtable::Ptr{Cvoid}) = check(ccall((:ilqr_register_sensor, LIB[]), Cint, (Ptr{Cvoid},), vtable))
sensor_count() = Int(ccall((:ilqr_sensor_count, LIB[]), Cint, ()))
sensor_name(i::Integer) = unsafe_string(ccall((:ilqr_sensor_name, LIB[]), Cstring, (Int32,), i))
function sensor_dims(sensor::String)
    nx = Ref{Int32}(0); ny = Ref{Int32}(0); ns = Ref{Int32}(0)
    check(ccall((:ilqr_sensor_dims, LIB[]), Cint, (Cstring, Ref{Int32}, Ref{Int32}, Ref{Int32}), sensor, nx, ny, ns))
    return Int(nx[]), Int(ny[]), Int(ns[])
end

# s :: ns shared by the batch or (ns, B) one column per instance; nothing where the sensor has no parameters
sensor_s(s) = s === nothing ? Ptr{Float64}(C_NULL) : pointer(s)
per_instance_s(s) = Int32(s !== nothing && ndims(s) == 2 ? 1 : 0)

# The sensor linearised at x_lin :: (nx, B) (ilqr_sensor_linearise). Returns (H :: (nx, ny, B), column-major here is the header's
# [B][ny][nx]; yhat :: (ny, B)); with x_prior the reference output of an iterated filter.
function sensor_linearise!(s::Solver, sensor::String, x_lin::Matrix{Float64}; sp = nothing, x_prior::Union{Nothing,Matrix{Float64}} = nothing)
    _, ny, _ = sensor_dims(sensor)
    H = Array{Float64,3}(undef, s.nx, ny, s.B); yhat = Matrix{Float64}(undef, ny, s.B)
    GC.@preserve sp begin
        check(ccall((:ilqr_sensor_linearise, LIB[]), Cint,
                    (Ptr{Cvoid}, Cstring, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    s.handle, sensor, per_instance_s(sp), sensor_s(sp), x_lin, x_prior === nothing ? Ptr{Float64}(C_NULL) : x_prior, H, yhat))
    end
    return H, yhat
end

# What the sensor reads of the plant states x :: (nx, B) (ilqr_plant_measure_sensor). Returns y :: (ny, B).
function plant_measure_sensor!(s::Solver, sensor::String, x::Matrix{Float64}; sp = nothing, step::Integer = 0,
                               sigma_y::Union{Nothing,Vector{Float64}} = nothing, seed::Integer = 0, first_instance::Integer = 0)
    _, ny, _ = sensor_dims(sensor)
    y = Matrix{Float64}(undef, ny, s.B)
    GC.@preserve sp begin
        check(ccall((:ilqr_plant_measure_sensor, LIB[]), Cint,
                    (Ptr{Cvoid}, Cstring, Int32, Ptr{Float64}, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    s.handle, sensor, per_instance_s(sp), sensor_s(sp), UInt64(seed), Int64(first_instance), Int32(step),
                    sigma_y === nothing ? Ptr{Float64}(C_NULL) : sigma_y, x, y))
    end
    return y
end

# The measurement update of the (iterated) extended Kalman filter with the sensor (ilqr_estimate_update_sensor); xhat and P are
# updated in place. Returns (innovation :: (ny, B), nis :: B, first_bad :: B).
function estimate_update_sensor!(s::Solver, sensor::String, xhat::Matrix{Float64}, P::Array{Float64,3}, y::Matrix{Float64}, r::Vector{Float64};
                                 sp = nothing, iterations::Integer = 1)
    _, ny, _ = sensor_dims(sensor)
    @assert size(xhat) == (s.nx, s.B) && size(P) == (s.nx, s.nx, s.B) && size(y) == (ny, s.B) && length(r) == ny
    innovation = Matrix{Float64}(undef, ny, s.B)
    nis = Vector{Float64}(undef, s.B)
    first_bad = Vector{Int32}(undef, s.B)
    GC.@preserve sp begin
        check(ccall((:ilqr_estimate_update_sensor, LIB[]), Cint,
                    (Ptr{Cvoid}, Cstring, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                     Ptr{Int32}),
                    s.handle, sensor, per_instance_s(sp), sensor_s(sp), Int32(iterations), r, y, xhat, P, innovation, nis, first_bad))
    end
    return innovation, nis, first_bad
end

# The device forms take raw device pointers on the handle's device (ilqr_*_device); r and sigma_y stay host vectors.
sensor_linearise_device!(s::Solver, sensor::String, per::Integer, d_s::Ptr{Float64}, d_x_lin::Ptr{Float64}, d_x_prior::Ptr{Float64}, d_H::Ptr{Float64},
                         d_yhat::Ptr{Float64}) =
    check(ccall((:ilqr_sensor_linearise_device, LIB[]), Cint,
                (Ptr{Cvoid}, Cstring, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), s.handle, sensor, Int32(per), d_s,
                d_x_lin, d_x_prior, d_H, d_yhat))
plant_measure_sensor_device!(s::Solver, sensor::String, per::Integer, d_s::Ptr{Float64}, seed::Integer, first_instance::Integer, step::Integer,
                             sigma_y::Ptr{Float64}, d_x::Ptr{Float64}, d_y::Ptr{Float64}) =
    check(ccall((:ilqr_plant_measure_sensor_device, LIB[]), Cint,
                (Ptr{Cvoid}, Cstring, Int32, Ptr{Float64}, UInt64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), s.handle, sensor, Int32(per),
                d_s, UInt64(seed), Int64(first_instance), Int32(step), sigma_y, d_x, d_y))
estimate_update_sensor_device!(s::Solver, sensor::String, per::Integer, d_s::Ptr{Float64}, iterations::Integer, r::Vector{Float64}, d_y::Ptr{Float64},
                               d_xhat::Ptr{Float64}, d_P::Ptr{Float64}, d_innovation::Ptr{Float64}, d_nis::Ptr{Float64}, d_first_bad::Ptr{Int32}) =
    check(ccall((:ilqr_estimate_update_sensor_device, LIB[]), Cint,
                (Ptr{Cvoid}, Cstring, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Int32}), s.handle, sensor, Int32(per), d_s, Int32(iterations), r, d_y, d_xhat, d_P, d_innovation, d_nis, d_first_bad))

# ilqr_nl_sensor, field for field
struct NlSensor
    sensor::Cstring
    ns_per_instance::Int32
    s::Ptr{Float64}
    r::Ptr{Float64}
    q::Ptr{Float64}
    sigma_y::Ptr{Float64}
    iterations::Int32
end

# mpc_run_sensor! with the compiled nonlinear sensor (ilqr_mpc_run_nlsensor): r and sigma_y :: ny, sp :: ns or (ns, B). Returns
# (x, u, log, first_nonfinite, y_cl :: (ny, periods, B), saturated, xhat, pdiag, nis, P0). (The symbol is looked up by hand, as
# mpc_run_io!'s.)
function mpc_run_nlsensor!(s::Solver, sensor::String, r::Vector{Float64}, P0::Array{Float64,3}; sp = nothing, iterations::Integer = 1,
                           periods::Integer, steps::Integer = 1, plant_feedback::Bool = false, shift_feedback::Bool = false,
                           shift_tail::Symbol = :hold, warm::Bool = true, duals_tail::Symbol = :hold, duals_penalty::Symbol = :keep,
                           seed::Integer = 0, first_instance::Integer = 0, sigma_x::Union{Nothing,Vector{Float64}} = nothing,
                           x0::Union{Nothing,Matrix{Float64}} = nothing, xhat0::Union{Nothing,Matrix{Float64}} = nothing,
                           q::Union{Nothing,Vector{Float64}} = nothing, sigma_y::Union{Nothing,Vector{Float64}} = nothing,
                           u_min::Union{Nothing,Vector{Float64}} = nothing, u_max::Union{Nothing,Vector{Float64}} = nothing, delay::Integer = 0)
    _, ny, _ = sensor_dims(sensor)
    @assert length(r) == ny && size(P0) == (s.nx, s.nx, s.B)
    R = periods * steps
    x = Array{Float64,3}(undef, s.nx, R + 1, s.B); u = Array{Float64,3}(undef, s.nu, R, s.B)
    log = Array{Float64,3}(undef, 9, periods, s.B); nf = Vector{Int32}(undef, s.B)
    y_cl = Array{Float64,3}(undef, ny, periods, s.B); saturated = Vector{Int32}(undef, s.B)
    xhat = Array{Float64,3}(undef, s.nx, periods, s.B); pdiag = Array{Float64,3}(undef, s.nx, periods, s.B); nis = Matrix{Float64}(undef, periods, s.B)
    nul = Ptr{Float64}(C_NULL)
    ptr(v) = v === nothing ? nul : pointer(v)
    check(ccall((:ilqr_set_options, LIB[]), Cint, (Ptr{Cvoid}, Ref{Options}), s.handle, s.options))
    GC.@preserve sensor sp r q sigma_y sigma_x u_min u_max begin
        d = MpcDesc(Int32(periods), Int32(steps), Int32(plant_feedback ? 1 : 0), Int32(shift_feedback ? 1 : 0),
                    Int32(shift_tail === :hold ? 0 : 1), Int32(warm ? 1 : 0), Int32(duals_tail === :hold ? 0 : 1),
                    Int32(duals_penalty === :keep ? 0 : 1), UInt64(seed), Int64(first_instance), ptr(sigma_x))
        io = PlantIO(ptr(u_min), ptr(u_max), nul, Int32(delay), Int32(0))
        sens = NlSensor(Base.unsafe_convert(Cstring, sensor), per_instance_s(sp), sensor_s(sp), pointer(r), ptr(q), ptr(sigma_y), Int32(iterations))
        fn = Libdl.dlsym(Libdl.dlopen(LIB[]), :ilqr_mpc_run_nlsensor)
        check(ccall(fn, Cint, (Ptr{Cvoid}, Ref{MpcDesc}, Ref{PlantIO}, Ref{NlSensor}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                               Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    s.handle, d, io, sens, x0 === nothing ? nul : x0, xhat0 === nothing ? nul : xhat0, P0, nul, nul, x, u, log, nf, nul, nul, y_cl,
                    saturated, xhat, pdiag, nis))
    end
    return x, u, log, nf, y_cl, saturated, xhat, pdiag, nis, P0
end

end # module
