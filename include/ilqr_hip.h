/*
 * ilqr_hip.h — C-ABI of the MI355X-native batched iLQR / augmented-Lagrangian solver.
 *
 * The reference (thowell/IterativeLQR.jl v0.2.3, pure Julia) has no FFI layer;
 * this header is the boundary a Julia `ccall` wrapper (or the Python ctypes
 * mirror in iterativelqr.jl_amd/) binds to. Each entry point names the reference
 * interface it replaces (paths relative to /root/reference). One handle owns a
 * BATCH of independent problem instances of one model, on one GPU (ilqr_create)
 * or split over several (ilqr_create_sharded); every instance behaves exactly
 * like one reference `Solver`.
 *
 * Conventions: every function returns 0 on success, <0 on error (never
 * throws); ilqr_last_error() gives the message. The caller owns all host
 * pointers; the handle owns device memory. Host arrays are instance-major:
 * x[b][t][i], u[b][t][j]; matrices are column-major like Julia
 * (K[b][t][col][row]). All arithmetic is fp64 (the reference is Float64 only).
 * A handle is not thread-safe. Calls that return data synchronise the stream.
 */
#ifndef ILQR_HIP_H
#define ILQR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILQR_OK 0
#define ILQR_ERR_INVALID (-1)
#define ILQR_ERR_HIP (-2)
#define ILQR_ERR_MODEL (-3)
#define ILQR_ERR_NO_DEVICE (-4)
#define ILQR_ERR_LDS (-5)

typedef struct ilqr_handle ilqr_handle;

/* Options{T} — src/options.jl:1-15, field for field (constraint_norm is
 * carried but, as in the reference, never read). line_search: 1 = :armijo,
 * 0 = :none. verbose is ignored by the device; the host mirror prints the reference's per-iteration report from the
 * trace (ilqr_enable_trace) when it is set. */
typedef struct {
    int32_t line_search;
    int32_t max_iterations;
    int32_t max_dual_updates;
    double min_step_size;
    double objective_tolerance;
    double lagrangian_gradient_tolerance;
    double constraint_tolerance;
    double constraint_norm;
    double initial_constraint_penalty;
    double scaling_penalty;
    double max_penalty;
    int32_t reset_cache;
    int32_t verbose;
} ilqr_options;

/* What `Solver(dynamics, costs[, constraints])` needs — src/solver.jl:11-46. */
typedef struct {
    const char* model;          /* built-in model name ("acrobot", "car", ...) or the
                                   name registered by a generated model library */
    const char* model_library;  /* optional path of a generated model module (.so)
                                   to dlopen first (iterativelqr.jl_amd/codegen.py) */
    int32_t horizon;            /* T (number of states) */
    int32_t batch;              /* B independent instances */
    int32_t device;             /* HIP device ordinal */
    int32_t constrained;        /* 1: Solver(dynamics, costs, constraints) → AL solve
                                   0: Solver(dynamics, costs) → plain iLQR */
} ilqr_problem_desc;

/* SolverData scalars — src/data/solver.jl:4-18 — plus bookkeeping. */
typedef struct {
    double objective;
    double gradient_norm;
    double max_violation;
    double step_size;
    int32_t iterations;        /* data.iterations (inner iterations, all outer loops) */
    int32_t outer_iterations;  /* AL iterations executed */
    int32_t status;            /* data.status of the last forward pass */
    int32_t potrf_info;        /* first non-zero LAPACK-style info of the Quu Cholesky
                                  (the reference ignores it, src/backward_pass.jl:69) */
    int32_t rollouts;          /* closed-loop rollouts executed */
    int32_t reserved;
} ilqr_stats;

const char* ilqr_last_error(void);
int ilqr_device_count(void);

/* Options() defaults — src/options.jl:1-15 */
int ilqr_default_options(ilqr_options* opt);

/* Solver(...) — src/solver.jl:11-46. Fails loudly (ILQR_ERR_NO_DEVICE) when no
 * HIP device is present: there is no CPU fallback. */
int ilqr_create(const ilqr_problem_desc* desc, ilqr_handle** out);
/* The same Solver with its batch spread over several GPUs of the node — the reference's caller holds ONE Solver and calls
 * solve! (src/solver.jl:28-46, src/solve.jl:137-143); a Julia host has no process launcher. The instances are split into
 * contiguous ranges of ceil(batch / n_devices), range i on devices[i] (desc->device is ignored; an ordinal may repeat). Inside
 * the library every range is a handle of its own with its own workspace and stream on its device; launches are asynchronous
 * on all of them, blocking copies run on one host thread per device. Every entry point below takes the returned handle
 * unchanged: host arrays stay instance-major over the WHOLE batch and are scattered / gathered over the ranges. No data
 * crosses devices (the instances are independent). Not available on it: ilqr_initialize_rollout_device and ilqr_get_stream
 * (one device's pointers / stream); ilqr_timing_get reports the slowest device. */
int ilqr_create_sharded(const ilqr_problem_desc* desc, const int32_t* devices, int32_t n_devices, ilqr_handle** out);
int ilqr_destroy(ilqr_handle* h);
int ilqr_set_options(ilqr_handle* h, const ilqr_options* opt);   /* solver.options */
int ilqr_get_dims(const ilqr_handle* h, int32_t* nx, int32_t* nu, int32_t* nw,
                  int32_t* nc_stage, int32_t* nc_term, int32_t* horizon, int32_t* batch);

/* Solver(...; parameters = θ) — src/solver.jl:12,29, src/data/problem.jl:25-30: per-instance,
 * per-timestep parameter vectors w: [B][T][nw] (the terminal entry is used by the terminal cost /
 * constraint). Only for models with num_parameter > 0; zero until set; ilqr_reset keeps them. */
int ilqr_set_parameters(ilqr_handle* h, const double* w);

/* Fresh-solver state (all buffers zero, objective = Inf) — what constructing a
 * new reference Solver gives (src/data/problem.jl:32-38, src/data/solver.jl:37). */
int ilqr_reset(ilqr_handle* h);

/* initialize_controls!(solver, ū) / initialize_states!(solver, x̄) — src/solver.jl:56-66.
 * Host pointers. */
int ilqr_initialize_controls(ilqr_handle* h, const double* u);
int ilqr_initialize_states(ilqr_handle* h, const double* x);
/* x̄ = rollout(dynamics, x1, ū) (src/rollout.jl:33-42) followed by both
 * initialisers, executed on the device. x1: [B][nx], u: [B][T-1][nu].
 * The *_device variant takes DEVICE pointers (inputs already resident in HBM)
 * and is asynchronous on the handle's stream. */
int ilqr_initialize_rollout(ilqr_handle* h, const double* x1, const double* u);
int ilqr_initialize_rollout_device(ilqr_handle* h, const double* d_x1, const double* d_u);
/* The same from the inputs the handle keeps in HBM since the last ilqr_initialize_rollout (every device of a sharded handle
 * keeps its own range): a re-solve of the same (x1, ū) — solve!(solver) again after initialize_controls!/initialize_states!,
 * src/solver.jl:56-66 — without a host-to-device copy. Asynchronous. */
int ilqr_initialize_rollout_resident(ilqr_handle* h);

/* The same from the best of `candidates` action sequences per instance. Every candidate s of instance b is rolled out open-loop
 * from x1[b] under the handle's parameters (selector columns included), x = rollout(dynamics, x1[b], u[b][s]), src/rollout.jl:33-42,
 * and scored on the device: cost = the plain objective Σ cost (src/costs.jl:48-55, summed in timestep order; not the
 * augmented-Lagrangian merit), max_violation = constraint_violation over its trajectory (src/data/constraints.jl:23-39; 0 on a
 * handle created unconstrained), first_nonfinite = −1 or the first 0-based t at which a component of x_t is not finite (as in
 * ilqr_rollout_policy). score = cost when violation_weight == 0, else cost + violation_weight · max_violation. A candidate is
 * eligible when its score is finite and its first_nonfinite is −1; chosen[b] = the eligible candidate with the lowest score, ties
 * to the lowest index, or −1 when none is eligible — candidate 0 is installed then, so the handle's state is always defined.
 * Afterwards the handle is in exactly the state ilqr_initialize_rollout(h, x1, u[:, chosen]) leaves it in (x̄, ū,
 * states_eq_nominal, the resident inputs: ilqr_initialize_rollout_resident replays the winners); policy, duals, scalars, trace
 * and timing are untouched. Refused (ILQR_ERR_INVALID) without touching the GPU: candidates < 1, null x1 or u, a negative or
 * non-finite violation_weight. Host form: stages through device buffers the handle owns and reuses; on a sharded handle every
 * instance's candidates go to the device that owns the instance. Device form: every pointer a device pointer on the handle's
 * device, asynchronous on the handle's stream; refused on a sharded handle. */
int ilqr_initialize_rollout_candidates(ilqr_handle* h, int32_t candidates, double violation_weight,
                                       const double* x1,            /* [B][nx] */
                                       const double* u,             /* [B][S][T-1][nu] */
                                       int32_t* chosen,             /* NULL, or [B] */
                                       double* cost,                /* NULL, or [B][S] */
                                       double* max_violation,       /* NULL, or [B][S] */
                                       int32_t* first_nonfinite);   /* NULL, or [B][S] */
int ilqr_initialize_rollout_candidates_device(ilqr_handle* h, int32_t candidates, double violation_weight, const double* d_x1, const double* d_u,
                                              int32_t* d_chosen, double* d_cost, double* d_max_violation, int32_t* d_first_nonfinite);

/* The same with the candidates DRAWN ON THE DEVICE around a base sequence — a sampling (MPPI-style) warm start without a host
 * array of candidates. Candidate 0 of instance b is base_u[b] itself (copied); candidate s >= 1 is
 *     u[b][s][t][j] = base_u[b][t][j] + sigma[j] · z(seed, first_instance + b, s, t, j)     (product and sum rounded separately)
 *     z(seed, b, s, t, j):  key = seed ^ (b·2^40 + s·2^24 + t·2^4 + j),  h1 = splitmix64(key),  h2 = splitmix64(h1),
 *                           U(h) = ((h >> 11) + 0.5) / 2^53,  z = sqrt(−2 · log(U(h1))) · cos(6.283185307179586 · U(h2))
 * (t the 0-based step, j the action component; on a sharded handle b counts over the whole batch). Scores, eligibility, the tie
 * rule, chosen and the "candidate 0 when nobody is eligible" rule are those of ilqr_initialize_rollout_candidates. What is
 * installed: ILQR_SAMPLE_PICK: the winner (the base for chosen == −1); ILQR_SAMPLE_BLEND: base + sigma_j · Σ_s w_s · z(b, s, t, j),
 * summed in ascending s, with w_s = exp(−(score_s − score_min) / temperature) for eligible s, 0 otherwise, divided by their sum
 * (the base when chosen == −1). Afterwards the handle is in exactly the state ilqr_initialize_rollout(h, x1, u_installed) leaves
 * it in (ilqr_initialize_rollout_resident replays it); policy, duals, scalars, trace and timing are untouched. x1 == NULL / base_u
 * == NULL: the handle's resident inputs — after ilqr_shift_horizon: the shifted start and guess. weights: blend: w; pick: 1 at
 * chosen, else 0. u_out: the candidates as drawn. sigma is a HOST pointer in both forms. Refused (ILQR_ERR_INVALID) without
 * touching the GPU: candidates < 1 or > 65536, an unknown mode, null sigma or a negative or non-finite entry of it, a negative or
 * non-finite violation_weight, blend with a temperature that is not finite and > 0, first_instance < 0 or first_instance + batch
 * > 2^23, T − 1 > 2^20, nu > 16, a null handle, a NULL x1 or base_u on a handle without resident inputs. Host form: stages through
 * device buffers the handle owns and reuses, works on a sharded handle, synchronous. Device form: every pointer but sigma a device
 * pointer on the handle's device, asynchronous on the handle's stream; refused on a sharded handle. */
#define ILQR_SAMPLE_PICK 0
#define ILQR_SAMPLE_BLEND 1
int ilqr_sample_rollout_candidates(ilqr_handle* h, int32_t candidates, int32_t mode, uint64_t seed, int64_t first_instance,
                                   const double* sigma,         /* HOST [nu], finite, >= 0 */
                                   double violation_weight, double temperature,
                                   const double* x1,            /* NULL, or [B][nx] */
                                   const double* base_u,        /* NULL, or [B][T-1][nu] */
                                   int32_t* chosen,             /* NULL, or [B] */
                                   double* cost,                /* NULL, or [B][S] */
                                   double* max_violation,       /* NULL, or [B][S] */
                                   int32_t* first_nonfinite,    /* NULL, or [B][S] */
                                   double* weights,             /* NULL, or [B][S] */
                                   double* u_out);              /* NULL, or [B][S][T-1][nu] */
int ilqr_sample_rollout_candidates_device(ilqr_handle* h, int32_t candidates, int32_t mode, uint64_t seed, int64_t first_instance,
                                          const double* sigma, double violation_weight, double temperature,
                                          const double* d_x1, const double* d_base_u, int32_t* d_chosen, double* d_cost,
                                          double* d_max_violation, int32_t* d_first_nonfinite, double* d_weights, double* d_u_out);
/* z of the definition above on the host, without a device: z[b][s][t][j] for b < batch (instance first_instance + b), s <
 * candidates, t < steps, j < nu; row s == 0 is zero. The device draws the same integers and evaluates log, sqrt and cos with its
 * own library: the two agree to a few ulp of |z| <= 8.7. Refused: a null z, batch, candidates, steps or nu < 0, candidates >
 * 65536, steps > 2^20, nu > 16, first_instance < 0 or first_instance + batch > 2^23. */
int ilqr_candidate_noise(uint64_t seed, int64_t first_instance, int32_t batch, int32_t candidates, int32_t steps, int32_t nu,
                         double* z);

/* Receding-horizon shift of a solved handle by k = `steps` control periods, on the device (N = T − 1; x̄, ū, K, θ as the handle
 * holds them when the call is made). Start state: x1'[b] = x1[b] (the measured state) if given, else x̄_k[b]. Parameters (models
 * with user parameters only): θ'_t = θ_{t+k} for t + k <= T−1; the remaining k rows are w_tail[b][t − (T−k)] if given, else
 * θ_{T−1}. Actions, feedback == 0: u'_t = ū_{t+k} for t < N−k (pure copies), then ū_{N−1} (ILQR_SHIFT_TAIL_HOLD) or 0
 * (ILQR_SHIFT_TAIL_ZERO). feedback != 0: the shifted policy run closed-loop from x1' under θ' over the head,
 * u'_t = ū_{t+k} + K_{t+k} (x'_t − x̄_{t+k}), x'_{t+1} = f(x'_t, u'_t, θ'_t), x'_0 = x1' (src/rollout.jl:24-29 with α = 0, formed as
 * (ū + K x') − K x̄), t < N−k; the tail as above, on ū without feedback — no gain exists beyond the horizon. (x1', u') go to the
 * handle's resident inputs and ilqr_initialize_rollout_device runs on them: afterwards the handle is in exactly the state
 * ilqr_set_parameters(h, θ') + ilqr_initialize_rollout(h, x1', u') leave it in, and ilqr_initialize_rollout_resident replays it.
 * K, k, P, p, duals, penalties, the named scalars, trace and timing are untouched (the policy is stale afterwards, as after every
 * initialiser). steps == 0 is allowed: with feedback and an x1 it re-anchors the nominal trajectory at a measured state.
 * Refused (ILQR_ERR_INVALID) without touching the GPU: a null handle, steps < 0 or > T−1, an unknown tail, w_tail on a model
 * without user parameters or with steps == 0, steps > 0 on a handle with stage selectors (a lowered problem's structure belongs to
 * horizon positions), feedback without a policy (the rule of ilqr_rollout_policy). Host form: x1 and w_tail are staged through
 * device buffers the handle owns and reuses; works on a sharded handle; synchronous. Device form: device pointers on the handle's
 * device, asynchronous on the handle's stream; refused on a sharded handle. */
#define ILQR_SHIFT_TAIL_HOLD 0
#define ILQR_SHIFT_TAIL_ZERO 1
int ilqr_shift_horizon(ilqr_handle* h, int32_t steps, int32_t tail, int32_t feedback,
                       const double* x1,      /* NULL, or [B][nx]: the measured states */
                       const double* w_tail); /* NULL, or [B][steps][nw_user] */
int ilqr_shift_horizon_device(ilqr_handle* h, int32_t steps, int32_t tail, int32_t feedback,
                              const double* d_x1, const double* d_w_tail);

/* Receding-horizon shift of the augmented-Lagrangian state by k = `steps` control periods, on the device, in place (N = T − 1,
 * ncs / nct stage / terminal constraint rows; λ = constraint_dual, ρ = constraint_penalty as the handle holds them, C = N·ncs + nct
 * doubles per instance, stage row t at t·ncs, the terminal rows at N·ncs). Duals: λ'_t = λ_{t+k} for t < N−k (pure copies: signs
 * of inequality rows are kept); the last k stage rows get λ_{N−1}, the old last stage row (ILQR_DUALS_TAIL_HOLD), or 0
 * (ILQR_DUALS_TAIL_ZERO); the terminal rows stay where they are — the terminal constraint stays at the end of the horizon.
 * Penalties, ILQR_DUALS_PENALTY_KEEP: ρ moves exactly as λ does, tail rows under HOLD copy the old last stage row, under ZERO they
 * get the handle's initial_constraint_penalty; ILQR_DUALS_PENALTY_RESET: every entry of ρ becomes initial_constraint_penalty.
 * steps == 0 is allowed: KEEP is then the identity, RESET resets ρ only. Nothing else of the handle changes: trajectory, policy, θ,
 * scalars, trace, timing, resident inputs. The companion of ilqr_shift_horizon, which leaves duals and penalties untouched.
 * Refused (ILQR_ERR_INVALID) without touching the GPU: a null handle, a handle created unconstrained, steps < 0 or > T−1, an
 * unknown tail or penalty, steps > 0 on a handle with stage selectors (the rule of ilqr_shift_horizon, for its reason), a handle
 * that holds no duals yet — duals are held after ilqr_solve / ilqr_solve_warm on a constrained handle, ILQR_STAGE_AL_BEGIN,
 * ilqr_solve_shared_step or a host write of constraint_penalty through ilqr_set_buffer, until ilqr_reset; on a sharded handle
 * every shard must hold them. Host form: synchronous, works on a sharded handle. Device form: asynchronous on the handle's stream;
 * refused on a sharded handle. */
#define ILQR_DUALS_TAIL_HOLD 0
#define ILQR_DUALS_TAIL_ZERO 1
#define ILQR_DUALS_PENALTY_KEEP 0
#define ILQR_DUALS_PENALTY_RESET 1
int ilqr_shift_duals(ilqr_handle* h, int32_t steps, int32_t tail, int32_t penalty);
int ilqr_shift_duals_device(ilqr_handle* h, int32_t steps, int32_t tail, int32_t penalty);

/* solve!(solver) — src/solve.jl:137-143. Asynchronous: enqueues the whole
 * AL/iLQR solve of every instance on the handle's stream. */
int ilqr_solve(ilqr_handle* h);
/* ilqr_solve with src/solve.jl:95-103 (λ ← 0, ρ ← ρ0) skipped: the solve uses the duals and penalties the workspace holds, e.g.
 * those of the last solve moved along by ilqr_shift_duals. reset!(solver.data) (:93) and everything else run unchanged: the
 * Lagrangian gradient and the scalars are zeroed, outer_iterations counts from 1. This is not a reference behaviour — the reference
 * opens every constrained solve cold. Every kernel family honours it (hand-over included); asynchronous, sharded-capable and timed
 * like ilqr_solve. Refused (ILQR_ERR_INVALID): a null handle, a handle created unconstrained, a handle that holds no duals (the
 * rule above: with ρ = 0 everywhere the solve would silently be the unconstrained one). */
int ilqr_solve_warm(ilqr_handle* h);
int ilqr_synchronize(ilqr_handle* h);

/* The plant of a closed MPC loop, on the device: every instance's plant state x[b] is advanced by k = `steps` control periods under
 * the head of the handle's plan, horizon positions 0 .. k−1 of x̄, ū, K, θ as the handle holds them when the call is made. For
 * i = 0 .. k−1, with g = step0 + i the global plant step:
 *     u_i = ū_i (feedback == 0), else ū_i + K_i (x − x̄_i)   (src/rollout.jl:24-28 as ilqr_rollout_policy forms it with step_size = 0:
 *                                                            (ū + K x) − K x̄)
 *     w_i = the user's columns of w_plant[b][i] if given (a plant / model mismatch), else of θ_i; the selector columns of a lowered
 *           problem are always θ_i's
 *     x ← f(x, u_i, w_i), then x_j ← x_j + sigma_x[j] · z(seed, first_instance + b, 1 + j / 16, g, j % 16) for every component j
 *           with sigma_x[j] != 0 (product and sum rounded separately)
 * z is the z of ilqr_sample_rollout_candidates, its candidate field carrying the state component's high bits offset by one:
 * ilqr_candidate_noise(seed, first_instance, B, 1 + ceil(nx / 16), step0 + k, 16, z) is the host twin (its row 0 is zero by
 * contract; the offset keeps every drawn component out of it). x_out: the plant states, row 0 the input state; u_out: the actions
 * applied; first_nonfinite: −1, or the first i with a non-finite component of the state after step i. The call READS the handle, as
 * ilqr_rollout_policy does: workspace, scalars, trace, timing and resident inputs are untouched. Refused (ILQR_ERR_INVALID) without
 * touching the GPU: a null handle or x, steps < 1 or > T−1, step0 < 0 or step0 + steps > 2^20, first_instance < 0 or first_instance
 * + batch > 2^23, a negative or non-finite sigma_x entry, nx > 64, w_plant on a model without user parameters, feedback without a
 * policy (the rule of ilqr_rollout_policy). Host form: stages through device buffers the handle owns and reuses, works on a
 * sharded handle (b counts over the whole batch), synchronous. Device form: every pointer but sigma_x a device pointer on the
 * handle's device, asynchronous on the handle's stream; refused on a sharded handle. */
int ilqr_plant_step(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                    const double* sigma_x,     /* HOST, NULL or [nx], finite, >= 0 */
                    const double* w_plant,     /* NULL, or [B][steps][nw_user] */
                    double* x,                 /* [B][nx], in: plant state, out: plant state after k steps */
                    double* x_out,             /* NULL, or [B][steps+1][nx]  (row 0 = the input state) */
                    double* u_out,             /* NULL, or [B][steps][nu]    (the actions applied) */
                    int32_t* first_nonfinite); /* NULL, or [B] */
int ilqr_plant_step_device(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                           const double* sigma_x, const double* d_w_plant, double* d_x, double* d_x_out, double* d_u_out,
                           int32_t* d_first_nonfinite);

/* The closed MPC loop of B controllers over P = periods re-solves, enqueued once and synchronised once. From the plant state x0[b]
 * (NULL: x̄_0 of the handle) the call runs for p = 0 .. P−1, with k = steps, on a plant state that stays on the device:
 *   1. ilqr_plant_step_device(k, plant_feedback, seed, first_instance, step0 = p·k, sigma_x, w_plant rows p·k .., ...)
 *   2. ilqr_shift_horizon_device(k, shift_tail, shift_feedback, x1 = the plant state, NULL)
 *   3. warm: ilqr_shift_duals_device(k, duals_tail, duals_penalty)
 *   4. warm: ilqr_solve_warm, else ilqr_solve
 *   5. row p of the log: the nine scalars of ilqr_stats of every instance, as doubles, in ilqr_stats order
 * and leaves the handle in exactly the state that sequence of calls leaves it in. x_cl: the plant states of the run (row 0 = x0);
 * u_cl: the actions applied; first_nonfinite: −1, or the global plant step index of the first non-finite plant state. The arrays
 * of the run live in device buffers the handle owns and reuses; they are copied out after the one synchronise at the end. Refused
 * (ILQR_ERR_INVALID) before any launch: a null descriptor, periods < 1, periods · steps > 2^20, everything ilqr_plant_step,
 * ilqr_shift_horizon and ilqr_shift_duals refuse for these arguments (a handle with stage selectors among them), warm on a handle
 * created unconstrained or without duals, either feedback without a policy. Works on a sharded handle: every device runs its
 * shard's loop. */
typedef struct {
    int32_t periods;          /* P >= 1 re-solves */
    int32_t steps;            /* k >= 1 control periods between re-solves */
    int32_t plant_feedback;   /* the plant applies ū + K (x − x̄) instead of ū */
    int32_t shift_feedback;   /* feedback argument of ilqr_shift_horizon */
    int32_t shift_tail;       /* ILQR_SHIFT_TAIL_* */
    int32_t warm;             /* 1: ilqr_shift_duals + ilqr_solve_warm; 0: ilqr_solve (cold) */
    int32_t duals_tail, duals_penalty;   /* ILQR_DUALS_*; read when warm */
    uint64_t seed; int64_t first_instance;
    const double* sigma_x;    /* HOST, NULL or [nx] */
} ilqr_mpc_desc;
#define ILQR_MPC_LOG_W 9      /* objective, gradient_norm, max_violation, step_size, iterations, outer_iterations, status, potrf_info, rollouts — ilqr_stats order */
int ilqr_mpc_run(ilqr_handle* h, const ilqr_mpc_desc* d,
                 const double* x0,          /* NULL (= x̄_0 of the handle), or [B][nx] */
                 const double* w_plant,     /* NULL, or [B][P*k][nw_user] */
                 double* x_cl,              /* NULL, or [B][P*k+1][nx] */
                 double* u_cl,              /* NULL, or [B][P*k][nu] */
                 double* log,               /* NULL, or [B][P][ILQR_MPC_LOG_W] */
                 int32_t* first_nonfinite); /* NULL, or [B]: global plant step index, or -1 */

/* The score of plant steps, on the device: the realised stage cost and constraint violation of the states a plant visited and the
 * actions it applied — what a closed loop is judged by, as opposed to the predicted objective and violation of ilqr_stats. For
 * i = 0 .. k−1, k = `steps`, with x_i = x[b][i] (the state the action was applied from) and u_i = u[b][i]:
 *     w_i = the user's columns of w_plant[b][i] if given, else of θ_i as the handle holds them when the call is made; the selector
 *           columns of a lowered problem are always θ_i's   (the rule of ilqr_plant_step)
 *     cost[b][i]      = the stage cost at (x_i, u_i, w_i)     (src/costs.jl:48-55: one stage term; no terminal term)
 *     violation[b][i] = max over the stage constraint rows of max(0, c) (inequality rows) or |c| (equality rows) at (x_i, u_i, w_i),
 *                       NaN-propagating (src/data/constraints.jl:23-39); 0 on a handle created unconstrained or when nc_stage == 0
 * Nothing is summed: every element is a pure function of its own three rows, so its bits depend neither on the batch nor on
 * `steps` nor on its neighbours, and a non-finite row reaches no other element. To be called while the handle still holds the plan
 * the steps were taken under (ilqr_shift_horizon overwrites θ_0 .. θ_{k−1}). The call READS the handle, as ilqr_plant_step does.
 * Refused (ILQR_ERR_INVALID) without touching the GPU: steps < 1 or > T−1, a null x, u or cost, a null handle, w_plant on a model
 * without user parameters. Host form: stages through device buffers the handle owns and reuses, works on a sharded handle,
 * synchronous. Device form: every pointer a device pointer on the handle's device, asynchronous on the handle's stream; refused on
 * a sharded handle. */
int ilqr_plant_score(ilqr_handle* h, int32_t steps,
                     const double* w_plant,     /* NULL, or [B][steps][nw_user] */
                     const double* x,           /* [B][steps+1][nx]: ilqr_plant_step's x_out (row `steps` is not read) */
                     const double* u,           /* [B][steps][nu]:   ilqr_plant_step's u_out */
                     double* cost,              /* [B][steps] */
                     double* violation);        /* NULL, or [B][steps] */
int ilqr_plant_score_device(ilqr_handle* h, int32_t steps, const double* d_w_plant, const double* d_x, const double* d_u, double* d_cost,
                            double* d_violation);

/* ilqr_mpc_run following a previewed parameter stream, and scored. Per period p the loop of ilqr_mpc_run gains
 *   1b. cl_cost given: ilqr_plant_score_device(k, w_plant rows p·k .., the plant states and actions of step 1) into rows p·k .. p·k+k−1
 *       of cl_cost / cl_violation — before the shift, which overwrites the θ rows the plant ran under
 *   2.  w_preview given: ilqr_shift_horizon_device(..., w_tail = rows p·k .. p·k+k−1 of w_preview[b]) — the k parameter rows that
 *       enter the horizon are the caller's (a reference trajectory, a moving obstacle, a scheduled set-point) instead of copies of
 *       the old last row. After P periods θ_t is the original θ_{t+P·k} where t + P·k <= T−1, else w_preview[b][t + P·k − T].
 * With w_preview, cl_cost and cl_violation NULL the call is ilqr_mpc_run, bit for bit. Still one enqueue and one synchronise; every
 * buffer of the run is allocated before its first launch. Refused (ILQR_ERR_INVALID) before any launch: everything ilqr_mpc_run
 * refuses, w_preview on a model without user parameters, cl_violation without cl_cost. Works on a sharded handle. */
int ilqr_mpc_run_preview(ilqr_handle* h, const ilqr_mpc_desc* d,
                         const double* x0,          /* NULL (= x̄_0 of the handle), or [B][nx] */
                         const double* w_plant,     /* NULL, or [B][P*k][nw_user] */
                         const double* w_preview,   /* NULL, or [B][P*k][nw_user] */
                         double* x_cl,              /* NULL, or [B][P*k+1][nx] */
                         double* u_cl,              /* NULL, or [B][P*k][nu] */
                         double* log,               /* NULL, or [B][P][ILQR_MPC_LOG_W] */
                         int32_t* first_nonfinite,  /* NULL, or [B]: global plant step index, or -1 */
                         double* cl_cost,           /* NULL, or [B][P*k]: realised stage cost of every plant step */
                         double* cl_violation);     /* NULL, or [B][P*k]: realised stage violation; needs cl_cost */

/* The seam between plant and controller: actuator limits, measurement noise and a compute delay.
 *
 * ilqr_plant_step_limited is ilqr_plant_step with an actuator that saturates. After the action is formed, feedback included, and
 * before it is recorded in u_out and handed to the dynamics, every component r is limited by plain comparisons:
 *     u ← u < u_min[r] ? u_min[r] : (u > u_max[r] ? u_max[r] : u)
 * so a NaN action stays NaN (first_nonfinite marks the state it produces) and a limit of ∓Inf leaves every finite action bit for
 * bit. A null u_min (u_max) is no limit on that side; with both null the call is ilqr_plant_step, bit for bit. u_out records the
 * action APPLIED, so ilqr_plant_score of it judges what the actuator did. saturated[b]: the number of (step, component) pairs with
 * u < u_min[r] or u > u_max[r]. Refused (ILQR_ERR_INVALID) without touching the GPU: everything ilqr_plant_step refuses, a NaN
 * limit, u_min[r] > u_max[r], limits on a model with nu > 16 (they travel by value, as sigma_x does). Host and device form as
 * ilqr_plant_step's: u_min and u_max are HOST arrays in both. */
int ilqr_plant_step_limited(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                            const double* sigma_x,     /* HOST, NULL or [nx], finite, >= 0 */
                            const double* u_min,       /* HOST, NULL or [nu]: no NaN; -Inf = no limit */
                            const double* u_max,       /* HOST, NULL or [nu]: no NaN, >= u_min; +Inf = no limit */
                            const double* w_plant,     /* NULL, or [B][steps][nw_user] */
                            double* x,                 /* [B][nx], in: plant state, out: plant state after k steps */
                            double* x_out,             /* NULL, or [B][steps+1][nx]  (row 0 = the input state) */
                            double* u_out,             /* NULL, or [B][steps][nu]    (the actions applied) */
                            int32_t* first_nonfinite,  /* NULL, or [B] */
                            int32_t* saturated);       /* NULL, or [B] */
int ilqr_plant_step_limited_device(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                                   const double* sigma_x, const double* u_min, const double* u_max, const double* d_w_plant, double* d_x,
                                   double* d_x_out, double* d_u_out, int32_t* d_first_nonfinite, int32_t* d_saturated);

/* What a controller is given of a plant state: for every instance b and state component j
 *     y[b][j] = x[b][j]                                                                       (sigma_y NULL, or sigma_y[j] == 0)
 *     y[b][j] = x[b][j] + sigma_y[j] · z(seed, first_instance + b, 5 + j / 16, step, j % 16)  (product and sum rounded separately)
 * z as in ilqr_plant_step; `step` is the number of plant steps taken when the measurement is made. The process noise of
 * ilqr_plant_step draws from candidate fields 1 .. 4 and the measurement from 5 .. 8, so under one seed the two streams are disjoint:
 * ilqr_candidate_noise(seed, first_instance, B, 9, step + 1, 16, z) is the host twin (rows 5 .., step `step`). The call reads
 * nothing of the handle but its dimensions, device and stream. Refused (ILQR_ERR_INVALID) without touching the GPU: a null handle, x
 * or y, step < 0 or >= 2^20, first_instance < 0 or first_instance + batch > 2^23, a negative or non-finite sigma_y entry, nx > 64.
 * Host form: works on a sharded handle, synchronous. Device form: x and y device pointers (they may be the same array),
 * asynchronous on the handle's stream; refused on a sharded handle. */
int ilqr_plant_measure(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step,
                       const double* sigma_y,          /* HOST, NULL or [nx], finite, >= 0 */
                       const double* x,                /* [B][nx] */
                       double* y);                     /* [B][nx] */
int ilqr_plant_measure_device(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, const double* sigma_y, const double* d_x,
                              double* d_y);

/* ilqr_mpc_run_preview with the seam in the loop. The plant state xp stays the truth; the controller works from its own view xc of it.
 * Per period p, with k = steps:
 *   delay == 1, before the plant launch: xc = ilqr_plant_measure_device(step = p·k, sigma_y, xp), then xc moves on by k steps under
 *       the head of the plan in flight — ilqr_plant_step_limited_device with the same feedback flag and limits, no sigma_x, no
 *       w_plant, no outputs: the controller's model prediction of time (p+1)·k from a measurement one period old, which is when a
 *       solve that takes one period has to start
 *   1.  ilqr_plant_step_limited_device on xp as in ilqr_mpc_run, with u_min, u_max; saturated accumulates over the run
 *   delay == 0, after the plant launch: xc = ilqr_plant_measure_device(step = (p+1)·k, sigma_y, xp)
 *   y_cl[b][p] = xc, what the controller was given; 1b .. 5 as before, the shift with x1 = xc.
 * x_cl, u_cl, cl_cost and cl_violation report the true plant and the actions applied. Still one enqueue and one synchronise, every
 * buffer grown before the first launch. With io NULL — or all its pointers NULL and delay 0 — and y_cl and saturated NULL the call is
 * ilqr_mpc_run_preview: no launch, buffer or argument differs. Refused (ILQR_ERR_INVALID) before any launch: everything
 * ilqr_mpc_run_preview, ilqr_plant_step_limited and ilqr_plant_measure refuse for these arguments (a measurement step >= 2^20:
 * with delay 0 the last one is taken at P·k), delay not 0 or 1. Works on a sharded handle. */
typedef struct {
    const double* u_min;      /* HOST, NULL or [nu] */
    const double* u_max;      /* HOST, NULL or [nu] */
    const double* sigma_y;    /* HOST, NULL or [nx] */
    int32_t delay;            /* 0: the re-solve starts from a measurement of the state it is applied from; 1: from a one-period prediction */
    int32_t reserved;
} ilqr_plant_io;
int ilqr_mpc_run_io(ilqr_handle* h, const ilqr_mpc_desc* d,
                    const ilqr_plant_io* io,   /* NULL: none */
                    const double* x0,          /* NULL (= x̄_0 of the handle), or [B][nx] */
                    const double* w_plant,     /* NULL, or [B][P*k][nw_user] */
                    const double* w_preview,   /* NULL, or [B][P*k][nw_user] */
                    double* x_cl,              /* NULL, or [B][P*k+1][nx] */
                    double* u_cl,              /* NULL, or [B][P*k][nu]: the actions applied */
                    double* log,               /* NULL, or [B][P][ILQR_MPC_LOG_W] */
                    int32_t* first_nonfinite,  /* NULL, or [B]: global plant step index, or -1 */
                    double* cl_cost,           /* NULL, or [B][P*k] */
                    double* cl_violation,      /* NULL, or [B][P*k]; needs cl_cost */
                    double* y_cl,              /* NULL, or [B][P][nx]: what the controller was given per period */
                    int32_t* saturated);       /* NULL, or [B] */

/* An extended Kalman filter between the plant's sensor and the controller, batched on the device. Per instance b: the estimate
 * x̂ [nx]; its covariance P [nx][nx], row-major, symmetric, both triangles stored; q [nx] the process noise variances (diagonal Q);
 * r [nx] the measurement noise variances (diagonal R); measured [nx] a 0/1 mask (NULL: every component is measured).
 *
 * ilqr_estimate_predict, the time update over k = steps control periods under the head of the handle's plan, for i = 0 .. k−1:
 *     u_i = what ilqr_plant_step_limited forms from the state it is handed, here x̂: ū_i, or with feedback ū_i + K_i (x̂ − x̄_i),
 *           then the limits
 *     w_i = θ_i as the handle holds it (the filter knows the controller's model only: there is no w_plant); the selector columns
 *           of a lowered problem follow ilqr_plant_step's rule
 *     F   = ∂f/∂x (x̂, u_i, w_i), the model's own dynamics state Jacobian — the one the solver linearises with — taken before the
 *           state moves
 *     x̂  ← f(x̂, u_i, w_i), no noise: bit for bit the state ilqr_plant_step_limited_device gives from the same input with the same
 *           flag and limits and no sigma_x
 *     P  ← F P Fᵀ + diag(q): the elements with row >= column are computed and each is copied to its mirror, so the stored matrix
 *           is exactly symmetric. The summation order inside the two products is the kernel's; it depends on the model's sizes
 *           alone: the same instance gives the same bits in any batch.
 * ilqr_estimate_update, the measurement update with y [nx]: for j = 0 .. nx−1 in increasing order where measured[j], on the x̂ and P
 * the previous j left:
 *     ν_j = y_j − x̂_j,  s_j = P_jj + r_j. If s_j is not a finite number > 0 the component is skipped and first_bad[b] becomes j
 *           (the first such j is kept; −1 if there is none)
 *     g = P[:, j] / s_j;  x̂ ← x̂ + g · ν_j;  P_ab ← P_ab − g_a · P_jb for a >= b, from the column and row as they were before this j,
 *           then mirrored
 *     nis[b] = Σ_j ν_j² / s_j over the components that were updated; innovation[b][j] = ν_j, or 0 where the component was not
 *           measured or was skipped
 * R being diagonal, the sequence equals the batch update with S = H P Hᵀ + R, and nis equals νᵀ S⁻¹ ν.
 * Both calls read the handle and change none of its state. Refused (ILQR_ERR_INVALID) before any launch: everything
 * ilqr_plant_step_limited refuses for the same arguments; a null xhat, P, y or r; a negative or non-finite q entry; an r entry that
 * is not finite and > 0 at a measured component; a mask entry other than 0 or 1; nx > 64. Host forms: work on a sharded handle,
 * synchronous. Device forms: xhat, P, y, innovation, nis and first_bad device pointers, asynchronous on the handle's stream;
 * refused on a sharded handle. */
int ilqr_estimate_predict(ilqr_handle* h, int32_t steps, int32_t feedback,
                          const double* u_min,            /* HOST, NULL or [nu]: ilqr_plant_step_limited's rules */
                          const double* u_max,            /* HOST, NULL or [nu] */
                          const double* q,                /* HOST, NULL (= 0) or [nx], finite, >= 0 */
                          double* xhat,                   /* [B][nx] in / out */
                          double* P);                     /* [B][nx][nx] in / out */
int ilqr_estimate_predict_device(ilqr_handle* h, int32_t steps, int32_t feedback, const double* u_min, const double* u_max, const double* q,
                                 double* d_xhat, double* d_P);
int ilqr_estimate_update(ilqr_handle* h,
                         const int32_t* measured,         /* HOST, NULL or [nx] of 0 / 1 */
                         const double* r,                 /* HOST [nx]; finite and > 0 where measured */
                         const double* y,                 /* [B][nx]; unmeasured components are not read */
                         double* xhat,                    /* [B][nx] in / out */
                         double* P,                       /* [B][nx][nx] in / out */
                         double* innovation,              /* NULL, or [B][nx] */
                         double* nis,                     /* NULL, or [B] */
                         int32_t* first_bad);             /* NULL, or [B] */
int ilqr_estimate_update_device(ilqr_handle* h, const int32_t* measured, const double* r, const double* d_y, double* d_xhat, double* d_P,
                                double* d_innovation, double* d_nis, int32_t* d_first_bad);

/* A state covariance propagated down the handle's plan under its feedback policy: how far the closed-loop state and the actions are
 * expected to stray from the plan at each step of the horizon, to first order, when the plan starts from an estimate with covariance
 * P0 (the filter's P) and the model is disturbed by process noise of variances q. S = steps, 1 <= S <= T − 1; feedback 0 or 1;
 * P0 [B][nx][nx] row-major: only the elements with row >= column are read, and they are mirrored. For t = 0 .. S−1, with Σ_0 = P0:
 *     A   = ∂f/∂x, Bm = ∂f/∂u at (x̄_t, ū_t, θ_t) as the handle holds them — the NOMINAL point of the plan, not an estimate — the
 *           model's own dynamics Jacobians, the ones the solver linearises with; the selector columns of a lowered problem are θ_t's
 *     Φ   = A + Bm · K_t where feedback, else Φ = A. With feedback == 0, K is not read: a NaN in K changes nothing
 *     udiag[b][t][r] = Σ_a Σ_b K_t(r, a) Σ_t(a, b) K_t(r, b) where feedback, else 0: the variance of action r
 *     Σ_{t+1} = Φ Σ_t Φᵀ + diag(q): the elements with row >= column are computed and each is copied to its mirror, so the stored
 *           matrix is exactly symmetric
 * Outputs, every one may be NULL, but not all of them together: sdiag [B][S+1][nx] the diagonals of Σ_0 .. Σ_S; udiag [B][S][nu];
 * sigma [B][S+1][nx][nx] every Σ_t; P_out [B][nx][nx] = Σ_S, which may alias P0; first_nonfinite [B]: −1, or the first t in 0 .. S
 * with a non-finite entry on the diagonal of Σ_t — that instance's later outputs are unspecified, other instances are unaffected.
 * The summation orders are the kernel's; they are fixed by the model's sizes alone, so an instance's bits depend neither on B nor on
 * its neighbours, nor on which optional outputs are asked for.
 * The call READS the handle: workspace, scalars, statistics, trace and timing are unchanged. Refused (ILQR_ERR_INVALID) before any
 * launch: steps out of range; feedback other than 0 or 1; a null P0; all outputs null; a negative or non-finite q entry; nx > 64 or
 * nu > 16; feedback == 1 on a handle that holds no policy yet (ilqr_rollout_policy's rule). Host form: synchronous, works on a
 * sharded handle (each instance goes to the device that owns it). Device form: every array a device pointer, asynchronous on the
 * handle's stream, refused on a sharded handle.
 * Not offered: actuator limits (a saturated action has no gain); a non-diagonal Q; measurement updates along the horizon;
 * constraint-row variances and automatic back-offs; integration into ilqr_mpc_run_* — the device form on the handle's stream is what
 * a caller enqueues between their own per-period calls. */
int ilqr_plan_covariance(ilqr_handle* h, int32_t steps, int32_t feedback,
                         const double* q,                 /* HOST, NULL (= 0) or [nx], finite, >= 0 */
                         const double* P0,                /* [B][nx][nx] */
                         double* sdiag,                   /* NULL, or [B][S+1][nx] */
                         double* udiag,                   /* NULL, or [B][S][nu] */
                         double* sigma,                   /* NULL, or [B][S+1][nx][nx] */
                         double* P_out,                   /* NULL, or [B][nx][nx]; may alias P0 */
                         int32_t* first_nonfinite);       /* NULL, or [B] */
int ilqr_plan_covariance_device(ilqr_handle* h, int32_t steps, int32_t feedback, const double* q, const double* d_P0, double* d_sdiag,
                                double* d_udiag, double* d_sigma, double* d_P_out, int32_t* d_first_nonfinite);

/* ilqr_mpc_run_io with the filter between sensor and controller. Per period p, with k = steps:
 *   delay == 0:  1. the plant step on xp;  2. y = ilqr_plant_measure_device(step = (p+1)·k, sigma_y, xp);
 *                3. ilqr_estimate_predict_device(k, plant_feedback, the limits, q) under the plan in flight;
 *                4. ilqr_estimate_update_device(y);  5. xc = x̂
 *   delay == 1, before the plant launch:  1. y = measure(step = p·k);  2. the update;  3. the prediction of k steps under the plan in
 *                flight;  4. xc = x̂, which now stands at time (p+1)·k;  5. then the plant step
 * and the loop goes on as ilqr_mpc_run_io's: the shift with x1 = xc, and so on. y_cl[b][p] is the measurement taken, every component as
 * ilqr_plant_measure writes it; xhat_cl[b][p] = xc; pdiag_cl[b][p] the diagonal of P at that moment; nis_cl[b][p] that period's nis. P
 * holds P0 on entry and the last covariance on return. Still one enqueue and one synchronise, every buffer grown before the first
 * launch. With est NULL the call is ilqr_mpc_run_io: no launch, buffer or argument differs. Refused (ILQR_ERR_INVALID) before any
 * launch: everything ilqr_mpc_run_io and the two estimator calls refuse; est with P NULL; xhat0, P, xhat_cl, pdiag_cl or nis_cl
 * without est. Works on a sharded handle. */
typedef struct {
    const int32_t* measured;   /* HOST, NULL or [nx] */
    const double* q;           /* HOST, NULL or [nx] */
    const double* r;           /* HOST, [nx] */
} ilqr_estimator;
int ilqr_mpc_run_est(ilqr_handle* h, const ilqr_mpc_desc* d,
                     const ilqr_plant_io* io,   /* NULL: none */
                     const ilqr_estimator* est, /* NULL: ilqr_mpc_run_io */
                     const double* x0,          /* NULL (= x̄_0 of the handle), or [B][nx] */
                     const double* xhat0,       /* NULL (= the first plant state), or [B][nx] */
                     double* P,                 /* [B][nx][nx] in: P0, out: the last covariance */
                     const double* w_plant, const double* w_preview, double* x_cl, double* u_cl, double* log, int32_t* first_nonfinite,
                     double* cl_cost, double* cl_violation, double* y_cl, int32_t* saturated,       /* as ilqr_mpc_run_io's */
                     double* xhat_cl,           /* NULL, or [B][P][nx] */
                     double* pdiag_cl,          /* NULL, or [B][P][nx] */
                     double* nis_cl);           /* NULL, or [B][P] */

/* A linear sensor for the filter and the loop: y = H x + v, v ~ N(0, diag(r)), with ny outputs, 1 <= ny <= 64; ny may be smaller or
 * LARGER than nx (an absolute link angle q1 + q2, two redundant sensors of one state, a combination of modes). Per instance b:
 * x̂ [nx]; P [nx][nx], row-major, symmetric, both triangles stored; H [ny][nx], row-major, shared by the batch (per_instance_H == 0) or
 * one per instance, [B][ny][nx] (per_instance_H == 1); r [ny]; y [ny]; optionally ŷ [ny].
 *
 * ilqr_estimate_update_linear, the measurement update. On entry c_j = 0, or with yhat given c_j = ŷ_j − h_j·x̂₀, where x̂₀ is the
 * estimate on entry and h_j row j of H: ŷ is then the caller's h(x̂₀) of a nonlinear sensor and H its ∂h/∂x there, linearised once at
 * the prior as an extended Kalman filter does. For j = 0 .. ny−1 in increasing order, on the x̂ and P the previous j left:
 *     d   = P h_jᵀ, nx sums over the ascending column index
 *     s_j = h_j·d + r_j;  ν_j = (y_j − c_j) − h_j·x̂. If s_j is not a finite number > 0 the row is skipped and first_bad[b] becomes j
 *           (the first such j is kept; −1 if there is none)
 *     g = d / s_j;  x̂ ← x̂ + g · ν_j;  P_ab ← P_ab − g_a · d_b for a >= b, from d as it was, then mirrored: the stored matrix is
 *           exactly symmetric
 *     nis[b] = Σ_j ν_j² / s_j over the rows that were updated; innovation[b][j] = ν_j, or 0 where the row was skipped
 * R being diagonal, the sequence equals the batch update with S = H P Hᵀ + R. The order inside every sum is the kernel's and depends
 * on the model's sizes and ny alone: the same instance gives the same bits in any batch. The call reads nothing of the handle but
 * its dimensions, device and stream.
 *
 * ilqr_plant_measure_linear, the measurement: y[b][j] = Σ_k H_jk x[b][k], one FMA chain over ascending k starting from +0, then
 * + sigma_y[j] · z(seed, first_instance + b, 5 + j / 16, step, j % 16) where sigma_y[j] != 0, product and sum rounded separately; z is
 * ilqr_plant_measure's, unchanged. The key fields are 5 .. 8 — the SAME fields and the same host
 * twin as ilqr_plant_measure's, ilqr_candidate_noise(seed, first_instance, B, 9, step + 1, 16, z): a run uses one kind of measurement
 * or the other, never both, so sharing the stream is intended. With H the identity the result is ilqr_plant_measure's.
 *
 * Refused (ILQR_ERR_INVALID) before any launch: ny < 1 or ny > 64; a null handle, H, r, y, x, xhat or P; per_instance_H other than
 * 0 or 1; a non-finite entry of an H given on the host; an r entry that is not finite and > 0; a negative or non-finite sigma_y entry;
 * nx > 64; for the measurement everything ilqr_plant_measure refuses. Host forms: every array a host array; work on a sharded handle;
 * synchronous. Device forms: H, y, yhat, xhat, P, innovation, nis, first_bad (update) and H, x, y (measurement) device pointers; r
 * and sigma_y stay host arrays of ny <= 64 doubles, which travel in the argument segment of a one-wave launch that writes them to
 * the handle's buffer: they are read when the call is made, so the caller's array may go away at once, successive calls may carry
 * different values, and nothing waits for the stream. Asynchronous on the handle's stream; refused on a sharded handle. */
int ilqr_estimate_update_linear(ilqr_handle* h, int32_t ny, int32_t per_instance_H,
                                const double* H,           /* [ny][nx], or [B][ny][nx] */
                                const double* r,           /* HOST [ny], finite, > 0 */
                                const double* y,           /* [B][ny] */
                                const double* yhat,        /* NULL, or [B][ny] */
                                double* xhat,              /* [B][nx] in / out */
                                double* P,                 /* [B][nx][nx] in / out */
                                double* innovation,        /* NULL, or [B][ny] */
                                double* nis,               /* NULL, or [B] */
                                int32_t* first_bad);       /* NULL, or [B] */
int ilqr_estimate_update_linear_device(ilqr_handle* h, int32_t ny, int32_t per_instance_H, const double* d_H, const double* r, const double* d_y,
                                       const double* d_yhat, double* d_xhat, double* d_P, double* d_innovation, double* d_nis,
                                       int32_t* d_first_bad);
int ilqr_plant_measure_linear(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, int32_t ny,
                              const double* H,             /* HOST [ny][nx] */
                              const double* sigma_y,       /* HOST, NULL or [ny], finite, >= 0 */
                              const double* x,             /* [B][nx] */
                              double* y);                  /* [B][ny] */
int ilqr_plant_measure_linear_device(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, int32_t ny, const double* d_H,
                                     const double* sigma_y, const double* d_x, double* d_y);

/* ilqr_mpc_run_est's loop with the linear sensor in the place of the selection of state components: the measurement becomes
 * ilqr_plant_measure_linear_device(ny, the shared H, sensor->sigma_y), taken at the same step index, and the update
 * ilqr_estimate_update_linear_device(ny, shared H, r, no yhat). The time update (with sensor->q), the order of the four calls per
 * delay, xc = x̂ and the logs xhat_cl, pdiag_cl, nis_cl are ilqr_mpc_run_est's. y_cl[b][p] is the measurement taken, ny numbers. H, r
 * and sigma_y are copied to the device once, before the first launch; still one enqueue and one synchronise, every buffer grown
 * before the first launch. With sensor NULL the call is ilqr_mpc_run_io: no launch, buffer or argument differs. Refused
 * (ILQR_ERR_INVALID) before any launch: everything ilqr_mpc_run_io, ilqr_estimate_predict and the two calls above refuse;
 * io->sigma_y non-null together with a sensor (the sensor's own [ny] array replaces it); a sensor with P NULL; xhat0, P, xhat_cl,
 * pdiag_cl or nis_cl without a sensor. Works on a sharded handle. Not offered: a non-diagonal R, an H that varies with time inside
 * the loop, outlier gating. (A nonlinear h(x, s): ilqr_compile_sensor and ilqr_mpc_run_nlsensor below.) */
typedef struct {
    int32_t ny, reserved;
    const double* H;           /* HOST [ny][nx], shared by the batch */
    const double* r;           /* HOST [ny] */
    const double* q;           /* HOST, NULL or [nx] */
    const double* sigma_y;     /* HOST, NULL or [ny] */
} ilqr_sensor;
int ilqr_mpc_run_sensor(ilqr_handle* h, const ilqr_mpc_desc* d,
                        const ilqr_plant_io* io,   /* NULL: none */
                        const ilqr_sensor* sensor, /* NULL: ilqr_mpc_run_io */
                        const double* x0, const double* xhat0, double* P, const double* w_plant, const double* w_preview, double* x_cl,
                        double* u_cl, double* log, int32_t* first_nonfinite, double* cl_cost, double* cl_violation,       /* as ilqr_mpc_run_est's */
                        double* y_cl,              /* NULL, or [B][P][ny] */
                        int32_t* saturated, double* xhat_cl, double* pdiag_cl, double* nis_cl);

/* A NONLINEAR sensor y = h(x, s) + v, v ~ N(0, diag(r)), for the filter and the loop: a range, a bearing, a camera pixel, sin(q) of an
 * encoder. The sensor is a compiled module of its own, apart from the model (one model runs with several sensors): nx inputs,
 * 1 <= ny <= 64 outputs (ny may exceed nx), 0 <= ns <= 64 sensor parameters s — beacon positions, a focal length — shared by the batch,
 * [ns] (per_instance_s == 0), or one row per instance, [B][ns] (per_instance_s == 1).
 *
 * ilqr_compile_sensor: `source` is C code that defines ONE function, row-wise so that no thread ever holds ny · nx numbers,
 *     ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s);
 * which writes *y = h_j(x, s) and dydx[k] = dh_j/dx_k for k < nx; dydx is pre-zeroed by the caller, so only non-zero partials need be
 * written; math.h names and ilqr::sincos_fast are available as in model sources. The library wraps the source
 * (csrc/ilqr_sensor_adapter.hpp; floating-point contraction is off around it, so h_j is the same bits wherever it is evaluated),
 * compiles it for gfx950 with hipcc as a child process as ilqr_compile_model does — cached under a hash of source, name, dimensions,
 * the sensor ABI version and the library's kernel headers and flags, as lib/models/libilqr_sensor_<name>_c<tag>.so; temporary files
 * under process-unique names, the module moved into place atomically — loads it and returns the registered name
 * <name>_c<tag> and the module path. ilqr_load_sensor_library loads a module some process compiled earlier (no compiler needed).
 * Refused (ILQR_ERR_INVALID): a null argument; a name that is not a C identifier; nx outside 1 .. 64, ny outside 1 .. 64, ns outside
 * 0 .. 64; output buffers that are too small.
 *
 * ilqr_sensor_linearise: H_out[b][j][0 .. nx) = row j of dh/dx at x_lin[b], layout [B][ny][nx] row-major — what
 * ilqr_estimate_update_linear reads with per_instance_H == 1; yhat_out[b][j] = h_j(x_lin[b], s), or with x_prior given
 *     yhat_out[b][j] = h_j + SUM_k H_jk (x_prior[b][k] - x_lin[b][k]),
 * one FMA chain over ascending k = 0 .. nx-1 that starts from h_j, each difference rounded first: the reference output of an
 * iterated filter whose prior is x_prior.
 * ilqr_plant_measure_sensor: y[b][j] = h_j(x[b], s), then + sigma_y[j] · z(seed, first_instance + b, 5 + j / 16, step, j % 16) where
 * sigma_y[j] != 0, product and sum rounded separately; z, the key fields 5 .. 8 and the host twin ilqr_candidate_noise(seed,
 * first_instance, B, 9, step + 1, 16, z) are ilqr_plant_measure's, shared on purpose as the linear sensor shares them. With sigma_y
 * NULL y is bit for bit the yhat of ilqr_sensor_linearise at x.
 * ilqr_estimate_update_sensor, the measurement update of the extended Kalman filter with this sensor. iterations == 1: bit for
 * bit ilqr_sensor_linearise_device(x_lin = xhat, x_prior = NULL) into H and yhat buffers the handle owns and reuses, followed by
 * ilqr_estimate_update_linear_device(ny, per_instance_H = 1, H, r, y, yhat, ...): the existing update, untouched. iterations = N,
 * 2 <= N <= 8, the ITERATED filter: the prior (x0, P0) = (xhat, P) on entry is kept in buffers of the handle; iteration 0 is the
 * above; iteration i >= 1 linearises at the estimate iteration i-1 left with x_prior = x0, restores xhat <- x0 and P <- P0, and runs
 * the same update — whose c_j = yhat_j - h_j·x0 is then exactly the offset of the Gauss-Newton IEKF. The outputs are the last
 * iteration's.
 *
 * Refused (ILQR_ERR_INVALID) before any launch: a sensor name that is not registered; a sensor whose nx is not the handle's;
 * per_instance_s other than 0 or 1; a null s with ns > 0; a non-finite entry of an s given on the host; iterations outside 1 .. 8;
 * everything ilqr_estimate_update_linear and ilqr_plant_measure_linear refuse for the same arguments (a null array, an r entry that
 * is not finite and > 0, a negative or non-finite sigma_y entry, step and first_instance outside the noise key's fields). Host
 * forms: every array a host array; work on a sharded handle; synchronous. Device forms: s, x_lin, x_prior, H_out, yhat_out, x, y,
 * xhat, P, innovation, nis, first_bad device pointers; r and sigma_y stay host arrays of ny doubles that travel as
 * ilqr_estimate_update_linear_device's do and are read when the call is made; asynchronous on the handle's stream; refused on a
 * sharded handle. */
typedef struct {
    const char* name;        /* C identifier */
    int32_t nx, ny, ns;      /* inputs, outputs, sensor parameters */
    const char* source;
    int32_t flags;           /* 0 */
} ilqr_sensor_source;
int ilqr_compile_sensor(const ilqr_sensor_source* src, char* registered_name, size_t name_len, char* library_path, size_t path_len);
int ilqr_load_sensor_library(const char* path);
/* Sensor registry (compiled sensor modules call ilqr_register_sensor from a static initialiser; vtable: a
 * const struct ilqr_sensor_vtable*, csrc/ilqr_device_sensor_nl.hpp). */
int ilqr_register_sensor(const void* vtable);
int ilqr_sensor_count(void);
const char* ilqr_sensor_name(int32_t i);
int ilqr_sensor_dims(const char* sensor, int32_t* nx, int32_t* ny, int32_t* ns);
int ilqr_sensor_linearise(ilqr_handle* h, const char* sensor, int32_t per_instance_s,
                          const double* s,                 /* NULL (ns == 0), [ns] or [B][ns] */
                          const double* x_lin,             /* [B][nx] */
                          const double* x_prior,           /* NULL, or [B][nx] */
                          double* H_out,                   /* [B][ny][nx] */
                          double* yhat_out);               /* [B][ny] */
int ilqr_sensor_linearise_device(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* d_s, const double* d_x_lin,
                                 const double* d_x_prior, double* d_H_out, double* d_yhat_out);
int ilqr_plant_measure_sensor(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, uint64_t seed,
                              int64_t first_instance, int32_t step,
                              const double* sigma_y,       /* HOST, NULL or [ny], finite, >= 0 */
                              const double* x,             /* [B][nx] */
                              double* y);                  /* [B][ny] */
int ilqr_plant_measure_sensor_device(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* d_s, uint64_t seed,
                                     int64_t first_instance, int32_t step, const double* sigma_y, const double* d_x, double* d_y);
int ilqr_estimate_update_sensor(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, int32_t iterations,
                                const double* r,           /* HOST [ny], finite, > 0 */
                                const double* y,           /* [B][ny] */
                                double* xhat,              /* [B][nx] in / out */
                                double* P,                 /* [B][nx][nx] in / out */
                                double* innovation,        /* NULL, or [B][ny] */
                                double* nis,               /* NULL, or [B] */
                                int32_t* first_bad);       /* NULL, or [B] */
int ilqr_estimate_update_sensor_device(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* d_s, int32_t iterations,
                                       const double* r, const double* d_y, double* d_xhat, double* d_P, double* d_innovation, double* d_nis,
                                       int32_t* d_first_bad);

/* ilqr_mpc_run_sensor's loop with the nonlinear sensor: the measurement launch is ilqr_plant_measure_sensor_device(sensor, s,
 * sigma_y) at the same step index, and the update ilqr_estimate_update_sensor_device(sensor, s, iterations, r) with the period's
 * measurement. The order of the four calls per delay, the time update (with q), xc = xhat, y_cl [B][P][ny], xhat_cl, pdiag_cl and
 * nis_cl stay ilqr_mpc_run_est's. s (per instance where ns_per_instance == 1: [B][ns]), r and sigma_y are copied to the device once,
 * before the first launch; H, yhat and the prior's buffers too are grown before it; still one enqueue and one synchronise. With
 * sensor NULL the call is ilqr_mpc_run_io: no launch, buffer or argument differs. Refused (ILQR_ERR_INVALID) before any launch:
 * everything ilqr_mpc_run_sensor refuses for the same arguments (io->sigma_y together with a sensor among it) and everything
 * ilqr_estimate_update_sensor and ilqr_plant_measure_sensor refuse. Works on a sharded handle. Not offered: a sensor that reads the
 * model's parameters theta_t; an s that varies with time inside the loop; a non-diagonal R; outlier gating. */
typedef struct {
    const char* sensor;        /* registered name (ilqr_compile_sensor) */
    int32_t ns_per_instance;   /* 0: s [ns] shared by the batch; 1: s [B][ns] */
    const double* s;           /* HOST, NULL where ns == 0 */
    const double* r;           /* HOST [ny] */
    const double* q;           /* HOST, NULL or [nx] */
    const double* sigma_y;     /* HOST, NULL or [ny] */
    int32_t iterations;        /* 1 .. 8; 1: the extended Kalman filter, more: the iterated one */
} ilqr_nl_sensor;
int ilqr_mpc_run_nlsensor(ilqr_handle* h, const ilqr_mpc_desc* d,
                          const ilqr_plant_io* io,        /* NULL: none */
                          const ilqr_nl_sensor* sensor,   /* NULL: ilqr_mpc_run_io */
                          const double* x0, const double* xhat0, double* P, const double* w_plant, const double* w_preview, double* x_cl,
                          double* u_cl, double* log, int32_t* first_nonfinite, double* cl_cost, double* cl_violation,     /* as ilqr_mpc_run_est's */
                          double* y_cl,                   /* NULL, or [B][P][ny] */
                          int32_t* saturated, double* xhat_cl, double* pdiag_cl, double* nis_cl);

/* Stage-level entry points for parity tests (one kernel each, mode = :nominal):
 * the reference functions they run are listed per id. */
enum {
    ILQR_STAGE_COST_NOMINAL = 0,   /* cost!(data, problem, mode=:nominal) — src/data/methods.jl:13-30 */
    ILQR_STAGE_GRADIENTS = 1,      /* gradients!(problem)                 — src/gradients.jl:92-98   */
    ILQR_STAGE_BACKWARD_PASS = 2,  /* backward_pass! + lagrangian_gradient! — src/backward_pass.jl, src/solve.jl:67-83 */
    ILQR_STAGE_FORWARD_PASS = 3,   /* forward_pass!                       — src/forward_pass.jl:1-56 */
    ILQR_STAGE_RESET_MODEL_OBJECTIVE = 4, /* reset!(model); reset!(objective) — src/solve.jl:9-10 */
    ILQR_STAGE_ILQR_SOLVE = 5,     /* ilqr_solve!                         — src/solve.jl:1-54       */
    ILQR_STAGE_AL_UPDATE = 6,      /* augmented_lagrangian_update!        — src/augmented_lagrangian.jl:87-110 */
    /* host-stepped outer loop, for solve!(solver; augmented_lagrangian_callback!) — src/solve.jl:88,125:
     * AL_BEGIN once (:93-103), then AL_OUTER per outer iteration (:105-122, skipping instances that already
     * met the constraint tolerance); the caller runs its callback between AL_OUTER launches. */
    ILQR_STAGE_AL_BEGIN = 7,
    ILQR_STAGE_AL_OUTER = 8,
    /* SHARED STEP SIZE over a whole (multi-GPU) batch — not in the reference (every Solver there line-searches alone); the
     * optional mode of the north star: all instances take the SAME Armijo step, decided on the summed merit. The line search
     * of forward_pass! (src/forward_pass.jl:26-52) is stepped from the host, everything else stays per instance:
     *   SS_INNER_BEGIN            src/solve.jl:9-21 for every instance whose outer loop is still running
     *   SS_TRIAL(alpha, first)    rollout!(alpha) + cost!(mode = :current) (src/forward_pass.jl:34-36); with first != 0 also
     *                             J_prev and delta_grad_product (:13-20). The caller sums objective, "j_prev" and
     *                             "delta_grad_product" over the instances with "inner_done" == 0 (and over ranks: ONE all-reduce
     *                             of three doubles) and tests  sum J <= sum J_prev + 1e-4 alpha sum delta  (:44)
     *   SS_FINISH(alpha, accept)  update_nominal_trajectory! or line-search failure, then src/solve.jl:27-51 per instance
     *   SS_OUTER                  src/solve.jl:113-122 per instance
     * (ilqr_run_stage_param; the whole loop: ilqr_solve_shared_step below). With a batch of one it reproduces solve! exactly. */
    ILQR_STAGE_SS_INNER_BEGIN = 9,
    ILQR_STAGE_SS_TRIAL = 10,
    ILQR_STAGE_SS_FINISH = 11,
    ILQR_STAGE_SS_OUTER = 12
};
int ilqr_run_stage(ilqr_handle* h, int32_t stage);
int ilqr_run_stage_param(ilqr_handle* h, int32_t stage, double param, int32_t flag);

/* solve! with ONE step size per inner iteration for the whole batch — over every rank of a multi-GPU job when `reduce` sums across
 * them. Not a reference behaviour (every reference Solver line-searches alone; a shared step changes every iterate): the optional
 * mode of the north star, "at most an all-reduce of the line-search merit for a shared step size". The Armijo loop of
 * forward_pass! (src/forward_pass.jl:26-52) runs here, on the host, over the SUMMED merit of the instances still in their inner
 * loop: per trial one SS_TRIAL launch, one reduction of three doubles {sum J(alpha), sum J_prev, sum grad_L' dz}, then SS_FINISH;
 * linearisation, Riccati pass, convergence tests and dual updates stay per instance on the device (stages SS_* above).
 *   reduce(values, n, ctx): replace values[0..n) by their sum over all ranks, return 0 (an RCCL / MPI all-reduce in a host with
 *     several processes; NULL = one process: the identity). It is called the same number of times on every rank.
 *   steps / steps_cap / n_steps (optional): the accepted step size of every inner iteration (0 = line search failed), in order.
 *     *n_steps is the number of inner iterations the solve took; min(*n_steps, steps_cap) entries of steps are written (a caller
 *     that sized steps for fewer must not read beyond steps_cap).
 * With a batch of ONE instance the mode reproduces ilqr_solve exactly. Constrained solvers only. Synchronous. */
typedef int (*ilqr_allreduce_sum_fn)(double* values, int32_t n, void* ctx);
int ilqr_solve_shared_step(ilqr_handle* h, ilqr_allreduce_sum_fn reduce, void* ctx, double* steps, int32_t steps_cap, int32_t* n_steps);

/* get_trajectory(solver) — src/solver.jl:48-50: nominal states [B][T][nx] and
 * actions [B][T-1][nu]. */
int ilqr_get_trajectory(ilqr_handle* h, double* x, double* u);
/* solver.policy.K / .k — src/data/policy.jl:25-26. K: [B][T-1][nx][nu] (column-major nu×nx). */
int ilqr_get_policy(ilqr_handle* h, double* K, double* k);
/* solver.data.* — one record per instance. */
int ilqr_get_stats(ilqr_handle* h, ilqr_stats* stats);

/* Closed-loop rollouts of the handle's CURRENT policy (K_t, k_t) around its nominal trajectory (x̄, ū), from `samples` initial
 * states per instance — rollout!(policy, problem; step_size), src/rollout.jl:1-31, started anywhere instead of at x̄_1:
 *     x_1 = x1[b][s],   u_t = ū_t + K_t (x_t − x̄_t) + step_size k_t,   x_{t+1} = f(x_t, u_t, w_t)
 * in the reference's operation order (src/rollout.jl:24-28); step_size = 0 is pure tracking, x1 = x̄_1 with step_size > 0 is the
 * reference's rollout!. w_t: the handle's parameters, or the sample's own w[b][s][t] (the user's columns; a lowered problem's
 * selector columns stay the handle's). Per sample: cost = the plain objective Σ cost (src/costs.jl:48-55, not the
 * augmented-Lagrangian merit); max_violation = constraint_violation over the sample's trajectory (src/data/constraints.jl:23-39;
 * 0 on a handle created unconstrained); first_nonfinite = −1, or the first 0-based t at which a component of x[b][s][t] is not
 * finite (from there on that sample's outputs are unspecified; other samples are unaffected); optionally the trajectories.
 * The call READS the handle: workspace, scalars, statistics, trace, timing and resident inputs are unchanged, a later solve behaves
 * as if the call had not happened. Refused (ILQR_ERR_INVALID) without touching the GPU: samples < 1, null x1 or cost, w on a model
 * without parameters, a handle that holds no policy yet (no solve, no backward-pass stage, no host write of K / k since the
 * last reset). Host form: stages through device buffers the handle owns and reuses; on a sharded handle every instance's samples
 * go to the device that owns the instance. Device form: every pointer a device pointer on the handle's device, asynchronous on
 * the handle's stream; refused on a sharded handle. */
int ilqr_rollout_policy(ilqr_handle* h, int32_t samples, double step_size,
                        const double* x1,            /* [B][S][nx] */
                        const double* w,             /* NULL, or [B][S][T][nw] */
                        double* cost,                /* [B][S] */
                        double* max_violation,       /* NULL, or [B][S] */
                        int32_t* first_nonfinite,    /* NULL, or [B][S] */
                        double* x,                   /* NULL, or [B][S][T][nx] */
                        double* u);                  /* NULL, or [B][S][T-1][nu] */
int ilqr_rollout_policy_device(ilqr_handle* h, int32_t samples, double step_size, const double* d_x1, const double* d_w, double* d_cost,
                               double* d_max_violation, int32_t* d_first_nonfinite, double* d_x, double* d_u);

/* Raw workspace access by reference field name (parity tests):
 * "nominal_states","nominal_actions","states","actions","jacobian_state",
 * "jacobian_action","gradient_state","gradient_action","hessian_state_state",
 * "hessian_action_action","hessian_action_state","K","k","P","p",
 * "gradient_state_lagrangian"(Qx−p),"gradient_action_lagrangian"(Qu),
 * "violations","constraint_dual","constraint_penalty","active_set","parameters".
 * Layout: [B][per-instance length]; ilqr_buffer_len gives the per-instance length.
 * Large models (nx > 4 or nu > 4): the kernels work on compact rows (state-dependent Jacobian entries, structurally non-zero
 * Hessian entries); the full jacobian_* / hessian_* arrays are a mirror. A value written with ilqr_set_buffer at a constant
 * Jacobian position or outside the Hessian pattern cannot be represented there and is dropped: ilqr_get_buffer afterwards
 * returns what the kernels use (the constant, a zero), not what was written. */
int ilqr_buffer_len(const ilqr_handle* h, const char* name, size_t* len);
int ilqr_get_buffer(ilqr_handle* h, const char* name, double* out);
int ilqr_set_buffer(ilqr_handle* h, const char* name, const double* in);
/* solver.policy.action_value.* — src/data/policy.jl:58-64: "Qx","Qu","Qxx","Quu","Qux" (read-only through
 * ilqr_get_buffer). The fused solve keeps them in registers; after this call the backward-pass STAGE
 * (ILQR_STAGE_BACKWARD_PASS, ILQR_STAGE_ILQR_SOLVE) also stores them to HBM. */
int ilqr_enable_action_value_buffers(ilqr_handle* h);
/* Index of a named SolverData scalar inside the "_scalars" buffer: "objective","max_violation","step_size","status",
 * "iterations","gradient_norm","outer_iterations","potrf_info","rollouts","done" (host-stepped AL loop: instance met
 * the constraint tolerance), "delta_grad_product" (∇Lᵀ·Δz of the last forward_pass!, src/forward_pass.jl:20),
 * "trace_len" (rows the last solve wrote to the trace), "count" (length of "_scalars"); shared-step mode: "obj_prev",
 * "inner_done", "j_prev", "inner_it"; "resume" (hand-over bookkeeping, 0 after a solve);
 * "literal_backward_passes" (two-wave latency kernel, models with one action: backward passes of the last solve that met a
 * non-positive pivot and were repeated in LAPACK's literal arithmetic — 0 on healthy instances); "t_start", "t_end" (when the
 * instance's workgroup started / finished its solve in the latency or large-model kernel: ticks of the device's 100 MHz
 * real-time counter) and "hw_id_wave0" … "hw_id_wave3" (where its waves ran: HW_REG_HW_ID + 2^32 * XCC_ID) — what
 * tools/finish_times.py reads. -1 if unknown. */
int ilqr_scalar_slot(const char* name);

/* Kernel variant of ilqr_solve. Large models (nx > 4 or nu > 4): 0 = auto, 1 = four waves per instance (two instances per CU),
 * 4 = ONE wave per instance (six per CU: 25 KB of LDS each) for models whose matrices are single 16x16 tiles (nx, nu <= 16) — the same phase
 * functions with the four wave roles of a phase run in turn, bitwise the four-wave results; auto takes it once the batch exceeds
 * 8 x CUs (an instance alone is faster on four waves; residency wins beyond that). Small models (nx, nu <= 4): 0 = auto — the latency kernel
 * (two waves per instance, all iteration state in LDS) while the batch fits the chip at one instance per SIMD (batch <= 4 x CUs),
 * the packed kernel beyond that and for horizons whose LDS-resident set exceeds the 160 KiB of a CU; 1 = latency; 2 = throughput
 * (one wave per instance, Jacobians in HBM / L2; superseded by the packed kernel, kept for A/B runs); 3 = packed — FOUR
 * instances per wave on the four blocks of v_mfma_f64_4x4x4, workspace streamed from HBM / L2 through a 13 KB LDS chunk buffer
 * per wave, no horizon limit — with a SECOND wave per pack as linearisation server (chunk ch - 1 linearised into a second LDS buffer
 * while the Riccati steps of chunk ch run; bitwise the one-wave results) wherever the buffers fit the CU's LDS at the batch's
 * residency (up to 4 packs per CU, i.e. batch <= 16 x CUs); 5 = packed, one wave per pack always; 6 = packed, two waves where they
 * fit (= 3; kept distinct for A/B runs). All run the same arithmetic up to the association of a few sums. */
int ilqr_set_kernel_variant(ilqr_handle* h, int32_t variant);
/* The kernel ilqr_solve launches for this handle as it stands (never 0): 1 latency / four waves per instance, 2 throughput,
 * 4 one wave per instance (large models), 5 packed with one wave per pack, 6 packed with two. */
int ilqr_resolved_kernel_variant(ilqr_handle* h, int32_t* variant);
/* Straggler hand-over of the packed kernel (no counterpart in the reference, which is one trajectory per Solver): a batched
 * launch lasts as long as its slowest instance, and in the packed kernel a straggler keeps a whole wave at 120-240 us per
 * cycle (one line-search trial per cycle). Instances that leave the packed kernel do so with their state complete in the
 * workspace block — at the start of an outer iteration of constrained_ilqr_solve! (src/solve.jl:105) or at the head of an
 * inner iteration of ilqr_solve! (src/solve.jl:22), where the block holds the nominal trajectory, the linearisation, the
 * accumulated Hessians, K, k and the loop's scalars — and a second launch on the same stream finishes exactly those with the
 * latency kernel (two waves per instance, state in LDS: 50-75 us per iteration, a rejected trial one rollout instead of a
 * cycle). The two kernels do the same arithmetic (trajectories, policies and duals bitwise: tests/test_gpu_parity.py), so
 * which instances change kernels, and when, never shows in a result.
 *   ilqr_set_handover(outer): -1 (default) = by head count, below; 0 = no hand-over; k >= 2 = an instance still unconverged
 *     when it ENTERS outer iteration k leaves at that boundary.
 *   ilqr_set_handover_live(live), used when outer = -1: once no more than `live` instances of the batch are still running,
 *     every survivor leaves at its next resumable point. -1 auto = min(1024, batch / 4), what the latency kernel holds at full
 *     speed; 0 off; n >= 1 as given.
 * One wave per pack (the packed kernel's form above four packs per CU, two packs per workgroup): the workgroups finish the
 * handed-over instances THEMSELVES — once both its packs are through, a workgroup takes instances from a device-wide queue
 * and runs the latency kernel's code on each, so the second launch finds nothing left (it stays as the net) — and a straggler
 * does not wait for the head count: under that rule
 *   ilqr_set_handover_mark(rejected): an instance whose rejected line-search trials (src/forward_pass.jl:51; those of forward
 *     passes that ended in an acceptance) exceed the mean over the batch so far by `rejected`, while more than half the batch is
 *     still running, is marked at the head of its next
 *     inner iteration; its workgroup's two packs leave at their next resumable points and the workgroup finishes the marked
 *     instance at once (BASELINE config 4: instance 2300 of shard 2 — 682 iterations, 1354 rollouts, the others 347 — is
 *     marked in its second iteration). -1 auto = 6; 0 never; n >= 1 as given. Marks are taken only while the launch is ONE round of
 *     workgroups (all resident: up to 8192 instances per GPU on an MI355X); beyond that the head-count rule alone applies.
 * The two-wave solvers (latency kernel, resume launch, the workgroups above) take the trials of a line search
 * (src/forward_pass.jl:28-52) in rounds of up to four, rolled out at once by the four 16-lane rows of one wave; trial by trial the
 * search is the reference's, and so are its results. */
int ilqr_set_handover(ilqr_handle* h, int32_t outer);
int ilqr_set_handover_live(ilqr_handle* h, int32_t live);
int ilqr_set_handover_mark(ilqr_handle* h, int32_t rejected);
/* What the last ilqr_solve did there: instances that went through the queue, instances marked as stragglers. */
int ilqr_get_handover_stats(ilqr_handle* h, int32_t* queued, int32_t* marked);

/* Per-iteration record of what the reference prints when `verbose` (src/solve.jl:40-45): for every
 * instance up to `capacity` rows of 8 doubles {outer, inner, objective, gradient_norm, max_violation,
 * step_size, status, rollouts-so-far} written by ilqr_solve. capacity 0 disables (default). */
int ilqr_enable_trace(ilqr_handle* h, int32_t capacity);
int ilqr_get_trace(ilqr_handle* h, double* out /* [B][capacity][8] */);

/* Device-side handles for callers that time or chain work themselves. */
int ilqr_get_stream(ilqr_handle* h, void** hip_stream);
/* Average device time (ms) of the solve kernel over the ilqr_solve calls since
 * the last ilqr_timing_reset, measured with HIP events on the handle's stream. */
int ilqr_timing_reset(ilqr_handle* h);
int ilqr_timing_get(ilqr_handle* h, double* solve_kernel_ms_avg, int32_t* launches);

/* Dynamics(f, fx, fu, ...) / Cost(...) / Constraint(f, fx, fu, ...) with USER-SUPPLIED callables — src/dynamics.jl:55-60,
 * src/costs.jl:1-15, src/constraints.jl:54-64 — for hosts without Python (the Julia wrapper hands over what
 * Symbolics.build_function(..., target = CTarget()) emits; a C program writes it by hand). `source` is C code defining,
 * each as `ILQR_MODEL_FN void NAME(double* out, const double* x, const double* u, const double* w)` with the reference's
 * in-place contract (out column-major, pre-zeroed by the caller; u is a dummy for the terminal functions; math.h names
 * and ilqr::sincos_fast are available):
 *     dynamics, dynamics_jacobian_state, dynamics_jacobian_action,
 *     cost_stage, cost_stage_gradient_state, cost_stage_gradient_action, cost_stage_hessian_state_state,
 *     cost_stage_hessian_action_action, cost_stage_hessian_action_state,
 *     cost_terminal, cost_terminal_gradient_state, cost_terminal_hessian_state_state,
 *     constraint_stage, constraint_stage_jacobian_state, constraint_stage_jacobian_action          (only if nc_stage > 0)
 *     constraint_terminal, constraint_terminal_jacobian_state                                       (only if nc_term > 0)
 * ineq_stage / ineq_term: bit i set = constraint row i is an inequality (indices_inequality, 0-based).
 * The library wraps the source (csrc/ilqr_model_adapter.hpp), compiles it for gfx950 with hipcc as a child process (cached
 * by a hash of the source; ILQR_HIPCC / ILQR_CSRC_DIR override the tool and the kernel headers), loads the module and
 * returns the name to put into ilqr_problem_desc.model and the module path for ilqr_problem_desc.model_library.
 * nx <= 64, nu <= 16, at most 64 constraint rows per stage here (ilqr_compile_model_rows: 256). Models with nx > 4 or nu > 4 run on the large path, which streams only the state-dependent Jacobian
 * entries and the structurally non-zero Hessian entries per timestep: for opaque callables these are found by PROBING — the
 * source is compiled a second time with the host C++ compiler (ILQR_HOSTCXX, else g++ / c++ / clang++) and the Jacobian,
 * Hessian and constraint-Jacobian callables are evaluated at 48 points spread over magnitudes 1e-3 ... 1e3 and both signs
 * (x, u and w alike; selector parameters of a lowered model cycle through every kind); an entry bitwise equal and finite at
 * all of them is a constant (the role Symbolics' sparse expressions play in the reference, src/dynamics.jl:16-34); an entry
 * that is NaN / Inf anywhere counts as state-dependent / non-zero.
 * ASSUMPTION, and its limit: a derivative entry that is constant on every probed point is taken to be constant EVERYWHERE.
 * That holds for smooth expressions; a PIECEWISE callable — a clamp or saturation (derivative 1 inside a box, 0 outside), fabs,
 * max(0, .) penalties, contact switches, terms active only in a region — can look constant on all 48 points and is then baked
 * in wrongly for instances that leave the probed regime. Models with such callables must set flags = ILQR_MODEL_DENSE_TABLES
 * (per model; ILQR_NO_STRUCTURE_PROBE in the environment does the same for the whole process). Source that does not compile
 * for the host also gets the dense tables (correct at every size, but slow: all nx (nx + nu) Jacobian entries are evaluated,
 * stored and patched per timestep). ilqr_model_compact_sizes reports what a module was built with.
 * The dynamics callable itself stays opaque: every lane of the rollout evaluates the whole vector function. */
#define ILQR_MODEL_DENSE_TABLES 1   /* flags: no structure probe for THIS model (every Jacobian entry state-dependent, every Hessian entry non-zero) */
typedef struct {
    const char* name;        /* C identifier */
    int32_t nx, nu, nw;      /* num_state, num_action, num_parameter */
    int32_t nc_stage, nc_term;
    uint64_t ineq_stage, ineq_term;
    const char* source;
    int32_t flags;           /* 0 or ILQR_MODEL_DENSE_TABLES */
} ilqr_model_source;
int ilqr_compile_model(const ilqr_model_source* src, char* registered_name, size_t name_len, char* library_path, size_t path_len);
/* The same for constraints with more than 64 rows per stage (the reference has no limit: Constraint(f, fx, fu, nc, ...;
 * indices_inequality), src/constraints.jl:54-64): the inequality rows as arrays of 64-bit words, row i = bit i % 64 of word i / 64,
 * ceil(nc_stage / 64) and ceil(nc_term / 64) words (NULL = the struct's mask, for a kind with at most 64 rows). Up to
 * ILQR_MAX_CONSTRAINT_ROWS rows per stage; beyond 64 the per-timestep constraint values no longer fit a thread's registers
 * (correct, slower). */
#define ILQR_MAX_CONSTRAINT_ROWS 256
int ilqr_compile_model_rows(const ilqr_model_source* src, const uint64_t* ineq_stage_words, const uint64_t* ineq_term_words,
                            char* registered_name, size_t name_len, char* library_path, size_t path_len);

/* ---- Vectors of DISTINCT per-step objects and time-varying DIMENSIONS — README.md:26 of the reference ("costs, constraints and
 * dynamics can differ at every timestep"): Solver(dynamics::Vector{Dynamics}, costs::Vector{Cost}, constraints) keeps one object
 * per timestep (src/solver.jl:28-46) and sizes every buffer per timestep (num_next_state may differ from num_state,
 * src/dynamics.jl:5-7, src/data/model.jl:11-16, src/data/policy.jl:44-78). The device kernels are compiled for ONE stage template
 * (one Dynamics / stage Cost / stage Constraint of fixed dimensions, one terminal Cost / Constraint), so the host side LOWERS the
 * per-step objects onto it, exactly:
 *   - the distinct objects of a category ("kinds", in order of first appearance) become one combined callable that takes one
 *     extra per-timestep parameter per kind, a one-hot SELECTOR s_k(t) in {0, 1} riding in theta_t behind the user's own
 *     parameters; the combined callable runs the kind whose selector is set (a branch, not a product: a kind that is switched
 *     off may be outside its domain at that step); a category with a single kind gets no selectors;
 *   - constraint kinds are stacked: kind k owns rows [constraint_row0[k], + nc_k) of the combined stage constraint, the rows of
 *     the kinds that are off read c = 0 with zero Jacobian — their multipliers stay 0 and they add nothing to the AL cost, its
 *     gradient, the Gauss-Newton Hessian or max_violation (src/augmented_lagrangian.jl:39-110, src/gradients.jl:23-81,
 *     src/data/constraints.jl:23-46);
 *   - dimensions are zero-padded to the largest num_state / num_action of the horizon: padded next-state rows are 0, padded
 *     actions get the stage cost u^2 / 2 (Quu stays positive definite and block-diagonal with the real block, so its Cholesky
 *     and solves leave the real block untouched and return K = 0, k = 0 for the padding), padded states enter no function.
 *     Host arrays (x1, u, trajectories, gains) are the padded ones; state_dims[t] / action_dims[t] entries of step t are real.
 * ilqr_plan_stages computes the plan from the kinds alone (no device, no compiler): template dimensions, selector columns, the
 * selector table, row offsets and inequality masks. ilqr_compile_model_stages composes the combined callables from C source
 * of the kinds' callables and compiles them like ilqr_compile_model. ilqr_set_stage_selectors hands the table to a handle.
 * (The Python host traces symbolic objects: its lowering.py asks ilqr_plan_stages for the plan and gates the expressions
 * accordingly; a Julia or C host goes through ilqr_compile_model_stages.) */
#define ILQR_MAX_STAGE_KINDS 16
typedef struct {
    int32_t horizon;                    /* T: T-1 dynamics, T costs, T constraints (src/data/problem.jl:28-30) */
    int32_t num_parameter;              /* the user's parameters per timestep (largest num_parameter of all objects) */
    /* Dynamics kinds — src/dynamics.jl:1-12: kind k maps (dynamics_nx[k], dynamics_nu[k]) -> dynamics_nx_next[k] */
    int32_t n_dynamics;
    const int32_t* dynamics_nx; const int32_t* dynamics_nu; const int32_t* dynamics_nx_next;
    const int32_t* dynamics_of_step;    /* [T-1]: kind acting at step t */
    /* stage Cost kinds — src/costs.jl:1-15 */
    int32_t n_costs;
    const int32_t* cost_nx; const int32_t* cost_nu;
    const int32_t* cost_of_step;        /* [T-1] */
    /* stage Constraint kinds — src/constraints.jl:1-13; a step without rows names a kind with constraint_nc = 0
     * (Constraint(), src/constraints.jl:45-52). n_constraints = 0: no stage constraints at all (constraint_of_step unused). */
    int32_t n_constraints;
    const int32_t* constraint_nc; const int32_t* constraint_nx; const int32_t* constraint_nu;
    const uint64_t* constraint_ineq;    /* [n_constraints][4]: four 64-bit words per kind, row i of the kind an inequality = bit i % 64 of its word i / 64 */
    const int32_t* constraint_of_step;  /* [T-1] */
    /* terminal Cost / Constraint: num_state = nx_term (must be the last dynamics' num_next_state) */
    int32_t nx_term, nc_term;
    uint64_t ineq_term[4];              /* inequality rows of the terminal constraint, as words */
} ilqr_stage_kinds;
typedef struct {
    int32_t nx, nu;                     /* template dimensions: largest num_state / num_action of the horizon */
    int32_t nw;                         /* template parameters per timestep = num_parameter + n_selectors */
    int32_t nc_stage, nc_term;          /* rows of the combined stage constraint (all kinds stacked), terminal rows */
    int32_t n_selectors;
    int32_t sel_dynamics, sel_cost, sel_constraint;   /* first parameter column of the category's one-hot block; -1: one kind, no selectors */
    int32_t constraint_row0[ILQR_MAX_STAGE_KINDS];    /* first row of kind k in the combined stage constraint */
    uint64_t ineq_stage_words[4];       /* inequality rows of the combined stage constraint (row i = bit i % 64 of word i / 64) */
} ilqr_stage_plan;
/* selectors: [T][plan->n_selectors] written densely (row T-1, the terminal step, is all zero); selectors_len = doubles available
 * (T * (n_dynamics + n_costs + n_constraints) always suffices). state_dims: [T], action_dims: [T-1]. Any output pointer but
 * `plan` may be NULL. Fails with ILQR_ERR_INVALID when the chain of dimensions is inconsistent (dynamics[t].num_next_state !=
 * dynamics[t+1].num_state, a cost or constraint whose dimensions are not its step's), as the reference would throw at
 * x[t+1] .= dynamics!(...) (src/rollout.jl:29). */
int ilqr_plan_stages(const ilqr_stage_kinds* kinds, ilqr_stage_plan* plan, double* selectors, size_t selectors_len,
                     int32_t* state_dims, int32_t* action_dims);
/* `source`: C code defining, with the contract of ilqr_compile_model (ILQR_MODEL_FN void NAME(double* out, const double* x,
 * const double* u, const double* w), out column-major IN THE KIND'S OWN DIMENSIONS and pre-zeroed; w = the user's parameters),
 *     for every Dynamics kind k:    dynamics_<k>, dynamics_<k>_jacobian_state, dynamics_<k>_jacobian_action
 *     for every stage Cost kind k:  cost_stage_<k>, cost_stage_<k>_gradient_state, cost_stage_<k>_gradient_action,
 *                                   cost_stage_<k>_hessian_state_state, cost_stage_<k>_hessian_action_action, cost_stage_<k>_hessian_action_state
 *     for every Constraint kind k with rows: constraint_stage_<k>, constraint_stage_<k>_jacobian_state, constraint_stage_<k>_jacobian_action
 *     cost_terminal, cost_terminal_gradient_state, cost_terminal_hessian_state_state,
 *     constraint_terminal, constraint_terminal_jacobian_state                                         (only if nc_term > 0)
 * The library writes the combined, padded callables of the template around them (selector branches, re-striding of the
 * matrices into the template's leading dimensions, u^2 / 2 on padded actions) and compiles the result as ilqr_compile_model
 * does. Outputs as ilqr_plan_stages plus the registered name and module path for ilqr_problem_desc. After ilqr_create:
 * ilqr_set_stage_selectors(h, selectors, plan.n_selectors). */
int ilqr_compile_model_stages(const char* name, const ilqr_stage_kinds* kinds, const char* source, ilqr_stage_plan* plan,
                              double* selectors, size_t selectors_len, int32_t* state_dims, int32_t* action_dims,
                              char* registered_name, size_t name_len, char* library_path, size_t path_len);
/* The selector table of a lowered problem, [T][n_selectors] (n_selectors <= num_parameter of the model): the handle keeps it and
 * writes it into the last n_selectors parameter columns of every instance, now and on every ilqr_set_parameters — which from
 * here on takes the USER's parameters only, w: [B][T][nw - n_selectors], as ilqr_get_dims reports them. n_selectors = 0 detaches.
 * The user's columns (the first nw - n_selectors of every timestep) keep what an earlier ilqr_set_parameters put there. */
int ilqr_set_stage_selectors(ilqr_handle* h, const double* selectors, int32_t n_selectors);

/* Synthetic inputs of the benchmark workloads, generated on the host by ONE function that every host language
 * can call, so that a Julia or C program solves the same instances as the Python bench: value (b, t, j) is a pure function of
 * (seed, b, t, j) — key = seed ^ (b * 2^20 + t * 2^4 + j), splitmix64(key) -> U(0,1), a second splitmix64 round for the Box-Muller
 * partner, z = sqrt(-2 ln u1) cos(2 pi u2) — so shards [first, first + B) of a larger batch are slices of it.
 *   model: "particle" (u = 0.1 z, examples/particle.jl:30), "acrobot" (u = z, test/acrobot.jl:86-88), "car" / "car_goal" / "car_obs"
 *   (instance 0: test/car.jl:24-29 exactly; b >= 1: u scaled by 1 + 0.5 U(-1,1)_b, (x, y) of x1 jittered by 0.05 z), "synth32"
 *   (x1 = 0.5 z, u = 0), "synth12" (x1 = 0.5 z, u = 0.1 z). x1: [B][nx], ubar: [B][T-1][nu] of that model. No device needed.
 * (bench.py measures on this function's output since round 6 — `--generator pcg64` brings back the numpy PCG64 streams the figures of
 * rounds 1-5 were measured on; workloads.make_inputs(generator = "splitmix64") calls it; bench/julia_ref.jl reads its output
 * through tools/dump_inputs.py or `ccall`s it.) */
int ilqr_synthetic_inputs(const char* model, int32_t horizon, uint64_t seed, int64_t first_instance, int32_t batch, double* x1, double* ubar);

/* Test hook: evaluates one of the device-side scalar routines of csrc/ilqr_math.hpp on cuda device 0 — "recip_fast",
 * "rsqrt_fast", "sqrt_fast" (the d of sqrt_rsqrt_fast), "sin_fast", "cos_fast" — elementwise, y[i] = f(x[i]). These replace
 * IEEE division / sqrt and libm on the serial chains (src/rollout.jl:27-29, src/backward_pass.jl:68-75); the tests pin their
 * values at 0, subnormal, huge and non-finite arguments against the IEEE results. Host pointers. */
int ilqr_device_math(const char* fn, const double* x, double* y, int32_t n);

/* Model registry (generated model modules call this from a static initialiser). */
struct ilqr_model_vtable;
int ilqr_register_model(const struct ilqr_model_vtable* vt);
/* The kernels a model module registers beside its vtable, under the same name and after it (ext: a const ilqr_model_ext*,
 * csrc/ilqr_device.hpp); a table built against other headers, or for a model that is not registered, is refused. */
int ilqr_register_model_ext(const void* ext);
int ilqr_model_count(void);
const char* ilqr_model_name(int32_t i);
/* Large models (nx > 4 or nu > 4): how many Jacobian entries per timestep the kernels treat as state-dependent and how many
 * Hessian entries as structurally non-zero (the rest are constants / zeros: generated tables for symbolic models, found by
 * probing the callables on the host for ilqr_compile_model); 0, 0 for small models. */
int ilqr_model_compact_sizes(const char* model, int32_t* jac_nvar, int32_t* hess_nnz);

#ifdef __cplusplus
}
#endif
#endif
