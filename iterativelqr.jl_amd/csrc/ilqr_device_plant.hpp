// The plant of a closed MPC loop on the device (ilqr_plant_step, ilqr_mpc_run, include/ilqr_hip.h): the head of the handle's plan
// applied to the model's own dynamics from a plant state that lives in HBM. With k = steps, g = step0 + i the global plant step and
// x̄, ū, K, θ as the workspace holds them, for i = 0 .. k−1
//
//   u_i = ū_i                       (feedback == 0)
//   u_i = ū_i + K_i (x − x̄_i)       (feedback != 0; src/rollout.jl:24-28 with α = 0, formed as (ū + K x) − K x̄: plant_feedback_row,
//                                    the arithmetic of shift_feedback_kernel / shift_feedback_large_kernel at s = i)
//   w_i = the user's columns of w_plant[b][i] if given, else of θ_i; the selector columns of a lowered problem are θ_i's
//   x ← f(x, u_i, w_i),  then  x_j ← x_j + sigma_x[j] · z(seed, b0 + b, 1 + j / 16, g, j % 16)   for every j with sigma_x[j] != 0
//
// (product and sum rounded separately). z is sample_z (ilqr_device_sample.hpp), unchanged: the key's candidate field carries the
// state component's high bits offset by one, its step field the global plant step, so ilqr_candidate_noise(seed, b0, B,
// 1 + ceil(nx / 16), step0 + k, 16, z) is the host twin — its row 0 is zero by contract, and the offset keeps every drawn
// component out of it. The fields stay disjoint for nx <= 64 (candidate <= 4), g < 2^20, b0 + b < 2^23: the entry points refuse
// anything beyond.
//
// The kernels READ the workspace and write only the caller's plant arrays: x (in place, every lane or wave its own instance's row:
// read once at the start, written once at the end), x_out, u_out, first_nonfinite. No atomics, no cross-instance traffic.
//
// plant_step_kernel (nx, nu <= 4): ONE INSTANCE PER LANE as shift_feedback_kernel and init_rollout_kernel, the state in registers,
// generated M::dyn: an instance's bits depend neither on B nor on its neighbours.
// plant_step_large_kernel: ONE WAVE PER INSTANCE as shift_feedback_large_kernel / policy_rollout_large_kernel (DynAff / dyn_row, row
// i of K_i on lane i, x, u and w_i through LDS). Lane j < nx owns state row j and draws that row's noise: rows beyond lane 15 have
// their own key (candidate field 1 + j / 16).
//
// The actuator's limits (clamp != 0; ilqr_plant_step_limited, ilqr_mpc_run_io): after the action row is formed, feedback included, and
// before it is stored to u_out and handed to the dynamics,  u ← u < u_lo[r] ? u_lo[r] : (u > u_hi[r] ? u_hi[r] : u)  — plain
// comparisons, so a NaN action stays NaN (the non-finite mark catches it) and a limit of ∓Inf leaves every finite action bit for bit.
// u_out records the action APPLIED; saturated[b] counts the (step, component) pairs with u < u_lo[r] or u > u_hi[r]. The limits
// travel by value as sigma does (nu <= 16). With clamp == 0 the branch is uniform and nothing of the step changes.
//
// plant_measure_kernel: what the controller is given of a plant state, one lane per (instance, component):
//   y[b][j] = x[b][j]                                                             (sigma_y null, or sigma_y[j] == 0)
//   y[b][j] = x[b][j] + sigma_y[j] · z(seed, b0 + b, 5 + j / 16, step, j % 16)    (product and sum rounded separately)
// with `step` the number of plant steps taken when the measurement is made. The process noise uses candidate fields 1 .. 4, the
// measurement 5 .. 8: the two streams are disjoint, and ilqr_candidate_noise(seed, b0, B, 9, step + 1, 16, z) is the host twin.
//
// mpc_log_kernel: one thread per (instance, column) copies the nine scalars of ilqr_stats out of the scalar block into row p of
// the log. Plain vector stores.
#pragma once

#include <stdint.h>

namespace ilqr {

enum { PLANT_MAX_NX = 64, PLANT_MAX_NU = 16, PLANT_MAX_STEPS = 1 << 20, PLANT_MAX_INSTANCES = 1 << 23, MPC_LOG_W = 9, MPC_LOG_THREADS = 256,
       PLANT_MEASURE_FIELD0 = 5, PLANT_MEASURE_THREADS = 256 };

struct PlantArgs {
    const double* ws;        // the handle's workspace (read-only here)
    Layout L;
    int B;
    int steps;               // k, 1 .. T-1
    int feedback;
    int n_sel;               // trailing parameter columns that stay the handle's (stage selectors) when w is given
    int step0;               // global index of plant step 0 of this call
    int noise;               // sigma holds a vector (some entry may still be 0)
    int nf_global;           // 0: first_nonfinite is written, -1 or the local step i; 1 (the loop): it is kept when >= 0, else -1 or
                             // step0 + i, and saturated is added to
    uint64_t seed;
    long long b0;            // global index of the handle's instance 0
    double sigma[PLANT_MAX_NX];   // sigma_x by value: the first nx entries
    const double* w;         // null, or rows of nw - n_sel doubles: row (b · w_ld + w_row0 + i)
    double* x;               // [B][nx] in / out
    double* x_out;           // null, or rows of nx doubles: row (b · x_ld + x_row0 + i), i = 0 .. k (row 0 = the input state)
    double* u_out;           // null, or rows of nu doubles: row (b · u_ld + u_row0 + i), i = 0 .. k-1
    int* nonfinite;          // null, or [B]
    long long w_ld, w_row0, x_ld, x_row0, u_ld, u_row0;
    // mpc_log_kernel
    double* log;             // [B][log_ld][MPC_LOG_W]
    int log_ld, log_row;
    // the actuator's limits
    int clamp;               // u_lo, u_hi hold the limits (an entry may still be ∓Inf)
    int* saturated;          // null, or [B]: the (step, component) pairs the clamp changed
    double u_lo[PLANT_MAX_NU], u_hi[PLANT_MAX_NU];       // by value: the first nu entries
};
static_assert(sizeof(PlantArgs) <= 4096, "the kernel argument segment");

struct MeasureArgs {
    int B;
    int noise;               // sigma holds a vector (some entry may still be 0)
    int step;                // plant steps taken when the measurement is made
    uint64_t seed;
    long long b0;            // global index of the handle's instance 0
    double sigma[PLANT_MAX_NX];   // sigma_y by value: the first nx entries
    const double* x;         // [B][nx]
    double* y;               // [B][nx]
};

// row i of ū_s + K_s (x − x̄_s) with x read through xv(j): kx and kb are the two FMA chains over j = 0 .. n−1, then (ū + kx) − kb
template <class M, class XV>
__device__ __forceinline__ double plant_feedback_row(const double* g, const Layout& L, int s, int i, XV xv) {
    constexpr int n = M::NX, m = M::NU, KN = m * n;
    const double* Ks = g + L.K + s * KN;
    double kx = 0.0, kb = 0.0;
#pragma unroll
    for (int j = 0; j < n; ++j) { kx = fma(Ks[j * m + i], xv(j), kx); kb = fma(Ks[j * m + i], g[L.xb + s * n + j], kb); }
    return (g[L.ub + s * m + i] + kx) - kb;                                                        // (:24-28), α = 0
}

__device__ __forceinline__ double plant_noise(const PlantArgs& a, double x, double sigma, int b, int i, int j) {
    return __dadd_rn(x, __dmul_rn(sigma, sample_z(a.seed, a.b0 + b, 1 + j / 16, a.step0 + i, j % 16)));
}

// the limits at work on one action: plain comparisons (a NaN passes through)
__device__ __forceinline__ double plant_clamp(double u, double lo, double hi, bool& changed) {
    changed = u < lo || u > hi;
    return u < lo ? lo : (u > hi ? hi : u);
}
__device__ __forceinline__ int plant_sat_in(const PlantArgs& a, int b) { return (a.saturated && a.nf_global) ? a.saturated[b] : 0; }

// what first_nonfinite gets: the first step with a non-finite state, local or global, or what an earlier call of the loop left
__device__ __forceinline__ int plant_nf_in(const PlantArgs& a, int b) { return (a.nonfinite && a.nf_global) ? a.nonfinite[b] : -1; }
__device__ __forceinline__ int plant_nf_mark(const PlantArgs& a, int nf, bool fin, int i) {
    return (nf < 0 && !fin) ? (a.nf_global ? a.step0 + i : i) : nf;
}

template <class M>
__global__ __launch_bounds__(64) void plant_step_kernel(PlantArgs a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const int k = a.steps, nwu = NW - a.n_sel;
    const double* wp = a.w ? a.w + ((size_t)b * (size_t)a.w_ld + (size_t)a.w_row0) * (size_t)(nwu > 0 ? nwu : 0) : nullptr;
    double* xo = a.x_out ? a.x_out + ((size_t)b * (size_t)a.x_ld + (size_t)a.x_row0) * n : nullptr;
    double* uo = a.u_out ? a.u_out + ((size_t)b * (size_t)a.u_ld + (size_t)a.u_row0) * m : nullptr;
    double xt[n];
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = a.x[(size_t)b * n + i];
    if (xo) {
#pragma unroll
        for (int i = 0; i < n; ++i) xo[i] = xt[i];
    }
    int nf = plant_nf_in(a, b), sat = plant_sat_in(a, b);
    for (int i = 0; i < k; ++i) {
        double ut[m], y[n];
#pragma unroll
        for (int r = 0; r < m; ++r)
            ut[r] = a.feedback ? plant_feedback_row<M>(g, L, i, r, [&](int j) { return xt[j]; }) : g[L.ub + i * m + r];
        if constexpr (m <= PLANT_MAX_NU) {
            if (a.clamp) {                                                                     // (the same branch on every lane)
#pragma unroll
                for (int r = 0; r < m; ++r) {
                    bool changed;
                    ut[r] = plant_clamp(ut[r], a.u_lo[r], a.u_hi[r], changed);
                    sat += changed ? 1 : 0;
                }
            }
        }
        if (uo) {
#pragma unroll
            for (int r = 0; r < m; ++r) uo[(size_t)i * m + r] = ut[r];
        }
        double w[cdim<NW>::v];
        load_w<NW>(g + L.w, i, w);
        if constexpr (NW > 0) {
            if (wp) {
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (j < nwu) w[j] = wp[(size_t)i * nwu + j];
            }
        }
        M::dyn(xt, ut, w, y);                                                                  // (:29)
        bool fin = true;
#pragma unroll
        for (int j = 0; j < n; ++j) {
            if (a.noise && a.sigma[j] != 0.0) y[j] = plant_noise(a, y[j], a.sigma[j], b, i, j);      // (the same branch on every lane)
            xt[j] = y[j];
            fin = fin && (fabs(y[j]) < __builtin_huge_val());                                  // false for ±Inf and NaN
        }
        nf = plant_nf_mark(a, nf, fin, i);
        if (xo) {
#pragma unroll
            for (int j = 0; j < n; ++j) xo[(size_t)(i + 1) * n + j] = xt[j];
        }
    }
#pragma unroll
    for (int i = 0; i < n; ++i) a.x[(size_t)b * n + i] = xt[i];
    if (a.nonfinite) a.nonfinite[b] = nf;
    if (a.saturated) a.saturated[b] = sat;
}

template <class M>
__global__ __launch_bounds__(64) void plant_step_large_kernel(PlantArgs a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW;
    static_assert(n <= PLANT_MAX_NX, "sigma_x travels by value");
    __shared__ double sx[n], su[m], sw[cdim<NW>::v];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const int k = a.steps, nwu = NW - a.n_sel;
    const double* wp = a.w ? a.w + ((size_t)b * (size_t)a.w_ld + (size_t)a.w_row0) * (size_t)(nwu > 0 ? nwu : 0) : nullptr;
    double* xo = a.x_out ? a.x_out + ((size_t)b * (size_t)a.x_ld + (size_t)a.x_row0) * n : nullptr;
    double* uo = a.u_out ? a.u_out + ((size_t)b * (size_t)a.u_ld + (size_t)a.u_row0) * m : nullptr;
    DynAff<M> aff;
    aff.init(lane);
    const int xrow = DynAff<M>::SPLIT ? (lane & 31) : lane;
    double xl = xrow < n ? a.x[(size_t)b * n + xrow] : 0.0;
    double sg = 0.0;                                                          // sigma_x of the row this lane owns (lane < nx)
    if (a.noise) {
#pragma unroll
        for (int j = 0; j < n; ++j) sg = (lane == j) ? a.sigma[j] : sg;
    }
    double ulo = 0.0, uhi = 0.0;                                              // the limits of the action row this lane owns (lane < nu)
    if constexpr (m <= PLANT_MAX_NU) {
        if (a.clamp) {
#pragma unroll
            for (int j = 0; j < m; ++j) { ulo = (lane == j) ? a.u_lo[j] : ulo; uhi = (lane == j) ? a.u_hi[j] : uhi; }
        }
    }
    int nf = plant_nf_in(a, b), sat = plant_sat_in(a, b);
    if (lane == 0) sw[0] = 0.0;
    for (int i = 0; i < k; ++i) {
        if (lane < n) { sx[lane] = xl; if (xo) xo[(size_t)i * n + lane] = xl; }
        for (int j = lane; j < NW; j += 64) sw[j] = (wp && j < nwu) ? wp[(size_t)i * nwu + j] : g[L.w + i * NW + j];
        wave_lds_fence();
        policy_wave_sync();
        bool changed = false;
        if (lane < m) {                                                       // row `lane` of K_i
            double v = a.feedback ? plant_feedback_row<M>(g, L, i, lane, [&](int j) { return sx[j]; }) : g[L.ub + i * m + lane];
            if (a.clamp) v = plant_clamp(v, ulo, uhi, changed);
            su[lane] = v;
            if (uo) uo[(size_t)i * m + lane] = v;
        }
        if (a.clamp) sat += __popcll(__ballot(changed));                      // (uniform: every lane of the wave votes)
        wave_lds_fence();
        policy_wave_sync();
        double ua[m];
#pragma unroll
        for (int j = 0; j < m; ++j) ua[j] = su[j];
        xl = dyn_row<M>(aff, sx, ua, xl, lane, sw, 0);                        // (:29)
        if (sg != 0.0) xl = plant_noise(a, xl, sg, b, i, lane);               // (lanes that own no row have sg == 0)
        const bool bad = lane < n && !(fabs(xl) < __builtin_huge_val());
        nf = plant_nf_mark(a, nf, __ballot(bad) == 0ull, i);
        wave_lds_fence();
        policy_wave_sync();                                                   // sx, su, sw are rewritten by the next step
    }
    if (lane < n) { a.x[(size_t)b * n + lane] = xl; if (xo) xo[(size_t)k * n + lane] = xl; }
    if (lane == 0 && a.nonfinite) a.nonfinite[b] = nf;
    if (lane == 0 && a.saturated) a.saturated[b] = sat;
}

// One lane per (instance, component). sigma_y comes out of the argument segment through a chain of selects over the model's nx, as
// the large plant kernel picks its row's sigma_x: no indexed access, no scratch.
template <class M>
__global__ __launch_bounds__(PLANT_MEASURE_THREADS) void plant_measure_kernel(MeasureArgs a) {
    constexpr int n = M::NX;
    static_assert(n <= PLANT_MAX_NX, "sigma_y travels by value");
    const size_t e = (size_t)blockIdx.x * PLANT_MEASURE_THREADS + threadIdx.x;
    if (e >= (size_t)a.B * n) return;
    const int b = (int)(e / n), j = (int)(e % n);
    double v = a.x[e];
    if (a.noise) {
        double sg = 0.0;
#pragma unroll
        for (int c = 0; c < n; ++c) sg = (j == c) ? a.sigma[c] : sg;
        if (sg != 0.0) v = __dadd_rn(v, __dmul_rn(sg, sample_z(a.seed, a.b0 + b, PLANT_MEASURE_FIELD0 + j / 16, a.step, j % 16)));
    }
    a.y[e] = v;
}

// Templated on the model only so that every module carries its own copy (the kernel reads nothing of M: the Layout has it all).
template <class M>
__global__ __launch_bounds__(MPC_LOG_THREADS) void mpc_log_kernel(PlantArgs a) {
    const int e = blockIdx.x * MPC_LOG_THREADS + threadIdx.x;
    if (e >= a.B * MPC_LOG_W) return;
    const int b = e / MPC_LOG_W, c = e % MPC_LOG_W;
    // ilqr_stats order
    const int slot = c == 0 ? S_OBJECTIVE : c == 1 ? S_GRADIENT_NORM : c == 2 ? S_MAX_VIOLATION : c == 3 ? S_STEP_SIZE : c == 4 ? S_ITERATIONS
                   : c == 5 ? S_OUTER_ITERATIONS : c == 6 ? S_STATUS : c == 7 ? S_POTRF_INFO : S_ROLLOUTS;
    a.log[((size_t)b * (size_t)a.log_ld + (size_t)a.log_row) * MPC_LOG_W + c] = a.ws[(size_t)b * (size_t)a.L.stride + a.L.scal + slot];
}

template <class M>
int launch_plant(const PlantArgs* a, void* stream) {
    if (a->B < 1 || a->steps < 1 || a->steps > a->L.T - 1 || !a->x || M::NX > PLANT_MAX_NX || (a->clamp && M::NU > PLANT_MAX_NU)) return -1;
    if constexpr (is_large<M>::value)
        hipLaunchKernelGGL(plant_step_large_kernel<M>, dim3((unsigned)a->B), dim3(64), 0, (hipStream_t)stream, *a);
    else
        hipLaunchKernelGGL(plant_step_kernel<M>, dim3((unsigned)((a->B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class M>
int launch_plant_measure(const MeasureArgs* a, void* stream) {
    if (a->B < 1 || !a->x || !a->y || a->step < 0 || a->step >= PLANT_MAX_STEPS || M::NX > PLANT_MAX_NX) return -1;
    const size_t grid = ((size_t)a->B * M::NX + PLANT_MEASURE_THREADS - 1) / PLANT_MEASURE_THREADS;
    hipLaunchKernelGGL(plant_measure_kernel<M>, dim3((unsigned)grid), dim3(PLANT_MEASURE_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class M>
int launch_mpc_log(const PlantArgs* a, void* stream) {
    if (a->B < 1 || !a->log || a->log_row < 0 || a->log_row >= a->log_ld) return -1;
    const size_t grid = ((size_t)a->B * MPC_LOG_W + MPC_LOG_THREADS - 1) / MPC_LOG_THREADS;
    hipLaunchKernelGGL(mpc_log_kernel<M>, dim3((unsigned)grid), dim3(MPC_LOG_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
