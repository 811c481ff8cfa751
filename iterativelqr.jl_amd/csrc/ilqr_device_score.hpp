// The score of a closed MPC loop on the device (ilqr_plant_score, ilqr_mpc_run_preview, include/ilqr_hip.h): the realised stage cost
// and constraint violation of plant steps, from the states the plant visited and the actions it applied. With k = steps, for
// instance b and step i = 0 .. k−1
//
//   x_i = row i of the plant-state rows (the state the action was applied from),  u_i = row i of the applied actions
//   w_i = the user's columns of w_plant[b][i] if given, else of θ_i as the workspace holds them when the kernel runs; the selector
//         columns of a lowered problem are θ_i's                                      (the rule of plant_step_kernel)
//   cost[b][i]      = cost_s(x_i, u_i, w_i)                                           (src/costs.jl:48-55: one stage term, no terminal term)
//   violation[b][i] = max over the stage rows of max(0, c) (inequality) or |c| (equality), c = con_s(x_i, u_i, w_i), from 0
//                     (src/data/constraints.jl:23-39; 0 on an unconstrained handle or without stage rows)
//
// plant_score_kernel: ONE LANE PER (instance, step) ELEMENT, e = b · k + i on lane e % 64 of workgroup e / 64 — the k rows of an
// instance are contiguous in x, u, w_plant and θ, so neighbouring lanes read neighbouring rows and write neighbouring outputs. An
// element is a pure function of its own three rows: no serial chain, no cross-lane arithmetic, no atomics, no LDS, nothing summed.
// Its bits depend neither on B nor on k nor on its neighbours; a non-finite row gives what the arithmetic gives (policy_violation's
// NaN-propagating max) and touches no other element. The same form serves small and large models: x_i and u_i are per-lane copies,
// as policy_rollout_large_kernel evaluates M::cost_s / M::con_s. The kernel READS the workspace (θ only) and writes only the
// caller's two output arrays.
#pragma once

namespace ilqr {

struct ScoreArgs {
    const double* ws;        // the handle's workspace (read-only here: θ)
    Layout L;
    int B;
    int steps;               // k, 1 .. T-1
    int n_sel;               // trailing parameter columns that stay the handle's (stage selectors) when w is given
    int constrained;
    const double* w;         // null, or rows of nw - n_sel doubles: row (b · w_ld + w_row0 + i)
    const double* x;         // rows of nx doubles: row (b · x_ld + x_row0 + i)
    const double* u;         // rows of nu doubles: row (b · u_ld + u_row0 + i)
    double* cost;            // element (b · cost_ld + cost_row0 + i)
    double* viol;            // null, or element (b · viol_ld + viol_row0 + i)
    long long w_ld, w_row0, x_ld, x_row0, u_ld, u_row0, cost_ld, cost_row0, viol_ld, viol_row0;
};

enum { SCORE_THREADS = 64 };

template <class M>
__global__ __launch_bounds__(SCORE_THREADS) void plant_score_kernel(ScoreArgs a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW, ncs = M::NCS;
    const long long e = (long long)blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (e >= (long long)a.B * a.steps) return;
    const size_t b = (size_t)(e / a.steps);
    const int i = (int)(e % a.steps);
    const Layout& L = a.L;
    const double* g = a.ws + b * (size_t)L.stride;
    const int nwu = NW - a.n_sel;
    const double* xr = a.x + (b * (size_t)a.x_ld + (size_t)a.x_row0 + (size_t)i) * n;
    const double* ur = a.u + (b * (size_t)a.u_ld + (size_t)a.u_row0 + (size_t)i) * m;
    double xt[n], ut[m], w[cdim<NW>::v];
#pragma unroll
    for (int j = 0; j < n; ++j) xt[j] = xr[j];
#pragma unroll
    for (int j = 0; j < m; ++j) ut[j] = ur[j];
    load_w<NW>(g + L.w, i, w);
    if constexpr (NW > 0) {
        if (a.w) {
            const double* wr = a.w + (b * (size_t)a.w_ld + (size_t)a.w_row0 + (size_t)i) * (size_t)(nwu > 0 ? nwu : 0);
#pragma unroll
            for (int j = 0; j < NW; ++j)
                if (j < nwu) w[j] = wr[j];
        }
    }
    a.cost[b * (size_t)a.cost_ld + (size_t)a.cost_row0 + (size_t)i] = M::cost_s(xt, ut, w);
    if (a.viol) {
        double v = 0.0;
        if constexpr (ncs > 0) {
            if (a.constrained) {
                double cv[ncs];
                M::con_s(xt, ut, w, cv);
                v = policy_violation<M, true, ncs>(0.0, cv);
            }
        }
        a.viol[b * (size_t)a.viol_ld + (size_t)a.viol_row0 + (size_t)i] = v;
    }
}

template <class M>
int launch_plant_score(const ScoreArgs* a, void* stream) {
    if (a->B < 1 || a->steps < 1 || a->steps > a->L.T - 1 || !a->x || !a->u || !a->cost) return -1;
    const size_t grid = ((size_t)a->B * (size_t)a->steps + SCORE_THREADS - 1) / SCORE_THREADS;
    if (grid > 0x7fffffffull) return -1;
    hipLaunchKernelGGL(plant_score_kernel<M>, dim3((unsigned)grid), dim3(SCORE_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
