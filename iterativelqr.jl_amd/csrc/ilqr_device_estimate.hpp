// A batched extended Kalman filter between the plant's sensor and the controller (ilqr_estimate_predict, ilqr_estimate_update,
// ilqr_mpc_run_est, include/ilqr_hip.h): per instance an estimate x̂ [nx] and its covariance P [nx][nx] (row-major, symmetric, both
// triangles stored) that live in HBM, q and r the diagonals of the process and measurement noise covariances.
//
// TIME UPDATE over k = steps control periods under the head of the handle's plan, for i = 0 .. k−1
//
//   u_i = the action ilqr_plant_step_limited forms from the state it is handed, here x̂: ū_i, or ū_i + K_i (x̂ − x̄_i)
//         (plant_feedback_row), then the limits (plant_clamp)
//   w_i = θ_i as the handle holds it (the filter knows the controller's model only: there is no w_plant)
//   F   = ∂f/∂x (x̂, u_i, w_i), the model's own dynamics state Jacobian, taken BEFORE the state moves: M::dyn_jac on the small
//         families; on the large family the constant table JAC_CONST_FX with the state-dependent entries (dyn_jac_var, or
//         dyn_jac_var_own + JAC_VAR_ADD where they are elementwise) patched in through JAC_VAR_IDX, as the solve kernel's LDS copy
//   x̂  ← f(x̂, u_i, w_i): M::dyn / dyn_row, the step of plant_step_kernel / plant_step_large_kernel without noise: the same bits
//   P  ← F P Fᵀ + diag(q): T = F P, then the elements of T Fᵀ with row >= column, each copied to its mirror
//
// MEASUREMENT UPDATE with y [nx]: for j = 0 .. nx−1 in increasing order where measured[j], on the x̂ and P the previous j left
//
//   ν = y_j − x̂_j,  s = P_jj + r_j;  s not a finite number > 0: the component is skipped, first_bad = the first such j (else −1)
//   g = P[:, j] / s;  x̂ ← x̂ + g ν;  P_ab ← P_ab − g_a P_jb for a >= b from the column and row as they were, then mirrored
//   nis = Σ ν² / s over the updated components; innovation[j] = ν, or 0 where not measured or skipped
//
// The kernels READ the workspace and write only the caller's arrays. No atomics, no cross-instance traffic, plain vector stores;
// every sum runs in an order fixed by the model's sizes alone, so an instance's bits depend neither on B nor on its neighbours.
//
// estimate_predict_kernel / estimate_update_kernel (nx, nu <= 4): ONE INSTANCE PER LANE as plant_step_kernel; x̂, F, T and P in
// registers, P read from HBM once per call and written once.
// estimate_predict_large_kernel: ONE WAVE PER INSTANCE as plant_step_large_kernel. F, P and T in LDS, column-major with leading
// dimension EstDims::ld, zero-padded to 16 x 16 tiles; both products on v_mfma_f64_16x16x4 through tile_mm / tile_store of the large
// solve kernel (ilqr_device_large.hpp, unchanged): T = F P every tile, T Fᵀ the tiles on or below the diagonal. P is symmetric,
// so the B operand of the first product is read as P(j, k) and every fragment read runs along a column: consecutive doubles
// across the 16 lanes of a fragment row, and ld ≡ 16 (mod 32) puts the two fragment rows of a half-wave on disjoint banks.
// estimate_update_large_kernel: ONE WAVE PER INSTANCE, lane a owns row a of P (in LDS). Row j goes through LDS to every lane; lane a
// reads its row through the mirror (column a: consecutive doubles across the wave) and writes both places.
#pragma once

#include <stdint.h>

namespace ilqr {

struct EstArgs {
    const double* ws;        // the handle's workspace (read-only here)
    Layout L;
    int B;
    int steps;               // predict: k, 1 .. T-1
    int feedback;
    int clamp;               // u_lo, u_hi hold the limits (an entry may still be ∓Inf)
    unsigned mask[2];        // update: bit j of word j / 32 — component j is measured
    double u_lo[PLANT_MAX_NU], u_hi[PLANT_MAX_NU];       // by value: the first nu entries
    double q[PLANT_MAX_NX];  // predict: the process noise variances by value, the first nx entries
    double r[PLANT_MAX_NX];  // update: the measurement noise variances by value
    double* xhat;            // [B][nx] in / out
    double* P;               // [B][nx][nx] in / out
    const double* y;         // update: [B][nx]; unmeasured components are not read
    double* innovation;      // update: null, or [B][nx]
    double* nis;             // update: null, or [B]
    int* first_bad;          // update: null, or [B]
};
static_assert(sizeof(EstArgs) <= 4096, "the kernel argument segment");

// a finite number > 0 (false for NaN)
__device__ __forceinline__ bool est_pivot_ok(double s) { return s > 0.0 && s < __builtin_huge_val(); }

template <class M>
__global__ __launch_bounds__(64) void estimate_predict_kernel(EstArgs a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    double* Pg = a.P + (size_t)b * n * n;
    double xt[n], P[n * n];
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = a.xhat[(size_t)b * n + i];
#pragma unroll
    for (int i = 0; i < n * n; ++i) P[i] = Pg[i];
    for (int i = 0; i < a.steps; ++i) {
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
                }
            }
        }
        double w[cdim<NW>::v];
        load_w<NW>(g + L.w, i, w);
        double fx[n * n], fu[n * m];                                                           // F(r, c) = fx[c · n + r]
        M::dyn_jac(xt, ut, w, fx, fu);
        M::dyn(xt, ut, w, y);                                                                  // (:29)
#pragma unroll
        for (int j = 0; j < n; ++j) xt[j] = y[j];
        double T[n * n];                                                                       // T = F P
#pragma unroll
        for (int r = 0; r < n; ++r)
#pragma unroll
            for (int c = 0; c < n; ++c) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < n; ++j) s = fma(fx[j * n + r], P[j * n + c], s);
                T[r * n + c] = s;
            }
#pragma unroll
        for (int r = 0; r < n; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < n; ++j) s = fma(T[r * n + j], fx[j * n + c], s);
                if (r == c) s = __dadd_rn(s, a.q[r]);
                P[r * n + c] = s;
                P[c * n + r] = s;
            }
    }
#pragma unroll
    for (int i = 0; i < n; ++i) a.xhat[(size_t)b * n + i] = xt[i];
#pragma unroll
    for (int i = 0; i < n * n; ++i) Pg[i] = P[i];
}

template <class M>
__global__ __launch_bounds__(64) void estimate_update_kernel(EstArgs a) {
    constexpr int n = M::NX;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* Pg = a.P + (size_t)b * n * n;
    double xt[n], P[n * n], inn[n];
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = a.xhat[(size_t)b * n + i];
#pragma unroll
    for (int i = 0; i < n * n; ++i) P[i] = Pg[i];
    double nis = 0.0;
    int bad = -1;
#pragma unroll
    for (int j = 0; j < n; ++j) {
        inn[j] = 0.0;
        if (!(a.mask[j / 32] >> (j % 32) & 1u)) continue;                                      // (the same branch on every lane)
        const double nu = a.y[(size_t)b * n + j] - xt[j], s = P[j * n + j] + a.r[j];
        if (!est_pivot_ok(s)) { bad = bad < 0 ? j : bad; continue; }
        double row[n], gn[n];
#pragma unroll
        for (int c = 0; c < n; ++c) { row[c] = P[j * n + c]; gn[c] = P[c * n + j] / s; }
#pragma unroll
        for (int r = 0; r < n; ++r) {
            xt[r] = xt[r] + gn[r] * nu;
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                const double v = P[r * n + c] - gn[r] * row[c];
                P[r * n + c] = v;
                P[c * n + r] = v;
            }
        }
        nis += nu * nu / s;
        inn[j] = nu;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) a.xhat[(size_t)b * n + i] = xt[i];
#pragma unroll
    for (int i = 0; i < n * n; ++i) Pg[i] = P[i];
    if (a.innovation) {
#pragma unroll
        for (int i = 0; i < n; ++i) a.innovation[(size_t)b * n + i] = inn[i];
    }
    if (a.nis) a.nis[b] = nis;
    if (a.first_bad) a.first_bad[b] = bad;
}

// LDS of the large predict kernel: three NP x NP matrices with leading dimension ld (doubles), then x̂, u, θ_i and q
template <class M>
struct EstDims {
    static constexpr int n = M::NX, m = M::NU, NW = M::NW;
    static constexpr int NP = (n + 15) / 16 * 16, NT = NP / 16;
    static constexpr int ld = NP % 32 == 0 ? NP + 16 : NP;                   // ≡ 16 (mod 32)
    static constexpr int oF = 0, oP = oF + ld * NP, oT = oP + ld * NP, oX = oT + ld * NP, oU = oX + 64, oQ = oU + (m + 1) / 2 * 2,
                         oW = oQ + 64, total = oW + (NW > 0 ? (NW + 1) / 2 * 2 : 2);
    static constexpr size_t predict_bytes = sizeof(double) * (size_t)total;
    // the update kernel: one matrix, row pitch odd in doubles (the mirrored store walks a column), then x̂, y, r and row j
    static constexpr int uld = n | 1, uX = uld * n + 1, uY = uX + 64, uR = uY + 64, uRow = uR + 64, utotal = uRow + 64;
    static constexpr size_t update_bytes = sizeof(double) * (size_t)utotal;
};

// F at (x̂, u_i, θ_i) into the LDS copy whose constant entries are in place: the state-dependent entries of ∂f/∂x
template <class M>
__device__ __forceinline__ void est_jacobian_large(double* sF, const double* sx, const double (&ua)[M::NU], const double* sw, int lane) {
    constexpr int n = M::NX, JV = M::JAC_NVAR, ld = EstDims<M>::ld;
    if constexpr (JV > 0) {
        double w[cdim<M::NW>::v];
        load_w<M::NW>(sw, 0, w);
        if constexpr (M::JAC_VAR_ELEMENTWISE) {
            for (int q = lane; q < JV; q += 64) {
                const int idx = M::JAC_VAR_IDX[q];
                if (idx < n * n) sF[(idx / n) * ld + idx % n] = M::dyn_jac_var_own(sx[M::JAC_VAR_SRC[q]], w) + M::JAC_VAR_ADD[0][q];
            }
        } else {
            double xa[n], v[JV];
#pragma unroll
            for (int j = 0; j < n; ++j) xa[j] = sx[j];
            M::dyn_jac_var(xa, ua, w, v);                                     // (every lane: the same values)
            if constexpr (JV <= 256) {
#pragma unroll
                for (int q = 0; q < JV; ++q)
                    if (M::JAC_VAR_IDX[q] < n * n && lane == (q & 63)) sF[(M::JAC_VAR_IDX[q] / n) * ld + M::JAC_VAR_IDX[q] % n] = v[q];
            } else {
                for (int q = lane; q < JV; q += 64) {
                    const int idx = M::JAC_VAR_IDX[q];
                    if (idx < n * n) sF[(idx / n) * ld + idx % n] = v[q];
                }
            }
        }
    }
}

template <class M>
__global__ __launch_bounds__(64) void estimate_predict_large_kernel(EstArgs a) {
    typedef EstDims<M> D;
    constexpr int n = M::NX, m = M::NU, NW = M::NW, NP = D::NP, NT = D::NT, ld = D::ld;
    static_assert(n <= PLANT_MAX_NX, "q travels by value, one state row per lane");
    extern __shared__ __attribute__((aligned(16))) double est_lds[];
    double *sF = est_lds + D::oF, *sP = est_lds + D::oP, *sT = est_lds + D::oT, *sx = est_lds + D::oX, *su = est_lds + D::oU,
           *sq = est_lds + D::oQ, *sw = est_lds + D::oW;
    const int b = blockIdx.x, lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    double* Pg = a.P + (size_t)b * n * n;
    DynAff<M> aff;
    aff.init(lane);
    const int xrow = DynAff<M>::SPLIT ? (lane & 31) : lane;
    double xl = xrow < n ? a.xhat[(size_t)b * n + xrow] : 0.0;
    double ql = 0.0;                                                          // q of the row this lane owns (lane < nx)
#pragma unroll
    for (int j = 0; j < n; ++j) ql = (lane == j) ? a.q[j] : ql;
    double ulo = 0.0, uhi = 0.0;                                              // the limits of the action row this lane owns (lane < nu)
    if constexpr (m <= PLANT_MAX_NU) {
        if (a.clamp) {
#pragma unroll
            for (int j = 0; j < m; ++j) { ulo = (lane == j) ? a.u_lo[j] : ulo; uhi = (lane == j) ? a.u_hi[j] : uhi; }
        }
    }
    for (int e = lane; e < D::total; e += 64) est_lds[e] = 0.0;              // the padding of the tiles
    wave_lds_fence();
    policy_wave_sync();
    for (int e = lane; e < n * n; e += 64) {
        sF[(e / n) * ld + e % n] = M::JAC_CONST_FX[0][e];
        sP[(e / n) * ld + e % n] = Pg[e];                                     // (symmetric: row-major is column-major)
    }
    sq[lane] = ql;
    for (int i = 0; i < a.steps; ++i) {
        if (lane < n) sx[lane] = xl;
        for (int j = lane; j < NW; j += 64) sw[j] = g[L.w + i * NW + j];
        wave_lds_fence();
        policy_wave_sync();
        if (lane < m) {                                                       // row `lane` of K_i
            double v = a.feedback ? plant_feedback_row<M>(g, L, i, lane, [&](int j) { return sx[j]; }) : g[L.ub + i * m + lane];
            bool changed = false;
            if (a.clamp) v = plant_clamp(v, ulo, uhi, changed);
            su[lane] = v;
        }
        wave_lds_fence();
        policy_wave_sync();
        double ua[m];
#pragma unroll
        for (int j = 0; j < m; ++j) ua[j] = su[j];
        est_jacobian_large<M>(sF, sx, ua, sw, lane);                          // before the state moves
        xl = dyn_row<M>(aff, sx, ua, xl, lane, sw, 0);                        // (:29)
        wave_lds_fence();
        policy_wave_sync();
        for (int t = 0; t < NT * NT; ++t) {                                   // T = F P: A(i, k) = F(i, k), B(k, j) = P(j, k)
            const int I = t / NT, J = t % NT;
            const double4_t acc = tile_mm<NP, 1, ld, ld, 1>(sF + 16 * I, sP + 16 * J, li, lk);
            tile_store<ld>(sT, acc, 16 * I, 16 * J, li, lk);
        }
        wave_lds_fence();
        policy_wave_sync();
        for (int I = 0; I < NT; ++I)                                          // P = T Fᵀ + diag(q): A(i, k) = T(i, k), B(k, j) = F(j, k)
            for (int J = 0; J <= I; ++J) {
                const double4_t acc = tile_mm<NP, 1, ld, ld, 1>(sT + 16 * I, sF + 16 * J, li, lk);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * I + lk + 4 * r, col = 16 * J + li;
                    if (row < n && col <= row) {
                        const double v = row == col ? __dadd_rn(acc[r], sq[row]) : acc[r];
                        sP[col * ld + row] = v;
                        sP[row * ld + col] = v;
                    }
                }
            }
        wave_lds_fence();
        policy_wave_sync();                                                   // sx, su, sw and the state-dependent entries of F are rewritten by the next step
    }
    if (lane < n) a.xhat[(size_t)b * n + lane] = xl;
    for (int e = lane; e < n * n; e += 64) Pg[e] = sP[(e / n) * ld + e % n];
}

template <class M>
__global__ __launch_bounds__(64) void estimate_update_large_kernel(EstArgs a) {
    typedef EstDims<M> D;
    constexpr int n = M::NX, ld = D::uld;
    static_assert(n <= PLANT_MAX_NX, "r travels by value, one row of P per lane");
    extern __shared__ __attribute__((aligned(16))) double est_lds[];
    double *sP = est_lds, *sx = est_lds + D::uX, *sy = est_lds + D::uY, *sr = est_lds + D::uR, *srow = est_lds + D::uRow;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.B) return;
    double* Pg = a.P + (size_t)b * n * n;
    double rl = 0.0;                                                          // r of the row this lane owns (lane < nx)
#pragma unroll
    for (int j = 0; j < n; ++j) rl = (lane == j) ? a.r[j] : rl;
    const unsigned word = lane < 32 ? a.mask[0] : a.mask[1];
    const bool mine = lane < n && (word >> (lane & 31) & 1u) != 0;            // this lane's component is measured
    double xl = lane < n ? a.xhat[(size_t)b * n + lane] : 0.0;
    for (int e = lane; e < n * n; e += 64) sP[(e / n) * ld + e % n] = Pg[e];
    sy[lane] = mine ? a.y[(size_t)b * n + lane] : 0.0;
    sr[lane] = rl;
    double nis = 0.0, inn = 0.0;
    int bad = -1;
    for (int j = 0; j < n; ++j) {
        const unsigned wj = j < 32 ? a.mask[0] : a.mask[1];
        if (!(wj >> (j & 31) & 1u)) continue;                                 // (uniform)
        sx[lane] = xl;
        wave_lds_fence();
        policy_wave_sync();
        const double nu = sy[j] - sx[j], s = sP[j * ld + j] + sr[j];         // (uniform: every lane reads the same words)
        if (!est_pivot_ok(s)) {
            bad = bad < 0 ? j : bad;
            wave_lds_fence();
            policy_wave_sync();
            continue;
        }
        const double pj = lane < n ? sP[j * ld + lane] : 0.0;                 // P(j, a) = P(a, j)
        const double gn = pj / s;
        srow[lane] = pj;
        wave_lds_fence();
        policy_wave_sync();
        xl = xl + gn * nu;
        if (lane < n)
            for (int c = 0; c <= lane; ++c) {                                 // element (a, c), c <= a, read at its mirror (c, a)
                const double v = sP[c * ld + lane] - gn * srow[c];
                sP[c * ld + lane] = v;
                sP[lane * ld + c] = v;
            }
        nis += nu * nu / s;
        inn = lane == j ? nu : inn;
        wave_lds_fence();
        policy_wave_sync();
    }
    wave_lds_fence();
    policy_wave_sync();
    if (lane < n) {
        a.xhat[(size_t)b * n + lane] = xl;
        if (a.innovation) a.innovation[(size_t)b * n + lane] = inn;
    }
    for (int e = lane; e < n * n; e += 64) Pg[e] = sP[(e / n) * ld + e % n];
    if (lane == 0 && a.nis) a.nis[b] = nis;
    if (lane == 0 && a.first_bad) a.first_bad[b] = bad;
}

// dynamic LDS above the 64 KiB default needs the per-device function attribute (set on every such launch, as ModelModule::go)
template <class K>
int est_launch(K kernel, unsigned grid, size_t lds, void* stream, const EstArgs& a) {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class M>
int launch_estimate_predict(const EstArgs* a, void* stream) {
    if (a->B < 1 || a->steps < 1 || a->steps > a->L.T - 1 || !a->xhat || !a->P || M::NX > PLANT_MAX_NX || (a->clamp && M::NU > PLANT_MAX_NU)) return -1;
    if constexpr (is_large<M>::value)
        return est_launch(estimate_predict_large_kernel<M>, (unsigned)a->B, EstDims<M>::predict_bytes, stream, *a);
    else
        return est_launch(estimate_predict_kernel<M>, (unsigned)((a->B + 63) / 64), 0, stream, *a);
}

template <class M>
int launch_estimate_update(const EstArgs* a, void* stream) {
    if (a->B < 1 || !a->xhat || !a->P || !a->y || M::NX > PLANT_MAX_NX) return -1;
    if constexpr (is_large<M>::value)
        return est_launch(estimate_update_large_kernel<M>, (unsigned)a->B, EstDims<M>::update_bytes, stream, *a);
    else
        return est_launch(estimate_update_kernel<M>, (unsigned)((a->B + 63) / 64), 0, stream, *a);
}

}  // namespace ilqr
