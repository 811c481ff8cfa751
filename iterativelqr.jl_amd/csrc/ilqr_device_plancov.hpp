// A state covariance propagated down the handle's plan under its feedback policy (ilqr_plan_covariance, include/ilqr_hip.h): per
// instance Σ_0 = P0 [nx][nx] (row-major; the elements with row >= column are read and mirrored), and for t = 0 .. S−1
//
//   A   = ∂f/∂x, Bm = ∂f/∂u at (x̄_t, ū_t, θ_t) as the workspace holds them — the NOMINAL point, not an estimate: M::dyn_jac on the
//         small families (M::dyn is not called); on the large family the constant tables JAC_CONST_FX / JAC_CONST_FU with the
//         state-dependent entries (dyn_jac_var, or dyn_jac_var_own + JAC_VAR_ADD where they are elementwise) patched in through
//         JAC_VAR_IDX — BOTH ranges of it: an index >= nx·nx belongs to ∂f/∂u (est_jacobian_large drops those)
//   Φ   = A + Bm K_t (feedback), else A; K_t in plant_feedback_row's layout, Ks[j · m + i] = K_t(i, j). Without feedback K is not read
//   udiag[t][r] = Σ_a K_t(r, a) (Σ_b Σ_t(a, b) K_t(r, b)) (feedback), else 0
//   Σ_{t+1} = Φ Σ_t Φᵀ + diag(q): T = Φ Σ_t, then the elements of T Φᵀ with row >= column, each copied to its mirror
//
// Outputs, each null or an array of the caller's: sdiag [B][S+1][nx], udiag [B][S][nu], sigma [B][S+1][nx][nx], P_out [B][nx][nx]
// (= Σ_S; may alias P0: P0 is read once, before the first store), first_nonfinite [B] (−1, or the first t in 0 .. S with a
// non-finite entry on the diagonal of Σ_t).
//
// The kernels READ the workspace and write only the caller's arrays. No atomics, no cross-instance traffic, plain vector stores;
// every sum runs in an order fixed by the model's sizes alone, and nothing that is computed depends on which outputs are asked for,
// so an instance's bits depend neither on B, nor on its neighbours, nor on the optional outputs.
//
// plan_covariance_kernel (nx, nu <= 4): ONE INSTANCE PER LANE as estimate_predict_kernel; Σ, A, Bm, K_t, Φ and T in registers, every
// product an FMA chain in ascending index, Φ(r, c) starting from A(r, c).
// plan_covariance_large_kernel: ONE WAVE PER INSTANCE as estimate_predict_large_kernel. A / Φ, Σ and T in LDS at EstDims' padding
// (column-major, ld ≡ 16 (mod 32), zero-padded to 16 x 16 tiles), Bm and K_t as two panels of 16 rows of ld doubles (row k of the
// panel: column k of Bm, row k of K_t), so that Φ = A + Bm K_t accumulates onto A's tile in place (KD = 16), T = Φ Σ and T Φᵀ read
// their fragments along columns as the filter's products do; all on v_mfma_f64_16x16x4 through tile_mm / tile_load / tile_store of
// ilqr_device_large.hpp, unchanged. Φ takes A's place, so under feedback A's constant entries are put back at the start of every
// step (without feedback they are written once, as Bm's always are). udiag: the panel product Σ K_tᵀ into T's place, then lane r
// forms the dot product of row r of K_t with column r of it. Wave barriers only.
#pragma once

#include <stdint.h>

namespace ilqr {

struct PlanCovArgs {
    const double* ws;        // the handle's workspace (read-only here)
    Layout L;
    int B;
    int steps;               // S, 1 .. T-1
    int feedback;
    double q[PLANT_MAX_NX];  // the process noise variances by value, the first nx entries (0 where the caller gave none)
    const double* P0;        // [B][nx][nx]
    double* sdiag;           // null, or [B][S+1][nx]
    double* udiag;           // null, or [B][S][nu]
    double* sigma;           // null, or [B][S+1][nx][nx]
    double* P_out;           // null, or [B][nx][nx]
    int* nonfinite;          // null, or [B]
};
static_assert(sizeof(PlanCovArgs) <= 4096, "the kernel argument segment");

__device__ __forceinline__ bool plancov_finite(double v) { return fabs(v) < __builtin_huge_val(); }      // (false for NaN)

template <class M>
__global__ __launch_bounds__(64) void plan_covariance_kernel(PlanCovArgs a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const double* Pg = a.P0 + (size_t)b * n * n;
    const size_t S1 = (size_t)a.steps + 1;
    double P[n * n];
#pragma unroll
    for (int r = 0; r < n; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            const double v = Pg[r * n + c];
            P[r * n + c] = v;
            P[c * n + r] = v;
        }
    int nf = -1;
    for (int t = 0;; ++t) {
        bool fin = true;
#pragma unroll
        for (int j = 0; j < n; ++j) fin = fin && plancov_finite(P[j * n + j]);
        nf = (nf < 0 && !fin) ? t : nf;
        if (a.sdiag) {
#pragma unroll
            for (int j = 0; j < n; ++j) a.sdiag[((size_t)b * S1 + t) * n + j] = P[j * n + j];
        }
        if (a.sigma) {
#pragma unroll
            for (int e = 0; e < n * n; ++e) a.sigma[((size_t)b * S1 + t) * n * n + e] = P[e];
        }
        if (t == a.steps) break;
        double xt[n], ut[m], w[cdim<NW>::v];
#pragma unroll
        for (int j = 0; j < n; ++j) xt[j] = g[L.xb + t * n + j];
#pragma unroll
        for (int r = 0; r < m; ++r) ut[r] = g[L.ub + t * m + r];
        load_w<NW>(g + L.w, t, w);
        double fx[n * n], fu[n * m];                                                           // A(r, c) = fx[c · n + r], Bm(r, i) = fu[i · n + r]
        M::dyn_jac(xt, ut, w, fx, fu);
        if (a.feedback) {                                                                      // (the same branch on every lane)
            double K[m * n];                                                                   // K_t(i, j) = K[j · m + i]
#pragma unroll
            for (int e = 0; e < m * n; ++e) K[e] = g[L.K + t * (m * n) + e];
            if (a.udiag) {
#pragma unroll
                for (int r = 0; r < m; ++r) {
                    double s = 0.0;
#pragma unroll
                    for (int i = 0; i < n; ++i) {
                        double v = 0.0;
#pragma unroll
                        for (int j = 0; j < n; ++j) v = fma(P[i * n + j], K[j * m + r], v);
                        s = fma(K[i * m + r], v, s);
                    }
                    a.udiag[((size_t)b * a.steps + t) * m + r] = s;
                }
            }
#pragma unroll
            for (int r = 0; r < n; ++r)
#pragma unroll
                for (int c = 0; c < n; ++c) {
                    double s = fx[c * n + r];
#pragma unroll
                    for (int i = 0; i < m; ++i) s = fma(fu[i * n + r], K[c * m + i], s);
                    fx[c * n + r] = s;                                                         // Φ takes A's place
                }
        } else if (a.udiag) {
#pragma unroll
            for (int r = 0; r < m; ++r) a.udiag[((size_t)b * a.steps + t) * m + r] = 0.0;
        }
        double T[n * n];                                                                       // T = Φ Σ
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
    if (a.P_out) {
#pragma unroll
        for (int e = 0; e < n * n; ++e) a.P_out[(size_t)b * n * n + e] = P[e];
    }
    if (a.nonfinite) a.nonfinite[b] = nf;
}

// LDS of the large kernel: three NP x NP matrices with leading dimension ld (EstDims' padding), the panels of Bm and K_t (16 rows of
// ld doubles each), then x̄_t, ū_t, q and θ_t
template <class M>
struct PlanCovDims {
    static constexpr int n = M::NX, m = M::NU, NW = M::NW;
    static constexpr int NP = EstDims<M>::NP, NT = EstDims<M>::NT, ld = EstDims<M>::ld;
    static constexpr int oA = 0, oS = oA + ld * NP, oT = oS + ld * NP, oB = oT + ld * NP, oK = oB + 16 * ld, oX = oK + 16 * ld, oU = oX + 64,
                         oQ = oU + 16, oW = oQ + 64, total = oW + (NW > 0 ? (NW + 1) / 2 * 2 : 2);
    static constexpr size_t bytes = sizeof(double) * (size_t)total;
    static_assert(bytes <= 160 * 1024, "the LDS of a CU");
};

// A and Bm at (x̄_t, ū_t, θ_t) into the LDS copies whose constant entries are in place: the state-dependent entries of BOTH Jacobians
template <class M>
__device__ __forceinline__ void plancov_jacobians_large(double* sA, double* sB, const double* sx, const double* su, const double* sw, int lane) {
    constexpr int n = M::NX, m = M::NU, JV = M::JAC_NVAR, ld = PlanCovDims<M>::ld;
    if constexpr (JV > 0) {
        auto put = [&](int idx, double v) {                                    // entry idx of [fx (n·n) | fu (n·m)], column-major inside each
            if (idx < n * n) sA[(idx / n) * ld + idx % n] = v;
            else sB[((idx - n * n) / n) * ld + (idx - n * n) % n] = v;
        };
        double w[cdim<M::NW>::v];
        load_w<M::NW>(sw, 0, w);
        if constexpr (M::JAC_VAR_ELEMENTWISE) {
            for (int q = lane; q < JV; q += 64) put(M::JAC_VAR_IDX[q], M::dyn_jac_var_own(sx[M::JAC_VAR_SRC[q]], w) + M::JAC_VAR_ADD[0][q]);
        } else {
            double xa[n], ua[m], v[JV];
#pragma unroll
            for (int j = 0; j < n; ++j) xa[j] = sx[j];
#pragma unroll
            for (int j = 0; j < m; ++j) ua[j] = su[j];
            M::dyn_jac_var(xa, ua, w, v);                                     // (every lane: the same values)
            if constexpr (JV <= 256) {
#pragma unroll
                for (int q = 0; q < JV; ++q)
                    if (lane == (q & 63)) put(M::JAC_VAR_IDX[q], v[q]);
            } else {
                for (int q = lane; q < JV; q += 64) put(M::JAC_VAR_IDX[q], v[q]);
            }
        }
    }
}

template <class M>
__global__ __launch_bounds__(64) void plan_covariance_large_kernel(PlanCovArgs a) {
    typedef PlanCovDims<M> D;
    constexpr int n = M::NX, m = M::NU, NW = M::NW, NP = D::NP, NT = D::NT, ld = D::ld;
    static_assert(n <= PLANT_MAX_NX && m <= PLANT_MAX_NU, "q travels by value, one state row per lane; K_t is one panel of 16 rows");
    extern __shared__ __attribute__((aligned(16))) double plancov_lds[];
    double *sA = plancov_lds + D::oA, *sS = plancov_lds + D::oS, *sT = plancov_lds + D::oT, *sB = plancov_lds + D::oB, *sK = plancov_lds + D::oK,
           *sx = plancov_lds + D::oX, *su = plancov_lds + D::oU, *sq = plancov_lds + D::oQ, *sw = plancov_lds + D::oW;
    const int b = blockIdx.x, lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const double* Pg = a.P0 + (size_t)b * n * n;
    const size_t S1 = (size_t)a.steps + 1;
    double ql = 0.0;                                                          // q of the row this lane owns (lane < nx)
#pragma unroll
    for (int j = 0; j < n; ++j) ql = (lane == j) ? a.q[j] : ql;
    for (int e = lane; e < D::total; e += 64) plancov_lds[e] = 0.0;          // the padding of the tiles and of the panels
    wave_lds_fence();
    policy_wave_sync();
    for (int e = lane; e < n * n; e += 64) {
        const int r = e / n, c = e % n;
        sA[r * ld + c] = M::JAC_CONST_FX[0][e];
        sS[r * ld + c] = r >= c ? Pg[e] : Pg[c * n + r];                      // the lower triangle and its mirror
    }
    for (int e = lane; e < n * m; e += 64) sB[(e / n) * ld + e % n] = M::JAC_CONST_FU[0][e];
    sq[lane] = ql;
    int nf = -1;
    for (int t = 0;; ++t) {
        wave_lds_fence();
        policy_wave_sync();                                                   // Σ_t is in place
        const double dl = lane < n ? sS[lane * ld + lane] : 0.0;
        const bool bad = __builtin_amdgcn_ballot_w64(!plancov_finite(dl)) != 0;
        nf = (nf < 0 && bad) ? t : nf;
        if (a.sdiag && lane < n) a.sdiag[((size_t)b * S1 + t) * n + lane] = dl;
        if (a.sigma)
            for (int e = lane; e < n * n; e += 64) a.sigma[((size_t)b * S1 + t) * n * n + e] = sS[(e / n) * ld + e % n];
        if (t == a.steps) break;
        if (lane < n) sx[lane] = g[L.xb + t * n + lane];
        if (lane < m) su[lane] = g[L.ub + t * m + lane];
        for (int j = lane; j < NW; j += 64) sw[j] = g[L.w + t * NW + j];
        if (a.feedback) {                                                     // (uniform)
            if (t > 0)
                for (int e = lane; e < n * n; e += 64) sA[(e / n) * ld + e % n] = M::JAC_CONST_FX[0][e];      // Φ_{t−1} took A's place
            for (int e = lane; e < m * n; e += 64) sK[(e % m) * ld + e / m] = g[L.K + t * (m * n) + e];        // K_t(i, j) = Ks[j · m + i]
        }
        wave_lds_fence();
        policy_wave_sync();
        plancov_jacobians_large<M>(sA, sB, sx, su, sw, lane);
        wave_lds_fence();
        policy_wave_sync();
        if (a.feedback) {
            if (a.udiag) {
                for (int I = 0; I < NT; ++I) {                                // Σ K_tᵀ into T's place: A(i, k) = Σ(i, k), B(k, j) = K_t(j, k)
                    const double4_t acc = tile_mm<NP, 1, ld, 1, ld>(sS + 16 * I, sK, li, lk);
                    tile_store<ld>(sT, acc, 16 * I, 0, li, lk);
                }
                wave_lds_fence();
                policy_wave_sync();
                if (lane < m) {
                    double s = 0.0;
                    for (int i = 0; i < n; ++i) s = fma(sK[lane * ld + i], sT[lane * ld + i], s);
                    a.udiag[((size_t)b * a.steps + t) * m + lane] = s;
                }
                wave_lds_fence();
                policy_wave_sync();                                           // T's place is free again
            }
            for (int tt = 0; tt < NT * NT; ++tt) {                            // Φ = A + Bm K_t, tile by tile in place: A(i, k) = Bm(i, k), B(k, j) = K_t(k, j)
                const int I = tt / NT, J = tt % NT;
                double4_t acc = tile_load<ld>((const double*)sA, 16 * I, 16 * J, li, lk);
                acc = tile_mm<16, 1, ld, ld, 1>(sB + 16 * I, sK + 16 * J, li, lk, acc);
                tile_store<ld>(sA, acc, 16 * I, 16 * J, li, lk);
            }
            wave_lds_fence();
            policy_wave_sync();
        } else if (a.udiag && lane < m) {
            a.udiag[((size_t)b * a.steps + t) * m + lane] = 0.0;
        }
        for (int tt = 0; tt < NT * NT; ++tt) {                                // T = Φ Σ: A(i, k) = Φ(i, k), B(k, j) = Σ(j, k)
            const int I = tt / NT, J = tt % NT;
            const double4_t acc = tile_mm<NP, 1, ld, ld, 1>(sA + 16 * I, sS + 16 * J, li, lk);
            tile_store<ld>(sT, acc, 16 * I, 16 * J, li, lk);
        }
        wave_lds_fence();
        policy_wave_sync();
        for (int I = 0; I < NT; ++I)                                          // Σ = T Φᵀ + diag(q): A(i, k) = T(i, k), B(k, j) = Φ(j, k)
            for (int J = 0; J <= I; ++J) {
                const double4_t acc = tile_mm<NP, 1, ld, ld, 1>(sT + 16 * I, sA + 16 * J, li, lk);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * I + lk + 4 * r, col = 16 * J + li;
                    if (row < n && col <= row) {
                        const double v = row == col ? __dadd_rn(acc[r], sq[row]) : acc[r];
                        sS[col * ld + row] = v;
                        sS[row * ld + col] = v;
                    }
                }
            }
    }
    if (a.P_out)
        for (int e = lane; e < n * n; e += 64) a.P_out[(size_t)b * n * n + e] = sS[(e / n) * ld + e % n];
    if (lane == 0 && a.nonfinite) a.nonfinite[b] = nf;
}

template <class M>
int launch_plan_covariance(const PlanCovArgs* a, void* stream) {
    if (a->B < 1 || a->steps < 1 || a->steps > a->L.T - 1 || !a->P0 || (a->feedback != 0 && a->feedback != 1) ||
        !(a->sdiag || a->udiag || a->sigma || a->P_out || a->nonfinite))
        return -1;
    if constexpr (M::NX > PLANT_MAX_NX || M::NU > PLANT_MAX_NU) {
        return -1;
    } else if constexpr (is_large<M>::value) {
        constexpr size_t lds = PlanCovDims<M>::bytes;
        // dynamic LDS above the 64 KiB default needs the per-device function attribute (set on every such launch, as est_launch)
        if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(plan_covariance_large_kernel<M>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
        hipLaunchKernelGGL(plan_covariance_large_kernel<M>, dim3((unsigned)a->B), dim3(64), lds, (hipStream_t)stream, *a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    } else {
        hipLaunchKernelGGL(plan_covariance_kernel<M>, dim3((unsigned)((a->B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
}

}  // namespace ilqr
