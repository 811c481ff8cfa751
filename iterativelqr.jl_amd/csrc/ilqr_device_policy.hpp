// Batched closed-loop rollouts of a solved handle's policy (ilqr_rollout_policy, include/ilqr_hip.h):
//
//   x_1 = x1[b][s],   u_t = ū_t + K_t (x_t − x̄_t) + α k_t,   x_{t+1} = f(x_t, u_t, w_t)        (src/rollout.jl:19-30)
//
// for S samples of every instance b, with the plain objective Σ cost (src/costs.jl:48-55), constraint_violation
// (src/data/constraints.jl:23-39) and the first timestep with a non-finite state per sample. The kernels READ the handle's
// workspace (x̄, ū, K, k, θ) and write only to the caller's output arrays.
//
// Small models (nx, nu <= 4): ONE SAMPLE PER LANE, a workgroup of 1 .. 4 waves per (instance, block of samples). What a timestep
// needs of the instance — K_t, a_t = α k_t + ū_t, b_t = K_t x̄_t, θ_t — is the same for every lane: the workgroup stages it in LDS
// in chunks of POLICY_CHUNK timesteps (so no horizon limit) and the step reads it with broadcast LDS loads. State, cost, violation
// and the non-finite mark stay in the lane's registers for the whole horizon and are stored once. There is no cross-lane
// arithmetic: a sample's numbers do not depend on its neighbours. Trajectory output: a lane's own store would be strided by
// T·nx doubles, so each wave parks POLICY_TILE timesteps of its 64 samples in an LDS tile ([sample][step][component], odd row
// stride) and writes it out as contiguous runs of POLICY_TILE·nx doubles per sample.
//
// Large models: ONE WAVE PER SAMPLE in the manner of init_rollout_large_kernel (DynAff / dyn_row, x and u through LDS), row i of
// K_t on lane i; every lane evaluates the same cost and constraint terms of the step.
#pragma once

namespace ilqr {

struct PolicyArgs {
    const double* ws;        // the handle's workspace (read-only here)
    Layout L;
    int B, S;
    int constrained;
    int n_sel;               // trailing parameter columns that stay the handle's (stage selectors) when w is given
    int waves;               // small models: waves per workgroup (1 .. 4)
    double alpha;            // step_size
    const double* x1;        // [B][S][nx]
    const double* w;         // null, or [B][S][T][nw - n_sel]
    double* cost;            // [B][S]
    double* viol;            // null, or [B][S]
    int* nonfinite;          // null, or [B][S]
    double* x;               // null, or [B][S][T][nx]
    double* u;               // null, or [B][S][T-1][nu]
};

enum { POLICY_CHUNK = 16, POLICY_TILE = 8 };
static_assert(POLICY_CHUNK % POLICY_TILE == 0, "a tile never straddles two chunks");

template <class M>
struct PolicyDims {
    static constexpr int n = M::NX, m = M::NU, NW = M::NW;
    static constexpr int RS = m * n + 2 * m + NW;                       // doubles per staged timestep: K_t | a_t | b_t | θ_t
    static constexpr int POL = pad2(POLICY_CHUNK * RS);
    static constexpr int XS = POLICY_TILE * n + 1, US = POLICY_TILE * m + 1;   // tile row strides (odd: 64 lanes, 32 bank pairs)
    static constexpr int TILE = pad2(64 * XS + 64 * US);                // doubles per wave
    static constexpr int pow2(int v) { int p = 1; while (p < v) p *= 2; return p; }
    static constexpr int WX = pow2(POLICY_TILE * n), WU = pow2(POLICY_TILE * m);       // lanes that write out one sample's run
    static_assert(WX <= 64 && WU <= 64, "one run per pass of the wave");
    static constexpr size_t lds_bytes(int waves, bool traj) { return sizeof(double) * (size_t)(POL + (traj ? waves * TILE : 0)); }
};

__device__ __forceinline__ void policy_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// max(0, c) on inequality rows, |c| on equality rows, NaN-propagating like the reference's max
template <class M, bool STAGE, int NC>
__device__ __forceinline__ double policy_violation(double v, const double (&cv)[NC]) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const bool ineq = STAGE ? IneqMask<M>::s(i) : IneqMask<M>::t(i);
        v = nanmax(v, ineq ? nanmax(0.0, cv[i]) : fabs(cv[i]));
    }
    return v;
}

template <class M>
__global__ __launch_bounds__(256) void policy_rollout_kernel(PolicyArgs a) {
    typedef PolicyDims<M> D;
    constexpr int n = M::NX, m = M::NU, NW = M::NW, ncs = M::NCS, nct = M::NCT, RS = D::RS, KN = m * n;
    extern __shared__ __attribute__((aligned(16))) double policy_lds[];
    const Layout& L = a.L;
    const int T = L.T, N = T - 1, S = a.S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
    const int blocks = (S + nthreads - 1) / nthreads;
    const int b = blockIdx.x / blocks, s_wave = (blockIdx.x % blocks) * nthreads + 64 * wave;
    if (b >= a.B) return;
    // a lane behind the last sample runs the last sample again and stores nothing: every lane reaches every barrier
    const bool live = s_wave + lane < S;
    const int s = live ? s_wave + lane : S - 1;
    const size_t bs = (size_t)b * S + s;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const bool traj = a.x != nullptr || a.u != nullptr;
    double* pol = policy_lds;
    double* tx = policy_lds + D::POL + wave * D::TILE;
    double* tu = tx + 64 * D::XS;
    const int nwu = NW - a.n_sel;
    const double* wsmp = a.w ? a.w + bs * (size_t)T * (size_t)(nwu > 0 ? nwu : 0) : nullptr;

    double xt[n];
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = a.x1[bs * n + i];
    double J = 0.0, viol = 0.0;
    int nf = -1;

    for (int t0 = 0; t0 < T; t0 += POLICY_CHUNK) {
        const int cnt = (T - t0) < POLICY_CHUNK ? (T - t0) : POLICY_CHUNK;
        __syncthreads();                                   // the previous chunk has been read by every wave
        for (int e = tid; e < cnt * RS; e += nthreads) {
            const int st = e / RS, r = e % RS, t = t0 + st;
            double v = 0.0;
            if (r >= KN + 2 * m) {
                v = g[L.w + t * NW + (r - KN - 2 * m)];
            } else if (t < N) {
                if (r < KN) {
                    v = g[L.K + t * KN + r];
                } else if (r < KN + m) {
                    const int i = r - KN;
                    v = fma(g[L.k + t * m + i], a.alpha, g[L.ub + t * m + i]);                 // α k + ū   (:24-26)
                } else {
                    const int i = r - KN - m;
                    for (int j = 0; j < n; ++j) v = fma(g[L.K + t * KN + j * m + i], g[L.xb + t * n + j], v);   // K x̄
                }
            }
            pol[e] = v;
        }
        __syncthreads();
        for (int st = 0; st < cnt; ++st) {
            const int t = t0 + st, tq = t % POLICY_TILE;
            const double* row = pol + st * RS;
            bool fin = true;
#pragma unroll
            for (int i = 0; i < n; ++i) fin = fin && (fabs(xt[i]) < __builtin_huge_val());     // false for ±Inf and NaN
            nf = (nf < 0 && !fin) ? t : nf;
            double w[cdim<NW>::v];
            w[0] = 0.0;
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = row[KN + 2 * m + i];
            if constexpr (NW > 0) {
                if (wsmp) {
#pragma unroll
                    for (int i = 0; i < NW; ++i)
                        if (i < nwu) w[i] = wsmp[(size_t)t * nwu + i];
                }
            }
            if (traj) {
#pragma unroll
                for (int i = 0; i < n; ++i) tx[lane * D::XS + tq * n + i] = xt[i];
            }
            if (t < N) {
                double ut[m];
#pragma unroll
                for (int i = 0; i < m; ++i) {
                    double kx = 0.0;
#pragma unroll
                    for (int j = 0; j < n; ++j) kx = fma(row[j * m + i], xt[j], kx);
                    ut[i] = (row[KN + i] + kx) - row[KN + m + i];                              // (:27), (:28)
                }
                J += M::cost_s(xt, ut, w);
                if constexpr (ncs > 0) {
                    if (a.constrained) {
                        double cv[ncs];
                        M::con_s(xt, ut, w, cv);
                        viol = policy_violation<M, true, ncs>(viol, cv);
                    }
                }
                if (traj) {
#pragma unroll
                    for (int i = 0; i < m; ++i) tu[lane * D::US + tq * m + i] = ut[i];
                }
                double y[n];
                M::dyn(xt, ut, w, y);                                                          // (:29)
#pragma unroll
                for (int i = 0; i < n; ++i) xt[i] = y[i];
            } else {
                J += M::cost_t(xt, w);
                if constexpr (nct > 0) {
                    if (a.constrained) {
                        double cv[nct];
                        M::con_t(xt, w, cv);
                        viol = policy_violation<M, false, nct>(viol, cv);
                    }
                }
            }
            if (traj && (tq == POLICY_TILE - 1 || t == T - 1)) {
                // the tile holds steps [tb, t] of the wave's samples: sample r's run goes out from D::WX (D::WU) neighbouring lanes
                const int tb = t - tq, cx = (tq + 1) * n, cu = ((t < N ? t + 1 : N) - tb) * m;
                policy_wave_sync();
                if (a.x) {
                    const int l = lane % D::WX;
                    for (int r = lane / D::WX; r < 64; r += 64 / D::WX)
                        if (l < cx && s_wave + r < S) a.x[(((size_t)b * S + s_wave + r) * T + tb) * n + l] = tx[r * D::XS + l];
                }
                if (a.u && cu > 0) {
                    const int l = lane % D::WU;
                    for (int r = lane / D::WU; r < 64; r += 64 / D::WU)
                        if (l < cu && s_wave + r < S) a.u[(((size_t)b * S + s_wave + r) * N + tb) * m + l] = tu[r * D::US + l];
                }
                policy_wave_sync();
            }
        }
    }
    if (live) {
        a.cost[bs] = J;
        if (a.viol) a.viol[bs] = viol;
        if (a.nonfinite) a.nonfinite[bs] = nf;
    }
}

template <class M>
__global__ __launch_bounds__(64) void policy_rollout_large_kernel(PolicyArgs a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW, ncs = M::NCS, nct = M::NCT, KN = m * n;
    __shared__ double sx[n], su[m], sw[cdim<NW>::v];
    const Layout& L = a.L;
    const int T = L.T, N = T - 1, S = a.S, lane = threadIdx.x;
    const int b = blockIdx.x / S, s = blockIdx.x % S;
    if (b >= a.B) return;
    const size_t bs = (size_t)b * S + s;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const int nwu = NW - a.n_sel;
    const double* wsmp = a.w ? a.w + bs * (size_t)T * (size_t)(nwu > 0 ? nwu : 0) : nullptr;
    DynAff<M> aff;
    aff.init(lane);
    const int xrow = DynAff<M>::SPLIT ? (lane & 31) : lane;
    double xl = xrow < n ? a.x1[bs * n + xrow] : 0.0;
    double J = 0.0, viol = 0.0;
    int nf = -1;
    if (lane == 0) sw[0] = 0.0;
    for (int t = 0; t < T; ++t) {
        if (lane < n) { sx[lane] = xl; if (a.x) a.x[(bs * T + t) * n + lane] = xl; }
        for (int i = lane; i < NW; i += 64) sw[i] = (wsmp && i < nwu) ? wsmp[(size_t)t * nwu + i] : g[L.w + t * NW + i];
        wave_lds_fence();
        policy_wave_sync();
        double xa[n], w[cdim<NW>::v];
        bool fin = true;
#pragma unroll
        for (int j = 0; j < n; ++j) { xa[j] = sx[j]; fin = fin && (fabs(xa[j]) < __builtin_huge_val()); }
#pragma unroll
        for (int i = 0; i < cdim<NW>::v; ++i) w[i] = sw[i];
        nf = (nf < 0 && !fin) ? t : nf;
        if (t < N) {
            if (lane < m) {                                                   // row `lane` of K_t
                const double* Kt = g + L.K + t * KN;
                double kx = 0.0, kb = 0.0;
#pragma unroll
                for (int j = 0; j < n; ++j) { kx = fma(Kt[j * m + lane], xa[j], kx); kb = fma(Kt[j * m + lane], g[L.xb + t * n + j], kb); }
                const double v = (fma(g[L.k + t * m + lane], a.alpha, g[L.ub + t * m + lane]) + kx) - kb;    // (:24-28)
                su[lane] = v;
                if (a.u) a.u[(bs * N + t) * m + lane] = v;
            }
            wave_lds_fence();
            policy_wave_sync();
            double ua[m];
#pragma unroll
            for (int j = 0; j < m; ++j) ua[j] = su[j];
            J += M::cost_s(xa, ua, w);
            if constexpr (ncs > 0) {
                if (a.constrained) {
                    double cv[ncs];
                    M::con_s(xa, ua, w, cv);
                    viol = policy_violation<M, true, ncs>(viol, cv);
                }
            }
            xl = dyn_row<M>(aff, sx, ua, xl, lane, sw, 0);                    // (:29)
        } else {
            J += M::cost_t(xa, w);
            if constexpr (nct > 0) {
                if (a.constrained) {
                    double cv[nct];
                    M::con_t(xa, w, cv);
                    viol = policy_violation<M, false, nct>(viol, cv);
                }
            }
        }
        wave_lds_fence();
        policy_wave_sync();                                                   // sx, su, sw are rewritten by the next step
    }
    if (lane == 0) {
        a.cost[bs] = J;
        if (a.viol) a.viol[bs] = viol;
        if (a.nonfinite) a.nonfinite[bs] = nf;
    }
}

template <class M>
int launch_policy_rollout(const PolicyArgs* a, void* stream) {
    if (a->B < 1 || a->S < 1) return -1;
    if constexpr (is_large<M>::value) {
        const size_t grid = (size_t)a->B * (size_t)a->S;
        if (grid > 0x7fffffffull) return -1;
        hipLaunchKernelGGL(policy_rollout_large_kernel<M>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, *a);
    } else {
        const int waves = a->waves < 1 ? 1 : (a->waves > 4 ? 4 : a->waves), nthreads = 64 * waves;
        const size_t grid = (size_t)a->B * (size_t)((a->S + nthreads - 1) / nthreads);
        if (grid > 0x7fffffffull) return -1;
        const bool traj = a->x != nullptr || a->u != nullptr;
        const size_t lds = PolicyDims<M>::lds_bytes(waves, traj);
        auto kernel = policy_rollout_kernel<M>;
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
        PolicyArgs q = *a;
        q.waves = waves;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(nthreads), lds, (hipStream_t)stream, q);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
