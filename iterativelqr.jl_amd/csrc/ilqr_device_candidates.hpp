// Scoring and selection of candidate initial guesses (ilqr_initialize_rollout_candidates, include/ilqr_hip.h): for S action
// sequences per instance b
//
//   x_1 = x1[b],   x_{t+1} = f(x_t, u[b][s][t], w_t)                                                    (src/rollout.jl:33-42)
//
// with the plain objective Σ cost (src/costs.jl:48-55, summed in timestep order), constraint_violation
// (src/data/constraints.jl:23-39) and the first timestep with a non-finite state per candidate; then, per instance, the argmin
// of  score = cost [+ weight · max_violation]  over the eligible candidates and a copy of the winner's (x1, ū) into the handle's
// resident input buffers, from which the existing init_rollout kernels install it. The scoring kernels READ the handle's
// workspace (θ only) and write the caller's score arrays; the select kernel writes chosen[b] and the resident inputs.
//
// Small models (nx, nu <= 4): ONE CANDIDATE PER LANE, a workgroup of 1 .. 4 waves per (instance, block of candidates). x1[b]
// and θ_t are the same on every lane; θ_t is staged in LDS in chunks of CAND_CHUNK timesteps (no horizon limit) and read with
// broadcast LDS loads. A lane's own actions lie (T-1)·nu doubles from its neighbour's, so each wave loads CAND_TILE timesteps
// of its 64 candidates as contiguous runs of CAND_TILE·nu doubles per candidate — D::WU neighbouring lanes per run — into
// registers, parks them in an LDS tile ([candidate][step][component], odd row stride) and every lane reads its own row: the
// load-side mirror of the policy kernel's trajectory store. The loads of steps t+8.. are issued before steps t.. are computed.
// State, cost, violation and the non-finite mark stay in registers. There is no cross-lane arithmetic: a candidate's numbers do
// not depend on S or on its neighbours.
//
// Large models: ONE WAVE PER CANDIDATE in the manner of init_rollout_large_kernel (DynAff / dyn_row, x and u through LDS).
//
// Select: one workgroup per instance, a shuffle reduction per wave and a combine through LDS under the total order
// (eligible first, score, index) — no atomics, so the result does not depend on timing.
#pragma once

namespace ilqr {

struct CandArgs {
    const double* ws;        // the handle's workspace (read-only here)
    Layout L;
    int B, S;
    int constrained;
    int waves;               // small models: waves per workgroup of the scoring kernel (1 .. 4)
    double weight;           // violation_weight (finite, >= 0)
    const double* x1;        // [B][nx]
    const double* u;         // [B][S][T-1][nu]
    double* cost;            // [B][S]
    double* viol;            // [B][S]
    int* nonfinite;          // [B][S]
    int* chosen;             // null, or [B]
    double* r_x1;            // the handle's resident inputs: [B][nx] (may be x1 itself)
    double* r_u;             //                               [B][T-1][nu]
};

enum { CAND_CHUNK = 16, CAND_TILE = 8, CAND_SELECT_THREADS = 256 };
static_assert(CAND_CHUNK % CAND_TILE == 0, "a tile never straddles two chunks");

template <class M>
struct CandDims {
    static constexpr int m = M::NU, NW = M::NW;
    static constexpr int TH = pad2(CAND_CHUNK * NW);                    // staged θ of a chunk
    static constexpr int US = CAND_TILE * m + 1;                        // tile row stride (odd: 64 lanes, 32 bank pairs)
    static constexpr int TILE = pad2(64 * US);                          // doubles per wave
    static constexpr int pow2(int v) { int p = 1; while (p < v) p *= 2; return p; }
    static constexpr int WU = pow2(CAND_TILE * m);                      // lanes that load one candidate's run
    static_assert(WU <= 64, "one run per pass of the wave");
    static constexpr int PASSES = WU;                                   // 64 candidates / (64 / WU) per pass
    static constexpr size_t lds_bytes(int waves) { return sizeof(double) * (size_t)(TH + waves * TILE); }
};

// GEN (ilqr_device_sample.hpp): the candidates are drawn where they are loaded here — the arguments are SampleArgs, a tile element
// comes from sample_u (found at instantiation) and is stored to u_out when the caller wants the candidates as drawn
template <bool GEN> struct CandArgsFor { typedef CandArgs type; };

template <class M, bool GEN = false>
__global__ __launch_bounds__(256) void candidates_score_kernel(typename CandArgsFor<GEN>::type a) {
    typedef CandDims<M> D;
    constexpr int n = M::NX, m = M::NU, NW = M::NW, ncs = M::NCS, nct = M::NCT;
    extern __shared__ __attribute__((aligned(16))) double cand_lds[];
    const Layout& L = a.L;
    const int T = L.T, N = T - 1, S = a.S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
    const int blocks = (S + nthreads - 1) / nthreads;
    const int b = blockIdx.x / blocks, s_wave = (blockIdx.x % blocks) * nthreads + 64 * wave;
    if (b >= a.B) return;
    // a lane behind the last candidate runs the last candidate again and stores nothing: every lane reaches every barrier
    const bool live = s_wave + lane < S;
    const int s = live ? s_wave + lane : S - 1;
    const size_t bs = (size_t)b * S + s;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    double* th = cand_lds;
    double* tu = cand_lds + D::TH + wave * D::TILE;
    // this lane's share of a tile load: component lu of the run of candidate (lane / WU + k · 64 / WU) of the wave, k < PASSES
    const int lu = lane % D::WU, r0 = lane / D::WU;
    double pre[D::PASSES];
    auto fetch = [&](int tb) {                                          // steps [tb, min(tb + CAND_TILE, N)) of the wave's candidates
        const int cu = ((N - tb) < CAND_TILE ? (N - tb) : CAND_TILE) * m;
#pragma unroll
        for (int k = 0; k < D::PASSES; ++k) {
            const int r = r0 + k * (64 / D::WU);
            const int sr = s_wave + r < S ? s_wave + r : S - 1;
            if constexpr (GEN) {
                pre[k] = lu < cu ? sample_u(a, b, sr, tb + lu / m, lu % m) : 0.0;
                if (a.u_out && lu < cu && s_wave + r < S) a.u_out[(((size_t)b * S + sr) * N + tb) * m + lu] = pre[k];
            } else {
                pre[k] = lu < cu ? a.u[(((size_t)b * S + sr) * N + tb) * m + lu] : 0.0;
            }
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int k = 0; k < D::PASSES; ++k)
            if (lu < CAND_TILE * m) tu[(r0 + k * (64 / D::WU)) * D::US + lu] = pre[k];
    };

    double xt[n];
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = a.x1[(size_t)b * n + i];
    double J = 0.0, viol = 0.0;
    int nf = -1;
    if (N > 0) fetch(0);

    for (int t0 = 0; t0 < T; t0 += CAND_CHUNK) {
        const int cnt = (T - t0) < CAND_CHUNK ? (T - t0) : CAND_CHUNK;
        if constexpr (NW > 0) {
            __syncthreads();                               // the previous chunk has been read by every wave
            for (int e = tid; e < cnt * NW; e += nthreads) th[e] = g[L.w + t0 * NW + e];
            __syncthreads();
        }
        for (int st = 0; st < cnt; ++st) {
            const int t = t0 + st, tq = t % CAND_TILE;
            if (tq == 0 && t < N) {
                policy_wave_sync();                        // the previous tile has been read by every lane
                park();
                policy_wave_sync();
                if (t + CAND_TILE < N) fetch(t + CAND_TILE);
            }
            bool fin = true;
#pragma unroll
            for (int i = 0; i < n; ++i) fin = fin && (fabs(xt[i]) < __builtin_huge_val());     // false for ±Inf and NaN
            nf = (nf < 0 && !fin) ? t : nf;
            double w[cdim<NW>::v];
            w[0] = 0.0;
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = th[st * NW + i];
            if (t < N) {
                double ut[m];
#pragma unroll
                for (int i = 0; i < m; ++i) ut[i] = tu[lane * D::US + tq * m + i];
                J += M::cost_s(xt, ut, w);
                if constexpr (ncs > 0) {
                    if (a.constrained) {
                        double cv[ncs];
                        M::con_s(xt, ut, w, cv);
                        viol = policy_violation<M, true, ncs>(viol, cv);
                    }
                }
                double y[n];
                M::dyn(xt, ut, w, y);
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
        }
    }
    if (live) {
        a.cost[bs] = J;
        a.viol[bs] = viol;
        a.nonfinite[bs] = nf;
    }
}

template <class M, bool GEN = false>
__global__ __launch_bounds__(64) void candidates_score_large_kernel(typename CandArgsFor<GEN>::type a) {
    constexpr int n = M::NX, m = M::NU, NW = M::NW, ncs = M::NCS, nct = M::NCT;
    __shared__ double sx[n], su[m], sw[cdim<NW>::v];
    const Layout& L = a.L;
    const int T = L.T, N = T - 1, S = a.S, lane = threadIdx.x;
    const int b = blockIdx.x / S, s = blockIdx.x % S;
    if (b >= a.B) return;
    const size_t bs = (size_t)b * S + s;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const double* us = a.u + bs * (size_t)N * m;
    // action `lane` of step t: loaded, or (GEN) drawn and, when the caller wants the candidates as drawn, stored
    auto action = [&](int t) {
        if constexpr (GEN) {
            const double v = sample_u(a, b, s, t, lane);
            if (a.u_out) a.u_out[(bs * (size_t)N + t) * m + lane] = v;
            return v;
        } else {
            return us[(size_t)t * m + lane];
        }
    };
    DynAff<M> aff;
    aff.init(lane);
    const int xrow = DynAff<M>::SPLIT ? (lane & 31) : lane;
    double xl = xrow < n ? a.x1[(size_t)b * n + xrow] : 0.0;
    double ul = (lane < m && N > 0) ? action(0) : 0.0;
    double J = 0.0, viol = 0.0;
    int nf = -1;
    if (lane == 0) sw[0] = 0.0;
    for (int t = 0; t < T; ++t) {
        if (lane < n) sx[lane] = xl;
        if (lane < m) su[lane] = ul;
        for (int i = lane; i < NW; i += 64) sw[i] = g[L.w + t * NW + i];
        wave_lds_fence();
        policy_wave_sync();
        const double u_next = (lane < m && t + 1 < N) ? action(t + 1) : 0.0;
        double xa[n], w[cdim<NW>::v];
        bool fin = true;
#pragma unroll
        for (int j = 0; j < n; ++j) { xa[j] = sx[j]; fin = fin && (fabs(xa[j]) < __builtin_huge_val()); }
#pragma unroll
        for (int i = 0; i < cdim<NW>::v; ++i) w[i] = sw[i];
        nf = (nf < 0 && !fin) ? t : nf;
        if (t < N) {
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
            xl = dyn_row<M>(aff, sx, ua, xl, lane, sw, 0);
            ul = u_next;
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
        a.viol[bs] = viol;
        a.nonfinite[bs] = nf;
    }
}

// (eligible first, score, index): a total order, so the reduction's result does not depend on how it is bracketed. The three
// words travel as separate scalars (a struct of them goes through scratch).
__device__ __forceinline__ void cand_take_better(int& ok, double& score, int& idx, int qok, double qscore, int qidx) {
    const bool take = qok > ok || (qok == ok && (qscore < score || (qscore == score && qidx < idx)));
    ok = take ? qok : ok;
    score = take ? qscore : score;
    idx = take ? qidx : idx;
}

// score of candidate bs = b · S + s; false: not eligible
__device__ __forceinline__ bool cand_score(const CandArgs& a, size_t bs, double& sc) {
    const double c = a.cost[bs];
    sc = a.weight == 0.0 ? c : __dadd_rn(c, __dmul_rn(a.weight, a.viol[bs]));
    return (fabs(sc) < __builtin_huge_val()) && a.nonfinite[bs] == -1;
}

// The best candidate of instance b under that order, by a workgroup of CAND_SELECT_THREADS threads (every thread calls it and gets
// the result): ok = 0 when nobody is eligible.
__device__ __forceinline__ void cand_best(const CandArgs& a, int b, int& ok, double& score, int& idx) {
    constexpr int W = CAND_SELECT_THREADS / 64;
    __shared__ int part_ok[W], part_idx[W];
    __shared__ double part_score[W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = a.S;
    // an ineligible candidate carries score +Inf: the order never compares a NaN
    ok = 0; idx = 0x7fffffff;
    score = __builtin_huge_val();
    for (int s = tid; s < S; s += CAND_SELECT_THREADS) {
        double sc;
        const bool el = cand_score(a, (size_t)b * S + s, sc);
        cand_take_better(ok, score, idx, el ? 1 : 0, el ? sc : __builtin_huge_val(), s);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int qok = __shfl_xor(ok, d), qidx = __shfl_xor(idx, d);
        const double qscore = __shfl_xor(score, d);
        cand_take_better(ok, score, idx, qok, qscore, qidx);
    }
    if (lane == 0) { part_ok[wave] = ok; part_score[wave] = score; part_idx[wave] = idx; }
    __syncthreads();
    ok = part_ok[0]; score = part_score[0]; idx = part_idx[0];
#pragma unroll
    for (int v = 1; v < W; ++v) cand_take_better(ok, score, idx, part_ok[v], part_score[v], part_idx[v]);
}

// One workgroup per instance. Templated on the model only so that every module carries its own copy (the kernel reads nothing
// of M but the dimensions).
template <class M>
__global__ __launch_bounds__(CAND_SELECT_THREADS) void candidates_select_kernel(CandArgs a) {
    constexpr int n = M::NX, m = M::NU;
    const int b = blockIdx.x, tid = threadIdx.x, S = a.S, N = a.L.T - 1;
    if (b >= a.B) return;
    int ok, idx;
    double score;
    cand_best(a, b, ok, score, idx);
    const int win = ok ? idx : 0;                 // nobody eligible: candidate 0, so the handle's state is defined
    const double* src = a.u + ((size_t)b * S + win) * (size_t)N * m;
    double* dst = a.r_u + (size_t)b * N * m;
    for (int e = tid; e < N * m; e += CAND_SELECT_THREADS) dst[e] = src[e];
    if (a.r_x1 != a.x1 && tid < n) a.r_x1[(size_t)b * n + tid] = a.x1[(size_t)b * n + tid];
    if (tid == 0 && a.chosen) a.chosen[b] = ok ? idx : -1;
}

template <class M>
int launch_candidates(const CandArgs* a, void* stream) {
    if (a->B < 1 || a->S < 1) return -1;
    static_assert(M::NX <= CAND_SELECT_THREADS, "x1 is copied by one pass of the select workgroup");
    if constexpr (is_large<M>::value) {
        const size_t grid = (size_t)a->B * (size_t)a->S;
        if (grid > 0x7fffffffull) return -1;
        hipLaunchKernelGGL(candidates_score_large_kernel<M>, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, *a);
    } else {
        const int waves = a->waves < 1 ? 1 : (a->waves > 4 ? 4 : a->waves), nthreads = 64 * waves;
        const size_t grid = (size_t)a->B * (size_t)((a->S + nthreads - 1) / nthreads);
        if (grid > 0x7fffffffull) return -1;
        const size_t lds = CandDims<M>::lds_bytes(waves);
        auto kernel = candidates_score_kernel<M>;
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
        CandArgs q = *a;
        q.waves = waves;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(nthreads), lds, (hipStream_t)stream, q);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(candidates_select_kernel<M>, dim3((unsigned)a->B), dim3(CAND_SELECT_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
