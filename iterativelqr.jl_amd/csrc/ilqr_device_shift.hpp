// Receding-horizon shift of a solved handle (ilqr_shift_horizon, include/ilqr_hip.h): with k = steps, N = T − 1 and x̄, ū, K, θ as
// the workspace holds them,
//
//   x1' = x1[b]  or  x̄_k          θ'_t = θ_{t+k}  (t + k <= T−1),  then w_tail[b][t − (T−k)]  or  θ_{T−1}
//   open loop:    u'_t = ū_{t+k}  (t < N−k),  then ū_{N−1} (hold) or 0 (zero)
//   closed loop:  x'_0 = x1',  u'_t = ū_{t+k} + K_{t+k} (x'_t − x̄_{t+k}),  x'_{t+1} = f(x'_t, u'_t, θ'_t)  (t < N−k), tail as above
//
// (src/rollout.jl:24-28 in the order policy_rollout_kernel forms it with α = 0: (ū + K x') − K x̄). The kernels READ the
// workspace's x̄, ū, K and write (x1', u') to the handle's resident input buffers, from which the existing init_rollout kernels
// install them; the only workspace range written here is θ.
//
// θ is shifted in place, row t from row t + k of the same instance block: a parallel copy would race. shift_copy_kernel therefore
// writes θ' of the whole batch to a staging buffer of the handle (phase 0, together with x1' and the copied actions) and a
// second launch of it copies the staging buffer back (phase 1): every word of θ is read before the launch that overwrites it.
//
// shift_copy_kernel: one workgroup per instance, lanes along the instance's contiguous rows.
// shift_feedback_kernel (nx, nu <= 4): ONE INSTANCE PER LANE as init_rollout_kernel, the state in registers over the horizon, no
// cross-lane arithmetic: an instance's numbers do not depend on B or on its neighbours. Each lane reads ū, K, x̄ and θ' from its
// own block (strided by Layout::stride between lanes).
// shift_feedback_large_kernel: ONE WAVE PER INSTANCE as policy_rollout_large_kernel (DynAff / dyn_row, row i of K_{t+k} on lane
// i, x and u through LDS).
#pragma once

namespace ilqr {

struct ShiftArgs {
    double* ws;              // the handle's workspace: x̄, ū, K are read, θ is rewritten
    Layout L;
    int B;
    int steps;               // k, 0 .. T-1
    int tail;                // 0 hold, 1 zero (ILQR_SHIFT_TAIL_*)
    int feedback;            // closed loop: the copy kernel leaves u'_t, t < N − k, to the feedback kernel
    int phase;               // shift_copy_kernel: 0 = x1', u', θ' -> staging; 1 = staging -> θ
    const double* x1;        // null, or [B][nx]
    const double* w_tail;    // null, or rows of nw doubles: row (b · w_tail_ld + w_tail_row0 + j), j = 0 .. steps-1
    double* w_stage;         // null (θ stays), or [B][T][nw]
    double* r_x1;            // the handle's resident inputs: [B][nx]
    double* r_u;             //                               [B][T-1][nu]
    long long w_tail_ld, w_tail_row0;   // ilqr_shift_horizon: steps, 0; ilqr_mpc_run_preview: the run's P·k rows, p·k
};

enum { SHIFT_COPY_THREADS = 128 };

// Templated on the model only so that every module carries its own copy (the kernel reads nothing of M: the Layout has it all).
template <class M>
__global__ __launch_bounds__(SHIFT_COPY_THREADS) void shift_copy_kernel(ShiftArgs a) {
    const Layout& L = a.L;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= a.B) return;
    const int T = L.T, N = T - 1, n = L.nx, m = L.nu, nw = L.nw, k = a.steps;
    double* g = a.ws + (size_t)b * (size_t)L.stride;
    if (a.phase != 0) {
        const double* st = a.w_stage + (size_t)b * (size_t)(T * nw);
        for (int e = tid; e < T * nw; e += SHIFT_COPY_THREADS) g[L.w + e] = st[e];
        return;
    }
    const int head = (N - k) * m;                          // actions that have a source k steps later
    double* u = a.r_u + (size_t)b * (size_t)(N * m);
    for (int e = (a.feedback ? head : 0) + tid; e < N * m; e += SHIFT_COPY_THREADS)
        u[e] = e < head ? g[L.ub + e + k * m] : (a.tail == 0 ? g[L.ub + (N - 1) * m + e % m] : 0.0);
    if (tid < n) a.r_x1[(size_t)b * n + tid] = a.x1 ? a.x1[(size_t)b * n + tid] : g[L.xb + k * n + tid];
    if (a.w_stage) {
        double* st = a.w_stage + (size_t)b * (size_t)(T * nw);
        const int kept = (T - k) * nw;                     // rows that have a source k steps later
        const double* wt = a.w_tail ? a.w_tail + ((size_t)b * (size_t)a.w_tail_ld + (size_t)a.w_tail_row0) * (size_t)nw : nullptr;
        for (int e = tid; e < T * nw; e += SHIFT_COPY_THREADS)
            st[e] = e < kept ? g[L.w + e + k * nw] : (wt ? wt[e - kept] : g[L.w + (T - 1) * nw + e % nw]);
    }
}

template <class M>
__global__ __launch_bounds__(64) void shift_feedback_kernel(ShiftArgs a) {
    constexpr int n = M::NX, m = M::NU, KN = m * n;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const int N = L.T - 1, k = a.steps, H = N - k;
    double* u = a.r_u + (size_t)b * (size_t)(N * m);
    double xt[n];
#pragma unroll
    for (int i = 0; i < n; ++i) xt[i] = a.r_x1[(size_t)b * n + i];
    for (int t = 0; t < H; ++t) {
        const int s = t + k;
        const double* Ks = g + L.K + s * KN;
        double ut[m], y[n];
#pragma unroll
        for (int i = 0; i < m; ++i) {
            double kx = 0.0, kb = 0.0;
#pragma unroll
            for (int j = 0; j < n; ++j) { kx = fma(Ks[j * m + i], xt[j], kx); kb = fma(Ks[j * m + i], g[L.xb + s * n + j], kb); }
            ut[i] = (g[L.ub + s * m + i] + kx) - kb;                                           // (:24-28), α = 0
            u[t * m + i] = ut[i];
        }
        double w[cdim<M::NW>::v];
        load_w<M::NW>(g + L.w, t, w);                                                          // θ'_t: already shifted
        M::dyn(xt, ut, w, y);                                                                  // (:29)
#pragma unroll
        for (int i = 0; i < n; ++i) xt[i] = y[i];
    }
}

template <class M>
__global__ __launch_bounds__(64) void shift_feedback_large_kernel(ShiftArgs a) {
    constexpr int n = M::NX, m = M::NU, KN = m * n;
    __shared__ double sx[n], su[m];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    const double* g = a.ws + (size_t)b * (size_t)L.stride;
    const int N = L.T - 1, k = a.steps, H = N - k;
    double* u = a.r_u + (size_t)b * (size_t)(N * m);
    DynAff<M> aff;
    aff.init(lane);
    const int xrow = DynAff<M>::SPLIT ? (lane & 31) : lane;
    double xl = xrow < n ? a.r_x1[(size_t)b * n + xrow] : 0.0;
    for (int t = 0; t < H; ++t) {
        const int s = t + k;
        if (lane < n) sx[lane] = xl;
        wave_lds_fence();
        policy_wave_sync();
        if (lane < m) {                                                       // row `lane` of K_{t+k}
            const double* Ks = g + L.K + s * KN;
            double kx = 0.0, kb = 0.0;
#pragma unroll
            for (int j = 0; j < n; ++j) { kx = fma(Ks[j * m + lane], sx[j], kx); kb = fma(Ks[j * m + lane], g[L.xb + s * n + j], kb); }
            const double v = (g[L.ub + s * m + lane] + kx) - kb;              // (:24-28), α = 0
            su[lane] = v;
            u[t * m + lane] = v;
        }
        wave_lds_fence();
        policy_wave_sync();
        double ua[m];
#pragma unroll
        for (int j = 0; j < m; ++j) ua[j] = su[j];
        xl = dyn_row<M>(aff, sx, ua, xl, lane, g + L.w, t);                   // (:29), θ'_t: already shifted
        wave_lds_fence();
        policy_wave_sync();                                                   // sx, su are rewritten by the next step
    }
}

// phase 0 and, when θ moves, phase 1 of the copy kernel; then the feedback kernel over the head of the horizon
template <class M>
int launch_shift(const ShiftArgs* a, void* stream) {
    if (a->B < 1 || a->steps < 0 || a->steps > a->L.T - 1) return -1;
    static_assert(M::NX <= SHIFT_COPY_THREADS, "x1' is written by one pass of the copy workgroup");
    ShiftArgs q = *a;
    q.phase = 0;
    hipLaunchKernelGGL(shift_copy_kernel<M>, dim3((unsigned)q.B), dim3(SHIFT_COPY_THREADS), 0, (hipStream_t)stream, q);
    if (hipGetLastError() != hipSuccess) return -1;
    if (q.w_stage) {
        q.phase = 1;
        hipLaunchKernelGGL(shift_copy_kernel<M>, dim3((unsigned)q.B), dim3(SHIFT_COPY_THREADS), 0, (hipStream_t)stream, q);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    if (q.feedback && q.L.T - 1 - q.steps > 0) {
        if constexpr (is_large<M>::value)
            hipLaunchKernelGGL(shift_feedback_large_kernel<M>, dim3((unsigned)q.B), dim3(64), 0, (hipStream_t)stream, q);
        else
            hipLaunchKernelGGL(shift_feedback_kernel<M>, dim3((unsigned)((q.B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, q);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

}  // namespace ilqr
