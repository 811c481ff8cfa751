// Candidate initial guesses drawn on the device (ilqr_sample_rollout_candidates, include/ilqr_hip.h): candidate 0 of instance b is
// the base sequence itself, candidate s >= 1 is
//
//   u[b][s][t][j] = base[b][t][j] + sigma[j] · z(seed, b0 + b, s, t, j)          (product and sum rounded separately)
//   z:  key = seed ^ (b·2^40 + s·2^24 + t·2^4 + j),  h1 = splitmix64(key),  h2 = splitmix64(h1),
//       U(h) = ((h >> 11) + 0.5) / 2^53,  z = sqrt(−2 · log(U(h1))) · cos(6.283185307179586 · U(h2))
//
// the mix, U and the Box-Muller form of ilqr_synthetic_inputs with a key that also carries the candidate. The key's bit fields are
// disjoint for j < 16, t < 2^20, s < 2^16, b < 2^23 (the entry points refuse anything beyond). sample_z is the ONLY place that
// evaluates z on the device — the scoring kernels, the export and the installation call it through sample_u, so the winner that
// is regenerated at installation is bit for bit the one that was scored; ilqr_candidate_noise is its host twin (same integers,
// libm's log / sqrt / cos: a few ulp apart).
//
// Scoring: candidates_score_kernel / candidates_score_large_kernel (ilqr_device_candidates.hpp) instantiated with GEN = true: a
// lane draws in `fetch` exactly the tile elements it loads there otherwise (large models: lanes < nu draw u_next) and, when the
// caller wants the candidates, stores them — the contiguous runs it would have loaded. Cost, violation and non-finite arithmetic
// are the one piece of code both instantiations run.
//
// sample_weights_kernel: one workgroup of CAND_SELECT_THREADS per instance. cand_best gives the argmin (chosen[b], −1 when nobody is
// eligible). Blend: w_s = exp(−(score_s − score_min) / temperature) for eligible s, 0 otherwise, divided by their sum. ORDER OF
// THAT SUM: thread i adds its candidates i, i + 256, i + 512, .. in ascending s; the 256 partial sums are then combined by a
// fixed binary tree through LDS (partial[i] += partial[i + d], d = 128, 64, .. 1). No atomics: the sum does not depend on timing.
// Pick: w = 1 at the winner, 0 elsewhere (written only when the caller wants the weights).
//
// sample_install_kernel: one thread per (t, j) of an instance writes the resident ū — pick: sample_u of the winner (the base for
// winner 0 or chosen == −1); blend: base + sigma_j · (Σ_s w_s · z(b, s, t, j)), s ascending, every product and sum rounded
// separately, candidates of weight 0 skipped (the base when chosen == −1). Elementwise read-then-write: the base may be the resident
// buffer itself. The existing init_rollout kernels then install (x1, ū).
#pragma once

#include <stdint.h>

namespace ilqr {

enum { SAMPLE_PICK = 0, SAMPLE_BLEND = 1, SAMPLE_MAX_NU = 16, SAMPLE_MAX_CANDIDATES = 1 << 16, SAMPLE_MAX_STEPS = 1 << 20,
       SAMPLE_MAX_INSTANCES = 1 << 23, SAMPLE_INSTALL_THREADS = 256 };

struct SampleArgs : CandArgs {          // CandArgs::u is unused (null); chosen is never null here
    uint64_t seed;
    long long b0;            // global index of the handle's instance 0
    const double* sigma;     // [nu] (device)
    const double* base;      // [B][T-1][nu]; may be r_u itself
    double* u_out;           // null, or [B][S][T-1][nu]
    double* weights;         // [B][S]; pick: may be null
    int mode;                // SAMPLE_PICK / SAMPLE_BLEND
    double temperature;
};
template <> struct CandArgsFor<true> { typedef SampleArgs type; };

ILQR_HD uint64_t sample_mix(uint64_t z) {                                // splitmix64
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
ILQR_HD uint64_t sample_key(uint64_t seed, long long b, int s, int t, int j) {
    return seed ^ ((uint64_t)b << 40 | (uint64_t)s << 24 | (uint64_t)t << 4 | (uint64_t)j);      // disjoint fields: the sum is the or
}
ILQR_HD double sample_unif(uint64_t h) { return ((double)(h >> 11) + 0.5) * 0x1.0p-53; }         // (0, 1)

// IEEE sqrt, the device library's log, cos_fast (ilqr_math.hpp: 1.4 ulp; the argument lies in (0, 2π))
__device__ __forceinline__ double sample_z(uint64_t seed, long long b, int s, int t, int j) {
    const uint64_t h1 = sample_mix(sample_key(seed, b, s, t, j)), h2 = sample_mix(h1);
    const double r = __dsqrt_rn(__dmul_rn(-2.0, log(sample_unif(h1))));
    return __dmul_rn(r, cos_fast(__dmul_rn(6.283185307179586, sample_unif(h2))));
}

// u[b][s][t][j] as drawn; b: the instance inside the handle
__device__ __forceinline__ double sample_u(const SampleArgs& a, int b, int s, int t, int j) {
    const double base = a.base[((size_t)b * (size_t)(a.L.T - 1) + t) * a.L.nu + j];
    const double v = __dadd_rn(base, __dmul_rn(a.sigma[j], sample_z(a.seed, a.b0 + b, s, t, j)));
    return s == 0 ? base : v;
}

// Templated on the model only so that every module carries its own copy.
template <class M>
__global__ __launch_bounds__(CAND_SELECT_THREADS) void sample_weights_kernel(SampleArgs a) {
    __shared__ double partial[CAND_SELECT_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x, S = a.S;
    if (b >= a.B) return;
    int ok, idx;
    double best;
    cand_best(a, b, ok, best, idx);
    if (tid == 0) a.chosen[b] = ok ? idx : -1;
    if (!a.weights) return;
    double* w = a.weights + (size_t)b * S;
    if (a.mode == SAMPLE_PICK) {
        for (int s = tid; s < S; s += CAND_SELECT_THREADS) w[s] = (ok && s == idx) ? 1.0 : 0.0;
        return;
    }
    double acc = 0.0;
    for (int s = tid; s < S; s += CAND_SELECT_THREADS) {
        double sc;
        const bool el = cand_score(a, (size_t)b * S + s, sc);
        const double v = el ? exp(__ddiv_rn(-__dsub_rn(sc, best), a.temperature)) : 0.0;
        w[s] = v;
        acc = __dadd_rn(acc, v);
    }
    partial[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int d = CAND_SELECT_THREADS / 2; d >= 1; d >>= 1) {
        if (tid < d) partial[tid] = __dadd_rn(partial[tid], partial[tid + d]);
        __syncthreads();
    }
    const double total = partial[0];                                     // >= 1 when somebody is eligible: the winner's weight is exp(0)
    for (int s = tid; s < S; s += CAND_SELECT_THREADS) w[s] = ok ? __ddiv_rn(w[s], total) : 0.0;    // a thread reads back its own stores
}

template <class M>
__global__ __launch_bounds__(SAMPLE_INSTALL_THREADS) void sample_install_kernel(SampleArgs a) {
    constexpr int n = M::NX, m = M::NU;
    const int N = a.L.T - 1, S = a.S, tid = threadIdx.x;
    const int per = (N * m + SAMPLE_INSTALL_THREADS - 1) / SAMPLE_INSTALL_THREADS;      // workgroups per instance (>= 1: T >= 2)
    const int b = blockIdx.x / per, e = (blockIdx.x % per) * SAMPLE_INSTALL_THREADS + tid;
    if (b >= a.B) return;
    if (blockIdx.x % per == 0 && a.r_x1 != a.x1 && tid < n) a.r_x1[(size_t)b * n + tid] = a.x1[(size_t)b * n + tid];
    if (e >= N * m) return;
    const int t = e / m, j = e % m, win = a.chosen[b];
    const size_t o = (size_t)b * (size_t)(N * m) + e;
    double v = a.base[o];
    if (a.mode == SAMPLE_PICK) {
        if (win > 0) v = sample_u(a, b, win, t, j);
    } else if (win >= 0) {
        const double* w = a.weights + (size_t)b * S;
        double acc = 0.0;
        for (int s = 1; s < S; ++s) {                                    // (z of candidate 0 is 0)
            const double ws = w[s];                                      // the same on every lane of the workgroup
            if (ws != 0.0) acc = __dadd_rn(acc, __dmul_rn(ws, sample_z(a.seed, a.b0 + b, s, t, j)));
        }
        v = __dadd_rn(v, __dmul_rn(a.sigma[j], acc));
    }
    a.r_u[o] = v;
}

// scoring with the candidates drawn in place, the weights, the installation into the resident inputs
template <class M>
int launch_sample_candidates(const SampleArgs* a, void* stream) {
    if (a->B < 1 || a->S < 1 || a->S > SAMPLE_MAX_CANDIDATES || M::NU > SAMPLE_MAX_NU || a->L.T - 1 > SAMPLE_MAX_STEPS) return -1;
    if (!a->chosen || !a->sigma || !a->base || (a->mode == SAMPLE_BLEND && !a->weights)) return -1;
    static_assert(M::NX <= SAMPLE_INSTALL_THREADS, "x1 is copied by one pass of an install workgroup");
    if constexpr (is_large<M>::value) {
        const size_t grid = (size_t)a->B * (size_t)a->S;
        if (grid > 0x7fffffffull) return -1;
        hipLaunchKernelGGL((candidates_score_large_kernel<M, true>), dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, *a);
    } else {
        const int waves = a->waves < 1 ? 1 : (a->waves > 4 ? 4 : a->waves), nthreads = 64 * waves;
        const size_t grid = (size_t)a->B * (size_t)((a->S + nthreads - 1) / nthreads);
        if (grid > 0x7fffffffull) return -1;
        const size_t lds = CandDims<M>::lds_bytes(waves);
        auto kernel = candidates_score_kernel<M, true>;
        if (lds > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
        SampleArgs q = *a;
        q.waves = waves;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(nthreads), lds, (hipStream_t)stream, q);
    }
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(sample_weights_kernel<M>, dim3((unsigned)a->B), dim3(CAND_SELECT_THREADS), 0, (hipStream_t)stream, *a);
    if (hipGetLastError() != hipSuccess) return -1;
    const size_t per = ((size_t)(a->L.T - 1) * M::NU + SAMPLE_INSTALL_THREADS - 1) / SAMPLE_INSTALL_THREADS;
    if (per * (size_t)a->B > 0x7fffffffull) return -1;
    hipLaunchKernelGGL(sample_install_kernel<M>, dim3((unsigned)(per * (size_t)a->B)), dim3(SAMPLE_INSTALL_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
