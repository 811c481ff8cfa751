// A linear sensor y = H x + v, v ~ N(0, diag(r)), with ny outputs for the device Kalman filter and the MPC loop
// (ilqr_estimate_update_linear, ilqr_plant_measure_linear, ilqr_mpc_run_sensor, include/ilqr_hip.h). ny may be smaller or larger
// than nx (<= 64); H [ny][nx] row-major is shared by the batch (h_stride 0) or per instance (h_stride ny · nx).
//
// MEASUREMENT UPDATE. With x̂₀ the estimate on entry and h_j row j of H: c_j = 0, or with ŷ given c_j = ŷ_j − h_j·x̂₀ (ŷ is then the
// caller's h(x̂₀) of a nonlinear sensor, linearised once at the prior). For j = 0 .. ny−1 in increasing order, on the x̂ and P the
// previous j left:
//
//   d = P h_jᵀ (nx FMA chains over the ascending column index from +0),  s = h_j·d + r_j,  ν = (y_j − c_j) − h_j·x̂
//   s not a finite number > 0 (est_pivot_ok): the row is skipped, first_bad = the first such j (else −1)
//   g = d / s;  x̂ ← x̂ + g ν;  P_ab ← P_ab − g_a d_b for a >= b from d as it was, then mirrored: exactly symmetric
//   nis = Σ ν² / s over the updated rows; innovation[j] = ν, or 0 where the row was skipped
//
// MEASUREMENT. y[b][j] = Σ_k H_jk x[b][k], one FMA chain over ascending k from +0, then  + sigma[j] · z(seed, b0 + b, 5 + j / 16, step,
// j % 16)  where sigma[j] != 0 (product and sum rounded separately): the key fields of plant_measure_kernel. A run uses one kind of
// measurement or the other, so the two share the stream on purpose.
//
// H, r, sigma, y and ŷ are HBM pointers: nothing of length ny is indexed at run time out of the argument segment. The kernels read and
// write only the caller's arrays, each element by the lane (wave) that owns the instance. No atomics, no cross-instance traffic, plain
// vector stores; every sum runs in an order fixed by the model's sizes and ny alone.
//
// sensor_update_kernel (nx, nu <= 4): ONE INSTANCE PER LANE as estimate_update_kernel; x̂, x̂₀ and P in registers for the whole call
// (read from HBM once, written once), a runtime loop over the rows; per row the lane reads h_j (compile-time indexed), r_j, y_j, ŷ_j
// from HBM — with a shared H every lane of the wave the same words. A skipped row is a per-lane branch.
// sensor_update_large_kernel: ONE WAVE PER INSTANCE as estimate_update_large_kernel, lane a owns row a of P (LDS, odd row pitch
// EstDims::uld). y, r and ŷ go to LDS once (lane j its entry); per row lane a loads h_j[a] (consecutive doubles across the wave) and
// puts it and x̂_a into LDS, forms d_a reading its row of P through the mirror P(c, a) (consecutive doubles across lanes), and every
// lane evaluates s, h_j·x̂ and h_j·x̂₀ from LDS in the same fixed order, so the branch on a bad pivot is uniform.
// plant_measure_linear_kernel: one lane per (instance, output), neighbouring lanes store neighbouring doubles.
#pragma once

#include <stdint.h>

namespace ilqr {

enum { SENSOR_MAX_NY = 64 };

struct SensorArgs {
    int B;
    int ny;                  // 1 .. SENSOR_MAX_NY
    long long h_stride;      // doubles between two instances' H: 0 (shared) or ny · nx
    const double* H;         // [ny][nx], or [B][ny][nx]
    const double* r;         // update: [ny]
    const double* y;         // update: [B][ny]
    const double* yhat;      // update: null, or [B][ny]
    double* xhat;            // update: [B][nx] in / out
    double* P;               // update: [B][nx][nx] in / out
    double* innovation;      // update: null, or [B][ny]
    double* nis;             // update: null, or [B]
    int* first_bad;          // update: null, or [B]
    // the measurement
    int step;                // plant steps taken when the measurement is made
    uint64_t seed;
    long long b0;            // global index of the handle's instance 0
    const double* sigma;     // null, or [ny]
    const double* x;         // [B][nx]
    double* y_out;           // [B][ny]
};
static_assert(sizeof(SensorArgs) <= 4096, "the kernel argument segment");

template <class M>
__global__ __launch_bounds__(64) void sensor_update_kernel(SensorArgs a) {
    constexpr int n = M::NX;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double* Pg = a.P + (size_t)b * n * n;
    const double* Hb = a.H + (size_t)b * (size_t)a.h_stride;
    const size_t row0 = (size_t)b * (size_t)a.ny;
    double xt[n], x0[n], P[n * n];
#pragma unroll
    for (int i = 0; i < n; ++i) x0[i] = xt[i] = a.xhat[(size_t)b * n + i];
#pragma unroll
    for (int i = 0; i < n * n; ++i) P[i] = Pg[i];
    double nis = 0.0;
    int bad = -1;
    for (int j = 0; j < a.ny; ++j) {
        double h[n], d[n];
#pragma unroll
        for (int c = 0; c < n; ++c) h[c] = Hb[(size_t)j * n + c];
        double s = 0.0, hx = 0.0, cj = 0.0;
#pragma unroll
        for (int r = 0; r < n; ++r) {
            double t = 0.0;
#pragma unroll
            for (int c = 0; c < n; ++c) t = fma(P[r * n + c], h[c], t);
            d[r] = t;
        }
#pragma unroll
        for (int c = 0; c < n; ++c) { s = fma(h[c], d[c], s); hx = fma(h[c], xt[c], hx); }
        s = s + a.r[j];
        if (a.yhat) {                                                                          // (the same branch on every lane)
            double h0 = 0.0;
#pragma unroll
            for (int c = 0; c < n; ++c) h0 = fma(h[c], x0[c], h0);
            cj = a.yhat[row0 + j] - h0;
        }
        const double nu = (a.y[row0 + j] - cj) - hx;
        const bool ok = est_pivot_ok(s);
        if (ok) {
            double gn[n];
#pragma unroll
            for (int c = 0; c < n; ++c) gn[c] = d[c] / s;
#pragma unroll
            for (int r = 0; r < n; ++r) {
                xt[r] = xt[r] + gn[r] * nu;
#pragma unroll
                for (int c = 0; c <= r; ++c) {
                    const double v = P[r * n + c] - gn[r] * d[c];
                    P[r * n + c] = v;
                    P[c * n + r] = v;
                }
            }
            nis += nu * nu / s;
        } else {
            bad = bad < 0 ? j : bad;
        }
        if (a.innovation) a.innovation[row0 + j] = ok ? nu : 0.0;
    }
#pragma unroll
    for (int i = 0; i < n; ++i) a.xhat[(size_t)b * n + i] = xt[i];
#pragma unroll
    for (int i = 0; i < n * n; ++i) Pg[i] = P[i];
    if (a.nis) a.nis[b] = nis;
    if (a.first_bad) a.first_bad[b] = bad;
}

// LDS of the large kernel: estimate_update_large_kernel's (P with row pitch uld, then four 64-double vectors: here x̂, h_j, x̂₀ and
// d) plus y, r and ŷ
template <class M>
struct SensorDims {
    typedef EstDims<M> D;
    static constexpr int sY = D::utotal, sR = sY + 64, sYh = sR + 64, total = sYh + 64;
    static constexpr size_t bytes = sizeof(double) * (size_t)total;
};

template <class M>
__global__ __launch_bounds__(64) void sensor_update_large_kernel(SensorArgs a) {
    typedef EstDims<M> D;
    typedef SensorDims<M> S;
    constexpr int n = M::NX, ld = D::uld;
    static_assert(n <= PLANT_MAX_NX, "one row of P per lane");
    extern __shared__ __attribute__((aligned(16))) double est_lds[];
    double *sP = est_lds, *sx = est_lds + D::uX, *sh = est_lds + D::uY, *sx0 = est_lds + D::uR, *sd = est_lds + D::uRow, *sy = est_lds + S::sY,
           *sr = est_lds + S::sR, *syh = est_lds + S::sYh;
    const int b = blockIdx.x, lane = threadIdx.x, ny = a.ny;
    if (b >= a.B) return;
    double* Pg = a.P + (size_t)b * n * n;
    const double* Hb = a.H + (size_t)b * (size_t)a.h_stride;
    const size_t row0 = (size_t)b * (size_t)ny;
    const bool lin = a.yhat != nullptr;                                       // (uniform)
    double xl = lane < n ? a.xhat[(size_t)b * n + lane] : 0.0;
    for (int e = lane; e < n * n; e += 64) sP[(e / n) * ld + e % n] = Pg[e];
    sx0[lane] = xl;
    sy[lane] = lane < ny ? a.y[row0 + lane] : 0.0;
    sr[lane] = lane < ny ? a.r[lane] : 0.0;
    syh[lane] = lin && lane < ny ? a.yhat[row0 + lane] : 0.0;
    double nis = 0.0, inn = 0.0;                                              // inn: ν of row `lane`
    int bad = -1;
    double hl = lane < n ? Hb[lane] : 0.0;                                    // h_0[a]
    for (int j = 0; j < ny; ++j) {
        sh[lane] = hl;
        sx[lane] = xl;
        if (j + 1 < ny) hl = lane < n ? Hb[(size_t)(j + 1) * n + lane] : 0.0;     // the next row is on its way while this one is worked on
        wave_lds_fence();
        policy_wave_sync();
        double dl = 0.0;                                                      // d_a = Σ_c P(a, c) h_c, P(a, c) read at its mirror (c, a)
        if (lane < n) {
#pragma unroll 8
            for (int c = 0; c < n; ++c) dl = fma(sP[c * ld + lane], sh[c], dl);
        }
        sd[lane] = dl;
        wave_lds_fence();
        policy_wave_sync();
        double s = 0.0, hx = 0.0, cj = 0.0;                                   // (uniform: every lane reads the same words in the same order)
#pragma unroll 8
        for (int c = 0; c < n; ++c) { s = fma(sh[c], sd[c], s); hx = fma(sh[c], sx[c], hx); }
        s = s + sr[j];
        if (lin) {
            double h0 = 0.0;
#pragma unroll 8
            for (int c = 0; c < n; ++c) h0 = fma(sh[c], sx0[c], h0);
            cj = syh[j] - h0;
        }
        const double nu = (sy[j] - cj) - hx;
        if (est_pivot_ok(s)) {
            const double gn = dl / s;
            xl = xl + gn * nu;
            if (lane < n)
                for (int c = 0; c <= lane; ++c) {                             // element (a, c), c <= a, read at its mirror (c, a)
                    const double v = sP[c * ld + lane] - gn * sd[c];
                    sP[c * ld + lane] = v;
                    sP[lane * ld + c] = v;
                }
            nis += nu * nu / s;
            inn = lane == j ? nu : inn;
        } else {
            bad = bad < 0 ? j : bad;
        }
        wave_lds_fence();
        policy_wave_sync();                                                   // sh, sx and sd are rewritten by the next row
    }
    if (lane < n) a.xhat[(size_t)b * n + lane] = xl;
    if (lane < ny && a.innovation) a.innovation[row0 + lane] = inn;
    for (int e = lane; e < n * n; e += 64) Pg[e] = sP[(e / n) * ld + e % n];
    if (lane == 0 && a.nis) a.nis[b] = nis;
    if (lane == 0 && a.first_bad) a.first_bad[b] = bad;
}

template <class M>
__global__ __launch_bounds__(PLANT_MEASURE_THREADS) void plant_measure_linear_kernel(SensorArgs a) {
    constexpr int n = M::NX;
    const size_t e = (size_t)blockIdx.x * PLANT_MEASURE_THREADS + threadIdx.x;
    if (e >= (size_t)a.B * (size_t)a.ny) return;
    const int b = (int)(e / (size_t)a.ny), j = (int)(e % (size_t)a.ny);
    const double* hj = a.H + (size_t)b * (size_t)a.h_stride + (size_t)j * n;
    const double* xb = a.x + (size_t)b * n;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < n; ++k) v = fma(hj[k], xb[k], v);
    if (a.sigma) {
        const double sg = a.sigma[j];
        if (sg != 0.0) v = __dadd_rn(v, __dmul_rn(sg, sample_z(a.seed, a.b0 + b, PLANT_MEASURE_FIELD0 + j / 16, a.step, j % 16)));
    }
    a.y_out[e] = v;
}

template <class M>
int launch_sensor_update(const SensorArgs* a, void* stream) {
    if (a->B < 1 || a->ny < 1 || a->ny > SENSOR_MAX_NY || !a->H || !a->r || !a->y || !a->xhat || !a->P || M::NX > PLANT_MAX_NX ||
        (a->h_stride != 0 && a->h_stride != (long long)a->ny * M::NX)) return -1;
    if constexpr (is_large<M>::value) {
        static_assert(SensorDims<M>::bytes <= 64 * 1024, "dynamic LDS within the default limit: no function attribute to set");
        hipLaunchKernelGGL(sensor_update_large_kernel<M>, dim3((unsigned)a->B), dim3(64), SensorDims<M>::bytes, (hipStream_t)stream, *a);
    } else {
        hipLaunchKernelGGL(sensor_update_kernel<M>, dim3((unsigned)((a->B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class M>
int launch_plant_measure_linear(const SensorArgs* a, void* stream) {
    if (a->B < 1 || a->ny < 1 || a->ny > SENSOR_MAX_NY || !a->H || !a->x || !a->y_out || a->step < 0 || a->step >= PLANT_MAX_STEPS ||
        M::NX > PLANT_MAX_NX || (a->h_stride != 0 && a->h_stride != (long long)a->ny * M::NX)) return -1;
    const size_t grid = ((size_t)a->B * (size_t)a->ny + PLANT_MEASURE_THREADS - 1) / PLANT_MEASURE_THREADS;
    hipLaunchKernelGGL(plant_measure_linear_kernel<M>, dim3((unsigned)grid), dim3(PLANT_MEASURE_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
