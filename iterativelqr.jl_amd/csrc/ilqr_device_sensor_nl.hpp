// A nonlinear sensor y = h(x, s) + v, v ~ N(0, diag(r)), compiled like a model but as a module of its own (ilqr_compile_sensor,
// include/ilqr_hip.h): nx inputs, 1 <= ny <= 64 outputs (ny may exceed nx), 0 <= ns <= 64 sensor parameters s, shared by the batch
// (s_stride 0) or one row per instance (s_stride ns). The sensor is given ROW-WISE,
//
//   sensor_row(j, &y, dydx, x, s):  *y = h_j(x, s),  dydx[k] = ∂h_j/∂x_k for k < nx  (dydx pre-zeroed by the caller)
//
// so that a lane deals with one row of the Jacobian, nx doubles, never the ny · nx matrix. The kernel hands the sensor the row's own
// place in H as dydx, its element of ŷ as y and x as it lies in HBM: no per-thread array, no scratch whatever the sensor (DESIGN_LOG has
// the register table, "Compiled nonlinear sensors").
//
// sensor_linearise_kernel<S, JAC>: ONE LANE PER (INSTANCE, ROW). blockIdx.y = j, so all 64 lanes of a wave work on the same row and
// the `switch (j)` of a generated sensor is a uniform (scalar) branch; lane b = blockIdx.x · 64 + threadIdx.x.
//   JAC = true, the linearisation at x_lin:  H[b][j][0..nx) = row j of ∂h/∂x, layout [B][ny][nx] row-major — what
//     sensor_update_kernel reads with h_stride = ny · nx;  yhat[b][j] = h_j(x_lin[b], s), and with x_prior given
//     yhat[b][j] = h_j + Σ_k H_jk (x_prior_k − x_lin_k), ONE FMA chain over ascending k = 0 .. nx−1 that starts from h_j (the
//     difference rounded first): the ŷ of an iterated filter, for which the update's c_j = ŷ_j − h_j·x̂₀ is the IEKF offset.
//   JAC = false, the measurement:  y[b][j] = h_j(x[b], s), then + sigma[j] · z(seed, b0 + b, 5 + j / 16, step, j % 16) where
//     sigma[j] != 0 (product and sum rounded separately): the key fields of plant_measure_kernel and plant_measure_linear_kernel,
//     shared on purpose. No Jacobian is stored in this instantiation: the partials land in a row of LDS nobody reads.
// The user's code is compiled with floating-point contraction off (the generated module sets the pragma around it), so h_j is the
// same bits in both instantiations.
//
// x, s, sigma, H, yhat and y are HBM pointers; SensorNlArgs holds pointers and a few integers, nothing of length ny, nx or ns. Every
// element is written by the one lane that owns it with a plain vector store: no atomics, no cross-lane traffic, no barrier. The H
// stores of a wave are 64 segments of nx consecutive doubles, ny · nx doubles apart; they are not staged through LDS (DESIGN_LOG.md has
// the timing behind that).
#pragma once

#include <stdint.h>

namespace ilqr {

enum { SENSOR_NL_MAX_NS = 64, SENSOR_NL_MAX_ITERATIONS = 8 };

struct SensorNlArgs {
    int B;
    int step;                // measurement: plant steps taken when it is made
    long long s_stride;      // doubles between two instances' s: 0 (shared) or ns
    const double* s;         // [ns] or [B][ns]; may be null when ns == 0
    const double* x;         // [B][nx]: the point of linearisation, or the state measured
    const double* x_prior;   // linearisation: null, or [B][nx]
    double* H;               // linearisation: [B][ny][nx]
    double* yhat;            // linearisation: [B][ny]
    uint64_t seed;           // the measurement
    long long b0;            // global index of the handle's instance 0
    const double* sigma;     // null, or [ny]
    double* y_out;           // [B][ny]
};
static_assert(sizeof(SensorNlArgs) <= 4096, "the kernel argument segment");

template <class S, bool JAC>
__global__ __launch_bounds__(64) void sensor_linearise_kernel(SensorNlArgs a) {
    constexpr int n = S::NX, ny = S::NY;
    const int j = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B || j >= ny) return;
    const double* xb = a.x + (size_t)b * n;
    const double* sb = a.s ? a.s + (size_t)b * (size_t)a.s_stride : nullptr;
    const size_t e = (size_t)b * ny + j;
    if constexpr (JAC) {
        // The sensor writes straight to where its outputs live: dydx IS the lane's row of H in HBM, zeroed here and then written where
        // a partial is non-zero, y is the lane's element of ŷ, and x is read in place. The compiler merges neighbouring cases of the
        // switch into one whose stores go through a pointer or an index computed from j; with every target in global memory that is
        // address arithmetic — a per-thread array in its place became scratch (DESIGN_LOG.md, "Compiled nonlinear sensors").
        double* Hj = a.H + e * n;
        double* yj = a.yhat + e;
#pragma unroll
        for (int k = 0; k < n; ++k) Hj[k] = 0.0;
        *yj = 0.0;
        S::row(j, yj, Hj, xb, sb);
        if (a.x_prior) {                                                          // (the same branch on every lane)
            const double* xp = a.x_prior + (size_t)b * n;
            double y = *yj;
#pragma unroll 8
            for (int k = 0; k < n; ++k) y = fma(Hj[k], __dsub_rn(xp[k], xb[k]), y);
            *yj = y;
        }
    } else {
        // The measurement has nowhere in HBM for the partials: they go, with y, to a row of LDS the lane owns, zeroed first as the
        // contract promises, and nobody reads it (one address space for every target of the merged stores, so again no scratch; no
        // barrier: a lane reads only what it wrote). 64 · (nx + 1) doubles of static LDS per workgroup, 33 KB at nx = 64.
        __shared__ double sink[64 * (n + 1)];
        double* dl = sink + threadIdx.x * (n + 1);
#pragma unroll
        for (int k = 0; k <= n; ++k) dl[k] = 0.0;
        S::row(j, dl + n, dl, xb, sb);
        double y = dl[n];
        if (a.sigma) {
            const double sg = a.sigma[j];
            if (sg != 0.0) y = __dadd_rn(y, __dmul_rn(sg, sample_z(a.seed, a.b0 + b, PLANT_MEASURE_FIELD0 + j / 16, a.step, j % 16)));
        }
        a.y_out[e] = y;
    }
}

template <class S>
int launch_sensor_linearise(const SensorNlArgs* a, void* stream) {
    if (a->B < 1 || !a->x || !a->H || !a->yhat || (S::NS > 0 && !a->s) || (a->s_stride != 0 && a->s_stride != S::NS)) return -1;
    hipLaunchKernelGGL((sensor_linearise_kernel<S, true>), dim3((unsigned)((a->B + 63) / 64), (unsigned)S::NY), dim3(64), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class S>
int launch_sensor_measure(const SensorNlArgs* a, void* stream) {
    if (a->B < 1 || !a->x || !a->y_out || (S::NS > 0 && !a->s) || (a->s_stride != 0 && a->s_stride != S::NS) || a->step < 0 ||
        a->step >= PLANT_MAX_STEPS) return -1;
    hipLaunchKernelGGL((sensor_linearise_kernel<S, false>), dim3((unsigned)((a->B + 63) / 64), (unsigned)S::NY), dim3(64), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr

// Sensor module interface: what a compiled sensor (ilqr_compile_sensor) registers with the library. Apart from the models': one
// model runs with several sensors.
#define ILQR_SENSOR_ABI_VERSION 1   /* bump whenever SensorNlArgs or this struct change: stale sensor modules are refused */
extern "C" struct ilqr_sensor_vtable {
    int abi_version;     // ILQR_SENSOR_ABI_VERSION the module was compiled against
    int args_bytes;      // sizeof(ilqr::SensorNlArgs) it was compiled against
    const char* name;
    int nx, ny, ns;
    int (*launch_linearise)(const ilqr::SensorNlArgs* a, void* stream);
    int (*launch_measure)(const ilqr::SensorNlArgs* a, void* stream);
};
