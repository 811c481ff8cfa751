// Adapter from the C contract of a nonlinear sensor to the kernels of ilqr_device_sensor_nl.hpp — the seam behind
// ilqr_compile_sensor (include/ilqr_hip.h). The source defines ONE function,
//
//     ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s);
//
// which writes *y = h_j(x, s) and dydx[k] = ∂h_j/∂x_k for k < nx; dydx is pre-zeroed by the caller, so only non-zero partials need
// be written. math.h names and ilqr::sincos_fast are available as in model sources. ilqr_compile_sensor wraps the source into a
// struct F with a static forwarder, instantiates AdaptedSensor<F, nx, ny, ns> and registers the two launchers with the library.
// A sensor is a module of its own: it knows nothing of a model but nx.
#pragma once

#include "ilqr_device.hpp"

#define ILQR_SENSOR_FN __device__ __forceinline__ static

namespace ilqr {

template <class F, int NX_, int NY_, int NS_>
struct AdaptedSensor {
    static constexpr int NX = NX_, NY = NY_, NS = NS_;
    static_assert(NX >= 1 && NX <= PLANT_MAX_NX && NY >= 1 && NY <= SENSOR_MAX_NY && NS >= 0 && NS <= SENSOR_NL_MAX_NS,
                  "ilqr_compile_sensor: 1 <= nx <= 64, 1 <= ny <= 64, 0 <= ns <= 64");
    __device__ __forceinline__ static void row(int j, double* y, double* dydx, const double* x, const double* s) { F::sensor_row(j, y, dydx, x, s); }
};

template <class S>
struct SensorModule {
    static const ilqr_sensor_vtable* vtable() {
        static const ilqr_sensor_vtable vt = {ILQR_SENSOR_ABI_VERSION, (int)sizeof(SensorNlArgs), S::NAME, S::NX, S::NY, S::NS,
                                              &launch_sensor_linearise<S>, &launch_sensor_measure<S>};
        return &vt;
    }
};

}  // namespace ilqr

#define ILQR_DEFINE_SENSOR(SENSOR)                                                               \
    namespace {                                                                                  \
    struct Registrar_##SENSOR {                                                                  \
        Registrar_##SENSOR() { ilqr_register_sensor(ilqr::SensorModule<SENSOR>::vtable()); }     \
    } registrar_##SENSOR;                                                                        \
    }
