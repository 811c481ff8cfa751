/* Plain-C closed MPC loop with a NONLINEAR sensor between plant and controller (include/ilqr_hip.h: ilqr_compile_sensor,
 * ilqr_mpc_run_nlsensor): cars (car_obs) that see nothing but their ranges to two beacons — no heading reading. The sensor is C
 * source (SENSOR_SOURCE below: ny = 2, ns = 4, the beacon positions), compiled for the GPU at run time and cached; the
 * extended Kalman filter on the device linearises it at its own estimate every period (iterated ITERATIONS times) and gives the
 * controller the state it re-solves from. The whole run is ONE call with one stream synchronise at the end. Prints the mean squared
 * position error of the estimate beside that of prediction alone (the controller's model run from the same first estimate under
 * the actions the plant applied); exits non-zero if a plant state was not finite or the estimate did not beat prediction alone.
 *
 *   gcc -O2 -Iinclude examples/mpc_range.c -o mpc_range \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_range 64
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ilqr_hip.h"

#define CHECK(call)                                                                  \
    do {                                                                             \
        int rc_ = (call);                                                            \
        if (rc_ != ILQR_OK) {                                                        \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ilqr_last_error()); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

enum { T = 51, NX = 3, NU = 2, NW = 2, NY = 2, NS = 4, N = T - 1, PERIODS = 10, STEPS = 1, R = PERIODS * STEPS, ITERATIONS = 2 };

/* The sensor, written by hand: the ranges of a car (px, py, theta) to two beacons whose positions are the sensor parameters
 * s = (b0x, b0y, b1x, b1y). Row j: *y = |p - b_j|, dydx = (p - b_j) / |p - b_j| on (px, py); dydx[2] stays the zero it arrives as.
 * (tools/prebuild_models.py reads the lines between the two markers, so that the build leaves the module in the cache.) */
static const char SENSOR_SOURCE[] =
    /* SENSOR SOURCE BEGIN */
    "ILQR_SENSOR_FN void sensor_row(int j, double* y, double* dydx, const double* x, const double* s) {\n"
    "    const double dx = x[0] - s[2 * j], dy = x[1] - s[2 * j + 1];\n"
    "    const double rho = sqrt(dx * dx + dy * dy);\n"
    "    *y = rho;\n"
    "    dydx[0] = dx / rho;\n"
    "    dydx[1] = dy / rho;\n"
    "}\n"
    /* SENSOR SOURCE END */;

/* the car of test/car.jl as the model integrates it: explicit midpoint, h = 0.1 */
static void car_step(const double* x, const double* u, double* out) {
    const double h = 0.1, th = x[2] + 0.5 * h * u[1];
    out[0] = x[0] + h * u[0] * cos(th);
    out[1] = x[1] + h * u[0] * sin(th);
    out[2] = x[2] + h * u[1];
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    const ilqr_sensor_source src = {"range2", NX, NY, NS, SENSOR_SOURCE, 0};
    char name[128], path[1024];
    CHECK(ilqr_compile_sensor(&src, name, sizeof(name), path, sizeof(path)));
    int32_t snx, sny, sns;
    CHECK(ilqr_sensor_dims(name, &snx, &sny, &sns));
    printf("sensor %s (%d -> %d, %d parameters): %s\n", name, (int)snx, (int)sny, (int)sns, path);

    ilqr_problem_desc desc = {"car_obs", NULL, T, B, 0, 1};
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* w = malloc((size_t)B * T * NW * sizeof(double));
    double* xhat0 = malloc((size_t)B * NX * sizeof(double));
    double* x_cl = malloc((size_t)B * (R + 1) * NX * sizeof(double));
    double* u_cl = malloc((size_t)B * R * NU * sizeof(double));
    double* xhat_cl = malloc((size_t)B * PERIODS * NX * sizeof(double));
    double* nis_cl = malloc((size_t)B * PERIODS * sizeof(double));
    double* P = calloc((size_t)B * NX * NX, sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("car_obs", T, 20240607, 0, B, x1, u));
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < T; ++t) { w[((size_t)b * T + t) * NW] = 0.75; w[((size_t)b * T + t) * NW + 1] = 0.5; }       /* the obstacle */
        /* the first estimate: off by decimetres and by a tenth of a radian, and known to be that vague */
        xhat0[(size_t)b * NX] = x1[(size_t)b * NX] + 0.2;
        xhat0[(size_t)b * NX + 1] = x1[(size_t)b * NX + 1] - 0.15;
        xhat0[(size_t)b * NX + 2] = x1[(size_t)b * NX + 2] + 0.1;
        for (int j = 0; j < NX; ++j) P[((size_t)b * NX + j) * NX + j] = j < 2 ? 0.1 : 0.05;
    }
    const double beacons[NS] = {3.0, 2.0, -2.0, 3.0};
    const double sigma_y[NY] = {1.0e-2, 1.0e-2}, r[NY] = {1.0e-4, 1.0e-4};
    const double q[NX] = {1.0e-8, 1.0e-8, 1.0e-8};
    const ilqr_nl_sensor sensor = {name, 0, beacons, r, q, sigma_y, ITERATIONS};
    /* the plant applies the plan's action without the feedback term, as examples/mpc_estimator.c does and for its reason */
    ilqr_mpc_desc d = {PERIODS, STEPS, 0, 0, ILQR_SHIFT_TAIL_HOLD, 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP, 20240607, 0, NULL};
    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    CHECK(ilqr_set_options(h, &opt));
    CHECK(ilqr_set_parameters(h, w));
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));
    CHECK(ilqr_mpc_run_nlsensor(h, &d, NULL, &sensor, x1, xhat0, P, NULL, NULL, x_cl, u_cl, NULL, nf, NULL, NULL, NULL, NULL, xhat_cl, NULL, nis_cl));
    int ok = 1;
    double e_hat = 0.0, e_open = 0.0, nis = 0.0;
    for (int b = 0; b < B; ++b) {
        if (nf[b] != -1) { fprintf(stderr, "instance %d: non-finite plant state after step %d\n", b, (int)nf[b]); ok = 0; }
        double xo[NX] = {xhat0[(size_t)b * NX], xhat0[(size_t)b * NX + 1], xhat0[(size_t)b * NX + 2]}, xn[NX];
        for (int p = 0; p < PERIODS; ++p) {
            for (int i = 0; i < STEPS; ++i) {                                                    /* prediction alone, under the applied actions */
                car_step(xo, u_cl + ((size_t)b * R + (size_t)p * STEPS + i) * NU, xn);
                for (int j = 0; j < NX; ++j) xo[j] = xn[j];
            }
            const double* x = x_cl + ((size_t)b * (R + 1) + (size_t)(p + 1) * STEPS) * NX;      /* delay 0: measured after the period's steps */
            const double* xh = xhat_cl + ((size_t)b * PERIODS + p) * NX;
            for (int j = 0; j < 2; ++j) {
                e_hat += pow(xh[j] - x[j], 2) / ((double)B * PERIODS);
                e_open += pow(xo[j] - x[j], 2) / ((double)B * PERIODS);
            }
            nis += nis_cl[(size_t)b * PERIODS + p] / ((double)B * PERIODS);
        }
    }
    printf("position: mean squared error of the estimate %.3e, of prediction alone %.3e; mean nis %.3f\n", e_hat, e_open, nis);
    if (!(e_hat < e_open)) { fprintf(stderr, "the estimate did not beat prediction alone\n"); ok = 0; }
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(w); free(xhat0); free(x_cl); free(u_cl); free(xhat_cl); free(nis_cl); free(P); free(nf);
    return ok ? 0 : 3;
}
