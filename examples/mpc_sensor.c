/* Plain-C closed MPC loop with a linear sensor between plant and controller (include/ilqr_hip.h, ilqr_mpc_run_sensor): acrobots whose
 * first encoder reads the first joint angle q1 and whose second encoder reads the ABSOLUTE angle of the second link, q1 + q2 — so no
 * output is a state component — and whose joint velocities are not sensed at all: y = H x + v with H = [[1 0 0 0], [1 1 0 0]]. The
 * extended Kalman filter on the device — time update under the plan in flight, measurement update with the period's two readings —
 * gives the controller the state it re-solves from. The whole run is ONE call with one stream synchronise at the end. Prints the
 * mean squared error of the raw encoders (y_0 and y_1 - y_0) and of the estimate on the two angles against the true plant, the last
 * period's mean variance of the velocity estimate and the mean nis; exits non-zero if a plant state was not finite or the filter
 * did not beat its sensor on either angle.
 *
 *   gcc -O2 -Iinclude examples/mpc_sensor.c -o mpc_sensor \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_sensor 64
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

int main(int argc, char** argv) {
    enum { T = 51, NX = 4, NU = 1, NY = 2, N = T - 1, PERIODS = 8, STEPS = 1, R = PERIODS * STEPS };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"acrobot", NULL, T, B, 0, 1};
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* x_cl = malloc((size_t)B * (R + 1) * NX * sizeof(double));
    double* y_cl = malloc((size_t)B * PERIODS * NY * sizeof(double));
    double* xhat_cl = malloc((size_t)B * PERIODS * NX * sizeof(double));
    double* pdiag_cl = malloc((size_t)B * PERIODS * NX * sizeof(double));
    double* nis_cl = malloc((size_t)B * PERIODS * sizeof(double));
    double* P = calloc((size_t)B * NX * NX, sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("acrobot", T, 20240607, 0, B, x1, u));
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < NX; ++j) P[((size_t)b * NX + j) * NX + j] = j < 2 ? 1.0e-3 : 1.0e-1;       /* P0: the velocities are hardly known */

    const double H[NY * NX] = {1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0};
    const double sigma_y[NY] = {2.0e-2, 2.0e-2}, r[NY] = {4.0e-4, 4.0e-4};
    const double q[NX] = {1.0e-8, 1.0e-8, 1.0e-8, 1.0e-8};
    const ilqr_sensor sensor = {NY, 0, H, r, q, sigma_y};
    /* the plant applies the plan's action without the feedback term, as examples/mpc_estimator.c does and for its reason */
    ilqr_mpc_desc d = {PERIODS, STEPS, 0, 0, ILQR_SHIFT_TAIL_HOLD, 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP, 20240607, 0, NULL};
    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    CHECK(ilqr_set_options(h, &opt));
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));
    CHECK(ilqr_mpc_run_sensor(h, &d, NULL, &sensor, NULL, NULL, P, NULL, NULL, x_cl, NULL, NULL, nf, NULL, NULL, y_cl, NULL, xhat_cl, pdiag_cl, nis_cl));
    int ok = 1;
    double ey[2] = {0.0, 0.0}, eh[2] = {0.0, 0.0}, pv = 0.0, nis = 0.0;
    for (int b = 0; b < B; ++b) {
        if (nf[b] != -1) { fprintf(stderr, "instance %d: non-finite plant state after step %d\n", b, (int)nf[b]); ok = 0; }
        for (int p = 0; p < PERIODS; ++p) {
            const double* x = x_cl + ((size_t)b * (R + 1) + (size_t)(p + 1) * STEPS) * NX;      /* delay 0: measured after the period's steps */
            const double* y = y_cl + ((size_t)b * PERIODS + p) * NY;
            const double* xh = xhat_cl + ((size_t)b * PERIODS + p) * NX;
            const double raw[2] = {y[0], y[1] - y[0]};                                           /* what the encoders say about q1, q2 */
            for (int j = 0; j < 2; ++j) {
                ey[j] += pow(raw[j] - x[j], 2) / ((double)B * PERIODS);
                eh[j] += pow(xh[j] - x[j], 2) / ((double)B * PERIODS);
            }
            nis += nis_cl[(size_t)b * PERIODS + p] / ((double)B * PERIODS);
        }
        pv += (pdiag_cl[((size_t)b * PERIODS + PERIODS - 1) * NX + 2] + pdiag_cl[((size_t)b * PERIODS + PERIODS - 1) * NX + 3]) / (2.0 * B);
    }
    printf("q1: mean squared error of the encoder %.3e, of the estimate %.3e\n", ey[0], eh[0]);
    printf("q2: mean squared error of the encoders (y1 - y0) %.3e, of the estimate %.3e\n", ey[1], eh[1]);
    printf("velocities: mean variance of the estimate after %d periods %.3e (P0: 1.0e-01); mean nis %.3f\n", PERIODS, pv, nis);
    if (!(eh[0] < ey[0]) || !(eh[1] < ey[1])) { fprintf(stderr, "the estimate did not beat the encoders on both angles\n"); ok = 0; }
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(x_cl); free(y_cl); free(xhat_cl); free(pdiag_cl); free(nis_cl); free(P); free(nf);
    return ok ? 0 : 3;
}
