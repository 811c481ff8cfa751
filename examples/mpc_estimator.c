/* Plain-C closed MPC loop with an estimator between sensor and controller (include/ilqr_hip.h, ilqr_mpc_run_est): acrobots whose
 * two joint angles are measured with noise and whose joint velocities are not measured at all. An extended Kalman filter on the
 * device — time update under the plan in flight, measurement update with the period's angles — gives the controller the state it
 * re-solves from. The whole run is ONE call with one stream synchronise at the end. Prints the mean squared error of the measured
 * angles and of the estimate against the true plant, the last period's mean variance of the velocity estimate and the mean nis;
 * exits non-zero if a plant state was not finite or the filter did not beat its sensor on the angles.
 *
 *   gcc -O2 -Iinclude examples/mpc_estimator.c -o mpc_estimator \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_estimator 64
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
    enum { T = 51, NX = 4, NU = 1, N = T - 1, PERIODS = 8, STEPS = 1, R = PERIODS * STEPS };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"acrobot", NULL, T, B, 0, 1};
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* x_cl = malloc((size_t)B * (R + 1) * NX * sizeof(double));
    double* y_cl = malloc((size_t)B * PERIODS * NX * sizeof(double));
    double* xhat_cl = malloc((size_t)B * PERIODS * NX * sizeof(double));
    double* pdiag_cl = malloc((size_t)B * PERIODS * NX * sizeof(double));
    double* nis_cl = malloc((size_t)B * PERIODS * sizeof(double));
    double* P = calloc((size_t)B * NX * NX, sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("acrobot", T, 20240607, 0, B, x1, u));
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < NX; ++j) P[((size_t)b * NX + j) * NX + j] = j < 2 ? 1.0e-3 : 1.0e-1;       /* P0: the velocities are hardly known */

    const double sigma_y[NX] = {2.0e-2, 2.0e-2, 0.0, 0.0};
    const int32_t measured[NX] = {1, 1, 0, 0};
    const double q[NX] = {1.0e-8, 1.0e-8, 1.0e-8, 1.0e-8}, r[NX] = {4.0e-4, 4.0e-4, 1.0, 1.0};
    const ilqr_plant_io io = {NULL, NULL, sigma_y, 0, 0};
    const ilqr_estimator est = {measured, q, r};
    /* the plant applies the plan's action without the feedback term: on this swing-up a re-solve anchored 0.02 rad off leaves gains
     * under which the plant diverges, with or without a filter (DESIGN_LOG.md) */
    ilqr_mpc_desc d = {PERIODS, STEPS, 0, 0, ILQR_SHIFT_TAIL_HOLD, 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP, 20240607, 0, NULL};
    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    CHECK(ilqr_set_options(h, &opt));
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));
    CHECK(ilqr_mpc_run_est(h, &d, &io, &est, NULL, NULL, P, NULL, NULL, x_cl, NULL, NULL, nf, NULL, NULL, y_cl, NULL, xhat_cl, pdiag_cl, nis_cl));
    int ok = 1;
    double ey = 0.0, eh = 0.0, pv = 0.0, nis = 0.0;
    for (int b = 0; b < B; ++b) {
        if (nf[b] != -1) { fprintf(stderr, "instance %d: non-finite plant state after step %d\n", b, (int)nf[b]); ok = 0; }
        for (int p = 0; p < PERIODS; ++p) {
            const double* x = x_cl + ((size_t)b * (R + 1) + (size_t)(p + 1) * STEPS) * NX;      /* delay 0: measured after the period's steps */
            const size_t row = ((size_t)b * PERIODS + p) * NX;
            for (int j = 0; j < 2; ++j) {
                ey += pow(y_cl[row + j] - x[j], 2) / (2.0 * B * PERIODS);
                eh += pow(xhat_cl[row + j] - x[j], 2) / (2.0 * B * PERIODS);
            }
            nis += nis_cl[(size_t)b * PERIODS + p] / ((double)B * PERIODS);
        }
        pv += (pdiag_cl[((size_t)b * PERIODS + PERIODS - 1) * NX + 2] + pdiag_cl[((size_t)b * PERIODS + PERIODS - 1) * NX + 3]) / (2.0 * B);
    }
    printf("angles: mean squared error of the measurement %.3e, of the estimate %.3e\n", ey, eh);
    printf("velocities: mean variance of the estimate after %d periods %.3e (P0: 1.0e-01); mean nis %.3f\n", PERIODS, pv, nis);
    if (!(eh < ey)) { fprintf(stderr, "the estimate did not beat the measurement on the angles\n"); ok = 0; }
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(x_cl); free(y_cl); free(xhat_cl); free(pdiag_cl); free(nis_cl); free(P); free(nf);
    return ok ? 0 : 3;
}
