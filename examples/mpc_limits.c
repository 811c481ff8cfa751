/* Plain-C closed MPC loop with a plant that can be believed (include/ilqr_hip.h, ilqr_mpc_run_io): the cars of
 * examples/mpc_closed_loop.c, whose plan keeps the controls inside the box |u| <= 5, run eight control periods with feedback
 * ū + K (x − x̄) under a state disturbance — once with an ideal plant (ilqr_mpc_run_preview: the feedback term may leave the box, and
 * cl_violation only reports it), and once with the actuator limited to the box, a noisy measurement of the state and a solve that
 * takes one control period (delay 1: the re-solve is anchored at the controller's one-period prediction). Both runs are ONE call
 * each, with one stream synchronise at the end. Prints per run the largest |u| applied, the number of saturated (step, component)
 * pairs and the mean realised stage cost; exits non-zero if a limited action left the box or a plant state was not finite.
 *
 *   gcc -O2 -Iinclude examples/mpc_limits.c -o mpc_limits \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_limits 64
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
    enum { T = 51, NX = 3, NU = 2, N = T - 1, PERIODS = 8, STEPS = 1, R = PERIODS * STEPS };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"car", NULL, T, B, 0, 1};
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* u_cl = malloc((size_t)B * R * NU * sizeof(double));
    double* cost = malloc((size_t)B * R * sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    int32_t* saturated = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("car", T, 20240607, 0, B, x1, u));

    const double sigma_x[NX] = {2.0e-2, 2.0e-2, 2.0e-2}, sigma_y[NX] = {5.0e-3, 5.0e-3, 1.0e-2};
    const double u_min[NU] = {-5.0, -5.0}, u_max[NU] = {5.0, 5.0};
    const ilqr_plant_io io = {u_min, u_max, sigma_y, 1, 0};
    ilqr_mpc_desc d = {PERIODS, STEPS, 1, 0, ILQR_SHIFT_TAIL_HOLD, 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP, 20240607, 0, sigma_x};
    int ok = 1;
    for (int limited = 0; limited < 2; ++limited) {
        ilqr_handle* h = NULL;                 /* both runs start from the same solved plan */
        CHECK(ilqr_create(&desc, &h));
        CHECK(ilqr_set_options(h, &opt));
        CHECK(ilqr_initialize_rollout(h, x1, u));
        CHECK(ilqr_solve(h));
        if (limited) CHECK(ilqr_mpc_run_io(h, &d, &io, NULL, NULL, NULL, NULL, u_cl, NULL, nf, cost, NULL, NULL, saturated));
        else CHECK(ilqr_mpc_run_preview(h, &d, NULL, NULL, NULL, NULL, u_cl, NULL, nf, cost, NULL));
        double umax = 0.0, mean = 0.0;
        long sat = 0;
        for (size_t i = 0; i < (size_t)B * R * NU; ++i) umax = fmax(umax, fabs(u_cl[i]));
        for (size_t i = 0; i < (size_t)B * R; ++i) mean += cost[i] / ((double)B * R);
        for (int b = 0; b < B; ++b) {
            if (nf[b] != -1) { fprintf(stderr, "instance %d: non-finite plant state after step %d\n", b, (int)nf[b]); ok = 0; }
            if (limited) sat += saturated[b];
        }
        if (limited && umax > 5.0) { fprintf(stderr, "a limited action left the box: |u| = %.17g\n", umax); ok = 0; }
        printf("%s: largest |u| applied %.4f, %ld saturated, mean realised stage cost %.6f\n",
               limited ? "limits, measurement noise, delay 1" : "ideal plant                       ", umax, sat, mean);
        CHECK(ilqr_destroy(h));
    }
    free(x1); free(u); free(u_cl); free(cost); free(nf); free(saturated);
    return ok ? 0 : 3;
}
