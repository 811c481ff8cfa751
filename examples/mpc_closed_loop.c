/* Plain-C closed MPC loop on the device (include/ilqr_hip.h): a batch of cars (the reference's test/car.jl: goal [1, 1, 0] behind an
 * obstacle, boxed controls, 51-step horizon) is solved once; then ilqr_mpc_run runs eight control periods in ONE call — per period
 * the plant applies the first action of the plan under a state disturbance drawn on the device (sigma_x = 1e-3), the horizon and the
 * duals shift by one period from the plant state, and a warm re-solve follows — with one stream synchronise at the end. Nothing
 * crosses PCIe in between: compare examples/mpc_warm.c, which forms the plant on the host. Prints the mean outer and inner
 * iterations per period, read from the log; exits non-zero if a plant state or a logged max_violation was not finite.
 *
 *   gcc -O2 -Iinclude examples/mpc_closed_loop.c -o mpc_closed_loop \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_closed_loop 64
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
    enum { T = 51, NX = 3, NU = 2, N = T - 1, PERIODS = 8, STEPS = 1 };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"car", NULL, T, B, 0, 1};
    ilqr_handle* h = NULL;
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* x_cl = malloc((size_t)B * (PERIODS * STEPS + 1) * NX * sizeof(double));
    double* log = malloc((size_t)B * PERIODS * ILQR_MPC_LOG_W * sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("car", T, 20240607, 0, B, x1, u));
    CHECK(ilqr_create(&desc, &h));
    CHECK(ilqr_set_options(h, &opt));
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));

    const double sigma_x[NX] = {1.0e-3, 1.0e-3, 1.0e-3};
    ilqr_mpc_desc d = {PERIODS, STEPS, 0, 0, ILQR_SHIFT_TAIL_HOLD, 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP, 20240607, 0, sigma_x};
    CHECK(ilqr_mpc_run(h, &d, NULL, NULL, x_cl, NULL, log, nf));

    int ok = 1;
    for (int p = 0; p < PERIODS; ++p) {
        double outer = 0.0, inner = 0.0, worst = 0.0;
        for (int b = 0; b < B; ++b) {
            const double* row = log + ((size_t)b * PERIODS + p) * ILQR_MPC_LOG_W;      /* ilqr_stats order */
            if (!isfinite(row[2])) ok = 0;
            worst = fmax(worst, row[2]); inner += row[4]; outer += row[5];
        }
        printf("period %d: %.2f outer / %.2f inner iterations per instance, worst violation %.2e\n", p + 1, outer / B, inner / B, worst);
    }
    for (int b = 0; b < B; ++b)
        if (nf[b] != -1) { fprintf(stderr, "instance %d: non-finite plant state after step %d\n", b, (int)nf[b]); ok = 0; }
    const double* xe = x_cl + ((size_t)0 * (PERIODS * STEPS + 1) + PERIODS * STEPS) * NX;
    printf("instance 0 after %d periods: x = (%.4f, %.4f, %.4f)\n", PERIODS, xe[0], xe[1], xe[2]);
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(x_cl); free(log); free(nf);
    return ok ? 0 : 3;
}
