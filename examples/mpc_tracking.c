/* Plain-C tracking MPC on the device (include/ilqr_hip.h): a batch of cars (car_obs: the reference's test/car.jl with the obstacle
 * centre in the parameters theta_t = (p_x, p_y)) drives to its goal while the obstacle moves along a line, p(g) = p(0) + g * v at
 * global control period g. Two closed loops of PERIODS re-solves, each ONE call of ilqr_mpc_run_preview with one synchronise:
 *   preview: the horizon holds p(t) for t = 0 .. T-1 and every period the row that enters it is the obstacle's future position,
 *            w_preview[r] = p(T + r);
 *   held:    the controller believes the obstacle stands still at p(0) (w_preview = NULL: the last row is held).
 * In both the plant runs under the truth, w_plant[r] = p(r), and the realised stage cost and constraint violation of every plant
 * step are taken under it (cl_cost, cl_violation). Prints the summed realised cost and the maximum realised violation of both runs;
 * exits non-zero if a plant state or a score was not finite.
 *
 *   gcc -O2 -Iinclude examples/mpc_tracking.c -o mpc_tracking \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_tracking 64
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

enum { T = 51, NX = 3, NU = 2, NW = 2, N = T - 1, PERIODS = 30, STEPS = 1, R = PERIODS * STEPS };

/* the obstacle's centre at global control period g: from beside the car's path onto it */
static void obstacle(int g, double* p) {
    p[0] = 0.75 - 0.01 * g;
    p[1] = 0.5;
}

/* one closed loop; preview != 0: the controller sees the obstacle's future positions */
static int run(int B, int preview, double* cost_sum, double* viol_max, int* finite) {
    ilqr_problem_desc desc = {"car_obs", NULL, T, B, 0, 1};
    ilqr_handle* h = NULL;
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* w = malloc((size_t)B * T * NW * sizeof(double));
    double* w_plant = malloc((size_t)B * R * NW * sizeof(double));
    double* w_preview = malloc((size_t)B * R * NW * sizeof(double));
    double* cl_cost = malloc((size_t)B * R * sizeof(double));
    double* cl_viol = malloc((size_t)B * R * sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("car_obs", T, 20240607, 0, B, x1, u));
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < T; ++t) obstacle(preview ? t : 0, w + ((size_t)b * T + t) * NW);
        for (int r = 0; r < R; ++r) {
            obstacle(r, w_plant + ((size_t)b * R + r) * NW);               /* the truth the plant runs under and the score is taken under */
            obstacle(T + r, w_preview + ((size_t)b * R + r) * NW);         /* the row that enters the horizon after plant step r */
        }
    }
    CHECK(ilqr_create(&desc, &h));
    CHECK(ilqr_set_options(h, &opt));
    CHECK(ilqr_set_parameters(h, w));
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));
    ilqr_mpc_desc d = {PERIODS, STEPS, 0, 0, ILQR_SHIFT_TAIL_HOLD, 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP, 20240607, 0, NULL};
    CHECK(ilqr_mpc_run_preview(h, &d, NULL, w_plant, preview ? w_preview : NULL, NULL, NULL, NULL, nf, cl_cost, cl_viol));
    *cost_sum = 0.0; *viol_max = 0.0; *finite = 1;
    for (int b = 0; b < B; ++b) {
        if (nf[b] != -1) *finite = 0;
        for (int r = 0; r < R; ++r) {
            const double c = cl_cost[(size_t)b * R + r], v = cl_viol[(size_t)b * R + r];
            if (!isfinite(c) || !isfinite(v)) *finite = 0;
            *cost_sum += c;
            *viol_max = fmax(*viol_max, v);
        }
    }
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(w); free(w_plant); free(w_preview); free(cl_cost); free(cl_viol); free(nf);
    return 0;
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    int ok = 1;
    for (int preview = 1; preview >= 0; --preview) {
        double cost = 0.0, viol = 0.0;
        int finite = 1;
        if (run(B, preview, &cost, &viol, &finite) != 0) return 1;
        printf("%-8s %d periods, %d cars: realised cost %.6f per car, worst realised violation %.3e\n", preview ? "preview:" : "held:", PERIODS, B,
               cost / B, viol);
        ok = ok && finite;
    }
    return ok ? 0 : 3;
}
