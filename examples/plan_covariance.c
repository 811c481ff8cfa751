/* Plain-C caller of the plan covariance (include/ilqr_hip.h, ilqr_plan_covariance): acrobots are solved once, then the covariance of
 * an initial estimate is pushed down the whole plan, with the plan's feedback gains and without them, under a small process noise.
 * Prints, per horizon position, the batch mean of the largest state standard deviation in both cases and of the standard deviation
 * of the torque the feedback asks for: the numbers a constraint back-off, a horizon length or a sensor would be chosen by. Exits
 * non-zero if a covariance was not finite or a stored matrix was not symmetric.
 *
 *   gcc -O2 -Iinclude examples/plan_covariance.c -o plan_covariance \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./plan_covariance 64
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
    enum { T = 51, NX = 4, NU = 1, N = T - 1, S = N };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"acrobot", NULL, T, B, 0, 1};
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* P0 = calloc((size_t)B * NX * NX, sizeof(double));
    double* sd_fb = malloc((size_t)B * (S + 1) * NX * sizeof(double));
    double* sd_ol = malloc((size_t)B * (S + 1) * NX * sizeof(double));
    double* ud = malloc((size_t)B * S * NU * sizeof(double));
    double* PS = malloc((size_t)B * NX * NX * sizeof(double));
    int32_t* nf = malloc((size_t)B * sizeof(int32_t));
    CHECK(ilqr_synthetic_inputs("acrobot", T, 20240607, 0, B, x1, u));
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < NX; ++j) P0[((size_t)b * NX + j) * NX + j] = j < 2 ? 1.0e-4 : 1.0e-2;      /* what a filter might hand over */
    const double q[NX] = {1.0e-8, 1.0e-8, 1.0e-6, 1.0e-6};

    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    CHECK(ilqr_set_options(h, &opt));
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));
    CHECK(ilqr_plan_covariance(h, S, 1, q, P0, sd_fb, ud, NULL, PS, nf));          /* under the plan's gains K_t */
    CHECK(ilqr_plan_covariance(h, S, 0, q, P0, sd_ol, NULL, NULL, NULL, NULL));    /* the actions applied as planned */

    int ok = 1;
    for (int b = 0; b < B; ++b) {
        if (nf[b] != -1) { fprintf(stderr, "instance %d: a non-finite variance at step %d\n", b, (int)nf[b]); ok = 0; }
        for (int r = 0; r < NX; ++r)
            for (int c = 0; c < r; ++c)
                if (PS[((size_t)b * NX + r) * NX + c] != PS[((size_t)b * NX + c) * NX + r]) { fprintf(stderr, "instance %d: P_out is not symmetric\n", b); ok = 0; }
    }
    printf("step   max state std (feedback)   max state std (no feedback)   torque std\n");
    for (int t = 0; t <= S; t += 10) {
        double fb = 0.0, ol = 0.0, tq = 0.0;
        for (int b = 0; b < B; ++b) {
            double mf = 0.0, mo = 0.0;
            for (int j = 0; j < NX; ++j) {
                mf = fmax(mf, sd_fb[((size_t)b * (S + 1) + t) * NX + j]);
                mo = fmax(mo, sd_ol[((size_t)b * (S + 1) + t) * NX + j]);
            }
            fb += sqrt(mf) / B; ol += sqrt(mo) / B;
            if (t < S) tq += sqrt(ud[((size_t)b * S + t) * NU]) / B;
        }
        if (t < S) printf("%4d   %24.3e   %27.3e   %10.3e\n", t, fb, ol, tq);
        else printf("%4d   %24.3e   %27.3e            -\n", t, fb, ol);
    }
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(P0); free(sd_fb); free(sd_ol); free(ud); free(PS); free(nf);
    return ok ? 0 : 3;
}
