/* Plain-C caller of ilqr_rollout_policy (include/ilqr_hip.h): solve a batch of acrobot swing-ups, then run every instance's
 * feedback policy from S perturbed initial states and report how the closed loop fares.
 *
 *   gcc -O2 -Iinclude examples/policy_rollout.c -o policy_rollout \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./policy_rollout 256 1024
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

static double gauss(uint64_t* s) {   /* splitmix64 + Box-Muller */
    double u[2];
    for (int i = 0; i < 2; ++i) {
        uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        u[i] = ((double)(z >> 11) + 0.5) / 9007199254740992.0;
    }
    return sqrt(-2.0 * log(u[0])) * cos(6.283185307179586 * u[1]);
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 64, S = argc > 2 ? atoi(argv[2]) : 256, T = 101, nx = 4, nu = 1;
    ilqr_problem_desc desc = {"acrobot", NULL, T, B, 0, 1};
    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    CHECK(ilqr_set_options(h, &opt));

    double* x1 = calloc((size_t)B * nx, sizeof(double));
    double* ub = malloc((size_t)B * (T - 1) * nu * sizeof(double));
    uint64_t seed = 20240607;
    for (size_t i = 0; i < (size_t)B * (T - 1) * nu; ++i) ub[i] = gauss(&seed);
    /* before any solve there is no policy to run */
    double c0 = 0.0;
    if (ilqr_rollout_policy(h, 1, 0.0, x1, NULL, &c0, NULL, NULL, NULL, NULL) == ILQR_OK) {
        fprintf(stderr, "a fresh handle accepted ilqr_rollout_policy\n");
        return 3;
    }
    CHECK(ilqr_initialize_rollout(h, x1, ub));
    CHECK(ilqr_solve(h));
    double* xb = malloc((size_t)B * T * nx * sizeof(double));
    CHECK(ilqr_get_trajectory(h, xb, NULL));

    /* sample 0 of every instance starts on the nominal trajectory, the others 0.02 sigma away from it */
    const size_t BS = (size_t)B * S;
    double* xs = malloc(BS * nx * sizeof(double));
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < nx; ++i)
                xs[((size_t)b * S + s) * nx + i] = xb[(size_t)b * T * nx + i] + (s == 0 ? 0.0 : 0.02 * gauss(&seed));
    double* cost = malloc(BS * sizeof(double));
    double* viol = malloc(BS * sizeof(double));
    int32_t* nonfinite = malloc(BS * sizeof(int32_t));
    double* x = malloc(BS * T * nx * sizeof(double));
    CHECK(ilqr_rollout_policy(h, S, 0.0, xs, NULL, cost, viol, nonfinite, x, NULL));

    int finite = 0, near = 0;
    double track = 0.0;
    const double goal[4] = {3.14159265358979323846, 0.0, 0.0, 0.0};
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s) {
            const size_t bs = (size_t)b * S + s;
            const double* xT = x + (bs * T + (T - 1)) * nx;
            double e = 0.0;
            for (int i = 0; i < nx; ++i) e = fmax(e, fabs(xT[i] - goal[i]));
            finite += nonfinite[bs] == -1 && isfinite(cost[bs]);
            near += e < 0.2;
            if (s == 0)      /* tracking from the nominal start reproduces the nominal trajectory */
                for (int i = 0; i < nx; ++i) track = fmax(track, fabs(xT[i] - xb[((size_t)b * T + (T - 1)) * nx + i]));
        }
    printf("acrobot T=%d B=%d S=%d: %d/%zu samples finite, %d end within 0.2 of the goal, nominal start tracks to %.2e\n",
           T, B, S, finite, BS, near, track);
    const int ok = finite == (int)BS && track < 1.0e-6;
    printf(ok ? "policy rollout check passed\n" : "policy rollout check FAILED\n");
    CHECK(ilqr_destroy(h));
    free(x1); free(ub); free(xb); free(xs); free(cost); free(viol); free(nonfinite); free(x);
    return ok ? 0 : 2;
}
