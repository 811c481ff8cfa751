/* Plain-C receding-horizon loop with warm duals (include/ilqr_hip.h): a batch of cars (the reference's test/car.jl: goal [1, 1, 0]
 * behind an obstacle, boxed controls, 51-step horizon) is solved once; then, per control period, the plant applies the first action
 * under a small disturbance, ilqr_shift_horizon moves the trajectory on by one period from the measured state, ilqr_shift_duals
 * moves the multipliers and penalties along with it, and ilqr_solve_warm solves again without climbing the penalty ladder from
 * rho0. A second handle does the same shift but re-solves cold (ilqr_solve: lambda = 0, rho = rho0), for comparison. Prints the mean
 * outer and inner iterations per period of both.
 *
 *   gcc -O2 -Iinclude examples/mpc_warm.c -o mpc_warm \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_warm 64
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

static void means(const ilqr_stats* st, int B, double* outer, double* inner, double* worst) {
    *outer = 0.0; *inner = 0.0; *worst = 0.0;
    for (int b = 0; b < B; ++b) {
        *outer += st[b].outer_iterations; *inner += st[b].iterations;
        *worst = fmax(*worst, st[b].max_violation);
    }
    *outer /= B; *inner /= B;
}

int main(int argc, char** argv) {
    enum { T = 51, NX = 3, NU = 2, N = T - 1, PERIODS = 4 };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"car", NULL, T, B, 0, 1};
    ilqr_handle* h[2] = {NULL, NULL};                 /* 0: warm duals, 1: cold re-solves */
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    double* x1 = calloc((size_t)B * NX, sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* xb = malloc((size_t)B * T * NX * sizeof(double));
    ilqr_stats* st = malloc((size_t)B * sizeof(ilqr_stats));
    uint64_t seed = 20240607;
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < 2; ++i) x1[(size_t)b * NX + i] = b ? 0.05 * gauss(&seed) : 0.0;
        for (int t = 0; t < N; ++t) { u[((size_t)b * N + t) * NU] = 1.0e-2; u[((size_t)b * N + t) * NU + 1] = 1.0e-3; }   /* test/car.jl:28 */
    }
    double outer[2], inner[2], worst[2];
    for (int i = 0; i < 2; ++i) {
        CHECK(ilqr_create(&desc, &h[i]));
        CHECK(ilqr_set_options(h[i], &opt));
        CHECK(ilqr_initialize_rollout(h[i], x1, u));
        if (i == 0 && ilqr_solve_warm(h[i]) == ILQR_OK) {      /* no duals yet: a warm solve would be the unconstrained one */
            fprintf(stderr, "a handle without duals accepted a warm solve\n");
            return 3;
        }
        CHECK(ilqr_solve(h[i]));
    }
    CHECK(ilqr_get_stats(h[0], st));
    means(st, B, &outer[0], &inner[0], &worst[0]);
    printf("period 0: first solve, %.2f outer / %.2f inner iterations per instance\n", outer[0], inner[0]);

    int ok = 1;
    for (int p = 1; p <= PERIODS; ++p) {
        /* the plant: the planned next state plus a disturbance, measured (the same for both handles: their plans are the same bits
         * only in period 1, so each follows its own) */
        for (int i = 0; i < 2; ++i) {
            CHECK(ilqr_get_trajectory(h[i], xb, NULL));
            uint64_t s = seed + (uint64_t)p;
            for (int b = 0; b < B; ++b)
                for (int j = 0; j < NX; ++j) x1[(size_t)b * NX + j] = xb[((size_t)b * T + 1) * NX + j] + 1.0e-3 * gauss(&s);
            CHECK(ilqr_shift_horizon(h[i], 1, ILQR_SHIFT_TAIL_HOLD, 0, x1, NULL));
            if (i == 0) {
                CHECK(ilqr_shift_duals(h[i], 1, ILQR_DUALS_TAIL_HOLD, ILQR_DUALS_PENALTY_KEEP));
                CHECK(ilqr_solve_warm(h[i]));
            } else {
                CHECK(ilqr_solve(h[i]));
            }
            CHECK(ilqr_get_stats(h[i], st));
            means(st, B, &outer[i], &inner[i], &worst[i]);
            ok = ok && isfinite(worst[i]) && outer[i] >= 1.0;
        }
        printf("period %d: warm %.2f outer / %.2f inner iterations per instance (worst max_violation %.3e), cold %.2f / %.2f (%.3e)\n", p,
               outer[0], inner[0], worst[0], outer[1], inner[1], worst[1]);
    }
    printf(ok ? "mpc warm check passed\n" : "mpc warm check FAILED\n");
    CHECK(ilqr_destroy(h[0]));
    CHECK(ilqr_destroy(h[1]));
    free(x1); free(u); free(xb); free(st);
    return ok ? 0 : 2;
}
