/* Plain-C receding-horizon loop on ilqr_shift_horizon (include/ilqr_hip.h): a batch of particles (x+ = [x0 + x1, x1 + u], goal
 * [1, 0] at the end of an 11-step horizon) is solved, the first action is applied to a plant that adds a small disturbance, the
 * solved trajectory is shifted by one control period on the device — the shifted policy run closed-loop from the measured state —
 * and the handle is solved again: five periods. A second handle solves every period cold, from the same measured state and zero
 * actions, for comparison. Prints the mean inner iterations per period of both.
 *
 *   gcc -O2 -Iinclude examples/mpc_shift.c -o mpc_shift \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./mpc_shift 64
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

static double mean_iterations(const ilqr_stats* st, int B) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += st[b].iterations;
    return s / B;
}

int main(int argc, char** argv) {
    enum { T = 11, NX = 2, NU = 1, N = T - 1, PERIODS = 5 };
    const int B = argc > 1 ? atoi(argv[1]) : 64;
    if (B < 1) return 2;
    ilqr_problem_desc desc = {"particle", NULL, T, B, 0, 1};
    ilqr_handle *warm = NULL, *cold = NULL;
    CHECK(ilqr_create(&desc, &warm));
    CHECK(ilqr_create(&desc, &cold));
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    CHECK(ilqr_set_options(warm, &opt));
    CHECK(ilqr_set_options(cold, &opt));

    double* x1 = calloc((size_t)B * NX, sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* zero = calloc((size_t)B * N * NU, sizeof(double));
    double* xb = malloc((size_t)B * T * NX * sizeof(double));
    ilqr_stats* st = malloc((size_t)B * sizeof(ilqr_stats));
    uint64_t seed = 20240607;
    for (size_t i = 0; i < (size_t)B * N * NU; ++i) u[i] = 0.1 * gauss(&seed);

    /* the closed-loop shift needs a policy: refused before the first solve */
    CHECK(ilqr_initialize_rollout(warm, x1, u));
    if (ilqr_shift_horizon(warm, 1, ILQR_SHIFT_TAIL_HOLD, 1, NULL, NULL) == ILQR_OK) {
        fprintf(stderr, "a handle without a policy accepted a closed-loop shift\n");
        return 3;
    }
    CHECK(ilqr_solve(warm));
    CHECK(ilqr_get_stats(warm, st));
    printf("period 0: first solve, %.2f iterations per instance\n", mean_iterations(st, B));

    int ok = 1;
    for (int p = 1; p <= PERIODS; ++p) {
        /* the plant: the planned next state plus a disturbance, measured */
        CHECK(ilqr_get_trajectory(warm, xb, NULL));
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < NX; ++i) x1[(size_t)b * NX + i] = xb[((size_t)b * T + 1) * NX + i] + 0.01 * gauss(&seed);
        CHECK(ilqr_shift_horizon(warm, 1, ILQR_SHIFT_TAIL_HOLD, 1, x1, NULL));
        CHECK(ilqr_get_trajectory(warm, xb, NULL));
        for (int b = 0; b < B; ++b)             /* the shifted nominal trajectory starts at the measured state */
            for (int i = 0; i < NX; ++i) ok = ok && xb[(size_t)b * T * NX + i] == x1[(size_t)b * NX + i];
        CHECK(ilqr_solve(warm));
        CHECK(ilqr_get_stats(warm, st));
        const double it_warm = mean_iterations(st, B);
        double worst = 0.0;
        for (int b = 0; b < B; ++b) worst = fmax(worst, st[b].max_violation);
        ok = ok && isfinite(worst);

        CHECK(ilqr_reset(cold));
        CHECK(ilqr_initialize_rollout(cold, x1, zero));
        CHECK(ilqr_solve(cold));
        CHECK(ilqr_get_stats(cold, st));
        printf("period %d: %.2f iterations per instance after the shift, %.2f from a cold start (worst max_violation %.3e)\n", p, it_warm,
               mean_iterations(st, B), worst);
    }
    printf(ok ? "mpc shift check passed\n" : "mpc shift check FAILED\n");
    CHECK(ilqr_destroy(warm));
    CHECK(ilqr_destroy(cold));
    free(x1); free(u); free(zero); free(xb); free(st);
    return ok ? 0 : 2;
}
