/* Plain-C caller of ilqr_initialize_rollout_candidates (include/ilqr_hip.h): draw S candidate action sequences per acrobot
 * swing-up, let the device score them and start every solve from the best one.
 *
 *   gcc -O2 -Iinclude examples/candidate_init.c -o candidate_init \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./candidate_init 64 8
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
    const int B = argc > 1 ? atoi(argv[1]) : 64, S = argc > 2 ? atoi(argv[2]) : 8, T = 101, nx = 4, nu = 1, N = T - 1;
    ilqr_problem_desc desc = {"acrobot", NULL, T, B, 0, 1};
    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    CHECK(ilqr_set_options(h, &opt));

    /* candidate s of every instance: noise of amplitude s / S — candidate 0 is "do nothing" */
    const size_t BS = (size_t)B * S;
    double* x1 = calloc((size_t)B * nx, sizeof(double));
    double* u = malloc(BS * N * nu * sizeof(double));
    uint64_t seed = 20240607;
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < S; ++s)
            for (int t = 0; t < N * nu; ++t) u[((size_t)b * S + s) * N * nu + t] = ((double)s / S) * gauss(&seed);
    if (ilqr_initialize_rollout_candidates(h, 0, 0.0, x1, u, NULL, NULL, NULL, NULL) == ILQR_OK) {
        fprintf(stderr, "zero candidates were accepted\n");
        return 3;
    }

    int32_t* chosen = malloc((size_t)B * sizeof(int32_t));
    double* cost = malloc(BS * sizeof(double));
    double* viol = malloc(BS * sizeof(double));
    CHECK(ilqr_initialize_rollout_candidates(h, S, 0.0, x1, u, chosen, cost, viol, NULL));
    int in_range = 1, is_min = 1;
    for (int b = 0; b < B; ++b) {
        in_range = in_range && chosen[b] >= 0 && chosen[b] < S;
        if (!in_range) break;
        for (int s = 0; s < S; ++s) is_min = is_min && !(cost[(size_t)b * S + s] < cost[(size_t)b * S + chosen[b]]);
    }
    printf("chosen candidate of instance 0: %d of %d (cost %.6g, violation %.3g)\n", (int)chosen[0], S,
           in_range ? cost[chosen[0]] : NAN, in_range ? viol[chosen[0]] : NAN);

    CHECK(ilqr_solve(h));
    CHECK(ilqr_synchronize(h));
    ilqr_stats* st = malloc((size_t)B * sizeof(ilqr_stats));
    CHECK(ilqr_get_stats(h, st));
    double worst = 0.0;
    for (int b = 0; b < B; ++b) worst = fmax(worst, st[b].max_violation);
    printf("acrobot T=%d B=%d S=%d: solved from the chosen candidates, worst max_violation %.3e\n", T, B, S, worst);
    const int ok = in_range && is_min && isfinite(worst);
    printf(ok ? "candidate init check passed\n" : "candidate init check FAILED\n");
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(chosen); free(cost); free(viol); free(st);
    return ok ? 0 : 2;
}
