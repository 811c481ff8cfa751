/* Plain-C sampling warm start on ilqr_sample_rollout_candidates (include/ilqr_hip.h): a batch of acrobot swing-ups is solved, the
 * solved trajectory is shifted by one control period on the device, S candidates per instance are drawn ON THE DEVICE around the
 * shifted guess (candidate 0 is the guess itself), scored, the best one is installed, and the handle is solved again. No candidate
 * array crosses the bus on the way in; the program asks for the candidates as drawn only to check them: the winner is what the
 * handle holds, it never scores worse than the guess it was drawn around, and the host twin ilqr_candidate_noise reproduces it.
 *
 *   gcc -O2 -Iinclude examples/sample_candidates.c -o sample_candidates \
 *       -Literativelqr.jl_amd/lib -lilqr_hip -Wl,-rpath,$PWD/iterativelqr.jl_amd/lib -lm
 *   ./sample_candidates 16 32
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
    enum { T = 51, NX = 4, NU = 1, N = T - 1 };
    const int B = argc > 1 ? atoi(argv[1]) : 16, S = argc > 2 ? atoi(argv[2]) : 32;
    if (B < 1 || S < 1) return 2;
    const uint64_t seed = 20261018;
    const double sigma[NU] = {0.05};
    ilqr_problem_desc desc = {"acrobot", NULL, T, B, 0, 1};
    ilqr_handle* h = NULL;
    CHECK(ilqr_create(&desc, &h));
    ilqr_options opt;
    CHECK(ilqr_default_options(&opt));
    opt.verbose = 0;
    CHECK(ilqr_set_options(h, &opt));

    double* x1 = malloc((size_t)B * NX * sizeof(double));
    double* u = malloc((size_t)B * N * NU * sizeof(double));
    double* base = malloc((size_t)B * N * NU * sizeof(double));
    double* cost = malloc((size_t)B * S * sizeof(double));
    double* cand = malloc((size_t)B * S * N * NU * sizeof(double));
    double* z = malloc((size_t)B * S * N * NU * sizeof(double));
    int32_t* chosen = malloc((size_t)B * sizeof(int32_t));
    ilqr_stats* st = malloc((size_t)B * sizeof(ilqr_stats));
    CHECK(ilqr_synthetic_inputs("acrobot", T, 1, 0, B, x1, u));

    /* NULL x1 / base_u mean the resident inputs: refused while the handle holds none */
    if (ilqr_sample_rollout_candidates(h, S, ILQR_SAMPLE_PICK, seed, 0, sigma, 0.0, 1.0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == ILQR_OK) {
        fprintf(stderr, "a handle without resident inputs accepted NULL x1 / base_u\n");
        return 3;
    }
    CHECK(ilqr_initialize_rollout(h, x1, u));
    CHECK(ilqr_solve(h));
    CHECK(ilqr_get_stats(h, st));
    double it0 = 0.0;
    for (int b = 0; b < B; ++b) it0 += st[b].iterations;

    /* one control period later: shift, keep the shifted guess for the checks, sample around it */
    CHECK(ilqr_shift_horizon(h, 1, ILQR_SHIFT_TAIL_HOLD, 0, NULL, NULL));
    CHECK(ilqr_get_buffer(h, "nominal_actions", base));
    CHECK(ilqr_sample_rollout_candidates(h, S, ILQR_SAMPLE_PICK, seed, 0, sigma, 0.0, 1.0, NULL, NULL, chosen, cost, NULL, NULL, NULL, cand));
    CHECK(ilqr_get_buffer(h, "nominal_actions", u));
    CHECK(ilqr_candidate_noise(seed, 0, B, S, N, NU, z));
    printf("chosen candidate of instance 0: %d of %d (cost %.6f, the shifted guess %.6f)\n", chosen[0], S, cost[chosen[0] < 0 ? 0 : chosen[0]], cost[0]);
    int ok = 1;
    double worst = 0.0;
    for (int b = 0; b < B; ++b) {
        const int c = chosen[b];
        ok = ok && c >= 0 && c < S && cost[(size_t)b * S + c] <= cost[(size_t)b * S];
        if (c < 0) continue;
        for (int e = 0; e < N * NU; ++e) {
            const double drawn = cand[((size_t)b * S + c) * N * NU + e];
            ok = ok && u[(size_t)b * N * NU + e] == drawn;                                   /* installed: the winner, bit for bit */
            ok = ok && cand[(size_t)b * S * N * NU + e] == base[(size_t)b * N * NU + e];     /* candidate 0: the shifted guess */
            worst = fmax(worst, fabs(drawn - (base[(size_t)b * N * NU + e] + sigma[e % NU] * z[((size_t)b * S + c) * N * NU + e])));
        }
    }
    ok = ok && worst < 1e-13;      /* sigma · (a few ulp of |z| <= 8.7) */
    printf("winner against base + sigma * ilqr_candidate_noise: max difference %.3e\n", worst);

    CHECK(ilqr_solve(h));
    CHECK(ilqr_get_stats(h, st));
    double it1 = 0.0, viol = 0.0;
    for (int b = 0; b < B; ++b) { it1 += st[b].iterations; viol = fmax(viol, st[b].max_violation); }
    ok = ok && isfinite(viol);
    printf("%.2f iterations per instance in the first solve, %.2f after shift + sampling (worst max_violation %.3e)\n", it0 / B, it1 / B, viol);
    printf(ok ? "sample candidates check passed\n" : "sample candidates check FAILED\n");
    CHECK(ilqr_destroy(h));
    free(x1); free(u); free(base); free(cost); free(cand); free(z); free(chosen); free(st);
    return ok ? 0 : 2;
}
