// Host-side check of the launch plan (iterativelqr.jl_amd/csrc/ilqr_launch_plan.hpp); built and run by tests/test_launch_plan.py.
// Each row is one handle state and the launch written out by hand: kernel, grid, LDS, hand-over, pool and role settings. Prints
// one line per row and exits non-zero on the first row whose plan differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "ilqr_launch_plan.hpp"

using namespace ilqr;

// what the model modules export (ilqr_model_vtable: kernels, packed1_lds_bytes, packed2_lds_bytes) and the LDS of a workgroup of
// the latency kernel (Layout::lds_doubles * 8, large models: large_lds_doubles * 8) / the throughput kernel at the horizon
struct Model { const char* name; unsigned kernels; int p1, p2; size_t lds, slim; };
static const unsigned SMALL = 1u << K_LATENCY | 1u << K_STAGE | 1u << K_SLIM | 1u << K_STAGE_SLIM | 1u << K_PACKED1 | 1u << K_PACKED2 | 1u << K_RESUME;
static const unsigned MID = 1u << K_LATENCY | 1u << K_STAGE | 1u << K_MID | 1u << K_STAGE_MID;
static const unsigned LARGE = 1u << K_LATENCY | 1u << K_STAGE;
static const Model acrobot101 = {"acrobot T=101", SMALL, 28960, 28912, 39424, 20352};
static const Model acrobot201 = {"acrobot T=201", SMALL, 28960, 28912, 75424, 40352};
static const Model acrobot501 = {"acrobot T=501", SMALL, 28960, 28912, 183424, 100352};     // beyond the 160 KiB of a CU
static const Model acrobot51 = {"acrobot T=51", SMALL, 28960, 28912, 21424, 10352};
static const Model car51 = {"car T=51", SMALL, 22752, 22736, 28624, 19552};
static const Model synth12 = {"synth12 T=101", MID, 0, 0, 25008, 138944};
static const Model synth32 = {"synth32 T=101", LARGE, 0, 0, 61440, 0};
static const Model bigpack = {"small model, 50 KB packs", SMALL, 50000, 100000, 39424, 20352};  // one-wave form: 3 workgroups per CU
static const Model nopack = {"small model, no packed kernel", SMALL & ~(1u << K_PACKED1 | 1u << K_PACKED2 | 1u << K_RESUME), 0, 0, 39424, 20352};

static LaunchIn in(const Model& m, int B, int variant = 0) {
    LaunchIn i;
    i.variant = variant; i.B = B; i.num_simds = 1024;
    i.lds_bytes = m.lds; i.slim_lds_bytes = m.slim; i.lds_fits = m.lds <= 160 * 1024;
    i.kernels = m.kernels; i.packed1_lds_bytes = m.p1; i.packed2_lds_bytes = m.p2;
    i.constrained = true; i.max_dual_updates = 10;
    i.handover = -1; i.handover_live = -1; i.handover_mark = -1;
    const bool packed = (m.kernels >> K_PACKED1) & 1u, small = (m.kernels >> K_SLIM) & 1u;
    i.done_counter = packed; i.pool = packed; i.cu_slots = small;
    i.role_slots = true;
    return i;
}

struct Want {
    int kernel, grid;
    size_t lds;
    int ho_outer, ho_live;
    bool zero_pool, pool;
    int pool_mark, pool_cu, pool_ctl, pool_lds;
    bool role_slots;
    int cu_expect;
    bool resume;
};
// the common shapes: LDS-resident kernels (no hand-over), and the packed kernel
static Want plain(int kernel, int grid, size_t lds, int cu_expect = 0) { return {kernel, grid, lds, 0, 0, false, false, 0, 0, 0, 0, cu_expect > 0, cu_expect, false}; }
static Want error() { return {0, 0, 0, 0, 0, false, false, 0, 0, 0, 0, false, 0, false}; }

static int rows = 0;
static void check(const char* what, const LaunchPlan& p, const Want& w) {
    ++rows;
    char got[256], want[256];
    const char* fmt = "kernel %d grid %d lds %zu | ho %d live %d | pool zero %d on %d mark %d cu %d ctl %d lds %d | roles %d expect %d | resume %d";
    std::snprintf(got, sizeof got, fmt, p.kernel, p.grid, p.lds, p.handover_outer, p.handover_live, p.zero_pool, p.pool, p.pool_mark,
                  p.pool_cu, p.pool_ctl, p.pool_lds, p.role_slots, p.cu_expect, p.resume);
    std::snprintf(want, sizeof want, fmt, w.kernel, w.grid, w.lds, w.ho_outer, w.ho_live, w.zero_pool, w.pool, w.pool_mark,
                  w.pool_cu, w.pool_ctl, w.pool_lds, w.role_slots, w.cu_expect, w.resume);
    if (std::strcmp(got, want) != 0) {
        std::fprintf(stderr, "%s:\n  plan %s\n  want %s\n", what, got, want);
        std::exit(1);
    }
    std::printf("%s: %s\n", what, got);
}

int main() {
    LaunchIn i;
    // ---- auto, B <= #SIMDs: the latency kernel, one critical wave per SIMD: cu_expect = min(4, ceil(B / CUs))
    check("acrobot T=101 B=1024 auto (round 6 headline)", solve_plan(in(acrobot101, 1024)), plain(K_LATENCY, 1024, 39424, 4));
    check("acrobot T=101 B=16 auto", solve_plan(in(acrobot101, 16)), plain(K_LATENCY, 16, 39424, 1));
    check("acrobot T=101 B=600 auto", solve_plan(in(acrobot101, 600)), plain(K_LATENCY, 600, 39424, 3));
    // (not clamped by LDS residency: two workgroups of 75 KB fit a CU, cu_expect says four)
    check("acrobot T=201 B=1024 auto", solve_plan(in(acrobot201, 1024)), plain(K_LATENCY, 1024, 75424, 4));
    i = in(acrobot101, 1024); i.role_slots = false;
    check("acrobot T=101 B=1024 ILQR_ROLE_SLOTS=0", solve_plan(i), plain(K_LATENCY, 1024, 39424));
    check("synth12 T=101 B=1024 auto (no role table)", solve_plan(in(synth12, 1024)), plain(K_LATENCY, 1024, 25008));

    // ---- small model, B > #SIMDs: the packed kernel; two waves per pack where two chunk buffers fit at per_cu = ceil(packs / CUs)
    // car, 1024 packs on 256 CUs: 4 per CU x (22736 + 512) <= 160 KiB. Hand-over by head count (live = min(1024, B / 4)), the
    // queue handed to the kernel, every workgroup resident: marks on
    check("car T=51 B=4096 auto (round 6)", solve_plan(in(car51, 4096)),
          {K_PACKED2, 1024, 22736, 0, 1024, true, true, 6, 1, 0, 28624, true, 4, true});
    // acrobot at 8192: 8 packs per CU, two-wave form out; one-wave form, 1024 workgroups of two packs. The latency solver's 39 KB
    // beside the packs still leaves 4 workgroups per CU: the pool goes with it (control words at 39424 B), all resident, marks on
    check("acrobot T=101 B=8192 auto", solve_plan(in(acrobot101, 8192)),
          {K_PACKED1, 1024, 39424 + 64, 0, 1024, true, true, 6, 1, 39424 / 8, 39424, false, 0, true});
    // T=201: 75 KB would leave 2 workgroups per CU: no pool for the kernel (the queue is zeroed; control words behind the packs)
    check("acrobot T=201 B=8192 auto", solve_plan(in(acrobot201, 8192)),
          {K_PACKED1, 1024, 28960 + 64, 0, 1024, true, false, 6, 1, 28960 / 8, 75424, false, 0, true});
    // one round more than the chip holds (B = 8200: 1025 workgroups): nobody marked, no CU vacated
    check("acrobot T=101 B=8200 auto", solve_plan(in(acrobot101, 8200)),
          {K_PACKED1, 1025, 39424 + 64, 0, 1024, true, true, 0, 0, 39424 / 8, 39424, false, 0, true});
    // packs of 50 KB: 3 one-wave workgroups per CU (768 resident), with the pool or without: marks on at 512 workgroups, off at 1024
    check("50 KB packs B=4096 variant 5", solve_plan(in(bigpack, 4096, 5)),
          {K_PACKED1, 512, 50064, 0, 1024, true, true, 6, 1, 50000 / 8, 39424, false, 0, true});
    check("50 KB packs B=8192 auto", solve_plan(in(bigpack, 8192)),
          {K_PACKED1, 1024, 50064, 0, 1024, true, true, 0, 0, 50000 / 8, 39424, false, 0, true});
    // 100 KB two-wave workgroups: one per CU fits (per_cu 1), two do not (per_cu 2)
    check("100 KB two-wave B=1024 variant 6", solve_plan(in(bigpack, 1024, 6)),
          {K_PACKED2, 256, 100000, 0, 256, true, true, 6, 1, 0, 39424, true, 1, true});
    check("100 KB two-wave B=2048 auto", solve_plan(in(bigpack, 2048)),
          {K_PACKED1, 256, 50064, 0, 512, true, true, 6, 1, 50000 / 8, 39424, false, 0, true});
    // the two-wave form without role slots
    i = in(car51, 4096); i.role_slots = false;
    check("car T=51 B=4096 ILQR_ROLE_SLOTS=0", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 1024, true, true, 6, 1, 0, 28624, false, 0, true});

    // ---- a horizon beyond the LDS: the packed kernel for every variant (no hand-over: the latency kernel cannot take it), an
    // LDS error where the model has none
    for (int v = 0; v <= 6; ++v) {
        char what[64];
        std::snprintf(what, sizeof what, "acrobot T=501 B=1024 variant %d", v);
        check(what, solve_plan(in(acrobot501, 1024, v)), v == 5 ? Want{K_PACKED1, 128, 28960 + 64, 0, 0, false, false, 0, 0, 28960 / 8, 0, false, 0, false}
                                                                 : Want{K_PACKED2, 256, 28912, 0, 0, false, false, 0, 0, 0, 0, true, 1, false});
    }
    check("acrobot T=501 B=8192 auto", solve_plan(in(acrobot501, 8192)), {K_PACKED1, 1024, 28960 + 64, 0, 0, false, false, 0, 0, 28960 / 8, 0, false, 0, false});
    for (int v : {0, 1, 2, 4}) {
        i = in(synth12, 4096, v); i.lds_fits = false;
        check("synth12, horizon beyond the LDS", solve_plan(i), error());
        check("synth12, horizon beyond the LDS (stage)", stage_plan(i), error());
    }

    // ---- large models: one wave per instance (mid) beyond 2 x #SIMDs, where the model has it
    check("synth12 T=101 B=4096 auto (round 6)", solve_plan(in(synth12, 4096)), plain(K_MID, 4096, 25008));
    check("synth12 T=101 B=2048 auto", solve_plan(in(synth12, 2048)), plain(K_LATENCY, 2048, 25008));
    check("synth12 T=101 B=2049 auto", solve_plan(in(synth12, 2049)), plain(K_MID, 2049, 25008));
    check("synth12 T=101 B=16 variant 4", solve_plan(in(synth12, 16, 4)), plain(K_MID, 16, 25008));
    check("synth12 T=101 B=4096 variant 1", solve_plan(in(synth12, 4096, 1)), plain(K_LATENCY, 4096, 25008));
    check("synth32 T=101 B=4096 auto", solve_plan(in(synth32, 4096)), plain(K_LATENCY, 4096, 61440));
    check("synth32 T=101 B=512 auto", solve_plan(in(synth32, 512)), plain(K_LATENCY, 512, 61440));
    // a small model without the packed kernel: the throughput kernel beyond #SIMDs
    check("no packed kernel B=4096 auto", solve_plan(in(nopack, 4096)), plain(K_SLIM, 4096, 20352));

    // ---- both sides of auto's boundaries at 256 CUs (S = 1024 SIMDs), as tests/test_gpu_parity.py::test_auto_boundary_kernels_against_the_oracle
    // solves them on the device: acrobot T=51 at S | S + 1 (latency | packed, two waves per pack: 257 packs, 2 per CU, live = B / 4),
    // car T=51 at 16 C | 16 C + 4 (per-CU packs 4 -> 5: the one-wave form, 513 workgroups, the pool with the latency solver's 28 KB
    // beside the packs at 4 workgroups per CU, all resident) and synth12 at 2 S | 2 S + 1 (rows above: latency | mid)
    check("acrobot T=51 B=1024 auto (S)", solve_plan(in(acrobot51, 1024)), plain(K_LATENCY, 1024, 21424, 4));
    check("acrobot T=51 B=1025 auto (S + 1)", solve_plan(in(acrobot51, 1025)),
          {K_PACKED2, 257, 28912, 0, 256, true, true, 6, 1, 0, 21424, true, 2, true});
    check("car T=51 B=4100 auto (16 C + 4)", solve_plan(in(car51, 4100)),
          {K_PACKED1, 513, 28624 + 64, 0, 1024, true, true, 6, 1, 28624 / 8, 28624, false, 0, true});

    // ---- explicit variants, acrobot T=101 at 1024 (hand-over by head count: live = 256)
    check("acrobot T=101 B=1024 variant 1", solve_plan(in(acrobot101, 1024, 1)), plain(K_LATENCY, 1024, 39424, 4));
    check("acrobot T=101 B=1024 variant 2", solve_plan(in(acrobot101, 1024, 2)), plain(K_SLIM, 1024, 20352));
    check("acrobot T=101 B=1024 variant 3", solve_plan(in(acrobot101, 1024, 3)),
          {K_PACKED2, 256, 28912, 0, 256, true, true, 6, 1, 0, 39424, true, 1, true});
    check("acrobot T=101 B=1024 variant 4 (no such kernel)", solve_plan(in(acrobot101, 1024, 4)), plain(K_LATENCY, 1024, 39424, 4));
    check("acrobot T=101 B=1024 variant 5", solve_plan(in(acrobot101, 1024, 5)),
          {K_PACKED1, 128, 39424 + 64, 0, 256, true, true, 6, 1, 39424 / 8, 39424, false, 0, true});
    check("acrobot T=101 B=1024 variant 6", solve_plan(in(acrobot101, 1024, 6)),
          {K_PACKED2, 256, 28912, 0, 256, true, true, 6, 1, 0, 39424, true, 1, true});
    check("acrobot T=101 B=8192 variant 6 (does not fit)", solve_plan(in(acrobot101, 8192, 6)),
          {K_PACKED1, 1024, 39424 + 64, 0, 1024, true, true, 6, 1, 39424 / 8, 39424, false, 0, true});
    check("acrobot T=101 B=8192 variant 1", solve_plan(in(acrobot101, 8192, 1)), plain(K_LATENCY, 8192, 39424, 4));
    check("acrobot T=101 B=8192 variant 2", solve_plan(in(acrobot101, 8192, 2)), plain(K_SLIM, 8192, 20352));

    // ---- hand-over settings (car T=51 B=4096)
    check("car B=100 variant 6: live = B / 4", solve_plan(in(car51, 100, 6)), {K_PACKED2, 25, 22736, 0, 25, true, true, 6, 1, 0, 28624, true, 1, true});
    i = in(car51, 4096); i.constrained = false;
    check("car B=4096 unconstrained: no hand-over", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 0, false, false, 0, 0, 0, 0, true, 4, false});
    i = in(car51, 4096); i.handover = 0;
    check("car B=4096 hand-over off", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 0, false, false, 0, 0, 0, 0, true, 4, false});
    i = in(car51, 4096); i.handover_live = 10;
    check("car B=4096 live 10", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 10, true, true, 6, 1, 0, 28624, true, 4, true});
    i = in(car51, 4096); i.handover_live = 0;
    check("car B=4096 live 0", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 0, false, false, 0, 0, 0, 0, true, 4, false});
    i = in(car51, 4096); i.handover_mark = 3;
    check("car B=4096 mark 3", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 1024, true, true, 3, 1, 0, 28624, true, 4, true});
    i = in(car51, 4096); i.handover_mark = 0;
    check("car B=4096 mark 0", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 1024, true, true, 0, 1, 0, 28624, true, 4, true});
    i = in(car51, 4096); i.handover = 3;        // by outer iteration: no head count, nobody marked
    check("car B=4096 hand-over at outer 3", solve_plan(i), {K_PACKED2, 1024, 22736, 3, 0, true, true, 0, 1, 0, 28624, true, 4, true});
    i = in(car51, 4096); i.handover = 11;
    check("car B=4096 hand-over beyond max_dual_updates", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 0, false, false, 0, 0, 0, 0, true, 4, false});
    i = in(acrobot101, 8192); i.handover = 3;
    check("acrobot B=8192 hand-over at outer 3", solve_plan(i), {K_PACKED1, 1024, 39424 + 64, 3, 0, true, true, 0, 1, 39424 / 8, 39424, false, 0, true});
    i = in(car51, 4096); i.pool = false;
    check("car B=4096 without a queue", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 1024, false, false, 0, 0, 0, 0, true, 4, true});
    i = in(car51, 4096); i.done_counter = false;
    check("car B=4096 without a counter", solve_plan(i), {K_PACKED2, 1024, 22736, 0, 0, false, false, 0, 0, 0, 0, true, 4, false});

    // ---- stage kernels: the variant's mapping where the model has it
    check("acrobot stage variant 0", stage_plan(in(acrobot101, 1024)), plain(K_STAGE, 1024, 39424));
    check("acrobot stage variant 2", stage_plan(in(acrobot101, 1024, 2)), plain(K_STAGE_SLIM, 1024, 20352));
    check("acrobot stage variant 4", stage_plan(in(acrobot101, 1024, 4)), plain(K_STAGE, 1024, 39424));
    check("acrobot stage variant 6", stage_plan(in(acrobot101, 8192, 6)), plain(K_STAGE, 8192, 39424));
    check("synth12 stage variant 4", stage_plan(in(synth12, 4096, 4)), plain(K_STAGE_MID, 4096, 25008));
    check("synth12 stage variant 0", stage_plan(in(synth12, 4096)), plain(K_STAGE, 4096, 25008));
    check("synth12 stage variant 2", stage_plan(in(synth12, 4096, 2)), plain(K_STAGE, 4096, 25008));
    check("acrobot T=501 stage", stage_plan(in(acrobot501, 1024, 6)), error());

    std::printf("%d rows checked\n", rows);
    return 0;
}
