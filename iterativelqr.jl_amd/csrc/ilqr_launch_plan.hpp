// Which kernel a solve or stage launch runs on, and with what grid, LDS, hand-over, pool and role settings: the one statement of
// the rule. ilqr_solve, ilqr_run_stage_param and ilqr_resolved_kernel_variant (ilqr_api.hip) read their launch off it; the model
// module's launchers (ilqr_device.hpp: ModelModule::launch) only launch. Plain C++ (no HIP) like ilqr_ric_schedule.hpp, so that
// the host-side test pins its decisions (tests/test_launch_plan.py).
#pragma once
#include <cstddef>

namespace ilqr {

// the kernels of a model module (ilqr_model_vtable::launch, bit k of ilqr_model_vtable::kernels); 1-6 are the numbers of
// ilqr_set_kernel_variant / ilqr_resolved_kernel_variant
enum Kernel { K_LATENCY = 1, K_SLIM = 2, K_MID = 4, K_PACKED1 = 5, K_PACKED2 = 6, K_RESUME = 7, K_STAGE = 8, K_STAGE_SLIM = 9, K_STAGE_MID = 10 };
enum { LDS_CU = 160 * 1024, PK_CTL_BYTES = 64 };   // LDS of a CU; the one-wave packed form's control words (ilqr_device_packed.hpp: CTL_WORDS ints)

// workgroups of `bytes` of LDS that a CU holds (512-byte allocation granule), at most four
constexpr int lds_per_cu(size_t bytes) { const size_t k = LDS_CU / ((bytes + 511) & ~(size_t)511); return k < 4 ? (int)k : 4; }
// the packed kernel's two-wave form fits: its workgroups' LDS at per_cu workgroups per CU
constexpr bool packed2_fits(int lds2_bytes, int per_cu) { return lds2_bytes > 0 && per_cu >= 1 && per_cu <= 4 && (long long)per_cu * (lds2_bytes + 512) <= LDS_CU; }

struct LaunchIn {
    int variant;                  // ilqr_set_kernel_variant: 0 auto, 1-6
    int B, num_simds;             // batch; 4 x the device's CUs
    bool lds_fits;                // the LDS-resident kernels hold this horizon
    size_t lds_bytes, slim_lds_bytes;             // LDS of a workgroup of the latency / large kernels; of the throughput kernel
    unsigned kernels;                             // bit k: the model has kernel k
    int packed1_lds_bytes, packed2_lds_bytes;     // packed kernel: a one-wave workgroup's two chunk buffers; a two-wave workgroup
    bool constrained;
    int max_dual_updates;
    int handover, handover_live, handover_mark;   // ilqr_set_handover / _live / _mark (-1 auto)
    bool done_counter, pool, cu_slots;            // the handle has these buffers
    bool role_slots;                              // ILQR_ROLE_SLOTS is not 0
};

struct LaunchPlan {
    int kernel = 0;               // 0: no kernel of the model holds this horizon (ILQR_ERR_LDS)
    int grid = 0;
    size_t lds = 0;               // dynamic LDS bytes
    int handover_outer = 0, handover_live = 0;    // (handover_live > 0: the host zeroes done_counter)
    bool zero_pool = false;       // the host zeroes the hand-over queue: its counts are this solve's
    bool pool = false;            // ... and the kernel gets it
    int pool_mark = 0, pool_cu = 0, pool_ctl = 0, pool_lds = 0;
    bool role_slots = false;      // the host zeroes cu_slots and the kernel gets them
    int cu_expect = 0;
    bool resume = false;          // a resume launch of the latency kernel follows (grid B, lds_bytes)
};

inline LaunchPlan solve_plan(const LaunchIn& in) {
    LaunchPlan p;
    const auto has = [&](int k) { return (in.kernels >> k & 1u) != 0; };
    const int v = in.variant, cus = in.num_simds / 4 > 1 ? in.num_simds / 4 : 1;
    const bool beyond = v == 0 && in.B > in.num_simds;      // auto, and the batch does not fit one instance per SIMD
    // auto: the latency kernel while the batch fits the chip (one instance per SIMD); larger batches take the packed kernel (four
    // instances per wave, workspace streamed from HBM / L2) when the model has one (nx, nu <= 4), the throughput kernel otherwise.
    // Horizons whose LDS-resident set exceeds 160 KiB run on the packed kernel only.
    if (has(K_PACKED1) && (v == 3 || v == 5 || v == 6 || !in.lds_fits || beyond)) {
        // straggler hand-over: the survivors of a batch leave the packed kernel and are finished by the latency kernel (two waves
        // per instance, LDS-resident state; a rejected line-search trial costs it one rollout where it costs the packed kernel a
        // whole cycle of the wave) in a launch that follows on the stream. By head count (the default) — once no more than `live`
        // instances of the batch are still running, each of them leaves at the next head of an inner or outer iteration;
        // auto: live = min(1024, B / 4), what the latency kernel holds at full speed. By outer iteration (ilqr_set_handover(k >= 2))
        // — an instance entering outer iteration k leaves at that boundary. Both kernels do the same arithmetic, so which
        // instances change kernels, and when, never shows in a result.
        // (Measured and dropped: a pool of latency workgroups BESIDE the packed kernel taking leavers from a device queue — at
        // 8192 instances the packed kernel's 2048 waves fill every CU, a pool workgroup only starts once they retire)
        const bool can = in.constrained && in.lds_fits && in.done_counter;
        const int ho = in.handover < 0 ? 0 : in.handover;
        p.handover_outer = can && ho >= 2 && ho <= in.max_dual_updates ? ho : 0;
        p.handover_live = !can || in.handover >= 0 ? 0 : in.handover_live >= 0 ? in.handover_live : (in.B / 4 < 1024 ? in.B / 4 : 1024);
        p.resume = p.handover_outer > 0 || p.handover_live > 0;
        p.zero_pool = p.resume && in.pool;
        // two waves per pack (a linearisation server beside the solver wave) while the batch leaves every SIMD at most two waves and
        // a CU's LDS holds the second chunk buffers: up to 4 workgroups per CU (variant 5 = one wave per pack, 6 = two where they fit)
        const int packs = (in.B + 3) / 4, per_cu = (packs + cus - 1) / cus;
        int resident;                 // workgroups of the launch resident at once
        if (v != 5 && packed2_fits(in.packed2_lds_bytes, per_cu)) {
            p.kernel = K_PACKED2; p.grid = packs; p.lds = (size_t)in.packed2_lds_bytes;
            p.pool = p.zero_pool;
            resident = packs;         // (packed2_fits: per_cu workgroups on every CU)
            // one solver wave per SIMD (KArgs::cu_slots)
            p.role_slots = in.cu_slots && in.role_slots;
            p.cu_expect = p.role_slots ? (per_cu < 4 ? per_cu : 4) : 0;
        } else {
            // one-wave form: two packs per workgroup (four workgroups of 256-register waves per CU); it finishes the instances handed
            // over itself (ilqr_device_packed.hpp: solve_kernel_packed) with the pool where the latency solver's LDS fits without
            // costing residency
            p.kernel = K_PACKED1; p.grid = (packs + 1) / 2;
            size_t bufs = (size_t)in.packed1_lds_bytes;
            const size_t with_pool = bufs > in.lds_bytes ? bufs : in.lds_bytes;
            if (p.zero_pool && lds_per_cu(with_pool + PK_CTL_BYTES) >= lds_per_cu(bufs + PK_CTL_BYTES)) { bufs = with_pool; p.pool = true; }
            p.pool_ctl = (int)(bufs / sizeof(double));
            p.lds = bufs + PK_CTL_BYTES;
            resident = lds_per_cu(p.lds) * cus;
        }
        if (p.zero_pool) {
            // under the head-count rule an instance whose rejected line-search trials exceed the batch's mean by `mark` leaves at
            // once, and gets its CU to itself (config 4, shard 6: 126.6 -> 118.0 ms) — while every workgroup of the launch is
            // resident: otherwise a workgroup that waits holds the slots the next round needs, so nobody is marked, no CU is vacated
            // and an idle worker leaves as soon as the queue is empty (and the batch's mean says nothing while part of it has not started)
            p.pool_lds = (int)in.lds_bytes;
            p.pool_cu = p.grid <= resident;
            p.pool_mark = p.pool_cu && p.handover_live > 0 ? (in.handover_mark < 0 ? 6 : in.handover_mark) : 0;
        }
        return p;
    }
    if (!in.lds_fits) return p;
    p.grid = in.B; p.lds = in.lds_bytes;
    if (has(K_SLIM) && (v == 2 || beyond)) {
        p.kernel = K_SLIM; p.lds = in.slim_lds_bytes;
    } else if (has(K_MID) && (v == 4 || (v == 0 && in.B > 2 * in.num_simds))) {
        // Large models whose matrices are single tiles (nx, nu <= 16): the four-wave kernel holds 2 instances per CU, the one-wave
        // kernel SIX (248 VGPRs and 25 KB of LDS per wave: profiles/r04_synth12_b4096_mid_rocprofv3.txt). An instance alone is
        // faster on four waves (its windows run their tiles side by side: 3.9 k against 5.3 k clk per Riccati step on synth12, the
        // rollout beside the sensitivity sweep instead of behind it), so auto takes one wave per instance only where residency
        // wins: beyond 8 instances per CU the four-wave kernel works in more than four rounds (tools/mid_bench.py: equal at 2048
        // instances on 256 CUs, 1.28x at 4096, 1.47x at 8192).
        p.kernel = K_MID;
    } else {
        // two-wave latency kernel (four waves for large models): one critical wave per SIMD (KArgs::cu_slots; ILQR_ROLE_SLOTS=0
        // leaves the roles as launched: A/B runs)
        p.kernel = K_LATENCY;
        p.role_slots = in.cu_slots && in.role_slots;
        const int per_cu = (in.B + cus - 1) / cus;
        p.cu_expect = p.role_slots ? (per_cu < 4 ? per_cu : 4) : 0;
    }
    return p;
}

// a stage kernel (ilqr_run_stage_param) runs in the mapping selected by ilqr_set_kernel_variant: 2 = throughput (one wave per
// instance), 4 = one wave per instance of a large model, the latency kernel's otherwise; all of them LDS-resident
inline LaunchPlan stage_plan(const LaunchIn& in) {
    LaunchPlan p;
    if (!in.lds_fits) return p;
    p.kernel = K_STAGE; p.grid = in.B; p.lds = in.lds_bytes;
    if (in.variant == 2 && (in.kernels >> K_STAGE_SLIM & 1u)) { p.kernel = K_STAGE_SLIM; p.lds = in.slim_lds_bytes; }
    else if (in.variant == 4 && (in.kernels >> K_STAGE_MID & 1u)) p.kernel = K_STAGE_MID;
    return p;
}

}  // namespace ilqr
