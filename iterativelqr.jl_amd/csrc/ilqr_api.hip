// C-ABI implementation (include/ilqr_hip.h): handle management, HBM workspace,
// kernel launches on a private HIP stream, host<->device accessors.
// No CPU fallback: without a HIP device ilqr_create fails loudly.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ilqr_device.hpp"
#include "ilqr_host.hpp"

namespace ilqr {
// fresh-solver defaults after the workspace has been zero-filled:
// objective = Inf, step_size = 1 (src/data/solver.jl:37-39), ρ = 1, a = 1
// (src/augmented_lagrangian.jl:17-22).
__global__ void defaults_kernel(KArgs a) {
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const Layout& L = a.L;
    double* g = a.ws + (size_t)b * (size_t)L.stride;
    for (int i = threadIdx.x; i < L.C; i += blockDim.x) { g[L.rho + i] = 1.0; g[L.act + i] = 1.0; }
    if (threadIdx.x == 0) {
        g[L.scal + S_OBJECTIVE] = __builtin_huge_val();
        g[L.scal + S_STEP_SIZE] = 1.0;
    }
}

// ilqr_reset of an HBM-resident (large) model in ONE pass: zero the instance block except [keep_lo, keep_hi) — the full
// Jacobian / Hessian / value mirrors, rewritten or zeroed on demand — with 16-byte coalesced stores, then the fresh-solver
// defaults. (Two pitched hipMemset2DAsync calls took 0.43 ms per reset for 512 synth32 instances, a tenth of a BASELINE step.)
__global__ __launch_bounds__(256) void reset_large_kernel(KArgs a, int keep_lo, int keep_hi) {
    const int b = blockIdx.x / 8, part = blockIdx.x % 8;
    if (b >= a.B) return;
    const Layout& L = a.L;
    double2* g = reinterpret_cast<double2*>(a.ws + (size_t)b * (size_t)L.stride);
    const int lo2 = keep_lo / 2, hi2 = (keep_hi + 1) / 2, n2 = L.stride / 2;          // offsets are even (pad2), the stride a multiple of 16
    const int Cp = pad2(L.C);
    // the blocks of an instance run in any order: the ranges that get defaults (rho, act, scalars) are left to part 0 alone
    auto special = [&](int i) {
        const int d = 2 * i;
        return (d >= L.rho && d < L.rho + Cp) || (d >= L.act && d < L.act + Cp) || (d >= L.scal && d < L.scal + S_COUNT);
    };
    for (int i = part * 256 + threadIdx.x; i < n2; i += 8 * 256)
        if ((i < lo2 || i >= hi2) && !special(i)) g[i] = double2{0.0, 0.0};
    if (part == 0) {
        double* gd = a.ws + (size_t)b * (size_t)L.stride;
        for (int i = threadIdx.x; i < Cp; i += blockDim.x) { gd[L.rho + i] = i < L.C ? 1.0 : 0.0; gd[L.act + i] = i < L.C ? 1.0 : 0.0; }
        for (int i = threadIdx.x; i < S_COUNT; i += blockDim.x)
            gd[L.scal + i] = i == S_OBJECTIVE ? __builtin_huge_val() : (i == S_STEP_SIZE ? 1.0 : 0.0);
    }
}

}  // namespace ilqr

namespace {

thread_local std::string g_err;

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ILQR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)
// the same for a call that returns one of this file's own codes (and has set the error text)
#define ILQR_TRY(expr) do { const int rc_ = (expr); if (rc_ != ILQR_OK) return rc_; } while (0)

std::vector<const ilqr_model_vtable*>& registry() {
    static std::vector<const ilqr_model_vtable*> r;
    return r;
}
// compiled nonlinear sensors (ilqr_compile_sensor): a registry of their own, a sensor belongs to no model
std::vector<const ilqr_sensor_vtable*>& sensor_registry() {
    static std::vector<const ilqr_sensor_vtable*> r;
    return r;
}
const ilqr_sensor_vtable* find_sensor(const char* name) {
    for (auto* sv : sensor_registry())
        if (name && !std::strcmp(sv->name, name)) return sv;
    return nullptr;
}

// the kernels model modules register beside their vtables (ilqr_register_model_ext), by the vtable's name
std::vector<const ilqr_model_ext*>& ext_registry() {
    static std::vector<const ilqr_model_ext*> r;
    return r;
}
const ilqr_model_ext* find_ext(const char* name) {
    for (auto* e : ext_registry())
        if (name && !std::strcmp(e->name, name)) return e;
    return nullptr;
}

struct BufferDesc { const char* name; int offset; int len; };

}  // namespace

// what ilqr_host.hpp promises the model compiler (ilqr_model_compile.cpp)
int ilqr::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
const ilqr_model_vtable* ilqr::find_model(const char* name) {
    for (auto* vt : registry())
        if (!std::strcmp(vt->name, name)) return vt;
    return nullptr;
}
long long ilqr::model_abi_word() { return ILQR_MODEL_ABI_VERSION * 1000 + (long long)sizeof(ilqr::KArgs); }
bool ilqr::sensor_registered(const char* name) { return find_sensor(name) != nullptr; }
long long ilqr::sensor_abi_word() { return ILQR_SENSOR_ABI_VERSION * 1000 + (long long)sizeof(ilqr::SensorNlArgs); }
using ilqr::fail;
using ilqr::find_model;

// the stages (ilqr_handle::Stage) of ilqr_handle::pol, ::cand, ::shift, ::samp and ::plant by name
enum { POL_X1, POL_W, POL_COST, POL_VIOL, POL_NONFINITE, POL_X, POL_U, POL_STAGES };
enum { CAND_U, CAND_COST, CAND_VIOL, CAND_NONFINITE, CAND_CHOSEN, CAND_STAGES };
enum { SHIFT_X1, SHIFT_W_TAIL, SHIFT_W_STAGE, SHIFT_STAGES };
enum { SAMP_WEIGHTS, SAMP_U_OUT, SAMP_SIGMA, SAMP_STAGES };
enum { PLANT_X, PLANT_W, PLANT_X_OUT, PLANT_U_OUT, PLANT_NONFINITE, PLANT_LOG, PLANT_W_PREVIEW, PLANT_COST, PLANT_VIOL, PLANT_SATURATED, PLANT_XC,
       PLANT_Y, EST_P, EST_Y, EST_INNOVATION, EST_NIS, EST_FIRST_BAD, EST_XHAT_CL, EST_PDIAG_CL, EST_NIS_CL, SENS_H, SENS_R, SENS_SIGMA, SENS_YHAT, SENS_S,
       SENS_XLIN, SENS_XPRIOR, SENS_X0, SENS_P0, PCOV_SDIAG, PCOV_UDIAG, PCOV_SIGMA, PCOV_POUT, PLANT_STAGES };

struct ilqr_handle {
    const ilqr_model_vtable* vt;
    ilqr::Layout L;
    int B, device, constrained;
    ilqr_options opt;
    double* ws;
    size_t ws_bytes, lds_bytes;
    hipStream_t stream;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timing;
    double* d_x1;
    double* d_u;   // staging for host-pointer initialize_rollout
    double* trace;
    int trace_cap;
    int handover;         // straggler hand-over of the packed kernel: -1 auto (by head count), 0 off, k > 1 = instances entering outer iteration k
    int handover_live;    // head-count rule: survivors of the batch at which they all leave (-1 auto, 0 off)
    int* done_counter;    // device counter of finished instances for that rule
    int* pool;            // one-wave form of the packed kernel: queue of handed-over instances its workgroups finish themselves (POOL_Q + B ints)
    int handover_mark;    // rejected line-search trials above the batch's mean at which an instance is marked a straggler (-1 auto, 0 never)
    int* cu_slots = nullptr;   // latency kernel: critical waves per SIMD (ilqr::KArgs::cu_slots), CU_SLOT_CUS x 4 counters
    bool pool_valid = false;   // the queue words hold the counts of THIS handle's last solve (false after a solve that did not use the queue)
    int variant;          // 0 auto, 1 latency kernel (all-LDS, 2 waves per instance; large models: four waves per instance), 2 throughput kernel (slim), 3 packed kernel (4 instances per wave, no LDS), 4 one wave per instance of a large model with nx, nu <= 16
    bool lds_fits;        // the LDS-resident kernels can hold this horizon (otherwise only the packed kernel runs it)
    int num_simds;
    double* qv;           // optional action-value buffers Qx, Qu, Qxx, Quu, Qux (allocated on first use by a getter)
    ilqr::QLayout QL;
    // large (HBM-resident) models: the kernels stream a COMPACT form of the Jacobians and Hessians (Layout::fv, ::hc, see
    // ilqr_device_large.hpp); the reference's full jacobian_* / hessian_* arrays are a mirror written on demand
    bool full_stale;      // the full fx, fu, gxx, guu, gux arrays do not reflect the compact form (a getter materialises them first)
    bool P_dirty;         // P, p hold pre-reset values (only the backward-pass STAGE kernel writes them): zeroed lazily
    std::vector<BufferDesc> buffers;
    std::vector<BufferDesc> qbuffers;
    // ilqr_create_sharded: this handle owns no device memory itself but one sub-handle per entry of the device list, each with
    // its own contiguous range of instances [lo[i], lo[i] + shards[i]->B), workspace and stream on its device
    std::vector<ilqr_handle*> shards;
    std::vector<int> lo;
    // ilqr_set_stage_selectors: the one-hot selector table [T][n_sel] of a lowered problem (distinct per-step objects); it occupies
    // the LAST n_sel parameter columns of every instance, the caller's ilqr_set_parameters fills the first nw - n_sel
    std::vector<double> sel;
    int n_sel = 0;
    // a device buffer of the MPC-side entry points that grows on demand (grow()) and is reused by later calls
    struct Stage { void* p = nullptr; size_t cap = 0; };
    // ilqr_rollout_policy: K, k hold a policy (a solve, a backward-pass stage or a host write of K / k since the last reset), and the
    // device staging of its host form
    bool has_policy = false;
    Stage pol[POL_STAGES];
    // ilqr_initialize_rollout_candidates: the device staging of the candidates' u (host form) and of the scores — the host form's
    // outputs, and the handle's own buffers for the scores a caller did not ask for. ilqr_sample_rollout_candidates scores into
    // the same four.
    Stage cand[CAND_STAGES];
    // ilqr_shift_horizon: the device staging of x1 and w_tail (host form) and of the shifted parameters θ' of the whole batch,
    // which are read out of the workspace before a second launch writes them back
    Stage shift[SHIFT_STAGES];
    // ilqr_sample_rollout_candidates: the device staging of the weights (host form, and a blend whose caller does not ask for
    // them), of the candidates as drawn (host form) and of sigma, with the host copy of sigma the asynchronous upload reads
    Stage samp[SAMP_STAGES];
    std::vector<double> sample_sigma;
    // ilqr_shift_duals / ilqr_solve_warm: λ, ρ hold the duals of a solve (a constrained solve, the AL_BEGIN stage or a host write of
    // constraint_penalty since the last reset) — after a reset ρ is not a penalty ladder's and a warm solve would be refused
    bool has_duals = false;
    // ilqr_plant_step: the device staging of its host form (the plant state in and out, w_plant, x_out, u_out, first_nonfinite);
    // ilqr_mpc_run: the plant state, w_plant, the closed-loop trajectory, the log and first_nonfinite of the whole run;
    // ilqr_mpc_run_preview: w_preview and the realised scores of the run too; ilqr_plant_score: its host form (x, u and w_plant in
    // the stages of x_out, u_out and w_plant, the two scores in their own); ilqr_plant_step_limited: the saturation counts too;
    // ilqr_plant_measure: x in the stage of the plant state, y in its own; ilqr_mpc_run_io: the controller's state xc, what it was
    // given per period (y_cl, in the stage of y) and the saturation counts of the run; ilqr_estimate_predict / _update: the estimate in
    // the stage of xc, y in its own, the covariance, the innovation, nis and first_bad; ilqr_mpc_run_est: the covariance, the period's
    // measurement and nis, and the three per-period logs of the filter; ilqr_estimate_update_linear / ilqr_plant_measure_linear /
    // ilqr_mpc_run_sensor: H, r, sigma_y and ŷ; ilqr_sensor_linearise / ilqr_plant_measure_sensor / ilqr_estimate_update_sensor /
    // ilqr_mpc_run_nlsensor: the sensor parameters s, the point of linearisation and the prior of its host form, the Jacobians H
    // [B][ny][nx] and ŷ the update reads (in the stages of H and ŷ), and the prior (x̂₀, P₀) of the iterated filter;
    // ilqr_plan_covariance: P0 in the stage of the covariance, first_nonfinite in its own, sdiag, udiag, sigma and P_out
    Stage plant[PLANT_STAGES];
};

namespace {

bool has_kernel(const ilqr_model_vtable* vt, int k) { return (vt->kernels >> k & 1u) != 0; }

ilqr::KArgs make_args(const ilqr_handle* h) {
    ilqr::KArgs a;
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.constrained = h->constrained; a.stage = 0; a.opt = h->opt;
    a.x1 = nullptr; a.u_in = nullptr;
    a.trace = h->trace; a.trace_cap = h->trace_cap;
    a.qv = h->qv; a.QL = h->QL;
    a.stage_param = 0.0; a.stage_flag = 0;
    a.handover_outer = 0; a.resume = 0; a.handover_live = 0; a.done_counter = h->done_counter;
    a.pool = nullptr; a.pool_mark = 0; a.pool_lds = 0; a.pool_ctl = 0; a.pool_cu = 0; a.cu_slots = nullptr; a.cu_expect = 0;
    a.warm_duals = 0;
    return a;
}

void fill_buffers(ilqr_handle* h) {
    const ilqr::Layout& L = h->L;
    const int T = L.T, N = T - 1, n = L.nx, m = L.nu;
    h->buffers = {
        {"nominal_states", L.xb, T * n}, {"nominal_actions", L.ub, N * m},
        {"states", L.x, T * n}, {"actions", L.u, N * m},
        {"jacobian_state", L.fx, N * n * n}, {"jacobian_action", L.fu, N * n * m},
        {"gradient_state", L.gx, T * n}, {"gradient_action", L.gu, N * m},
        {"hessian_state_state", L.gxx, T * n * n}, {"hessian_action_action", L.guu, N * m * m},
        {"hessian_action_state", L.gux, N * m * n},
        {"K", L.K, N * m * n}, {"k", L.k, N * m}, {"P", L.P, T * n * n}, {"p", L.p, T * n},
        {"gradient_state_lagrangian", L.Lx, N * n}, {"gradient_action_lagrangian", L.Lu, N * m},
        {"violations", L.c, L.C}, {"constraint_dual", L.lam, L.C},
        {"constraint_penalty", L.rho, L.C}, {"active_set", L.act, L.C},
        {"parameters", L.w, T * L.nw},
        {"_scalars", L.scal, ilqr::S_COUNT},
    };
    const ilqr::QLayout& Q = h->QL;
    h->qbuffers = {
        {"Qx", Q.Qx, N * n}, {"Qu", Q.Qu, N * m}, {"Qxx", Q.Qxx, N * n * n}, {"Quu", Q.Quu, N * m * m}, {"Qux", Q.Qux, N * m * n},
    };
}

const BufferDesc* find_qbuffer(const ilqr_handle* h, const char* name) {
    for (auto& b : h->qbuffers)
        if (!std::strcmp(b.name, name)) return &b;
    return nullptr;
}

// the deferred parts of ilqr_reset / of a solve on a large model (see ilqr_handle::full_stale / P_dirty)
int settle_reset(ilqr_handle* h) {
    const ilqr::Layout& L = h->L;
    const size_t pitch = (size_t)L.stride * 8;
    if (h->P_dirty) {
        HIP_TRY(hipMemset2DAsync((char*)h->ws + (size_t)L.P * 8, pitch, 0, (size_t)(L.scal - L.P) * 8, (size_t)h->B, h->stream));
        h->P_dirty = false;
    }
    return ILQR_OK;
}
// full jacobian_* / hessian_* arrays <- compact form (dir 0) or the reverse (dir 1)
int mirror(ilqr_handle* h, int dir) {
    if (!h->vt->launch_mirror) return ILQR_OK;
    ilqr::KArgs a = make_args(h);
    if (h->vt->launch_mirror(&a, dir, h->stream) != 0) return fail(ILQR_ERR_HIP, "mirror kernel launch failed");
    if (dir == 0) h->full_stale = false;
    return ILQR_OK;
}
bool is_mirrored(const ilqr_handle* h, const BufferDesc* bd) {
    return h->vt->launch_mirror != nullptr && bd->offset >= h->L.fx && bd->offset < h->L.P && bd->offset != h->L.ring;
}

const BufferDesc* find_buffer(const ilqr_handle* h, const char* name) {
    for (auto& b : h->buffers)
        if (!std::strcmp(b.name, name)) return &b;
    return nullptr;
}

int copy_out(ilqr_handle* h, const BufferDesc* bd, double* out) {
    if (bd->len == 0) return ILQR_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (bd->offset >= h->L.P && bd->offset < h->L.scal) { const int rc = settle_reset(h); if (rc != ILQR_OK) return rc; }
    if (is_mirrored(h, bd) && h->full_stale) { const int rc = mirror(h, 0); if (rc != ILQR_OK) return rc; }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy2D(out, (size_t)bd->len * 8, h->ws + bd->offset, (size_t)h->L.stride * 8,
                        (size_t)bd->len * 8, (size_t)h->B, hipMemcpyDeviceToHost));
    return ILQR_OK;
}

int copy_in(ilqr_handle* h, const BufferDesc* bd, const double* in) {
    if (bd->len == 0) return ILQR_OK;
    HIP_TRY(hipSetDevice(h->device));
    if (bd->offset >= h->L.P && bd->offset < h->L.scal) { const int rc = settle_reset(h); if (rc != ILQR_OK) return rc; }
    const bool mirrored = is_mirrored(h, bd);
    if (mirrored && h->full_stale) { const int rc = mirror(h, 0); if (rc != ILQR_OK) return rc; }     // the OTHER full arrays must be current before the gather below
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy2D(h->ws + bd->offset, (size_t)h->L.stride * 8, in, (size_t)bd->len * 8,
                        (size_t)bd->len * 8, (size_t)h->B, hipMemcpyHostToDevice));
    // any direct write may break states == nominal: drop the shortcut flag
    std::vector<double> zeros(h->B, 0.0);
    HIP_TRY(hipMemcpy2D(h->ws + h->L.scal + ilqr::S_STATES_EQ_NOMINAL, (size_t)h->L.stride * 8, zeros.data(), 8, 8,
                        (size_t)h->B, hipMemcpyHostToDevice));
    if (mirrored) {
        if (bd->offset == h->L.fx || bd->offset == h->L.fu) {       // host-written Jacobians count as evaluated
            std::vector<double> ones(h->B, 1.0);
            HIP_TRY(hipMemcpy2D(h->ws + h->L.scal + ilqr::S_JAC_VALID, (size_t)h->L.stride * 8, ones.data(), 8, 8, (size_t)h->B, hipMemcpyHostToDevice));
        }
        const int rc = mirror(h, 1);
        if (rc != ILQR_OK) return rc;
        // The kernels work on the compact rows: what the host wrote at a CONSTANT Jacobian position or outside the Hessian pattern
        // is not representable there and is dropped by the gather. The full arrays count as stale from here on, so that a getter
        // shows what the kernels will use (the constant, a structural zero), not what was written.
        h->full_stale = true;
    }
    return ILQR_OK;
}

// Sharded handles: run f(sub-handle, first instance of its range) for every shard. Launch-type calls are asynchronous and go
// one after the other from the calling thread; calls that move data (blocking copies) run on one host thread per device.
template <class F>
int each_shard(ilqr_handle* h, F f, bool threaded = false) {
    const size_t G = h->shards.size();
    if (!threaded || G == 1) {
        for (size_t i = 0; i < G; ++i) { const int rc = f(h->shards[i], (size_t)h->lo[i]); if (rc != ILQR_OK) return rc; }
        return ILQR_OK;
    }
    std::vector<int> rcs(G, ILQR_OK);
    std::vector<std::string> msgs(G);
    std::vector<std::thread> th;
    for (size_t i = 0; i < G; ++i)
        th.emplace_back([&, i] { rcs[i] = f(h->shards[i], (size_t)h->lo[i]); if (rcs[i] != ILQR_OK) msgs[i] = g_err; });
    for (auto& t : th) t.join();
    for (size_t i = 0; i < G; ++i)
        if (rcs[i] != ILQR_OK) return fail(rcs[i], "device " + std::to_string(h->shards[i]->device) + ": " + msgs[i]);
    return ILQR_OK;
}
#define SHARDED(h) ((h) && !(h)->shards.empty())

// the handle, or every shard of a sharded one, holds member m (has_policy, has_duals, d_x1, d_u)
template <class M> bool every_shard_holds(const ilqr_handle* h, M ilqr_handle::*m) {
    if (h->shards.empty()) return (bool)(h->*m);
    for (const ilqr_handle* s : h->shards) if (!(s->*m)) return false;
    return true;
}

// the refusal of the *_device forms on a sharded handle; host_form: the entry point that takes host pointers
int refuse_sharded(const char* host_form) {
    return fail(ILQR_ERR_INVALID, std::string("device pointers belong to one device: call ") + host_form + " (host pointers) on a sharded handle");
}
// an optional array of the whole batch as a shard sees it
template <class T> T* at(T* p, size_t off) { return p ? p + off : nullptr; }
// waves per workgroup of the kernels that give every sample / candidate of an instance a lane
int waves_for(int32_t S) { return (S + 63) / 64 > 4 ? 4 : (S + 63) / 64; }

// the inputs the handle keeps in HBM: what init_rollout reads, and what the MPC-side initialisers install in place
int resident_inputs(ilqr_handle* h) {
    const size_t bx = (size_t)h->B * h->vt->nx * 8, bu = (size_t)h->B * (h->L.T - 1) * h->vt->nu * 8;
    if (!h->d_x1) HIP_TRY(hipMalloc((void**)&h->d_x1, bx));
    if (!h->d_u) HIP_TRY(hipMalloc((void**)&h->d_u, bu));
    return ILQR_OK;
}

// the one place that frees and reallocates a stage: not before the stream has finished with the old buffer
int grow(ilqr_handle* h, ilqr_handle::Stage& st, size_t bytes) {
    if (bytes <= st.cap) return ILQR_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (st.p) { HIP_TRY(hipFree(st.p)); st.p = nullptr; st.cap = 0; }
    HIP_TRY(hipMalloc(&st.p, bytes));
    st.cap = bytes;
    return ILQR_OK;
}

// a null output of a *_launch means the handle's own buffer
template <class T> int own_if_null(ilqr_handle* h, T*& out, ilqr_handle::Stage& st, size_t bytes) {
    if (out) return ILQR_OK;
    ILQR_TRY(grow(h, st, bytes));
    out = (T*)st.p;
    return ILQR_OK;
}

// One array of a host form: the stage that holds it on the device, the host array it is uploaded from (src) and / or downloaded to
// (dst), its element size and its extent in elements — per instance, or (shared) of the one copy the whole batch reads. An array the
// caller did not give has no bytes: it never allocates, and its device pointer is null — unless the form keeps it on the device all
// the same (keep: a buffer of the call that nobody uploads or downloads). IN_RESIDENT: the handle's resident inputs, stage 0 = d_x1,
// 1 = d_u, which never grow.
enum StageSet { IN_POL, IN_CAND, IN_SHIFT, IN_SAMP, IN_PLANT, IN_RESIDENT };
struct Staged {
    StageSet set; int stage; const void* src; void* dst; size_t elem, extent; bool shared, keep;
    void* p; size_t bytes;                     // on the handle the form runs on (run_staged fills them in)
    double* d() const { return (double*)p; }
    int32_t* i() const { return (int32_t*)p; }
    Staged kept(bool on) const { Staged s = *this; s.keep = on; return s; }
};
template <class T> Staged staged_in(StageSet set, int stage, const T* src, size_t extent) { return {set, stage, src, nullptr, sizeof(T), extent, false, false, nullptr, 0}; }
template <class T> Staged staged_out(StageSet set, int stage, T* dst, size_t extent) { return {set, stage, nullptr, dst, sizeof(T), extent, false, false, nullptr, 0}; }
template <class T> Staged staged_io(StageSet set, int stage, T* both, size_t extent) { return {set, stage, both, both, sizeof(T), extent, false, false, nullptr, 0}; }
Staged staged_shared(StageSet set, int stage, const double* src, size_t extent) { return {set, stage, src, nullptr, 8, extent, true, false, nullptr, 0}; }
Staged staged_device(StageSet set, int stage, bool on, size_t extent) { return {set, stage, nullptr, nullptr, 8, extent, false, on, nullptr, 0}; }

ilqr_handle::Stage& stage_of(ilqr_handle* h, const Staged& a) {
    switch (a.set) {
        case IN_POL: return h->pol[a.stage];
        case IN_CAND: return h->cand[a.stage];
        case IN_SHIFT: return h->shift[a.stage];
        case IN_SAMP: return h->samp[a.stage];
        default: return h->plant[a.stage];
    }
}

// A host form on ONE handle, whose instances are [lo, lo + B) of the caller's batch: every stage grown, then the inputs on their
// way to the device, then launch(h, lo, arrays) with the device pointers, then the outputs on their way back and the stream
// finished — the one synchronise, after which the caller may read them, and reuse the host arrays of the inputs.
template <class F> int run_staged_on(ilqr_handle* h, size_t lo, std::vector<Staged> arrays, F& launch) {
    HIP_TRY(hipSetDevice(h->device));
    for (Staged& a : arrays) {
        a.bytes = (a.src || a.dst || a.keep) ? (a.shared ? 1 : (size_t)h->B) * a.extent * a.elem : 0;
        if (a.set == IN_RESIDENT) {
            ILQR_TRY(resident_inputs(h));
            a.p = a.stage == 0 ? h->d_x1 : h->d_u;
        } else {
            ILQR_TRY(grow(h, stage_of(h, a), a.bytes));
            a.p = stage_of(h, a).p;
        }
        if (!a.bytes) a.p = nullptr;
    }
    for (const Staged& a : arrays)
        if (a.src && a.bytes) HIP_TRY(hipMemcpyAsync(a.p, a.src, a.bytes, hipMemcpyHostToDevice, h->stream));
    ILQR_TRY(launch(h, lo, arrays.data()));
    for (const Staged& a : arrays)
        if (a.dst && a.bytes) HIP_TRY(hipMemcpyAsync(a.dst, a.p, a.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ILQR_OK;
}

// The same on any handle. A sharded one: one host thread per shard, which sees every per-instance array from its first instance
// on (lo · extent elements further); shared arrays stay as they are, null stays null.
template <class F> int run_staged(ilqr_handle* h, const std::vector<Staged>& arrays, F launch) {
    if (!SHARDED(h)) return run_staged_on(h, 0, arrays, launch);
    return each_shard(h, [&](ilqr_handle* s, size_t lo) {
        std::vector<Staged> mine = arrays;
        for (Staged& a : mine) {
            if (a.shared) continue;
            a.src = at((const char*)a.src, lo * a.extent * a.elem);
            a.dst = at((char*)a.dst, lo * a.extent * a.elem);
        }
        return run_staged_on(s, lo, std::move(mine), launch); }, true);
}

// test hook (ilqr_device_math): the scalar routines of ilqr_math.hpp as the device executes them
__global__ void device_math_kernel(int which, const double* x, double* y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r = 0.0, s, c;
    switch (which) {
        case 0: r = ilqr::recip_fast(v); break;
        case 1: r = ilqr::rsqrt_fast(v); break;
        case 2: ilqr::sqrt_rsqrt_fast(v, r, s); break;
        case 3: ilqr::sincos_fast(v, r, c); break;
        default: ilqr::sincos_fast(v, s, r); break;
    }
    y[i] = r;
}

// ilqr_mpc_run_est: row p of the filter's per-period logs, one thread per (instance, component); plain vector stores
__global__ void estimate_log_kernel(int B, int n, int periods, int p, const double* xhat, const double* P, const double* nis, double* xhat_cl,
                                    double* pdiag_cl, double* nis_cl) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)B * n) return;
    const size_t b = e / n, j = e % n, row = b * (size_t)periods + (size_t)p;
    if (xhat_cl) xhat_cl[row * n + j] = xhat[e];
    if (pdiag_cl) pdiag_cl[row * n + j] = P[b * n * n + j * (n + 1)];
    if (nis_cl && j == 0) nis_cl[row] = nis[b];
}

// The device forms of the linear sensor: a host vector of up to 64 doubles (r, sigma_y) goes to the device IN THE ARGUMENT SEGMENT of
// this launch, so it is read when the call is made — the caller's array may go away at once, successive calls may carry different
// values, and nothing waits for the stream. Lane j picks entry j through a chain of selects (no indexed read of the segment).
struct SensorVector { double v[ilqr::SENSOR_MAX_NY]; };
__global__ void sensor_vector_kernel(SensorVector a, int count, double* out) {
    const int j = threadIdx.x;
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < ilqr::SENSOR_MAX_NY; ++c) v = (j == c) ? a.v[c] : v;
    if (j < count) out[j] = v;
}

}  // namespace

extern "C" {

const char* ilqr_last_error(void) { return g_err.c_str(); }

int ilqr_device_math(const char* fn, const double* x, double* y, int32_t n) {
    static const char* names[] = {"recip_fast", "rsqrt_fast", "sqrt_fast", "sin_fast", "cos_fast"};
    int which = -1;
    for (int i = 0; i < 5; ++i)
        if (fn && !std::strcmp(fn, names[i])) which = i;
    if (which < 0 || !x || !y || n < 0) return fail(ILQR_ERR_INVALID, "ilqr_device_math: unknown function or null argument");
    if (ilqr_device_count() < 1) return fail(ILQR_ERR_NO_DEVICE, "no HIP device");
    if (n == 0) return ILQR_OK;
    double *dx = nullptr, *dy = nullptr;
    hipError_t e;
    auto bail = [&](hipError_t err, const char* what) { if (dx) (void)hipFree(dx); if (dy) (void)hipFree(dy); return fail(ILQR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err)); };
    int prev_dev = 0;
    (void)hipGetDevice(&prev_dev);                       // the caller's current device is put back below
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{prev_dev};
    if ((e = hipSetDevice(0)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipMalloc(&dx, (size_t)n * 8)) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMalloc(&dy, (size_t)n * 8)) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemcpy(dx, x, (size_t)n * 8, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy");
    hipLaunchKernelGGL(device_math_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, which, dx, dy, n);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e, "launch");
    if ((e = hipMemcpy(y, dy, (size_t)n * 8, hipMemcpyDeviceToHost)) != hipSuccess) return bail(e, "hipMemcpy");
    (void)hipFree(dx); (void)hipFree(dy);
    return ILQR_OK;
}

// the synthetic inputs as a pure function of (seed, instance, timestep, component)
int ilqr_synthetic_inputs(const char* model, int32_t T, uint64_t seed, int64_t first, int32_t B, double* x1, double* ub) {
    if (!model || !x1 || !ub || T < 2 || B < 0 || first < 0) return fail(ILQR_ERR_INVALID, "ilqr_synthetic_inputs: bad argument");
    struct Kind { const char* name; int n, m, kind; };
    static const Kind kinds[] = {{"particle", 2, 1, 0}, {"acrobot", 4, 1, 1}, {"car", 3, 2, 2}, {"car_goal", 3, 2, 2}, {"car_obs", 3, 2, 2},
                                 {"synth32", 32, 8, 3}, {"synth12", 12, 5, 4}};
    const Kind* k = nullptr;
    for (const Kind& q : kinds) if (!std::strcmp(q.name, model)) k = &q;
    if (!k) return fail(ILQR_ERR_MODEL, std::string("ilqr_synthetic_inputs: no workload for model '") + model + "'");
    auto mix = [](uint64_t z) { z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    auto unif = [](uint64_t h) { return ((double)(h >> 11) + 0.5) / 9007199254740992.0; };          // (0, 1)
    auto key = [&](int64_t b, int t, int j) { return seed ^ (uint64_t)(b * (1ll << 20) + (int64_t)t * 16 + j); };
    auto U = [&](int64_t b, int t, int j) { return unif(mix(key(b, t, j))); };
    auto Z = [&](int64_t b, int t, int j) { const uint64_t h1 = mix(key(b, t, j)), h2 = mix(h1); return std::sqrt(-2.0 * std::log(unif(h1))) * std::cos(6.283185307179586 * unif(h2)); };
    const int n = k->n, m = k->m, N = T - 1;
    for (int i = 0; i < B; ++i) {
        const int64_t b = first + i;
        double* x = x1 + (size_t)i * n;
        double* u = ub + (size_t)i * N * m;
        for (int j = 0; j < n; ++j) x[j] = 0.0;
        for (int e = 0; e < N * m; ++e) u[e] = 0.0;
        switch (k->kind) {
            case 0: for (int t = 0; t < N; ++t) u[t] = 0.1 * Z(b, t, 0); break;
            case 1: for (int t = 0; t < N; ++t) u[t] = Z(b, t, 0); break;
            case 2: {
                const double sc = b > 0 ? 1.0 + 0.5 * (2.0 * U(b, 0, 8) - 1.0) : 1.0;
                for (int t = 0; t < N; ++t) { u[t * 2] = 1.0e-2 * sc; u[t * 2 + 1] = 1.0e-3 * sc; }
                if (b > 0) { x[0] = 0.05 * Z(b, 0, 9); x[1] = 0.05 * Z(b, 0, 10); }
                break;
            }
            case 3: break;                                                  // x1 below; u = 0
            default:
                for (int t = 0; t < N; ++t) for (int j = 0; j < m; ++j) u[t * m + j] = 0.1 * Z(b, t, j);
        }
        if (k->kind >= 3) for (int j = 0; j < n; ++j) x[j] = 0.5 * Z(b, T + j / 16, j % 16);     // component j of x1: key slot (T + j / 16, j % 16), behind the horizon's
    }
    return ILQR_OK;
}

// the host twin of ilqr::sample_z (ilqr_device_sample.hpp): the same key, mix and U; libm's log, sqrt and cos
int ilqr_candidate_noise(uint64_t seed, int64_t first_instance, int32_t batch, int32_t candidates, int32_t steps, int32_t nu, double* z) {
#pragma clang fp contract(off)
    if (!z || batch < 0 || candidates < 0 || steps < 0 || nu < 0) return fail(ILQR_ERR_INVALID, "ilqr_candidate_noise: bad argument");
    if (candidates > ilqr::SAMPLE_MAX_CANDIDATES || steps > ilqr::SAMPLE_MAX_STEPS || nu > ilqr::SAMPLE_MAX_NU)
        return fail(ILQR_ERR_INVALID, "ilqr_candidate_noise: candidates <= 65536, steps <= 2^20 and nu <= 16 (the key's bit fields)");
    if (first_instance < 0 || first_instance + (int64_t)batch > ilqr::SAMPLE_MAX_INSTANCES)
        return fail(ILQR_ERR_INVALID, "ilqr_candidate_noise: first_instance >= 0 and first_instance + batch <= 2^23 (the key's bit fields)");
    for (int32_t b = 0; b < batch; ++b)
        for (int32_t s = 0; s < candidates; ++s)
            for (int32_t t = 0; t < steps; ++t)
                for (int32_t j = 0; j < nu; ++j) {
                    const uint64_t h1 = ilqr::sample_mix(ilqr::sample_key(seed, first_instance + b, s, t, j)), h2 = ilqr::sample_mix(h1);
                    const double r = std::sqrt(-2.0 * std::log(ilqr::sample_unif(h1)));
                    z[(((size_t)b * candidates + s) * steps + t) * nu + j] = s == 0 ? 0.0 : r * std::cos(6.283185307179586 * ilqr::sample_unif(h2));
                }
    return ILQR_OK;
}

int ilqr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ilqr_default_options(ilqr_options* o) {
    if (!o) return fail(ILQR_ERR_INVALID, "null options");
    // src/options.jl:1-15
    o->line_search = 1; o->max_iterations = 100; o->max_dual_updates = 10;
    o->min_step_size = 1.0e-5; o->objective_tolerance = 1.0e-3; o->lagrangian_gradient_tolerance = 1.0e-3;
    o->constraint_tolerance = 5.0e-3; o->constraint_norm = INFINITY; o->initial_constraint_penalty = 1.0;
    o->scaling_penalty = 10.0; o->max_penalty = 1.0e8; o->reset_cache = 0; o->verbose = 1;
    return ILQR_OK;
}

int ilqr_register_model(const ilqr_model_vtable* vt) {
    if (!vt) return ILQR_ERR_INVALID;
    // a module built against other headers would be handed a KArgs / Layout it misreads: refuse it
    if (vt->abi_version != ILQR_MODEL_ABI_VERSION || vt->kargs_bytes != (int)sizeof(ilqr::KArgs))
        return fail(ILQR_ERR_MODEL, "model module was built against a different library version (ABI mismatch): rebuild it");
    if (!vt->name) return ILQR_ERR_INVALID;
    auto& r = registry();
    for (auto& e : r)
        if (!std::strcmp(e->name, vt->name)) { e = vt; return ILQR_OK; }
    r.push_back(vt);
    return ILQR_OK;
}
int ilqr_register_model_ext(const void* ext) {
    const ilqr_model_ext* e = (const ilqr_model_ext*)ext;
    if (!e) return ILQR_ERR_INVALID;
    if (e->ext_version != ILQR_MODEL_EXT_VERSION || e->args_bytes != (int)sizeof(ilqr::PlanCovArgs))
        return fail(ILQR_ERR_MODEL, "model module was built against a different library version (ABI mismatch): rebuild it");
    if (!e->name) return ILQR_ERR_INVALID;
    if (!find_model(e->name)) return fail(ILQR_ERR_MODEL, std::string("ilqr_register_model_ext: no model '") + e->name + "' is registered");
    auto& r = ext_registry();
    for (auto& x : r)
        if (!std::strcmp(x->name, e->name)) { x = e; return ILQR_OK; }
    r.push_back(e);
    return ILQR_OK;
}
int ilqr_model_count(void) { return (int)registry().size(); }

int ilqr_register_sensor(const void* vtable) {
    const ilqr_sensor_vtable* sv = (const ilqr_sensor_vtable*)vtable;
    if (!sv) return ILQR_ERR_INVALID;
    // a module built against other headers would be handed a SensorNlArgs it misreads: refuse it
    if (sv->abi_version != ILQR_SENSOR_ABI_VERSION || sv->args_bytes != (int)sizeof(ilqr::SensorNlArgs))
        return fail(ILQR_ERR_MODEL, "sensor module was built against a different library version (ABI mismatch): rebuild it");
    if (!sv->name) return ILQR_ERR_INVALID;
    auto& r = sensor_registry();
    for (auto& e : r)
        if (!std::strcmp(e->name, sv->name)) { e = sv; return ILQR_OK; }
    r.push_back(sv);
    return ILQR_OK;
}
int ilqr_sensor_count(void) { return (int)sensor_registry().size(); }
const char* ilqr_sensor_name(int32_t i) {
    return (i >= 0 && i < (int)sensor_registry().size()) ? sensor_registry()[i]->name : nullptr;
}
int ilqr_sensor_dims(const char* sensor, int32_t* nx, int32_t* ny, int32_t* ns) {
    const ilqr_sensor_vtable* sv = find_sensor(sensor);
    if (!sv) return fail(ILQR_ERR_INVALID, "ilqr_sensor_dims: unknown sensor");
    if (nx) *nx = sv->nx;
    if (ny) *ny = sv->ny;
    if (ns) *ns = sv->ns;
    return ILQR_OK;
}

const char* ilqr_model_name(int32_t i) {
    return (i >= 0 && i < (int)registry().size()) ? registry()[i]->name : nullptr;
}
int ilqr_model_compact_sizes(const char* model, int32_t* jac_nvar, int32_t* hess_nnz) {
    const ilqr_model_vtable* vt = model ? find_model(model) : nullptr;
    if (!vt) return fail(ILQR_ERR_MODEL, "unknown model");
    if (jac_nvar) *jac_nvar = vt->jac_nvar;
    if (hess_nnz) *hess_nnz = vt->hess_nnz;
    return ILQR_OK;
}

int ilqr_create(const ilqr_problem_desc* d, ilqr_handle** out) {
    if (!d || !out || !d->model) return fail(ILQR_ERR_INVALID, "null descriptor/model");
    if (d->horizon < 2 || d->batch < 1) return fail(ILQR_ERR_INVALID, "horizon must be >= 2 and batch >= 1");
    if (d->model_library && d->model_library[0]) {
        if (!dlopen(d->model_library, RTLD_NOW | RTLD_GLOBAL))
            return fail(ILQR_ERR_MODEL, std::string("dlopen failed: ") + dlerror());
    }
    const ilqr_model_vtable* vt = find_model(d->model);
    if (!vt) return fail(ILQR_ERR_MODEL, std::string("unknown model '") + d->model + "'");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(ILQR_ERR_NO_DEVICE, "no HIP device available: the batched solver has no CPU fallback");
    if (d->device < 0 || d->device >= ndev) return fail(ILQR_ERR_INVALID, "device ordinal out of range");
    ilqr_handle* h = new ilqr_handle();
    h->vt = vt; h->B = d->batch; h->device = d->device; h->constrained = d->constrained ? 1 : 0;
    h->L = ilqr::make_layout(vt->nx, vt->nu, vt->nw, vt->ncs, vt->nct, d->horizon, vt->jac_nvar, vt->hess_nnz);
    h->lds_bytes = ilqr::is_large_model(vt->nx, vt->nu) ? (size_t)ilqr::large_lds_doubles(vt->nx, vt->nu, vt->hess_nnz) * 8
                                                          : (size_t)h->L.lds_doubles * 8;
    h->ws = nullptr; h->d_x1 = nullptr; h->d_u = nullptr; h->stream = nullptr;
    h->trace = nullptr; h->trace_cap = 0; h->variant = 0; h->num_simds = 1024; h->handover = -1; h->handover_live = -1; h->done_counter = nullptr; h->pool = nullptr; h->handover_mark = -1;
    h->qv = nullptr; h->QL = ilqr::make_qlayout(vt->nx, vt->nu, d->horizon); h->full_stale = false; h->P_dirty = false;
    ilqr_default_options(&h->opt);
    fill_buffers(h);
    h->lds_fits = h->lds_bytes <= 160 * 1024;
    if (!h->lds_fits && !has_kernel(vt, ilqr::K_PACKED1)) {
        // the reference has no horizon limit (src/data/problem.jl:25-46); here only the streaming (packed) kernel is free of one
        delete h;
        return fail(ILQR_ERR_LDS, "per-instance working set exceeds the 160 KiB LDS of a gfx950 CU and this model has no "
                                  "streaming (packed) kernel; reduce the horizon");
    }
    // from here on every failure must release the handle
    auto bail = [&](hipError_t e, const char* what) {
        const int rc = fail(ILQR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        ilqr_destroy(h);
        return rc;
    };
    hipError_t e;
    if ((e = hipSetDevice(h->device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->device) == hipSuccess) h->num_simds = 4 * prop.multiProcessorCount;
    }
    h->ws_bytes = (size_t)h->B * (size_t)h->L.stride * 8;
    if ((e = hipMalloc((void**)&h->ws, h->ws_bytes)) != hipSuccess) return bail(e, "hipMalloc(workspace)");
    if (has_kernel(vt, ilqr::K_PACKED1) && (e = hipMalloc((void**)&h->done_counter, sizeof(int))) != hipSuccess) return bail(e, "hipMalloc(hand-over counter)");
    if (has_kernel(vt, ilqr::K_PACKED1) && (e = hipMalloc((void**)&h->pool, sizeof(int) * (size_t)(ilqr::POOL_Q + h->B + ilqr::POOL_CUS))) != hipSuccess) return bail(e, "hipMalloc(hand-over queue)");
    if ((e = hipMemsetAsync(h->ws, 0, h->ws_bytes, h->stream)) != hipSuccess) return bail(e, "hipMemsetAsync");
    if (!ilqr::is_large_model(vt->nx, vt->nu) && (e = hipMalloc((void**)&h->cu_slots, sizeof(int) * ilqr::CU_SLOT_INTS * ilqr::CU_SLOT_CUS)) != hipSuccess) return bail(e, "hipMalloc(role table)");
    if (h->pool && (e = hipMemsetAsync(h->pool, 0, sizeof(int) * (size_t)(ilqr::POOL_Q + h->B + ilqr::POOL_CUS), h->stream)) != hipSuccess) return bail(e, "hipMemsetAsync(hand-over queue)");
    *out = h;
    int rc = ilqr_reset(h);
    if (rc != ILQR_OK) { ilqr_destroy(h); *out = nullptr; return rc; }
    return ILQR_OK;
}

// Solver(...) over a device list — SURVEY §8(b)/(e): one reference-style handle whose batch is split into contiguous ranges of
// ceil(B / G) instances, range i on devices[i] (a device may be listed more than once). Every other entry point accepts the
// handle and scatters / gathers instance-major host arrays over the ranges.
int ilqr_create_sharded(const ilqr_problem_desc* d, const int32_t* devices, int32_t n_devices, ilqr_handle** out) {
    if (!d || !out || !d->model || !devices) return fail(ILQR_ERR_INVALID, "null descriptor/model/device list");
    if (n_devices < 1) return fail(ILQR_ERR_INVALID, "empty device list");
    if (d->horizon < 2 || d->batch < 1) return fail(ILQR_ERR_INVALID, "horizon must be >= 2 and batch >= 1");
    if (n_devices > d->batch) return fail(ILQR_ERR_INVALID, "more devices than instances");
    ilqr_handle* h = new ilqr_handle();
    h->vt = nullptr; h->ws = nullptr; h->d_x1 = nullptr; h->d_u = nullptr; h->stream = nullptr; h->trace = nullptr; h->qv = nullptr; h->done_counter = nullptr; h->pool = nullptr;
    h->B = d->batch; h->device = devices[0]; h->constrained = d->constrained ? 1 : 0; h->trace_cap = 0; h->variant = 0;
    const int per = (d->batch + n_devices - 1) / n_devices;
    for (int i = 0, lo = 0; i < n_devices && lo < d->batch; ++i, lo += per) {
        ilqr_problem_desc sd = *d;
        sd.device = devices[i];
        sd.batch = (d->batch - lo) < per ? (d->batch - lo) : per;
        ilqr_handle* sub = nullptr;
        const int rc = ilqr_create(&sd, &sub);
        if (rc != ILQR_OK) { const std::string msg = g_err; ilqr_destroy(h); return fail(rc, msg); }
        h->shards.push_back(sub);
        h->lo.push_back(lo);
    }
    const ilqr_handle* s0 = h->shards[0];
    h->vt = s0->vt; h->L = s0->L; h->QL = s0->QL; h->opt = s0->opt; h->lds_bytes = s0->lds_bytes; h->lds_fits = s0->lds_fits; h->num_simds = s0->num_simds;
    h->full_stale = false; h->P_dirty = false;
    fill_buffers(h);
    *out = h;
    return ILQR_OK;
}

int ilqr_destroy(ilqr_handle* h) {
    if (!h) return ILQR_OK;
    if (!h->shards.empty() || h->vt == nullptr) {
        for (ilqr_handle* s : h->shards) ilqr_destroy(s);
        delete h;
        return ILQR_OK;
    }
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (auto& p : h->timing) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (h->ws) hipFree(h->ws);
    if (h->d_x1) hipFree(h->d_x1);
    if (h->done_counter) hipFree(h->done_counter);
    if (h->pool) hipFree(h->pool);
    if (h->cu_slots) hipFree(h->cu_slots);
    if (h->d_u) hipFree(h->d_u);
    for (auto& st : h->pol) if (st.p) hipFree(st.p);
    for (auto& st : h->cand) if (st.p) hipFree(st.p);
    for (auto& st : h->shift) if (st.p) hipFree(st.p);
    for (auto& st : h->samp) if (st.p) hipFree(st.p);
    for (auto& st : h->plant) if (st.p) hipFree(st.p);
    if (h->trace) hipFree(h->trace);
    if (h->qv) hipFree(h->qv);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return ILQR_OK;
}

int ilqr_set_options(ilqr_handle* h, const ilqr_options* opt) {
    if (!h || !opt) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) { h->opt = *opt; return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_set_options(s, opt); }); }
    h->opt = *opt;
    return ILQR_OK;
}

int ilqr_get_dims(const ilqr_handle* h, int32_t* nx, int32_t* nu, int32_t* nw, int32_t* ncs, int32_t* nct,
                  int32_t* horizon, int32_t* batch) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (nx) *nx = h->vt->nx;
    if (nu) *nu = h->vt->nu;
    if (nw) *nw = h->vt->nw - h->n_sel;          // the USER's parameters per timestep (selector columns are the library's)
    if (ncs) *ncs = h->vt->ncs;
    if (nct) *nct = h->vt->nct;
    if (horizon) *horizon = h->L.T;
    if (batch) *batch = h->B;
    return ILQR_OK;
}

int ilqr_reset(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_reset(s); });
    HIP_TRY(hipSetDevice(h->device));
    h->has_policy = false;                            // K, k are zeroed below
    h->has_duals = false;                             // λ ← 0, and ρ ← 1 is the fresh solver's, not a solve's
    if (ilqr::is_large_model(h->vt->nx, h->vt->nu) && h->vt->nw == 0) {
        // HBM-resident models: zero the trajectories, gradients, gains, duals, scalars and the compact Jacobian / Hessian rows
        // now; the megabyte-sized full Jacobian / Hessian mirrors are rewritten from the compact form when a getter asks
        // for them, the value arrays P, p are zeroed when a getter, setter or stage call could observe them
        ilqr::KArgs ra = make_args(h);
        hipLaunchKernelGGL(ilqr::reset_large_kernel, dim3(h->B * 8), dim3(256), 0, h->stream, ra, h->L.fx, h->L.scal);
        HIP_TRY(hipGetLastError());
        h->full_stale = true; h->P_dirty = true;
        return ILQR_OK;
    } else if (h->vt->nw == 0) {
        HIP_TRY(hipMemsetAsync(h->ws, 0, h->ws_bytes, h->stream));
    } else {
        h->full_stale = ilqr::is_large_model(h->vt->nx, h->vt->nu);
        // keep the parameters θ (they belong to the problem, not to the solver state)
        const size_t pitch = (size_t)h->L.stride * 8, w0 = (size_t)h->L.w * 8, w1 = (size_t)h->L.zslot * 8;
        HIP_TRY(hipMemset2DAsync(h->ws, pitch, 0, w0, (size_t)h->B, h->stream));
        HIP_TRY(hipMemset2DAsync((char*)h->ws + w1, pitch, 0, pitch - w1, (size_t)h->B, h->stream));
    }
    ilqr::KArgs a = make_args(h);
    hipLaunchKernelGGL(ilqr::defaults_kernel, dim3(h->B), dim3(64), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return ILQR_OK;
}

int ilqr_initialize_controls(ilqr_handle* h, const double* u) {
    if (!h || !u) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_initialize_controls(s, u + lo * (size_t)(h->L.T - 1) * h->L.nu); }, true);
    return copy_in(h, find_buffer(h, "nominal_actions"), u);
}
int ilqr_initialize_states(ilqr_handle* h, const double* x) {
    if (!h || !x) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_initialize_states(s, x + lo * (size_t)h->L.T * h->L.nx); }, true);
    return copy_in(h, find_buffer(h, "nominal_states"), x);
}

// the full parameter block [B][T][nw] of a handle with selectors: the user's columns (NULL = zeros) followed by the table
static int write_parameters_with_selectors(ilqr_handle* h, const double* w_user) {
    const int T = h->L.T, nw = h->vt->nw, S = h->n_sel, nwu = nw - S;
    std::vector<double> full((size_t)h->B * T * nw, 0.0);
    if (!w_user && nwu > 0) {        // selectors alone (ilqr_set_stage_selectors): the user's columns keep what they hold
        const int rc = copy_out(h, find_buffer(h, "parameters"), full.data());
        if (rc != ILQR_OK) return rc;
    }
    for (int b = 0; b < h->B; ++b)
        for (int t = 0; t < T; ++t) {
            double* row = &full[((size_t)b * T + t) * nw];
            if (w_user) for (int j = 0; j < nwu; ++j) row[j] = w_user[((size_t)b * T + t) * nwu + j];
            for (int j = 0; j < S; ++j) row[nwu + j] = h->sel[(size_t)t * S + j];
        }
    return copy_in(h, find_buffer(h, "parameters"), full.data());
}

int ilqr_set_stage_selectors(ilqr_handle* h, const double* selectors, int32_t n_selectors) {
    if (!h || n_selectors < 0 || (n_selectors > 0 && !selectors)) return fail(ILQR_ERR_INVALID, "null argument");
    if (n_selectors > h->vt->nw) return fail(ILQR_ERR_INVALID, "more selector columns than the model has parameters");
    if (SHARDED(h)) {
        const int rc = each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_set_stage_selectors(s, selectors, n_selectors); }, true);
        if (rc == ILQR_OK) { h->n_sel = n_selectors; h->sel.assign(selectors, selectors + (size_t)h->L.T * n_selectors); }
        return rc;
    }
    h->n_sel = n_selectors;
    h->sel.assign(selectors, selectors + (size_t)h->L.T * n_selectors);
    if (n_selectors == 0) return ILQR_OK;
    return write_parameters_with_selectors(h, nullptr);
}

int ilqr_set_parameters(ilqr_handle* h, const double* w) {
    if (!h || !w) return fail(ILQR_ERR_INVALID, "null argument");
    const size_t nwu = (size_t)(h->L.nw - h->n_sel);
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_set_parameters(s, w + lo * (size_t)h->L.T * nwu); }, true);
    if (nwu == 0) return fail(ILQR_ERR_INVALID, "this model has no parameters (num_parameter == 0)");
    if (h->n_sel > 0) return write_parameters_with_selectors(h, w);
    return copy_in(h, find_buffer(h, "parameters"), w);
}

int ilqr_initialize_rollout_device(ilqr_handle* h, const double* d_x1, const double* d_u) {
    if (!h || !d_x1 || !d_u) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return refuse_sharded("ilqr_initialize_rollout");
    HIP_TRY(hipSetDevice(h->device));
    ilqr::KArgs a = make_args(h);
    a.x1 = d_x1; a.u_in = d_u;
    if (h->vt->launch_init(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "init_rollout launch failed");
    return ILQR_OK;
}

int ilqr_initialize_rollout(ilqr_handle* h, const double* x1, const double* u) {
    if (!h || !x1 || !u) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) {
        return ilqr_initialize_rollout(s, x1 + lo * (size_t)h->L.nx, u + lo * (size_t)(h->L.T - 1) * h->L.nu); }, true);
    HIP_TRY(hipSetDevice(h->device));
    ILQR_TRY(resident_inputs(h));
    const size_t bx = (size_t)h->B * h->vt->nx * 8, bu = (size_t)h->B * (h->L.T - 1) * h->vt->nu * 8;
    HIP_TRY(hipMemcpyAsync(h->d_x1, x1, bx, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_u, u, bu, hipMemcpyHostToDevice, h->stream));
    ILQR_TRY(ilqr_initialize_rollout_device(h, h->d_x1, h->d_u));
    HIP_TRY(hipStreamSynchronize(h->stream));   // host buffers may be reused by the caller
    return ILQR_OK;
}

// what the launch plan (ilqr_launch_plan.hpp) reads of the handle
static ilqr::LaunchIn launch_in(const ilqr_handle* h) {
    static const bool role_slots = !(std::getenv("ILQR_ROLE_SLOTS") && std::getenv("ILQR_ROLE_SLOTS")[0] == '0');
    ilqr::LaunchIn in;
    in.variant = h->variant; in.B = h->B; in.num_simds = h->num_simds;
    in.lds_fits = h->lds_fits; in.lds_bytes = h->lds_bytes; in.slim_lds_bytes = (size_t)h->L.lds_doubles_slim * 8;
    in.kernels = h->vt->kernels; in.packed1_lds_bytes = h->vt->packed1_lds_bytes; in.packed2_lds_bytes = h->vt->packed2_lds_bytes;
    in.constrained = h->constrained != 0; in.max_dual_updates = h->opt.max_dual_updates;
    in.handover = h->handover; in.handover_live = h->handover_live; in.handover_mark = h->handover_mark;
    in.done_counter = h->done_counter != nullptr; in.pool = h->pool != nullptr; in.cu_slots = h->cu_slots != nullptr;
    in.role_slots = role_slots;
    return in;
}

int ilqr_initialize_rollout_resident(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_initialize_rollout_resident(s); });
    if (!h->d_x1 || !h->d_u) return fail(ILQR_ERR_INVALID, "no resident inputs: ilqr_initialize_rollout (host pointers) has to come first");
    return ilqr_initialize_rollout_device(h, h->d_x1, h->d_u);
}

// ilqr_solve (warm == 0) and ilqr_solve_warm (warm == 1): one body, the launches differ in KArgs::warm_duals alone
static int solve_launch(ilqr_handle* h, int warm) {
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return solve_launch(s, warm); });      // asynchronous on every device's stream
    HIP_TRY(hipSetDevice(h->device));
    ilqr::KArgs a = make_args(h);
    a.qv = nullptr;
    a.warm_duals = warm;                              // (copied into the resume launch's arguments below)
    if (h->trace)      // rows of an earlier, longer solve must not survive
        HIP_TRY(hipMemsetAsync(h->trace, 0, (size_t)h->B * h->trace_cap * ilqr::TRACE_W * 8, h->stream));
    if (h->vt->launch_mirror) h->full_stale = true;   // the kernel works on the compact Jacobian / Hessian rows
    h->pool_valid = false;                            // (set again below when this solve zeroes and uses the hand-over queue)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto drop = [&](int rc) { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); return rc; };
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, h->stream) != hipSuccess)
        return drop(fail(ILQR_ERR_HIP, "hipEventCreate/Record failed"));
    const ilqr::LaunchPlan p = ilqr::solve_plan(launch_in(h));
    if (p.kernel == 0) return drop(fail(ILQR_ERR_LDS, "this horizon only runs on the packed kernel"));
    a.handover_outer = p.handover_outer; a.handover_live = p.handover_live;
    ilqr::KArgs r = a;
    r.resume = 1;                                     // the resume launch that finishes the instances handed over
    if (p.handover_live > 0) HIP_TRY(hipMemsetAsync(h->done_counter, 0, sizeof(int), h->stream));
    if (p.zero_pool) {
        HIP_TRY(hipMemsetAsync(h->pool, 0, sizeof(int) * (size_t)(ilqr::POOL_Q + h->B + ilqr::POOL_CUS), h->stream));
        h->pool_valid = true;
    }
    a.pool = p.pool ? h->pool : nullptr;
    a.pool_mark = p.pool_mark; a.pool_lds = p.pool_lds; a.pool_ctl = p.pool_ctl; a.pool_cu = p.pool_cu;
    if (p.role_slots) {
        HIP_TRY(hipMemsetAsync(h->cu_slots, 0, sizeof(int) * ilqr::CU_SLOT_INTS * ilqr::CU_SLOT_CUS, h->stream));
        a.cu_slots = h->cu_slots; a.cu_expect = p.cu_expect;
    }
    size_t lds = p.lds;
#ifdef ILQR_PK_DEBUG_HOOK      // phase-timing hook of tools/packed_phases.py (see ilqr_device_packed.hpp); never compiled into the product library
    if (const char* dbg = std::getenv("ILQR_PK_DEBUG"); dbg && (p.kernel == ilqr::K_PACKED1 || p.kernel == ilqr::K_PACKED2)) a.stage = std::atoi(dbg);
#endif
#ifdef ILQR_DBG_LDS_PAD_HOOK   // residency experiment of tools/mid_bench.py (more LDS per workgroup = fewer workgroups per CU); never in the product library
    if (const char* pad = std::getenv("ILQR_DBG_LDS_PAD"); pad && p.kernel == ilqr::K_MID) lds += (size_t)std::atoi(pad);
#endif
    if (h->vt->launch(p.kernel, &a, p.grid, lds, h->stream) != 0) return drop(fail(ILQR_ERR_HIP, "solve launch failed (kernel " + std::to_string(p.kernel) + ")"));
    if (p.resume && h->vt->launch(ilqr::K_RESUME, &r, h->B, h->lds_bytes, h->stream) != 0)
        return drop(fail(ILQR_ERR_HIP, "solve (hand-over resume) launch failed"));
    if (hipEventRecord(e1, h->stream) != hipSuccess) return drop(fail(ILQR_ERR_HIP, "hipEventRecord failed"));
    h->has_policy = true;
    if (h->constrained) h->has_duals = true;
    h->timing.emplace_back(e0, e1);
    if (h->timing.size() > 4096) {     // long-running callers that never read the timing: keep the newest half
        for (size_t i = 0; i < 2048; ++i) { hipEventDestroy(h->timing[i].first); hipEventDestroy(h->timing[i].second); }
        h->timing.erase(h->timing.begin(), h->timing.begin() + 2048);
    }
    return ILQR_OK;
}

int ilqr_solve(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    return solve_launch(h, 0);
}

int ilqr_solve_warm(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "ilqr_solve_warm: null handle");
    if (!h->constrained) return fail(ILQR_ERR_INVALID, "ilqr_solve_warm: the handle was created unconstrained: it has no duals to keep");
    if (!every_shard_holds(h, &ilqr_handle::has_duals)) return fail(ILQR_ERR_INVALID, "ilqr_solve_warm: the handle holds no duals yet (no constrained solve, no al_begin stage and no host write of constraint_penalty since the last reset)");
    return solve_launch(h, 1);
}

int ilqr_run_stage(ilqr_handle* h, int32_t stage) { return ilqr_run_stage_param(h, stage, 0.0, 0); }

int ilqr_run_stage_param(ilqr_handle* h, int32_t stage, double param, int32_t flag) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_run_stage_param(s, stage, param, flag); }, true);
    HIP_TRY(hipSetDevice(h->device));
    { const int rc = settle_reset(h); if (rc != ILQR_OK) return rc; }
    const ilqr::LaunchPlan p = ilqr::stage_plan(launch_in(h));
    if (p.kernel == 0) return fail(ILQR_ERR_LDS, "stage kernels are LDS-resident: this horizon only runs through ilqr_solve (packed kernel)");
    ilqr::KArgs a = make_args(h);
    a.stage = stage; a.stage_param = param; a.stage_flag = flag;
    if (stage != ILQR_STAGE_BACKWARD_PASS && stage != ILQR_STAGE_ILQR_SOLVE) a.qv = nullptr;
    if (h->vt->launch(p.kernel, &a, p.grid, p.lds, h->stream) != 0) return fail(ILQR_ERR_HIP, "stage launch failed (kernel " + std::to_string(p.kernel) + ")");
    if (h->vt->launch_mirror) h->full_stale = true;
    if (stage == ILQR_STAGE_BACKWARD_PASS || stage == ILQR_STAGE_ILQR_SOLVE || stage == ILQR_STAGE_SS_FINISH) h->has_policy = true;
    if (stage == ILQR_STAGE_AL_BEGIN) h->has_duals = true;      // (ilqr_solve_shared_step opens with this stage)
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ILQR_OK;
}

// solve! with one step size per inner iteration for the whole (multi-rank) batch: forward_pass!'s Armijo loop on the host over the
// summed merit (see ilqr_hip.h). The loop is the reference's (src/solve.jl:88-129 around :1-54, src/forward_pass.jl:26-52) with
// the per-instance phases as stage launches.
int ilqr_solve_shared_step(ilqr_handle* h, ilqr_allreduce_sum_fn reduce, void* ctx, double* steps, int32_t steps_cap, int32_t* n_steps) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (!h->constrained) return fail(ILQR_ERR_INVALID, "shared-step mode: constrained solvers only");
    const int B = h->B, NS = ilqr::S_COUNT;
    std::vector<double> sc((size_t)B * NS);
    auto scalars = [&]() { return ilqr_get_buffer(h, "_scalars", sc.data()); };
    auto allsum = [&](double* v, int n) -> int {
        if (!reduce) return ILQR_OK;
        return reduce(v, n, ctx) == 0 ? ILQR_OK : fail(ILQR_ERR_INVALID, "shared-step mode: the reduction callback failed");
    };
    const ilqr_options opt = h->opt;
    int count = 0, rc;
    if ((rc = ilqr_run_stage(h, ILQR_STAGE_AL_BEGIN)) != ILQR_OK) return rc;
    for (int outer = 0; outer < opt.max_dual_updates; ++outer) {
        if ((rc = ilqr_run_stage(h, ILQR_STAGE_SS_INNER_BEGIN)) != ILQR_OK) return rc;
        for (int it = 0; it < opt.max_iterations; ++it) {
            if ((rc = scalars()) != ILQR_OK) return rc;
            std::vector<char> active(B);
            double n_active = 0.0;
            for (int b = 0; b < B; ++b) {
                active[b] = sc[(size_t)b * NS + ilqr::S_DONE] == 0.0 && sc[(size_t)b * NS + ilqr::S_INNER_DONE] == 0.0;
                n_active += active[b];
            }
            if ((rc = allsum(&n_active, 1)) != ILQR_OK) return rc;
            if (n_active == 0.0) break;
            double alpha = 1.0;
            int first = 1, accepted = 0, trials = 1;
            while (alpha >= opt.min_step_size && trials <= 25) {                          // src/forward_pass.jl:28-29
                if ((rc = ilqr_run_stage_param(h, ILQR_STAGE_SS_TRIAL, alpha, first)) != ILQR_OK) return rc;
                if ((rc = scalars()) != ILQR_OK) return rc;
                double sums[3] = {0.0, 0.0, 0.0};
                for (int b = 0; b < B; ++b)
                    if (active[b]) {
                        sums[0] += sc[(size_t)b * NS + ilqr::S_OBJECTIVE]; sums[1] += sc[(size_t)b * NS + ilqr::S_J_PREV];
                        sums[2] += sc[(size_t)b * NS + ilqr::S_DELTA];
                    }
                if ((rc = allsum(sums, 3)) != ILQR_OK) return rc;                          // the data-path collective: three doubles
                if (sums[0] <= sums[1] + 1.0e-4 * alpha * sums[2]) { accepted = 1; break; }  // (:44) NaN ⇒ reject
                alpha *= 0.5;                                                            // (:51)
                first = 0;
                ++trials;
            }
            if ((rc = ilqr_run_stage_param(h, ILQR_STAGE_SS_FINISH, alpha, accepted)) != ILQR_OK) return rc;
            if (steps && count < steps_cap) steps[count] = accepted ? alpha : 0.0;
            ++count;
        }
        if ((rc = ilqr_run_stage(h, ILQR_STAGE_SS_OUTER)) != ILQR_OK) return rc;
        if ((rc = scalars()) != ILQR_OK) return rc;
        double n_open = 0.0;
        for (int b = 0; b < B; ++b) n_open += sc[(size_t)b * NS + ilqr::S_DONE] == 0.0;
        if ((rc = allsum(&n_open, 1)) != ILQR_OK) return rc;
        if (n_open == 0.0) break;
    }
    if (n_steps) *n_steps = count;
    return ILQR_OK;
}

int ilqr_synchronize(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_synchronize(s); });
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ILQR_OK;
}

int ilqr_get_trajectory(ilqr_handle* h, double* x, double* u) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) {
        return ilqr_get_trajectory(s, x ? x + lo * (size_t)h->L.T * h->L.nx : nullptr, u ? u + lo * (size_t)(h->L.T - 1) * h->L.nu : nullptr); }, true);
    int rc = ILQR_OK;
    if (x) rc = copy_out(h, find_buffer(h, "nominal_states"), x);
    if (rc == ILQR_OK && u) rc = copy_out(h, find_buffer(h, "nominal_actions"), u);
    return rc;
}

int ilqr_get_policy(ilqr_handle* h, double* K, double* k) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) {
        const size_t N = (size_t)(h->L.T - 1);
        return ilqr_get_policy(s, K ? K + lo * N * h->L.nu * h->L.nx : nullptr, k ? k + lo * N * h->L.nu : nullptr); }, true);
    int rc = ILQR_OK;
    if (K) rc = copy_out(h, find_buffer(h, "K"), K);
    if (rc == ILQR_OK && k) rc = copy_out(h, find_buffer(h, "k"), k);
    return rc;
}

int ilqr_get_stats(ilqr_handle* h, ilqr_stats* st) {
    if (!h || !st) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_get_stats(s, st + lo); }, true);
    std::vector<double> s((size_t)h->B * ilqr::S_COUNT);
    int rc = copy_out(h, find_buffer(h, "_scalars"), s.data());
    if (rc != ILQR_OK) return rc;
    for (int b = 0; b < h->B; ++b) {
        const double* v = &s[(size_t)b * ilqr::S_COUNT];
        st[b].objective = v[ilqr::S_OBJECTIVE]; st[b].gradient_norm = v[ilqr::S_GRADIENT_NORM];
        st[b].max_violation = v[ilqr::S_MAX_VIOLATION]; st[b].step_size = v[ilqr::S_STEP_SIZE];
        st[b].iterations = (int32_t)v[ilqr::S_ITERATIONS]; st[b].outer_iterations = (int32_t)v[ilqr::S_OUTER_ITERATIONS];
        st[b].status = (int32_t)v[ilqr::S_STATUS]; st[b].potrf_info = (int32_t)v[ilqr::S_POTRF_INFO];
        st[b].rollouts = (int32_t)v[ilqr::S_ROLLOUTS]; st[b].reserved = 0;
    }
    return ILQR_OK;
}

int ilqr_buffer_len(const ilqr_handle* h, const char* name, size_t* len) {
    if (!h || !name || !len) return fail(ILQR_ERR_INVALID, "null argument");
    const BufferDesc* bd = find_buffer(h, name);
    if (!bd) bd = find_qbuffer(h, name);
    if (!bd) return fail(ILQR_ERR_INVALID, std::string("unknown buffer '") + name + "'");
    *len = (size_t)bd->len;
    return ILQR_OK;
}
int ilqr_enable_action_value_buffers(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_enable_action_value_buffers(s); });
    if (h->qv) return ILQR_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->B * (size_t)h->QL.stride * 8;
    HIP_TRY(hipMalloc((void**)&h->qv, bytes));
    HIP_TRY(hipMemsetAsync(h->qv, 0, bytes, h->stream));
    return ILQR_OK;
}

int ilqr_scalar_slot(const char* name) {
    static const struct { const char* n; int i; } slots[] = {
        {"objective", ilqr::S_OBJECTIVE}, {"max_violation", ilqr::S_MAX_VIOLATION}, {"step_size", ilqr::S_STEP_SIZE},
        {"status", ilqr::S_STATUS}, {"iterations", ilqr::S_ITERATIONS}, {"gradient_norm", ilqr::S_GRADIENT_NORM},
        {"outer_iterations", ilqr::S_OUTER_ITERATIONS}, {"potrf_info", ilqr::S_POTRF_INFO}, {"rollouts", ilqr::S_ROLLOUTS},
        {"states_eq_nominal", ilqr::S_STATES_EQ_NOMINAL}, {"profile", ilqr::S_PROF}, {"done", ilqr::S_DONE},
        {"delta_grad_product", ilqr::S_DELTA}, {"trace_len", ilqr::S_TRACE_LEN}, {"count", ilqr::S_COUNT},
        {"obj_prev", ilqr::S_OBJ_PREV}, {"inner_done", ilqr::S_INNER_DONE}, {"j_prev", ilqr::S_J_PREV}, {"inner_it", ilqr::S_INNER_IT},
        {"resume", ilqr::S_RESUME}, {"literal_backward_passes", ilqr::S_LITERAL_PASSES},
        {"t_start", ilqr::S_T_START}, {"t_end", ilqr::S_T_END}, {"hw_id_wave0", ilqr::S_HW0}, {"hw_id_wave1", ilqr::S_HW1}, {"hw_id_wave2", ilqr::S_HW2}, {"hw_id_wave3", ilqr::S_HW3},
    };
    if (!name) return -1;
    for (auto& s_ : slots)
        if (!std::strcmp(s_.n, name)) return s_.i;
    return -1;
}

int ilqr_get_buffer(ilqr_handle* h, const char* name, double* out) {
    if (!h || !name || !out) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) {
        size_t len = 0;
        const int rc = ilqr_buffer_len(h, name, &len);
        if (rc != ILQR_OK) return rc;
        return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_get_buffer(s, name, out + lo * len); }, true);
    }
    if (const BufferDesc* qd = find_qbuffer(h, name)) {
        if (!h->qv) return fail(ILQR_ERR_INVALID, "action-value buffers are off: call ilqr_enable_action_value_buffers first");
        if (qd->len == 0) return ILQR_OK;
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy2D(out, (size_t)qd->len * 8, h->qv + qd->offset, (size_t)h->QL.stride * 8,
                            (size_t)qd->len * 8, (size_t)h->B, hipMemcpyDeviceToHost));
        return ILQR_OK;
    }
    const BufferDesc* bd = find_buffer(h, name);
    if (!bd) return fail(ILQR_ERR_INVALID, std::string("unknown buffer '") + name + "'");
    return copy_out(h, bd, out);
}
int ilqr_set_buffer(ilqr_handle* h, const char* name, const double* in) {
    if (!h || !name || !in) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) {
        size_t len = 0;
        const int rc = ilqr_buffer_len(h, name, &len);
        if (rc != ILQR_OK) return rc;
        return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_set_buffer(s, name, in + lo * len); }, true);
    }
    const BufferDesc* bd = find_buffer(h, name);
    if (!bd) return fail(ILQR_ERR_INVALID, std::string("unknown buffer '") + name + "'");
    const int rc = copy_in(h, bd, in);
    if (rc == ILQR_OK && (bd->offset == h->L.K || bd->offset == h->L.k)) h->has_policy = true;      // the caller's own policy
    if (rc == ILQR_OK && !std::strcmp(bd->name, "constraint_penalty")) h->has_duals = true;      // the caller's own penalties
    return rc;
}

// ---- closed-loop rollouts of the handle's policy from the caller's initial states (ilqr_device_policy.hpp)
// everything that can be refused without touching the GPU
static int policy_check(const ilqr_handle* h, int32_t samples, const double* x1, const double* w, const double* cost, const char* who) {
    const std::string me(who);
    if (samples < 1) return fail(ILQR_ERR_INVALID, me + ": samples must be >= 1");
    if (!x1) return fail(ILQR_ERR_INVALID, me + ": null x1");
    if (!cost) return fail(ILQR_ERR_INVALID, me + ": null cost");
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (w && h->vt->nw - h->n_sel <= 0) return fail(ILQR_ERR_INVALID, me + ": w given, but this model has no parameters (num_parameter == 0)");
    if (!every_shard_holds(h, &ilqr_handle::has_policy))
        return fail(ILQR_ERR_INVALID, me + ": the handle holds no policy yet (no solve and no backward_pass stage has run since the last reset)");
    return ILQR_OK;
}

static int policy_launch(ilqr_handle* h, int32_t samples, double step_size, const double* x1, const double* w, double* cost,
                         double* max_violation, int32_t* first_nonfinite, double* x, double* u) {
    if (!h->vt->launch_policy_rollout) return fail(ILQR_ERR_MODEL, "this model module has no policy rollout kernel");
    ilqr::PolicyArgs a;
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.S = samples; a.constrained = h->constrained; a.n_sel = h->n_sel;
    a.waves = waves_for(samples);
    a.alpha = step_size; a.x1 = x1; a.w = w; a.cost = cost; a.viol = max_violation; a.nonfinite = first_nonfinite; a.x = x; a.u = u;
    if (h->vt->launch_policy_rollout(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "policy rollout launch failed");
    return ILQR_OK;
}

int ilqr_rollout_policy_device(ilqr_handle* h, int32_t samples, double step_size, const double* x1, const double* w, double* cost,
                               double* max_violation, int32_t* first_nonfinite, double* x, double* u) {
    ILQR_TRY(policy_check(h, samples, x1, w, cost, "ilqr_rollout_policy_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_rollout_policy");
    HIP_TRY(hipSetDevice(h->device));
    return policy_launch(h, samples, step_size, x1, w, cost, max_violation, first_nonfinite, x, u);
}

int ilqr_rollout_policy(ilqr_handle* h, int32_t samples, double step_size, const double* x1, const double* w, double* cost,
                        double* max_violation, int32_t* first_nonfinite, double* x, double* u) {
    ILQR_TRY(policy_check(h, samples, x1, w, cost, "ilqr_rollout_policy"));
    const size_t S = (size_t)samples, T = (size_t)h->L.T, N = T - 1, n = (size_t)h->L.nx, m = (size_t)h->L.nu, nwu = (size_t)(h->L.nw - h->n_sel);
    return run_staged(h, {staged_in(IN_POL, POL_X1, x1, S * n), staged_in(IN_POL, POL_W, w, S * T * nwu), staged_out(IN_POL, POL_COST, cost, S),
                          staged_out(IN_POL, POL_VIOL, max_violation, S), staged_out(IN_POL, POL_NONFINITE, first_nonfinite, S),
                          staged_out(IN_POL, POL_X, x, S * T * n), staged_out(IN_POL, POL_U, u, S * N * m)},
                      [&](ilqr_handle* s, size_t, const Staged* a) {
                          return policy_launch(s, samples, step_size, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].i(), a[5].d(), a[6].d()); });
}

// ---- scoring and selection of candidate initial guesses (ilqr_device_candidates.hpp), then the existing init_rollout on the winners
// everything that can be refused without touching the GPU, before the handle is looked at
static int candidates_check(const ilqr_handle* h, int32_t candidates, double violation_weight, const double* x1, const double* u, const char* who) {
    const std::string me(who);
    if (candidates < 1) return fail(ILQR_ERR_INVALID, me + ": candidates must be >= 1");
    if (!x1) return fail(ILQR_ERR_INVALID, me + ": null x1");
    if (!u) return fail(ILQR_ERR_INVALID, me + ": null u");
    if (!(violation_weight >= 0.0) || !std::isfinite(violation_weight)) return fail(ILQR_ERR_INVALID, me + ": violation_weight must be finite and >= 0");
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    return ILQR_OK;
}

// every pointer a device pointer on h's device; x1 may be h->d_x1 itself. Null outputs are replaced by the handle's own buffers.
static int candidates_launch(ilqr_handle* h, int32_t candidates, double violation_weight, const double* x1, const double* u, int32_t* chosen,
                             double* cost, double* max_violation, int32_t* first_nonfinite) {
    if (!h->vt->launch_candidates) return fail(ILQR_ERR_MODEL, "this model module has no candidate scoring kernel");
    const size_t BS = (size_t)h->B * (size_t)candidates;
    ILQR_TRY(own_if_null(h, cost, h->cand[CAND_COST], BS * 8));
    ILQR_TRY(own_if_null(h, max_violation, h->cand[CAND_VIOL], BS * 8));
    ILQR_TRY(own_if_null(h, first_nonfinite, h->cand[CAND_NONFINITE], BS * 4));
    ilqr::CandArgs a;
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.S = candidates; a.constrained = h->constrained;
    a.waves = waves_for(candidates);
    a.weight = violation_weight; a.x1 = x1; a.u = u; a.cost = cost; a.viol = max_violation; a.nonfinite = first_nonfinite; a.chosen = chosen;
    a.r_x1 = h->d_x1; a.r_u = h->d_u;
    if (h->vt->launch_candidates(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "candidate scoring launch failed");
    return ilqr_initialize_rollout_device(h, h->d_x1, h->d_u);       // the code that defines the installed state
}

int ilqr_initialize_rollout_candidates_device(ilqr_handle* h, int32_t candidates, double violation_weight, const double* x1, const double* u,
                                              int32_t* chosen, double* cost, double* max_violation, int32_t* first_nonfinite) {
    ILQR_TRY(candidates_check(h, candidates, violation_weight, x1, u, "ilqr_initialize_rollout_candidates_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_initialize_rollout_candidates");
    HIP_TRY(hipSetDevice(h->device));
    ILQR_TRY(resident_inputs(h));
    return candidates_launch(h, candidates, violation_weight, x1, u, chosen, cost, max_violation, first_nonfinite);
}

int ilqr_initialize_rollout_candidates(ilqr_handle* h, int32_t candidates, double violation_weight, const double* x1, const double* u,
                                       int32_t* chosen, double* cost, double* max_violation, int32_t* first_nonfinite) {
    ILQR_TRY(candidates_check(h, candidates, violation_weight, x1, u, "ilqr_initialize_rollout_candidates"));
    const size_t S = (size_t)candidates, N = (size_t)h->L.T - 1, n = (size_t)h->L.nx, m = (size_t)h->L.nu;
    // x1 goes straight into the resident input (N == 0: no actions to stage; the launch gets d_u instead)
    return run_staged(h, {staged_in(IN_RESIDENT, 0, x1, n), staged_in(IN_CAND, CAND_U, u, S * N * m), staged_out(IN_CAND, CAND_COST, cost, S),
                          staged_out(IN_CAND, CAND_VIOL, max_violation, S), staged_out(IN_CAND, CAND_NONFINITE, first_nonfinite, S),
                          staged_out(IN_CAND, CAND_CHOSEN, chosen, 1)},
                      [&](ilqr_handle* s, size_t, const Staged* a) {
                          return candidates_launch(s, candidates, violation_weight, s->d_x1, a[1].p ? a[1].d() : s->d_u, a[5].i(), a[2].d(), a[3].d(), a[4].i()); });
}

// ---- candidates drawn on the device around a base sequence (ilqr_device_sample.hpp), then the existing init_rollout on what was installed
// everything that can be refused without touching the GPU; what needs no handle comes first
static int sample_check(const ilqr_handle* h, int32_t candidates, int32_t mode, int64_t first_instance, const double* sigma, double violation_weight,
                        double temperature, const double* x1, const double* base_u, const char* who) {
    const std::string me(who);
    if (candidates < 1 || candidates > ilqr::SAMPLE_MAX_CANDIDATES) return fail(ILQR_ERR_INVALID, me + ": candidates must lie in 1 .. 65536");
    if (mode != ILQR_SAMPLE_PICK && mode != ILQR_SAMPLE_BLEND) return fail(ILQR_ERR_INVALID, me + ": unknown mode");
    if (!sigma) return fail(ILQR_ERR_INVALID, me + ": null sigma");
    if (!(sigma[0] >= 0.0) || !std::isfinite(sigma[0])) return fail(ILQR_ERR_INVALID, me + ": sigma must be finite and >= 0");
    if (!(violation_weight >= 0.0) || !std::isfinite(violation_weight)) return fail(ILQR_ERR_INVALID, me + ": violation_weight must be finite and >= 0");
    if (mode == ILQR_SAMPLE_BLEND && (!(temperature > 0.0) || !std::isfinite(temperature))) return fail(ILQR_ERR_INVALID, me + ": temperature must be finite and > 0");
    if (first_instance < 0 || first_instance >= ilqr::SAMPLE_MAX_INSTANCES) return fail(ILQR_ERR_INVALID, me + ": first_instance must lie in 0 .. 2^23 - 1");
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (h->L.nu > ilqr::SAMPLE_MAX_NU) return fail(ILQR_ERR_INVALID, me + ": more than 16 action components");
    for (int j = 0; j < h->L.nu; ++j)
        if (!(sigma[j] >= 0.0) || !std::isfinite(sigma[j])) return fail(ILQR_ERR_INVALID, me + ": sigma must be finite and >= 0");
    if (h->L.T - 1 > ilqr::SAMPLE_MAX_STEPS) return fail(ILQR_ERR_INVALID, me + ": more than 2^20 steps");
    if (first_instance + (int64_t)h->B > ilqr::SAMPLE_MAX_INSTANCES) return fail(ILQR_ERR_INVALID, me + ": first_instance + batch must not exceed 2^23");
    if ((!x1 && !every_shard_holds(h, &ilqr_handle::d_x1)) || (!base_u && !every_shard_holds(h, &ilqr_handle::d_u)))
        return fail(ILQR_ERR_INVALID, me + ": NULL x1 / base_u mean the handle's resident inputs, and it holds none yet (no initialize_rollout or shift has run)");
    return ILQR_OK;
}

// every pointer but sigma a device pointer on h's device; x1 / base_u may be h->d_x1 / h->d_u themselves. Null outputs are replaced by
// the handle's own buffers where a kernel needs them.
static int sample_launch(ilqr_handle* h, int32_t candidates, int32_t mode, uint64_t seed, int64_t first_instance, const double* sigma,
                         double violation_weight, double temperature, const double* x1, const double* base_u, int32_t* chosen, double* cost,
                         double* max_violation, int32_t* first_nonfinite, double* weights, double* u_out) {
    if (!h->vt->launch_sample_candidates) return fail(ILQR_ERR_MODEL, "this model module has no candidate sampling kernel");
    ILQR_TRY(resident_inputs(h));
    const size_t BS = (size_t)h->B * (size_t)candidates, nu = (size_t)h->L.nu;
    ILQR_TRY(own_if_null(h, cost, h->cand[CAND_COST], BS * 8));
    ILQR_TRY(own_if_null(h, max_violation, h->cand[CAND_VIOL], BS * 8));
    ILQR_TRY(own_if_null(h, first_nonfinite, h->cand[CAND_NONFINITE], BS * 4));
    ILQR_TRY(own_if_null(h, chosen, h->cand[CAND_CHOSEN], (size_t)h->B * 4));
    if (mode == ILQR_SAMPLE_BLEND) ILQR_TRY(own_if_null(h, weights, h->samp[SAMP_WEIGHTS], BS * 8));
    h->sample_sigma.assign(sigma, sigma + nu);        // the caller's array may go away before the (asynchronous) copy has read it
    ILQR_TRY(grow(h, h->samp[SAMP_SIGMA], nu * 8));
    HIP_TRY(hipMemcpyAsync(h->samp[SAMP_SIGMA].p, h->sample_sigma.data(), nu * 8, hipMemcpyHostToDevice, h->stream));
    ilqr::SampleArgs a;
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.S = candidates; a.constrained = h->constrained;
    a.waves = waves_for(candidates);
    a.weight = violation_weight; a.x1 = x1 ? x1 : h->d_x1; a.u = nullptr; a.cost = cost; a.viol = max_violation; a.nonfinite = first_nonfinite; a.chosen = chosen;
    a.r_x1 = h->d_x1; a.r_u = h->d_u;
    a.seed = seed; a.b0 = first_instance; a.sigma = (const double*)h->samp[SAMP_SIGMA].p; a.base = base_u ? base_u : h->d_u; a.u_out = u_out; a.weights = weights;
    a.mode = mode; a.temperature = temperature;
    if (h->vt->launch_sample_candidates(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "candidate sampling launch failed");
    return ilqr_initialize_rollout_device(h, h->d_x1, h->d_u);       // the code that defines the installed state
}

int ilqr_sample_rollout_candidates_device(ilqr_handle* h, int32_t candidates, int32_t mode, uint64_t seed, int64_t first_instance, const double* sigma,
                                          double violation_weight, double temperature, const double* x1, const double* base_u, int32_t* chosen,
                                          double* cost, double* max_violation, int32_t* first_nonfinite, double* weights, double* u_out) {
    ILQR_TRY(sample_check(h, candidates, mode, first_instance, sigma, violation_weight, temperature, x1, base_u, "ilqr_sample_rollout_candidates_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_sample_rollout_candidates");
    HIP_TRY(hipSetDevice(h->device));
    return sample_launch(h, candidates, mode, seed, first_instance, sigma, violation_weight, temperature, x1, base_u, chosen, cost, max_violation,
                         first_nonfinite, weights, u_out);
}

int ilqr_sample_rollout_candidates(ilqr_handle* h, int32_t candidates, int32_t mode, uint64_t seed, int64_t first_instance, const double* sigma,
                                   double violation_weight, double temperature, const double* x1, const double* base_u, int32_t* chosen,
                                   double* cost, double* max_violation, int32_t* first_nonfinite, double* weights, double* u_out) {
    ILQR_TRY(sample_check(h, candidates, mode, first_instance, sigma, violation_weight, temperature, x1, base_u, "ilqr_sample_rollout_candidates"));
    const size_t S = (size_t)candidates, N = (size_t)h->L.T - 1, n = (size_t)h->L.nx, m = (size_t)h->L.nu;
    // the caller's x1 and base go straight into the resident inputs: the installation works in place
    return run_staged(h, {staged_in(IN_RESIDENT, 0, x1, n), staged_in(IN_RESIDENT, 1, base_u, N * m), staged_out(IN_CAND, CAND_COST, cost, S),
                          staged_out(IN_CAND, CAND_VIOL, max_violation, S), staged_out(IN_CAND, CAND_NONFINITE, first_nonfinite, S),
                          staged_out(IN_CAND, CAND_CHOSEN, chosen, 1), staged_out(IN_SAMP, SAMP_WEIGHTS, weights, S),
                          staged_out(IN_SAMP, SAMP_U_OUT, u_out, S * N * m)},
                      [&](ilqr_handle* s, size_t lo, const Staged* a) {
                          return sample_launch(s, candidates, mode, seed, first_instance + (int64_t)lo, sigma, violation_weight, temperature, s->d_x1,
                                               s->d_u, a[5].i(), a[2].d(), a[3].d(), a[4].i(), a[6].d(), a[7].d()); });
}

// ---- receding-horizon shift (ilqr_device_shift.hpp), then the existing init_rollout on the shifted inputs
// everything that can be refused without touching the GPU
static int shift_check(const ilqr_handle* h, int32_t steps, int32_t tail, int32_t feedback, const double* w_tail, const char* who) {
    const std::string me(who);
    if (steps < 0) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 0 .. T-1");
    if (tail != ILQR_SHIFT_TAIL_HOLD && tail != ILQR_SHIFT_TAIL_ZERO) return fail(ILQR_ERR_INVALID, me + ": unknown tail mode");
    if (w_tail && steps == 0) return fail(ILQR_ERR_INVALID, me + ": w_tail given with steps == 0: no parameter row enters the horizon");
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (steps > h->L.T - 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 0 .. T-1");
    if (w_tail && h->vt->nw - h->n_sel <= 0) return fail(ILQR_ERR_INVALID, me + ": w_tail given, but this model has no parameters (num_parameter == 0)");
    if (steps > 0 && h->n_sel > 0)
        return fail(ILQR_ERR_INVALID, me + ": the handle has stage selectors attached: the structure of a lowered problem belongs to horizon positions and cannot be shifted");
    if (feedback && !every_shard_holds(h, &ilqr_handle::has_policy))
        return fail(ILQR_ERR_INVALID, me + ": the handle holds no policy yet (no solve and no backward_pass stage has run since the last reset)");
    return ILQR_OK;
}

// x1, w_tail: null or device pointers on h's device. w_tail_ld < 0: the rows of ONE call, [B][steps][nw]; else instance b's rows
// start at row b · w_tail_ld + w_tail_row0 (the loop's run-long array)
static int shift_launch(ilqr_handle* h, int32_t steps, int32_t tail, int32_t feedback, const double* x1, const double* w_tail,
                        long long w_tail_ld, long long w_tail_row0) {
    if (!h->vt->launch_shift) return fail(ILQR_ERR_MODEL, "this model module has no horizon shift kernel");
    ILQR_TRY(resident_inputs(h));
    ilqr::ShiftArgs a;
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.steps = steps; a.tail = tail; a.feedback = feedback ? 1 : 0; a.phase = 0;
    a.x1 = x1; a.w_tail = w_tail; a.w_stage = nullptr; a.r_x1 = h->d_x1; a.r_u = h->d_u;
    a.w_tail_ld = w_tail_ld < 0 ? steps : w_tail_ld; a.w_tail_row0 = w_tail_ld < 0 ? 0 : w_tail_row0;
    if (steps > 0 && h->L.nw > 0) {            // (no selectors here: every parameter column is the user's)
        ILQR_TRY(grow(h, h->shift[SHIFT_W_STAGE], (size_t)h->B * h->L.T * h->L.nw * 8));
        a.w_stage = (double*)h->shift[SHIFT_W_STAGE].p;
    }
    if (h->vt->launch_shift(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "horizon shift launch failed");
    return ilqr_initialize_rollout_device(h, h->d_x1, h->d_u);       // the code that defines the installed state
}

int ilqr_shift_horizon_device(ilqr_handle* h, int32_t steps, int32_t tail, int32_t feedback, const double* x1, const double* w_tail) {
    ILQR_TRY(shift_check(h, steps, tail, feedback, w_tail, "ilqr_shift_horizon_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_shift_horizon");
    HIP_TRY(hipSetDevice(h->device));
    return shift_launch(h, steps, tail, feedback, x1, w_tail, -1, 0);
}

int ilqr_shift_horizon(ilqr_handle* h, int32_t steps, int32_t tail, int32_t feedback, const double* x1, const double* w_tail) {
    ILQR_TRY(shift_check(h, steps, tail, feedback, w_tail, "ilqr_shift_horizon"));
    const size_t n = (size_t)h->L.nx, kw = (size_t)steps * (size_t)(h->L.nw - h->n_sel);
    // (inputs only: what comes back is the synchronise, after which the caller may reuse its host arrays)
    return run_staged(h, {staged_in(IN_SHIFT, SHIFT_X1, x1, n), staged_in(IN_SHIFT, SHIFT_W_TAIL, w_tail, kw)},
                      [&](ilqr_handle* s, size_t, const Staged* a) { return shift_launch(s, steps, tail, feedback, a[0].d(), a[1].d(), -1, 0); });
}

// ---- receding-horizon shift of the duals and penalties (ilqr_device_duals.hpp)
// everything that can be refused without touching the GPU
static int duals_check(const ilqr_handle* h, int32_t steps, int32_t tail, int32_t penalty, const char* who) {
    const std::string me(who);
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (!h->constrained) return fail(ILQR_ERR_INVALID, me + ": the handle was created unconstrained: it has no duals to shift");
    if (steps < 0 || steps > h->L.T - 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 0 .. T-1");
    if (tail != ILQR_DUALS_TAIL_HOLD && tail != ILQR_DUALS_TAIL_ZERO) return fail(ILQR_ERR_INVALID, me + ": unknown tail mode");
    if (penalty != ILQR_DUALS_PENALTY_KEEP && penalty != ILQR_DUALS_PENALTY_RESET) return fail(ILQR_ERR_INVALID, me + ": unknown penalty mode");
    if (steps > 0 && h->n_sel > 0)
        return fail(ILQR_ERR_INVALID, me + ": the handle has stage selectors attached: the structure of a lowered problem belongs to horizon positions and cannot be shifted");
    if (!every_shard_holds(h, &ilqr_handle::has_duals)) return fail(ILQR_ERR_INVALID, me + ": the handle holds no duals yet (no constrained solve, no al_begin stage and no host write of constraint_penalty since the last reset)");
    return ILQR_OK;
}

int ilqr_shift_duals_device(ilqr_handle* h, int32_t steps, int32_t tail, int32_t penalty) {
    ILQR_TRY(duals_check(h, steps, tail, penalty, "ilqr_shift_duals_device"));
    if (SHARDED(h)) return fail(ILQR_ERR_INVALID, "ilqr_shift_duals_device: a sharded handle has one stream per device: call ilqr_shift_duals on it");
    if (!h->vt->launch_shift_duals) return fail(ILQR_ERR_MODEL, "this model module has no dual shift kernel");
    HIP_TRY(hipSetDevice(h->device));
    ilqr::DualsArgs a;
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.steps = steps; a.tail = tail; a.penalty = penalty; a.rho0 = h->opt.initial_constraint_penalty;
    if (h->vt->launch_shift_duals(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "dual shift launch failed");
    return ILQR_OK;
}

int ilqr_shift_duals(ilqr_handle* h, int32_t steps, int32_t tail, int32_t penalty) {
    ILQR_TRY(duals_check(h, steps, tail, penalty, "ilqr_shift_duals"));
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_shift_duals(s, steps, tail, penalty); });
    ILQR_TRY(ilqr_shift_duals_device(h, steps, tail, penalty));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ILQR_OK;
}

// ---- the plant of a closed MPC loop (ilqr_device_plant.hpp): the head of the plan applied to the dynamics from a plant state in HBM
// a standard deviation vector (sigma_x, sigma_y): finite and >= 0; its first `count` entries
static int sigma_check(const double* sigma, int count, const std::string& me, const char* name) {
    for (int j = 0; sigma && j < count; ++j)
        if (!(sigma[j] >= 0.0) || !std::isfinite(sigma[j])) return fail(ILQR_ERR_INVALID, me + ": " + name + " must be finite and >= 0");
    return ILQR_OK;
}
// the actuator's limits: no NaN, u_min <= u_max; their first `count` entries (a null vector: no limit on that side)
static int limits_check(const double* u_min, const double* u_max, int count, const std::string& me) {
    for (int j = 0; j < count; ++j) {
        if ((u_min && std::isnan(u_min[j])) || (u_max && std::isnan(u_max[j]))) return fail(ILQR_ERR_INVALID, me + ": a limit of the actuator is NaN");
        if (u_min && u_max && u_min[j] > u_max[j]) return fail(ILQR_ERR_INVALID, me + ": u_min must not exceed u_max");
    }
    return ILQR_OK;
}

// everything that can be refused without touching the GPU; what needs no handle comes first (of a vector: its first entry)
static int plant_check(const ilqr_handle* h, int32_t steps, int32_t feedback, int64_t first_instance, int64_t step0, int64_t total_steps,
                       const double* sigma_x, const double* u_min, const double* u_max, const double* w_plant, const char* who) {
    const std::string me(who);
    if (steps < 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 1 .. T-1");
    if (step0 < 0 || step0 + total_steps > ilqr::PLANT_MAX_STEPS) return fail(ILQR_ERR_INVALID, me + ": step0 >= 0 and no plant step index beyond 2^20 (the noise key's bit fields)");
    if (first_instance < 0 || first_instance >= ilqr::PLANT_MAX_INSTANCES) return fail(ILQR_ERR_INVALID, me + ": first_instance must lie in 0 .. 2^23 - 1");
    ILQR_TRY(sigma_check(sigma_x, 1, me, "sigma_x"));
    ILQR_TRY(limits_check(u_min, u_max, 1, me));
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (steps > h->L.T - 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 1 .. T-1");
    if (h->L.nx > ilqr::PLANT_MAX_NX) return fail(ILQR_ERR_INVALID, me + ": more than 64 state components");
    ILQR_TRY(sigma_check(sigma_x, h->L.nx, me, "sigma_x"));
    if ((u_min || u_max) && h->L.nu > ilqr::PLANT_MAX_NU) return fail(ILQR_ERR_INVALID, me + ": limits on more than 16 action components");
    ILQR_TRY(limits_check(u_min, u_max, h->L.nu, me));
    if (first_instance + (int64_t)h->B > ilqr::PLANT_MAX_INSTANCES) return fail(ILQR_ERR_INVALID, me + ": first_instance + batch must not exceed 2^23");
    if (w_plant && h->vt->nw - h->n_sel <= 0) return fail(ILQR_ERR_INVALID, me + ": w_plant given, but this model has no parameters (num_parameter == 0)");
    if (feedback && !every_shard_holds(h, &ilqr_handle::has_policy))
        return fail(ILQR_ERR_INVALID, me + ": the handle holds no policy yet (no solve and no backward_pass stage has run since the last reset)");
    return ILQR_OK;
}

// what a plant launch takes of the handle and of the call; the arrays are the caller's to fill in
static ilqr::PlantArgs plant_args(const ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                                  const double* sigma_x, const double* u_min, const double* u_max) {
    ilqr::PlantArgs a = {};
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.steps = steps; a.feedback = feedback ? 1 : 0; a.n_sel = h->n_sel; a.step0 = step0;
    a.noise = sigma_x != nullptr; a.nf_global = 0; a.seed = seed; a.b0 = first_instance;
    for (int j = 0; sigma_x && j < h->L.nx; ++j) a.sigma[j] = sigma_x[j];      // by value: the caller's array may go away at once
    a.clamp = (u_min || u_max) ? 1 : 0;
    for (int j = 0; a.clamp && j < h->L.nu; ++j) {
        a.u_lo[j] = u_min ? u_min[j] : -HUGE_VAL;
        a.u_hi[j] = u_max ? u_max[j] : HUGE_VAL;
    }
    return a;
}

// every pointer null or a device pointer on h's device; the arrays of ONE call: `steps` rows per instance (x_out: one more)
static int plant_launch(ilqr_handle* h, ilqr::PlantArgs a, const double* w_plant, double* x, double* x_out, double* u_out, int32_t* first_nonfinite,
                        int32_t* saturated) {
    if (!h->vt->launch_plant) return fail(ILQR_ERR_MODEL, "this model module has no plant kernel");
    a.w = w_plant; a.x = x; a.x_out = x_out; a.u_out = u_out; a.nonfinite = first_nonfinite; a.saturated = saturated;
    a.w_ld = a.steps; a.x_ld = a.steps + 1; a.u_ld = a.steps;
    if (h->vt->launch_plant(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "plant step launch failed");
    return ILQR_OK;
}

// ilqr_plant_step_device is this with u_min, u_max and saturated null: no buffer and no argument of the launch changes then
static int plant_step_device(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                             const double* sigma_x, const double* u_min, const double* u_max, const double* w_plant, double* x, double* x_out,
                             double* u_out, int32_t* first_nonfinite, int32_t* saturated, const char* who, const char* host_form) {
    if (!x) return fail(ILQR_ERR_INVALID, std::string(who) + ": null x");
    ILQR_TRY(plant_check(h, steps, feedback, first_instance, step0, steps, sigma_x, u_min, u_max, w_plant, who));
    if (SHARDED(h)) return refuse_sharded(host_form);
    HIP_TRY(hipSetDevice(h->device));
    return plant_launch(h, plant_args(h, steps, feedback, seed, first_instance, step0, sigma_x, u_min, u_max), w_plant, x, x_out, u_out,
                        first_nonfinite, saturated);
}

int ilqr_plant_step_device(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                           const double* sigma_x, const double* w_plant, double* x, double* x_out, double* u_out, int32_t* first_nonfinite) {
    return plant_step_device(h, steps, feedback, seed, first_instance, step0, sigma_x, nullptr, nullptr, w_plant, x, x_out, u_out, first_nonfinite,
                             nullptr, "ilqr_plant_step_device", "ilqr_plant_step");
}

int ilqr_plant_step_limited_device(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                                   const double* sigma_x, const double* u_min, const double* u_max, const double* w_plant, double* x,
                                   double* x_out, double* u_out, int32_t* first_nonfinite, int32_t* saturated) {
    return plant_step_device(h, steps, feedback, seed, first_instance, step0, sigma_x, u_min, u_max, w_plant, x, x_out, u_out, first_nonfinite,
                             saturated, "ilqr_plant_step_limited_device", "ilqr_plant_step_limited");
}

// ilqr_plant_step is this with u_min, u_max and saturated null
static int plant_step(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0, const double* sigma_x,
                      const double* u_min, const double* u_max, const double* w_plant, double* x, double* x_out, double* u_out,
                      int32_t* first_nonfinite, int32_t* saturated, const char* who) {
    if (!x) return fail(ILQR_ERR_INVALID, std::string(who) + ": null x");
    ILQR_TRY(plant_check(h, steps, feedback, first_instance, step0, steps, sigma_x, u_min, u_max, w_plant, who));
    const size_t k = (size_t)steps, n = (size_t)h->L.nx, m = (size_t)h->L.nu, nwu = (size_t)(h->L.nw - h->n_sel);
    // the plant state goes in and comes back
    return run_staged(h, {staged_io(IN_PLANT, PLANT_X, x, n), staged_in(IN_PLANT, PLANT_W, w_plant, k * nwu), staged_out(IN_PLANT, PLANT_X_OUT, x_out, (k + 1) * n),
                          staged_out(IN_PLANT, PLANT_U_OUT, u_out, k * m), staged_out(IN_PLANT, PLANT_NONFINITE, first_nonfinite, 1),
                          staged_out(IN_PLANT, PLANT_SATURATED, saturated, 1)},
                      [&](ilqr_handle* s, size_t lo, const Staged* a) {
                          return plant_launch(s, plant_args(s, steps, feedback, seed, first_instance + (int64_t)lo, step0, sigma_x, u_min, u_max), a[1].d(),
                                              a[0].d(), a[2].d(), a[3].d(), a[4].i(), a[5].i()); });
}

int ilqr_plant_step(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                    const double* sigma_x, const double* w_plant, double* x, double* x_out, double* u_out, int32_t* first_nonfinite) {
    return plant_step(h, steps, feedback, seed, first_instance, step0, sigma_x, nullptr, nullptr, w_plant, x, x_out, u_out, first_nonfinite, nullptr,
                      "ilqr_plant_step");
}

int ilqr_plant_step_limited(ilqr_handle* h, int32_t steps, int32_t feedback, uint64_t seed, int64_t first_instance, int32_t step0,
                            const double* sigma_x, const double* u_min, const double* u_max, const double* w_plant, double* x, double* x_out,
                            double* u_out, int32_t* first_nonfinite, int32_t* saturated) {
    return plant_step(h, steps, feedback, seed, first_instance, step0, sigma_x, u_min, u_max, w_plant, x, x_out, u_out, first_nonfinite, saturated,
                      "ilqr_plant_step_limited");
}

// ---- what the controller is given of a plant state (plant_measure_kernel, ilqr_device_plant.hpp)
// everything that can be refused without touching the GPU; what needs no handle comes first (of sigma_y: its first entry)
static int measure_check(const ilqr_handle* h, int64_t first_instance, int64_t step, const double* sigma_y, const char* who) {
    const std::string me(who);
    if (step < 0 || step >= ilqr::PLANT_MAX_STEPS) return fail(ILQR_ERR_INVALID, me + ": the measurement step must lie in 0 .. 2^20 - 1 (the noise key's bit fields)");
    if (first_instance < 0 || first_instance >= ilqr::PLANT_MAX_INSTANCES) return fail(ILQR_ERR_INVALID, me + ": first_instance must lie in 0 .. 2^23 - 1");
    ILQR_TRY(sigma_check(sigma_y, 1, me, "sigma_y"));
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (h->L.nx > ilqr::PLANT_MAX_NX) return fail(ILQR_ERR_INVALID, me + ": more than 64 state components");
    ILQR_TRY(sigma_check(sigma_y, h->L.nx, me, "sigma_y"));
    if (first_instance + (int64_t)h->B > ilqr::PLANT_MAX_INSTANCES) return fail(ILQR_ERR_INVALID, me + ": first_instance + batch must not exceed 2^23");
    return ILQR_OK;
}

// x, y: device pointers on h's device, [B][nx] each (they may be the same array)
static int measure_launch(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, const double* sigma_y, const double* x, double* y) {
    if (!h->vt->launch_plant_measure) return fail(ILQR_ERR_MODEL, "this model module has no measurement kernel");
    ilqr::MeasureArgs a = {};
    a.B = h->B; a.noise = sigma_y != nullptr; a.step = step; a.seed = seed; a.b0 = first_instance; a.x = x; a.y = y;
    for (int j = 0; sigma_y && j < h->L.nx; ++j) a.sigma[j] = sigma_y[j];      // by value: the caller's array may go away at once
    if (h->vt->launch_plant_measure(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "measurement launch failed");
    return ILQR_OK;
}

int ilqr_plant_measure_device(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, const double* sigma_y, const double* x, double* y) {
    if (!x || !y) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_device: null x or y");
    ILQR_TRY(measure_check(h, first_instance, step, sigma_y, "ilqr_plant_measure_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_plant_measure");
    HIP_TRY(hipSetDevice(h->device));
    return measure_launch(h, seed, first_instance, step, sigma_y, x, y);
}

int ilqr_plant_measure(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, const double* sigma_y, const double* x, double* y) {
    if (!x || !y) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure: null x or y");
    ILQR_TRY(measure_check(h, first_instance, step, sigma_y, "ilqr_plant_measure"));
    const size_t n = (size_t)h->L.nx;
    return run_staged(h, {staged_in(IN_PLANT, PLANT_X, x, n), staged_out(IN_PLANT, PLANT_Y, y, n)}, [&](ilqr_handle* s, size_t lo, const Staged* a) {
        return measure_launch(s, seed, first_instance + (int64_t)lo, step, sigma_y, a[0].d(), a[1].d()); });
}

// ---- the realised stage cost and violation of plant steps (ilqr_device_score.hpp)
// everything that can be refused without touching the GPU; what needs no handle comes first
static int score_check(const ilqr_handle* h, int32_t steps, const double* w_plant, const double* x, const double* u, const double* cost,
                       const char* who) {
    const std::string me(who);
    if (steps < 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 1 .. T-1");
    if (!x) return fail(ILQR_ERR_INVALID, me + ": null x");
    if (!u) return fail(ILQR_ERR_INVALID, me + ": null u");
    if (!cost) return fail(ILQR_ERR_INVALID, me + ": null cost");
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (steps > h->L.T - 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 1 .. T-1");
    if (w_plant && h->vt->nw - h->n_sel <= 0) return fail(ILQR_ERR_INVALID, me + ": w_plant given, but this model has no parameters (num_parameter == 0)");
    return ILQR_OK;
}

// what a score launch takes of the handle; the arrays, their leading dimensions and row offsets are the caller's to fill in
static ilqr::ScoreArgs score_args(const ilqr_handle* h, int32_t steps) {
    ilqr::ScoreArgs a = {};
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.steps = steps; a.n_sel = h->n_sel; a.constrained = h->constrained;
    return a;
}

// every pointer a device pointer on h's device (w_plant, violation: or null); the arrays of ONE call: `steps` rows per instance
// (x: one more)
static int score_launch(ilqr_handle* h, int32_t steps, const double* w_plant, const double* x, const double* u, double* cost, double* violation) {
    if (!h->vt->launch_plant_score) return fail(ILQR_ERR_MODEL, "this model module has no plant score kernel");
    ilqr::ScoreArgs a = score_args(h, steps);
    a.w = w_plant; a.x = x; a.u = u; a.cost = cost; a.viol = violation;
    a.w_ld = a.u_ld = a.cost_ld = a.viol_ld = steps; a.x_ld = steps + 1;
    if (h->vt->launch_plant_score(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "plant score launch failed");
    return ILQR_OK;
}

int ilqr_plant_score_device(ilqr_handle* h, int32_t steps, const double* w_plant, const double* x, const double* u, double* cost, double* violation) {
    ILQR_TRY(score_check(h, steps, w_plant, x, u, cost, "ilqr_plant_score_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_plant_score");
    HIP_TRY(hipSetDevice(h->device));
    return score_launch(h, steps, w_plant, x, u, cost, violation);
}

int ilqr_plant_score(ilqr_handle* h, int32_t steps, const double* w_plant, const double* x, const double* u, double* cost, double* violation) {
    ILQR_TRY(score_check(h, steps, w_plant, x, u, cost, "ilqr_plant_score"));
    const size_t k = (size_t)steps, n = (size_t)h->L.nx, m = (size_t)h->L.nu, nwu = (size_t)(h->L.nw - h->n_sel);
    return run_staged(h, {staged_in(IN_PLANT, PLANT_W, w_plant, k * nwu), staged_in(IN_PLANT, PLANT_X_OUT, x, (k + 1) * n), staged_in(IN_PLANT, PLANT_U_OUT, u, k * m),
                          staged_out(IN_PLANT, PLANT_COST, cost, k), staged_out(IN_PLANT, PLANT_VIOL, violation, k)},
                      [&](ilqr_handle* s, size_t, const Staged* a) { return score_launch(s, steps, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].d()); });
}

// ---- the extended Kalman filter between sensor and controller (ilqr_device_estimate.hpp)
// a variance vector (q): finite and >= 0; (r): finite and > 0 where measured; a mask entry: 0 or 1; their first `count` entries
static int variance_check(const int32_t* measured, const double* q, const double* r, int count, const std::string& me) {
    for (int j = 0; j < count; ++j) {
        if (measured && measured[j] != 0 && measured[j] != 1) return fail(ILQR_ERR_INVALID, me + ": a mask entry must be 0 or 1");
        if (q && (!(q[j] >= 0.0) || !std::isfinite(q[j]))) return fail(ILQR_ERR_INVALID, me + ": q must be finite and >= 0");
        if (r && (!measured || measured[j]) && (!(r[j] > 0.0) || !std::isfinite(r[j])))
            return fail(ILQR_ERR_INVALID, me + ": r must be finite and > 0 where measured");
    }
    return ILQR_OK;
}

// everything that can be refused without touching the GPU; what needs no handle comes first (of a vector: its first entry)
static int predict_check(const ilqr_handle* h, int32_t steps, int32_t feedback, const double* u_min, const double* u_max, const double* q,
                         const char* who) {
    const std::string me(who);
    ILQR_TRY(variance_check(nullptr, q, nullptr, 1, me));
    ILQR_TRY(plant_check(h, steps, feedback, 0, 0, steps, nullptr, u_min, u_max, nullptr, who));
    return variance_check(nullptr, q, nullptr, h->L.nx, me);
}
static int update_check(const ilqr_handle* h, const int32_t* measured, const double* r, const char* who) {
    const std::string me(who);
    if (!r) return fail(ILQR_ERR_INVALID, me + ": null r");
    ILQR_TRY(variance_check(measured, nullptr, r, 1, me));
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (h->L.nx > ilqr::PLANT_MAX_NX) return fail(ILQR_ERR_INVALID, me + ": more than 64 state components");
    return variance_check(measured, nullptr, r, h->L.nx, me);
}

// xhat, P: device pointers on h's device
static int predict_launch(ilqr_handle* h, int32_t steps, int32_t feedback, const double* u_min, const double* u_max, const double* q, double* xhat,
                          double* P) {
    if (!h->vt->launch_estimate_predict) return fail(ILQR_ERR_MODEL, "this model module has no estimator kernel");
    ilqr::EstArgs a = {};
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.steps = steps; a.feedback = feedback ? 1 : 0; a.xhat = xhat; a.P = P;
    a.clamp = (u_min || u_max) ? 1 : 0;
    for (int j = 0; a.clamp && j < h->L.nu; ++j) {
        a.u_lo[j] = u_min ? u_min[j] : -HUGE_VAL;
        a.u_hi[j] = u_max ? u_max[j] : HUGE_VAL;
    }
    for (int j = 0; q && j < h->L.nx; ++j) a.q[j] = q[j];                      // by value: the caller's array may go away at once
    if (h->vt->launch_estimate_predict(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "estimator time update launch failed");
    return ILQR_OK;
}

// y, xhat, P, innovation, nis, first_bad: device pointers on h's device (the last three: or null)
static int update_launch(ilqr_handle* h, const int32_t* measured, const double* r, const double* y, double* xhat, double* P, double* innovation,
                         double* nis, int32_t* first_bad) {
    if (!h->vt->launch_estimate_update) return fail(ILQR_ERR_MODEL, "this model module has no estimator kernel");
    ilqr::EstArgs a = {};
    a.B = h->B; a.xhat = xhat; a.P = P; a.y = y; a.innovation = innovation; a.nis = nis; a.first_bad = first_bad;
    for (int j = 0; j < h->L.nx; ++j) {
        if (!measured || measured[j]) a.mask[j / 32] |= 1u << (j % 32);
        a.r[j] = r[j];
    }
    if (h->vt->launch_estimate_update(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "estimator measurement update launch failed");
    return ILQR_OK;
}

int ilqr_estimate_predict_device(ilqr_handle* h, int32_t steps, int32_t feedback, const double* u_min, const double* u_max, const double* q,
                                 double* xhat, double* P) {
    if (!xhat || !P) return fail(ILQR_ERR_INVALID, "ilqr_estimate_predict_device: null xhat or P");
    ILQR_TRY(predict_check(h, steps, feedback, u_min, u_max, q, "ilqr_estimate_predict_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_estimate_predict");
    HIP_TRY(hipSetDevice(h->device));
    return predict_launch(h, steps, feedback, u_min, u_max, q, xhat, P);
}

int ilqr_estimate_predict(ilqr_handle* h, int32_t steps, int32_t feedback, const double* u_min, const double* u_max, const double* q, double* xhat,
                          double* P) {
    if (!xhat || !P) return fail(ILQR_ERR_INVALID, "ilqr_estimate_predict: null xhat or P");
    ILQR_TRY(predict_check(h, steps, feedback, u_min, u_max, q, "ilqr_estimate_predict"));
    const size_t n = (size_t)h->L.nx;
    // the estimate and its covariance go in and come back
    return run_staged(h, {staged_io(IN_PLANT, PLANT_XC, xhat, n), staged_io(IN_PLANT, EST_P, P, n * n)}, [&](ilqr_handle* s, size_t, const Staged* a) {
        return predict_launch(s, steps, feedback, u_min, u_max, q, a[0].d(), a[1].d()); });
}

int ilqr_estimate_update_device(ilqr_handle* h, const int32_t* measured, const double* r, const double* y, double* xhat, double* P,
                                double* innovation, double* nis, int32_t* first_bad) {
    if (!xhat || !P || !y) return fail(ILQR_ERR_INVALID, "ilqr_estimate_update_device: null xhat, P or y");
    ILQR_TRY(update_check(h, measured, r, "ilqr_estimate_update_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_estimate_update");
    HIP_TRY(hipSetDevice(h->device));
    return update_launch(h, measured, r, y, xhat, P, innovation, nis, first_bad);
}

int ilqr_estimate_update(ilqr_handle* h, const int32_t* measured, const double* r, const double* y, double* xhat, double* P, double* innovation,
                         double* nis, int32_t* first_bad) {
    if (!xhat || !P || !y) return fail(ILQR_ERR_INVALID, "ilqr_estimate_update: null xhat, P or y");
    ILQR_TRY(update_check(h, measured, r, "ilqr_estimate_update"));
    const size_t n = (size_t)h->L.nx;
    return run_staged(h, {staged_in(IN_PLANT, EST_Y, y, n), staged_io(IN_PLANT, PLANT_XC, xhat, n), staged_io(IN_PLANT, EST_P, P, n * n),
                          staged_out(IN_PLANT, EST_INNOVATION, innovation, n), staged_out(IN_PLANT, EST_NIS, nis, 1), staged_out(IN_PLANT, EST_FIRST_BAD, first_bad, 1)},
                      [&](ilqr_handle* s, size_t, const Staged* a) {
                          return update_launch(s, measured, r, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].d(), a[5].i()); });
}

// ---- a state covariance down the plan under its feedback policy (ilqr_device_plancov.hpp)
// everything that can be refused without touching the GPU; what needs no handle comes first (of q: its first entry)
static int plancov_check(const ilqr_handle* h, int32_t steps, int32_t feedback, const double* q, const double* P0, bool any_output, const char* who) {
    const std::string me(who);
    if (steps < 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 1 .. T-1");
    if (feedback != 0 && feedback != 1) return fail(ILQR_ERR_INVALID, me + ": feedback must be 0 or 1");
    if (!P0) return fail(ILQR_ERR_INVALID, me + ": null P0");
    if (!any_output) return fail(ILQR_ERR_INVALID, me + ": every output is null");
    ILQR_TRY(variance_check(nullptr, q, nullptr, 1, me));
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (steps > h->L.T - 1) return fail(ILQR_ERR_INVALID, me + ": steps must lie in 1 .. T-1");
    if (h->L.nx > ilqr::PLANT_MAX_NX) return fail(ILQR_ERR_INVALID, me + ": more than 64 state components");
    if (h->L.nu > ilqr::PLANT_MAX_NU) return fail(ILQR_ERR_INVALID, me + ": more than 16 action components");
    ILQR_TRY(variance_check(nullptr, q, nullptr, h->L.nx, me));
    if (feedback && !every_shard_holds(h, &ilqr_handle::has_policy))
        return fail(ILQR_ERR_INVALID, me + ": the handle holds no policy yet (no solve and no backward_pass stage has run since the last reset)");
    return ILQR_OK;
}

// every pointer a device pointer on h's device (the outputs: or null)
static int plancov_launch(ilqr_handle* h, int32_t steps, int32_t feedback, const double* q, const double* P0, double* sdiag, double* udiag,
                          double* sigma, double* P_out, int32_t* first_nonfinite) {
    const ilqr_model_ext* e = find_ext(h->vt->name);
    if (!e || !e->launch_plan_covariance) return fail(ILQR_ERR_MODEL, "this model module has no plan covariance kernel");
    ilqr::PlanCovArgs a = {};
    a.ws = h->ws; a.L = h->L; a.B = h->B; a.steps = steps; a.feedback = feedback; a.P0 = P0; a.sdiag = sdiag; a.udiag = udiag; a.sigma = sigma;
    a.P_out = P_out; a.nonfinite = first_nonfinite;
    for (int j = 0; q && j < h->L.nx; ++j) a.q[j] = q[j];                      // by value: the caller's array may go away at once
    if (e->launch_plan_covariance(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "plan covariance launch failed");
    return ILQR_OK;
}

int ilqr_plan_covariance_device(ilqr_handle* h, int32_t steps, int32_t feedback, const double* q, const double* P0, double* sdiag, double* udiag,
                                double* sigma, double* P_out, int32_t* first_nonfinite) {
    ILQR_TRY(plancov_check(h, steps, feedback, q, P0, sdiag || udiag || sigma || P_out || first_nonfinite, "ilqr_plan_covariance_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_plan_covariance");
    HIP_TRY(hipSetDevice(h->device));
    return plancov_launch(h, steps, feedback, q, P0, sdiag, udiag, sigma, P_out, first_nonfinite);
}

int ilqr_plan_covariance(ilqr_handle* h, int32_t steps, int32_t feedback, const double* q, const double* P0, double* sdiag, double* udiag,
                         double* sigma, double* P_out, int32_t* first_nonfinite) {
    ILQR_TRY(plancov_check(h, steps, feedback, q, P0, sdiag || udiag || sigma || P_out || first_nonfinite, "ilqr_plan_covariance"));
    const size_t n = (size_t)h->L.nx, m = (size_t)h->L.nu, S = (size_t)steps;
    // P0 and P_out have stages of their own: the kernel reads the one before it writes the other, whether or not the caller's alias
    return run_staged(h, {staged_in(IN_PLANT, EST_P, P0, n * n), staged_out(IN_PLANT, PCOV_SDIAG, sdiag, (S + 1) * n),
                          staged_out(IN_PLANT, PCOV_UDIAG, udiag, S * m), staged_out(IN_PLANT, PCOV_SIGMA, sigma, (S + 1) * n * n),
                          staged_out(IN_PLANT, PCOV_POUT, P_out, n * n), staged_out(IN_PLANT, PLANT_NONFINITE, first_nonfinite, 1)},
                      [&](ilqr_handle* s, size_t, const Staged* a) {
                          return plancov_launch(s, steps, feedback, q, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].d(), a[5].i()); });
}

// ---- a linear sensor y = H x + v with ny outputs (ilqr_device_sensor.hpp)
// everything that can be refused without touching the GPU; what needs no handle comes first. H_host: null where H is a device array;
// r: null where the call takes none (the measurement)
static int sensor_check(const ilqr_handle* h, int32_t ny, int32_t per_instance_H, const double* H_host, const double* r, const double* sigma_y,
                        const char* who) {
    const std::string me(who);
    if (ny < 1 || ny > ilqr::SENSOR_MAX_NY) return fail(ILQR_ERR_INVALID, me + ": ny must lie in 1 .. 64");
    if (per_instance_H != 0 && per_instance_H != 1) return fail(ILQR_ERR_INVALID, me + ": per_instance_H must be 0 or 1");
    for (int j = 0; r && j < ny; ++j)
        if (!(r[j] > 0.0) || !std::isfinite(r[j])) return fail(ILQR_ERR_INVALID, me + ": r must be finite and > 0");
    ILQR_TRY(sigma_check(sigma_y, ny, me, "sigma_y"));
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (h->L.nx > ilqr::PLANT_MAX_NX) return fail(ILQR_ERR_INVALID, me + ": more than 64 state components");
    const size_t count = (per_instance_H ? (size_t)h->B : 1) * (size_t)ny * (size_t)h->L.nx;
    for (size_t e = 0; H_host && e < count; ++e)
        if (!std::isfinite(H_host[e])) return fail(ILQR_ERR_INVALID, me + ": a non-finite entry of H");
    return ILQR_OK;
}

// a host vector of ny doubles (r, sigma_y) of a device form, on its way into its stage without a copy the stream could read late
static int sensor_vector_upload(ilqr_handle* h, ilqr_handle::Stage& st, const double* v, int32_t ny) {
    ILQR_TRY(grow(h, st, (size_t)ilqr::SENSOR_MAX_NY * 8));
    SensorVector a = {};
    for (int j = 0; j < ny; ++j) a.v[j] = v[j];
    hipLaunchKernelGGL(sensor_vector_kernel, dim3(1), dim3(ilqr::SENSOR_MAX_NY), 0, h->stream, a, (int)ny, (double*)st.p);
    if (hipGetLastError() != hipSuccess) return fail(ILQR_ERR_HIP, "sensor vector launch failed");
    return ILQR_OK;
}

// every pointer a device pointer on h's device (yhat, innovation, nis, first_bad: or null)
static int sensor_update_launch(ilqr_handle* h, int32_t ny, int32_t per_instance_H, const double* H, const double* r, const double* y,
                                const double* yhat, double* xhat, double* P, double* innovation, double* nis, int32_t* first_bad) {
    if (!h->vt->launch_sensor_update) return fail(ILQR_ERR_MODEL, "this model module has no linear sensor kernel");
    ilqr::SensorArgs a = {};
    a.B = h->B; a.ny = ny; a.h_stride = per_instance_H ? (long long)ny * h->L.nx : 0; a.H = H; a.r = r; a.y = y; a.yhat = yhat; a.xhat = xhat; a.P = P;
    a.innovation = innovation; a.nis = nis; a.first_bad = first_bad;
    if (h->vt->launch_sensor_update(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "linear sensor update launch failed");
    return ILQR_OK;
}

// H [ny][nx], sigma_y (or null), x, y: device pointers on h's device
static int measure_linear_launch(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, int32_t ny, const double* H,
                                 const double* sigma_y, const double* x, double* y) {
    if (!h->vt->launch_plant_measure_linear) return fail(ILQR_ERR_MODEL, "this model module has no linear sensor kernel");
    ilqr::SensorArgs a = {};
    a.B = h->B; a.ny = ny; a.H = H; a.sigma = sigma_y; a.step = step; a.seed = seed; a.b0 = first_instance; a.x = x; a.y_out = y;
    if (h->vt->launch_plant_measure_linear(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "linear measurement launch failed");
    return ILQR_OK;
}

int ilqr_estimate_update_linear_device(ilqr_handle* h, int32_t ny, int32_t per_instance_H, const double* H, const double* r, const double* y,
                                       const double* yhat, double* xhat, double* P, double* innovation, double* nis, int32_t* first_bad) {
    if (!H || !r || !y || !xhat || !P) return fail(ILQR_ERR_INVALID, "ilqr_estimate_update_linear_device: null H, r, y, xhat or P");
    ILQR_TRY(sensor_check(h, ny, per_instance_H, nullptr, r, nullptr, "ilqr_estimate_update_linear_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_estimate_update_linear");
    HIP_TRY(hipSetDevice(h->device));
    ILQR_TRY(sensor_vector_upload(h, h->plant[SENS_R], r, ny));
    return sensor_update_launch(h, ny, per_instance_H, H, (const double*)h->plant[SENS_R].p, y, yhat, xhat, P, innovation, nis, first_bad);
}

int ilqr_estimate_update_linear(ilqr_handle* h, int32_t ny, int32_t per_instance_H, const double* H, const double* r, const double* y,
                                const double* yhat, double* xhat, double* P, double* innovation, double* nis, int32_t* first_bad) {
    if (!H || !r || !y || !xhat || !P) return fail(ILQR_ERR_INVALID, "ilqr_estimate_update_linear: null H, r, y, xhat or P");
    ILQR_TRY(sensor_check(h, ny, per_instance_H, H, r, nullptr, "ilqr_estimate_update_linear"));
    const size_t n = (size_t)h->L.nx, m = (size_t)ny;
    // the estimate and its covariance go in and come back
    return run_staged(h, {per_instance_H ? staged_in(IN_PLANT, SENS_H, H, m * n) : staged_shared(IN_PLANT, SENS_H, H, m * n), staged_shared(IN_PLANT, SENS_R, r, m),
                          staged_in(IN_PLANT, EST_Y, y, m), staged_in(IN_PLANT, SENS_YHAT, yhat, m), staged_io(IN_PLANT, PLANT_XC, xhat, n),
                          staged_io(IN_PLANT, EST_P, P, n * n), staged_out(IN_PLANT, EST_INNOVATION, innovation, m), staged_out(IN_PLANT, EST_NIS, nis, 1),
                          staged_out(IN_PLANT, EST_FIRST_BAD, first_bad, 1)},
                      [&](ilqr_handle* s, size_t, const Staged* a) {
                          return sensor_update_launch(s, ny, per_instance_H, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].d(), a[5].d(), a[6].d(), a[7].d(), a[8].i()); });
}

int ilqr_plant_measure_linear_device(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, int32_t ny, const double* H,
                                     const double* sigma_y, const double* x, double* y) {
    if (!H || !x || !y) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_linear_device: null H, x or y");
    if (ny < 1 || ny > ilqr::SENSOR_MAX_NY) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_linear_device: ny must lie in 1 .. 64");
    ILQR_TRY(sigma_check(sigma_y, ny, "ilqr_plant_measure_linear_device", "sigma_y"));
    ILQR_TRY(measure_check(h, first_instance, step, nullptr, "ilqr_plant_measure_linear_device"));
    ILQR_TRY(sensor_check(h, ny, 0, nullptr, nullptr, sigma_y, "ilqr_plant_measure_linear_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_plant_measure_linear");
    HIP_TRY(hipSetDevice(h->device));
    if (sigma_y) ILQR_TRY(sensor_vector_upload(h, h->plant[SENS_SIGMA], sigma_y, ny));
    return measure_linear_launch(h, seed, first_instance, step, ny, H, sigma_y ? (const double*)h->plant[SENS_SIGMA].p : nullptr, x, y);
}

int ilqr_plant_measure_linear(ilqr_handle* h, uint64_t seed, int64_t first_instance, int32_t step, int32_t ny, const double* H,
                              const double* sigma_y, const double* x, double* y) {
    if (!H || !x || !y) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_linear: null H, x or y");
    if (ny < 1 || ny > ilqr::SENSOR_MAX_NY) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_linear: ny must lie in 1 .. 64");
    ILQR_TRY(sigma_check(sigma_y, ny, "ilqr_plant_measure_linear", "sigma_y"));
    ILQR_TRY(measure_check(h, first_instance, step, nullptr, "ilqr_plant_measure_linear"));
    ILQR_TRY(sensor_check(h, ny, 0, H, nullptr, sigma_y, "ilqr_plant_measure_linear"));
    const size_t n = (size_t)h->L.nx, m = (size_t)ny;
    return run_staged(h, {staged_shared(IN_PLANT, SENS_H, H, m * n), staged_shared(IN_PLANT, SENS_SIGMA, sigma_y, m), staged_in(IN_PLANT, PLANT_X, x, n),
                          staged_out(IN_PLANT, PLANT_Y, y, m)},
                      [&](ilqr_handle* s, size_t lo, const Staged* a) {
                          return measure_linear_launch(s, seed, first_instance + (int64_t)lo, step, ny, a[0].d(), a[1].d(), a[2].d(), a[3].d()); });
}

// ---- a nonlinear sensor y = h(x, s) + v compiled as a module of its own (ilqr_device_sensor_nl.hpp, ilqr_compile_sensor)
// everything that can be refused without touching the GPU; what needs no handle comes first. s_host: s is a host array (its entries
// are looked at); r, sigma_y: null where the call takes none; iterations: 1 where the call takes none
static int nl_sensor_args_check(const char* sensor, int32_t per_instance_s, const double* s, int32_t iterations, const double* r,
                                const double* sigma_y, const ilqr_sensor_vtable** out, const char* who) {
    const std::string me(who);
    if (!sensor) return fail(ILQR_ERR_INVALID, me + ": null sensor name");
    const ilqr_sensor_vtable* sv = find_sensor(sensor);
    if (!sv) return fail(ILQR_ERR_INVALID, me + ": unknown sensor '" + sensor + "' (ilqr_compile_sensor / ilqr_load_sensor_library register one)");
    if (per_instance_s != 0 && per_instance_s != 1) return fail(ILQR_ERR_INVALID, me + ": per_instance_s must be 0 or 1");
    if (iterations < 1 || iterations > ilqr::SENSOR_NL_MAX_ITERATIONS) return fail(ILQR_ERR_INVALID, me + ": iterations must lie in 1 .. 8");
    if (sv->ns > 0 && !s) return fail(ILQR_ERR_INVALID, me + ": null s for a sensor with parameters");
    for (int j = 0; r && j < sv->ny; ++j)
        if (!(r[j] > 0.0) || !std::isfinite(r[j])) return fail(ILQR_ERR_INVALID, me + ": r must be finite and > 0");
    ILQR_TRY(sigma_check(sigma_y, sv->ny, me, "sigma_y"));
    *out = sv;
    return ILQR_OK;
}
// what needs the handle: its nx, and with it the extent of a host s
static int nl_sensor_handle_check(const ilqr_handle* h, const ilqr_sensor_vtable* sv, int32_t per_instance_s, const double* s, bool s_host,
                                  const char* who) {
    const std::string me(who);
    if (!h) return fail(ILQR_ERR_INVALID, me + ": null handle");
    if (sv->nx != h->L.nx) return fail(ILQR_ERR_INVALID, me + ": the sensor's nx is not the handle's");
    if (h->L.nx > ilqr::PLANT_MAX_NX) return fail(ILQR_ERR_INVALID, me + ": more than 64 state components");
    const size_t count = (per_instance_s ? (size_t)h->B : 1) * (size_t)sv->ns;
    for (size_t e = 0; s && s_host && e < count; ++e)
        if (!std::isfinite(s[e])) return fail(ILQR_ERR_INVALID, me + ": a non-finite entry of s");
    return ILQR_OK;
}
static int nl_sensor_check(const ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, bool s_host, int32_t iterations,
                           const double* r, const double* sigma_y, const ilqr_sensor_vtable** out, const char* who) {
    ILQR_TRY(nl_sensor_args_check(sensor, per_instance_s, s, iterations, r, sigma_y, out, who));
    return nl_sensor_handle_check(h, *out, per_instance_s, s, s_host, who);
}

// the sensor parameters of a host form: one row per instance, or the one copy the batch reads
static Staged staged_s(const ilqr_sensor_vtable* sv, int32_t per_instance_s, const double* s) {
    return per_instance_s ? staged_in(IN_PLANT, SENS_S, s, (size_t)sv->ns) : staged_shared(IN_PLANT, SENS_S, s, (size_t)sv->ns);
}

// every pointer a device pointer on h's device (s: or null where ns == 0; x_prior: or null)
static int nl_linearise_launch(ilqr_handle* h, const ilqr_sensor_vtable* sv, int32_t per_instance_s, const double* s, const double* x_lin,
                               const double* x_prior, double* H, double* yhat) {
    ilqr::SensorNlArgs a = {};
    a.B = h->B; a.s_stride = per_instance_s ? sv->ns : 0; a.s = s; a.x = x_lin; a.x_prior = x_prior; a.H = H; a.yhat = yhat;
    if (sv->launch_linearise(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "sensor linearisation launch failed");
    return ILQR_OK;
}

// sigma_y (or null), x, y: device pointers on h's device
static int nl_measure_launch(ilqr_handle* h, const ilqr_sensor_vtable* sv, int32_t per_instance_s, const double* s, uint64_t seed,
                             int64_t first_instance, int32_t step, const double* sigma_y, const double* x, double* y) {
    ilqr::SensorNlArgs a = {};
    a.B = h->B; a.s_stride = per_instance_s ? sv->ns : 0; a.s = s; a.x = x; a.y_out = y; a.sigma = sigma_y; a.step = step; a.seed = seed;
    a.b0 = first_instance;
    if (sv->launch_measure(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "sensor measurement launch failed");
    return ILQR_OK;
}

// The update of `iterations` iterations: every pointer a device pointer on h's device. Hb [B][ny][nx] and yh [B][ny] are the buffers
// the linearisation writes and the existing update reads; x0 [B][nx] and P0 [B][nx][nx] keep the prior of the iterated filter (not
// touched where iterations == 1). Iteration i >= 1 linearises at the estimate iteration i−1 left BEFORE the prior is restored over it.
static int nl_update_launch(ilqr_handle* h, const ilqr_sensor_vtable* sv, int32_t per_instance_s, const double* s, int32_t iterations,
                            const double* r, const double* y, double* xhat, double* P, double* innovation, double* nis, int32_t* first_bad,
                            double* Hb, double* yh, double* x0, double* P0) {
    const size_t xb = (size_t)h->B * (size_t)h->L.nx * 8, pb = xb * (size_t)h->L.nx;
    if (iterations > 1) {
        HIP_TRY(hipMemcpyAsync(x0, xhat, xb, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(P0, P, pb, hipMemcpyDeviceToDevice, h->stream));
    }
    for (int32_t i = 0; i < iterations; ++i) {
        ILQR_TRY(nl_linearise_launch(h, sv, per_instance_s, s, xhat, i ? x0 : nullptr, Hb, yh));
        if (i) {
            HIP_TRY(hipMemcpyAsync(xhat, x0, xb, hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(P, P0, pb, hipMemcpyDeviceToDevice, h->stream));
        }
        ILQR_TRY(sensor_update_launch(h, sv->ny, 1, Hb, r, y, yh, xhat, P, innovation, nis, first_bad));
    }
    return ILQR_OK;
}

int ilqr_sensor_linearise_device(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, const double* x_lin,
                                 const double* x_prior, double* H_out, double* yhat_out) {
    if (!x_lin || !H_out || !yhat_out) return fail(ILQR_ERR_INVALID, "ilqr_sensor_linearise_device: null x_lin, H_out or yhat_out");
    const ilqr_sensor_vtable* sv = nullptr;
    ILQR_TRY(nl_sensor_check(h, sensor, per_instance_s, s, false, 1, nullptr, nullptr, &sv, "ilqr_sensor_linearise_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_sensor_linearise");
    HIP_TRY(hipSetDevice(h->device));
    return nl_linearise_launch(h, sv, per_instance_s, s, x_lin, x_prior, H_out, yhat_out);
}

int ilqr_sensor_linearise(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, const double* x_lin, const double* x_prior,
                          double* H_out, double* yhat_out) {
    if (!x_lin || !H_out || !yhat_out) return fail(ILQR_ERR_INVALID, "ilqr_sensor_linearise: null x_lin, H_out or yhat_out");
    const ilqr_sensor_vtable* sv = nullptr;
    ILQR_TRY(nl_sensor_check(h, sensor, per_instance_s, s, true, 1, nullptr, nullptr, &sv, "ilqr_sensor_linearise"));
    const size_t n = (size_t)h->L.nx, m = (size_t)sv->ny;
    return run_staged(h, {staged_s(sv, per_instance_s, s), staged_in(IN_PLANT, SENS_XLIN, x_lin, n), staged_in(IN_PLANT, SENS_XPRIOR, x_prior, n),
                          staged_out(IN_PLANT, SENS_H, H_out, m * n), staged_out(IN_PLANT, SENS_YHAT, yhat_out, m)},
                      [&](ilqr_handle* sh, size_t, const Staged* a) {
                          return nl_linearise_launch(sh, sv, per_instance_s, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].d()); });
}

int ilqr_plant_measure_sensor_device(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, uint64_t seed,
                                     int64_t first_instance, int32_t step, const double* sigma_y, const double* x, double* y) {
    if (!x || !y) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_sensor_device: null x or y");
    const ilqr_sensor_vtable* sv = nullptr;
    ILQR_TRY(nl_sensor_args_check(sensor, per_instance_s, s, 1, nullptr, sigma_y, &sv, "ilqr_plant_measure_sensor_device"));
    ILQR_TRY(measure_check(h, first_instance, step, nullptr, "ilqr_plant_measure_sensor_device"));
    ILQR_TRY(nl_sensor_handle_check(h, sv, per_instance_s, s, false, "ilqr_plant_measure_sensor_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_plant_measure_sensor");
    HIP_TRY(hipSetDevice(h->device));
    if (sigma_y) ILQR_TRY(sensor_vector_upload(h, h->plant[SENS_SIGMA], sigma_y, sv->ny));
    return nl_measure_launch(h, sv, per_instance_s, s, seed, first_instance, step, sigma_y ? (const double*)h->plant[SENS_SIGMA].p : nullptr, x, y);
}

int ilqr_plant_measure_sensor(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, uint64_t seed, int64_t first_instance,
                              int32_t step, const double* sigma_y, const double* x, double* y) {
    if (!x || !y) return fail(ILQR_ERR_INVALID, "ilqr_plant_measure_sensor: null x or y");
    const ilqr_sensor_vtable* sv = nullptr;
    ILQR_TRY(nl_sensor_args_check(sensor, per_instance_s, s, 1, nullptr, sigma_y, &sv, "ilqr_plant_measure_sensor"));
    ILQR_TRY(measure_check(h, first_instance, step, nullptr, "ilqr_plant_measure_sensor"));
    ILQR_TRY(nl_sensor_handle_check(h, sv, per_instance_s, s, true, "ilqr_plant_measure_sensor"));
    const size_t n = (size_t)h->L.nx, m = (size_t)sv->ny;
    return run_staged(h, {staged_s(sv, per_instance_s, s), staged_shared(IN_PLANT, SENS_SIGMA, sigma_y, m), staged_in(IN_PLANT, PLANT_X, x, n),
                          staged_out(IN_PLANT, PLANT_Y, y, m)},
                      [&](ilqr_handle* sh, size_t lo, const Staged* a) {
                          return nl_measure_launch(sh, sv, per_instance_s, a[0].d(), seed, first_instance + (int64_t)lo, step, a[1].d(), a[2].d(), a[3].d()); });
}

int ilqr_estimate_update_sensor_device(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, int32_t iterations,
                                       const double* r, const double* y, double* xhat, double* P, double* innovation, double* nis,
                                       int32_t* first_bad) {
    if (!r || !y || !xhat || !P) return fail(ILQR_ERR_INVALID, "ilqr_estimate_update_sensor_device: null r, y, xhat or P");
    const ilqr_sensor_vtable* sv = nullptr;
    ILQR_TRY(nl_sensor_check(h, sensor, per_instance_s, s, false, iterations, r, nullptr, &sv, "ilqr_estimate_update_sensor_device"));
    if (SHARDED(h)) return refuse_sharded("ilqr_estimate_update_sensor");
    HIP_TRY(hipSetDevice(h->device));
    // the handle's buffers, reused by later calls: they grow (and then wait for the stream) only when a call needs more than any before it
    const size_t B = (size_t)h->B, n = (size_t)h->L.nx, m = (size_t)sv->ny;
    ILQR_TRY(grow(h, h->plant[SENS_H], B * m * n * 8));
    ILQR_TRY(grow(h, h->plant[SENS_YHAT], B * m * 8));
    if (iterations > 1) {
        ILQR_TRY(grow(h, h->plant[SENS_X0], B * n * 8));
        ILQR_TRY(grow(h, h->plant[SENS_P0], B * n * n * 8));
    }
    ILQR_TRY(sensor_vector_upload(h, h->plant[SENS_R], r, sv->ny));
    return nl_update_launch(h, sv, per_instance_s, s, iterations, (const double*)h->plant[SENS_R].p, y, xhat, P, innovation, nis, first_bad,
                            (double*)h->plant[SENS_H].p, (double*)h->plant[SENS_YHAT].p, (double*)h->plant[SENS_X0].p, (double*)h->plant[SENS_P0].p);
}

int ilqr_estimate_update_sensor(ilqr_handle* h, const char* sensor, int32_t per_instance_s, const double* s, int32_t iterations, const double* r,
                                const double* y, double* xhat, double* P, double* innovation, double* nis, int32_t* first_bad) {
    if (!r || !y || !xhat || !P) return fail(ILQR_ERR_INVALID, "ilqr_estimate_update_sensor: null r, y, xhat or P");
    const ilqr_sensor_vtable* sv = nullptr;
    ILQR_TRY(nl_sensor_check(h, sensor, per_instance_s, s, true, iterations, r, nullptr, &sv, "ilqr_estimate_update_sensor"));
    const size_t n = (size_t)h->L.nx, m = (size_t)sv->ny;
    const bool it = iterations > 1;
    // the estimate and its covariance go in and come back; H, ŷ and the prior stay on the device
    return run_staged(h, {staged_s(sv, per_instance_s, s), staged_shared(IN_PLANT, SENS_R, r, m), staged_in(IN_PLANT, EST_Y, y, m),
                          staged_io(IN_PLANT, PLANT_XC, xhat, n), staged_io(IN_PLANT, EST_P, P, n * n), staged_out(IN_PLANT, EST_INNOVATION, innovation, m),
                          staged_out(IN_PLANT, EST_NIS, nis, 1), staged_out(IN_PLANT, EST_FIRST_BAD, first_bad, 1),
                          staged_device(IN_PLANT, SENS_H, true, m * n), staged_device(IN_PLANT, SENS_YHAT, true, m),
                          staged_device(IN_PLANT, SENS_X0, it, n), staged_device(IN_PLANT, SENS_P0, it, n * n)},
                      [&](ilqr_handle* sh, size_t, const Staged* a) {
                          return nl_update_launch(sh, sv, per_instance_s, a[0].d(), iterations, a[1].d(), a[2].d(), a[3].d(), a[4].d(), a[5].d(), a[6].d(),
                                                  a[7].i(), a[8].d(), a[9].d(), a[10].d(), a[11].d()); });
}

// ---- the closed MPC loop, enqueued once: per period plant step, score, horizon shift, dual shift, solve, log row
static_assert(ILQR_MPC_LOG_W == ilqr::MPC_LOG_W, "the log row of the header is the kernel's");
// One run of the loop as an entry point hands it over: the descriptor, the seam (io), the filter (est: the extended Kalman filter, or
// sens: the linear sensor in its place, or nls: the compiled nonlinear one, with nlv its module once the check has found it), every
// input and output array of the batch, and the entry point's name. What an entry point does not offer stays null.
struct MpcRun {
    const ilqr_mpc_desc* d; const ilqr_plant_io* io; const ilqr_estimator* est; const ilqr_sensor* sens; const ilqr_nl_sensor* nls;
    const ilqr_sensor_vtable* nlv;
    const double *x0, *xhat0, *w_plant, *w_preview;
    double *Pcov, *x_cl, *u_cl, *log, *cl_cost, *cl_violation, *y_cl, *xhat_cl, *pdiag_cl, *nis_cl;
    int32_t *first_nonfinite, *saturated;
    const char* who;
};
// The seam between plant and controller is in use: limits, measurement noise, a delay, a filter, or one of the two outputs that report
// on it. Otherwise the loop hands the shift the plant state itself: no launch, no buffer and no argument of it differs from ilqr_mpc_run's.
static bool mpc_measured(const MpcRun& r) {
    return (r.io && (r.io->u_min || r.io->u_max || r.io->sigma_y || r.io->delay)) || r.y_cl || r.saturated || r.est || r.sens || r.nls;
}
// everything its constituents refuse for these arguments, before any launch
// measured: the run goes through the measurement slot (mpc_measured)
static int mpc_check(const ilqr_handle* h, const MpcRun& r, bool measured) {
    const ilqr_mpc_desc* d = r.d; const ilqr_plant_io* io = r.io; const ilqr_estimator* est = r.est; const ilqr_sensor* sens = r.sens;
    const char* who = r.who;
    const std::string me(who);
    if (!d) return fail(ILQR_ERR_INVALID, me + ": null descriptor");
    if (sens) {                                    // the linear sensor in the estimator's place; what needs no handle, as its calls order it
        if (!r.Pcov) return fail(ILQR_ERR_INVALID, me + ": a sensor with a null P");
        if (io && io->sigma_y) return fail(ILQR_ERR_INVALID, me + ": io->sigma_y together with a sensor: the sensor's own sigma_y [ny] replaces it");
        if (!sens->H || !sens->r) return fail(ILQR_ERR_INVALID, me + ": null H or r");
        if (sens->ny < 1 || sens->ny > ilqr::SENSOR_MAX_NY) return fail(ILQR_ERR_INVALID, me + ": ny must lie in 1 .. 64");
        ILQR_TRY(variance_check(nullptr, sens->q, nullptr, 1, me));
        for (int j = 0; j < sens->ny; ++j)
            if (!(sens->r[j] > 0.0) || !std::isfinite(sens->r[j])) return fail(ILQR_ERR_INVALID, me + ": r must be finite and > 0");
        ILQR_TRY(sigma_check(sens->sigma_y, sens->ny, me, "sigma_y"));
    }
    const ilqr_nl_sensor* nls = r.nls;
    if (nls) {                                     // the compiled sensor in the estimator's place; what needs no handle, as its calls order it
        if (!r.Pcov) return fail(ILQR_ERR_INVALID, me + ": a sensor with a null P");
        if (io && io->sigma_y) return fail(ILQR_ERR_INVALID, me + ": io->sigma_y together with a sensor: the sensor's own sigma_y [ny] replaces it");
        if (!nls->r) return fail(ILQR_ERR_INVALID, me + ": null r");
        const ilqr_sensor_vtable* sv = nullptr;
        ILQR_TRY(nl_sensor_args_check(nls->sensor, nls->ns_per_instance, nls->s, nls->iterations, nls->r, nls->sigma_y, &sv, who));
        ILQR_TRY(variance_check(nullptr, nls->q, nullptr, 1, me));
    }
    if (!est && !sens && !nls && (r.xhat0 || r.Pcov || r.xhat_cl || r.pdiag_cl || r.nis_cl)) return fail(ILQR_ERR_INVALID, me + ": xhat0, P, xhat_cl, pdiag_cl or nis_cl without an estimator");
    if (est && !r.Pcov) return fail(ILQR_ERR_INVALID, me + ": an estimator with a null P");
    if (est) {                                     // what needs no handle, as the two estimator calls order it
        if (!est->r) return fail(ILQR_ERR_INVALID, me + ": null r");
        ILQR_TRY(variance_check(est->measured, est->q, est->r, 1, me));
    }
    if (d->periods < 1) return fail(ILQR_ERR_INVALID, me + ": periods must be >= 1");
    if (r.cl_violation && !r.cl_cost) return fail(ILQR_ERR_INVALID, me + ": cl_violation without cl_cost: the two scores come from one launch");
    if (io && io->delay != 0 && io->delay != 1) return fail(ILQR_ERR_INVALID, me + ": delay must be 0 or 1");
    const int64_t run_steps = (int64_t)d->periods * (int64_t)(d->steps > 0 ? d->steps : 0);
    // the last measurement: of the state after the run's last plant step (delay 0), before its last period (delay 1)
    const int64_t last_measured = io && io->delay ? run_steps - (d->steps > 0 ? d->steps : 0) : run_steps;
    if (measured) {                                // what needs no handle, as plant_check orders it
        if (last_measured >= ilqr::PLANT_MAX_STEPS) return fail(ILQR_ERR_INVALID, me + ": the measurement step must lie in 0 .. 2^20 - 1 (the noise key's bit fields)");
        ILQR_TRY(sigma_check(io ? io->sigma_y : nullptr, 1, me, "sigma_y"));
    }
    ILQR_TRY(plant_check(h, d->steps, d->plant_feedback, d->first_instance, 0, run_steps, d->sigma_x, io ? io->u_min : nullptr,
                         io ? io->u_max : nullptr, r.w_plant, who));
    if (measured) ILQR_TRY(measure_check(h, d->first_instance, last_measured, io ? io->sigma_y : nullptr, who));
    if (r.w_preview && h->vt->nw - h->n_sel <= 0) return fail(ILQR_ERR_INVALID, me + ": w_preview given, but this model has no parameters (num_parameter == 0)");
    ILQR_TRY(shift_check(h, d->steps, d->shift_tail, d->shift_feedback, r.w_preview, who));
    if (d->warm) {
        if (!h->constrained) return fail(ILQR_ERR_INVALID, me + ": warm on a handle created unconstrained: it has no duals to keep");
        ILQR_TRY(duals_check(h, d->steps, d->duals_tail, d->duals_penalty, who));
    }
    if (est) ILQR_TRY(variance_check(est->measured, est->q, est->r, h->L.nx, me));
    if (sens) {
        ILQR_TRY(variance_check(nullptr, sens->q, nullptr, h->L.nx, me));
        ILQR_TRY(sensor_check(h, sens->ny, 0, sens->H, sens->r, sens->sigma_y, who));
    }
    if (nls) {
        const ilqr_sensor_vtable* sv = nullptr;
        ILQR_TRY(variance_check(nullptr, nls->q, nullptr, h->L.nx, me));
        ILQR_TRY(nl_sensor_check(h, nls->sensor, nls->ns_per_instance, nls->s, true, nls->iterations, nls->r, nls->sigma_y, &sv, who));
    }
    return ILQR_OK;
}

// the arrays of a run (mpc_arrays) by name
enum { M_X, M_W, M_PREVIEW, M_X_CL, M_U_CL, M_LOG, M_NONFINITE, M_COST, M_VIOL, M_Y_CL, M_SATURATED, M_XC, M_P, M_XHAT_CL, M_PDIAG_CL, M_NIS_CL, M_SENS_H,
       M_SENS_R, M_SENS_SIGMA, M_YM, M_NIS, M_W_STAGE, M_RESIDENT, M_NL_S, M_NL_H, M_NL_YHAT, M_NL_X0, M_NL_P0 };

// Every buffer of the run exists before its first launch — the plant state also without an x0, the closed-loop trajectory the score
// reads even when the caller does not ask for it, the controller's state of a measured run, the period's measurement and nis of a
// filter, what the shift would allocate in its first call and the resident inputs — so that nothing between the first plant launch
// and the synchronise at the end waits for the device. The sensor's H, r and sigma_y are copied once, before the first launch; so are
// the compiled sensor's s, r and sigma_y, whose Jacobians, ŷ and (iterated) prior get their buffers here too.
static std::vector<Staged> mpc_arrays(const ilqr_handle* h, const MpcRun& r, bool measured) {
    const bool filt = r.est || r.sens || r.nls, score = r.cl_cost != nullptr, iterated = r.nls && r.nls->iterations > 1;
    const size_t ym_n = r.sens ? (size_t)r.sens->ny : (r.nls ? (size_t)r.nlv->ny : (size_t)h->L.nx);       // the numbers of one measurement
    const size_t nl_ns = r.nls ? (size_t)r.nlv->ns : 0;
    const size_t P = (size_t)r.d->periods, R = P * (size_t)r.d->steps, n = (size_t)h->L.nx, m = (size_t)h->L.nu, nwu = (size_t)(h->L.nw - h->n_sel);
    return {staged_in(IN_PLANT, PLANT_X, r.x0, n).kept(true), staged_in(IN_PLANT, PLANT_W, r.w_plant, R * nwu), staged_in(IN_PLANT, PLANT_W_PREVIEW, r.w_preview, R * nwu),
            staged_out(IN_PLANT, PLANT_X_OUT, r.x_cl, (R + 1) * n).kept(score), staged_out(IN_PLANT, PLANT_U_OUT, r.u_cl, R * m).kept(score),
            staged_out(IN_PLANT, PLANT_LOG, r.log, P * ILQR_MPC_LOG_W), staged_out(IN_PLANT, PLANT_NONFINITE, r.first_nonfinite, 1),
            staged_out(IN_PLANT, PLANT_COST, r.cl_cost, R), staged_out(IN_PLANT, PLANT_VIOL, r.cl_violation, R),
            staged_out(IN_PLANT, PLANT_Y, r.y_cl, P * ym_n), staged_out(IN_PLANT, PLANT_SATURATED, r.saturated, 1),
            staged_in(IN_PLANT, PLANT_XC, r.xhat0, n).kept(measured), staged_io(IN_PLANT, EST_P, r.Pcov, n * n),      // P0 in, the last covariance back
            staged_out(IN_PLANT, EST_XHAT_CL, r.xhat_cl, P * n), staged_out(IN_PLANT, EST_PDIAG_CL, r.pdiag_cl, P * n), staged_out(IN_PLANT, EST_NIS_CL, r.nis_cl, P),
            staged_shared(IN_PLANT, SENS_H, r.sens ? r.sens->H : nullptr, ym_n * n), staged_shared(IN_PLANT, SENS_R, r.sens ? r.sens->r : (r.nls ? r.nls->r : nullptr), ym_n),
            staged_shared(IN_PLANT, SENS_SIGMA, r.sens ? r.sens->sigma_y : (r.nls ? r.nls->sigma_y : nullptr), ym_n),
            staged_device(IN_PLANT, EST_Y, filt, ym_n), staged_device(IN_PLANT, EST_NIS, filt, 1),
            staged_device(IN_SHIFT, SHIFT_W_STAGE, h->L.nw > 0, (size_t)h->L.T * (size_t)h->L.nw), staged_device(IN_RESIDENT, 0, true, n),
            r.nls && r.nls->ns_per_instance ? staged_in(IN_PLANT, SENS_S, r.nls->s, nl_ns) : staged_shared(IN_PLANT, SENS_S, r.nls ? r.nls->s : nullptr, nl_ns),
            staged_device(IN_PLANT, SENS_H, r.nls != nullptr && !r.sens, ym_n * n), staged_device(IN_PLANT, SENS_YHAT, r.nls != nullptr, ym_n),
            staged_device(IN_PLANT, SENS_X0, iterated, n), staged_device(IN_PLANT, SENS_P0, iterated, n * n)};
}

// A run on one handle while it is enqueued: its arrays on the device, the plant state xp, the controller's view of it xc (what the shift
// is handed; with a filter the estimate x̂), where the measurement lands (ym: with a filter its own buffer, else xc), the period's nis,
// the closed-loop trajectory, the seam's host vectors, and which stages the periods go through.
struct MpcState {
    const Staged* a;
    double *xp, *xc, *ym, *d_nis, *d_x_cl, *d_u_cl;
    const double *u_min, *u_max, *sigma_y;
    bool measured, filt, delayed, score;
    long long rows;                            // plant steps of the run: the rows per instance of its arrays
    size_t ym_n;
};

// everything before the first period
static int mpc_begin(ilqr_handle* h, const MpcRun& r, MpcState& st) {
    const Staged* a = st.a;
    st.filt = r.est || r.sens || r.nls; st.delayed = r.io && r.io->delay == 1; st.score = r.cl_cost != nullptr;
    st.u_min = r.io ? r.io->u_min : nullptr; st.u_max = r.io ? r.io->u_max : nullptr; st.sigma_y = r.io ? r.io->sigma_y : nullptr;
    st.rows = (long long)r.d->periods * r.d->steps; st.ym_n = r.sens ? (size_t)r.sens->ny : (r.nls ? (size_t)r.nlv->ny : (size_t)h->L.nx);
    st.xp = a[M_X].d();
    st.xc = st.measured ? a[M_XC].d() : st.xp;
    st.d_x_cl = a[M_X_CL].d(); st.d_u_cl = a[M_U_CL].d();
    st.ym = st.filt ? a[M_YM].d() : st.xc;
    st.d_nis = a[M_NIS].d();
    const size_t row = (size_t)h->L.nx * 8;
    if (!r.x0) HIP_TRY(hipMemcpy2DAsync(st.xp, row, h->ws + h->L.xb, (size_t)h->L.stride * 8, row, (size_t)h->B, hipMemcpyDeviceToDevice, h->stream));     // x̄_0
    if (a[M_NONFINITE].p) HIP_TRY(hipMemsetAsync(a[M_NONFINITE].p, 0xff, a[M_NONFINITE].bytes, h->stream));       // -1: the plant kernel keeps the first mark
    if (a[M_SATURATED].p) HIP_TRY(hipMemsetAsync(a[M_SATURATED].p, 0, a[M_SATURATED].bytes, h->stream));          // the plant kernel adds to it
    if (st.filt && !r.xhat0) HIP_TRY(hipMemcpyAsync(st.xc, st.xp, a[M_XC].bytes, hipMemcpyDeviceToDevice, h->stream));           // x̂_0 = the first plant state
    return ILQR_OK;
}

// the measurement at plant step `step`, the update with it and the estimate's move to the end of the period under the plan in
// flight: the selection of state components, the linear sensor, or the compiled nonlinear one
static int mpc_measure(ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t step) {
    const ilqr_mpc_desc* d = r.d;
    if (r.nls) return nl_measure_launch(h, r.nlv, r.nls->ns_per_instance, st.a[M_NL_S].d(), d->seed, d->first_instance, step, st.a[M_SENS_SIGMA].d(), st.xp, st.ym);
    return r.sens ? measure_linear_launch(h, d->seed, d->first_instance, step, r.sens->ny, st.a[M_SENS_H].d(), st.a[M_SENS_SIGMA].d(), st.xp, st.ym)
                  : measure_launch(h, d->seed, d->first_instance, step, st.sigma_y, st.xp, st.ym);
}
static int mpc_update(ilqr_handle* h, const MpcRun& r, const MpcState& st) {
    if (r.nls) return nl_update_launch(h, r.nlv, r.nls->ns_per_instance, st.a[M_NL_S].d(), r.nls->iterations, st.a[M_SENS_R].d(), st.ym, st.xc, st.a[M_P].d(),
                                       nullptr, st.d_nis, nullptr, st.a[M_NL_H].d(), st.a[M_NL_YHAT].d(), st.a[M_NL_X0].d(), st.a[M_NL_P0].d());
    return r.sens ? sensor_update_launch(h, r.sens->ny, 0, st.a[M_SENS_H].d(), st.a[M_SENS_R].d(), st.ym, nullptr, st.xc, st.a[M_P].d(), nullptr, st.d_nis, nullptr)
                  : update_launch(h, r.est->measured, r.est->r, st.ym, st.xc, st.a[M_P].d(), nullptr, st.d_nis, nullptr);
}
static int mpc_predict(ilqr_handle* h, const MpcRun& r, const MpcState& st) {
    return predict_launch(h, r.d->steps, r.d->plant_feedback, st.u_min, st.u_max, r.est ? r.est->q : (r.sens ? r.sens->q : r.nls->q), st.xc, st.a[M_P].d());
}

// the seam before the plant steps of period p: a delayed run only
static int mpc_before_step(ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t p) {
    if (!st.delayed) return ILQR_OK;
    const ilqr_mpc_desc* d = r.d;
    ILQR_TRY(mpc_measure(h, r, st, p * d->steps));
    if (st.filt) {
        // the measurement of the state at p·k corrects the estimate, which then moves on to (p+1)·k under the plan in flight
        ILQR_TRY(mpc_update(h, r, st));
        return mpc_predict(h, r, st);
    }
    // the solve of this period started one period ago: from a measurement of the state at p·k, moved on by the controller's
    // own model under the plan in flight — same feedback and limits, no process noise, the handle's parameters, no outputs
    return plant_launch(h, plant_args(h, d->steps, d->plant_feedback, d->seed, d->first_instance, p * d->steps, nullptr, st.u_min, st.u_max), nullptr,
                        st.xc, nullptr, nullptr, nullptr, nullptr);
}

// the plant steps of period p: rows p·k .. of the run's arrays
static ilqr::PlantArgs mpc_plant_args(const ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t p) {
    const ilqr_mpc_desc* d = r.d;
    ilqr::PlantArgs a = plant_args(h, d->steps, d->plant_feedback, d->seed, d->first_instance, p * d->steps, d->sigma_x, st.u_min, st.u_max);
    a.w = st.a[M_W].d(); a.x = st.xp; a.x_out = st.d_x_cl; a.u_out = st.d_u_cl; a.nonfinite = st.a[M_NONFINITE].i();
    a.saturated = st.a[M_SATURATED].i();
    a.nf_global = 1;
    a.w_ld = st.rows; a.x_ld = st.rows + 1; a.u_ld = st.rows;
    a.w_row0 = a.x_row0 = a.u_row0 = (long long)p * d->steps;
    return a;
}

// the seam after them: the measurement of the new state and the filter (a run without delay), row p of y_cl and of the filter's logs
static int mpc_after_step(ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t p) {
    const Staged* a = st.a;
    const size_t B = (size_t)h->B, n = (size_t)h->L.nx, P = (size_t)r.d->periods;
    if (st.measured && !st.delayed) ILQR_TRY(mpc_measure(h, r, st, (p + 1) * r.d->steps));
    if (st.filt && !st.delayed) {                  // the estimate moves on to (p+1)·k under the plan in flight, then takes the measurement in
        ILQR_TRY(mpc_predict(h, r, st));
        ILQR_TRY(mpc_update(h, r, st));
    }
    if (a[M_Y_CL].p)                               // row p of y_cl: what the controller is given, with a filter the measurement taken
        HIP_TRY(hipMemcpy2DAsync(a[M_Y_CL].d() + (size_t)p * st.ym_n, P * st.ym_n * 8, st.ym, st.ym_n * 8, st.ym_n * 8, B, hipMemcpyDeviceToDevice, h->stream));
    if (a[M_XHAT_CL].p || a[M_PDIAG_CL].p || a[M_NIS_CL].p) {
        const unsigned grid = (unsigned)((B * n + 255) / 256);
        hipLaunchKernelGGL(estimate_log_kernel, dim3(grid), dim3(256), 0, h->stream, (int)B, (int)n, r.d->periods, p, st.xc, a[M_P].d(), st.d_nis,
                           a[M_XHAT_CL].d(), a[M_PDIAG_CL].d(), a[M_NIS_CL].d());
        if (hipGetLastError() != hipSuccess) return fail(ILQR_ERR_HIP, "estimator log launch failed");
    }
    return ILQR_OK;
}

// the score of period p's steps — before the shift: it overwrites the θ rows 0 .. k−1 the plant ran under
static int mpc_score(ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t p) {
    ilqr::ScoreArgs q = score_args(h, r.d->steps);
    q.w = st.a[M_W].d(); q.x = st.d_x_cl; q.u = st.d_u_cl; q.cost = st.a[M_COST].d(); q.viol = st.a[M_VIOL].d();
    q.w_ld = q.u_ld = q.cost_ld = q.viol_ld = st.rows; q.x_ld = st.rows + 1;
    q.w_row0 = q.x_row0 = q.u_row0 = q.cost_row0 = q.viol_row0 = (long long)p * r.d->steps;
    if (h->vt->launch_plant_score(&q, h->stream) != 0) return fail(ILQR_ERR_HIP, "plant score launch failed");
    return ILQR_OK;
}

// the re-solve of period p: the horizon shifted onto the controller's view of the plant state, the duals with it, the solve
static int mpc_resolve(ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t p) {
    const ilqr_mpc_desc* d = r.d;
    ILQR_TRY(shift_launch(h, d->steps, d->shift_tail, d->shift_feedback, st.xc, st.a[M_PREVIEW].d(), st.rows, (long long)p * d->steps));
    if (d->warm) ILQR_TRY(ilqr_shift_duals_device(h, d->steps, d->duals_tail, d->duals_penalty));
    return d->warm ? ilqr_solve_warm(h) : ilqr_solve(h);
}

// row p of the log: the solve's statistics beside the plant launch's arguments
static int mpc_log_row(ilqr_handle* h, const MpcRun& r, const MpcState& st, int32_t p) {
    ilqr::PlantArgs a = mpc_plant_args(h, r, st, p);
    a.log = st.a[M_LOG].d(); a.log_ld = r.d->periods; a.log_row = p;
    if (h->vt->launch_mpc_log(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "log launch failed");
    return ILQR_OK;
}

// the run on one handle whose instances start at `lo` of the caller's batch: the order of everything it enqueues
static int mpc_enqueue(ilqr_handle* h, const MpcRun& run, bool measured, size_t lo, const Staged* arrays) {
    ilqr_mpc_desc d = *run.d;
    d.first_instance += (int64_t)lo;
    MpcRun r = run;
    r.d = &d;
    MpcState st = {};
    st.a = arrays; st.measured = measured;
    ILQR_TRY(mpc_begin(h, r, st));
    for (int32_t p = 0; p < d.periods; ++p) {
        ILQR_TRY(mpc_before_step(h, r, st, p));
        ilqr::PlantArgs a = mpc_plant_args(h, r, st, p);
        if (h->vt->launch_plant(&a, h->stream) != 0) return fail(ILQR_ERR_HIP, "plant step launch failed");
        ILQR_TRY(mpc_after_step(h, r, st, p));
        if (st.score) ILQR_TRY(mpc_score(h, r, st, p));
        ILQR_TRY(mpc_resolve(h, r, st, p));
        if (arrays[M_LOG].p) ILQR_TRY(mpc_log_row(h, r, st, p));
    }
    return ILQR_OK;
}

// Every entry point of the loop is this. With nothing measured (mpc_measured) the seam is skipped, with w_preview, cl_cost and
// cl_violation null the preview and the score are: a null array has no bytes, no buffer and a null device pointer (run_staged), and
// every stage of a period looks at its own flag of MpcState alone — so no launch, no buffer and no argument differs from the plainer
// entry point's.
static int mpc_run(ilqr_handle* h, const MpcRun& r) {
    const bool measured = mpc_measured(r);
    ILQR_TRY(mpc_check(h, r, measured));
    if (!h->vt->launch_plant || !h->vt->launch_mpc_log) return fail(ILQR_ERR_MODEL, "this model module has no plant kernel");
    if (r.cl_cost && !h->vt->launch_plant_score) return fail(ILQR_ERR_MODEL, "this model module has no plant score kernel");
    if (measured && !h->vt->launch_plant_measure) return fail(ILQR_ERR_MODEL, "this model module has no measurement kernel");
    if (r.est && (!h->vt->launch_estimate_predict || !h->vt->launch_estimate_update)) return fail(ILQR_ERR_MODEL, "this model module has no estimator kernel");
    if (r.sens && (!h->vt->launch_estimate_predict || !h->vt->launch_sensor_update || !h->vt->launch_plant_measure_linear))
        return fail(ILQR_ERR_MODEL, "this model module has no linear sensor kernel");
    if (r.nls && (!h->vt->launch_estimate_predict || !h->vt->launch_sensor_update))
        return fail(ILQR_ERR_MODEL, "this model module has no estimator or sensor update kernel for a nonlinear sensor to run on");
    return run_staged(h, mpc_arrays(h, r, measured),
                      [&](ilqr_handle* s, size_t lo, const Staged* arrays) { return mpc_enqueue(s, r, measured, lo, arrays); });
}

int ilqr_mpc_run(ilqr_handle* h, const ilqr_mpc_desc* d, const double* x0, const double* w_plant, double* x_cl, double* u_cl, double* log,
                 int32_t* first_nonfinite) {
    MpcRun r = {}; r.who = "ilqr_mpc_run"; r.d = d;
    r.x0 = x0; r.w_plant = w_plant;
    r.x_cl = x_cl; r.u_cl = u_cl; r.log = log; r.first_nonfinite = first_nonfinite;
    return mpc_run(h, r);
}

int ilqr_mpc_run_preview(ilqr_handle* h, const ilqr_mpc_desc* d, const double* x0, const double* w_plant, const double* w_preview, double* x_cl,
                         double* u_cl, double* log, int32_t* first_nonfinite, double* cl_cost, double* cl_violation) {
    MpcRun r = {}; r.who = "ilqr_mpc_run_preview"; r.d = d;
    r.x0 = x0; r.w_plant = w_plant; r.w_preview = w_preview;
    r.x_cl = x_cl; r.u_cl = u_cl; r.log = log; r.first_nonfinite = first_nonfinite; r.cl_cost = cl_cost; r.cl_violation = cl_violation;
    return mpc_run(h, r);
}

int ilqr_mpc_run_io(ilqr_handle* h, const ilqr_mpc_desc* d, const ilqr_plant_io* io, const double* x0, const double* w_plant, const double* w_preview,
                    double* x_cl, double* u_cl, double* log, int32_t* first_nonfinite, double* cl_cost, double* cl_violation, double* y_cl,
                    int32_t* saturated) {
    MpcRun r = {}; r.who = "ilqr_mpc_run_io"; r.d = d; r.io = io;
    r.x0 = x0; r.w_plant = w_plant; r.w_preview = w_preview;
    r.x_cl = x_cl; r.u_cl = u_cl; r.log = log; r.first_nonfinite = first_nonfinite; r.cl_cost = cl_cost; r.cl_violation = cl_violation;
    r.y_cl = y_cl; r.saturated = saturated;
    return mpc_run(h, r);
}

int ilqr_mpc_run_est(ilqr_handle* h, const ilqr_mpc_desc* d, const ilqr_plant_io* io, const ilqr_estimator* est, const double* x0, const double* xhat0,
                     double* P, const double* w_plant, const double* w_preview, double* x_cl, double* u_cl, double* log, int32_t* first_nonfinite,
                     double* cl_cost, double* cl_violation, double* y_cl, int32_t* saturated, double* xhat_cl, double* pdiag_cl, double* nis_cl) {
    MpcRun r = {}; r.who = "ilqr_mpc_run_est"; r.d = d; r.io = io; r.est = est;
    r.x0 = x0; r.xhat0 = xhat0; r.Pcov = P; r.w_plant = w_plant; r.w_preview = w_preview;
    r.x_cl = x_cl; r.u_cl = u_cl; r.log = log; r.first_nonfinite = first_nonfinite; r.cl_cost = cl_cost; r.cl_violation = cl_violation;
    r.y_cl = y_cl; r.saturated = saturated; r.xhat_cl = xhat_cl; r.pdiag_cl = pdiag_cl; r.nis_cl = nis_cl;
    return mpc_run(h, r);
}

int ilqr_mpc_run_sensor(ilqr_handle* h, const ilqr_mpc_desc* d, const ilqr_plant_io* io, const ilqr_sensor* sensor, const double* x0,
                        const double* xhat0, double* P, const double* w_plant, const double* w_preview, double* x_cl, double* u_cl, double* log,
                        int32_t* first_nonfinite, double* cl_cost, double* cl_violation, double* y_cl, int32_t* saturated, double* xhat_cl,
                        double* pdiag_cl, double* nis_cl) {
    MpcRun r = {}; r.who = "ilqr_mpc_run_sensor"; r.d = d; r.io = io; r.sens = sensor;
    r.x0 = x0; r.xhat0 = xhat0; r.Pcov = P; r.w_plant = w_plant; r.w_preview = w_preview;
    r.x_cl = x_cl; r.u_cl = u_cl; r.log = log; r.first_nonfinite = first_nonfinite; r.cl_cost = cl_cost; r.cl_violation = cl_violation;
    r.y_cl = y_cl; r.saturated = saturated; r.xhat_cl = xhat_cl; r.pdiag_cl = pdiag_cl; r.nis_cl = nis_cl;
    return mpc_run(h, r);
}

int ilqr_mpc_run_nlsensor(ilqr_handle* h, const ilqr_mpc_desc* d, const ilqr_plant_io* io, const ilqr_nl_sensor* sensor, const double* x0,
                          const double* xhat0, double* P, const double* w_plant, const double* w_preview, double* x_cl, double* u_cl, double* log,
                          int32_t* first_nonfinite, double* cl_cost, double* cl_violation, double* y_cl, int32_t* saturated, double* xhat_cl,
                          double* pdiag_cl, double* nis_cl) {
    MpcRun r = {}; r.who = "ilqr_mpc_run_nlsensor"; r.d = d; r.io = io; r.nls = sensor;
    r.nlv = sensor && sensor->sensor ? find_sensor(sensor->sensor) : nullptr;          // (an unknown name: mpc_check refuses it)
    r.x0 = x0; r.xhat0 = xhat0; r.Pcov = P; r.w_plant = w_plant; r.w_preview = w_preview;
    r.x_cl = x_cl; r.u_cl = u_cl; r.log = log; r.first_nonfinite = first_nonfinite; r.cl_cost = cl_cost; r.cl_violation = cl_violation;
    r.y_cl = y_cl; r.saturated = saturated; r.xhat_cl = xhat_cl; r.pdiag_cl = pdiag_cl; r.nis_cl = nis_cl;
    return mpc_run(h, r);
}

int ilqr_set_kernel_variant(ilqr_handle* h, int32_t variant) {
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_set_kernel_variant(s, variant); });
    if (!h || variant < 0 || variant > 6) return fail(ILQR_ERR_INVALID, "variant must be 0 (auto), 1 (latency), 2 (throughput), 3 (packed), 4 (one wave per instance of a large model), 5 / 6 (packed with one / two waves per pack)");
    if (variant == 4 && !has_kernel(h->vt, ilqr::K_MID))
        return fail(ILQR_ERR_INVALID, "the one-wave variant exists for large models with nx, nu <= 16 only");
    if ((variant == 3 || variant == 5 || variant == 6) && !has_kernel(h->vt, ilqr::K_PACKED1))
        return fail(ILQR_ERR_INVALID, "the packed variant exists for small models (nx, nu <= 4) only");
    if ((variant == 1 || variant == 2) && !h->lds_fits)
        return fail(ILQR_ERR_LDS, "this horizon exceeds the LDS-resident kernels: only the packed variant can run it");
    if (variant == 2 && !has_kernel(h->vt, ilqr::K_SLIM))
        return fail(ILQR_ERR_INVALID, "the throughput variant exists for small models (nx, nu <= 4) only");
    h->variant = variant;
    return ILQR_OK;
}

// what ilqr_solve launches for this handle as it stands (variant, batch, horizon): the kernel of its launch plan
int ilqr_resolved_kernel_variant(ilqr_handle* h, int32_t* variant) {
    if (!h || !variant) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return ilqr_resolved_kernel_variant(h->shards[0], variant);
    *variant = ilqr::solve_plan(launch_in(h)).kernel;
    return ILQR_OK;
}

int ilqr_set_handover(ilqr_handle* h, int32_t outer) {
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_set_handover(s, outer); });
    if (!h || outer < -1 || outer == 1) return fail(ILQR_ERR_INVALID, "hand-over: -1 (auto), 0 (off) or the outer iteration (>= 2) from which stragglers leave the packed kernel");
    h->handover = outer;
    return ILQR_OK;
}

int ilqr_set_handover_live(ilqr_handle* h, int32_t live) {
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_set_handover_live(s, live); });
    if (!h || live < -1) return fail(ILQR_ERR_INVALID, "hand-over by head count: -1 (auto), 0 (off) or the number of surviving instances at which they leave the packed kernel");
    h->handover_live = live;
    return ILQR_OK;
}

int ilqr_set_handover_mark(ilqr_handle* h, int32_t rejected) {
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_set_handover_mark(s, rejected); });
    if (!h || rejected < -1) return fail(ILQR_ERR_INVALID, "straggler mark: -1 (auto), 0 (never) or the number of rejected line-search trials above the batch's mean at which an instance leaves the packed kernel at once");
    h->handover_mark = rejected;
    return ILQR_OK;
}

int ilqr_get_handover_stats(ilqr_handle* h, int32_t* queued, int32_t* marked) {
    if (!h || !queued || !marked) return fail(ILQR_ERR_INVALID, "null argument");
    *queued = 0; *marked = 0;
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) {
        int32_t q = 0, m = 0;
        const int rc = ilqr_get_handover_stats(s, &q, &m);
        *queued += q; *marked += m;
        return rc; });
    if (h->pool == nullptr || !h->pool_valid) return ILQR_OK;      // the last solve did not go through the queue: 0 / 0
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int words[ilqr::POOL_Q];
    HIP_TRY(hipMemcpy(words, h->pool, sizeof(words), hipMemcpyDeviceToHost));
    *queued = words[ilqr::POOL_TAIL]; *marked = words[ilqr::POOL_MARKED];
    return ILQR_OK;
}

int ilqr_enable_trace(ilqr_handle* h, int32_t capacity) {
    if (!h || capacity < 0) return fail(ILQR_ERR_INVALID, "bad argument");
    if (SHARDED(h)) { h->trace_cap = capacity; return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_enable_trace(s, capacity); }); }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->trace) { HIP_TRY(hipFree(h->trace)); h->trace = nullptr; }
    h->trace_cap = capacity;
    if (capacity > 0) {
        const size_t bytes = (size_t)h->B * capacity * ilqr::TRACE_W * 8;
        HIP_TRY(hipMalloc((void**)&h->trace, bytes));
        HIP_TRY(hipMemset(h->trace, 0, bytes));
    }
    return ILQR_OK;
}

int ilqr_get_trace(ilqr_handle* h, double* out) {
    if (!h || !out) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t lo) { return ilqr_get_trace(s, out + lo * (size_t)h->trace_cap * ilqr::TRACE_W); }, true);
    if (!h->trace) return fail(ILQR_ERR_INVALID, "trace not enabled");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->trace, (size_t)h->B * h->trace_cap * ilqr::TRACE_W * 8, hipMemcpyDeviceToHost));
    return ILQR_OK;
}

int ilqr_get_stream(ilqr_handle* h, void** s) {
    if (!h || !s) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) return fail(ILQR_ERR_INVALID, "a sharded handle has one stream per device: synchronise with ilqr_synchronize");
    *s = (void*)h->stream;
    return ILQR_OK;
}

int ilqr_timing_reset(ilqr_handle* h) {
    if (!h) return fail(ILQR_ERR_INVALID, "null handle");
    if (SHARDED(h)) return each_shard(h, [&](ilqr_handle* s, size_t) { return ilqr_timing_reset(s); });
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (auto& p : h->timing) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    h->timing.clear();
    return ILQR_OK;
}

int ilqr_timing_get(ilqr_handle* h, double* ms_avg, int32_t* launches) {
    if (!h || !ms_avg) return fail(ILQR_ERR_INVALID, "null argument");
    if (SHARDED(h)) {          // the devices run side by side: the slowest shard's kernel time
        double worst = 0.0; int32_t nl = 0;
        const int rc = each_shard(h, [&](ilqr_handle* s, size_t) {
            double ms = 0.0; int32_t n_ = 0;
            const int r = ilqr_timing_get(s, &ms, &n_);
            if (ms > worst) worst = ms;
            nl = n_;
            return r; });
        *ms_avg = worst;
        if (launches) *launches = nl;
        return rc;
    }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double total = 0.0;
    for (auto& p : h->timing) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        total += ms;
    }
    *ms_avg = h->timing.empty() ? 0.0 : total / (double)h->timing.size();
    if (launches) *launches = (int32_t)h->timing.size();
    return ILQR_OK;
}

}  // extern "C"
