// Receding-horizon shift of the augmented-Lagrangian state of a handle (ilqr_shift_duals, include/ilqr_hip.h): with k = steps,
// N = T − 1, ncs / nct stage / terminal rows and λ, ρ as the workspace holds them (C = N·ncs + nct doubles per instance, stage row t
// at t·ncs, the terminal rows at N·ncs — al_update's indexing),
//
//   λ'_t = λ_{t+k}  (t < N−k),  then λ_{N−1} (hold) or 0 (zero);  the terminal rows stay
//   ρ'   keep:  as λ, the tail under zero gets ρ0;   reset:  ρ0 in every entry
//
// Pure copies: signs of inequality rows and bits are kept. The kernel reads only the Layout and writes only L.lam and L.rho.
//
// The shift is in place inside an instance block, element e from element e + k·ncs of the same range: a parallel copy would race.
// No staging buffer here (shift_copy_kernel's way, two launches): ONE workgroup owns an instance and walks its stage rows in
// ascending chunks of DUALS_THREADS elements — every lane reads its element's source into a register, the workgroup meets at a
// barrier, every lane writes. Why that is race-free: the element e reads a location s >= e (head: s = e + k·ncs; held tail: the
// same column of row N−1) in the pass of chunk(e), BEFORE that pass's barrier; a location s is written in the pass of chunk(s) >=
// chunk(e), AFTER that pass's barrier — or never: an element whose source is itself (row N−1 under hold) is not stored at all. So
// every read of a word comes before the barrier that precedes its only write. The trip count is the same for all lanes.
#pragma once

namespace ilqr {

struct DualsArgs {
    double* ws;              // the handle's workspace: only λ (L.lam) and ρ (L.rho) are touched
    Layout L;
    int B;
    int steps;               // k, 0 .. T-1
    int tail;                // 0 hold, 1 zero (ILQR_DUALS_TAIL_*)
    int penalty;             // 0 keep, 1 reset (ILQR_DUALS_PENALTY_*)
    double rho0;             // the handle's initial_constraint_penalty
};

enum { DUALS_THREADS = 128 };

// Templated on the model only so that every module carries its own copy (the kernel reads nothing of M: the Layout has it all).
template <class M>
__global__ __launch_bounds__(DUALS_THREADS) void shift_duals_kernel(DualsArgs a) {
    const Layout& L = a.L;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= a.B) return;                                  // (the whole workgroup: no barrier below is met by part of one)
    const int ncs = L.ncs, S = (L.T - 1) * ncs, kd = a.steps * ncs, head = S - kd;      // head: elements with a source k steps later
    double* lam = a.ws + (size_t)b * (size_t)L.stride + L.lam;
    double* rho = a.ws + (size_t)b * (size_t)L.stride + L.rho;
    const bool keep = a.penalty == 0, hold = a.tail == 0;
    if (kd > 0) {                                          // (hence ncs > 0; k == 0 or no stage rows: λ stays)
        for (int base = 0; base < S; base += DUALS_THREADS) {
            const int e = base + tid;
            const bool in = e < S, copied = in && (e < head || hold);
            const int src = e < head ? e + kd : S - ncs + e % ncs;
            double l = 0.0, r = a.rho0;
            if (copied) { l = lam[src]; if (keep) r = rho[src]; }
            __syncthreads();
            if (in && !(copied && src == e)) { lam[e] = l; if (keep) rho[e] = r; }
        }
    }
    if (!keep) for (int e = tid; e < L.C; e += DUALS_THREADS) rho[e] = a.rho0;
}

template <class M>
int launch_shift_duals(const DualsArgs* a, void* stream) {
    if (a->B < 1 || a->steps < 0 || a->steps > a->L.T - 1) return -1;
    hipLaunchKernelGGL(shift_duals_kernel<M>, dim3((unsigned)a->B), dim3(DUALS_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ilqr
