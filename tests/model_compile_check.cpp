// Host-side check of the model compiler (iterativelqr.jl_amd/csrc/ilqr_model_compile.cpp); built together with it and run by
// tests/test_model_compile_host.py: no hipcc, no libilqr_hip.so, no GPU. argv: the C source of synth12, a scratch directory.
// Prints one line per check and exits non-zero on the first that fails.
// Second form, run by tests/test_coupled_problem.py: --probe, a scratch directory, then pairs of files — the C callables of a model
// and the compact Hessian row expected of the probe ("nx nu nc_stage", "nxx nuu nux", the indices, the tile starts; a fifth line, where
// tests/test_coupled_dynamics.py gives one: the state-dependent Jacobian entries, indices into [fx (nx*nx) | fu (nx*nu)], both column-major).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <utility>
#include "ilqr_host.hpp"

using namespace ilqr;
namespace fs = std::filesystem;

// what ilqr_api.hip gives the model compiler inside the library
static std::string last_error;
int ilqr::fail(int code, const std::string& msg) { last_error = msg; return code; }
const ilqr_model_vtable* ilqr::find_model(const char*) { return nullptr; }
long long ilqr::model_abi_word() { return 0; }

static int checks = 0;
#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, last_error.c_str()); std::exit(1); } \
        ++checks; std::printf("ok %s\n", #cond);                                                        \
    } while (0)

static size_t count(const std::string& s, const std::string& what) {
    size_t n = 0;
    for (size_t p = s.find(what); p != std::string::npos; p = s.find(what, p + 1)) ++n;
    return n;
}
static bool same(const ModelStructure& a, const ModelStructure& b) {
    return a.found == b.found && a.fxc == b.fxc && a.fuc == b.fuc && a.jac_var == b.jac_var && a.hess_idx == b.hess_idx &&
           a.tile_start == b.tile_start && a.nxx == b.nxx && a.nuu == b.nuu && a.nux == b.nux;
}
static std::vector<fs::path> bins(const std::string& dir) {
    std::vector<fs::path> v;
    for (auto& e : fs::directory_iterator(dir)) if (e.path().extension() == ".bin") v.push_back(e.path());
    return v;
}

static std::vector<int> ints(const std::string& line) {
    std::vector<int> v;
    std::stringstream s(line);
    for (int e; s >> e;) v.push_back(e);
    return v;
}

// the probe on models whose Hessians are coupled: gux entries, off-diagonal gxx / guu entries, several gxx tiles
static int probe_given_models(int argc, char** argv) {
    const std::string dir = argv[2];
    for (int a = 3; a + 1 < argc; a += 2) {
        std::stringstream text;
        text << std::ifstream(argv[a]).rdbuf();
        const std::string source = text.str();
        std::ifstream expect(argv[a + 1]);
        std::string l0, l1, l2, l3, l4;
        std::getline(expect, l0); std::getline(expect, l1); std::getline(expect, l2); std::getline(expect, l3); std::getline(expect, l4);
        const std::vector<int> dims = ints(l0), sizes = ints(l1), idx = ints(l2), starts = ints(l3);
        CHECK(dims.size() == 3 && sizes.size() == 3 && (int)idx.size() == sizes[0] + sizes[1] + sizes[2]);
        ilqr_model_source src = {"coupled_host", dims[0], dims[1], 0, dims[2], 0, (1ull << dims[2]) - 1, 0, source.c_str(), 0};
        const ModelStructure ms = probe_model_structure(&src, dir, "coupled", ProbeHints());
        CHECK(ms.found);
        CHECK(ms.nxx == sizes[0] && ms.nuu == sizes[1] && ms.nux == sizes[2] && (ms.nux > 0 || !l4.empty()));
        CHECK(ms.hess_idx == idx);
        CHECK(ms.tile_start == starts);
        if (!l4.empty()) CHECK(ms.jac_var == ints(l4));
    }
    std::printf("%d checks passed\n", checks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 5 && std::strcmp(argv[1], "--probe") == 0) return probe_given_models(argc, argv);
    if (argc != 3) return 2;
    std::stringstream text;
    text << std::ifstream(argv[1]).rdbuf();
    const std::string synth12 = text.str(), dir = argv[2];

    // ---- the probe on synth12 (tests/test_structure_probe.py asserts the same numbers through the whole library):
    // fx = I + h (A + diag(0.1 cos x_i + 0.02 u_{i mod 5})): the 12 diagonal entries depend on the state; fu = h (B + 0.02 x_i at
    // (i, i mod 5)): 12 more. gxx: the diagonal (cost; the terminal rows' Gauss-Newton terms lie on it), guu: the diagonal, gux: nothing
    ilqr_model_source src = {"synth12_host", 12, 5, 0, 10, 3, (1ull << 10) - 1, 0, synth12.c_str(), 0};
    const ModelStructure ms = probe_model_structure(&src, dir, "check", ProbeHints());
    CHECK(ms.found);
    CHECK(ms.jac_var.size() == 24);
    CHECK(ms.nxx == 12 && ms.nuu == 5 && ms.nux == 0 && ms.hess_idx.size() == 12 + 5);
    CHECK(ms.fxc.size() == 12 * 12 && ms.fuc.size() == 12 * 5 && ms.tile_start.size() == 2);
    CHECK(fs::is_empty(dir));                                            // the probe's temporary files are gone

    // ---- switched off for this model
    ilqr_model_source dense = src;
    dense.flags = ILQR_MODEL_DENSE_TABLES;
    const ModelStructure off = probe_model_structure(&dense, dir, "check", ProbeHints());
    CHECK(!off.found && off.note.find("ILQR_MODEL_DENSE_TABLES") != std::string::npos);

    // ---- the cache: probed once, then served from the .bin; a truncated .bin is ignored and written again
    const ModelStructure c1 = probe_model_structure_cached(&src, dir, "check", ProbeHints());
    CHECK(c1.found && same(c1, ms) && c1.note.find("structure from") == std::string::npos);
    CHECK(bins(dir).size() == 1);
    const fs::path bin = bins(dir)[0];
    const auto full = fs::file_size(bin);
    const ModelStructure c2 = probe_model_structure_cached(&src, dir, "check", ProbeHints());
    CHECK(c2.note == "structure from " + bin.string() && same(c2, ms));
    fs::resize_file(bin, full / 2);
    const ModelStructure c3 = probe_model_structure_cached(&src, dir, "check", ProbeHints());
    CHECK(c3.found && same(c3, ms) && c3.note.find("structure from") == std::string::npos);
    CHECK(fs::file_size(bin) == full);
    const ModelStructure c4 = probe_model_structure_cached(&dense, dir, "check", ProbeHints());
    CHECK(!c4.found);                                                    // a model that is switched off is not served from the cache

    // ---- the stage plan of a hand-written problem, T = 5, one user parameter:
    //   step 0:      dynamics 0 (2 states, 1 action -> 3 states), cost 0 (2, 1), constraint 0 (2 equality rows)
    //   steps 1 - 3: dynamics 1 (3, 2 -> 3),                       cost 1 (3, 2), constraint 1 (3 rows, rows 0 and 2 inequalities)
    //   terminal:    3 states, 1 constraint row
    const int32_t d_nx[2] = {2, 3}, d_nu[2] = {1, 2}, d_next[2] = {3, 3}, c_nx[2] = {2, 3}, c_nu[2] = {1, 2};
    const int32_t q_nc[2] = {2, 3}, q_nx[2] = {2, 3}, q_nu[2] = {1, 2}, of_step[4] = {0, 1, 1, 1};
    const uint64_t q_ineq[2 * 4] = {0, 0, 0, 0, 0b101, 0, 0, 0};
    ilqr_stage_kinds k;
    std::memset(&k, 0, sizeof(k));
    k.horizon = 5; k.num_parameter = 1;
    k.n_dynamics = 2; k.dynamics_nx = d_nx; k.dynamics_nu = d_nu; k.dynamics_nx_next = d_next; k.dynamics_of_step = of_step;
    k.n_costs = 2; k.cost_nx = c_nx; k.cost_nu = c_nu; k.cost_of_step = of_step;
    k.n_constraints = 2; k.constraint_nc = q_nc; k.constraint_nx = q_nx; k.constraint_nu = q_nu; k.constraint_ineq = q_ineq; k.constraint_of_step = of_step;
    k.nx_term = 3; k.nc_term = 1;
    ilqr_stage_plan pl;
    double sel[5 * 6];
    int32_t sdim[5], adim[4];
    CHECK(ilqr_plan_stages(&k, &pl, sel, 5 * 6, sdim, adim) == ILQR_OK);
    // largest dimensions; all three categories vary, so the selector blocks follow the user's one parameter: columns 1-2, 3-4, 5-6
    CHECK(pl.nx == 3 && pl.nu == 2 && pl.nw == 7 && pl.n_selectors == 6);
    CHECK(pl.sel_dynamics == 1 && pl.sel_cost == 3 && pl.sel_constraint == 5);
    // kinds stacked: kind 0 owns rows 0-1, kind 1 rows 2-4; its inequality rows 0 and 2 are rows 2 and 4 of the stack
    CHECK(pl.nc_stage == 5 && pl.nc_term == 1 && pl.constraint_row0[0] == 0 && pl.constraint_row0[1] == 2);
    CHECK(pl.ineq_stage_words[0] == 0b10100 && pl.ineq_stage_words[1] == 0 && pl.ineq_stage_words[2] == 0 && pl.ineq_stage_words[3] == 0);
    const double want_sel[5 * 6] = {1, 0, 1, 0, 1, 0,  0, 1, 0, 1, 0, 1,  0, 1, 0, 1, 0, 1,  0, 1, 0, 1, 0, 1,  0, 0, 0, 0, 0, 0};
    CHECK(std::memcmp(sel, want_sel, sizeof(sel)) == 0);
    const int32_t want_s[5] = {2, 3, 3, 3, 3}, want_a[4] = {1, 2, 2, 2};
    CHECK(std::memcmp(sdim, want_s, sizeof(sdim)) == 0 && std::memcmp(adim, want_a, sizeof(adim)) == 0);
    ilqr_stage_kinds bad = k;
    const int32_t wrong_next[2] = {2, 3};                                // dynamics 0 no longer produces the 3 states of step 1
    bad.dynamics_nx_next = wrong_next;
    CHECK(ilqr_plan_stages(&bad, &pl, nullptr, 0, nullptr, nullptr) == ILQR_ERR_INVALID && last_error.find("does not produce") != std::string::npos);
    CHECK(ilqr_plan_stages(&k, &pl, nullptr, 0, nullptr, nullptr) == ILQR_OK);

    // ---- the composed source around trivial kinds: every callable writes 1 to its first output, except the state Jacobian of
    // dynamics 1, whose first entry is x[0], and the matrices below, which say where the template's padded copies must put them:
    // both Jacobians of constraint 0 fill column 0 of their two rows; constraint 1 (3 rows) has column 1 of its rows 0 and 2 in the
    // state Jacobian and of its row 0 in the action Jacobian; the action-state Hessian of cost 0 (1 x 2) has its column 1
    const std::pair<const char*, const char*> special[] = {
        {"dynamics_1_jacobian_state", "o[0] = x[0];"},
        {"constraint_stage_0_jacobian_state", "o[0] = 1.0; o[1] = 1.0;"}, {"constraint_stage_0_jacobian_action", "o[0] = 1.0; o[1] = 1.0;"},
        {"constraint_stage_1_jacobian_state", "o[1 * 3 + 0] = 1.0; o[1 * 3 + 2] = 1.0;"}, {"constraint_stage_1_jacobian_action", "o[1 * 3 + 0] = 1.0;"},
        {"cost_stage_0_hessian_action_state", "o[1] = 1.0;"}};
    std::string kinds;
    auto def = [&](const std::string& name) {
        const char* body = "o[0] = 1.0;";
        for (auto& sp : special) if (name == sp.first) body = sp.second;
        kinds += "ILQR_MODEL_FN void " + name + "(double* o, const double* x, const double* u, const double* w) { " + body + " }\n";
    };
    const std::vector<std::string> dyn = {"", "_jacobian_state", "_jacobian_action"}, con = dyn;
    const std::vector<std::string> cost = {"", "_gradient_state", "_gradient_action", "_hessian_state_state", "_hessian_action_action", "_hessian_action_state"};
    for (int q = 0; q < 2; ++q) {
        for (auto& s : dyn) def("dynamics_" + std::to_string(q) + s);
        for (auto& s : cost) def("cost_stage_" + std::to_string(q) + s);
        for (auto& s : con) def("constraint_stage_" + std::to_string(q) + s);
    }
    for (const char* s : {"cost_terminal", "cost_terminal_gradient_state", "cost_terminal_hessian_state_state", "constraint_terminal", "constraint_terminal_jacobian_state"}) def(s);
    const std::string all = compose_stage_source(&k, pl, kinds.c_str());
    const std::string head = "namespace kinds {\n" + kinds + "\n}\n";
    CHECK(all.compare(0, head.size(), head) == 0);
    const std::string combined = all.substr(head.size());
    std::vector<std::string> names = {"cost_terminal", "cost_terminal_gradient_state", "cost_terminal_hessian_state_state", "constraint_terminal", "constraint_terminal_jacobian_state"};
    for (auto& s : dyn) names.push_back("dynamics" + s);
    for (auto& s : cost) names.push_back("cost_stage" + s);
    for (auto& s : con) names.push_back("constraint_stage" + s);
    bool once = names.size() == 17;
    for (auto& nm : names) once = once && count(combined, "ILQR_MODEL_FN void " + nm + "(") == 1;
    CHECK(once && count(combined, "ILQR_MODEL_FN") == 17);
    // one selector chain per combined callable of a varying category: 3 for the dynamics, 6 for the cost, 3 for the constraint
    CHECK(count(combined, "    if (w[1] > 0.5) {") == 3 && count(combined, "    else if (w[2] > 0.5) {") == 3);
    CHECK(count(combined, "    if (w[3] > 0.5) {") == 6 && count(combined, "    else if (w[4] > 0.5) {") == 6);
    CHECK(count(combined, "    if (w[5] > 0.5) {") == 3 && count(combined, "    else if (w[6] > 0.5) {") == 3);
    CHECK(count(combined, "> 0.5") == 24);
    // it compiles and runs as the probe wraps it, with the hints ilqr_compile_model_stages passes. By the lowering rules: fx[0]
    // is 1 under dynamics 0 and x[0] under dynamics 1, every other Jacobian entry is constant. The Hessian pattern pins the padded
    // copies by position, since a Gauss-Newton term couples the columns that share a ROW of cx (5 x 3) and cu (5 x 2). Constraint 1
    // owns rows 2-4 of the stack: rows 2 and 4 hold state 1, row 2 holds action 1, and rows 0-1 (constraint 0) hold state 0 and
    // action 0, so there are no cross terms: gxx (0, 0) and (1, 1) = 1 * 3 + 1, guu (0, 0) and (1, 1) = 1 * 2 + 1, gux (action 0,
    // state 0) and (action 1, state 1) = 1 * 2 + 1. An entry copied to another row or column of the stack meets state 0 or
    // action 0 there, or leaves the row-2 pair apart. The costs add the first entry of each; cost 0 pads action 1 with the unit
    // diagonal guu (1, 1), and its gux column 1 lands at 1 * 2 + 0 under the template's two actions
    ilqr_model_source lowered = {"lowered", pl.nx, pl.nu, pl.nw, pl.nc_stage, pl.nc_term, pl.ineq_stage_words[0], 0, all.c_str(), 0};
    ProbeHints hints;
    hints.sel[0] = pl.sel_dynamics; hints.sel[1] = pl.sel_cost; hints.sel[2] = pl.sel_constraint;
    hints.kinds[0] = hints.kinds[1] = hints.kinds[2] = 2;
    const ModelStructure ls = probe_model_structure(&lowered, dir, "lowered", hints);
    CHECK(ls.found);
    CHECK(ls.jac_var == std::vector<int>{0});
    CHECK(ls.nxx == 2 && ls.nuu == 2 && ls.nux == 3 && (ls.hess_idx == std::vector<int>{0, 4, 0, 3, 0, 2, 3}));

    std::printf("%d checks passed\n", checks);
    return 0;
}
