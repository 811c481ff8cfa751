// The seam between the two host halves of libilqr_hip.so: ilqr_api.hip (handles, registry, launches; compiled by hipcc) and
// ilqr_model_compile.cpp (the model compiler; plain C++17, no HIP). Device code does not include this header. Everything in it
// is internal: hidden from the library's dynamic symbol table, which holds the entry points of include/ilqr_hip.h alone.
#pragma once
#include <string>
#include <vector>
#include "../../include/ilqr_hip.h"

#define ILQR_INTERNAL __attribute__((visibility("hidden")))

namespace ilqr {

// ---- defined in ilqr_api.hip, where the registry and the one thread-local error string (ilqr_last_error) live
ILQR_INTERNAL int fail(int code, const std::string& msg);                  // sets the message, returns code
ILQR_INTERNAL const ilqr_model_vtable* find_model(const char* name);       // the registered module of that name, or nullptr
// eighth word of a model module's hash: ILQR_MODEL_ABI_VERSION * 1000 + sizeof(KArgs)
ILQR_INTERNAL long long model_abi_word();
// the sensor registry's side of the same (ilqr_compile_sensor): a registered sensor module's presence, and the word of its hash,
// ILQR_SENSOR_ABI_VERSION * 1000 + sizeof(SensorNlArgs)
ILQR_INTERNAL bool sensor_registered(const char* name);
ILQR_INTERNAL long long sensor_abi_word();

// ---- defined in ilqr_model_compile.cpp
// what the structure probe found of a large model's callables
struct ILQR_INTERNAL ModelStructure {
    bool found = false;
    std::vector<double> fxc, fuc;          // constant Jacobian entries (0 where state-dependent)
    std::vector<int> jac_var;              // indices into [fx | fu] of the state-dependent ones
    std::vector<int> hess_idx, tile_start; // compact Hessian row: [gxx by 16x16 tile | guu | gux], indices inside each matrix
    int nxx = 0, nuu = 0, nux = 0;
    std::string note;
};
// selector columns of a lowered model (ilqr_compile_model_stages): the probe must visit every kind of every category
struct ILQR_INTERNAL ProbeHints { int sel[3] = {-1, -1, -1}; int kinds[3] = {0, 0, 0}; };

// temporary files go to dir, named after tag
ILQR_INTERNAL ModelStructure probe_model_structure(const ilqr_model_source* src, const std::string& dir, const std::string& tag, const ProbeHints& hints);
// the same, served from dir/probe_<tag>_<hash of hints>.bin when a successful probe left one there
ILQR_INTERNAL ModelStructure probe_model_structure_cached(const ilqr_model_source* src, const std::string& dir, const std::string& tag, const ProbeHints& hints);
ILQR_INTERNAL std::string compose_stage_source(const ilqr_stage_kinds* k, const ilqr_stage_plan& pl, const char* user_source);

}  // namespace ilqr
