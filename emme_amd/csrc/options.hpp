// options.hpp -- the per-context options (emme_options_t, include/emme_hip.h) as plain C++, no HIP: their defaults,
// the EMME_* environment overrides, the range check, and which contexts take the tiled layout.  emme_capi.hip holds
// the ABI functions that call them; host_selftest.cpp pins every default, bound and override.
#pragma once
#include <string>

#include "../../include/emme_hip.h"

namespace emme {

void set_error(const std::string& msg);

void options_default(emme_options_t& o);
// The EMME_* environment variables: developer overrides, read ONCE per context (at creation), winning over
// the caller's struct.  Library callers use emme_options_t.
void options_env_overrides(emme_options_t& o);
int options_check(const emme_options_t* o);

// Which contexts get the tiled record layout + dense (matrix-core) fill (assemble_dense.hip): both quadrature orders,
// electrostatic and electromagnetic (BASELINE.json's configurations use electrostatic GK15 and electromagnetic GK31),
// on folded records, with the default fill option.  The dense path carries the safe_exp-clamped tails (<= 4e-14 absolute), so inputs whose absolute quadrature
// goal (integration_accuracy) is tighter than 1e-9 keep the exact kernels.
bool wants_tiled(const emme_params_t& p, bool folded, int fill);

}  // namespace emme
