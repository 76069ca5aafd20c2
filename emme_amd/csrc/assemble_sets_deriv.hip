// assemble_sets_deriv.hip -- M(omega_b) and the exact dM/domega for batch items that each carry their own parameter
// set: k_assemble_sets_deriv and launch_assemble_sets_deriv, the derivative sets reading of
// assemble_nodes_text.hpp.  Its own translation unit, as assemble_sets.hip.
#define EMME_NODES_SETS 1
#define EMME_NODES_DERIV 1
#include "assemble_nodes_text.hpp"
