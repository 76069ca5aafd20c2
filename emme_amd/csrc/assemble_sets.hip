// assemble_sets.hip -- M(omega_b) for batch items that each carry their own parameter set:
// k_assemble_sets and launch_assemble_sets, the plain sets reading of assemble_nodes_text.hpp.  Its own translation
// unit, so that the kernel keeps its own register allocation.
#define EMME_NODES_SETS 1
#define EMME_NODES_DERIV 0
#include "assemble_nodes_text.hpp"
