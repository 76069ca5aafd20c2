// assemble_sets_list_deriv.hip -- M and M' of the integrals the derivative tile fill over parameter sets handed over,
// from scratch: k_assemble_sets_deriv_list and launch_assemble_sets_deriv_list, the derivative reading
// of assemble_sets_list_text.hpp.  Its own translation unit, as assemble_sets.hip.
#define EMME_SETS_LIST_SHAPE 0
#define EMME_SETS_LIST_DERIV 1
#include "assemble_sets_list_text.hpp"
