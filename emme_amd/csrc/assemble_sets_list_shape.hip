// assemble_sets_list_shape.hip -- the integrals the tile fill over parameter sets handed over on electromagnetic and GK31
// contexts, from scratch: k_assemble_sets_list_shape<PTS> and launch_assemble_sets_list_shape, the plain
// shape reading of assemble_sets_list_text.hpp.  Its own translation unit, as assemble_sets_list.hip.
#define EMME_SETS_LIST_SHAPE 1
#define EMME_SETS_LIST_DERIV 0
#include "assemble_sets_list_text.hpp"
