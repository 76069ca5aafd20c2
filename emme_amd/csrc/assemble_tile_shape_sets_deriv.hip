// assemble_tile_shape_sets_deriv.hip -- M(omega) and the exact dM/domega from the table-free tile fill over parameter
// sets for electromagnetic contexts and the 31-point rule: k_assemble_tile_shape_sets_deriv<PTS, NM>
// and launch_assemble_tile_shape_sets_deriv, the derivative shape sets reading of assemble_tile_text.hpp.  Its own
// translation unit, as assemble_tile_shape_deriv.hip.
#define EMME_TILE_SHAPE 1
#define EMME_TILE_SETS 1
#define EMME_TILE_DERIV 1
#include "assemble_tile_text.hpp"
