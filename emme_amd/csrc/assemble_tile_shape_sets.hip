// assemble_tile_shape_sets.hip -- the table-free tile fill over parameter sets for electromagnetic contexts and the
// 31-point rule, a set per omega chunk: k_assemble_tile_shape_sets<PTS, NM> and
// launch_assemble_tile_shape_sets, the plain shape sets reading of assemble_tile_text.hpp.  Its own translation unit, as
// assemble_tile_shape.hip.
#define EMME_TILE_SHAPE 1
#define EMME_TILE_SETS 1
#define EMME_TILE_DERIV 0
#include "assemble_tile_text.hpp"
