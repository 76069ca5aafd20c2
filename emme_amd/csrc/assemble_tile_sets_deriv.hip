// assemble_tile_sets_deriv.hip -- M(omega_b) and the exact dM/domega from the table-free tile fill over parameter sets
// (DESIGN.md 13.7): k_assemble_tile_sets_deriv and launch_assemble_tile_sets_deriv, the ES15 derivative sets reading of
// assemble_tile_text.hpp.  Its own translation unit, as assemble_tile.hip.
#define EMME_TILE_SHAPE 0
#define EMME_TILE_SETS 1
#define EMME_TILE_DERIV 1
#include "assemble_tile_text.hpp"
