// assemble_tile_deriv.hip -- M(omega) and the exact dM/domega from one table-free tile fill:
// k_assemble_tile_deriv and launch_assemble_tile_deriv, the ES15 derivative reading of assemble_tile_text.hpp.  Its
// own translation unit, as assemble_tile.hip.
#define EMME_TILE_SHAPE 0
#define EMME_TILE_SETS 0
#define EMME_TILE_DERIV 1
#include "assemble_tile_text.hpp"
