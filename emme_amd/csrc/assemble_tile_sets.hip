// assemble_tile_sets.hip -- the table-free tile fill for batch items that each carry their own parameter set, a set per
// omega chunk: k_assemble_tile_sets and launch_assemble_tile_sets, the ES15 plain sets reading of
// assemble_tile_text.hpp.  Its own translation unit, as assemble_tile.hip.
#define EMME_TILE_SHAPE 0
#define EMME_TILE_SETS 1
#define EMME_TILE_DERIV 0
#include "assemble_tile_text.hpp"
