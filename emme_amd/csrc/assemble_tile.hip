// assemble_tile.hip -- the table-free tile fill of electrostatic GK15 batches that have no node cache: k_assemble_tile
// and launch_assemble_tile, the ES15 plain (M, fused secant) reading of assemble_tile_text.hpp.  Its own translation unit,
// so that the kernel is compiled from a token stream that holds nothing of the other readings.
#define EMME_TILE_SHAPE 0
#define EMME_TILE_SETS 0
#define EMME_TILE_DERIV 0
#include "assemble_tile_text.hpp"
