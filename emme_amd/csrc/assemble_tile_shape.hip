// assemble_tile_shape.hip -- the table-free tile fill for electromagnetic contexts and the 31-point rule:
// k_assemble_tile_shape<PTS, NM> and launch_assemble_tile_shape, the plain (M, fused secant) shape reading of
// assemble_tile_text.hpp.  Its own translation unit, so that the kernels are compiled from a token stream that holds
// nothing of the other readings.
#define EMME_TILE_SHAPE 1
#define EMME_TILE_SETS 0
#define EMME_TILE_DERIV 0
#include "assemble_tile_text.hpp"
