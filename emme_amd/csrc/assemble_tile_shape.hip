// assemble_tile_shape.hip -- the table-free tile fill for electromagnetic contexts and the 31-point rule:
// k_assemble_tile_shape<PTS, NM> and launch_assemble_tile_shape, the plain (M, fused secant) reading of
// assemble_tile_shape_text.hpp.  Its own translation unit, so that the kernels are compiled from a token stream that holds
// nothing of the derivative kernels.
#define EMME_TILE_DERIV 0
#include "assemble_tile_shape_text.hpp"
