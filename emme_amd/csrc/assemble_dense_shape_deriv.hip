// assemble_dense_shape_deriv.hip -- M(omega) and the exact dM/domega from the tiled node cache for electromagnetic
// contexts and the 31-point rule: k_btab_shape_deriv<PTS, NM>, k_assemble_dense_shape_deriv<PTS, NM>
// for (15, 3), (31, 1) and (31, 3) and their launchers, the shape reading of assemble_dense_deriv_text.hpp, in their
// own translation unit.
#define EMME_DENSE_DERIV_SHAPE 1
#include "assemble_dense_deriv_text.hpp"
