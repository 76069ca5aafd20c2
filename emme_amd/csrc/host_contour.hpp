// host_contour.hpp -- the host arithmetic of the contour eigensolver (host_contour.cpp, plain C++): what
// emme_find_roots_in_contour (contour.hip) uses besides the C ABI's emme_contour_eigs.
#pragma once

namespace emme {

// Winding number of det M along a closed contour from arg det M at its nodes, in contour order (args[j] at t_j,
// N >= 2, any branch of the angle): W = sum_j wrap(arg_{j+1} - arg_j) / 2 pi, the last difference closing the
// curve.  *resolved = every |wrapped step| <= max_step and |W - round W| <= 0.05.  Returns round(W).
int contour_winding(const double* args, int N, double max_step, bool* resolved, double* W_raw);

}  // namespace emme
