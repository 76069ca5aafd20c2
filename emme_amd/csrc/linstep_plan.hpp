// linstep_plan.hpp -- how many workgroups each matrix of a blocked LU launch gets, decided from host data alone
// (plain C++, no HIP).  trace_solve (ctx_linstep.hip) launches with it; host_selftest.cpp pins the choices.
#pragma once
#include <algorithm>

namespace emme {

// n: order; n_live: matrices of the launch (>= 1); n_cu: compute units; lu_split: the option (k > 0 pins k, 1 = one
// workgroup per matrix); lu_one_wg: a hand-over timed out once on this context; fits: the whole L21 panel fits one
// workgroup's LDS (otherwise the chunked build runs, which needs helper workgroups)
inline int lu_workgroups(int n, int n_live, int n_cu, int lu_split, bool lu_one_wg, bool fits) {
    if (lu_one_wg) return 1;
    int nwg = 1;
    if (lu_split > 0) {
        nwg = std::min(lu_split, 16);
    } else if (n >= 128) {
        // every workgroup of a matrix must be resident at once (they wait for each other):
        // never more workgroups than compute units.  Below n = 128 the hand-over costs more
        // than the idle units are worth, and beyond 8 the factoring workgroup is the limit.
        // (n = 256: four are enough, role 0 is the limit then; n = 512: two A-helpers pay)
        nwg = std::max(1, std::min(n >= 768 ? 16 : (n >= 384 ? 8 : 4), n_cu / n_live));
    }
    if (!fits && nwg < 2 && lu_split != 1) nwg = 2;  // (the chunked build needs two)
    return nwg;
}

}  // namespace emme
