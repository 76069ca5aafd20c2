// fold_combine.hpp -- what the two folded steps' kernels (linstep_fold.hip; eigpair_fold.hip, DESIGN.md
// 14.2) say the same way: which half problem a workgroup has, how the two halves' codes make the chain's, and the 2 x 2
// matrix of the rank-2 correction.  Device code.
#pragma once
#include "tri_solve.hpp"

namespace emme {
namespace fold {

// Half problem h = 2b + s of chain b: s = 0 the even (+) block, s = 1 the odd (-) one.  sgn: e+ = e_0, e- = -e_0, the
// folds of e_{n-1}; u, ud: the folds u_s and u'_s of the chain's edge vectors (edges [nbatch][4][m]: u+, u-, u'+, u'-)
struct Half {
    int b;
    double sgn;
    const double2 *u, *ud;
    __device__ __forceinline__ Half(int h, const double2* edges, int m)
        : b(h >> 1), sgn((h & 1) ? -1.0 : 1.0), u(edges + ((size_t)(h >> 1) * 4 + (h & 1)) * m), ud(u + 2 * (size_t)m) {}
};

// the chain's code from its halves' (0, the column at which a factorisation stopped, or a negative code): the even
// half's first; a column of the odd half counts from m
__device__ __forceinline__ int merge_half_info(int even, int odd, int m) {
    return even != 0 ? even : odd > 0 ? odd + m : odd;
}

// K = I + [[e.a, e.b], [u.a, u.b]] and its determinant; ok: det K is finite and not zero
struct WoodburyK {
    cd k11, k12, k21, k22, det;
    bool ok;
    __device__ __forceinline__ WoodburyK(cd ea, cd eb, cd ua, cd ub)
        : k11(mk(1.0, 0.0) + ea), k12(eb), k21(ua), k22(mk(1.0, 0.0) + ub) {
        det = k11 * k22 - k12 * k21;
        ok = (det.x != 0.0 || det.y != 0.0) && isfinite(det.x) && isfinite(det.y);
    }
};

// q-th sum of a chain from its halves' (pp, pm: the even and the odd half's): a bilinear form of two unnormalised folds
// is twice the form of the vectors
__device__ __forceinline__ cd both(const double2* pp, const double2* pm, int q) {
    return 0.5 * (trisolve::ld2(&pp[q]) + trisolve::ld2(&pm[q]));
}

}  // namespace fold
}  // namespace emme
