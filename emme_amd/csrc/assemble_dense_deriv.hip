// assemble_dense_deriv.hip -- M(omega) and the exact dM/domega from the tiled node cache for electrostatic GK15
// (DESIGN.md 12.1): k_btab_deriv, k_assemble_dense_deriv and their launchers, the electrostatic GK15 reading of
// assemble_dense_deriv_text.hpp, in their own translation unit, and the kernel that finishes the
// integrals they hand over.
#define EMME_DENSE_DERIV_SHAPE 0
#include "assemble_dense_deriv_text.hpp"

namespace emme {

namespace {

// ---- the integrals that left the cache ----------------------------------------------------------------------------
// DerivListArgs and k_assemble_deriv_list, the electrostatic GK15 reading of assemble_deriv_list_text.hpp: a lane group
// per work-list entry (batch << 32 | pair), from scratch, M and M' of the integral.
#define EMME_DERIV_LIST_SHAPE 0
#include "assemble_deriv_list_text.hpp"

}  // namespace

hipError_t launch_assemble_deriv_list(const AssembleLaunch& L, const unsigned long long* worklist,
                                      const unsigned int* count, hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || !L.Md) return hipErrorInvalidValue;
    DerivListArgs A;
    A.P = L.P;
    A.tab = L.tab;
    A.pairs = (const ushort2*)L.pairs;
    A.omega = (const double2*)L.omega;
    A.M = (double2*)L.M;
    A.Md = (double2*)L.Md;
    A.intervals = L.intervals;
    A.status = L.status;
    A.worklist = worklist;
    A.worklist_count = count;
    A.skip_lost = L.skip_lost;
    const size_t lds = tables_stack_lds_bytes(L.P.N, 16);
    // (the list length is on the device: a fixed grid strides over it, workgroups without a share return at once)
    hipLaunchKernelGGL(k_assemble_deriv_list, dim3(2048), dim3(256), lds, stream, A);
    return hipGetLastError();
}

}  // namespace emme
