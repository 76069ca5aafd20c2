// assemble_tile_shape_deriv.hip -- M(omega) and the exact dM/domega from one table-free tile fill for electromagnetic
// contexts and the 31-point rule: k_assemble_tile_shape_deriv<PTS, NM> and
// launch_assemble_tile_shape_deriv, the derivative shape reading of assemble_tile_text.hpp, in their own translation
// unit, and the kernel that finishes the integrals they hand over.
#define EMME_TILE_SHAPE 1
#define EMME_TILE_SETS 0
#define EMME_TILE_DERIV 1
#include "assemble_tile_text.hpp"
#include "launch_grid.hpp"

namespace emme {

namespace {

// ---- the integrals that kernel handed over --------------------------------------------------------------------------
// DerivListShapeArgs and k_assemble_deriv_list_shape<PTS>, the shape reading of assemble_deriv_list_text.hpp: a lane
// group of 16 (GK15) or 32 (GK31) lanes per work-list entry (batch << 32 | pair nm + moment), from scratch, M and M' of
// the integral, every moment's scatter.
#define EMME_DERIV_LIST_SHAPE 1
#include "assemble_deriv_list_text.hpp"

}  // namespace

hipError_t launch_assemble_deriv_list_shape(const AssembleLaunch& L, const unsigned long long* worklist,
                                            const unsigned int* count, hipStream_t stream) {
    if ((L.gk_points != 15 && L.gk_points != 31) || !L.Md) return hipErrorInvalidValue;
    DerivListShapeArgs A;
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
    const size_t lds = tables_stack_lds_bytes(L.P.N, L.gk_points == 15 ? 16 : 8);
    // (the list length is on the device: a fixed grid strides over it, workgroups without a share return at once)
    if (L.gk_points == 15)
        hipLaunchKernelGGL(k_assemble_deriv_list_shape<15>, dim3(2048), dim3(256), lds, stream, A);
    else
        hipLaunchKernelGGL(k_assemble_deriv_list_shape<31>, dim3(2048), dim3(256), lds, stream, A);
    return hipGetLastError();
}

}  // namespace emme
