// assemble_wl.hip -- batched fill, "omega-lane" form: the kernel of choice when several
// omega candidates are assembled for the same parameter set (the root-search batch).
//
// Observation (emme_device.hpp::node_data): for a fixed pair (i,j), moment m and contour
// sense, the integrand at a quadrature node is  exp(A0 + T w)(w Q1 + Q0)  where A0, T, Q1, Q0
// do not depend on omega -- and they contain everything expensive (the Miller recurrence for
// I0/I1, sincos of the abscissa, two rsqrt).  The reference recomputes all of it for every
// omega (src/Parameters.cpp:113-184 is called once per matrix entry per omega).
//
// Mapping.  A lane group of GW = 16 (GK15) / 32 (GK31) lanes owns one (pair, moment) item and
// GW omegas of the batch at a time, and alternates two phases per quadrature interval:
//   phase 1  lane = node : lane r evaluates the omega-independent NodeData of node r and
//            parks it in LDS (64 B per node);
//   phase 2  lane = omega: every lane walks the 15 (31) nodes in the reference's summation
//            order, finishing F with its own omega (one complex exp + three complex products
//            per node), and accumulates its private Kronrod / Gauss sums -- no cross-lane
//            reduction, and the accept/split decision is per lane.
// Each omega keeps its own adaptive tree (same decisions as the reference); the group walks
// the UNION of the trees depth-first: an interval is evaluated when at least one lane's next
// node is that interval, and lanes whose tree does not contain it sit the round out.
//
// The kernels themselves, k_assemble_wl<PTS> and k_assemble_wl_deriv<PTS> (M' alongside), are the two readings of
// assemble_wl_text.hpp; this file holds what both take (the argument struct) and the launcher.
#include <hip/hip_runtime.h>

#include "assemble_common.hpp"
#include "launch.hpp"
#include "launch_grid.hpp"

namespace emme {

namespace {

struct AsmWlArgs {
    DevParams P;
    const double* tab;     // eta[N] | g[N] | b[N]
    const ushort2* pairs;  // (i, j), i < j, ordered by j - i
    int npairs;
    const int* act_idx;    // [n_act] batch index of every omega handled by this launch
    int n_act;
    const double2* omega;  // [nbatch]
    double2* M;            // [nbatch][dim][dim]
    const double2* Mold;   // null, or [nbatch][dim][dim] -> also write Mp = (M - Mold)/domega
    double2* Mp;
    const double2* domega;
    unsigned long long* intervals;  // [nbatch]
    int* status;                    // [nbatch]
    unsigned long long* rounds;     // [1] interval rounds walked by all groups (diagnostic)
};

#ifndef EMME_WL_MIN_WAVES
#define EMME_WL_MIN_WAVES 3
#endif

#define EMME_WL_DERIV 0  // k_assemble_wl
#include "assemble_wl_text.hpp"
#undef EMME_WL_DERIV
#define EMME_WL_DERIV 1  // k_assemble_wl_deriv
#include "assemble_wl_text.hpp"
#undef EMME_WL_DERIV

}  // namespace

hipError_t launch_assemble_wl(const AssembleLaunch& L, const int* act_idx, int n_act,
                              hipStream_t stream) {
    AsmWlArgs A;
    A.P = L.P;
    A.tab = L.tab;
    A.pairs = (const ushort2*)L.pairs;
    A.npairs = L.npairs;
    A.act_idx = act_idx;
    A.n_act = n_act;
    A.omega = (const double2*)L.omega;
    A.M = (double2*)L.M;
    A.Mold = (const double2*)L.Mold;
    A.Mp = (double2*)L.Mp;
    A.domega = (const double2*)L.domega;
    A.intervals = L.intervals;
    A.status = L.status;
    A.rounds = L.rounds;
    const int gw = L.gk_points == 15 ? 16 : 32;
    const int groups_per_block = 256 / gw;
    const int chunks = (n_act + gw - 1) / gw;
    const long nitems = (long)L.npairs * L.P.nm;
    dim3 grid(lane_group_grid_x(nitems, L.items_per_group, groups_per_block), (unsigned)chunks), block(256);
    // the tables and stacks, then 4 double2 of node data per lane
    const size_t lds = tables_stack_lds_bytes(L.P.N, groups_per_block) + (size_t)256 * 4 * sizeof(double2);
    if (L.Md) {
        if (L.Mold) return hipErrorInvalidValue;  // (the derivative fill has no fused secant)
        if (L.gk_points == 15)
            hipLaunchKernelGGL(k_assemble_wl_deriv<15>, grid, block, lds, stream, A, (double2*)L.Md);
        else
            hipLaunchKernelGGL(k_assemble_wl_deriv<31>, grid, block, lds, stream, A, (double2*)L.Md);
    } else if (L.gk_points == 15)
        hipLaunchKernelGGL(k_assemble_wl<15>, grid, block, lds, stream, A);
    else
        hipLaunchKernelGGL(k_assemble_wl<31>, grid, block, lds, stream, A);
    return hipGetLastError();
}

}  // namespace emme
