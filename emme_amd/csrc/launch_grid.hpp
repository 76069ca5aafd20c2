// launch_grid.hpp -- host arithmetic that the launchers of the lane-group fills share: the grid's x extent and the
// dynamic LDS of "tables + one interval stack per lane group".  Host only; the kernels compute their own offsets.
#pragma once
#include <cstddef>

#include "assemble_common.hpp"

namespace emme {

// x extent of a grid whose lane groups take about `items_per_group` of the `nitems` work items each, `groups_per_block`
// groups to a workgroup: that keeps the tail short without starving the chip when the batch is small
inline unsigned lane_group_grid_x(long nitems, int items_per_group, int groups_per_block) {
    long want_groups = (nitems + items_per_group - 1) / items_per_group;
    long gx = (want_groups + groups_per_block - 1) / groups_per_block;
    if (gx < 1) gx = 1;
    if (gx > 65535) gx = 65535;
    return (unsigned)gx;
}

// x extent of a dense fill's grid: one workgroup per (group of 4 tiles, omega chunk).  xcd_grouped: the tile groups are
// rounded up to a multiple of the eight XCDs, so that workgroup id & 7 names the XCD whose L2 a tile group's chunks share
// (DESIGN.md 5.1c); the kernel returns at once for the tile groups past the last one
inline unsigned dense_tile_grid_x(int ntiles, int nchunks, bool xcd_grouped) {
    const long ntg = (ntiles + 3) / 4;
    return (unsigned)((xcd_grouped ? (ntg + 7) / 8 * 8 : ntg) * nchunks);
}

// bytes of the eta | g | b tables of an N-point lattice, padded to a double2 boundary
inline size_t tables_lds_bytes(int N) { return ((size_t)3 * N + (3 * N & 1)) * sizeof(double); }

// the tables plus, per lane group, the (mid, r) stack of a depth-first walk down to EMME_MAX_DEPTH
inline size_t tables_stack_lds_bytes(int N, int groups_per_block) {
    return tables_lds_bytes(N) + (size_t)groups_per_block * EMME_MAX_DEPTH * sizeof(double2);
}

}  // namespace emme
