// fill_plan.hpp -- what one fill launches, decided from host data alone (plain C++, no HIP): the omega order, the
// contour classes, the omega chunks of the cached kernels and the integrals per lane group.  ctx_fill.hip turns a
// plan into launches; host_selftest.cpp pins the plans of the shapes DESIGN.md 5.0 was tuned on.
#pragma once
#include <cmath>
#include <vector>

namespace emme {

// the context facts and option values (emme_options_t) a plan depends on
struct FillShape {
    bool tiled = false, folded = true;
    int nm = 1, gk_points = 15, npairs = 0;
    bool fill_lanes = false;  // fill option EMME_FILL_LANES: independent lanes instead of the union walk
    int dense_min_tasks = 2000;
    double dense_cost_ratio = 4.0;
    int union_ipg_few = 2, union_few_chunks = 3;
    bool deriv = false;  // a derivative request on the tiled cache: twin columns, so a chunk holds 8 / nm omegas, never wide
    int lane_group() const { return gk_points == 15 ? 16 : 32; }
};

// contour class of an omega: 0 for Re omega < 0 (omi = +1), 1 otherwise
inline int contour_class(double re_omega) { return -std::copysign(1.0, re_omega) > 0.0 ? 0 : 1; }

// order <- the items host_active marks (null = all), most expensive first if cost is given (stable; items that
// share a lane group walk the union of their quadrature trees, so neighbours should cost alike), then the items
// wide marks (null = none) moved to the front.  Returns how many those are.
int plan_order(int nbatch, const int* host_active, const unsigned long long* cost, const unsigned char* wide,
               std::vector<int>& order);

// omegas per contour class, and the class (-1: none) that holds so few of them -- at most a sixteenth, and fewer
// than the other -- that it is not worth a node cache it does not have yet
struct ClassCensus {
    int count[2] = {0, 0};
    int minority = -1;
};
ClassCensus plan_classes(const std::vector<int>& order, const double* host_omega, const bool has_cache[2]);

// integrals per lane group of a launch of `units` lane-group columns
int items_per_group_for(const FillShape& s, long units);

// The cached fill's omega chunks over an order that plan_order made: chunks <- (first position, size) per chunk
// and, for the dense fill (s.tiled), behind them position -> (chunk << 8 | column).  The first n_wide positions
// get a chunk each (none of them for a derivative request, s.deriv: it has no wide-list build).
struct ChunkPlan {
    bool union_walk = false;  // the union-walk kernel's policy: full chunks, three items per group
    int nchunks = 0;
    int items_per_group = 1;
};
ChunkPlan plan_chunks(const FillShape& s, const std::vector<int>& order, const unsigned long long* cost, int n_wide,
                      std::vector<int>& chunks);

// The tile fill's omega chunks (assemble_tile.hip: one wave builds the phase block of ONE contour class per interval).
// `order` (from plan_order) is regrouped -- class by class, each class keeping its order -- and cut into chunks of
// <= 16 omegas that never mix contour classes (contour_class(host_omega[2 b])): the dense_min_tasks halving on the
// launch's chunk count, the dense_cost_ratio cut where costs are given.  chunks <- the dense fill's table, (first
// position, size) per chunk with the most expensive chunk first, and behind it position -> (chunk << 8 | column).
// host_set given (a fill over parameter sets, DESIGN.md 13.7: item b belongs to set host_set[b]): the groups are the
// (set, contour class) pairs, in ascending order of the set, and a chunk mixes neither sets nor classes.
ChunkPlan plan_tile_chunks(const FillShape& s, std::vector<int>& order, const double* host_omega,
                           const unsigned long long* cost, std::vector<int>& chunks, const int* host_set = nullptr);

}  // namespace emme
