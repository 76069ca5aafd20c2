// fill_plan.cpp -- the host arithmetic of the fill dispatcher (fill_plan.hpp); DESIGN.md 5.0 has the measurements
// behind the constants.
#include "fill_plan.hpp"

#include <algorithm>

namespace emme {

int plan_order(int nbatch, const int* host_active, const unsigned long long* cost, const unsigned char* wide,
               std::vector<int>& order) {
    order.clear();
    for (int b = 0; b < nbatch; ++b)
        if (!host_active || host_active[b] != 0) order.push_back(b);
    if (cost) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    int n_wide = 0;
    if (wide) {
        std::stable_partition(order.begin(), order.end(), [&](int b) { return wide[b] != 0; });
        for (int b : order) n_wide += wide[b] != 0;
    }
    return n_wide;
}

// A contour class that holds only a few of the call's omegas and has no cache yet does not get one for their
// sake: its main part costs as much to build as for a full batch (N = 512: 32 ms, and another 32 for the first
// subtree), while those few omegas cost 0.7 ms each through the uncached kernel -- a context that lives for
// one root search (BASELINE configs[4]: a fresh one per k_rho, one or two of 32 chains on the Re omega > 0
// side) never earns it back.  Once the class is more than a sixteenth of the batch its cache is built.
ClassCensus plan_classes(const std::vector<int>& order, const double* host_omega, const bool has_cache[2]) {
    ClassCensus cs;
    for (int b : order) ++cs.count[contour_class(host_omega[2 * b])];
    const int n_act = (int)order.size();
    for (int k = 0; k < 2 && cs.minority < 0; ++k)
        if (cs.count[0] > 0 && cs.count[1] > 0 && !has_cache[k] && cs.count[k] * 16 <= n_act &&
            cs.count[k] < cs.count[1 - k])
            cs.minority = k;
    return cs;
}

int items_per_group_for(const FillShape& s, long units) {
    // enough lane groups to give every SIMD several waves, but a few integrals per group
    // when the batch is large so the start-up cost (table staging) is amortised
    const long total = (long)s.npairs * s.nm * units;
    const long target_groups = 256L * 16 * (64 / s.lane_group()) * 4;
    return (int)std::min(std::max(total / target_groups, 1L), 8L);
}

ChunkPlan plan_chunks(const FillShape& s, const std::vector<int>& order, const unsigned long long* cost, int n_wide,
                      std::vector<int>& ch) {
    ChunkPlan plan;
    const int gw = s.lane_group();
    // the union-walk kernel (electrostatic GK15 on folded records, assemble_cached.hip): lanes
    // that sit a round out cost little there, so its chunks are always full and each group
    // takes three items (measured optimum: 86.5 ms vs 104 with the policy below)
    plan.union_walk = (!s.fill_lanes || s.tiled) && s.folded && s.nm == 1 && s.gk_points == 15;
    // Omega chunks of unequal size.  Every lane walks ONE omega's trees, so an
    // omega whose integrals need 3x the intervals keeps its lane busy 3x longer than its
    // neighbours'.  A chunk of n omegas gives each of them gw/n lanes per group: expensive
    // omegas go into small chunks, cheap ones share a chunk 16 (32) at a time.  The order is
    // sorted by cost, most expensive first, so chunk capacities only grow along the list.
    ch.clear();
    if (!order.empty()) {
        std::vector<unsigned long long> cs;
        for (int b : order) cs.push_back(cost ? cost[b] : 1ull);
        std::vector<unsigned long long> sorted = cs;
        std::sort(sorted.begin(), sorted.end());
        const double typical = (double)std::max<unsigned long long>(sorted[sorted.size() / 2], 1ull);
        // dense fill: one wave walks a (16-pair tile, chunk) serially, so (a) a chunk of omegas whose
        // trees do not overlap costs the SUM of their walks in one wave -- expensive omegas get narrow
        // chunks like in the independent-lane kernels -- and (b) a launch needs several times more
        // tile tasks than the chip holds waves: the widest chunk shrinks until there are at least
        // EMME_DENSE_MIN_TASKS (2000; 8000 while every lane ended with a global atomic -- with the counters
        // summed per workgroup 0 .. 3000 are equal, 44.7 ms of fill per bench search, and 8000 costs 45.8)
        // (dense fill: a chunk is 16 COLUMNS -- 16 omegas, or 5 omegas x 3 moments)
        // (a derivative request, s.deriv: K and K' of a column are twin columns -- 8 K columns: 8 omegas, or 2 omegas
        // x 3 moments)
        const int tile_cap = (s.deriv ? 8 : 16) / s.nm;
        int dense_cap = s.tiled ? tile_cap : gw;
        if (s.tiled) {
            const long ntiles = (s.npairs + 15) / 16;
            const long min_tasks = s.dense_min_tasks;
            while (dense_cap > 2 && ((long)order.size() + dense_cap - 1) / dense_cap * ntiles < min_tasks) dense_cap >>= 1;
        }
        size_t q = 0;
        for (; !s.deriv && q < (size_t)n_wide; ++q) ch.push_back((int)q), ch.push_back(1);
        while (q < order.size()) {
            int cap = s.tiled ? dense_cap : gw;
            while ((!plan.union_walk || s.tiled) && cap > (s.tiled ? 2 : 1) &&
                   (double)cs[q] * cap > typical * (s.tiled ? tile_cap * s.dense_cost_ratio : gw * 1.5))
                cap >>= 1;
            const int n = (int)std::min<size_t>((size_t)cap, order.size() - q);
            ch.push_back((int)q);
            ch.push_back(n);
            q += (size_t)n;
        }
    }
    plan.nchunks = (int)ch.size() / 2;
    if (s.tiled) {
        ch.resize(ch.size() + order.size());
        int* map = ch.data() + 2 * plan.nchunks;
        for (int k = 0; k < plan.nchunks; ++k)
            for (int w = 0; w < ch[2 * k + 1]; ++w) map[ch[2 * k] + w] = (k << 8) | w;
    }
    // up to three chunks (late Newton steps: <= 48 omegas) leave the SIMDs short of waves
    // with three items per group: two then (measured: one is worse again -- every
    // workgroup stages the grid tables; EMME_UNION_IPG_FEW / EMME_UNION_FEW_CHUNKS)
    if (!plan.union_walk)
        plan.items_per_group = items_per_group_for(s, plan.nchunks > 0 ? plan.nchunks : 1);
    else
        plan.items_per_group = plan.nchunks <= s.union_few_chunks ? std::max(1, s.union_ipg_few) : 3;
    return plan;
}

ChunkPlan plan_tile_chunks(const FillShape& s, std::vector<int>& order, const double* host_omega,
                           const unsigned long long* cost, std::vector<int>& ch, const int* host_set) {
    ChunkPlan plan;
    ch.clear();
    if (order.empty()) return plan;
    // group by group -- (parameter set, contour class), or the class alone without host_set; inside a group the order
    // plan_order made (most expensive first where costs are given)
    auto group_of = [&](int b) { return 2L * (host_set ? host_set[b] : 0) + contour_class(host_omega[2 * b]); };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return group_of(a) < group_of(b); });
    const size_t n = order.size();
    std::vector<size_t> ends;  // one past the last position of every group
    for (size_t q = 1; q <= n; ++q)
        if (q == n || group_of(order[q]) != group_of(order[q - 1])) ends.push_back(q);
    std::vector<unsigned long long> cs;
    for (int b : order) cs.push_back(cost ? cost[b] : 1ull);
    std::vector<unsigned long long> sorted = cs;
    std::sort(sorted.begin(), sorted.end());
    const double typical = (double)std::max<unsigned long long>(sorted[n / 2], 1ull);
    // one wave walks a (16-pair tile, chunk) serially and a launch needs several times more tile tasks than the chip
    // holds waves: the widest chunk shrinks until there are dense_min_tasks of them (plan_chunks)
    // (a chunk is 16 COLUMNS -- 16 omegas, or 5 omegas x 3 moments: plan_chunks)
    const int tile_cap = 16 / s.nm;
    int cap_all = tile_cap;
    const long ntiles = (s.npairs + 15) / 16;
    auto chunks_at = [&](int cap) {
        long k = 0;
        size_t first = 0;
        for (size_t end : ends) k += (long)((end - first + cap - 1) / cap), first = end;
        return k;
    };
    while (cap_all > 2 && chunks_at(cap_all) * ntiles < (long)s.dense_min_tasks) cap_all >>= 1;
    // an omega that costs dense_cost_ratio times the typical one gets a narrow chunk: its trees overlap nobody's
    struct Chunk {
        int first, size;
        unsigned long long cost;
    };
    std::vector<Chunk> cut;
    size_t g = 0;
    for (size_t q = 0; q < n;) {
        while (ends[g] <= q) ++g;
        const size_t end = ends[g];  // a chunk ends where its group does
        int cap = cap_all;
        while (cap > 2 && (double)cs[q] * cap > typical * (tile_cap * s.dense_cost_ratio)) cap >>= 1;
        const int m = (int)std::min<size_t>((size_t)cap, end - q);
        cut.push_back({(int)q, m, cs[q]});
        q += (size_t)m;
    }
    // chunk-major launch order: the most expensive chunk first (its tasks are the longest)
    std::stable_sort(cut.begin(), cut.end(), [](const Chunk& a, const Chunk& b) { return a.cost > b.cost; });
    for (const Chunk& k : cut) ch.push_back(k.first), ch.push_back(k.size);
    plan.nchunks = (int)cut.size();
    ch.resize(ch.size() + n);
    int* map = ch.data() + 2 * plan.nchunks;
    for (int k = 0; k < plan.nchunks; ++k)
        for (int w = 0; w < ch[2 * k + 1]; ++w) map[ch[2 * k] + w] = (k << 8) | w;
    plan.union_walk = true;
    plan.items_per_group = 1;
    return plan;
}

}  // namespace emme
