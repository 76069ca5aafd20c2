// host_plan_deriv_selftest.cpp -- the fill planner (fill_plan.cpp) on derivative requests (FillShape::deriv, DESIGN.md
// 12): chunks of at most 8 omegas (K and K' of an omega are twin columns of the 16-column GEMM), the same halving below
// dense_min_tasks and the same dense_cost_ratio cut, never a wide chunk -- and the plans of plain requests beside them,
// which the flag must leave alone.  Built without device code and run under AddressSanitizer + UBSan by
// `make -C emme_amd/csrc host-sanitize`.
#include <cstdio>
#include <vector>

#include "fill_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                                 \
        }                                                                               \
    } while (0)

static emme::FillShape shape(int npoints, bool deriv) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = true, s.folded = true, s.nm = 1, s.gk_points = 15;
    s.npairs = npoints * (npoints - 1) / 2;
    s.deriv = deriv;
    return s;
}

struct Plan {
    emme::ChunkPlan plan;
    std::vector<int> ch;
    int size(int k) const { return ch[2 * k + 1]; }
    int first(int k) const { return ch[2 * k]; }
};

static Plan make(int npoints, bool deriv, const std::vector<unsigned long long>& cost, int n_wide,
                 const unsigned char* wide = nullptr) {
    Plan p;
    std::vector<int> order;
    const int n = (int)cost.size();
    const int nw = emme::plan_order(n, nullptr, cost.data(), wide, order);
    CHECK(nw == n_wide);
    p.plan = emme::plan_chunks(shape(npoints, deriv), order, cost.data(), n_wide, p.ch);
    // every plan: the chunks tile the order, and the position map behind them names chunk and column
    int q = 0;
    for (int k = 0; k < p.plan.nchunks; ++k) {
        CHECK(p.first(k) == q);
        CHECK(p.size(k) >= 1);
        q += p.size(k);
    }
    CHECK(q == n);
    CHECK((int)p.ch.size() == 2 * p.plan.nchunks + n);
    for (int k = 0; k < p.plan.nchunks; ++k)
        for (int w = 0; w < p.size(k); ++w) CHECK(p.ch[2 * p.plan.nchunks + p.first(k) + w] == ((k << 8) | w));
    return p;
}

int main() {
    const std::vector<unsigned long long> flat(128, 1000ull);
    {
        // the headline shape, 128 omegas of equal cost: 8 chunks of 16 plain, 16 chunks of 8 for a derivative request
        const Plan a = make(256, false, flat, 0), d = make(256, true, flat, 0);
        CHECK(a.plan.nchunks == 8);
        for (int k = 0; k < a.plan.nchunks; ++k) CHECK(a.size(k) == 16);
        CHECK(d.plan.nchunks == 16);
        for (int k = 0; k < d.plan.nchunks; ++k) CHECK(d.size(k) == 8);
        CHECK(a.plan.union_walk == d.plan.union_walk && a.plan.items_per_group == d.plan.items_per_group);
    }
    {
        // a short batch: one chunk either way (2040 tile tasks are enough)
        const std::vector<unsigned long long> four(4, 1000ull);
        const Plan a = make(256, false, four, 0), d = make(256, true, four, 0);
        CHECK(a.plan.nchunks == 1 && a.size(0) == 4);
        CHECK(d.plan.nchunks == 1 && d.size(0) == 4);
        const std::vector<unsigned long long> twelve(12, 1000ull);
        const Plan d12 = make(256, true, twelve, 0);
        CHECK(d12.plan.nchunks == 2 && d12.size(0) == 8 && d12.size(1) == 4);
        CHECK(make(256, false, twelve, 0).plan.nchunks == 1);
    }
    {
        // the halving below dense_min_tasks (2000): npoints 48 has 71 tiles; 128 omegas in chunks of 8 are 1136 tasks,
        // in chunks of 4 they are 2272 -- for the plain request 16 -> 8 -> 4 likewise
        const Plan a = make(48, false, flat, 0), d = make(48, true, flat, 0);
        CHECK(a.plan.nchunks == 32 && d.plan.nchunks == 32);
        for (int k = 0; k < 32; ++k) CHECK(a.size(k) == 4 && d.size(k) == 4);
        // ... and it stops at 2
        const std::vector<unsigned long long> eight(8, 1000ull);
        const Plan d8 = make(24, true, eight, 0);
        CHECK(d8.plan.nchunks == 4);
        for (int k = 0; k < 4; ++k) CHECK(d8.size(k) == 2);
    }
    {
        // the dense_cost_ratio cut (4): an omega of 10 x the typical cost ends up in a chunk of 2 (10 x 4 > 8 x 4 >= 10 x 2),
        // where the plain plan gives it a chunk of 4 (10 x 8 > 16 x 4 >= 10 x 4)
        std::vector<unsigned long long> cost = flat;
        cost[17] = 10000ull;
        const Plan a = make(256, false, cost, 0), d = make(256, true, cost, 0);
        CHECK(a.size(0) == 4 && a.size(1) == 16);
        CHECK(d.size(0) == 2 && d.size(1) == 8);
        for (int k = 0; k < d.plan.nchunks; ++k) CHECK(d.size(k) <= 8);
    }
    {
        // wide items (root search: omegas whose level lists overflowed): a chunk each in front for the plain request;
        // a derivative request has no wide-list build and plans them like every other omega
        std::vector<unsigned char> wide(128, 0);
        wide[5] = wide[99] = 1;
        const Plan a = make(256, false, flat, 2, wide.data()), d = make(256, true, flat, 2, wide.data());
        CHECK(a.size(0) == 1 && a.size(1) == 1 && a.size(2) == 16);
        CHECK(a.plan.nchunks == 2 + 8);  // (126 omegas: 7 chunks of 16 and one of 14)
        CHECK(d.plan.nchunks == 16);
        for (int k = 0; k < d.plan.nchunks; ++k) CHECK(d.size(k) == 8);
    }
    {
        // no omegas, no chunks
        const std::vector<int> none;
        std::vector<int> ch(3, 7);
        const emme::ChunkPlan p = emme::plan_chunks(shape(256, true), none, nullptr, 0, ch);
        CHECK(p.nchunks == 0 && ch.empty());
    }
    if (failures) {
        std::fprintf(stderr, "host_plan_deriv_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_plan_deriv_selftest ok\n");
    return 0;
}
