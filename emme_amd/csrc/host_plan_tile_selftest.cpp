// host_plan_tile_selftest.cpp -- the chunk plan of the table-free tile fill (fill_plan.cpp: plan_tile_chunks, DESIGN.md
// 5.3b): chunks of at most 16 omegas that never mix contour classes, the dense_min_tasks halving, the dense_cost_ratio
// cut, the most expensive chunk first.  Built without device code and run under AddressSanitizer + UBSan by
// `make -C emme_amd/csrc host-sanitize`.
#include <algorithm>
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

static emme::FillShape shape(int npoints) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = true, s.folded = true, s.nm = 1, s.gk_points = 15;
    s.npairs = npoints * (npoints - 1) / 2;
    return s;
}

struct Plan {
    emme::ChunkPlan plan;
    std::vector<int> order, ch;
    int size(int k) const { return ch[2 * k + 1]; }
    int first(int k) const { return ch[2 * k]; }
};

// re[b]: Re omega_b; cost may be empty
static Plan make(int npoints, const std::vector<double>& re, const std::vector<unsigned long long>& cost,
                 const int* active = nullptr) {
    Plan p;
    const int n = (int)re.size();
    std::vector<double> om(2 * n, 0.25);
    for (int b = 0; b < n; ++b) om[2 * b] = re[b];
    const unsigned long long* cs = cost.empty() ? nullptr : cost.data();
    emme::plan_order(n, active, cs, nullptr, p.order);
    const std::vector<int> before = p.order;
    p.plan = emme::plan_tile_chunks(shape(npoints), p.order, om.data(), cs, p.ch);
    const int m = (int)p.order.size();
    // the order is a regrouping of what plan_order made, and inside a class it keeps that order
    {
        std::vector<int> a = before, b = p.order;
        std::sort(a.begin(), a.end()), std::sort(b.begin(), b.end());
        CHECK(a == b);
        for (int cls = 0; cls < 2; ++cls) {
            std::vector<int> x, y;
            for (int v : before)
                if (emme::contour_class(re[v]) == cls) x.push_back(v);
            for (int v : p.order)
                if (emme::contour_class(re[v]) == cls) y.push_back(v);
            CHECK(x == y);
        }
    }
    // the chunks cover every position once, hold 1 .. 16 omegas of ONE class, and the map behind them names chunk and column
    std::vector<int> seen(m, 0);
    CHECK((int)p.ch.size() == 2 * p.plan.nchunks + m);
    for (int k = 0; k < p.plan.nchunks; ++k) {
        CHECK(p.size(k) >= 1 && p.size(k) <= 16);
        CHECK(p.first(k) >= 0 && p.first(k) + p.size(k) <= m);
        for (int w = 0; w < p.size(k); ++w) {
            const int pos = p.first(k) + w;
            ++seen[pos];
            CHECK(emme::contour_class(re[p.order[pos]]) == emme::contour_class(re[p.order[p.first(k)]]));
            CHECK(p.ch[2 * p.plan.nchunks + pos] == ((k << 8) | w));
        }
    }
    for (int v : seen) CHECK(v == 1);
    // the most expensive chunk first
    if (cs)
        for (int k = 1; k < p.plan.nchunks; ++k) CHECK(cs[p.order[p.first(k - 1)]] >= cs[p.order[p.first(k)]]);
    return p;
}

int main() {
    {
        // both classes interleaved in the order: 40 omegas, every other one on the Re omega > 0 side
        std::vector<double> re(40);
        for (int b = 0; b < 40; ++b) re[b] = (b & 1) ? 0.5 : -0.5;
        const Plan p = make(256, re, {});
        CHECK(p.plan.nchunks == 4);  // 20 per class: 16 + 4 each
        int sizes[2][2] = {{0, 0}, {0, 0}};
        for (int k = 0; k < 4; ++k) ++sizes[emme::contour_class(re[p.order[p.first(k)]])][p.size(k) == 16 ? 0 : 1];
        CHECK(sizes[0][0] == 1 && sizes[0][1] == 1 && sizes[1][0] == 1 && sizes[1][1] == 1);
        // with costs, interleaved too
        std::vector<unsigned long long> cost(40);
        for (int b = 0; b < 40; ++b) cost[b] = 1000ull + (unsigned long long)((b * 7) % 40);
        make(256, re, cost);
    }
    {
        // one omega: one chunk of one, either class
        const Plan a = make(256, {-0.8}, {}), b = make(256, {0.6}, {}), z = make(256, {0.0}, {});
        CHECK(a.plan.nchunks == 1 && a.size(0) == 1 && a.first(0) == 0);
        CHECK(b.plan.nchunks == 1 && b.size(0) == 1);
        CHECK(z.plan.nchunks == 1 && z.size(0) == 1);
        // one grid point pair (npoints 2): still one chunk (the halving stops at 2 and never makes an empty chunk)
        const Plan c = make(2, {-0.8}, {});
        CHECK(c.plan.nchunks == 1 && c.size(0) == 1);
    }
    {
        // 17 omegas of one class: 16 + 1 on the headline grid (2040 tiles: 2 chunks are enough tasks)
        const Plan p = make(256, std::vector<double>(17, -0.3), {});
        CHECK(p.plan.nchunks == 2 && p.size(0) == 16 && p.size(1) == 1 && p.first(1) == 16);
        // an empty class beside it: nothing of class 1 appears
        for (int k = 0; k < p.plan.nchunks; ++k) CHECK(emme::contour_class(-0.3) == 0);
        // the other class empty
        const Plan q = make(256, std::vector<double>(17, 0.3), {});
        CHECK(q.plan.nchunks == 2 && q.size(0) == 16 && q.size(1) == 1);
    }
    {
        // the halving below dense_min_tasks (2000): npoints 48 has 71 tiles; 128 omegas of one class in chunks of 16 are
        // 568 tasks, of 8 1136, of 4 2272
        const Plan p = make(48, std::vector<double>(128, -0.3), {});
        CHECK(p.plan.nchunks == 32);
        for (int k = 0; k < 32; ++k) CHECK(p.size(k) == 4);
        // ... and it stops at 2
        const Plan q = make(24, std::vector<double>(8, -0.3), {});
        CHECK(q.plan.nchunks == 4);
        for (int k = 0; k < 4; ++k) CHECK(q.size(k) == 2);
    }
    {
        // costs spanning the ratio cut (4): an omega of 10 x the typical cost gets a chunk of 4 (10 x 8 > 16 x 4 >= 10 x 4),
        // and it is the first chunk of the launch; the cut is taken per class
        std::vector<unsigned long long> cost(128, 1000ull);
        cost[17] = 10000ull;
        std::vector<double> re(128, -0.3);
        const Plan p = make(256, re, cost);
        CHECK(p.order[0] == 17 && p.first(0) == 0 && p.size(0) == 4 && p.size(1) == 16);
        for (int b = 64; b < 128; ++b) re[b] = 0.3;
        cost[100] = 10000ull;
        const Plan q = make(256, re, cost);
        CHECK(q.size(0) == 4 && q.size(1) == 4);
        CHECK(q.order[q.first(0)] == 17 && q.order[q.first(1)] == 100);
        // a cost 100 x the typical: the cut stops at chunks of 2
        cost[17] = 100000ull;
        CHECK(make(256, re, cost).size(0) == 2);
    }
    {
        // an active mask: only the marked items are planned
        std::vector<int> active(32, 0);
        for (int b = 0; b < 32; b += 3) active[b] = 1;
        std::vector<double> re(32);
        for (int b = 0; b < 32; ++b) re[b] = (b % 2) ? 0.4 : -0.4;
        const Plan p = make(256, re, {}, active.data());
        CHECK((int)p.order.size() == 11);
        CHECK(p.plan.nchunks == 2);
    }
    {
        // no omegas, no chunks
        std::vector<int> none, ch(3, 7);
        const double om[2] = {0.0, 0.0};
        const emme::ChunkPlan p = emme::plan_tile_chunks(shape(256), none, om, nullptr, ch);
        CHECK(p.nchunks == 0 && ch.empty());
    }
    if (failures) {
        std::fprintf(stderr, "host_plan_tile_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_plan_tile_selftest ok\n");
    return 0;
}
