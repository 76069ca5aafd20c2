// host_plan_tile_sets_selftest.cpp -- the chunk plan of the table-free tile fill over parameter sets (fill_plan.cpp:
// plan_tile_chunks with host_set): the order regrouped by (set, contour class), each group keeping the
// order plan_order made; chunks of at most 16 omegas that mix neither sets nor classes; the dense_min_tasks halving on
// the launch's total chunk count; the dense_cost_ratio cut; the most expensive chunk first.  Built without device code
// and run under AddressSanitizer + UBSan by `make -C emme_amd/csrc host-sanitize`.
#include <algorithm>
#include <cstdio>
#include <utility>
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

static emme::FillShape shape(int npoints, int dense_min_tasks = 2000) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = true, s.folded = true, s.nm = 1, s.gk_points = 15;
    s.npairs = npoints * (npoints - 1) / 2;
    s.dense_min_tasks = dense_min_tasks;
    return s;
}

struct Plan {
    emme::ChunkPlan plan;
    std::vector<int> order, ch;
    int size(int k) const { return ch[2 * k + 1]; }
    int first(int k) const { return ch[2 * k]; }
};

// re[b]: Re omega_b, set[b]: its parameter set; cost may be empty
static Plan make(const emme::FillShape& s, const std::vector<double>& re, const std::vector<int>& set,
                 const std::vector<unsigned long long>& cost, const int* active = nullptr) {
    Plan p;
    const int n = (int)re.size();
    std::vector<double> om(2 * n, 0.25);
    for (int b = 0; b < n; ++b) om[2 * b] = re[b];
    const unsigned long long* cs = cost.empty() ? nullptr : cost.data();
    emme::plan_order(n, active, cs, nullptr, p.order);
    const std::vector<int> before = p.order;
    p.plan = emme::plan_tile_chunks(s, p.order, om.data(), cs, p.ch, set.data());
    const int m = (int)p.order.size();
    auto group = [&](int b) { return std::make_pair(set[b], emme::contour_class(re[b])); };
    // the order is a regrouping of what plan_order made: groups ascend, and inside a group that order is kept
    {
        std::vector<int> a = before, b = p.order;
        std::sort(a.begin(), a.end()), std::sort(b.begin(), b.end());
        CHECK(a == b);
        for (int q = 1; q < m; ++q) CHECK(group(p.order[q - 1]) <= group(p.order[q]));
        for (int v : before) {
            std::vector<int> x, y;
            for (int u : before)
                if (group(u) == group(v)) x.push_back(u);
            for (int u : p.order)
                if (group(u) == group(v)) y.push_back(u);
            CHECK(x == y);
        }
    }
    // the chunks cover every position once, hold 1 .. 16 omegas of ONE set and ONE class, and the map behind them
    // names chunk and column
    std::vector<int> seen(m, 0);
    CHECK((int)p.ch.size() == 2 * p.plan.nchunks + m);
    for (int k = 0; k < p.plan.nchunks; ++k) {
        CHECK(p.size(k) >= 1 && p.size(k) <= 16);
        CHECK(p.first(k) >= 0 && p.first(k) + p.size(k) <= m);
        for (int w = 0; w < p.size(k); ++w) {
            const int pos = p.first(k) + w;
            ++seen[pos];
            CHECK(group(p.order[pos]) == group(p.order[p.first(k)]));
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
        // twelve items over three sets in shuffled set order, both classes inside set 3: four groups, a chunk each, in
        // the order (set, class) -- what tests/test_gpu_tile_sets.py relies on with dense_min_tasks = 0
        const std::vector<int> set = {3, 0, 4, 3, 0, 3, 4, 0, 3, 4, 3, 0};
        const std::vector<double> re = {-0.8, -0.5, -0.3, 0.4, -0.6, -0.2, -0.7, -0.9, 0.6, -0.4, -0.1, -0.35};
        const Plan p = make(shape(16, 0), re, set, {});
        CHECK(p.plan.nchunks == 4);
        const std::vector<int> want = {1, 4, 7, 11, 0, 5, 10, 3, 8, 2, 6, 9};
        CHECK(p.order == want);
        CHECK(p.size(0) == 4 && p.size(1) == 3 && p.size(2) == 2 && p.size(3) == 3);
        CHECK(p.first(0) == 0 && p.first(1) == 4 && p.first(2) == 7 && p.first(3) == 9);
    }
    {
        // without host_set the plan is the one-set plan: the same order and table as the five-argument call
        std::vector<double> re(40), om(80, 0.25);
        for (int b = 0; b < 40; ++b) re[b] = (b & 1) ? 0.5 : -0.5, om[2 * b] = re[b];
        std::vector<int> o1, o2, c1, c2;
        emme::plan_order(40, nullptr, nullptr, nullptr, o1);
        o2 = o1;
        const std::vector<int> zeros(40, 0);
        const emme::ChunkPlan a = emme::plan_tile_chunks(shape(256), o1, om.data(), nullptr, c1);
        const emme::ChunkPlan b = emme::plan_tile_chunks(shape(256), o2, om.data(), nullptr, c2, zeros.data());
        CHECK(a.nchunks == b.nchunks && o1 == o2 && c1 == c2);
    }
    {
        // more than one chunk per group: 20 omegas of one class on set 1 and 3 on set 0 (npoints 24: 18 tiles)
        std::vector<int> set(23, 1);
        set[5] = set[11] = set[19] = 0;
        const Plan p = make(shape(24, 0), std::vector<double>(23, -0.3), set, {});
        CHECK(p.plan.nchunks == 3);
        CHECK(p.size(0) == 3 && p.size(1) == 16 && p.size(2) == 4);
        CHECK(p.order[0] == 5 && p.order[1] == 11 && p.order[2] == 19);
    }
    {
        // the halving counts the chunks of the whole launch: npoints 48 has 71 tiles; 8 sets x 16 omegas of one class in
        // chunks of 16 are 568 tasks, of 8 1136, of 4 2272
        std::vector<int> set(128);
        for (int b = 0; b < 128; ++b) set[b] = b % 8;
        const Plan p = make(shape(48), std::vector<double>(128, -0.3), set, {});
        CHECK(p.plan.nchunks == 32);
        for (int k = 0; k < 32; ++k) CHECK(p.size(k) == 4);
        // ... and groups of 3 are cut to 2 + 1 once the cap is 2: 4 sets x 3 omegas at npoints 24 (18 tiles)
        std::vector<int> set3(12);
        for (int b = 0; b < 12; ++b) set3[b] = b / 3;
        const Plan q = make(shape(24), std::vector<double>(12, -0.3), set3, {});
        CHECK(q.plan.nchunks == 8);
        for (int k = 0; k < 8; ++k) CHECK(q.size(k) == (k % 2 ? 1 : 2));
    }
    {
        // costs: inside a group the most expensive omega first; an omega of 10 x the typical cost gets a chunk of 4,
        // and that chunk is the launch's first although its set is the last
        std::vector<int> set(128);
        for (int b = 0; b < 128; ++b) set[b] = b / 32;
        std::vector<unsigned long long> cost(128, 1000ull);
        cost[100] = 10000ull;
        const Plan p = make(shape(256), std::vector<double>(128, -0.3), set, cost);
        CHECK(p.size(0) == 4 && p.order[p.first(0)] == 100 && p.first(0) == 96);
        CHECK(p.plan.nchunks == 2 + 2 + 2 + 3);  // 32 = 16 + 16 per set; set 3: 4 + 16 + 12
    }
    {
        // an active mask: only the marked items are planned; a set without items makes no chunk
        std::vector<int> active(32, 0), set(32);
        for (int b = 0; b < 32; ++b) set[b] = b % 4, active[b] = (b % 4) != 2;
        const Plan p = make(shape(256), std::vector<double>(32, 0.4), set, {}, active.data());
        CHECK((int)p.order.size() == 24 && p.plan.nchunks == 3);
    }
    {
        // no omegas, no chunks
        std::vector<int> none, ch(3, 7);
        const double om[2] = {0.0, 0.0};
        const int set[1] = {0};
        const emme::ChunkPlan p = emme::plan_tile_chunks(shape(256), none, om, nullptr, ch, set);
        CHECK(p.nchunks == 0 && ch.empty());
    }
    if (failures) {
        std::fprintf(stderr, "host_plan_tile_sets_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_plan_tile_sets_selftest ok\n");
    return 0;
}
