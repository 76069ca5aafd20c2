// host_plan_tile_shape_sets_selftest.cpp -- the chunk plan of the table-free tile fill over parameter sets on an
// electromagnetic context (fill_plan.cpp: plan_tile_chunks with nm = 3 and host_set): a chunk is 16
// columns = 5 omegas x 3 moments of ONE set and ONE contour class; the position map is a bijection; the most expensive
// chunk comes first; the dense_min_tasks halving (5 -> 2) counts the chunks of the whole launch, not those of a set.
// Built without device code and run under AddressSanitizer + UBSan by `make -C emme_amd/csrc host-sanitize`.
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

static emme::FillShape shape(int npoints, int gk, int dense_min_tasks = 2000) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = true, s.folded = true, s.nm = 3, s.gk_points = gk;
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

// re[b]: Re omega_b, set[b]: its parameter set; cost may be empty.  Checks what holds for every plan.
static Plan make(const emme::FillShape& s, const std::vector<double>& re, const std::vector<int>& set,
                 const std::vector<unsigned long long>& cost) {
    Plan p;
    const int n = (int)re.size();
    std::vector<double> om(2 * n, 0.25);
    for (int b = 0; b < n; ++b) om[2 * b] = re[b];
    const unsigned long long* cs = cost.empty() ? nullptr : cost.data();
    emme::plan_order(n, nullptr, cs, nullptr, p.order);
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
    // chunks of 1 .. 5 omegas of ONE set and ONE class; the map behind the chunk table names chunk and column of every
    // position, and every position belongs to exactly one (chunk, column): a bijection
    std::vector<int> seen(m, 0);
    CHECK((int)p.ch.size() == 2 * p.plan.nchunks + m);
    for (int k = 0; k < p.plan.nchunks; ++k) {
        CHECK(p.size(k) >= 1 && p.size(k) <= 5);
        CHECK(p.first(k) >= 0 && p.first(k) + p.size(k) <= m);
        for (int w = 0; w < p.size(k); ++w) {
            const int pos = p.first(k) + w;
            ++seen[pos];
            CHECK(group(p.order[pos]) == group(p.order[p.first(k)]));
            CHECK(p.ch[2 * p.plan.nchunks + pos] == ((k << 8) | w));
        }
    }
    for (int v : seen) CHECK(v == 1);
    {
        std::vector<int> codes(p.ch.begin() + 2 * p.plan.nchunks, p.ch.end());
        std::sort(codes.begin(), codes.end());
        CHECK(std::adjacent_find(codes.begin(), codes.end()) == codes.end());
    }
    // the most expensive chunk first
    if (cs)
        for (int k = 1; k < p.plan.nchunks; ++k) CHECK(cs[p.order[p.first(k - 1)]] >= cs[p.order[p.first(k)]]);
    return p;
}

int main() {
    for (int gk : {15, 31}) {
        {
            // twelve items over three sets in shuffled set order, both classes inside sets 1 and 2, six omegas in the
            // group (set 1, Re omega < 0): chunks of 5 + 1 -- what tests/test_gpu_tile_shape_sets.py relies on with
            // dense_min_tasks = 0
            const std::vector<int> set = {1, 0, 2, 1, 0, 1, 2, 1, 1, 0, 1, 1};
            const std::vector<double> re = {-1.656, -0.85, 0.4, 0.4, -1.656, -0.85, -1.6, -1.6, -1.7, -0.142, -1.64, -0.9};
            const Plan p = make(shape(10, gk, 0), re, set, {});
            const std::vector<int> want = {1, 4, 9, 0, 5, 7, 8, 10, 11, 3, 6, 2};
            CHECK(p.order == want);
            CHECK(p.plan.nchunks == 6);
            const std::vector<int> table = {0, 3, 3, 5, 8, 1, 9, 1, 10, 1, 11, 1};
            CHECK(std::vector<int>(p.ch.begin(), p.ch.begin() + 12) == table);
        }
        {
            // the halving counts the chunks of the whole launch.  npoints 64 has 126 tiles: 16 sets x 5 omegas of one class
            // are 16 chunks of 5 = 2016 tasks, enough; 15 sets are 1890 tasks, short: the capacity goes 5 -> 2 and
            // every set's five omegas are cut 2 + 2 + 1
            std::vector<int> set(80);
            for (int b = 0; b < 80; ++b) set[b] = b % 16;
            const Plan p = make(shape(64, gk), std::vector<double>(80, -0.3), set, {});
            CHECK(p.plan.nchunks == 16);
            for (int k = 0; k < 16; ++k) CHECK(p.size(k) == 5);
            std::vector<int> set15(75);
            for (int b = 0; b < 75; ++b) set15[b] = b % 15;
            const Plan q = make(shape(64, gk), std::vector<double>(75, -0.3), set15, {});
            CHECK(q.plan.nchunks == 45);
            for (int k = 0; k < 45; ++k) CHECK(q.size(k) == (k % 3 == 2 ? 1 : 2));
            // ... and it stops at 2: npoints 48 (71 tiles), 8 sets x 5 omegas: 24 chunks, 1704 tasks, still short
            std::vector<int> set8(40);
            for (int b = 0; b < 40; ++b) set8[b] = b / 5;
            const Plan r = make(shape(48, gk), std::vector<double>(40, -0.3), set8, {});
            CHECK(r.plan.nchunks == 24);
            for (int k = 0; k < 24; ++k) CHECK(r.size(k) == (k % 3 == 2 ? 1 : 2));
        }
        {
            // both classes in every set: 4 sets x (7 + 3) omegas, npoints 256: chunks 5 + 2 and 3 per set, never mixed
            std::vector<int> set(40);
            std::vector<double> re(40);
            for (int b = 0; b < 40; ++b) set[b] = b % 4, re[b] = (b / 4) % 10 < 7 ? -0.5 : 0.5;
            const Plan p = make(shape(256, gk), re, set, {});
            CHECK(p.plan.nchunks == 12);
        }
        {
            // costs: an omega of 10 x the typical cost gets a chunk of 2 (10 x 5 > 5 x 4 >= 10 x 2), and that chunk is
            // the launch's first although its set is the last
            std::vector<int> set(40);
            for (int b = 0; b < 40; ++b) set[b] = b / 10;
            std::vector<unsigned long long> cost(40, 1000ull);
            cost[33] = 10000ull;
            const Plan p = make(shape(256, gk), std::vector<double>(40, -0.3), set, cost);
            CHECK(p.size(0) == 2 && p.order[p.first(0)] == 33 && p.first(0) == 30);
            CHECK(p.plan.nchunks == 2 + 2 + 2 + 3);  // 10 = 5 + 5 per set; set 3: 2 + 5 + 3
        }
    }
    if (failures) {
        std::fprintf(stderr, "host_plan_tile_shape_sets_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_plan_tile_shape_sets_selftest ok\n");
    return 0;
}
