// host_plan_tile_shape_selftest.cpp -- the chunk plan of the table-free tile fill for electromagnetic contexts
// (fill_plan.cpp: plan_tile_chunks with nm = 3): a chunk is 16 columns = 5 omegas x 3 moments, so no
// chunk holds more than 5 omegas; chunks never mix contour classes, every omega is planned exactly once, the most
// expensive chunk comes first and the dense_min_tasks halving ends at 2.  For nm = 1 the plans are those of
// host_plan_tile_selftest.cpp's cases, compared here against what that self-test pins.  Built without device code and run
// under AddressSanitizer + UBSan by `make -C emme_amd/csrc host-sanitize`.
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

static emme::FillShape shape(int npoints, int nm, int gk) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = true, s.folded = true, s.nm = nm, s.gk_points = gk;
    s.npairs = npoints * (npoints - 1) / 2;
    return s;
}

struct Plan {
    emme::ChunkPlan plan;
    std::vector<int> order, ch;
    int size(int k) const { return ch[2 * k + 1]; }
    int first(int k) const { return ch[2 * k]; }
};

// re[b]: Re omega_b; cost may be empty.  Checks what holds for every plan: a regrouping of plan_order's list that keeps
// its order inside a class, chunks of 1 .. 16 / nm omegas of ONE class that cover every position once, the position
// map behind them, the most expensive chunk first.
static Plan make(int npoints, int nm, int gk, const std::vector<double>& re, const std::vector<unsigned long long>& cost) {
    Plan p;
    const int n = (int)re.size(), cap = 16 / nm;
    std::vector<double> om(2 * n, 0.25);
    for (int b = 0; b < n; ++b) om[2 * b] = re[b];
    const unsigned long long* cs = cost.empty() ? nullptr : cost.data();
    emme::plan_order(n, nullptr, cs, nullptr, p.order);
    const std::vector<int> before = p.order;
    p.plan = emme::plan_tile_chunks(shape(npoints, nm, gk), p.order, om.data(), cs, p.ch);
    const int m = (int)p.order.size();
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
    std::vector<int> seen(m, 0);
    CHECK((int)p.ch.size() == 2 * p.plan.nchunks + m);
    for (int k = 0; k < p.plan.nchunks; ++k) {
        CHECK(p.size(k) >= 1 && p.size(k) <= cap);
        CHECK(p.first(k) >= 0 && p.first(k) + p.size(k) <= m);
        for (int w = 0; w < p.size(k); ++w) {
            const int pos = p.first(k) + w;
            ++seen[pos];
            CHECK(emme::contour_class(re[p.order[pos]]) == emme::contour_class(re[p.order[p.first(k)]]));
            CHECK(p.ch[2 * p.plan.nchunks + pos] == ((k << 8) | w));
        }
    }
    for (int v : seen) CHECK(v == 1);
    if (cs)
        for (int k = 1; k < p.plan.nchunks; ++k) CHECK(cs[p.order[p.first(k - 1)]] >= cs[p.order[p.first(k)]]);
    return p;
}

int main() {
    for (int gk : {15, 31}) {
        {
            // 128 omegas of one class on the N = 256 grid (2040 tiles): 25 chunks of 5 and one of 3
            const Plan p = make(256, 3, gk, std::vector<double>(128, -0.3), {});
            CHECK(p.plan.nchunks == 26);
            int n5 = 0, n3 = 0;
            for (int k = 0; k < p.plan.nchunks; ++k) n5 += p.size(k) == 5, n3 += p.size(k) == 3;
            CHECK(n5 == 25 && n3 == 1);
        }
        {
            // both classes interleaved: 12 omegas, every other one on the Re omega > 0 side: 5 + 1 per class
            std::vector<double> re(12);
            for (int b = 0; b < 12; ++b) re[b] = (b & 1) ? 0.5 : -0.5;
            const Plan p = make(256, 3, gk, re, {});
            CHECK(p.plan.nchunks == 4);
            std::vector<unsigned long long> cost(12);
            for (int b = 0; b < 12; ++b) cost[b] = 1000ull + (unsigned long long)((b * 7) % 12);
            make(256, 3, gk, re, cost);
        }
        {
            // 3 + 1 omegas on a 10-point grid (45 pairs, 3 tiles): few tasks, the capacity is halved to 2: chunks of
            // 2 + 1 for the class of three, 1 for the other -- 3 chunks
            const Plan p = make(10, 3, gk, {-1.656, -0.85, 0.4, -0.142}, {});
            CHECK(p.plan.nchunks == 3);
            int sizes[3] = {p.size(0), p.size(1), p.size(2)};
            std::sort(sizes, sizes + 3);
            CHECK(sizes[0] == 1 && sizes[1] == 1 && sizes[2] == 2);
        }
        {
            // the halving below dense_min_tasks (2000) goes 5 -> 2 and stops there: npoints 48 has 71 tiles, 40 omegas in
            // chunks of 5 are 568 tasks, of 2 1420 -- still short, and still 2
            const Plan p = make(48, 3, gk, std::vector<double>(40, -0.3), {});
            CHECK(p.plan.nchunks == 20);
            for (int k = 0; k < 20; ++k) CHECK(p.size(k) == 2);
            // one omega, one pair: one chunk of one
            const Plan q = make(2, 3, gk, {-0.8}, {});
            CHECK(q.plan.nchunks == 1 && q.size(0) == 1 && q.first(0) == 0);
        }
        {
            // the cost cut (dense_cost_ratio 4): an omega of 10 x the typical cost gets a chunk of 2 (10 x 5 > 5 x 4 >= 10 x 2)
            // and it is the first chunk of the launch; per class
            std::vector<unsigned long long> cost(128, 1000ull);
            cost[17] = 10000ull;
            std::vector<double> re(128, -0.3);
            const Plan p = make(256, 3, gk, re, cost);
            CHECK(p.order[0] == 17 && p.first(0) == 0 && p.size(0) == 2 && p.size(1) == 5);
            for (int b = 64; b < 128; ++b) re[b] = 0.3;
            cost[100] = 10000ull;
            const Plan q = make(256, 3, gk, re, cost);
            CHECK(q.size(0) == 2 && q.size(1) == 2);
            CHECK(q.order[q.first(0)] == 17 && q.order[q.first(1)] == 100);
        }
    }
    // ---- nm = 1: the plans host_plan_tile_selftest.cpp pins, for either rule ----
    for (int gk : {15, 31}) {
        {
            std::vector<double> re(40);
            for (int b = 0; b < 40; ++b) re[b] = (b & 1) ? 0.5 : -0.5;
            const Plan p = make(256, 1, gk, re, {});
            // class 0 first (positions 0 .. 19), chunks in the order they were cut (equal costs: the sort is stable)
            const std::vector<int> want = {0, 16, 16, 4, 20, 16, 36, 4};
            CHECK(p.plan.nchunks == 4 && std::vector<int>(p.ch.begin(), p.ch.begin() + 8) == want);
        }
        {
            const Plan p = make(256, 1, gk, std::vector<double>(17, -0.3), {});
            const std::vector<int> want = {0, 16, 16, 1};
            CHECK(p.plan.nchunks == 2 && std::vector<int>(p.ch.begin(), p.ch.begin() + 4) == want);
        }
        {
            const Plan p = make(48, 1, gk, std::vector<double>(128, -0.3), {});
            CHECK(p.plan.nchunks == 32);
            for (int k = 0; k < 32; ++k) CHECK(p.size(k) == 4 && p.first(k) == 4 * k);
            const Plan q = make(24, 1, gk, std::vector<double>(8, -0.3), {});
            CHECK(q.plan.nchunks == 4);
            for (int k = 0; k < 4; ++k) CHECK(q.size(k) == 2 && q.first(k) == 2 * k);
        }
        {
            std::vector<unsigned long long> cost(128, 1000ull);
            cost[17] = 10000ull;
            const Plan p = make(256, 1, gk, std::vector<double>(128, -0.3), cost);
            CHECK(p.order[0] == 17 && p.first(0) == 0 && p.size(0) == 4 && p.size(1) == 16);
            cost[17] = 100000ull;
            CHECK(make(256, 1, gk, std::vector<double>(128, -0.3), cost).size(0) == 2);
        }
    }
    if (failures) {
        std::fprintf(stderr, "host_plan_tile_shape_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_plan_tile_shape_selftest ok\n");
    return 0;
}
