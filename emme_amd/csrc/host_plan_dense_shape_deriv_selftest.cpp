// host_plan_dense_shape_deriv_selftest.cpp -- the fill planner (fill_plan.cpp) on derivative requests of electromagnetic
// and GK31 contexts on the tiled cache (FillShape::deriv with nm = 3 or gk_points = 31): the twin-column
// layout of k_assemble_dense_shape_deriv holds 8 K columns, so a chunk is at most 8 electrostatic omegas or 2 omegas x 3
// moments; the halving below dense_min_tasks and the dense_cost_ratio cut are plan_chunks' (both stop at 2, which is
// where an electromagnetic chunk starts), never a wide chunk, and the position map names chunk and position.  Electrostatic
// GK15 keeps its 8 (host_plan_deriv_selftest.cpp), plain requests keep 16 / nm.  Built without device code and run under
// AddressSanitizer + UBSan by `make -C emme_amd/csrc host-sanitize`.
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

static emme::FillShape shape(int npoints, int gk_points, int nm, bool deriv) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = true, s.folded = true, s.nm = nm, s.gk_points = gk_points;
    s.npairs = npoints * (npoints - 1) / 2;
    s.deriv = deriv;
    return s;
}

struct Plan {
    emme::ChunkPlan plan;
    std::vector<int> ch;
    int size(int k) const { return ch[2 * k + 1]; }
    int first(int k) const { return ch[2 * k]; }
    int widest() const {
        int w = 0;
        for (int k = 0; k < plan.nchunks; ++k) w = size(k) > w ? size(k) : w;
        return w;
    }
};

static Plan make(const emme::FillShape& s, const std::vector<unsigned long long>& cost, const unsigned char* wide = nullptr) {
    Plan p;
    std::vector<int> order;
    const int n = (int)cost.size();
    const int nw = emme::plan_order(n, nullptr, cost.data(), wide, order);
    p.plan = emme::plan_chunks(s, order, cost.data(), nw, p.ch);
    // every plan: the chunks tile the order, and the position map behind them names chunk and position
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

static std::vector<unsigned long long> flat(int n) { return std::vector<unsigned long long>((size_t)n, 1000ull); }

int main() {
    const emme::FillShape em31 = shape(256, 31, 3, true), em15 = shape(256, 15, 3, true), es31 = shape(256, 31, 1, true);
    {
        // capacities per shape, 128 omegas of equal cost on the N = 256 lattice: 2, 2, 8 -- and 8 for electrostatic
        // GK15, 5 / 5 / 16 / 16 for the plain requests of the four shapes
        const Plan a = make(em31, flat(128)), b = make(em15, flat(128)), c = make(es31, flat(128));
        CHECK(a.plan.nchunks == 64 && b.plan.nchunks == 64 && c.plan.nchunks == 16);
        for (int k = 0; k < 64; ++k) CHECK(a.size(k) == 2 && b.size(k) == 2);
        for (int k = 0; k < 16; ++k) CHECK(c.size(k) == 8);
        const Plan e = make(shape(256, 15, 1, true), flat(128));
        CHECK(e.plan.nchunks == 16 && e.widest() == 8);
        CHECK(make(shape(256, 31, 3, false), flat(128)).widest() == 5);
        CHECK(make(shape(256, 15, 3, false), flat(128)).widest() == 5);
        CHECK(make(shape(256, 31, 1, false), flat(128)).widest() == 16);
        CHECK(make(shape(256, 15, 1, false), flat(128)).widest() == 16);
    }
    {
        // the position map for n = 1, capacity, capacity + 1 (make() checks every entry; here the chunk sizes)
        for (const emme::FillShape& s : {em31, em15, es31}) {
            const int cap = 8 / s.nm;
            const Plan one = make(s, flat(1)), full = make(s, flat(cap)), over = make(s, flat(cap + 1));
            CHECK(one.plan.nchunks == 1 && one.size(0) == 1);
            CHECK(full.plan.nchunks == 1 && full.size(0) == cap);
            CHECK(over.plan.nchunks == 2 && over.size(0) == cap && over.size(1) == 1);
            CHECK(make(s, flat(128)).widest() == cap);
        }
    }
    {
        // the halving below dense_min_tasks (2000): npoints 48 has 71 tiles.  Electrostatic GK31: 128 omegas in chunks
        // of 8 are 1136 tasks, in chunks of 4 they are 2272.  8 omegas on npoints 24 (18 tiles): 8 -> 4 -> 2, and it
        // stops there.  An electromagnetic chunk starts at 2 and is never halved: one omega per chunk would leave 10 of
        // the 16 columns idle.
        const Plan c = make(shape(48, 31, 1, true), flat(128));
        CHECK(c.plan.nchunks == 32);
        for (int k = 0; k < 32; ++k) CHECK(c.size(k) == 4);
        const Plan c8 = make(shape(24, 31, 1, true), flat(8));
        CHECK(c8.plan.nchunks == 4 && c8.widest() == 2);
        const Plan a = make(shape(24, 31, 3, true), flat(8)), b = make(shape(24, 15, 3, true), flat(8));
        CHECK(a.plan.nchunks == 4 && b.plan.nchunks == 4);
        for (int k = 0; k < 4; ++k) CHECK(a.size(k) == 2 && b.size(k) == 2);
        // dense_min_tasks = 0 (one chunk where the batch fits one): no halving
        emme::FillShape s0 = shape(24, 31, 1, true);
        s0.dense_min_tasks = 0;
        const Plan c0 = make(s0, flat(8));
        CHECK(c0.plan.nchunks == 1 && c0.size(0) == 8);
    }
    {
        // the dense_cost_ratio cut (4): an electrostatic GK31 omega of 10 x the typical cost ends up in a chunk of 2
        // (10 x 4 > 8 x 4 >= 10 x 2); an electromagnetic one keeps its chunk of 2 (the cut stops at 2 as well)
        std::vector<unsigned long long> cost = flat(128);
        cost[17] = 10000ull;
        const Plan c = make(es31, cost), a = make(em31, cost);
        CHECK(c.size(0) == 2 && c.size(1) == 8 && c.widest() == 8);
        CHECK(a.size(0) == 2 && a.widest() == 2 && a.plan.nchunks == 64);
        emme::FillShape loose = es31;
        loose.dense_cost_ratio = 100.0;
        CHECK(make(loose, cost).size(0) == 8);
    }
    {
        // wide items (root search: omegas whose level lists overflowed) are planned like every other omega
        std::vector<unsigned char> wide(128, 0);
        wide[5] = wide[99] = 1;
        const Plan a = make(em31, flat(128), wide.data()), c = make(es31, flat(128), wide.data());
        CHECK(a.plan.nchunks == 64 && a.size(0) == 2 && a.size(1) == 2);
        CHECK(c.plan.nchunks == 16 && c.size(0) == 8);
    }
    {
        // no omegas, no chunks
        const std::vector<int> none;
        std::vector<int> ch(3, 7);
        const emme::ChunkPlan p = emme::plan_chunks(em31, none, nullptr, 0, ch);
        CHECK(p.nchunks == 0 && ch.empty());
    }
    if (failures) {
        std::fprintf(stderr, "host_plan_dense_shape_deriv_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host_plan_dense_shape_deriv_selftest ok\n");
    return 0;
}
