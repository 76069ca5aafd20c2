// sens_plan_selftest.cpp -- the chunk plan of emme_root_sensitivities_sets (sens_plan.cpp) and the rounding-level rule,
// stand-alone under AddressSanitizer + UBSan (make host-sanitize).
#include <cmath>
#include <cstdio>
#include <limits>

#include "sens_plan.hpp"

using namespace emme;

static int fails = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++fails;                                                      \
        }                                                                 \
    } while (0)

// every root and every pair exactly once, in order, no chunk above the cap
static void check_cover(const SensPlan& p, int ngood, int ndir) {
    int next = 0;
    for (const SensChunk& c : p.base) {
        CHECK(c.first == next && c.count >= 1 && 2 * c.count <= p.cap);
        next += c.count;
    }
    CHECK(next == ngood);
    next = 0;
    for (const SensChunk& c : p.pairs) {
        CHECK(c.first == next && c.count >= 1 && 2 * c.count <= p.cap);
        next += c.count;
    }
    CHECK(next == ngood * ndir);
    CHECK(p.cap >= 2 && p.cap % 2 == 0);
}

int main() {
    // a cap below one pair's two matrices is rounded up to one pair
    {
        const SensPlan p = sens_plan(2, 6, 1, 16);
        CHECK(p.cap == 2);
        CHECK(p.base.size() == 2 && p.pairs.size() == 12);
        check_cover(p, 2, 6);
    }
    // an odd cap holds the whole pairs below it
    {
        const SensPlan p = sens_plan(2, 6, 3, 16);
        CHECK(p.cap == 2 && p.pairs.size() == 12);
        check_cover(p, 2, 6);
    }
    // a cap that splits inside a root's directions: 6 directions, 4 pairs per chunk -> 4 | 4 | 4, the second chunk
    // begins at direction 4 of root 0 and ends at direction 1 of root 1
    {
        const SensPlan p = sens_plan(2, 6, 8, 16);
        CHECK(p.cap == 8 && p.base.size() == 1 && p.base[0].count == 2);
        CHECK(p.pairs.size() == 3);
        CHECK(p.pairs[1].first == 4 && p.pairs[1].count == 4);
        CHECK(p.pairs[1].first / 6 == 0 && (p.pairs[1].first + p.pairs[1].count - 1) / 6 == 1);
        check_cover(p, 2, 6);
    }
    // ndir = 0: base chunks only
    {
        const SensPlan p = sens_plan(5, 0, 4, 16);
        CHECK(p.pairs.empty() && p.base.size() == 3 && p.base[2].count == 1);
        check_cover(p, 5, 0);
    }
    // one chunk: the automatic budget at a small order
    {
        const SensPlan p = sens_plan(2, 6, 0, 16);
        CHECK(p.cap == SENS_AUTO_MAX_ITEMS);
        CHECK(p.base.size() == 1 && p.pairs.size() == 1 && p.pairs[0].count == 12);
        check_cover(p, 2, 6);
    }
    // the automatic budget in bytes: 1 GiB of 4 MiB matrices at order 512; never below one pair
    CHECK(sens_cap(0, 512) == 256);
    CHECK(sens_cap(0, 2048) == 16);
    CHECK(sens_cap(0, 1 << 15) == 2);
    // no good root: nothing to do
    {
        const SensPlan p = sens_plan(0, 3, 0, 16);
        CHECK(p.base.empty() && p.pairs.empty());
    }
    // many roots, a cap that does not divide them
    {
        const SensPlan p = sens_plan(37, 3, 10, 64);
        CHECK(p.base.size() == 8 && p.pairs.size() == 23);
        check_cover(p, 37, 3);
    }
    // the rounding-level rule
    const double eps = std::numeric_limits<double>::epsilon();
    CHECK(sens_form_at_rounding(0.0, 16, 1.0, 1.0));
    CHECK(sens_form_at_rounding(64.0 * 16 * eps, 16, 1.0, 1.0));
    CHECK(!sens_form_at_rounding(65.0 * 16 * eps, 16, 1.0, 1.0));
    CHECK(!sens_form_at_rounding(0.58, 16, 3.0, 1.0));
    CHECK(!sens_form_at_rounding(std::nan(""), 16, 1.0, 1.0));
    CHECK(!sens_form_at_rounding(1.0, 16, std::nan(""), 1.0));
    if (fails == 0) std::printf("sens_plan_selftest: ok\n");
    return fails ? 1 : 0;
}
