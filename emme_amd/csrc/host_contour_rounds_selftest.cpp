// host_contour_rounds_selftest.cpp -- the round plan of the region search over (parameter set, contour) items
// (host_contour.cpp: ContourRounds), of which the search on one contour is the one-item case without a
// set, and the argument rules, candidates and root filter, built without device code and run under AddressSanitizer +
// UBSan by `make -C emme_amd/csrc host-sanitize`.  The log-dets a device would hand back are made up: arg det = W t on the item's ellipse, so an item
// resolves its count once 2 pi W / N <= pi / 2.  Covered: ragged doubling, an item dropped in mid-call, an item at its
// max_points, two items on one set, L doubling of a subset, nodes without factors left out of the sums, the node sequence
// and weights of one item without a set.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "host_contour.hpp"

namespace emme {
void set_error(const std::string&) {}
}  // namespace emme

static int failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                                 \
        }                                                                               \
    } while (0)

static emme_contour_t contour(double cx, double cy, double a, double b, int points, int max_points, int probes) {
    emme_contour_t c;
    emme_contour_default(&c);
    c.center[0] = cx, c.center[1] = cy, c.semi_axes[0] = a, c.semi_axes[1] = b;
    c.points = points, c.max_points = max_points, c.probes = probes;
    return c;
}

int main() {
    using emme::ContourRounds;
    // item:        0: resolves at once   1: one doubling   2: two doublings, set 1 again   3: stuck at max_points
    //              4: dropped while it doubles
    const int set[5] = {0, 1, 1, 2, 0};
    const int zeros[5] = {1, 3, 5, 5, 3};
    const emme_contour_t cts[5] = {contour(-0.8, 0.2, 0.2, 0.1, 8, 512, 8), contour(-0.7, 0.1, 0.1, 0.1, 8, 512, 8),
                                   contour(-0.7, 0.1, 0.1, 0.1, 8, 512, 8), contour(0.6, 0.1, 0.2, 0.2, 8, 16, 1),
                                   contour(0.6, 0.1, 0.2, 0.2, 8, 512, 8)};
    ContourRounds plan(5, set, cts);
    std::vector<double> ld;
    auto logdets = [&]() {  // arg det = W t at every node so far
        ld.assign(2 * (size_t)plan.nodes(), 0.0);
        for (int k = 0; k < 5; ++k) {
            const ContourRounds::Item& it = plan.items[k];
            for (size_t q = 0; q < it.nodes.size(); ++q)
                ld[2 * (size_t)it.nodes[q] + 1] = std::remainder(zeros[k] * 2.0 * M_PI * it.node_m[q] / it.ct.max_points, 2.0 * M_PI);
        }
    };
    // round 0: the start nodes of every item, items in order
    CHECK(plan.plan_nodes());
    CHECK(plan.r_first == 0 && plan.nodes() == 40 && plan.r_item.size() == 40 && plan.r_omega.size() == 80);
    for (int q = 0; q < 40; ++q) CHECK(plan.r_item[q] == q / 8 && plan.r_set[q] == set[q / 8] && plan.node_item[q] == q / 8);
    for (int j = 0; j < 8; ++j) {
        CHECK(plan.items[0].node_m[j] == 64 * j && plan.items[3].node_m[j] == 2 * j);
        const double t = 2.0 * M_PI * j / 8;
        CHECK(plan.r_omega[2 * j] == cts[0].center[0] + cts[0].semi_axes[0] * std::cos(2.0 * M_PI * (64 * j) / 512));
        CHECK(std::fabs(plan.r_omega[2 * (24 + j) + 1] - (0.1 + 0.2 * std::sin(t))) < 1e-15);
    }
    logdets();
    plan.take_logdets(ld.data());
    CHECK(plan.items[0].W == 1 && !plan.items[0].adding);
    for (int k = 1; k < 5; ++k) CHECK(plan.items[k].W == -1 && plan.items[k].adding);
    // round 1: the midpoints of items 1 .. 4; item 4 loses a node fill
    CHECK(plan.plan_nodes());
    CHECK(plan.r_first == 40 && plan.r_item.size() == 32 && plan.nodes() == 72);
    for (int q = 0; q < 32; ++q) CHECK(plan.r_item[q] == 1 + q / 8);
    for (int j = 0; j < 8; ++j) CHECK(plan.items[1].node_m[8 + j] == 32 * (2 * j + 1) && plan.items[1].nodes[8 + j] == 40 + j);
    plan.drop(4, EMME_ENUMERIC);
    plan.drop(4, EMME_EDEVICE);  // (the first error stays)
    logdets();
    plan.take_logdets(ld.data());
    CHECK(plan.items[1].W == 3 && !plan.items[1].adding && plan.items[1].N == 16);
    CHECK(plan.items[2].W == -1 && plan.items[2].adding);
    CHECK(plan.items[3].W == -1 && !plan.items[3].adding && plan.items[3].N == 16);  // at its max_points
    CHECK(plan.items[4].dropped && plan.items[4].status == EMME_ENUMERIC && plan.items[4].W == -1 && !plan.items[4].adding);
    // round 2: item 2 alone
    CHECK(plan.plan_nodes());
    CHECK(plan.r_first == 72 && plan.r_item.size() == 16 && plan.nodes() == 88);
    for (int q = 0; q < 16; ++q) CHECK(plan.r_item[q] == 2 && plan.r_set[q] == 1);
    logdets();
    plan.take_logdets(ld.data());
    CHECK(plan.items[2].W == 5 && plan.items[2].N == 32);
    CHECK(!plan.plan_nodes() && plan.nodes() == 88 && plan.r_item.empty());
    // an item's nodes are those of a search of its own: every m once, in the order created
    for (int k = 0; k < 4; ++k) {
        const ContourRounds::Item& it = plan.items[k];
        CHECK((int)it.nodes.size() == it.N && (int)it.node_m.size() == it.N);
        std::vector<int> seen(it.ct.max_points, 0);
        for (int m : it.node_m) CHECK(m % (it.ct.max_points / it.N) == 0 && seen[m]++ == 0);
        for (size_t q = 1; q < it.nodes.size(); ++q) CHECK(it.nodes[q] > it.nodes[q - 1]);
    }
    // the moment pass: items 0 .. 3, one node of item 1 without factors
    std::vector<int> info(plan.nodes(), 0), which, off, idx;
    std::vector<double> wz;
    info[plan.items[1].nodes[3]] = 2;
    CHECK(plan.plan_moments(info.data(), which, off, idx, wz));
    CHECK(which == std::vector<int>({0, 1, 2, 3}) && off == std::vector<int>({0, 8, 23, 55, 71}));
    CHECK(wz.size() == 4 * (size_t)plan.nodes());
    for (int g = 0; g < 4; ++g)
        for (int q = off[g]; q < off[g + 1]; ++q) CHECK(plan.node_item[idx[q]] == which[g] && info[idx[q]] == 0);
    for (int q = off[1] + 1; q < off[2]; ++q) CHECK(idx[q] > idx[q - 1]);
    {
        // item 2, its node 9 (a midpoint of round 1): w = omega'(t) / (i N) with the final N = 32
        const ContourRounds::Item& it = plan.items[2];
        const double t = 2.0 * M_PI * it.node_m[9] / 512, a = 0.1, b = 0.1;
        const double* o = &wz[4 * (size_t)it.nodes[9]];
        CHECK(std::fabs(o[0] - b * std::cos(t) / 32) < 1e-17 && std::fabs(o[1] - a * std::sin(t) / 32) < 1e-17);
        CHECK(std::fabs(o[2] - std::cos(t)) < 1e-15 && std::fabs(o[3] - std::sin(t)) < 1e-15);
    }
    // ranks: items 0 and 3 are done, items 1 and 2 double L; then item 1 alone, up to the cap of 64
    int l0 = -1, nl = -1;
    CHECK(!plan.take_rank(0, 1, &l0, &nl) && plan.items[0].k == 1 && plan.items[0].L == 8);
    CHECK(plan.take_rank(1, 8, &l0, &nl) && l0 == 8 && nl == 8 && plan.items[1].L == 16);
    CHECK(plan.take_rank(2, 8, &l0, &nl) && l0 == 8 && nl == 8);
    CHECK(!plan.take_rank(3, 0, &l0, &nl) && plan.items[3].L == 1);
    CHECK(plan.plan_moments(info.data(), which, off, idx, wz) && which == std::vector<int>({1, 2}));
    CHECK(plan.take_rank(1, 16, &l0, &nl) && l0 == 16 && nl == 16);
    CHECK(!plan.take_rank(2, 5, &l0, &nl) && plan.items[2].L == 16 && plan.items[2].k == 5);
    CHECK(plan.plan_moments(info.data(), which, off, idx, wz) && which == std::vector<int>({1}) && off.back() == 15);
    CHECK(plan.take_rank(1, 32, &l0, &nl) && l0 == 32 && nl == 32 && plan.items[1].L == 64);
    CHECK(plan.plan_moments(info.data(), which, off, idx, wz));
    CHECK(!plan.take_rank(1, 64, &l0, &nl) && plan.items[1].L == 64);
    CHECK(!plan.plan_moments(info.data(), which, off, idx, wz) && which.empty());
    // an item dropped by a failed Beyn step takes no further part
    {
        ContourRounds two(2, set, cts);
        CHECK(two.plan_nodes());
        two.drop(0, EMME_ENUMERIC);
        CHECK(two.plan_moments(info.data(), which, off, idx, wz) && which == std::vector<int>({1}));
    }
    // The search on one contour is this plan with one item and no set.  Spelled out, what the driver that
    // emme_find_roots_in_contour had of its own did with points = 4, max_points = 16 and a count that resolves on 16
    // nodes: nodes at t = 2 pi m / 16 with m = 0, 4, 8, 12, then the midpoints 2, 6, 10, 14, then the odd m; omega from
    // the centre and the semi-axes; the count on the nodes sorted by m; the weights of all 16 nodes with the final N.
    {
        const double cx = -0.8, cy = 0.2, ea = 0.2, eb = 0.1, rho = std::max(ea, eb);
        const emme_contour_t c1 = contour(cx, cy, ea, eb, 4, 16, 8);
        ContourRounds one(1, nullptr, &c1);
        CHECK(one.items[0].set == 0 && one.items[0].L == 8);
        const int want_m[16] = {0, 4, 8, 12, 2, 6, 10, 14, 1, 3, 5, 7, 9, 11, 13, 15};
        const int first[3] = {0, 4, 8}, cnt[3] = {4, 4, 8};
        const ContourRounds::Item& it = one.items[0];
        for (int r = 0; r < 3; ++r) {
            CHECK(one.plan_nodes());
            CHECK(one.r_first == first[r] && (int)one.r_item.size() == cnt[r] && one.nodes() == first[r] + cnt[r]);
            CHECK(it.N == first[r] + cnt[r] && (int)it.nodes.size() == it.N && (int)one.r_omega.size() == 2 * cnt[r]);
            for (int q = 0; q < cnt[r]; ++q) {
                const int j = first[r] + q, m = want_m[j];
                CHECK(one.r_item[q] == 0 && it.nodes[j] == j && it.node_m[j] == m);
                const double t = 2.0 * M_PI * m / 16;
                CHECK(one.r_omega[2 * q] == cx + ea * std::cos(t) && one.r_omega[2 * q + 1] == cy + eb * std::sin(t));
            }
            // steps of 2.8 between neighbours on the contour leave the count open; on 16 nodes arg det = 2 t
            ld.assign(2 * (size_t)one.nodes(), 0.0);
            for (int j = 0; j < it.N; ++j)
                ld[2 * j + 1] = r < 2 ? ((it.node_m[j] / (16 / it.N)) & 1 ? 2.8 : 0.0)
                                      : std::remainder(2 * 2.0 * M_PI * it.node_m[j] / 16, 2.0 * M_PI);
            one.take_logdets(ld.data());
            CHECK(it.adding == (r < 2) && it.W == (r < 2 ? -1 : 2));
        }
        CHECK(!one.plan_nodes() && it.N == 16 && one.nodes() == 16);
        std::vector<int> ok(16, 0);
        CHECK(one.plan_moments(ok.data(), which, off, idx, wz));
        CHECK(which == std::vector<int>({0}) && off == std::vector<int>({0, 16}) && wz.size() == 64);
        for (int j = 0; j < 16; ++j) {
            // w = omega'(t) / (i N), z = (omega - c) / rho with rho = max(a, b)
            const double t = 2.0 * M_PI * want_m[j] / 16, dre = -ea * std::sin(t), dim_ = eb * std::cos(t);
            CHECK(idx[j] == j && wz[4 * j] == dim_ / 16 && wz[4 * j + 1] == -dre / 16);
            CHECK(wz[4 * j + 2] == ea * std::cos(t) / rho && wz[4 * j + 3] == eb * std::sin(t) / rho);
        }
        // a count left open at max_points goes on to the moments all the same, with winding -1
        const emme_contour_t c2 = contour(cx, cy, ea, eb, 4, 4, 8);
        ContourRounds capped(1, nullptr, &c2);
        CHECK(capped.plan_nodes());
        ld.assign(8, 0.0);
        ld[3] = ld[7] = 2.8;
        capped.take_logdets(ld.data());
        CHECK(!capped.plan_nodes() && capped.items[0].W == -1 && capped.items[0].N == 4);
        CHECK(capped.plan_moments(ok.data(), which, off, idx, wz) && off.back() == 4);
        // no set with several items: every item on set 0
        ContourRounds none(5, nullptr, cts);
        CHECK(none.plan_nodes() && none.r_item.size() == 40);
        for (int k = 0; k < 5; ++k) CHECK(none.items[k].set == 0);
    }
    // the argument rules
    {
        emme_contour_t c = cts[0];
        CHECK(emme::contour_arg_error(&c) == nullptr);
        c.size = 4;
        CHECK(std::string(emme::contour_arg_error(&c)).find("wrong size") != std::string::npos);
        c = cts[0], c.semi_axes[1] = -0.1;
        CHECK(std::string(emme::contour_arg_error(&c)).find("semi-axes") != std::string::npos);
        c = cts[0], c.center[0] = NAN;
        CHECK(std::string(emme::contour_arg_error(&c)).find("semi-axes") != std::string::npos);
        c = cts[0], c.center[0] = -0.1;
        CHECK(std::string(emme::contour_arg_error(&c)).find("Re omega = 0") != std::string::npos);
        c = cts[0], c.points = 12;
        CHECK(std::string(emme::contour_arg_error(&c)).find("powers of two") != std::string::npos);
        c = cts[0], c.max_points = 4;
        CHECK(std::string(emme::contour_arg_error(&c)).find("powers of two") != std::string::npos);
        c = cts[0], c.probes = 65;
        CHECK(std::string(emme::contour_arg_error(&c)).find("probes") != std::string::npos);
        c = cts[0], c.rank_tol = 1.0;
        CHECK(std::string(emme::contour_arg_error(&c)).find("rank_tol") != std::string::npos);
    }
    // candidates and the kept roots
    {
        const emme_contour_t& c = cts[0];  // centre -0.8 + 0.2i, a = 0.2, b = 0.1: rho = 0.2
        const double mu[8] = {0.5, 0.0, 0.0, 0.7, NAN, 0.0, 1.4, 0.0};  // radius 0.5, 1.4, NaN, 1.4
        std::vector<double> g;
        emme::contour_candidates(c, 4, mu, g);
        CHECK(g.size() == 6 && std::fabs(g[0] + 0.7) < 1e-15 && std::fabs(g[3] - 0.34) < 1e-15 && std::fabs(g[4] + 0.52) < 1e-15);
        // chains: inside, a duplicate of it, outside, failed, out of steps with a last step above tol, one more inside
        const int step_limit = 2;
        const double r[12] = {-0.8, 0.21, -0.8, 0.21 + 1e-9, -0.5, 0.2, -0.8, 0.2, -0.75, 0.2, -0.85, 0.25};
        const int its[6] = {1, 1, 1, 1, 3, 3}, inf[6] = {0, 0, 0, EMME_ENUMERIC, 0, 0};
        std::vector<double> path(2 * 6 * 3, 0.0);
        path[2 * (4 * 3 + 2)] = -0.75, path[2 * (4 * 3 + 2) + 1] = 0.2, path[2 * (4 * 3 + 1)] = -0.76, path[2 * (4 * 3 + 1) + 1] = 0.2;
        path[2 * (5 * 3 + 2)] = -0.85, path[2 * (5 * 3 + 2) + 1] = 0.25, path[2 * (5 * 3 + 1)] = -0.85, path[2 * (5 * 3 + 1) + 1] = 0.25;
        const std::vector<emme::ContourRoot> f = emme::contour_keep_roots(c, 1e-6, step_limit, 6, r, its, inf, path.data());
        CHECK(f.size() == 2 && f[0].im == 0.25 && f[0].it == 3 && f[1].im == 0.21 && f[1].re == -0.8);
    }
    if (failures) {
        std::fprintf(stderr, "%d contour round-plan self-test failures\n", failures);
        return 1;
    }
    std::printf("contour round-plan self-test ok (ASan + UBSan clean)\n");
    return 0;
}
