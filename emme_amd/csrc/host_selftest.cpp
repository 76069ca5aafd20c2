// host_selftest.cpp -- the host layer above the C ABI (JSON dialect reader, parameters, tables,
// scan generator, null vector, driver error paths, the fill planner) built WITHOUT the device code and run under
// AddressSanitizer + UBSan:   make -C emme_amd/csrc host-sanitize
// (GPU sanitizers are not available on the target pool; this covers the CPU side.)
// The device entry points the driver calls are stubbed to fail with EMME_EDEVICE, so
// emme_run_json is exercised up to and including its "no device" error record.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "fill_plan.hpp"

namespace emme {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace emme

extern "C" {
const char* emme_last_error(void) { return emme::g_err.c_str(); }
int emme_ctx_create(const emme_params_t*, int, emme_ctx_t** out) {
    *out = nullptr;
    emme::set_error("no HIP device (host self-test build)");
    return EMME_EDEVICE;
}
void emme_ctx_destroy(emme_ctx_t*) {}
int emme_ctx_dim(const emme_ctx_t*) { return EMME_EINVAL; }
int emme_solve_roots(emme_ctx_t*, const double*, int, double, int, double*, int*, int*, double*) { return EMME_EDEVICE; }
int emme_ctx_get_matrix(emme_ctx_t*, int, double*) { return EMME_EDEVICE; }
int emme_null_vectors_batch(emme_ctx_t*, int, int, const double*, double*, int*) { return EMME_EDEVICE; }
}

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// ---- the fill planner (fill_plan.cpp) -------------------------------------------------------------------------
// Expected plans are those of the dispatcher before the planner was lifted out of it (recorded by running that
// code on these inputs), so a change here is a change of what the fill launches.
struct PlanCase {
    const char* name;
    emme::FillShape s;
    int nbatch;
    std::vector<int> active;              // empty = all
    std::vector<unsigned long long> cost; // empty = none
    std::vector<unsigned char> wide;      // empty = none
    int positive = 0;                     // this many omegas, spread over the batch, at Re omega > 0
    bool has_cache[2] = {false, false};
    std::vector<double> omegas() const {
        std::vector<double> w(2 * (size_t)nbatch, 0.25);
        for (int b = 0; b < nbatch; ++b) w[2 * b] = -0.8;
        for (int k = 0; k < positive; ++k) w[2 * ((k * nbatch) / positive + 1)] = 0.5;
        return w;
    }
};

static emme::FillShape plan_shape(bool tiled, int nm, int gk_points, int npoints) {
    emme::FillShape s;  // (option values: the defaults of emme_options_default)
    s.tiled = tiled, s.nm = nm, s.gk_points = gk_points, s.npairs = npoints * (npoints + 1) / 2;
    return s;
}

static std::vector<unsigned long long> cost_ramp(int n) {
    std::vector<unsigned long long> c(n);
    for (int b = 0; b < n; ++b) c[b] = 500 + (unsigned long long)b * b * b / 8;
    return c;
}

static std::vector<PlanCase> plan_cases() {
    std::vector<PlanCase> v;
    std::vector<unsigned char> wide(128, 0);
    wide[7] = wide[100] = 1;
    // the headline search: electrostatic GK15, dense fill, 128 chains, two of them on the wide-list build
    v.push_back({"headline", plan_shape(true, 1, 15, 256), 128, {}, cost_ramp(128), wide});
    // a late Newton step of it: five chains left
    std::vector<int> five(128, 0);
    five[3] = five[40] = five[41] = five[90] = five[127] = 1;
    v.push_back({"headline, 5 live", plan_shape(true, 1, 15, 256), 128, five, cost_ramp(128), wide});
    v.push_back({"headline, 5 live, narrow chunks", plan_shape(true, 1, 15, 256), 128, five, cost_ramp(128), {}});
    v.back().s.dense_min_tasks = 100000000;
    v.push_back({"headline, union walk", plan_shape(false, 1, 15, 256), 128, five, cost_ramp(128), {}});
    // electromagnetic, tiled: 5 omegas x 3 moments per chunk
    v.push_back({"electromagnetic tiled", plan_shape(true, 3, 31, 64), 23, {}, cost_ramp(23), {}});
    // GK31 on independent lanes: lane groups of 32, chunks halve where an omega costs 1.5x the typical one
    v.push_back({"GK31 lanes", plan_shape(false, 1, 31, 96), 70, {}, cost_ramp(70), {}});
    v.push_back({"no costs", plan_shape(true, 1, 15, 256), 40, {}, {}, {}});
    v.push_back({"all inactive", plan_shape(true, 1, 15, 256), 16, std::vector<int>(16, 0), cost_ramp(16), {}});
    // contour classes: 3 of 64 omegas at Re omega > 0 are a minority while their class has no cache, 5 are not
    v.push_back({"minority 3 of 64", plan_shape(true, 1, 15, 48), 64, {}, {}, {}, 3, {true, false}});
    v.push_back({"minority 3 of 64, cached", plan_shape(true, 1, 15, 48), 64, {}, {}, {}, 3, {true, true}});
    v.push_back({"5 of 64", plan_shape(true, 1, 15, 48), 64, {}, {}, {}, 5, {true, false}});
    return v;
}

struct PlanExpected {
    const char* name;
    std::vector<int> order;
    int n_wide;
    std::vector<int> chunks;  // (first, size) per chunk
    int items_per_group;
    bool union_walk;
    int count[2], minority;
};

static void check_fill_plans() {
    const std::vector<PlanExpected> expected = {
        {"headline",
         {100, 7, 127, 126, 125, 124, 123, 122, 121, 120, 119, 118, 117, 116, 115, 114, 113, 112, 111, 110, 109, 108, 107, 106, 105, 104, 103, 102, 101, 99, 98, 97,
          96, 95, 94, 93, 92, 91, 90, 89, 88, 87, 86, 85, 84, 83, 82, 81, 80, 79, 78, 77, 76, 75, 74, 73, 72, 71, 70, 69, 68, 67, 66, 65,
          64, 63, 62, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52, 51, 50, 49, 48, 47, 46, 45, 44, 43, 42, 41, 40, 39, 38, 37, 36, 35, 34, 33,
          32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 6, 5, 4, 3, 2, 0, 1},
         2, {0, 1, 1, 1, 2, 8, 10, 8, 18, 8, 26, 8, 34, 16, 50, 16, 66, 16, 82, 16, 98, 16, 114, 14},
         3, true, {128, 0}, -1},
        {"headline, 5 live",
         {127, 90, 41, 40, 3},
         0, {0, 2, 2, 3},
         2, true, {5, 0}, -1},
        {"headline, 5 live, narrow chunks",
         {127, 90, 41, 40, 3},
         0, {0, 2, 2, 2, 4, 1},
         2, true, {5, 0}, -1},
        {"headline, union walk",
         {127, 90, 41, 40, 3},
         0, {0, 5},
         2, true, {5, 0}, -1},
        {"electromagnetic tiled",
         {22, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 0, 1},
         0, {0, 2, 2, 2, 4, 2, 6, 2, 8, 2, 10, 2, 12, 2, 14, 2, 16, 2, 18, 2, 20, 2, 22, 1},
         2, false, {23, 0}, -1},
        {"GK31 lanes",
         {69, 68, 67, 66, 65, 64, 63, 62, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52, 51, 50, 49, 48, 47, 46, 45, 44, 43, 42, 41, 40, 39, 38,
          37, 36, 35, 34, 33, 32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6,
          5, 4, 3, 2, 0, 1},
         0, {0, 4, 4, 8, 12, 8, 20, 16, 36, 32, 68, 2},
         1, false, {70, 0}, -1},
        {"no costs",
         {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
          32, 33, 34, 35, 36, 37, 38, 39},
         0, {0, 16, 16, 16, 32, 8},
         2, true, {40, 0}, -1},
        {"all inactive",
         {},
         0, {},
         0, false, {0, 0}, -1},
        {"minority 3 of 64",
         {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
          32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63},
         0, {0, 2, 2, 2, 4, 2, 6, 2, 8, 2, 10, 2, 12, 2, 14, 2, 16, 2, 18, 2, 20, 2, 22, 2, 24, 2, 26, 2, 28, 2, 30, 2,
          32, 2, 34, 2, 36, 2, 38, 2, 40, 2, 42, 2, 44, 2, 46, 2, 48, 2, 50, 2, 52, 2, 54, 2, 56, 2, 58, 2, 60, 2, 62, 2},
         3, true, {61, 3}, 1},
        {"minority 3 of 64, cached",
         {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
          32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63},
         0, {0, 2, 2, 2, 4, 2, 6, 2, 8, 2, 10, 2, 12, 2, 14, 2, 16, 2, 18, 2, 20, 2, 22, 2, 24, 2, 26, 2, 28, 2, 30, 2,
          32, 2, 34, 2, 36, 2, 38, 2, 40, 2, 42, 2, 44, 2, 46, 2, 48, 2, 50, 2, 52, 2, 54, 2, 56, 2, 58, 2, 60, 2, 62, 2},
         3, true, {61, 3}, -1},
        {"5 of 64",
         {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
          32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63},
         0, {0, 2, 2, 2, 4, 2, 6, 2, 8, 2, 10, 2, 12, 2, 14, 2, 16, 2, 18, 2, 20, 2, 22, 2, 24, 2, 26, 2, 28, 2, 30, 2,
          32, 2, 34, 2, 36, 2, 38, 2, 40, 2, 42, 2, 44, 2, 46, 2, 48, 2, 50, 2, 52, 2, 54, 2, 56, 2, 58, 2, 60, 2, 62, 2},
         3, true, {59, 5}, -1},
    };
    const std::vector<PlanCase> cases = plan_cases();
    CHECK(cases.size() == expected.size());
    for (size_t k = 0; k < cases.size() && k < expected.size(); ++k) {
        const PlanCase& pc = cases[k];
        const PlanExpected& e = expected[k];
        CHECK(std::strcmp(pc.name, e.name) == 0);
        std::vector<int> order, chunks;
        const int n_wide = emme::plan_order(pc.nbatch, pc.active.empty() ? nullptr : pc.active.data(),
                                            pc.cost.empty() ? nullptr : pc.cost.data(),
                                            pc.wide.empty() ? nullptr : pc.wide.data(), order);
        CHECK(order == e.order && n_wide == e.n_wide);
        if (order.empty()) {  // nothing to launch: the dispatcher returns before it plans anything else
            CHECK(e.chunks.empty());
            continue;
        }
        const std::vector<double> w = pc.omegas();
        const emme::ClassCensus cls = emme::plan_classes(order, w.data(), pc.has_cache);
        CHECK(cls.count[0] == e.count[0] && cls.count[1] == e.count[1] && cls.minority == e.minority);
        const emme::ChunkPlan plan = emme::plan_chunks(pc.s, order, pc.cost.empty() ? nullptr : pc.cost.data(), n_wide, chunks);
        const int n = (int)order.size();
        CHECK(plan.nchunks == (int)e.chunks.size() / 2 && plan.items_per_group == e.items_per_group && plan.union_walk == e.union_walk);
        CHECK((int)chunks.size() == 2 * plan.nchunks + (pc.s.tiled ? n : 0));
        CHECK(std::vector<int>(chunks.begin(), chunks.begin() + 2 * plan.nchunks) == e.chunks);
        // the chunks tile the order without gap or overlap, the wide items first and one per chunk, none wider
        // than the kernel's columns; every map entry names its own chunk and column
        int next = 0;
        for (int q = 0; q < plan.nchunks; ++q) {
            const int first = chunks[2 * q], size = chunks[2 * q + 1];
            CHECK(first == next && size >= 1 && size <= (pc.s.tiled ? 16 / pc.s.nm : pc.s.lane_group()));
            if (q < n_wide) CHECK(size == 1 && pc.wide[order[first]] != 0);
            for (int col = 0; pc.s.tiled && col < size; ++col) CHECK(chunks[2 * plan.nchunks + first + col] == ((q << 8) | col));
            next = first + size;
        }
        CHECK(next == n);
        for (int pos = n_wide; pos < n; ++pos) CHECK(pc.wide.empty() || pc.wide[order[pos]] == 0);
    }
    // integrals per lane group of the uncached kernels (headline shape: 128 omegas omega-lane, one omega on nodes)
    const emme::FillShape head = plan_shape(true, 1, 15, 256);
    CHECK(emme::items_per_group_for(head, 128 / 16) == 4 && emme::items_per_group_for(head, 1) == 1);
    CHECK(emme::items_per_group_for(plan_shape(false, 3, 31, 512), 64) == 8);
    CHECK(emme::contour_class(-0.8) == 0 && emme::contour_class(0.5) == 1 && emme::contour_class(0.0) == 1 &&
          emme::contour_class(-0.0) == 0);
}

static const char* kInput =
    "{ \"conf\": \"tokamak\", \"method\": \"eigen\", \"iteration_method\": \"TraceSecant\", \"q\": 1.4, \"shat\": 0.78,"
    " \"tau\": 1.0, \"epsilon_n\": 0.45, \"epsilon_r\": 0.0, \"eta_i\": 3.13, \"eta_e\": 3.13, \"k_rho\": 0.3182,"
    " \"beta_e\": 0.0, \"R\": 1.0, \"vt\": 1.0, \"length\": 14.0, \"theta\": 0.0, \"npoints\": 24,"
    " \"omega_d_coeff\": 1.01, \"water_bag_weight_vpara\": 1.0, \"water_bag_weight_vperp\": 1.0,"
    " \"drift_center_transformation_switch\": true, \"iteration_step_limit\": 20, \"iteration_precision\": 1.0e-6,"
    " \"integration_precision\": 1e-6, \"integration_accuracy\": 1.0e-9, \"integration_iteration_limit\": 20,"
    " \"integration_start_points\": 15, \"arc_coeff\": 1.0, \"initial_guess\": [-0.8, 0.25], \"q\": 9.9 }";

int main() {
    // parameters: the reference's dialect -- a number without '.' is an INTEGER ("1e-6" -> 1),
    // the first of duplicate keys wins
    emme_params_t p;
    std::memset(&p, 0, sizeof p);
    CHECK(emme_params_from_json(kInput, &p) == EMME_OK);
    CHECK(p.npoints == 24 && p.q == 1.4 && p.integration_precision == 1.0 && p.integration_accuracy == 1.0e-9);
    CHECK(p.iteration_method == EMME_METHOD_TRACE_SECANT && p.conf == EMME_CONF_TOKAMAK);
    CHECK(std::fabs(p.b_theta - 0.3182 * 0.3182) < 1e-15);
    // errors keep the reference's texts
    CHECK(emme_params_from_json("{ \"conf\": \"tokamak\" }", &p) == EMME_EJSON);
    CHECK(std::strstr(emme_last_error(), "Failed to accessing key") != nullptr);
    CHECK(emme_params_from_json("{ \"conf\": ", &p) == EMME_EJSON);
    CHECK(emme_params_from_json("", &p) == EMME_EJSON);
    CHECK(emme_params_from_json(nullptr, &p) == EMME_EINVAL);
    // tables and weights
    CHECK(emme_params_from_json(kInput, &p) == EMME_OK);
    std::vector<double> eta(p.npoints), g(p.npoints), b(p.npoints);
    double dx = 0.0;
    CHECK(emme_tables(&p, eta.data(), g.data(), b.data(), &dx) == EMME_OK);
    CHECK(std::fabs(eta.front() + 14.0) < 1e-15 && std::fabs(eta.back() - 14.0) < 1e-12);
    CHECK(std::fabs(dx - 28.0 / 23.0) < 1e-15);
    CHECK(emme_weight(24, 0, 1) == 2.951388888888883 && emme_weight(24, 0, 10) == 1.0);
    CHECK(emme_weight(24, 3, 23) == 0.5);
    // scan generator (src/main.cpp:139-172, 264-324): head, then towards tail0, then (turning
    // point) from the head towards tail1
    double vals[64];
    int turn[64];
    int n = emme_scan_values(1.01, 0.1, 0.91, 0.01, vals, turn, 64);
    CHECK(n >= 2 && n <= 64 && vals[0] == 1.01);
    for (int k = 0; k < n; ++k) CHECK(vals[k] > 0.0 && vals[k] < 1.02 && (turn[k] == 0 || turn[k] == 1));
    CHECK(emme_scan_values(1.01, 0.1, 0.91, 0.01, vals, turn, 3) == 3);       // truncated to the buffer
    CHECK(emme_scan_values(1.01, 0.1, 0.91, 0.01, nullptr, nullptr, 64) == n);  // counting only
    // null vector of a rank-deficient complex symmetric matrix
    const int m = 9;
    std::vector<std::complex<double>> X(m * m), A(m * m, 0.0), v(m);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1 << 24) - 0.5; };
    for (auto& x : X) x = {rnd(), rnd()};
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j)
            for (int k = 0; k < m - 1; ++k)  // the last "eigenvalue" is zero
                A[i * m + j] += X[i * m + k] * std::complex<double>(1.0 + k, 0.3 * k) * X[j * m + k];
    CHECK(emme_null_vector(reinterpret_cast<double*>(A.data()), m, reinterpret_cast<double*>(v.data())) == EMME_OK);
    double res = 0.0, nv = 0.0, na = 0.0;
    for (int i = 0; i < m; ++i) {
        std::complex<double> r = 0.0;
        for (int j = 0; j < m; ++j) r += A[i * m + j] * v[j], na = std::fmax(na, std::abs(A[i * m + j]));
        res = std::fmax(res, std::abs(r));
        nv += std::norm(v[i]);
    }
    CHECK(std::fabs(nv - 1.0) < 1e-12 && res < 1e-7 * na);
    // driver: wrong method is refused with the reference's text; a good input reaches the
    // (stubbed) device and the failure comes back as an error, not a crash or a leak
    char* out = nullptr;
    std::string bad(kInput);
    bad.replace(bad.find("\"eigen\""), 7, "\"PIC\"");
    CHECK(emme_run_json(bad.c_str(), nullptr, &out) == EMME_EJSON && out == nullptr);
    CHECK(std::strstr(emme_last_error(), "Method 'PIC' is not supported") != nullptr);
    const int rc = emme_run_json(kInput, nullptr, &out);
    CHECK(rc != EMME_OK || out != nullptr);
    if (out) emme_free(out);
    check_fill_plans();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("host self-test ok (ASan + UBSan clean)");
    return 0;
}
