// host_selftest.cpp -- the host layer above the C ABI (JSON dialect reader, parameters, tables,
// scan generator, null vector, driver error paths, the fill planner, the options, the LU workgroup count, a root
// search's step feedback) built WITHOUT the device code and run under
// AddressSanitizer + UBSan:   make -C emme_amd/csrc host-sanitize
// (GPU sanitizers are not available on the target pool; this covers the CPU side.)
// The device entry points the driver calls are stubbed to fail with EMME_EDEVICE, so
// emme_run_json is exercised up to and including its "no device" error record.
#include <cctype>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "fill_plan.hpp"
#include "linstep_plan.hpp"
#include "options.hpp"
#include "step_feedback.hpp"

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
int emme_ctx_bind_param_sets(emme_ctx_t*, const emme_params_t*, int) { return EMME_EDEVICE; }
int emme_solve_roots_sets(emme_ctx_t*, const int*, const double*, int, int, double, int, double*, int*, int*, double*) {
    return EMME_EDEVICE;
}
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

// ---- the options (options.cpp) ---------------------------------------------------------------------------------
struct IntOpt {
    const char* name;  // of the field; "EMME_" + its upper case is the environment override, unless `env` names it
    int emme_options_t::*f;
    int dflt;
    int lo_ok, lo_bad, hi_ok, hi_bad;  // last accepted / first rejected value at either end (kNone: no bound there)
    const char* env;                   // null: irregular override, with a case of its own below
};
struct DblOpt {
    const char* name;
    double emme_options_t::*f;
    double dflt, lo_ok, lo_bad;
    const char* env;
};
static const int kNone = 0x7fffffff;
static const std::vector<IntOpt> kIntOpts = {
    {"cache_min_batch", &emme_options_t::cache_min_batch, 8, 1, 0, kNone, kNone, "EMME_CACHE_MIN_BATCH"},
    {"cache_min_depth", &emme_options_t::cache_min_depth, 0, 0, -1, kNone, kNone, "EMME_CACHE_MIN_DEPTH"},
    {"fill", &emme_options_t::fill, EMME_FILL_AUTO, EMME_FILL_AUTO, -1, EMME_FILL_LANES, 3, nullptr},
    {"phase_table", &emme_options_t::phase_table, 1, kNone, kNone, kNone, kNone, "EMME_PHASE_TABLE"},
    {"em_shared", &emme_options_t::em_shared, 1, kNone, kNone, kNone, kNone, "EMME_EM_SHARED"},
    {"wl_min", &emme_options_t::wl_min, 4, 1, 0, kNone, kNone, "EMME_WL_MIN"},
    {"union_sel", &emme_options_t::union_sel, 2, 1, 0, 4, 5, "EMME_UNION_SEL"},
    {"union_ipg_few", &emme_options_t::union_ipg_few, 2, 1, 0, kNone, kNone, "EMME_UNION_IPG_FEW"},
    {"union_few_chunks", &emme_options_t::union_few_chunks, 3, 0, -1, kNone, kNone, "EMME_UNION_FEW_CHUNKS"},
    {"coop_wide_min", &emme_options_t::coop_wide_min, 4096, -1, -2, kNone, kNone, "EMME_COOP_WIDE_MIN"},
    {"defer_one_group", &emme_options_t::defer_one_group, 0, kNone, kNone, kNone, kNone, nullptr},
    {"dense_min_cols", &emme_options_t::dense_min_cols, 3, 1, 0, 17, 18, "EMME_DENSE_MIN_COLS"},
    {"dense_min_tasks", &emme_options_t::dense_min_tasks, 2000, 0, -1, kNone, kNone, "EMME_DENSE_MIN_TASKS"},
    {"dense_wide", &emme_options_t::dense_wide, 0, kNone, kNone, kNone, kNone, "EMME_DENSE_WIDE"},
    {"skip_lost", &emme_options_t::skip_lost, 1, kNone, kNone, kNone, kNone, "EMME_SKIP_LOST"},
    {"lu_split", &emme_options_t::lu_split, 0, 0, -1, 16, 17, "EMME_LU_SPLIT"},
    {"lu_group_min_n", &emme_options_t::lu_group_min_n, 256, kNone, kNone, kNone, kNone, nullptr},
    {"lu_spin_limit", &emme_options_t::lu_spin_limit, 16000000, 1, 0, kNone, kNone, "EMME_LU_SPIN_LIMIT"},
    {"lu_unblocked", &emme_options_t::lu_unblocked, 0, kNone, kNone, kNone, kNone, nullptr},
    {"deriv_cached", &emme_options_t::deriv_cached, 0, 0, -1, 1, 2, "EMME_DERIV_CACHED"},
    {"tile_uncached", &emme_options_t::tile_uncached, 0, 0, -1, 1, 2, "EMME_TILE_UNCACHED"},
    {"dense_stage", &emme_options_t::dense_stage, 1, 0, -1, 1, 2, "EMME_DENSE_STAGE"},
};
static const std::vector<DblOpt> kDblOpts = {
    {"node_cache_gb", &emme_options_t::node_cache_gb, 176.0, 0.0, -1e-300, "EMME_NODE_CACHE_GB"},
    {"dense_cost_ratio", &emme_options_t::dense_cost_ratio, 4.0, 1e-300, 0.0, "EMME_DENSE_COST_RATIO"},
};
static const char* const kIrregularEnv[] = {"EMME_DENSE", "EMME_UNION", "EMME_DEFER_ONE_GROUP", "EMME_LU_GROUP", "EMME_LU_UNBLOCKED"};

static emme_options_t default_options() {
    emme_options_t o;
    emme::options_default(o);
    return o;
}

// a and b agree in every field but (at most) the one `except` points at
static bool same_options(const emme_options_t& a, const emme_options_t& b, const void* except = nullptr) {
    bool same = a.size == b.size;
    for (const IntOpt& k : kIntOpts) same &= &(a.*k.f) == except || a.*k.f == b.*k.f;
    for (const DblOpt& k : kDblOpts) same &= &(a.*k.f) == except || a.*k.f == b.*k.f;
    return same;
}

// options_default + the environment as it stands
static emme_options_t overridden(int fill = EMME_FILL_AUTO) {
    emme_options_t o = default_options();
    o.fill = fill;
    emme::options_env_overrides(o);
    return o;
}

static void check_options(const emme_params_t& params) {
    for (const IntOpt& k : kIntOpts)
        if (k.env) unsetenv(k.env);
    for (const DblOpt& k : kDblOpts) unsetenv(k.env);
    for (const char* e : kIrregularEnv) unsetenv(e);

    // defaults
    const emme_options_t d = default_options();
    CHECK(d.size == (int)sizeof(emme_options_t) && emme::options_check(&d) == EMME_OK);
    for (const IntOpt& k : kIntOpts) CHECK(d.*k.f == k.dflt);
    for (const DblOpt& k : kDblOpts) CHECK(d.*k.f == k.dflt);
    CHECK(same_options(overridden(), d));  // (an empty environment overrides nothing)

    // bounds: the last accepted and the first rejected value of each
    auto accepts = [&](auto field, auto value) {
        emme_options_t o = d;
        o.*field = value;
        emme::set_error("");
        const int rc = emme::options_check(&o);
        CHECK(rc == EMME_OK || (rc == EMME_EINVAL && std::strcmp(emme_last_error(), "emme_options_t: value out of range") == 0));
        return rc == EMME_OK;
    };
    for (const IntOpt& k : kIntOpts) {
        if (k.lo_ok != kNone) CHECK(accepts(k.f, k.lo_ok) && !accepts(k.f, k.lo_bad));
        if (k.hi_ok != kNone) CHECK(accepts(k.f, k.hi_ok) && !accepts(k.f, k.hi_bad));
    }
    for (const DblOpt& k : kDblOpts) CHECK(accepts(k.f, k.lo_ok) && !accepts(k.f, k.lo_bad) && !accepts(k.f, std::nan("")));
    for (int v = -1; v <= 9; ++v) CHECK(accepts(&emme_options_t::union_sel, v) == (v == 1 || v == 2 || v == 4));
    CHECK(accepts(&emme_options_t::dense_min_cols, 1) && accepts(&emme_options_t::dense_min_cols, 17));
    CHECK(!accepts(&emme_options_t::dense_min_cols, 0) && !accepts(&emme_options_t::dense_min_cols, 18));
    CHECK(accepts(&emme_options_t::lu_split, 0) && accepts(&emme_options_t::lu_split, 16) && !accepts(&emme_options_t::lu_split, 17));
    CHECK(accepts(&emme_options_t::deriv_cached, 1) && !accepts(&emme_options_t::deriv_cached, 2));
    CHECK(!accepts(&emme_options_t::node_cache_gb, std::nan("")));
    {
        emme_options_t o = d;
        o.size = (int)sizeof(emme_options_t) - 4;
        CHECK(emme::options_check(&o) == EMME_EINVAL && std::strstr(emme_last_error(), "size field does not match") != nullptr);
    }

    // environment overrides: the regular ones set their field to the number they hold, and nothing else
    for (const IntOpt& k : kIntOpts) {
        if (!k.env) continue;
        CHECK(std::string(k.env) == "EMME_" + [&] { std::string u(k.name); for (char& ch : u) ch = (char)std::toupper(ch); return u; }());
        setenv(k.env, "7", 1);
        const emme_options_t o = overridden();
        CHECK(o.*k.f == 7 && same_options(o, d, &(o.*k.f)));
        unsetenv(k.env);
    }
    for (const DblOpt& k : kDblOpts) {
        setenv(k.env, "2.5", 1);
        const emme_options_t o = overridden();
        CHECK(o.*k.f == 2.5 && same_options(o, d, &(o.*k.f)));
        unsetenv(k.env);
    }
    // EMME_DENSE=0 acts on FILL_AUTO only; EMME_UNION=0 on every mode, and wins
    setenv("EMME_DENSE", "0", 1);
    CHECK(overridden(EMME_FILL_AUTO).fill == EMME_FILL_UNION && overridden(EMME_FILL_UNION).fill == EMME_FILL_UNION &&
          overridden(EMME_FILL_LANES).fill == EMME_FILL_LANES);
    {
        const emme_options_t o = overridden();
        CHECK(same_options(o, d, &o.fill));
    }
    setenv("EMME_UNION", "0", 1);
    CHECK(overridden(EMME_FILL_AUTO).fill == EMME_FILL_LANES);
    setenv("EMME_DENSE", "1", 1);
    CHECK(overridden(EMME_FILL_AUTO).fill == EMME_FILL_LANES && overridden(EMME_FILL_UNION).fill == EMME_FILL_LANES);
    setenv("EMME_UNION", "1", 1);
    CHECK(same_options(overridden(), d) && overridden(EMME_FILL_UNION).fill == EMME_FILL_UNION);
    unsetenv("EMME_DENSE"), unsetenv("EMME_UNION");
    // EMME_LU_GROUP: zero and below mean "never"
    for (const char* v : {"0", "-3"}) {
        setenv("EMME_LU_GROUP", v, 1);
        const emme_options_t o = overridden();
        CHECK(o.lu_group_min_n == -1 && same_options(o, d, &o.lu_group_min_n));
    }
    setenv("EMME_LU_GROUP", "128", 1);
    CHECK(overridden().lu_group_min_n == 128);
    unsetenv("EMME_LU_GROUP");
    // EMME_DEFER_ONE_GROUP and EMME_LU_UNBLOCKED act by presence, whatever they hold
    for (const char* v : {"", "0", "1"}) {
        setenv("EMME_DEFER_ONE_GROUP", v, 1);
        emme_options_t o = overridden();
        CHECK(o.defer_one_group == 1 && same_options(o, d, &o.defer_one_group));
        unsetenv("EMME_DEFER_ONE_GROUP");
        setenv("EMME_LU_UNBLOCKED", v, 1);
        o = overridden();
        CHECK(o.lu_unblocked == 1 && same_options(o, d, &o.lu_unblocked));
        unsetenv("EMME_LU_UNBLOCKED");
    }
    // an override is taken as it is; the range check that follows it at context creation refuses it
    setenv("EMME_UNION_SEL", "3", 1);
    {
        const emme_options_t o = overridden();
        CHECK(o.union_sel == 3 && emme::options_check(&o) == EMME_EINVAL);
    }
    unsetenv("EMME_UNION_SEL");

    // wants_tiled: both quadrature orders, folded records, goal no tighter than 1e-9, the default fill mode
    emme_params_t p = params;
    p.integration_accuracy = 1e-9;
    for (int pts : {15, 21, 31}) {
        p.integration_start_points = pts;
        CHECK(emme::wants_tiled(p, true, EMME_FILL_AUTO) == (pts != 21));
        CHECK(!emme::wants_tiled(p, false, EMME_FILL_AUTO));
        CHECK(!emme::wants_tiled(p, true, EMME_FILL_UNION) && !emme::wants_tiled(p, true, EMME_FILL_LANES));
    }
    p.integration_accuracy = 9e-10;
    CHECK(!emme::wants_tiled(p, true, EMME_FILL_AUTO));
}

// ---- workgroups per matrix of the blocked LU (linstep_plan.hpp), on 256 compute units ----------------------------
static void check_lu_workgroups() {
    auto nwg = [](int n, int live, int lu_split = 0, bool one_wg = false, bool fits = true) {
        return emme::lu_workgroups(n, live, 256, lu_split, one_wg, fits);
    };
    CHECK(nwg(256, 128) == 2);  // the headline search: two compute units per matrix
    CHECK(nwg(256, 18) == 4);   // a late step: four are enough at this order
    CHECK(nwg(512, 32) == 8);
    CHECK(nwg(768, 4) == 16);
    CHECK(nwg(64, 1) == 1);
    CHECK(nwg(127, 1) == 1 && nwg(128, 1) == 4);
    CHECK(nwg(256, 128, 40) == 16 && nwg(256, 128, 3) == 3);  // pinned, capped at 16
    CHECK(nwg(256, 1, 0, true) == 1 && nwg(256, 1, 8, true) == 1 && nwg(600, 1, 0, true, false) == 1);
    CHECK(nwg(600, 300, 0, false, false) == 2);  // (256 / 300 = 0 -> 1, and the chunked build needs two)
    CHECK(nwg(600, 300, 0, false, true) == 1);
    CHECK(nwg(600, 4, 1, false, false) == 1);    // pinned to one: the caller falls back to the unblocked kernel
}

// ---- a root search's step feedback (step_feedback.hpp): three takes over five items, N = 24 (276 pairs) ---------
static void check_step_feedback() {
    using V = std::vector<unsigned long long>;
    using W = std::vector<unsigned char>;
    const int npairs = 24 * 23 / 2;  // 276 / 8 = 34.5: 34 overflowed integrals stay below the eighth, 35 reach it
    emme::StepFeedback fb;
    fb.begin(5);
    CHECK(fb.cost == V(5, 0) && fb.iv_prev == V(5, 0) && fb.wide == W(5, 0) && !fb.pub_valid);
    // the bootstrap fill, read back by the host itself: counters only
    const V iv1 = {100, 200, 300, 400, 0};
    fb.take(iv1.data());
    CHECK(fb.cost == (V{100, 200, 300, 400, 0}) && fb.iv_prev == iv1 && fb.wide == W(5, 0));
    CHECK(!fb.pub_valid && fb.last_deferred == 0);
    // a step's fill: item 3 was not filled (keeps its cost) and is wide from now on; item 2 just below the threshold
    const V iv2 = {150, 260, 390, 400, 0};
    const std::vector<unsigned int> ov2 = {0, 0, 34, 100, 0};
    unsigned int deferred = 7;
    fb.take(iv2.data(), ov2.data(), npairs, &deferred);
    CHECK(fb.cost == (V{50, 60, 90, 400, 0}) && fb.iv_prev == iv2 && fb.wide == (W{0, 0, 0, 1, 0}));
    CHECK(fb.pub_valid && fb.last_deferred == 7);
    fb.pub_valid = false;  // (the next fill uses the count)
    // the next: item 1 retired, item 2 reaches the threshold, item 3 overflows nothing and stays wide
    const V iv3 = {175, 260, 400, 520, 0};
    const std::vector<unsigned int> ov3 = {0, 0, 35, 0, 0};
    deferred = 0;
    fb.take(iv3.data(), ov3.data(), npairs, &deferred);
    CHECK(fb.cost == (V{25, 60, 10, 120, 0}) && fb.iv_prev == iv3 && fb.wide == (W{0, 0, 1, 1, 0}));
    CHECK(fb.pub_valid && fb.last_deferred == 0);
    // a take without the deferred count (the Newton search's counters travel without overflow counts) leaves both
    fb.pub_valid = false, fb.last_deferred = 9;
    fb.take(iv3.data());
    CHECK(!fb.pub_valid && fb.last_deferred == 9 && fb.cost == (V{25, 60, 10, 120, 0}) && fb.wide == (W{0, 0, 1, 1, 0}));
    fb.begin(2);  // the next search
    CHECK(fb.cost == V(2, 0) && fb.iv_prev == V(2, 0) && fb.wide == W(2, 0));
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
    check_options(p);
    check_lu_workgroups();
    check_step_feedback();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("host self-test ok (ASan + UBSan clean)");
    return 0;
}
