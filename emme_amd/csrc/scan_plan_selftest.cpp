// scan_plan_selftest.cpp -- the round plan of the lock-step scan driver (scan_plan.cpp): every point
// of an axis' value sequence exactly once, each continuing from the previous point of its line, the second direction
// from the head, as many rounds as the longest line + 1, and the axes that cannot ride along left out.  Built without
// device code and run under AddressSanitizer + UBSan by `make -C emme_amd/csrc host-sanitize`.
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "scan_plan.hpp"

namespace emme {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace emme

static int failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                                 \
        }                                                                               \
    } while (0)

// the value sequence of one axis, as emme_scan_values gives it (host_driver.cpp)
static std::vector<double> values_of(const emme::ScanAxis& a, std::vector<int>& turning) {
    emme::ScanGen gen(a.head, a.step, a.t0, a.t1);
    std::vector<double> v;
    bool cont, turn;
    double x;
    gen.next(cont, turn, x);
    while (cont) {
        v.push_back(x), turning.push_back(turn ? 1 : 0);
        gen.next(cont, turn, x);
    }
    return v;
}

int main() {
    const std::string text =
        "{\"method\": \"eigen\", \"initial_guess\": [-0.8, 0.25], \"npoints\": {\"head\": 24, \"step\": 8, \"tail\": 40},"
        " \"omega_d_coeff\": {\"head\": 1.01, \"step\": 0.1, \"tail\": [0.81, 1.21]},"
        " \"eta_i\": {\"head\": 2.5, \"step\": 0.25, \"tail\": 3.5},"
        " \"iteration_precision\": {\"head\": 1.0e-6, \"step\": 1.0e-6, \"tail\": 3.0e-6},"
        " \"beta_e\": {\"head\": 0.0, \"step\": 0.01, \"tail\": 0.02}, \"q\": 1.4}";
    const emme::ScanPlan plan = emme::make_scan_plan(emme::json_parse(text));
    CHECK(plan.axes.size() == 5);
    CHECK(plan.axes[0].key == "npoints" && plan.axes[0].sequential);
    CHECK(plan.axes[1].key == "omega_d_coeff" && !plan.axes[1].sequential);
    CHECK(plan.axes[2].key == "eta_i" && !plan.axes[2].sequential);
    CHECK(plan.axes[3].key == "iteration_precision" && plan.axes[3].sequential);
    CHECK(plan.axes[4].key == "beta_e" && plan.axes[4].sequential);  // 0 -> 0.01: through zero
    int longest = 0;
    size_t at = 0;
    for (size_t a = 0; a < plan.axes.size(); ++a) {
        std::vector<int> turning;
        const std::vector<double> v = values_of(plan.axes[a], turning);
        int in_line = 0;
        for (size_t k = 0; k < v.size(); ++k, ++at) {
            CHECK(at < plan.points.size());
            if (at >= plan.points.size()) break;
            const emme::ScanPoint& p = plan.points[at];
            CHECK(p.axis == (int)a && p.index == (int)k && p.value == v[k]);
            if (turning[k]) in_line = 0;
            const int want_pred = k == 0 ? -1 : (in_line == 0 ? 0 : (int)k - 1);
            CHECK(p.pred == want_pred);
            if (k > 0) ++in_line;
            CHECK(p.round == (plan.axes[a].sequential ? -1 : in_line));
            if (!plan.axes[a].sequential && in_line > longest) longest = in_line;
            // a point's predecessor is solved in an earlier round
            if (p.round > 0) CHECK(plan.points[at - k + p.pred].round < p.round);
        }
    }
    CHECK(at == plan.points.size());
    CHECK(plan.nrounds == longest + 1);
    CHECK(longest == 4);  // eta_i: 2.5 -> 3.5 in steps of 0.25

    // the C export: the same numbers, clipped to the caller's arrays
    int axis[4], index[4], round[4], pred[4], seq[2], na = 0, nr = 0;
    const int np = emme_scan_plan(text.c_str(), 4, axis, index, round, pred, 2, seq, &na, &nr);
    CHECK(np == (int)plan.points.size() && na == 5 && nr == plan.nrounds);
    for (int k = 0; k < 4; ++k) CHECK(axis[k] == plan.points[k].axis && round[k] == plan.points[k].round);
    CHECK(seq[0] == 1 && seq[1] == 0);
    CHECK(emme_scan_plan(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == EMME_EINVAL);
    CHECK(emme_scan_plan("{\"a\": {\"head\": 1.0}}", 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) ==
          EMME_EJSON);
    // no axis: nothing to plan
    CHECK(emme::make_scan_plan(emme::json_parse("{\"q\": 1.4}")).nrounds == 0);

    if (failures) {
        std::fprintf(stderr, "scan_plan_selftest: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("scan_plan_selftest: ok\n");
    return 0;
}
