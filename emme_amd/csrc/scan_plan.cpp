// scan_plan.cpp -- the round plan of the lock-step scan driver (scan_plan.hpp) and its host-only export for tests,
// emme_scan_plan.
#include "scan_plan.hpp"

#include <algorithm>
#include <stdexcept>

#include "../../include/emme_hip.h"

namespace emme {

void set_error(const std::string& msg);

std::vector<ScanAxis> scan_axes(const JsonValue& all) {
    std::vector<ScanAxis> axes;
    for (const auto& m : all.members) {
        if (!m.second.is_object()) continue;
        ScanAxis a;
        a.key = m.first;
        a.head = m.second.at("head").number();
        a.head_is_int = m.second.at("head").kind == JsonValue::Int;
        a.step = m.second.at("step").number();
        const JsonValue& tail = m.second.at("tail");
        if (tail.is_array()) {
            a.t0 = tail.at((size_t)0).number();
            a.t1 = tail.at((size_t)1).number();
        } else {
            a.t0 = tail.number();
            a.t1 = a.head + .5 * std::copysign(a.step, a.head - a.t0);
        }
        axes.push_back(a);
    }
    return axes;
}

namespace {

// the value a point's parameter set gets: an integer head truncates every scan value (include/JsonParser.h:176-186)
double set_value(const ScanAxis& a, double v) { return a.head_is_int ? (double)(int)v : v; }

bool fixes_shape_or_call(const std::string& key) {
    return key == "npoints" || key == "integration_start_points" || key == "iteration_method" ||
           key == "iteration_precision" || key == "iteration_step_limit";
}

}  // namespace

ScanPlan make_scan_plan(const JsonValue& all) {
    ScanPlan plan;
    plan.axes = scan_axes(all);
    int longest = -1;
    for (size_t a = 0; a < plan.axes.size(); ++a) {
        ScanAxis& ax = plan.axes[a];
        ScanGen gen(ax.head, ax.step, ax.t0, ax.t1);
        bool cont, turning;
        double value;
        gen.next(cont, turning, value);
        const size_t first = plan.points.size();
        int line = 0, in_line = 0;  // points of the current line so far (the head counts for neither)
        int line_len[2] = {0, 0};
        while (cont) {
            ScanPoint p;
            p.axis = (int)a, p.index = (int)(plan.points.size() - first), p.value = value;
            if (turning) line = 1, in_line = 0;
            p.line = line;
            if (p.index == 0) {
                p.round = 0, p.pred = -1;
            } else {
                ++in_line;
                p.round = in_line;
                p.pred = in_line == 1 ? 0 : p.index - 1;
                line_len[line] = in_line;
            }
            plan.points.push_back(p);
            gen.next(cont, turning, value);
        }
        ax.sequential = fixes_shape_or_call(ax.key);
        if (ax.key == "beta_e") {  // through zero: the matrix doubles its order
            const bool es = set_value(ax, ax.head) == 0.0;
            for (size_t k = first; k < plan.points.size(); ++k)
                if ((set_value(ax, plan.points[k].value) == 0.0) != es) ax.sequential = true;
        }
        if (ax.sequential) {
            for (size_t k = first; k < plan.points.size(); ++k) plan.points[k].round = -1;
        } else if (plan.points.size() > first) {
            longest = std::max(longest, std::max(line_len[0], line_len[1]));
        }
    }
    plan.nrounds = longest + 1;
    return plan;
}

}  // namespace emme

extern "C" int emme_scan_plan(const char* input_text, int max_points, int* axis, int* index, int* round, int* pred,
                              int max_axes, int* sequential, int* n_axes, int* n_rounds) {
    if (!input_text || max_points < 0 || max_axes < 0) return EMME_EINVAL;
    try {
        const emme::ScanPlan plan = emme::make_scan_plan(emme::json_parse(input_text, "input.json"));
        const int np = (int)std::min<size_t>(plan.points.size(), (size_t)max_points);
        for (int k = 0; k < np; ++k) {
            const emme::ScanPoint& p = plan.points[k];
            if (axis) axis[k] = p.axis;
            if (index) index[k] = p.index;
            if (round) round[k] = p.round;
            if (pred) pred[k] = p.pred;
        }
        const int na = (int)std::min<size_t>(plan.axes.size(), (size_t)max_axes);
        for (int a = 0; a < na; ++a)
            if (sequential) sequential[a] = plan.axes[a].sequential ? 1 : 0;
        if (n_axes) *n_axes = (int)plan.axes.size();
        if (n_rounds) *n_rounds = plan.nrounds;
        return (int)plan.points.size();
    } catch (const std::exception& e) {
        emme::set_error(e.what());
        return EMME_EJSON;
    }
}
