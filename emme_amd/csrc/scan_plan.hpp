// scan_plan.hpp -- the {head, step, tail} scan generator and the round plan of the lock-step scan driver
// (emme_run_json_lockstep, host_driver.cpp).  Plain host C++: no device, no context.
//
// The sequential driver walks one axis after the other and, on an axis, one point after the other, each from the
// previous point's root.  What it visits falls into LINES (axis, direction) that do not depend on each other: every
// axis restarts from initial_guess, and the second direction of an axis restarts from the root of the axis' head
// (from initial_guess if the head failed).  The plan puts the head of every axis into round 0 and the t-th point of
// every line into round t, so that a round's points can be solved side by side and each finds the root it continues
// from in an earlier round.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_json.hpp"

namespace emme {

// get_scan_generator, src/main.cpp:139-172
struct ScanGen {
    double head, step, left_tail, right_tail, current, current_tail;
    bool to_left = true, is_first = true;
    ScanGen(double h, double s, double l, double r)
        : head(h), step(s), left_tail(l), right_tail(r), current(h), current_tail(l) {}
    bool within() const {
        return std::abs(current - head) <= (std::abs(current_tail - head) + 0.01 * std::abs(step));
    }
    // returns (continue, turning, value)
    void next(bool& cont, bool& turning, double& value) {
        if (!is_first) current += std::copysign(step, (current_tail - head));
        is_first = false;
        if (within()) {
            cont = true, turning = false, value = current;
            return;
        }
        to_left = !to_left;
        current_tail = right_tail;
        current = head + std::copysign(step, (current_tail - head));
        cont = !to_left && within();
        turning = true;
        value = current;
    }
};

// one scan axis: a top-level key of input.json written {head, step, tail} (src/main.cpp:225-242)
struct ScanAxis {
    std::string key;
    double head = 0, step = 0, t0 = 0, t1 = 0;
    bool head_is_int = false;
    // an axis that cannot ride along in a lock-step round: its key changes what all parameter sets of one context
    // share (npoints, beta_e through zero, integration_start_points, iteration_method), or it is iteration_precision /
    // iteration_step_limit, which a search takes per call.  The sequential driver runs it.
    bool sequential = false;
};

// one point an axis visits.  index: its position in the axis' value sequence (emme_scan_values); line: 0 the head
// and the first direction, 1 the second direction; round: -1 on a sequential axis; pred: the index, on the same axis,
// of the point the sequential driver would have solved last before it on this line -- the previous point of the line,
// the head for the first point of either direction, -1 for the head itself (initial_guess)
struct ScanPoint {
    int axis = 0, index = 0, line = 0, round = -1, pred = -1;
    double value = 0;
};

struct ScanPlan {
    std::vector<ScanAxis> axes;     // in input order
    std::vector<ScanPoint> points;  // axis by axis, each in the order of its value sequence
    int nrounds = 0;                // 1 + the longest line of the axes that ride along; 0 if none does
};

// every top-level key of `all` whose value is an object, as the sequential driver reads it (throws like JsonValue)
std::vector<ScanAxis> scan_axes(const JsonValue& all);
ScanPlan make_scan_plan(const JsonValue& all);

}  // namespace emme
