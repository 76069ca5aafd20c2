// step_feedback.hpp -- what a root search learns from the fill of one step and hands to the next (plain C++, no
// HIP): every item's cost (interval count of its last fill, which orders the omegas), the items that take the
// wide-list build of the dense fill, and the count of deferred integrals.  Both search loops (ctx_search.hip) feed
// it; the fill dispatcher (ctx_fill.hip) reads it; host_selftest.cpp pins the rule.
#pragma once
#include <vector>

namespace emme {

struct StepFeedback {
    std::vector<unsigned long long> iv_prev, cost;  // running interval counter at the last take; cost of the last fill
    std::vector<unsigned char> wide;  // items whose chunks take the 128-entry build of the dense fill (root search)
    unsigned int last_deferred = 0;   // integrals the previous cached fill deferred
    bool pub_valid = false;           // last_deferred holds the previous fill's count (taken here, not yet used)

    void begin(int n) { iv_prev.assign(n, 0), cost.assign(n, 0), wide.assign(n, 0); }

    // iv: every item's running interval counter.  A counter that moved gives the item's new cost, one that did not
    // (the item was not filled) keeps the old.  overflow, if given: integrals per item that did not fit the
    // 64-entry level lists; an eighth of the item's npairs makes it wide for the rest of the search.  deferred, if
    // given: the fill's deferred count.
    void take(const unsigned long long* iv, const unsigned int* overflow = nullptr, int npairs = 0,
              const unsigned int* deferred = nullptr) {
        for (size_t b = 0; b < iv_prev.size(); ++b) {
            if (overflow && overflow[b] * 8u >= (unsigned)npairs) wide[b] = 1;
            if (iv[b] != iv_prev[b]) cost[b] = iv[b] - iv_prev[b];
            iv_prev[b] = iv[b];
        }
        if (deferred) last_deferred = *deferred, pub_valid = true;
    }
};

}  // namespace emme
