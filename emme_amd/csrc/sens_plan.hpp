// sens_plan.hpp -- host plan of emme_root_sensitivities_sets: how many matrices a call holds at once,
// the chunks its fills run in, and the rule that tells a form at its own rounding level.  Plain C++ (sens_plan.cpp),
// under the sanitizer build through sens_plan_selftest.cpp; the rule is shared with the finish kernel of sym_forms.hip.
#pragma once
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define EMME_SENS_HD __host__ __device__
#else
#define EMME_SENS_HD
#endif

namespace emme {

// max_items = 0: the matrices of SENS_AUTO_BYTES, at least one pair's two and at most SENS_AUTO_MAX_ITEMS (the batch
// scratch of a fill grows with the item count)
constexpr size_t SENS_AUTO_BYTES = (size_t)1 << 30;
constexpr int SENS_AUTO_MAX_ITEMS = 4096;

// A call works on the `good` roots (those with a finite eigenpair) in their order.  A base chunk is a run of roots:
// one derivative fill gives M and M' of each, two matrices per root.  A neighbour chunk is a run of (root, direction)
// pairs in row-major order -- pair q is root q / ndir, direction q % ndir -- and one plain fill gives the two
// neighbour matrices of each.  A chunk may begin and end inside a root's directions.
struct SensChunk {
    int first, count;
};
struct SensPlan {
    int cap = 0;  // matrices held at once: always even, >= 2
    std::vector<SensChunk> base;   // over roots
    std::vector<SensChunk> pairs;  // over (root, direction) pairs; empty when ndir = 0
};

// The cap a call runs under.  max_items = 0 is the automatic budget above; a cap below one pair's two matrices (1) is
// rounded UP to one pair, an odd cap down to the whole pairs it holds.
int sens_cap(int max_items, int dim);
SensPlan sens_plan(int ngood, int ndir, int max_items, int dim);

// |x^T M' x| <= 64 n eps |M'|_F |x|^2: the form is at its own rounding level (a multiple or defective root, or not an
// eigenvector).  A non-finite operand answers false: that is another failure.
EMME_SENS_HD inline bool sens_form_at_rounding(double abs_form, int n, double fro_mp, double vnorm2) {
    const double eps = 2.220446049250313e-16;
    return abs_form <= 64.0 * n * eps * fro_mp * vnorm2;
}

}  // namespace emme
