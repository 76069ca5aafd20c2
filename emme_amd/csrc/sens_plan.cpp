// sens_plan.cpp -- the chunk plan of emme_root_sensitivities_sets (sens_plan.hpp).  No device.
#include "sens_plan.hpp"

#include <algorithm>

namespace emme {

int sens_cap(int max_items, int dim) {
    if (max_items <= 0) {
        const size_t per = (size_t)std::max(dim, 1) * (size_t)std::max(dim, 1) * 16;
        const size_t fit = SENS_AUTO_BYTES / per;
        max_items = (int)std::min<size_t>(fit, (size_t)SENS_AUTO_MAX_ITEMS);
    }
    return std::max(2, max_items - max_items % 2);
}

namespace {

void runs(int total, int per, std::vector<SensChunk>& out) {
    for (int first = 0; first < total; first += per) out.push_back({first, std::min(per, total - first)});
}

}  // namespace

SensPlan sens_plan(int ngood, int ndir, int max_items, int dim) {
    SensPlan p;
    p.cap = sens_cap(max_items, dim);
    if (ngood < 1) return p;
    const int per = p.cap / 2;  // roots of a base chunk = pairs of a neighbour chunk: two matrices each
    runs(ngood, per, p.base);
    if (ndir > 0) runs(ngood * ndir, per, p.pairs);
    return p;
}

}  // namespace emme
