// pair_list.hpp -- the pair lists of a context and the grid symmetry that lets a fill take half of them (DESIGN.md
// 5.0c).  Plain C++, no device: host_pair_list_selftest.cpp runs it under the sanitizers (make host-sanitize).
#pragma once
#include <cmath>
#include <vector>

namespace emme {

// (i, j), i < j: the layout of ushort2, which is what the kernels read the lists as
struct PairIJ {
    unsigned short x, y;
};
static_assert(sizeof(PairIJ) == 4, "PairIJ is uploaded as ushort2");

// Every pair (i < j) ordered by diagonal offset j - i (see assemble.hip header).
inline void full_pair_list(int N, std::vector<PairIJ>& pairs) {
    pairs.clear();
    pairs.reserve((size_t)N * (N - 1) / 2);
    for (int off = 1; off < N; ++off)
        for (int i = 0; i + off < N; ++i) pairs.push_back({(unsigned short)i, (unsigned short)(i + off)});
}

// One pair of every mirror-image couple {(i, j), (N-1-j, N-1-i)}, in the same order: of each diagonal the entries
// with 2 i <= N-1-off.  The entry with 2 i == N-1-off (i + j == N-1) is its own mirror.
inline void half_pair_list(int N, std::vector<PairIJ>& pairs) {
    pairs.clear();
    for (int off = 1; off < N; ++off)
        for (int i = 0; 2 * i <= N - 1 - off; ++i) pairs.push_back({(unsigned short)i, (unsigned short)(i + off)});
}

// its length: (all pairs + the floor(N / 2) self-mirror ones) / 2
inline long half_pair_count(int N) { return ((long)N * (N - 1) / 2 + N / 2) / 2; }

// Is the grid symmetric under i -> N-1-i -- eta and g odd, b even, each to `tol` of the table's largest magnitude?
// tab: eta[N] | g[N] | b[N].  The integrand of a pair depends on the grid through eta_i - eta_j, g_i - g_j, b_i b_j
// and b_i + b_j alone (make_pair_const), which such a grid gives pair (i, j) and its mirror alike.
inline bool grid_is_mirror_symmetric(const double* tab, int N, double tol) {
    const double sign[3] = {1.0, 1.0, -1.0};  // t[i] + sign t[N-1-i] = 0
    for (int k = 0; k < 3; ++k) {
        const double* t = tab + (size_t)k * N;
        double mx = 0.0, err = 0.0;
        for (int i = 0; i < N; ++i) {
            if (!std::isfinite(t[i])) return false;
            mx = std::fmax(mx, std::fabs(t[i]));
            err = std::fmax(err, std::fabs(t[i] + sign[k] * t[N - 1 - i]));
        }
        if (!(err <= tol * mx)) return false;
    }
    return true;
}

}  // namespace emme
