// host_pair_list_selftest.cpp -- the half pair list of mirror-image couples (pair_list.hpp): every
// pair (i < j) is in the half list or the mirror of exactly one entry that is not its own mirror; the length matches the
// closed form; the order is the full list's.  Also the symmetry test of the grid tables.  Plain C++ with its own main
// (make host-sanitize runs it under AddressSanitizer + UBSan).
#include <cstdio>
#include <vector>

#include "pair_list.hpp"

using namespace emme;

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_fail;                                                     \
        }                                                                 \
    } while (0)

static void check_lists(int N) {
    std::vector<PairIJ> full, half;
    full_pair_list(N, full);
    half_pair_list(N, half);
    CHECK((long)full.size() == (long)N * (N - 1) / 2);
    CHECK((long)half.size() == half_pair_count(N));
    // covered[i][j]: times (i, j) is written -- by its own entry, or as the mirror of an entry that is not self-mirror
    std::vector<int> covered((size_t)N * N, 0);
    int self_mirror = 0;
    long prev_key = -1;
    for (const PairIJ& p : half) {
        const int i = p.x, j = p.y;
        CHECK(i < j && j < N);
        const long key = (long)(j - i) * N + i;  // diagonal-offset order, as the full list
        CHECK(key > prev_key);
        prev_key = key;
        ++covered[(size_t)i * N + j];
        if (i + j == N - 1) {
            ++self_mirror;
            continue;
        }
        const int i2 = N - 1 - j, j2 = N - 1 - i;
        CHECK(i2 >= 0 && i2 < j2 && j2 < N);
        CHECK(j2 - i2 == j - i);  // same diagonal: same band weight
        ++covered[(size_t)i2 * N + j2];
    }
    CHECK(self_mirror == N / 2);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) CHECK(covered[(size_t)i * N + j] == (i < j ? 1 : 0));
    // the half list is a subsequence of the full one
    size_t q = 0;
    for (const PairIJ& p : full)
        if (q < half.size() && half[q].x == p.x && half[q].y == p.y) ++q;
    CHECK(q == half.size());
}

static void check_symmetry() {
    const int N = 25;
    std::vector<double> tab(3 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        const double x = i - 0.5 * (N - 1);
        tab[i] = 0.37 * x, tab[N + i] = x * x * x - 2.0 * x, tab[2 * N + i] = 1.0 + 0.1 * x * x;
    }
    CHECK(grid_is_mirror_symmetric(tab.data(), N, 1e-13));
    std::vector<double> t = tab;
    t[3] *= 1.0 + 1e-15;  // rounding noise of a table
    CHECK(grid_is_mirror_symmetric(t.data(), N, 1e-13));
    for (int k = 0; k < 3; ++k) {  // a real asymmetry in any one table
        t = tab;
        t[(size_t)k * N + 3] += 1e-6;
        CHECK(!grid_is_mirror_symmetric(t.data(), N, 1e-13));
    }
    t = tab;
    for (int i = 0; i < N; ++i) t[2 * N + i] = 0.1 * (i - 0.5 * (N - 1));  // b odd instead of even
    CHECK(!grid_is_mirror_symmetric(t.data(), N, 1e-13));
    t = tab;
    t[N + 1] = std::nan("");
    CHECK(!grid_is_mirror_symmetric(t.data(), N, 1e-13));
}

int main() {
    for (int N : {2, 3, 16, 24, 25, 255, 256}) check_lists(N);
    CHECK(half_pair_count(256) == 16384);
    check_symmetry();
    if (g_fail) {
        std::printf("host_pair_list_selftest: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("host_pair_list_selftest: ok\n");
    return 0;
}
