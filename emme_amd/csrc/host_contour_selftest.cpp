// host_contour_selftest.cpp -- the host half of the contour eigensolver (host_contour.cpp: one-sided Jacobi SVD, the
// Hessenberg + shifted QR eigenvalues, the winding arithmetic) built without device code and run under AddressSanitizer
// + UBSan by `make -C emme_amd/csrc host-sanitize`, on sizes from 1 to the 64-probe cap, rank-deficient and zero
// moments, fewer eigenvalue slots than the rank, and bad arguments.
#include <cmath>
#include <complex>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "host_contour.hpp"

namespace emme {
void set_error(const std::string&) {}
}  // namespace emme

static int failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                                 \
        }                                                                               \
    } while (0)

using cd = std::complex<double>;

// deterministic pseudo-random numbers in [-1, 1)
static double rnd(unsigned long long& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * 0x1.0p-53 * 2.0 - 1.0;
}

// A0 = U S W^H, A1 = U diag(lam) S W^H with U (n x k), W (L x k) of orthonormal columns (Gram-Schmidt), S = diag(sig)
static void moments(int n, int L, int k, const std::vector<cd>& lam, std::vector<cd>& A0, std::vector<cd>& A1,
                    unsigned long long seed) {
    auto orth = [&](int rows, std::vector<std::vector<cd>>& Q) {
        Q.assign(k, std::vector<cd>(rows));
        for (int j = 0; j < k; ++j) {
            for (auto& v : Q[j]) v = cd(rnd(seed), rnd(seed));
            for (int p = 0; p < j; ++p) {
                cd d = 0.0;
                for (int i = 0; i < rows; ++i) d += std::conj(Q[p][i]) * Q[j][i];
                for (int i = 0; i < rows; ++i) Q[j][i] -= d * Q[p][i];
            }
            double nr = 0.0;
            for (auto& v : Q[j]) nr += std::norm(v);
            for (auto& v : Q[j]) v /= std::sqrt(nr);
        }
    };
    std::vector<std::vector<cd>> U, W;
    orth(n, U);
    orth(L, W);
    A0.assign((size_t)n * L, 0.0);
    A1.assign((size_t)n * L, 0.0);
    for (int j = 0; j < k; ++j) {
        const double sig = std::pow(10.0, -2.0 * j / std::max(1, k));
        for (int i = 0; i < n; ++i)
            for (int l = 0; l < L; ++l) {
                const cd t = U[j][i] * sig * std::conj(W[j][l]);
                A0[(size_t)i * L + l] += t;
                A1[(size_t)i * L + l] += lam[j] * t;
            }
    }
}

int main() {
    // rank k < L: every eigenvalue of diag(lam) back, the rank found, the singular values descending
    const int shapes[][3] = {{1, 1, 1}, {3, 7, 3}, {50, 7, 5}, {50, 64, 20}, {70, 64, 64}};
    for (const auto& sh : shapes) {
        const int n = sh[0], L = sh[1], k = sh[2];
        std::vector<cd> lam(k), A0, A1;
        unsigned long long seed = 1000u + n * 7u + L;
        for (auto& x : lam) x = cd(rnd(seed), rnd(seed));
        moments(n, L, k, lam, A0, A1, seed);
        std::vector<cd> mu(64);
        std::vector<double> sig(L);
        int kk = -1;
        CHECK(emme_contour_eigs(n, L, reinterpret_cast<double*>(A0.data()), reinterpret_cast<double*>(A1.data()), 1e-8, 64,
                                reinterpret_cast<double*>(mu.data()), &kk, sig.data()) == EMME_OK);
        CHECK(kk == k);
        for (int l = 1; l < L; ++l) CHECK(sig[l] <= sig[l - 1]);
        for (int j = 0; j < k; ++j) {
            double best = 1e300;
            for (int q = 0; q < kk; ++q) best = std::min(best, std::abs(mu[q] - lam[j]));
            CHECK(best < 1e-9);
        }
        // fewer slots than the rank: only max_eigs written, the rank still reported
        if (k > 1) {
            std::vector<cd> few(2, cd(7.0, 7.0));
            few.resize(3, cd(9.0, 9.0));
            CHECK(emme_contour_eigs(n, L, reinterpret_cast<double*>(A0.data()), reinterpret_cast<double*>(A1.data()), 1e-8, 2,
                                    reinterpret_cast<double*>(few.data()), &kk, nullptr) == EMME_OK);
            CHECK(kk == k && few[2] == cd(9.0, 9.0));
        }
    }
    // zero moments: rank 0, nothing written
    {
        std::vector<cd> A0(50 * 8, 0.0), mu(64, cd(3.0, 3.0));
        int kk = -1;
        CHECK(emme_contour_eigs(50, 8, reinterpret_cast<double*>(A0.data()), reinterpret_cast<double*>(A0.data()), 1e-8, 64,
                                reinterpret_cast<double*>(mu.data()), &kk, nullptr) == EMME_OK);
        CHECK(kk == 0 && mu[0] == cd(3.0, 3.0));
    }
    // bad arguments
    {
        std::vector<double> A(2 * 4 * 3, 0.0), mu(128);
        int kk = 0;
        CHECK(emme_contour_eigs(0, 3, A.data(), A.data(), 1e-8, 64, mu.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigs(4, 65, A.data(), A.data(), 1e-8, 64, mu.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigs(4, 3, A.data(), A.data(), 0.0, 64, mu.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigs(4, 3, A.data(), A.data(), 1e-8, 0, mu.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigs(4, 3, nullptr, A.data(), 1e-8, 64, mu.data(), &kk, nullptr) == EMME_EINVAL);
    }
    // winding: arg of (z - z0)^2 (z - z1) on the unit circle, z0 inside and z1 outside -> 2; coarse or NaN -> unresolved
    {
        auto args = [](int N, double nan_at) {
            std::vector<double> a(N);
            for (int j = 0; j < N; ++j) {
                const cd z = std::polar(1.0, 2.0 * M_PI * j / N);
                a[j] = j == nan_at ? NAN : std::arg((z - cd(0.2, 0.1)) * (z - cd(0.2, 0.1)) * (z - cd(3.0, 0.0)));
            }
            return a;
        };
        bool res = false;
        double raw = 0.0;
        std::vector<double> a = args(64, -1);
        CHECK(emme::contour_winding(a.data(), 64, 0.5 * M_PI, &res, &raw) == 2 && res && std::fabs(raw - 2.0) < 1e-12);
        a = args(4, -1);
        emme::contour_winding(a.data(), 4, 0.5 * M_PI, &res, &raw);
        CHECK(!res);
        a = args(64, 5);
        CHECK(emme::contour_winding(a.data(), 64, 0.5 * M_PI, &res, nullptr) == -1 && !res);
    }
    // the defaults
    {
        emme_contour_t c;
        emme_contour_default(&c);
        CHECK(c.size == (int)sizeof(emme_contour_t) && c.points >= 4 && c.max_points >= c.points && c.probes >= 1 &&
              c.probes <= 64 && c.rank_tol > 0.0 && c.rank_tol < 1.0);
        emme_contour_default(nullptr);
    }
    if (failures) {
        std::fprintf(stderr, "%d contour self-test failures\n", failures);
        return 1;
    }
    std::printf("contour self-test ok (ASan + UBSan clean)\n");
    return 0;
}
