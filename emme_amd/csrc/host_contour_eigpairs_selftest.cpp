// host_contour_eigpairs_selftest.cpp -- the Beyn step with eigenvectors (emme_contour_eigpairs, host_contour.cpp) built
// without device code and run under AddressSanitizer + UBSan by `make -C emme_amd/csrc host-sanitize`: moments
// A0 = sum_j v_j r_j^H, A1 = sum_j lam_j v_j r_j^H with NON-orthogonal v_j (the eigenvectors of a non-normal pencil), from
// order 1 to the 64-probe cap; every returned vector must lie on the v_j of its mu, have unit norm, and mu, k and sigma
// must be emme_contour_eigs' bit for bit.  k = 1 makes B - mu I exactly zero (the perturbed shift); a repeated
// eigenvalue, fewer slots than the rank, vecs = NULL, zero moments and bad arguments are covered too.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
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

static double* dp(std::vector<cd>& v) { return reinterpret_cast<double*>(v.data()); }

// k unit vectors of length n, each random plus `lean` times its predecessor: not orthogonal
static std::vector<std::vector<cd>> leaning(int n, int k, double lean, unsigned long long& seed) {
    std::vector<std::vector<cd>> V(k, std::vector<cd>(n));
    for (int j = 0; j < k; ++j) {
        double nr = 0.0;
        for (int i = 0; i < n; ++i) {
            V[j][i] = cd(rnd(seed), rnd(seed)) + (j > 0 ? lean * V[j - 1][i] * std::sqrt((double)n) : cd(0.0));
            nr += std::norm(V[j][i]);
        }
        for (auto& x : V[j]) x /= std::sqrt(nr);
    }
    return V;
}

static double overlap(const cd* a, const std::vector<cd>& b) {
    cd d = 0.0;
    double na = 0.0, nb = 0.0;
    for (size_t i = 0; i < b.size(); ++i) d += std::conj(a[i]) * b[i], na += std::norm(a[i]), nb += std::norm(b[i]);
    return std::abs(d) / std::sqrt(na * nb);
}

int main() {
    const int shapes[][3] = {{1, 1, 1}, {5, 4, 1}, {5, 4, 3}, {24, 8, 3}, {65, 8, 8}, {70, 64, 20}, {70, 64, 64}};
    for (const auto& sh : shapes) {
        const int n = sh[0], L = sh[1], k = sh[2];
        unsigned long long seed = 77u + n * 13u + L * 5u + k;
        std::vector<cd> lam(k);
        for (auto& x : lam) x = cd(rnd(seed), rnd(seed));
        const std::vector<std::vector<cd>> V = leaning(n, k, k <= 8 ? 0.5 : 0.05, seed), R = leaning(L, k, 0.0, seed);
        std::vector<cd> A0((size_t)n * L, 0.0), A1((size_t)n * L, 0.0);
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < n; ++i)
                for (int l = 0; l < L; ++l) {
                    const cd t = V[j][i] * std::conj(R[j][l]);
                    A0[(size_t)i * L + l] += t, A1[(size_t)i * L + l] += lam[j] * t;
                }
        std::vector<cd> mu(64), mu0(64), vecs((size_t)64 * n, cd(5.0, 5.0));
        std::vector<double> sig(L), sig0(L);
        int kk = -1, kk0 = -1;
        CHECK(emme_contour_eigs(n, L, dp(A0), dp(A1), 1e-8, 64, dp(mu0), &kk0, sig0.data()) == EMME_OK);
        CHECK(emme_contour_eigpairs(n, L, dp(A0), dp(A1), 1e-8, 64, dp(mu), dp(vecs), &kk, sig.data()) == EMME_OK);
        CHECK(kk == k && kk0 == k);
        CHECK(std::memcmp(mu.data(), mu0.data(), sizeof(cd) * k) == 0);
        CHECK(std::memcmp(sig.data(), sig0.data(), sizeof(double) * L) == 0);
        for (int q = 0; q < kk; ++q) {
            int j = 0;
            for (int p = 1; p < k; ++p)
                if (std::abs(mu[q] - lam[p]) < std::abs(mu[q] - lam[j])) j = p;
            CHECK(std::abs(mu[q] - lam[j]) < 1e-8);
            const double ov = overlap(&vecs[(size_t)q * n], V[j]);
            double nr = 0.0;
            for (int i = 0; i < n; ++i) nr += std::norm(vecs[(size_t)q * n + i]);
            CHECK(std::fabs(std::sqrt(nr) - 1.0) < 1e-13);
            if (!(1.0 - ov < 1e-7)) std::fprintf(stderr, "n %d L %d k %d q %d: 1 - overlap %.3e\n", n, L, k, q, 1.0 - ov);
            CHECK(1.0 - ov < 1e-7);
        }
        // rows beyond the rank are not written
        if (kk < 64) CHECK(vecs[(size_t)kk * n] == cd(5.0, 5.0));
        // vecs = NULL is the old function; fewer slots than the rank: only max_eigs rows written
        CHECK(emme_contour_eigpairs(n, L, dp(A0), dp(A1), 1e-8, 64, dp(mu), nullptr, &kk, nullptr) == EMME_OK && kk == k);
        CHECK(std::memcmp(mu.data(), mu0.data(), sizeof(cd) * k) == 0);
        if (k > 2) {
            std::vector<cd> few((size_t)3 * n, cd(9.0, 9.0)), m2(3, cd(9.0, 9.0));
            CHECK(emme_contour_eigpairs(n, L, dp(A0), dp(A1), 1e-8, 2, dp(m2), dp(few), &kk, nullptr) == EMME_OK);
            CHECK(kk == k && m2[2] == cd(9.0, 9.0) && few[(size_t)2 * n] == cd(9.0, 9.0) && few[0] != cd(9.0, 9.0));
            CHECK(std::memcmp(few.data(), vecs.data(), sizeof(cd) * 2 * n) == 0);
        }
    }
    // a repeated eigenvalue: B = lam I on a two-dimensional space; any unit vector of span{v_0, v_1} is an eigenvector
    {
        const int n = 12, L = 4;
        unsigned long long seed = 5;
        const std::vector<std::vector<cd>> V = leaning(n, 2, 0.3, seed), R = leaning(L, 2, 0.0, seed);
        const cd lam(0.25, -0.5);
        std::vector<cd> A0((size_t)n * L, 0.0), A1((size_t)n * L, 0.0), mu(64), vecs((size_t)64 * n);
        for (int j = 0; j < 2; ++j)
            for (int i = 0; i < n; ++i)
                for (int l = 0; l < L; ++l) A0[(size_t)i * L + l] += V[j][i] * std::conj(R[j][l]);
        for (size_t e = 0; e < A0.size(); ++e) A1[e] = lam * A0[e];
        int kk = -1;
        CHECK(emme_contour_eigpairs(n, L, dp(A0), dp(A1), 1e-8, 64, dp(mu), dp(vecs), &kk, nullptr) == EMME_OK && kk == 2);
        for (int q = 0; q < 2; ++q) {
            CHECK(std::abs(mu[q] - lam) < 1e-12);
            double nr = 0.0;
            for (int i = 0; i < n; ++i) nr += std::norm(vecs[(size_t)q * n + i]);
            CHECK(std::isfinite(nr) && std::fabs(std::sqrt(nr) - 1.0) < 1e-13);
        }
    }
    // zero moments: rank 0, nothing written
    {
        std::vector<cd> A0(50 * 8, 0.0), mu(64, cd(3.0, 3.0)), vecs(64 * 50, cd(3.0, 3.0));
        int kk = -1;
        CHECK(emme_contour_eigpairs(50, 8, dp(A0), dp(A0), 1e-8, 64, dp(mu), dp(vecs), &kk, nullptr) == EMME_OK);
        CHECK(kk == 0 && mu[0] == cd(3.0, 3.0) && vecs[0] == cd(3.0, 3.0));
    }
    // bad arguments
    {
        std::vector<double> A(2 * 4 * 3, 0.0), mu(128), v(2 * 64 * 4);
        int kk = 0;
        CHECK(emme_contour_eigpairs(0, 3, A.data(), A.data(), 1e-8, 64, mu.data(), v.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigpairs(4, 65, A.data(), A.data(), 1e-8, 64, mu.data(), v.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigpairs(4, 3, A.data(), A.data(), 1.0, 64, mu.data(), v.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigpairs(4, 3, A.data(), A.data(), 1e-8, 0, mu.data(), v.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigpairs(4, 3, A.data(), nullptr, 1e-8, 64, mu.data(), v.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigpairs(4, 3, A.data(), A.data(), 1e-8, 64, nullptr, v.data(), &kk, nullptr) == EMME_EINVAL);
        CHECK(emme_contour_eigpairs(4, 3, A.data(), A.data(), 1e-8, 64, mu.data(), v.data(), nullptr, nullptr) == EMME_EINVAL);
    }
    if (failures) {
        std::fprintf(stderr, "%d contour eigenpair self-test failures\n", failures);
        return 1;
    }
    std::printf("contour eigenpair self-test ok (ASan + UBSan clean)\n");
    return 0;
}
