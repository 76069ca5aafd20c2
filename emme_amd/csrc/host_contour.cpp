// host_contour.cpp -- the host half of the contour eigensolver: the Beyn step on the contour
// moments (W.-J. Beyn, "An integral method for solving nonlinear eigenvalue problems", Linear Algebra Appl. 436,
// 2012, algorithm 1) and the argument-principle count.  Plain C++: the moments are n x L with L <= 64, the
// reduced matrix k x k with k <= L, so none of it is worth a device round trip, and no LAPACK is linked:
//   one-sided (Hestenes) Jacobi for the thin SVD A0 = U S W^H -- columns are rotated until pairwise orthogonal,
//     which gives every singular value to high relative accuracy, the noise floor included;
//   Householder reduction of B to Hessenberg form, then the explicitly shifted QR iteration (Wilkinson shifts,
//     an exceptional shift every 10 sweeps without deflation) for the eigenvalues of B.
#include <algorithm>
#include <cmath>
#include <complex>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/emme_hip.h"
#include "host_contour.hpp"

namespace emme {
void set_error(const std::string& msg);
}

namespace {

using cd = std::complex<double>;
constexpr double kEps = 2.220446049250313e-16;

// one-sided Jacobi on the columns of G (L columns of length n, G[l][i]); W (L x L, W[l][r] = row r of column l)
// accumulates the rotations, so that on exit  A0 W = G  with orthogonal columns
void jacobi_columns(int n, int L, std::vector<std::vector<cd>>& G, std::vector<std::vector<cd>>& W) {
    W.assign(L, std::vector<cd>(L, 0.0));
    for (int l = 0; l < L; ++l) W[l][l] = 1.0;
    for (int sweep = 0; sweep < 80; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < L - 1; ++p)
            for (int q = p + 1; q < L; ++q) {
                double al = 0.0, be = 0.0;
                cd ga = 0.0;
                for (int i = 0; i < n; ++i) {
                    al += std::norm(G[p][i]), be += std::norm(G[q][i]);
                    ga += std::conj(G[p][i]) * G[q][i];
                }
                const double g = std::abs(ga);
                if (!(g > 4.0 * kEps * std::sqrt(al * be)) || g == 0.0) continue;
                rotated = true;
                // the phase of <p, q> moves onto column q, then a real rotation zeroes the now real coupling
                const cd ph = std::conj(ga) / g;
                const double zeta = (be - al) / (2.0 * g);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < n; ++i) {
                    const cd xp = G[p][i], xq = G[q][i] * ph;
                    G[p][i] = c * xp - s * xq, G[q][i] = s * xp + c * xq;
                }
                for (int r = 0; r < L; ++r) {
                    const cd xp = W[p][r], xq = W[q][r] * ph;
                    W[p][r] = c * xp - s * xq, W[q][r] = s * xp + c * xq;
                }
            }
        if (!rotated) break;
    }
}

// eigenvalues of the k x k complex matrix H (row-major, destroyed); false if the QR iteration did not converge
bool eigenvalues(int k, std::vector<cd>& H, std::vector<cd>& ev) {
    auto h = [&](int r, int c) -> cd& { return H[(size_t)r * k + c]; };
    // Householder reduction to upper Hessenberg form
    for (int j = 0; j + 2 < k; ++j) {
        double xn = 0.0;
        for (int r = j + 1; r < k; ++r) xn += std::norm(h(r, j));
        xn = std::sqrt(xn);
        if (xn == 0.0) continue;
        const cd x0 = h(j + 1, j);
        const cd alpha = -(std::abs(x0) > 0.0 ? x0 / std::abs(x0) : cd(1.0)) * xn;
        std::vector<cd> v(k, 0.0);
        for (int r = j + 1; r < k; ++r) v[r] = h(r, j);
        v[j + 1] -= alpha;
        double vv = 0.0;
        for (int r = j + 1; r < k; ++r) vv += std::norm(v[r]);
        if (vv == 0.0) continue;
        for (int c = j; c < k; ++c) {  // H <- (I - 2 v v^H / v^H v) H
            cd s = 0.0;
            for (int r = j + 1; r < k; ++r) s += std::conj(v[r]) * h(r, c);
            s *= 2.0 / vv;
            for (int r = j + 1; r < k; ++r) h(r, c) -= s * v[r];
        }
        for (int r = 0; r < k; ++r) {  // H <- H (I - 2 v v^H / v^H v)
            cd s = 0.0;
            for (int c = j + 1; c < k; ++c) s += h(r, c) * v[c];
            s *= 2.0 / vv;
            for (int c = j + 1; c < k; ++c) h(r, c) -= s * std::conj(v[c]);
        }
        for (int r = j + 2; r < k; ++r) h(r, j) = 0.0;
    }
    ev.assign(k, 0.0);
    std::vector<double> cs(k);
    std::vector<cd> sn(k);
    int hi = k - 1, iter = 0, total = 0;
    while (hi >= 0) {
        int l = hi;
        for (; l > 0; --l)
            if (std::abs(h(l, l - 1)) <= kEps * (std::abs(h(l, l)) + std::abs(h(l - 1, l - 1)))) {
                h(l, l - 1) = 0.0;
                break;
            }
        if (l == hi) {  // a 1 x 1 block has split off
            ev[hi] = h(hi, hi);
            --hi, iter = 0;
            continue;
        }
        if (++total > 60 * k) return false;
        ++iter;
        cd mu;
        if (iter % 10 == 0) {
            mu = h(hi, hi) + 0.75 * std::abs(h(hi, hi - 1));  // exceptional shift
        } else {  // Wilkinson: the eigenvalue of the trailing 2 x 2 block nearer its last diagonal entry
            const cd a = h(hi - 1, hi - 1), b = h(hi - 1, hi), c = h(hi, hi - 1), d = h(hi, hi);
            const cd half = 0.5 * (a - d), disc = std::sqrt(half * half + b * c);
            const cd e1 = 0.5 * (a + d) + disc, e2 = 0.5 * (a + d) - disc;
            mu = std::abs(e1 - d) < std::abs(e2 - d) ? e1 : e2;
        }
        // explicit QR step on the window [l, hi]: H - mu I = Q R, H <- R Q + mu I
        for (int j = l; j <= hi; ++j) h(j, j) -= mu;
        for (int j = l; j < hi; ++j) {
            const cd x = h(j, j), y = h(j + 1, j);
            const double r = std::hypot(std::abs(x), std::abs(y));
            double c;
            cd s;
            if (r == 0.0) {
                c = 1.0, s = 0.0;
            } else if (std::abs(x) == 0.0) {
                c = 0.0, s = 1.0;
            } else {
                c = std::abs(x) / r, s = (x / std::abs(x)) * std::conj(y) / r;
            }
            cs[j] = c, sn[j] = s;
            for (int col = j; col <= hi; ++col) {
                const cd u = h(j, col), w = h(j + 1, col);
                h(j, col) = c * u + s * w, h(j + 1, col) = -std::conj(s) * u + c * w;
            }
        }
        for (int j = l; j < hi; ++j) {
            const double c = cs[j];
            const cd s = sn[j];
            for (int r = l; r <= std::min(j + 2, hi); ++r) {
                const cd u = h(r, j), w = h(r, j + 1);
                h(r, j) = u * c + w * std::conj(s), h(r, j + 1) = -u * s + w * c;
            }
        }
        for (int j = l; j <= hi; ++j) h(j, j) += mu;
    }
    return true;
}

// y (k complex, unit 2-norm): the eigenvector of the k x k matrix B (row-major, kept) for its eigenvalue mu, by inverse
// iteration on a partial-pivot LU of B - mu I.  mu comes from the QR iteration, so the shifted matrix is singular to
// rounding and one or two solves align y; where a pivot is exactly zero the shift is moved by a few eps |B| and the
// factorisation repeated.
void eigenvector_of(int k, const std::vector<cd>& B, cd mu, std::vector<cd>& y) {
    double bnorm = 0.0;
    for (const cd& b : B) bnorm = std::max(bnorm, std::abs(b));
    if (!(bnorm > 0.0)) bnorm = 1.0;
    std::vector<cd> A((size_t)k * k);
    std::vector<int> piv(k);
    auto a = [&](int r, int c) -> cd& { return A[(size_t)r * k + c]; };
    for (int attempt = 0; attempt < 8; ++attempt) {
        const cd shift = mu + (attempt == 0 ? cd(0.0) : cd(1.0, 1.0) * (kEps * bnorm * std::ldexp(1.0, 2 * attempt)));
        A = B;
        for (int j = 0; j < k; ++j) a(j, j) -= shift;
        bool singular = false;
        for (int j = 0; j < k && !singular; ++j) {
            int p = j;
            for (int r = j + 1; r < k; ++r)
                if (std::abs(a(r, j)) > std::abs(a(p, j))) p = r;
            piv[j] = p;
            if (p != j)
                for (int c = 0; c < k; ++c) std::swap(a(j, c), a(p, c));
            if (std::abs(a(j, j)) == 0.0 || !std::isfinite(std::abs(a(j, j)))) {
                singular = true;
                break;
            }
            for (int r = j + 1; r < k; ++r) {
                const cd m = a(r, j) / a(j, j);
                a(r, j) = m;
                for (int c = j + 1; c < k; ++c) a(r, c) -= m * a(j, c);
            }
        }
        if (singular) continue;
        // a start vector with weight on every component, then three solves
        y.resize(k);
        for (int i = 0; i < k; ++i) y[i] = cd(1.0 + 0.37 * std::sin(1.0 + i), 0.21 * std::cos(2.0 * i));
        bool ok = true;
        for (int sweep = 0; sweep < 3 && ok; ++sweep) {
            for (int j = 0; j < k; ++j) {
                std::swap(y[j], y[piv[j]]);
                for (int r = j + 1; r < k; ++r) y[r] -= a(r, j) * y[j];
            }
            for (int j = k - 1; j >= 0; --j) {
                for (int c = j + 1; c < k; ++c) y[j] -= a(j, c) * y[c];
                y[j] /= a(j, j);
            }
            // (scaled by the largest entry first: the solution of a nearly singular system may be huge)
            double big = 0.0;
            for (int i = 0; i < k; ++i) big = std::max(big, std::max(std::fabs(y[i].real()), std::fabs(y[i].imag())));
            ok = big > 0.0 && std::isfinite(big);
            if (!ok) break;
            double nrm = 0.0;
            for (int i = 0; i < k; ++i) y[i] /= big, nrm += std::norm(y[i]);
            nrm = std::sqrt(nrm);
            for (int i = 0; i < k; ++i) y[i] /= nrm;
        }
        if (ok) return;
    }
    // (not reached for a finite B: eight shifts cannot all hit an eigenvalue exactly)
    y.assign(k, 0.0);
    y[0] = 1.0;
}

}  // namespace

namespace emme {

int contour_winding(const double* args, int N, double max_step, bool* resolved, double* W_raw) {
    double sum = 0.0;
    bool ok = true;
    for (int j = 0; j < N; ++j) {
        const double d = std::remainder(args[(j + 1) % N] - args[j], 2.0 * M_PI);
        ok = ok && std::isfinite(d) && std::fabs(d) <= max_step;
        sum += d;
    }
    const double W = sum / (2.0 * M_PI);
    ok = ok && std::isfinite(W) && std::fabs(W - std::nearbyint(W)) <= 0.05;
    if (resolved) *resolved = ok;
    if (W_raw) *W_raw = W;
    return std::isfinite(W) ? (int)std::nearbyint(W) : -1;
}

const char* contour_arg_error(const emme_contour_t* ct) {
    auto pow2 = [](int x) { return x > 0 && (x & (x - 1)) == 0; };
    if (ct->size != (int)sizeof(emme_contour_t)) return "emme_contour_t of the wrong size (fill it with emme_contour_default)";
    const double cx = ct->center[0], cy = ct->center[1], ea = ct->semi_axes[0], eb = ct->semi_axes[1];
    if (!(ea > 0.0 && eb > 0.0) || !std::isfinite(ea) || !std::isfinite(eb) || !std::isfinite(cx) || !std::isfinite(cy))
        return "the semi-axes must be positive and finite";
    if (!(std::fabs(cx) > ea))
        return "the ellipse reaches Re omega = 0 (|Re c| <= a); M(omega) is analytic in one half-plane only";
    if (!pow2(ct->points) || ct->points < 4 || !pow2(ct->max_points) || ct->max_points < ct->points)
        return "points and max_points must be powers of two, 4 <= points <= max_points";
    if (ct->probes < 1 || ct->probes > 64 || !(ct->rank_tol > 0.0 && ct->rank_tol < 1.0))
        return "probes must lie in 1 .. 64 and rank_tol in (0, 1)";
    return nullptr;
}

namespace {
double norm_radius(const emme_contour_t& ct, double re, double im) {
    return std::hypot((re - ct.center[0]) / ct.semi_axes[0], (im - ct.center[1]) / ct.semi_axes[1]);
}
}  // namespace

void contour_candidates(const emme_contour_t& ct, int k, const double* mu, std::vector<double>& guesses,
                        std::vector<int>* kept) {
    const double rho = std::max(ct.semi_axes[0], ct.semi_axes[1]);
    for (int q = 0; q < k; ++q) {
        const double re = ct.center[0] + rho * mu[2 * q], im = ct.center[1] + rho * mu[2 * q + 1];
        if (!(std::isfinite(re) && std::isfinite(im) && norm_radius(ct, re, im) < 1.5)) continue;
        guesses.push_back(re), guesses.push_back(im);
        if (kept) kept->push_back(q);
    }
}

std::vector<ContourRoot> contour_keep_roots(const emme_contour_t& ct, double tol, int step_limit, int ng, const double* r,
                                            const int* its, const int* inf, const double* path) {
    // a chain that used every step converged only if its last step was below tol (src/main.cpp:53-56)
    auto converged = [&](int q) {
        if (its[q] <= step_limit) return true;
        if (step_limit < 1) return false;
        const double* w = &path[2 * ((size_t)q * (step_limit + 1) + step_limit)];
        return std::hypot(w[0] - w[-2], w[1] - w[-1]) < tol * std::hypot(w[0], w[1]);
    };
    std::vector<ContourRoot> found;
    for (int q = 0; q < ng; ++q) {
        if (inf[q] != 0 || !converged(q) || !(norm_radius(ct, r[2 * q], r[2 * q + 1]) < 1.0)) continue;
        bool dup = false;
        for (const ContourRoot& f : found)
            dup |= std::hypot(f.re - r[2 * q], f.im - r[2 * q + 1]) <= 10.0 * tol * std::hypot(r[2 * q], r[2 * q + 1]);
        if (!dup) found.push_back({r[2 * q], r[2 * q + 1], its[q], inf[q], q});
    }
    std::stable_sort(found.begin(), found.end(), [](const ContourRoot& x, const ContourRoot& y) { return x.im > y.im; });
    return found;
}

// ---- the round plan of a region search over (set, contour) items -------------------------------
ContourRounds::ContourRounds(int nitems, const int* set, const emme_contour_t* contours) : items(nitems) {
    for (int k = 0; k < nitems; ++k) items[k].set = set ? set[k] : 0, items[k].ct = contours[k], items[k].L = contours[k].probes;
}

bool ContourRounds::plan_nodes() {
    r_first = nodes();
    r_item.clear(), r_set.clear(), r_omega.clear();
    for (int k = 0; k < (int)items.size(); ++k) {
        Item& it = items[k];
        if (it.dropped || !it.adding) continue;
        const int cap = it.ct.max_points;
        const int add = it.N == 0 ? it.ct.points : it.N;
        for (int j = 0; j < add; ++j) {
            // the start nodes t_j = 2 pi j / N; later the midpoints of the N nodes held
            const int m = it.N == 0 ? j * (cap / add) : (2 * j + 1) * (cap / (2 * it.N));
            const double t = 2.0 * M_PI * m / cap;
            it.nodes.push_back(nodes()), it.node_m.push_back(m);
            node_item.push_back(k);
            r_item.push_back(k), r_set.push_back(it.set);
            r_omega.push_back(it.ct.center[0] + it.ct.semi_axes[0] * std::cos(t));
            r_omega.push_back(it.ct.center[1] + it.ct.semi_axes[1] * std::sin(t));
        }
        it.N += add;
    }
    return !r_item.empty();
}

void ContourRounds::drop(int item, int status) {
    Item& it = items[item];
    if (it.dropped) return;
    it.dropped = true, it.adding = it.doubling = false;
    it.status = status, it.W = -1, it.k = 0;
}

void ContourRounds::take_logdets(const double* logdet) {
    std::vector<int> ord;
    std::vector<double> args;
    for (Item& it : items) {
        if (it.dropped || !it.adding) continue;
        // argument principle on the item's nodes in contour order
        ord.resize(it.nodes.size());
        std::iota(ord.begin(), ord.end(), 0);
        std::sort(ord.begin(), ord.end(), [&](int x, int y) { return it.node_m[x] < it.node_m[y]; });
        args.resize(ord.size());
        for (size_t q = 0; q < ord.size(); ++q) args[q] = logdet[2 * (size_t)it.nodes[ord[q]] + 1];
        bool resolved = false;
        const int w = contour_winding(args.data(), it.N, 0.5 * M_PI, &resolved, nullptr);
        if (resolved) it.W = w;
        // N doubles by the midpoints while the count is unresolved, up to max_points
        it.adding = !resolved && 2 * it.N <= it.ct.max_points;
    }
}

bool ContourRounds::plan_moments(const int* info, std::vector<int>& which, std::vector<int>& off, std::vector<int>& idx,
                                 std::vector<double>& wz) const {
    which.clear(), idx.clear();
    off.assign(1, 0);
    wz.assign(4 * (size_t)nodes(), 0.0);
    for (int k = 0; k < (int)items.size(); ++k) {
        const Item& it = items[k];
        if (it.dropped || !it.doubling) continue;
        const double ea = it.ct.semi_axes[0], eb = it.ct.semi_axes[1], rho = std::max(ea, eb);
        for (size_t q = 0; q < it.nodes.size(); ++q) {
            const int node = it.nodes[q];
            // trapezoid weights of the item's final N: w = omega'(t) / (i N), z = (omega - c) / rho
            const double t = 2.0 * M_PI * it.node_m[q] / it.ct.max_points;
            const double dre = -ea * std::sin(t), dim_ = eb * std::cos(t);
            double* o = &wz[4 * (size_t)node];
            o[0] = dim_ / it.N, o[1] = -dre / it.N;
            o[2] = ea * std::cos(t) / rho, o[3] = eb * std::sin(t) / rho;
            if (info[node] == 0) idx.push_back(node);
        }
        which.push_back(k);
        off.push_back((int)idx.size());
    }
    return !which.empty();
}

bool ContourRounds::take_rank(int item, int k, int* l0, int* nl) {
    Item& it = items[item];
    it.k = k;
    // L doubles while A0 keeps full numerical rank
    if (k < it.L || it.L >= 64) {
        it.doubling = false;
        return false;
    }
    const int L2 = std::min(2 * it.L, 64);
    *l0 = it.L, *nl = L2 - it.L;
    it.L = L2;
    return true;
}

}  // namespace emme

namespace {

// The Beyn step (Beyn 2012, algorithm 1, steps 3-5) on moments A0 = sum w_j X_j, A1 = sum w_j z_j X_j
// and, vecs given, the eigenvectors v_c = U_k y_c of M for every mu_c written (y_c: the eigenvector of B for mu_c)
int beyn_step(const char* who, int n, int L, const double* A0, const double* A1, double rank_tol, int max_eigs, double* mu,
              double* vecs, int* k_out, double* sigma) {
    if (n < 1 || L < 1 || L > 64 || !A0 || !A1 || !mu || !k_out || max_eigs < 1 || !(rank_tol > 0.0 && rank_tol < 1.0)) {
        emme::set_error(std::string(who) + ": need n >= 1, 1 <= L <= 64, A0, A1, mu, k, max_eigs >= 1 and 0 < rank_tol < 1");
        return EMME_EINVAL;
    }
    const cd* a0 = reinterpret_cast<const cd*>(A0);
    const cd* a1 = reinterpret_cast<const cd*>(A1);
    std::vector<std::vector<cd>> G(L, std::vector<cd>(n)), W;
    for (int i = 0; i < n; ++i)
        for (int l = 0; l < L; ++l) G[l][i] = a0[(size_t)i * L + l];
    jacobi_columns(n, L, G, W);
    std::vector<double> s(L);
    for (int l = 0; l < L; ++l) {
        double t = 0.0;
        for (int i = 0; i < n; ++i) t += std::norm(G[l][i]);
        s[l] = std::sqrt(t);
    }
    std::vector<int> ord(L);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return s[x] > s[y]; });
    if (sigma)
        for (int l = 0; l < L; ++l) sigma[l] = s[ord[l]];
    const double s1 = s[ord[0]];
    int k = 0;
    while (k < L && s1 > 0.0 && s[ord[k]] > rank_tol * s1) ++k;
    *k_out = k;
    if (k == 0) return EMME_OK;
    // B = U_k^H A1 W_k S_k^-1, with U_l = G_l / s_l
    std::vector<cd> B((size_t)k * k), a1w(n);
    for (int q = 0; q < k; ++q) {
        const int cq = ord[q];
        for (int i = 0; i < n; ++i) {
            cd t = 0.0;
            for (int r = 0; r < L; ++r) t += a1[(size_t)i * L + r] * W[cq][r];
            a1w[i] = t;
        }
        for (int p = 0; p < k; ++p) {
            const int cp = ord[p];
            cd t = 0.0;
            for (int i = 0; i < n; ++i) t += std::conj(G[cp][i]) * a1w[i];
            B[(size_t)p * k + q] = t / (s[cp] * s[cq]);
        }
    }
    std::vector<cd> ev, Bkept;
    if (vecs) Bkept = B;  // (the QR iteration destroys its operand)
    if (!eigenvalues(k, B, ev)) {
        emme::set_error(std::string(who) + ": the QR iteration on the reduced matrix did not converge");
        return EMME_ENUMERIC;
    }
    for (int q = 0; q < std::min(k, max_eigs); ++q) mu[2 * q] = ev[q].real(), mu[2 * q + 1] = ev[q].imag();
    if (!vecs) return EMME_OK;
    std::vector<cd> y, v(n);
    for (int q = 0; q < std::min(k, max_eigs); ++q) {
        eigenvector_of(k, Bkept, ev[q], y);
        // v = U_k y, U_p = G_p / s_p; U_k is orthonormal to rounding only, so the norm is taken again
        double nrm = 0.0;
        for (int i = 0; i < n; ++i) {
            cd t = 0.0;
            for (int p = 0; p < k; ++p) t += G[ord[p]][i] * (y[p] / s[ord[p]]);
            v[i] = t, nrm += std::norm(t);
        }
        nrm = std::sqrt(nrm);
        cd* row = reinterpret_cast<cd*>(vecs) + (size_t)q * n;
        for (int i = 0; i < n; ++i) row[i] = v[i] / nrm;
    }
    return EMME_OK;
}

}  // namespace

extern "C" {

void emme_contour_default(emme_contour_t* c) {
    if (!c) return;
    *c = emme_contour_t{};
    c->size = (int)sizeof(emme_contour_t);
    // the count resolves at N = 8 .. 64 on the test contours; sigma(A0) levels off 3e-9 .. 8e-7 below
    // sigma_1 once it does (the fill's own accuracy), the modes stand at >= 0.1 sigma_1
    c->points = 32;
    c->max_points = 512;
    c->probes = 8;
    c->rank_tol = 1e-5;
}

// The Beyn step (Beyn 2012, algorithm 1, steps 3-5) on given moments
int emme_contour_eigs(int n, int L, const double* A0, const double* A1, double rank_tol, int max_eigs, double* mu,
                      int* k_out, double* sigma) {
    return beyn_step("emme_contour_eigs", n, L, A0, A1, rank_tol, max_eigs, mu, nullptr, k_out, sigma);
}

// ... with the eigenvectors v_c = U_k y_c that the step yields beside every mu_c
int emme_contour_eigpairs(int n, int L, const double* A0, const double* A1, double rank_tol, int max_eigs, double* mu,
                          double* vecs, int* k_out, double* sigma) {
    return beyn_step("emme_contour_eigpairs", n, L, A0, A1, rank_tol, max_eigs, mu, vecs, k_out, sigma);
}

}  // extern "C"
