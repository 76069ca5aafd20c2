// assemble_common.hpp -- the leaf pieces that the fill kernels share (assemble.hip, assemble_wl.hip,
// assemble_cached.hip, assemble_dense.hip, the cached derivative fills assemble_dense_deriv.hip and
// assemble_dense_shape_deriv.hip through assemble_dense_deriv_text.hpp, the table-free tile fills assemble_tile*.hip
// through assemble_tile_text.hpp; probe.hip for the tables): the Gauss-Kronrod
// tables, the caps, the accept / split rule of the adaptive quadrature, kappa_e, the pair weights, the three ways an
// entry of M is stored, the small helpers of the dense fills and the leaves of the tile fills.  The kernel BODIES stay
// separate texts: what is here are forceinline leaves that perform the same operations in the same
// order at every call site, and that left the device assembly of every caller unchanged when they moved here.
#pragma once
#include <hip/hip_runtime.h>

#include "emme_device.hpp"

namespace emme {
namespace {

// Caps of the adaptive quadrature that the reference does not have.  Its only limit is the depth
// integration_iteration_limit (`ldexp(scale, max_sub) > 0.99 (b - a)`, include/functions.h:240),
// 100 in the shipped inputs; every fill kernel here additionally stops refining at depth
// EMME_MAX_DEPTH (the interval is then pi/2 * 2^-40 = 1.4e-12 wide: a finite integrand of this
// family is resolved long before -- deepest tree met in the tests and the bench: 21 -- and a NaN
// never splits, its comparisons being false) or after EMME_MAX_INTERVALS intervals of one
// integral, and flags the matrix (status -> EMME_ENUMERIC) instead of walking on.  The same two
// numbers in every kernel, so that the flag does not depend on which kernel served the integral.
constexpr int EMME_MAX_DEPTH = 40;
constexpr int EMME_MAX_INTERVALS = 1 << 18;
// Largest modulus of an integral the device path stands for.  The Newton step's pivot search compares |x|^2, which
// overflows beyond 1.3e154, so a matrix with a larger entry could not be factored anyway.  The
// reference (std::abs = hypot, LAPACK's scaled arithmetic) goes on to 1e308 -- where, on the headline lattice,
// its own intermediates overflow first (chain 80's iterate -0.0055-0.734i: entries up to 3e202, two of them
// inf; its zsysv then fails, include/solver.h:142-153).  Such a matrix is flagged (status -> EMME_ENUMERIC).
// (The accept/split rule used to overflow as well, and on far smaller matrices: gk_modulus below.)
constexpr double EMME_MAX_ENTRY = 1e150;
__device__ __forceinline__ bool kappa_bad(cd k) { return !(fabs(k.x) < EMME_MAX_ENTRY && fabs(k.y) < EMME_MAX_ENTRY); }

// ---- the accept / split rule (include/functions.h:203-208, 231-247) ------------------------------------------
// Square root of the error estimates: the exact one, or (the dense fills) the hardware reciprocal-square-root seed
// + two Newton steps of frsqrt (<= 1 ulp for normal arguments), 0 for 0 and NaN for NaN.
__device__ __forceinline__ double fsqrt_pos(double x) {
    const double y = x * frsqrt(x);
    return x > 0.0 ? y : x;
}
struct SqrtExact {
    static __device__ __forceinline__ double of(double x) { return sqrt(x); }
};
struct SqrtSeeded {
    static __device__ __forceinline__ double of(double x) { return fsqrt_pos(x); }
};
// |x + i y| for the rule: sqrt(x^2 + y^2), the same bits as ever wherever the squares are representable.  They are not
// from |z| = 1.3e154 on, and the Kronrod sum of ONE interval gets there long before the finished integral reaches
// EMME_MAX_ENTRY: far below the real axis the integrand is 1e12 times its integral (tokamak example, omega = 0.5-4.9i:
// nodes of 1.8e156 under an integral of 3e143).  The modulus then came out infinite, `inf > inf` accepted the interval
// whatever its error, and the integral ended decades off -- flagged only where the wrong value happened to pass
// EMME_MAX_ENTRY.  The reference takes std::abs = hypot there; here the squares are taken on 2^-520 z (exact) instead.
// A NaN sum goes the same way and stays NaN.
// From 2^52 EMME_MAX_ENTRY = 4.5e165 on the modulus is reported infinite as before: an integral that sums such
// intervals cannot come back below EMME_MAX_ENTRY with one correct bit, so its matrix is lost, and `inf > inf` ends the
// walk at once instead of refining what nobody will read (the lost matrix of a root search costs what it used to).
template <class Sqrt = SqrtExact>
__device__ __forceinline__ double gk_modulus(double x, double y) {
    const double n2 = fma(x, x, y * y);
    if (__builtin_expect(n2 <= 1.7976931348623157e308, 1)) return Sqrt::of(n2);
    const double xs = x * 0x1p-520, ys = y * 0x1p-520;
    const double m = Sqrt::of(fma(xs, xs, ys * ys));
    return m >= (EMME_MAX_ENTRY * 0x1p52) * 0x1p-520 ? __builtin_inf() : m * 0x1p520;
}
// The rule's two moduli, |K| and |K - G|, behind ONE test: the sum of the two sums of squares is representable exactly
// when neither needs the rescaled form (a NaN takes it and stays NaN).
template <class Sqrt = SqrtExact>
__device__ __forceinline__ void gk_moduli(double kx, double ky, double dx, double dy, double& absK, double& absD) {
    const double nk = fma(kx, kx, ky * ky), nd = fma(dx, dx, dy * dy);
    if (__builtin_expect(nk + nd <= 1.7976931348623157e308, 1)) {
        absK = Sqrt::of(nk), absD = Sqrt::of(nd);
    } else {
        absK = gk_modulus<Sqrt>(kx, ky), absD = gk_modulus<Sqrt>(dx, dy);
    }
}
// Does the interval of half-width `scale` at bisection depth `depth`, with Kronrod sum K and Gauss sum G (both
// before the factor scale), have to be split?  :203-208: err = max(|K - G|, 2 eps |K|) scale; :231-233:
// |rel * integral|; :237-239: abs_tol is set by the first interval of the integral (the root) and is what the
// caller keeps per integral; :240-242: ldexp(scale, max_sub) > 0.99 (b - a) with scale = (b - a) 2^-(depth+1)
// (up to rounding far below the 1 % margin) is exactly depth < max_sub.  inv_scale = 2 / (b - a).
template <class Sqrt = SqrtExact>
__device__ __forceinline__ bool gk_split(cd K, cd G, double scale, double inv_scale, int depth, const DevParams& P,
                                         double& abs_tol) {
    const double dKx = K.x - G.x, dKy = K.y - G.y;
    double absK, absD;
    gk_moduli<Sqrt>(K.x, K.y, dKx, dKy, absK, absD);
    double err = fmax(absD, absK * (2.0 * 2.220446049250313e-16));
    err *= scale;
    const double rel_abs = P.rel_tol * (absK * scale);
    if (abs_tol == 0.0) abs_tol = rel_abs;
    return depth < P.max_sub && err > abs_tol * inv_scale + P.prec_goal && err > rel_abs + P.prec_goal;
}
// per-lane node tables: lane r of a group -> (signed abscissa, Kronrod weight, Gauss weight)
__device__ const double kX15[8] = {0.,
                                   0.20778495500789847,
                                   0.40584515137739717,
                                   0.58608723546769113,
                                   0.74153118559939444,
                                   0.86486442335976907,
                                   0.94910791234275852,
                                   0.99145537112081264};
__device__ const double kWg15[4] = {0.41795918367346939, 0.38183005050511894,
                                    0.27970539148927667, 0.12948496616886969};
__device__ const double kWk15[8] = {2.09482141084727828e-01, 2.04432940075298892e-01,
                                    1.90350578064785410e-01, 1.69004726639267903e-01,
                                    1.40653259715525919e-01, 1.04790010322250184e-01,
                                    6.30920926299785533e-02, 2.29353220105292250e-02};
__device__ const double kX31[16] = {0.0,
                                    0.1011420669187175,
                                    0.20119409399743452,
                                    0.29918000715316881,
                                    0.39415134707756337,
                                    0.48508186364023968,
                                    0.57097217260853885,
                                    0.65099674129741697,
                                    0.72441773136017005,
                                    0.79041850144246593,
                                    0.84820658341042722,
                                    0.8972645323440819,
                                    0.9372733924007059,
                                    0.96773907567913913,
                                    0.98799251802048543,
                                    0.99800229869339706};
__device__ const double kWg31[8] = {0.20257824192556112, 0.19843148532711152,
                                    0.18616100001556193, 0.1662692058169939,
                                    0.1395706779261542,  0.10715922046717143,
                                    0.07036604748810768, 0.030753241996119};
__device__ const double kWk31[16] = {
    0.10133000701479155,   0.100769845523875595,  0.099173598721791959,  0.0966427269836236785,
    0.093126598170825321,  0.0885644430562117706, 0.083080502823133021,  0.0768496807577203789,
    0.069854121318728259,  0.0620095678006706403, 0.053481524690928087,  0.0445897513247648766,
    0.035346360791375846,  0.0254608473267153202, 0.0150079473293161225, 0.00537747987292334899};

template <int PTS>
__device__ __forceinline__ GkLane gk_lane(int r) {
    constexpr int H = (PTS + 1) / 2;  // 8 or 16 (centre + H-1 pairs)
    const double* X = PTS == 15 ? kX15 : kX31;
    const double* WK = PTS == 15 ? kWk15 : kWk31;
    const double* WG = PTS == 15 ? kWg15 : kWg31;
    GkLane g;
    if (r >= PTS) {  // padding lane: evaluates the centre again with zero weight
        g.x = 0.0, g.wk = 0.0, g.wg = 0.0;
        return g;
    }
    const int i = r < H ? r : r - (H - 1);  // node index 0..H-1
    g.x = r < H ? X[i] : -X[i];
    g.wk = WK[i];
    // Gauss nodes of the embedded rule: the centre and the even Kronrod nodes
    // (include/functions.h:190-199; both embedded orders, 7 and 15, are odd)
    g.wg = (i % 2 == 0) ? WG[i / 2] : 0.0;
    return g;
}

// all-reduce over a lane group of 16 (one DPP row) or 32 (two rows) lanes
template <int GW>
__device__ __forceinline__ double group_sum(double v) {
    v = row16_sum(v);
    if (GW == 32) v += __shfl_xor(v, 16);
    return v;
}

// Interval counters (one per batch item) leave a workgroup once per omega slot: the lanes add theirs up in
// LDS, one designated lane per slot (`flusher`) carries the sum to memory after a barrier.  Every workgroup
// of a fill launch adds to the same <= 128 counters: at one global atomic per lane the dense fill spent 10 %
// of a launch waiting for them.  s_iv: LDS, one word per slot, zeroed before the kernel's
// first barrier.
__device__ __forceinline__ void block_add_intervals(unsigned long long* s_iv, unsigned long long* intervals,
                                                    int slot, bool has_w, bool flusher, int b,
                                                    unsigned long long mine) {
    if (!intervals) return;  // (uniform)
    if (has_w && mine) atomicAdd(&s_iv[slot], mine);
    __syncthreads();
    if (flusher) {
        const unsigned long long v = s_iv[slot];
        if (v) atomicAdd(&intervals[b], v);
    }
}

// Adiabatic-electron closed forms kappa_e (src/Parameters.cpp:186-209).
__device__ __forceinline__ cd kappa_e(int m, const DevParams& P, double de, double dg, cd omega) {
    if (m == 1) {
        // -i qR/(2 vt tau) (omega - ws_e) sgn(de)
        const double c = P.qR / (2.0 * P.vt * P.tau) * (de / fabs(de));
        const cd a = mk(omega.x - P.omega_s_e, omega.y);
        return mk(c * a.y, -(c * a.x));
    }
    if (m == 2) {
        const double f = (P.qR * P.qR) / (2.0 * P.vt * P.vt * P.tau) * de / fabs(de);
        const cd wa = mk(omega.x - P.omega_s_e, omega.y);
        const cd a = de * (omega * wa);
        const double b1e = P.cbe * dg;
        const cd b = (b1e * P.vt / P.qR) * mk(omega.x - P.omega_s_e * (1.0 + P.eta_e), omega.y);
        return f * (a - b);
    }
    return mk(0.0, 0.0);
}

// d kappa_e / d omega (the derivative fills): m = 1: -i c; m = 2: f (de (2 omega - ws_e) - b1e vt / qR); m = 0: 0
__device__ __forceinline__ cd kappa_e_d(int m, const DevParams& P, double de, double dg, cd omega) {
    if (m == 1) {
        const double c = P.qR / (2.0 * P.vt * P.tau) * (de / fabs(de));
        return mk(0.0, -c);
    }
    if (m == 2) {
        const double f = (P.qR * P.qR) / (2.0 * P.vt * P.vt * P.tau) * de / fabs(de);
        const double b1e = P.cbe * dg;
        return f * mk(de * (2.0 * omega.x - P.omega_s_e) - b1e * P.vt / P.qR, de * (2.0 * omega.y));
    }
    return mk(0.0, 0.0);
}

// SingularityHandler weight for i < j (src/singularity_handler.cpp:4-20): end-corrected
// band near the diagonal, 1 elsewhere, minus one half on the last column.
__device__ __forceinline__ double pair_weight(int i, int j, int N) {
    const int d = j - i;
    double w = d <= 5 ? (d == 1   ? 2.951388888888883
                         : d == 2 ? -2.4305555555555305
                         : d == 3 ? 4.166666666667441
                         : d == 4 ? -0.3472222222224549
                                  : 1.159722222222284)
                      : 1.0;
    if (j == N - 1) w -= 0.5;
    return w;
}

// ---- entries of M ----------------------------------------------------------------------------------------------
// One entry idx = row * dim + col of a matrix at `Mb`: with the fused secant quotient Mp = (M - Mold) / domega
// (include/solver.h:54-57; rdw = 1 / domega, Moldb null = none), or M and the same entry of M'.
__device__ __forceinline__ void store_entry_secant(double2* Mb, const double2* Moldb, double2* Mpb, cd rdw, size_t idx,
                                                   cd v) {
    Mb[idx] = make_double2(v.x, v.y);
    if (Moldb) {
        const double2 o = Moldb[idx];
        const cd d = (v - mk(o.x, o.y)) * rdw;
        Mpb[idx] = make_double2(d.x, d.y);
    }
}
__device__ __forceinline__ void store_entry_twin(double2* Mb, double2* Mdb, size_t idx, cd v, cd vd) {
    Mb[idx] = make_double2(v.x, v.y);
    Mdb[idx] = make_double2(vd.x, vd.y);
}

// A_ij = -kappa_all(0) W_ij dx (include/solver.h:448-453): the factor of kappa
__device__ __forceinline__ double pair_entry_weight(int i, int j, int N, double dx) {
    return -(pair_weight(i, j, N) * dx);
}

// ---- small helpers of the dense fills ----------------------------------------------------------------------------
// (wg / wk) of node slot sn of a tile block: the Gauss rule's weight relative to the Kronrod weight; 0 for
// Kronrod-only nodes
template <int PTS>
__device__ __forceinline__ double gauss_ratio(int sn) {
    if (sn >= (PTS - 1) / 2) return 0.0;          // (7 / 15 Gauss nodes, slots 0 ..)
    const int q = sn == 0 ? 0 : ((sn + 1) & ~1);  // slots (1,2) (3,4) (5,6) .. are nodes +-x2, +-x4, +-x6 ..
    return PTS == 15 ? kWg15[q >> 1] / kWk15[q] : kWg31[q >> 1] / kWk31[q];
}
// the pointer lane k holds (k wave-uniform): two v_readlane, not a bpermute through LDS.  It points to GLOBAL memory
// and comes back as an address-space-1 pointer (as uniform() in linstep_blocked.hip): rebuilt from an integer as a
// generic one, every load through it is a FLAT load, which counts in lgkmcnt as well as vmcnt and which the
// compiler can only wait for with a full drain -- the 16 operand loads of an MFMA round then retire together
// (vmcnt(0)) before the first MFMA instead of one k-step at a time.
__device__ __forceinline__ const double* lane_ptr(const double* p, int k) {
    const unsigned long long bits = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits >> 32), k);
    typedef const __attribute__((address_space(1))) double GD;
    GD* g = (GD*)(((unsigned long long)hi << 32) | lo);
    return (const double*)g;
}

__device__ __forceinline__ PairConst make_pair_const(const DevParams& P, double eta_i, double eta_j,
                                                     double bi, double bj, double dg) {
    PairConst pc;
    pc.de = eta_i - eta_j;
    pc.beta1 = P.cb * dg;
    pc.s = sqrt(bi * bj);
    pc.inv_s = 1.0 / pc.s;
    pc.bsum = bi + bj;
    const double qRd = P.qR * pc.de;
    pc.c_lam = 0.5 * P.vt / qRd * pc.beta1;
    pc.c_nv = qRd / P.vt;
    return pc;
}

// one MFMA accumulator: the 4 rows of a 16 x 16 FP64 tile that a lane holds
typedef double v4d __attribute__((ext_vector_type(4)));

// The interval at bisection depth `depth` with path bits `path` (most significant = first split, 1 = right half), by
// the reference's bisection arithmetic, so that every abscissa is bit-identical to the CPU's
__device__ __forceinline__ void interval_bounds_d(int depth, unsigned long long path, double& l, double& r) {
    l = 0.0;
    r = M_PI / 2.0;
    for (int s = depth - 1; s >= 0; --s) {
        const double mid = (r + l) / 2;
        if ((path >> s) & 1)
            l = mid;
        else
            r = mid;
    }
}

// ---- leaves of the table-free tile fills (assemble_tile_text.hpp) ------------------------------------------------------
// what the lanes of a wave wrote to LDS is visible to every lane of the wave afterwards
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// a PairConst to and from its LDS row of 8 doubles (the last one padding)
__device__ __forceinline__ void pair_const_to_row(double* row, const PairConst& pc) {
    row[0] = pc.de, row[1] = pc.beta1, row[2] = pc.s, row[3] = pc.inv_s;
    row[4] = pc.bsum, row[5] = pc.c_lam, row[6] = pc.c_nv, row[7] = 0.0;
}
__device__ __forceinline__ PairConst pair_const_of_row(const double* row) {
    PairConst pc;
    pc.de = row[0], pc.beta1 = row[1], pc.s = row[2], pc.inv_s = row[3];
    pc.bsum = row[4], pc.c_lam = row[5], pc.c_nv = row[6];
    return pc;
}
// One element of a phase block by k_btab's rule: wk exp(T omega), with T, omega and wk read from *tp, *omp and *wkp
// HERE and in this order (passed by value the surrounding kernels change).  exp(T omega) beyond 1e304 gives NaN: an
// integral of this omega that uses the node ends non-finite and flags its matrix (EMME_ENUMERIC) instead of dropping
// the term; a NaN omega goes through and poisons its own column only.
__device__ __forceinline__ cd weighted_phase(const double2* tp, const double2* omp, const double* wkp) {
    const double2 t = *tp, omw = *omp;
    const double ax = fma(t.x, omw.x, -(t.y * omw.y)), ay = fma(t.x, omw.y, t.y * omw.x);
    cd ev;
    if (!(ax > 700.0)) {
        double sa, ca;
        sincos(ay, &sa, &ca);
        const double ea = exp(ax);
        ev = mk(ea * ca, ea * sa);
    } else {
        ev = mk(__builtin_nan(""), __builtin_nan(""));
    }
    const double wk = *wkp;
    return mk(wk * ev.x, wk * ev.y);
}

}  // namespace
}  // namespace emme
