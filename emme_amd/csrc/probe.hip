// probe.hip -- the device building blocks of the fill, one item per thread (tests / tooling only).
//
// Nothing here is on a hot path: every kernel evaluates ONE primitive of emme_device.hpp per thread, with the
// arguments the fill kernels would hand it, and writes the result to the thread's own output slot.  The point
// is to see a single node: the fill kernels only ever show sums over thousands of them.
#include "assemble_common.hpp"
#include "ctx.hpp"

namespace emme {
namespace {

// ---- the Bessel helper alone --------------------------------------------------------------------
// util::bessel_i_alter_helper (include/functions.h:381-408) as the fill kernels evaluate it:
// out = {y0, y1, mu + y0, Re z < 0 ? z : -z} per argument.
// |z| as the reference's std::abs gives it (hypot, correctly rounded but for near-ties): the exact sum of the exact
// squares as an unevaluated pair, its square root with one Newton correction on the exact residual.  The Miller start
// index n0 = floor|z| + 1 is a floor of this number: sqrt(norm2(z)) is an ulp off often enough to start the
// recurrence one index away from the reference at |z| = an integer, which moves the normalised ratios by the
// algorithm's own error (6e-10 of the larger one, DESIGN.md appendix "pointwise accuracy").  Helper arguments are far
// from the overflow and underflow of a square: no scaling.
__device__ double cabs_rounded(cd z) {
#pragma clang fp contract(off)
    const double xx = z.x * z.x, yy = z.y * z.y;
    const double xl = fma(z.x, z.x, -xx), yl = fma(z.y, z.y, -yy);
    const double h = xx + yy;
    const double v = h - xx;
    const double l = ((xx - (h - v)) + (yy - v)) + (xl + yl);
    const double s = sqrt(h);
    if (!(s > 0.0)) return s;
    return s + (fma(-s, s, h) + l) / (2.0 * s);
}

__global__ void k_bessel_probe(const double2* z, int n, double2* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const cd zz = mk(z[k].x, z[k].y);
    const double zabs = cabs_rounded(zz);
    cd y0, y1, mutot;
    bessel_miller(rcp(zz), zabs, 1.0 / zabs, zz.x < 0.0, y0, y1, mutot);
    out[4 * k + 0] = make_double2(y0.x, y0.y);
    out[4 * k + 1] = make_double2(y1.x, y1.y);
    out[4 * k + 2] = make_double2(mutot.x, mutot.y);
    out[4 * k + 3] = zz.x < 0.0 ? make_double2(zz.x, zz.y) : make_double2(-zz.x, -zz.y);
}

// ---- one math primitive per argument (FN = EMME_FN_* of include/emme_hip.h) ------------------------
// The TransConsts copies get their coefficients the way the fill kernels do: once per thread, before the
// evaluation, pinned in scalar (trans_consts) or vector (trans_consts_v) registers.
template <int FN>
__global__ void k_elementary_probe(const double* x, int n, double* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (FN == 0) {
        out[k] = frcp(x[k]);
    } else if (FN == 1) {
        out[k] = frsqrt(x[k]);
    } else if (FN == 2) {
        out[k] = fexp(x[k]);
    } else if (FN == 3) {
        const TransConsts tc = trans_consts();
        out[k] = fexp(x[k], tc);
    } else if (FN == 4) {
        const TransConsts tc = trans_consts_v();
        out[k] = fexp(x[k], tc);
    } else if (FN == 5) {
        double s, c;
        fsincos(x[k], s, c);
        out[2 * k] = s, out[2 * k + 1] = c;
    } else if (FN == 6) {
        const TransConsts tc = trans_consts();
        double s, c;
        fsincos(x[k], s, c, tc);
        out[2 * k] = s, out[2 * k + 1] = c;
    } else if (FN == 7) {
        const TransConsts tc = trans_consts_v();
        double s, c;
        fsincos(x[k], s, c, tc);
        out[2 * k] = s, out[2 * k + 1] = c;
    } else {
        const cd r = rcp(mk(x[2 * k], x[2 * k + 1]));
        out[2 * k] = r.x, out[2 * k + 1] = r.y;
    }
}

// ---- the pointwise integrand in its four formulations ------------------------------------------------
// Per item: pair (i, j), moment m, abscissa x, omega.  The pair constants are make_pair_const on the context's
// tables, as in every fill kernel; the contour sense is that of the item's omega.
template <int FORM>
__global__ void k_integrand_probe(IntegrandProbe A) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    const int N = A.P.N;
    const double* eta = A.tab;
    const double* gtab = A.tab + N;
    const double* btab = A.tab + 2 * N;
    const int i = A.i[k], j = A.j[k], m = A.m[k];
    const double x = A.x[k];
    const PairConst pc = make_pair_const(A.P, eta[i], eta[j], btab[i], btab[j], gtab[i] - gtab[j]);
    OmegaConst oc;
    oc.omega = mk(A.omega[2 * k], A.omega[2 * k + 1]);
    oc.omi = -copysign(1.0, oc.omega.x);
    double* o = A.out + (size_t)integrand_probe_doubles(FORM) * k;
    if (FORM == 0) {
        const cd f = integrand(x, A.P, pc, oc, m);
        o[0] = f.x, o[1] = f.y;
    } else if (FORM == 1) {
        cd fd;
        const cd f = integrand_d(x, A.P, pc, oc, m, fd);
        o[0] = f.x, o[1] = f.y, o[2] = fd.x, o[3] = fd.y;
    } else if (FORM == 2) {
        const TransConsts tc = trans_consts();
        const NodeData d = node_data(x, A.P, pc, oc.omi, m);
        const cd f = node_eval(d, oc.omega, tc);
        o[0] = d.A0.x, o[1] = d.A0.y, o[2] = d.T.x, o[3] = d.T.y;
        o[4] = d.Q1.x, o[5] = d.Q1.y, o[6] = d.Q0.x, o[7] = d.Q0.y;
        o[8] = f.x, o[9] = f.y;
    } else {
        const cd w = node_w(x, A.P, oc.omi);
        o[0] = w.x, o[1] = w.y;
    }
}

}  // namespace

hipError_t launch_bessel_probe(const double* z, int n, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_bessel_probe, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, (const double2*)z, n,
                       (double2*)out);
    return hipGetLastError();
}

hipError_t launch_elementary_probe(int fn, const double* x, int n, double* out, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    switch (fn) {
#define EMME_PROBE_CASE(F) \
    case F: hipLaunchKernelGGL((k_elementary_probe<F>), grid, block, 0, stream, x, n, out); break;
        EMME_PROBE_CASE(0)
        EMME_PROBE_CASE(1)
        EMME_PROBE_CASE(2)
        EMME_PROBE_CASE(3)
        EMME_PROBE_CASE(4)
        EMME_PROBE_CASE(5)
        EMME_PROBE_CASE(6)
        EMME_PROBE_CASE(7)
        EMME_PROBE_CASE(8)
#undef EMME_PROBE_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_integrand_probe(const IntegrandProbe& A, hipStream_t stream) {
    const dim3 grid((unsigned)((A.n + 63) / 64)), block(64);
    switch (A.form) {
        case 0: hipLaunchKernelGGL((k_integrand_probe<0>), grid, block, 0, stream, A); break;
        case 1: hipLaunchKernelGGL((k_integrand_probe<1>), grid, block, 0, stream, A); break;
        case 2: hipLaunchKernelGGL((k_integrand_probe<2>), grid, block, 0, stream, A); break;
        case 3: hipLaunchKernelGGL((k_integrand_probe<3>), grid, block, 0, stream, A); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace emme

// ---- the entry points (include/emme_hip.h): no context, buffers of the call's own, the default stream ---------------
using namespace emme;

extern "C" {

int emme_bessel_batch(const double* z, int n, double* out) {
    if (!z || !out || n < 1) return EMME_EINVAL;
    EMME_TRY(require_device());
    DeviceBuffer<double> dz, dout;
    HIP_TRY(dz.grow(sizeof(double) * 2 * n));
    HIP_TRY(dout.grow(sizeof(double) * 8 * n));
    HIP_TRY(hipMemcpy(dz, z, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    HIP_TRY(launch_bessel_probe(dz, n, dout, nullptr));
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * 8 * n, hipMemcpyDeviceToHost));
    return EMME_OK;
}

int emme_elementary_batch(int fn, const double* x, int n, double* out) {
    if (!x || !out || n < 1 || fn < 0 || fn > EMME_FN_CRCP) return EMME_EINVAL;
    EMME_TRY(require_device());
    const size_t n_in = fn == EMME_FN_CRCP ? 2 : 1;
    const size_t n_out = fn >= EMME_FN_SINCOS ? 2 : 1;
    DeviceBuffer<double> dx, dout;
    HIP_TRY(dx.grow(sizeof(double) * n_in * n));
    HIP_TRY(dout.grow(sizeof(double) * n_out * n));
    HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n_in * n, hipMemcpyHostToDevice));
    HIP_TRY(launch_elementary_probe(fn, dx, n, dout, nullptr));
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * n_out * n, hipMemcpyDeviceToHost));
    return EMME_OK;
}

int emme_integrand_batch(const emme_params_t* p, int form, int n, const int* i, const int* j, const int* m,
                         const double* x, const double* omega, double* out) {
    if (!p || !i || !j || !m || !x || !omega || !out || n < 1 || form < 0 || form > EMME_FORM_W) return EMME_EINVAL;
    EMME_TRY(check_npoints(p));
    // the scalars DevParams divides by: a zero or non-finite one would put inf / NaN into every item
    for (const double v : {p->arc_coeff, p->vt, p->tau, p->q, p->R, p->omega_s_i}) {
        if (!std::isfinite(v) || v == 0.0) {
            set_error("emme_integrand_batch: arc_coeff, vt, tau, q, R and omega_s_i must be finite and non-zero");
            return EMME_EINVAL;
        }
    }
    const int nm = std::fpclassify(p->beta_e) == FP_ZERO ? 1 : 3;
    for (int k = 0; k < n; ++k) {
        const bool pair_ok = i[k] >= 0 && i[k] < j[k] && j[k] < p->npoints;
        const bool x_ok = x[k] > 0.0 && x[k] < M_PI / 2;  // (false for NaN)
        if (!pair_ok || m[k] < 0 || m[k] >= nm || !x_ok) {
            set_error("emme_integrand_batch: item " + std::to_string(k) +
                      " needs 0 <= i < j < npoints, a moment of the context (0, or 0..2 with beta_e != 0) and x in (0, pi/2)");
            return EMME_EINVAL;
        }
    }
    EMME_TRY(require_device());
    IntegrandProbe A;
    std::vector<double> tab;
    dev_params_from(p, A.P, tab);
    A.form = form, A.n = n;
    const size_t per = (size_t)integrand_probe_doubles(form);
    DeviceBuffer<double> dtab, dx, dw, dout;
    DeviceBuffer<int> dijm;
    HIP_TRY(dtab.grow(sizeof(double) * tab.size()));
    HIP_TRY(dx.grow(sizeof(double) * n));
    HIP_TRY(dw.grow(sizeof(double) * 2 * n));
    HIP_TRY(dout.grow(sizeof(double) * per * n));
    HIP_TRY(dijm.grow(sizeof(int) * 3 * (size_t)n));
    HIP_TRY(hipMemcpy(dtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dw, omega, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    int* d_ijm = dijm;
    HIP_TRY(hipMemcpy(d_ijm, i, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ijm + n, j, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ijm + 2 * (size_t)n, m, sizeof(int) * n, hipMemcpyHostToDevice));
    A.tab = dtab, A.i = d_ijm, A.j = d_ijm + n, A.m = d_ijm + 2 * (size_t)n;
    A.x = dx, A.omega = dw, A.out = dout;
    HIP_TRY(launch_integrand_probe(A, nullptr));
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * per * n, hipMemcpyDeviceToHost));
    return EMME_OK;
}

}  // extern "C"
