// assemble_sets_list_text.hpp -- the ONE text of the kernels that finish, from scratch, the integrals the tile fill over
// parameter sets handed over (k_assemble_tile_sets, k_assemble_tile_sets_deriv: a split that does not fit the 64-entry
// level list, a poisoned (pair, interval)), and their shape forms k_assemble_tile_shape_sets<PTS, NM>,
// k_assemble_tile_shape_sets_deriv<PTS, NM>.  The form of the two readings of
// assemble_deriv_list_text.hpp: a lane group per work-list entry (batch << 32 | item), lane = node, the depth-first
// walk with the accept / split rule spelled out.  Two selectors, four readings:
//
//   SHAPE DERIV  read by                              yields
//     0     0    assemble_sets_list.hip               SetsListArgs, k_assemble_sets_list, launch_assemble_sets_list
//     0     1    assemble_sets_list_deriv.hip         SetsDerivListArgs, k_assemble_sets_deriv_list,
//                                                     launch_assemble_sets_deriv_list
//     1     0    assemble_sets_list_shape.hip         SetsListShapeArgs, k_assemble_sets_list_shape<PTS>,
//                                                     launch_assemble_sets_list_shape
//     1     1    assemble_sets_list_shape_deriv.hip   SetsDerivListShapeArgs, k_assemble_sets_deriv_list_shape<PTS>,
//                                                     launch_assemble_sets_deriv_list_shape
//
// EMME_SETS_LIST_DERIV 0: `integrand` per lane, M of the integral; 1: `integrand_d` per lane, M and M'.
// EMME_SETS_LIST_SHAPE 0: electrostatic GK15 only, k_assemble_deriv_list's form -- no template, a lane group of 16,
// __launch_bounds__(256, 3), item = pair, moment 0, no kappa_e (it is zero there), plain stores of the one block.
// EMME_SETS_LIST_SHAPE 1: electromagnetic and GK31 contexts, k_assemble_deriv_list_shape<PTS>'s form -- a lane group of
// 16 (GK15) or 32 (GK31), bounds (256, 2), item = pair nm + moment, kappa_e and (derivative) kappa_e', all three moments
// scattered as k_assemble_deriv does, through store_entry_twin or the same stores on M alone.
//
// The one-set list kernels take one DevParams per launch and stage one table per workgroup.  Here the work list has one
// SEGMENT and one counter per parameter set -- the tile kernel appends to the segment of its chunk's set -- and
// blockIdx.y is the set: a workgroup serves entries of ONE set, reads that set's scalars once, by value, before its
// first store (scalar loads: assemble_nodes_text.hpp) and stages that set's tables.  A workgroup without a share of its
// set's segment -- every workgroup of a set that handed nothing over -- returns before it stages anything.
//
// Whole translation units (includes, namespace, argument struct, kernel, launcher), as the sets readings of
// assemble_nodes_text.hpp.  No include guard: a text, not a header of declarations.
#if !defined(EMME_SETS_LIST_DERIV) || !defined(EMME_SETS_LIST_SHAPE)
#error "assemble_sets_list_text.hpp is read by the four assemble_sets_list*.hip units only, with EMME_SETS_LIST_SHAPE and EMME_SETS_LIST_DERIV set"
#endif
#include <hip/hip_runtime.h>

#include "assemble_common.hpp"
#include "launch.hpp"
#include "launch_grid.hpp"

namespace emme {

namespace {

#if EMME_SETS_LIST_SHAPE && EMME_SETS_LIST_DERIV
struct SetsDerivListShapeArgs {
#elif EMME_SETS_LIST_SHAPE
struct SetsListShapeArgs {
#elif EMME_SETS_LIST_DERIV
struct SetsDerivListArgs {
#else
struct SetsListArgs {
#endif
    const DevParams* sets;  // [nsets]: the scalars of every bound parameter set
    const double* tabs;     // [nsets][3N]: eta | g | b of every set
    const ushort2* pairs;
    const double2* omega;
    double2* M;
#if EMME_SETS_LIST_DERIV
    double2* Md;
#endif
    unsigned long long* intervals;
    int* status;
    const unsigned long long* worklist;  // the segments, one behind the other
    const int* seg;                      // [nsets]: where the segment of every set begins
    const unsigned int* counts;          // [nsets]: entries in every segment
    int skip_lost;
};

#if EMME_SETS_LIST_SHAPE
template <int PTS>
#if EMME_SETS_LIST_DERIV
__global__ __launch_bounds__(256, 2) void k_assemble_sets_deriv_list_shape(SetsDerivListShapeArgs A) {
#else
__global__ __launch_bounds__(256, 2) void k_assemble_sets_list_shape(SetsListShapeArgs A) {
#endif
    constexpr int GW = PTS == 15 ? 16 : 32, GROUPS_PER_BLOCK = 256 / GW, MAXD = EMME_MAX_DEPTH;
#else
#if EMME_SETS_LIST_DERIV
__global__ __launch_bounds__(256, 3) void k_assemble_sets_deriv_list(SetsDerivListArgs A) {
#else
__global__ __launch_bounds__(256, 3) void k_assemble_sets_list(SetsListArgs A) {
#endif
    constexpr int PTS = 15, GW = 16, GROUPS_PER_BLOCK = 256 / GW, MAXD = EMME_MAX_DEPTH;
#endif
    extern __shared__ double lds_tab[];  // eta | g | b (3N doubles) | per-group (mid, r) stack

    const int s = blockIdx.y;  // uniform per workgroup
    const int nitems = (int)A.counts[s];
    if ((int)(blockIdx.x * GROUPS_PER_BLOCK) >= nitems) return;  // (block-uniform: no tables for an empty share)
    const DevParams P = A.sets[s];  // by value, before the first store: scalar loads (see the header)
#if EMME_SETS_LIST_SHAPE
    const int N = P.N, dim = P.dim, nm = P.nm;
#else
    const int N = P.N, dim = P.dim;
#endif
    const double* tab = A.tabs + (size_t)s * 3 * N;
    const unsigned long long* worklist = A.worklist + A.seg[s];
    for (int k = threadIdx.x; k < 3 * N; k += blockDim.x) lds_tab[k] = tab[k];
    __syncthreads();
    const double* eta = lds_tab;
    const double* gtab = lds_tab + N;
    const double* btab = lds_tab + 2 * N;
    double2* stk = reinterpret_cast<double2*>(lds_tab + 3 * N + (3 * N & 1)) + (threadIdx.x / GW) * MAXD;

    const int lane_in_group = threadIdx.x % GW;
    const int group = blockIdx.x * GROUPS_PER_BLOCK + threadIdx.x / GW;
    const int ngroups = gridDim.x * GROUPS_PER_BLOCK;
    const GkLane gk = gk_lane<PTS>(lane_in_group);
    const double qa = 0.0, qb = M_PI / 2.0;
    const double inv_scale = 2. / (qb - qa);
    const cd zero = mk(0.0, 0.0);

    for (int item = group; item < nitems; item += ngroups) {
        const unsigned long long e = worklist[item];
#if EMME_SETS_LIST_SHAPE
        const int it = (int)(e & 0xffffffffull), b = (int)(e >> 32);
        if (A.skip_lost && A.status[b] != 0) continue;  // (the matrix is lost already: uniform per group)
        const int p = it / nm, m = it - p * nm;
#else
        const int p = (int)(e & 0xffffffffull), b = (int)(e >> 32);
        if (A.skip_lost && A.status[b] != 0) continue;  // (the matrix is lost already: uniform per group)
        constexpr int m = 0;
#endif
        OmegaConst oc;
        oc.omega = mk(A.omega[b].x, A.omega[b].y);
        oc.omi = -copysign(1.0, oc.omega.x);
        const ushort2 ij = A.pairs[p];
        const int i = ij.x, j = ij.y;
#if EMME_SETS_LIST_SHAPE
        const double dg = gtab[i] - gtab[j];
        const PairConst pc = make_pair_const(P, eta[i], eta[j], btab[i], btab[j], dg);
#else  // (no named dg here, as in assemble_deriv_list_text.hpp)
        const PairConst pc = make_pair_const(P, eta[i], eta[j], btab[i], btab[j], gtab[i] - gtab[j]);
#endif
        int depth = 0, item_intervals = 0, bad = 0;
        unsigned long long path = 0;
        double l = qa, r = qb, abs_tol = 0.0;
        cd sum = zero;
#if EMME_SETS_LIST_DERIV
        cd sum_d = zero;
#endif
        for (;;) {
            const double mid = (r + l) / 2;
            const double scale = (r - l) / 2;
            const double x = __dadd_rn(__dmul_rn(scale, gk.x), mid);
#if EMME_SETS_LIST_DERIV
            cd fd;
            const cd f = integrand_d(x, P, pc, oc, m, fd);
#else
            const cd f = integrand(x, P, pc, oc, m);
#endif
            const double Kx = group_sum<GW>(gk.wk * f.x), Ky = group_sum<GW>(gk.wk * f.y);
            const double Gx = group_sum<GW>(gk.wg * f.x), Gy = group_sum<GW>(gk.wg * f.y);
#if EMME_SETS_LIST_DERIV
            const double Kdx = group_sum<GW>(gk.wk * fd.x), Kdy = group_sum<GW>(gk.wk * fd.y);
#endif
            ++item_intervals;
            // (gk_split of assemble_common.hpp, spelled out as in assemble_deriv_list_text.hpp)
            const double dKx = Kx - Gx, dKy = Ky - Gy;
            const double absK = gk_modulus(Kx, Ky);
            double err = fmax(gk_modulus(dKx, dKy), absK * (2.0 * 2.220446049250313e-16));
            const cd integral = mk(Kx * scale, Ky * scale);
            err *= scale;
            const double rel_abs = P.rel_tol * (absK * scale);
            if (abs_tol == 0.0) abs_tol = rel_abs;
            bool split = depth < P.max_sub && err > abs_tol * inv_scale + P.prec_goal && err > rel_abs + P.prec_goal;
            if (split && (depth >= MAXD || item_intervals >= EMME_MAX_INTERVALS)) {
                split = false;
                bad = 1;
            }
            if (split) {
                stk[depth] = make_double2(mid, r);
                r = mid;
                ++depth;
                path <<= 1;
                continue;
            }
            sum = sum + integral;
#if EMME_SETS_LIST_DERIV
            sum_d = sum_d + mk(Kdx * scale, Kdy * scale);
#endif
            ++path;
            while (depth > 0 && !(path & 1)) {
                path >>= 1;
                --depth;
            }
            if (depth == 0) break;
            const double2 pr = stk[depth - 1];
            l = pr.x;
            r = pr.y;
        }
#if EMME_SETS_LIST_SHAPE
        cd kap = mk(P.pref * sum.y, -(P.pref * sum.x));
#if EMME_SETS_LIST_DERIV
        cd kd = mk(P.pref * sum_d.y, -(P.pref * sum_d.x));
        if (kappa_bad(kap) || kappa_bad(kd)) bad = 1;
        kd = kd + kappa_e_d(m, P, pc.de, dg, oc.omega);  // kappa' = -i pref sum' + kappa_e'
#else
        if (kappa_bad(kap)) bad = 1;
#endif
        kap = kap + kappa_e(m, P, pc.de, dg, oc.omega);
        if (lane_in_group == 0) {
            // blocks A (m = 0), B and its mirrors (m = 1), D (m = 2), as k_assemble_deriv_list_shape scatters them
            double2* Mb = A.M + (size_t)b * dim * dim;
#if EMME_SETS_LIST_DERIV
            double2* Mdb = A.Md + (size_t)b * dim * dim;
            auto store = [&](int rw, int c, cd v, cd vd) { store_entry_twin(Mb, Mdb, (size_t)rw * dim + c, v, vd); };
            const cd kx = kd;
#else
            auto store = [&](int rw, int c, cd v, cd) { Mb[(size_t)rw * dim + c] = make_double2(v.x, v.y); };
            const cd kx = zero;
#endif
            if (m == 0) {
                const double w = -(pair_weight(i, j, N) * P.dx);
                const cd v = w * kap, vd = w * kx;
                store(i, j, v, vd);
                store(j, i, v, vd);
            } else if (m == 1) {
                const cd v = P.dx * kap, vd = P.dx * kx;
                store(i, j + N, v, vd);
                store(j, i + N, -v, -vd);
                store(i + N, j, -v, -vd);
                store(j + N, i, v, vd);
            } else {
                const cd v = P.dx * kap, vd = P.dx * kx;
                store(i + N, j + N, v, vd);
                store(j + N, i + N, v, vd);
            }
#else
        const cd kap = mk(P.pref * sum.y, -(P.pref * sum.x));
#if EMME_SETS_LIST_DERIV
        const cd kd = mk(P.pref * sum_d.y, -(P.pref * sum_d.x));
        if (kappa_bad(kap) || kappa_bad(kd)) bad = 1;
#else
        if (kappa_bad(kap)) bad = 1;
#endif
        if (lane_in_group == 0) {
            const double w = pair_entry_weight(i, j, N, P.dx);
            const cd v = w * kap;
            double2* Mb = A.M + (size_t)b * dim * dim;
            Mb[(size_t)i * dim + j] = make_double2(v.x, v.y);
            Mb[(size_t)j * dim + i] = make_double2(v.x, v.y);
#if EMME_SETS_LIST_DERIV
            const cd vd = w * kd;
            double2* Mdb = A.Md + (size_t)b * dim * dim;
            Mdb[(size_t)i * dim + j] = make_double2(vd.x, vd.y);
            Mdb[(size_t)j * dim + i] = make_double2(vd.x, vd.y);
#endif
#endif
            if (A.intervals) atomicAdd(&A.intervals[b], (unsigned long long)item_intervals);
            if (bad) A.status[b] = 1;
        }
    }
}

}  // namespace

// L describes the batch (L.P: the context's own set, read for the shape only; L.tab is not read); sets / tabs / seg /
// counts are device arrays of nsets entries (see the argument struct).  The segments' lengths are on the device: a
// fixed grid per set strides over its segment, and workgroups without a share return at once.
#if EMME_SETS_LIST_SHAPE && EMME_SETS_LIST_DERIV
hipError_t launch_assemble_sets_deriv_list_shape(const AssembleLaunch& L, const DevParams* sets, const double* tabs,
                                                 int nsets, const unsigned long long* worklist, const int* seg,
                                                 const unsigned int* counts, hipStream_t stream) {
    const bool es15 = L.gk_points == 15 && L.P.dim == L.P.N;
    if ((L.gk_points != 15 && L.gk_points != 31) || es15 || !L.Md) return hipErrorInvalidValue;
    SetsDerivListShapeArgs A;
    A.Md = (double2*)L.Md;
#elif EMME_SETS_LIST_SHAPE
hipError_t launch_assemble_sets_list_shape(const AssembleLaunch& L, const DevParams* sets, const double* tabs, int nsets,
                                           const unsigned long long* worklist, const int* seg,
                                           const unsigned int* counts, hipStream_t stream) {
    const bool es15 = L.gk_points == 15 && L.P.dim == L.P.N;
    if ((L.gk_points != 15 && L.gk_points != 31) || es15 || L.Md) return hipErrorNotSupported;
    SetsListShapeArgs A;
#elif EMME_SETS_LIST_DERIV
hipError_t launch_assemble_sets_deriv_list(const AssembleLaunch& L, const DevParams* sets, const double* tabs, int nsets,
                                           const unsigned long long* worklist, const int* seg, const unsigned int* counts,
                                           hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || !L.Md) return hipErrorInvalidValue;
    SetsDerivListArgs A;
    A.Md = (double2*)L.Md;
#else
hipError_t launch_assemble_sets_list(const AssembleLaunch& L, const DevParams* sets, const double* tabs, int nsets,
                                     const unsigned long long* worklist, const int* seg, const unsigned int* counts,
                                     hipStream_t stream) {
    if (L.gk_points != 15 || L.P.dim != L.P.N || L.Md) return hipErrorNotSupported;
    SetsListArgs A;
#endif
    if (!sets || !tabs || !worklist || !seg || !counts || nsets < 1 || nsets > 65535) return hipErrorInvalidValue;
    A.sets = sets;
    A.tabs = tabs;
    A.pairs = (const ushort2*)L.pairs;
    A.omega = (const double2*)L.omega;
    A.M = (double2*)L.M;
    A.intervals = L.intervals;
    A.status = L.status;
    A.worklist = worklist;
    A.seg = seg;
    A.counts = counts;
    A.skip_lost = L.skip_lost;
#if EMME_SETS_LIST_SHAPE
    const size_t lds = tables_stack_lds_bytes(L.P.N, L.gk_points == 15 ? 16 : 8);
#else
    const size_t lds = tables_stack_lds_bytes(L.P.N, 16);
#endif
    const dim3 grid(256, (unsigned)nsets);
#if EMME_SETS_LIST_SHAPE && EMME_SETS_LIST_DERIV
    if (L.gk_points == 15)
        hipLaunchKernelGGL(k_assemble_sets_deriv_list_shape<15>, grid, dim3(256), lds, stream, A);
    else
        hipLaunchKernelGGL(k_assemble_sets_deriv_list_shape<31>, grid, dim3(256), lds, stream, A);
#elif EMME_SETS_LIST_SHAPE
    if (L.gk_points == 15)
        hipLaunchKernelGGL(k_assemble_sets_list_shape<15>, grid, dim3(256), lds, stream, A);
    else
        hipLaunchKernelGGL(k_assemble_sets_list_shape<31>, grid, dim3(256), lds, stream, A);
#elif EMME_SETS_LIST_DERIV
    hipLaunchKernelGGL(k_assemble_sets_deriv_list, grid, dim3(256), lds, stream, A);
#else
    hipLaunchKernelGGL(k_assemble_sets_list, grid, dim3(256), lds, stream, A);
#endif
    return hipGetLastError();
}

}  // namespace emme
